"""k_scan_lines (csrc/scan_lines.inc) run on the CPU under shuffled schedules, on the tables of the library's own
make_line_tables (csrc/line_tables.inc): tools/scan_lines_emu.cpp compiles both as they stand and launches every case of
tests/linewalk_cases.py as launch_lines_t does - the tables checked first, element by element, against the numpy
reference and against their definition; the grid of blocks x tiles walked through the kernel's own XCD mapping; the LDS
bytes of the host's own scan_lines_lds_dwords; the argument block behind late_arg sizeof(LineArgs) bytes.  Every case
runs under all eleven schedules (none was cut), the workgroups permuted in all but the first - so that the blocks of a
split target apply their transitions of its hit-level byte in orders no GPU run was ever asked for.  Every buffer is a
heap allocation of exactly its size and the program is built with the address and undefined-behaviour sanitizers.  Under
each schedule the tile counters, the per-target counts, the status word, the hit count, the hit records and every byte
of the hit-level masks must be the CPU oracle's.  First of all the emulator runs lw_wave_sum alone (DPP by the ISA's
account of it, tools/wave_emu.h).

Five control builds prove that the test can fail: a torn add, a torn or (the masks four targets share a word of), an LDS
block without the last wave's second queue buffer, pw and pm one entry short, mask one word short.  The emulator is a
stand-alone program; no GPU is involved, and the emulation is sequentially consistent and says nothing about caches,
time or the memory model.

CPU time, measured in one run of the suite where this was written: the main test here 46 s (22 s of them the build, 27 s
the emulator on 201 cases), the main test of tests/test_scanq_emu.py 30 s; each control 20 to 26 s, nearly all of it its
build.  The subprocess timeout is the sibling's."""
import os
import re
import subprocess

import linewalk_cases as lc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
         "-I" + os.path.join(REPO, "include")]
SRC = os.path.join(REPO, "tools", "scan_lines_emu.cpp")
NAMES = ("n", "tiles", "T", "levels", "L", "k", "line_pairs", "blocks", "tmax", "schedules", "launches", "points", "mid_drains", "drains",
         "in_place", "finish_all", "pushes", "split", "neg_deltas", "hits", "orders")
LINE = re.compile(r"case (\w+) ok: kernel (k_scan_lines<\w+, \d, -?\d(?:, 4)?>) " + " ".join(r"%s (-?\d+)" % name for name in NAMES) +
                  r" mid_qn ([\d,]+|-)")
MISMATCH = re.compile(r"MISMATCH case (\w+) schedule \d+ \(\w+\): ([a-z_ ]+?)(?: \(| (\d+):)")


def _constant(name):
    text = open(os.path.join(REPO, "well_duplicates_amd", "csrc", "scan_lines.inc")).read()
    return re.search(r"constexpr int %s = ([^;]+);" % name, text).group(1)


def _build(tmp_path, name, *defines):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++"] + FLAGS + list(defines) + [SRC, "-o", exe])
    return exe


def _files(tmp_path, select=lambda c: True):
    paths = []
    for case in lc.cases():
        if select(case):
            paths.append(str(tmp_path / (case.name + ".sqc")))
            lc.write_case(paths[-1], case)
    return paths


def test_every_schedule_gives_the_oracles_counts(tmp_path):
    assert (_constant("kLwTargets"), _constant("kLwPairs"), _constant("kLwStep"), _constant("kLwQCap"), _constant("kLwInPlace")) == \
        (str(lc.K_LW_TARGETS), str(lc.K_LW_PAIRS), "2 * kWave", str(lc.K_LW_QCAP), str(lc.K_LW_IN_PLACE)) and lc.K_LW_STEP == 2 * 64
    exe = _build(tmp_path, "scan_lines_emu")
    out = subprocess.run([exe] + _files(tmp_path), capture_output=True, text=True, timeout=900)
    print(out.stdout)                                     # per case: the instantiation, the blocks, the queues' events, the deltas
    assert out.returncode == 0 and "MISMATCH" not in out.stdout, (out.stdout[-3000:], out.stderr[-3000:])
    lines = out.stdout.strip().split("\n")
    assert re.fullmatch(r"selftest lw_wave_sum passed: inputs (\d+)", lines[0]) and int(lines[0].split()[-1]) >= 2 + 8 + 1 + 1, lines[0]
    rows = {row[0]: dict(zip(("kernel",) + NAMES, (row[1],) + tuple(int(v) for v in row[2:-1]))) for row in LINE.findall(out.stdout)}
    mid_qn = {row[0]: {int(v) for v in row[-1].split(",")} if row[-1] != "-" else set() for row in LINE.findall(out.stdout)}
    aside = set(re.findall(r"case (\w+) ok: does not apply", out.stdout))
    assert aside == {c.name for c in lc.cases() if c.kernel is None} and len(aside) == 4
    assert list(rows) == [c.name for c in lc.cases() if c.kernel] and len(lines) == 1 + len(rows) + len(aside)
    for case in lc.cases():
        if case.kernel is None:
            continue
        r = rows[case.name]
        assert r["kernel"] == case.kernel, (case.name, r["kernel"])
        assert (r["n"], r["tiles"], r["T"], r["levels"], r["L"], r["k"], r["line_pairs"]) == \
            (case.n, len(case.tiles), case.T, case.levels, case.L, case.kk, case.line_pairs)
        assert (r["blocks"], r["tmax"], r["split"]) == (case.blocks, case.tables["tmax"], case.split_targets()), (case.name, r)
        assert r["schedules"] == 11 and r["launches"] == 11 and r["points"] > 0, (case.name, r)
        assert r["hits"] == (lc.truth(case)["hits"].shape[0] if case.hit_cap >= 0 else -1)
        # the regimes ran
        if "split" in case.tags:
            assert r["split"] > 0, (case.name, r)
        if "negdelta" in case.tags:                       # a first hit that moved down or a last hit that moved up, block after block
            assert r["neg_deltas"] > 0, (case.name, r)
        if "queue" in case.tags:                          # a drain with items still to come, under every schedule: at exactly
            assert r["mid_drains"] >= 11 and r["pushes"] > r["drains"], (case.name, r)     # kLwQCap, and at one below it
            assert {lc.K_LW_QCAP, lc.K_LW_QCAP - 1} <= mid_qn[case.name], (case.name, mid_qn[case.name])
        if "equal" in case.tags or "striped" in case.tags:
            assert r["in_place"] >= 11, (case.name, r)
        if "striped" in case.tags:                        # 42 survivors are queued, 43 finished in place
            assert r["pushes"] >= 11, (case.name, r)
        if "slot4095" in case.tags or "cut256" in case.tags:
            assert r["pushes"] >= 11 and r["in_place"] == 0, (case.name, r)      # the duplicates went through the queue
    assert len({c.kernel for c in lc.cases() if c.kernel}) == 14
    # where the log is too small, different schedules keep different records in a different order
    for case in lc.cases():
        if case.name.endswith("equal_K100"):
            assert 0 < case.hit_cap < rows[case.name]["hits"] and rows[case.name]["orders"] >= 2, (case.name, rows[case.name])


def _run_control(tmp_path, exe, select):
    files = _files(tmp_path, select)
    assert files
    out = subprocess.run([exe] + files, capture_output=True, text=True, timeout=900)
    print(out.stdout[-3000:], out.stderr[:1500])
    return out


def test_a_torn_add_is_noticed(tmp_path):
    """-DWAVE_EMU_TORN_ADD: every equal-reads case - every pair a duplicate - must end in MISMATCH on its per-target counts
    or its hit records (the tile counters, which the same build tears in the tally phase, do not count here), and both
    kinds must show among the cases."""
    exe = _build(tmp_path, "scan_lines_emu_torn_add", "-DWAVE_EMU_TORN_ADD")
    out = _run_control(tmp_path, exe, lambda c: "equal" in c.tags)
    assert out.returncode == 1, (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    failed = {}
    for name, kind, _ in MISMATCH.findall(out.stdout):
        failed.setdefault(name, set()).add(kind)
    seen = set()
    for case in lc.cases():
        if "equal" in case.tags:
            kinds = failed.get(case.name, set()) & {"out_per_target", "hit record"}
            assert kinds, (case.name, failed.get(case.name))
            seen |= kinds
    assert seen == {"out_per_target", "hit record"}, seen


def test_a_torn_or_is_noticed(tmp_path):
    """-DWAVE_EMU_TORN_OR: another lane may set bits of a mask word between an atomicOr's load and its store.  The scripted
    split targets share their word with a target that has duplicates in the same blocks: a lost bit is a transition
    applied twice or never undone, and every such case must end in MISMATCH on a Hit, first-hit or last-hit counter."""
    exe = _build(tmp_path, "scan_lines_emu_torn_or", "-DWAVE_EMU_TORN_OR")
    out = _run_control(tmp_path, exe, lambda c: "sharedword" in c.tags)
    assert out.returncode == 1, (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    at = {name: int(i) for name, kind, i in MISMATCH.findall(out.stdout) if kind == "out_tile"}
    n = 0
    for case in lc.cases():
        if "sharedword" in case.tags:
            assert case.name in at, (case.name, out.stdout[-2000:])
            i = at[case.name] % (1 + 5 * case.levels)             # the counter within its tile's row: Targets, Wells, Dups, Hit, first, last
            assert i >= 1 + 2 * case.levels, (case.name, at[case.name])
            n += 1
    assert n == 2 * len(lc.FAMILIES) * len(lc.LAYOUTS)


def _sanitizer_report(tmp_path, define, tag):
    exe = _build(tmp_path, "scan_lines_emu_" + tag, define)
    n = 0
    for case in lc.cases():
        if tag in case.tags:
            out = _run_control(tmp_path, exe, lambda c: c.name == case.name)
            assert out.returncode != 0 and "AddressSanitizer: heap-buffer-overflow" in out.stderr and " ok:" not in out.stdout, \
                (case.name, out.returncode, out.stdout[-2000:], out.stderr[-2000:])
            n += 1
    assert n >= len(lc.FAMILIES) * len(lc.LAYOUTS)


def test_a_short_lds_block_is_a_sanitizer_report(tmp_path):
    """-DSCANL_EMU_SHORT_LDS: the LDS block lacks the last wave's second queue buffer.  The case whose last wave drains
    with survivors that live through a round must end in a report of the address sanitizer."""
    _sanitizer_report(tmp_path, "-DSCANL_EMU_SHORT_LDS", "lastdrain")


def test_short_pair_tables_are_a_sanitizer_report(tmp_path):
    """-DSCANL_EMU_SHORT_PW: pw and pm are one entry short.  The cases whose last block is one pair - pw's last entry, read
    as the block's idle well and through min(r, np - 1) - must end in a report of the address sanitizer."""
    _sanitizer_report(tmp_path, "-DSCANL_EMU_SHORT_PW", "bufend")


def test_a_short_mask_is_a_sanitizer_report(tmp_path):
    """-DSCANL_EMU_SHORT_MASK: mask is one word short.  The cases whose target T - 1 (T % 4 = 1: alone in its word, the
    last of the stride) has a duplicate must end in a report of the address sanitizer."""
    _sanitizer_report(tmp_path, "-DSCANL_EMU_SHORT_MASK", "lastword")
