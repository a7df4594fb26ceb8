"""The dense chain (csrc/scan_dense.inc) run on the CPU: tools/scan_dense_emu.cpp compiles the fourteen kernels as they
stand, launches every case of tests/dense_cases.py as ensure_dense_tables and launch_dense do - the launch arithmetic is
the library's own (csrc/dense_launch.inc) -, keeps every buffer, the LDS block of the compare stage included, in a heap
block of exactly its size under the address and undefined-behaviour sanitizers, models the inline-assembly LDS-DMA and
its counted waits in two modes (late: a piece lands only when a wait requires it, poison until then; early: at issue),
and runs each case under the eleven schedules of tools/emu_reads.h in both modes: 22 scans per case, none cut.  Before
a scan the device tables must equal, element by element, the numpy reference written from their definitions; under every
schedule the tile counters, per-target counts, status word, hit count and hit records must be the CPU oracle's.

The controls prove that the test can fail.  They are switches of the one binary (--control=NAME), not builds - a build
takes half a minute -, except the torn or and the torn add, which share one build of tools/wave_emu.h's two flags.
The emulator is a stand-alone program; no GPU is involved."""
import os
import re
import subprocess

import pytest

import dense_cases as dc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
         "-I" + os.path.join(REPO, "include")]
SRC = os.path.join(REPO, "tools", "scan_dense_emu.cpp")
NAMES = ("n", "tiles", "T", "levels", "L", "k", "groups", "window", "uniform", "idx16", "sym", "kpad", "win_dwords", "win_bufs", "npc", "tc",
         "parts", "runs", "launches", "points", "pieces", "queued", "overflow_win", "overflow_gather", "over_regions", "packed", "hits", "orders")
LINE = re.compile(r"case (\w+) ok: " + " ".join(r"%s (-?\d+)" % name for name in NAMES) + r" kernels \[(.*?)\]")
RUNS = 22                                                  # eleven schedules in each of the two DMA modes


def _constant(name, source):
    text = open(os.path.join(REPO, "well_duplicates_amd", "csrc", source)).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dense_emu")
    exe = str(tmp / "scan_dense_emu")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    files = {}
    for case in dc.cases():
        files[case.name] = str(tmp / (case.name + ".sqc"))
        dc.write_case(files[case.name], case)
    return exe, files, tmp


def _run(exe, paths, control=None):
    out = subprocess.run([exe] + (["--control=" + control] if control else []) + paths, capture_output=True, text=True, timeout=900)
    print(out.stdout[-6000:], out.stderr[:1500])
    return out


def test_every_schedule_and_dma_mode_gives_the_oracles_counts(emu):
    exe, files, _ = emu
    assert tuple(_constant(n, "wd_shared.h" if n in ("kSigCycles", "kRowGroups") else "dense_launch.inc")
                 for n in ("kSigCycles", "kMaxSeg", "kWinMaxK", "kWinGap", "kWinDwords", "kMarkBlock", "kWinBufs", "kWinBufsSym", "kRowGroups")) == \
        dc.CONSTANTS + (dc.K_ROW_GROUPS,)
    assert dc.K_ROW_CYCLES == 40 * dc.K_ROW_GROUPS
    out = _run(exe, [files[c.name] for c in dc.cases()])
    assert out.returncode == 0 and "MISMATCH" not in out.stdout, (out.stdout[-3000:], out.stderr[-3000:])
    rows = {}
    for row in LINE.findall(out.stdout):
        rows[row[0]] = dict(zip(NAMES, (int(v) for v in row[1:-1])), kernels=set(row[-1].split("; ")))
    assert list(rows) == [c.name for c in dc.cases()] and len(out.stdout.strip().split("\n")) == len(rows)
    ran = set()
    for case in dc.cases():
        r, tb = rows[case.name], case.tables()
        ran |= r["kernels"]
        assert (r["n"], r["tiles"], r["T"], r["levels"], r["L"], r["k"]) == (case.n, len(case.tiles), case.T, case.levels, case.L, case.kk)
        assert r["runs"] == RUNS and r["points"] > 0, (case.name, r)
        assert (r["groups"], r["window"], r["uniform"], r["idx16"], r["sym"], r["kpad"], r["win_dwords"]) == \
            (tb["groups"], tb["window_groups"], tb["uniform_groups"], tb["idx16"], tb["sym_on"], tb["kpad"], tb["window_dwords"]), case.name
        assert set(case.expect) <= r["kernels"], (case.name, case.expect, r["kernels"])
        assert r["hits"] == (dc.qc.truth(case)["hits"].shape[0] if case.hit_cap > 0 else -1)
        tags = case.tags
        if "win" in tags:
            assert r["window"] > 0 and r["pieces"] > 0, (case.name, r)
        if "gatheronly" in tags:
            assert r["window"] == 0 and r["pieces"] == 0 and any(k.startswith("k_dense_pairs<") for k in r["kernels"]), (case.name, r)
        if "gather" in tags:
            assert r["pieces"] == 0 and not any(k.startswith("k_dense_pairs_win") for k in r["kernels"]), (case.name, r)
        if "unordered" in tags:                            # one group keeps the gathers, the others have windows
            assert r["window"] == r["groups"] - 1 and r["sym"] == 0, (case.name, r)
        if "straddle" in tags:
            assert r["uniform"] == 0, (case.name, r)
        if "fullunion" in tags:                            # a union of exactly kpad elements still has its windows
            assert r["window"] == r["groups"] and all(w["n_el"] == r["kpad"] for w in tb["wins"]), (case.name, r)
        if "oneended31" in tags:                           # the first group: kpad - 1 elements above its centres, their own signatures at kpad - 1
            assert r["sym"] == 1 and r["window"] >= 1 and (tb["wins"][0]["n_el"], tb["wins"][0]["n"]) == (r["kpad"] - 1, r["kpad"]), (case.name, r)
        if "oneended32" in tags:                           # ... and kpad of them: the group keeps the gathers
            assert r["sym"] == 1 and tb["wins"][0] is None and any(k.startswith("k_dense_pairs<") for k in r["kernels"]), (case.name, r)
        if "symint32" in tags:
            assert (r["sym"], r["idx16"]) == (1, 0), (case.name, r)
        if "twoended" in tags:
            assert r["sym"] == 0, (case.name, r)
        if "bufs3" in tags:
            assert (r["win_bufs"], r["npc"], r["tc"]) == (3, 0, 5), (case.name, r)
        if "bufs2" in tags:
            assert (r["win_bufs"], r["npc"], r["sym"]) == (2, 0, 1), (case.name, r)
        if "int32" in tags:
            assert r["idx16"] == 0 and "k_transpose_nbr<int32_t>" in r["kernels"], (case.name, r)
        if "int16edge" in tags:
            assert r["idx16"] == 1, (case.name, r)
        if "overflow" in tags:
            assert r["overflow_win"] + r["overflow_gather"] >= RUNS, (case.name, r)
        if "levover" in tags:                              # Levenshtein leaves the group to k_dense_verify
            assert r["over_regions"] >= RUNS and r["packed"] == RUNS, (case.name, r)
        if "exact" in tags:                                # group 0: n_q == q_per, queued; group 1: q_per + 1, finished in place
            assert (r["queued"], r["overflow_win"], r["over_regions"]) == (3 * RUNS, RUNS, 0), (case.name, r)
        if "allmarked" in tags:
            assert r["packed"] == RUNS and r["overflow_win"] == 0 and r["queued"] == RUNS * case.n // 2, (case.name, r)
        if "parts" in tags:
            assert r["parts"] == 3 and r["packed"] == 3 * RUNS, (case.name, r)
        if "hitcap" in tags:                               # a log smaller than the hits: the schedules keep different records
            assert 0 < case.hit_cap < r["hits"] and r["orders"] >= 2, (case.name, r)
        if case.options["dense_pack"] == 0 and case.fam == "ham":
            assert r["packed"] == 0, (case.name, r)
    # the instantiations the host can launch that ran
    want = {"k_transpose_off", "k_transpose_nbr<int16_t>", "k_transpose_nbr<int32_t>", "k_dense_symcheck", "k_dense_windows", "k_dense_counts",
            "k_dense_mark", "k_dense_rank_words", "k_dense_rank_blocks", "k_dense_reduce", "k_dense_verify<true>", "k_dense_verify<false>",
            "k_dense_sig<true, true>", "k_dense_sig<true, false>", "k_dense_sig<false, true>", "k_dense_sig<false, false>",
            "k_dense_pack<4, true, true>", "k_dense_pack<4, true>", "k_dense_pack<4, false>", "k_dense_pack<1, true>", "k_dense_pack<1, false>"}
    for m in (0, 1, 2):
        want |= {"k_dense_pairs_win<%d, true, 0>" % m, "k_dense_pairs_win<%d, false, 0>" % m, "k_dense_pairs<%d, true, true>" % m,
                 "k_dense_pairs<%d, true, false>" % m}
    for m in (0, 1, 2):
        want |= {"k_dense_pairs_win<%d, true, %d>" % (m, npc) for npc in (4, 5, 6, 8)}
        want |= {"k_dense_pairs<%d, false, false>" % m, "k_dense_pairs<%d, false, true>" % m}
    assert want <= ran, sorted(want - ran)


def _mismatches(out):
    """{case: {kind}} and {case: {dma mode}} of a control's output"""
    kinds, modes = {}, {}
    for name, kind in re.findall(r"MISMATCH case (\w+) schedule \d+ \(\w+\): ([A-Za-z_ -]+?)(?: \(| \d+:)", out.stdout):
        kinds.setdefault(name, set()).add(kind)
    for name, mode in re.findall(r"MISMATCH case (\w+) under dma (\w+)", out.stdout):
        modes.setdefault(name, set()).add(mode)
    return kinds, modes


def test_an_issue_one_window_early_is_noticed_under_early_landing(emu):
    """The one-ended kernel asks for tile ti + ahead_max one window early: into the window tile ti is about to be compared
    in.  Every case whose waves walk more tiles than they have windows in flight must end in MISMATCH in the early mode,
    where the piece lands at issue and the tile is compared with another tile's signatures.  (The late mode sees it too,
    by the poison that stands in a piece's destination from its issue to its landing: recorded, and asserted.)"""
    exe, files, _ = emu
    sel = [c for c in dc.cases() if c.tables()["sym_on"] and c.options["dense_windows"] and c.tables()["window_groups"] and
           min(len(c.tiles), c.options["dense_tile_chunk"]) >= 3 and not c.options["dense_overlap"]]
    assert len(sel) >= 8 and {"bufs3", "pipe"} <= set().union(*(c.tags for c in sel))
    out = _run(exe, [files[c.name] for c in sel], "early_issue")
    assert out.returncode == 1
    kinds, modes = _mismatches(out)
    for c in sel:
        assert "early" in modes.get(c.name, set()), (c.name, modes.get(c.name), kinds.get(c.name))
        assert "late" in modes.get(c.name, set()), (c.name, modes.get(c.name), kinds.get(c.name))
    # a case whose waves walk fewer tiles than that never issues early: the control changes nothing there
    few = [c for c in dc.cases() if "pipe" in c.tags and min(len(c.tiles), c.options["dense_tile_chunk"]) <= 2]
    out = _run(exe, [files[c.name] for c in few], "early_issue")
    assert few and out.returncode == 0 and "MISMATCH" not in out.stdout


def test_a_lenient_wait_is_noticed_under_late_landing_only(emu):
    """Every wait one piece too lenient: every case with LDS windows must end in MISMATCH in the late mode - the last piece
    of a tile's window is still poison when the tile is compared - and in the early mode, where a piece lands at issue,
    in none."""
    exe, files, _ = emu
    sel = [c for c in dc.cases() if c.tags & {"pipe", "bufs3", "bufs2", "twoended"} and c.tables()["window_groups"] and c.options["dense_windows"] and
           not c.options["dense_overlap"]]
    assert len(sel) >= 8
    out = _run(exe, [files[c.name] for c in sel], "lenient_wait")
    assert out.returncode == 1
    kinds, modes = _mismatches(out)
    for c in sel:
        assert modes.get(c.name) == {"late"}, (c.name, modes.get(c.name), kinds.get(c.name))


@pytest.fixture(scope="module")
def torn(emu):
    exe = str(emu[2] / "scan_dense_emu_torn")
    subprocess.check_call(["g++"] + FLAGS + ["-DWAVE_EMU_TORN_OR", "-DWAVE_EMU_TORN_ADD", SRC, "-o", exe])
    return exe


def test_a_torn_or_is_noticed(emu, torn):
    """An or that another fiber may cut in two: a transition of a target's hit mask is applied twice.  Every equal-reads
    case - every pair a duplicate, a target's mask set from many lanes - must end in MISMATCH in the Hit / first / last
    counters (out_tile)."""
    sel = [c for c in dc.cases() if "equal" in c.tags]
    out = _run(torn, [emu[1][c.name] for c in sel], "torn_or")
    assert out.returncode == 1
    kinds, _ = _mismatches(out)
    for c in sel:
        assert "out_tile" in kinds.get(c.name, set()), (c.name, kinds.get(c.name))


def test_a_torn_add_is_noticed(emu, torn):
    """An add that another fiber may cut in two: MISMATCH in the tallies (out_tile, out_per_target) or the hit records of
    every equal-reads case, and both kinds among them."""
    sel = [c for c in dc.cases() if "equal" in c.tags]
    out = _run(torn, [emu[1][c.name] for c in sel], "torn_add")
    assert out.returncode == 1
    kinds, _ = _mismatches(out)
    seen = set()
    for c in sel:
        got = kinds.get(c.name, set()) & {"out_tile", "out_per_target", "hit record", "hit_count"}
        assert got, (c.name, kinds.get(c.name))
        seen |= got
    assert seen & {"out_tile", "out_per_target"} and seen & {"hit record", "hit_count"}, seen


def _sanitizer_report(emu, control, select):
    exe, files, _ = emu
    sel = [c for c in dc.cases() if select(c)]
    assert sel
    for c in sel:
        out = _run(exe, [files[c.name]], control)
        assert out.returncode != 0 and "AddressSanitizer: heap-buffer-overflow" in out.stderr and " ok:" not in out.stdout, \
            (c.name, out.returncode, out.stdout[-2000:], out.stderr[-2000:])


def test_a_short_lds_block_is_a_sanitizer_report(emu):
    """The LDS block of the compare stage without the last wave's last queue: where a workgroup's fourth wave has a
    window group, its survivor counts lie behind the block."""
    _sanitizer_report(emu, "short_lds", lambda c: c.tags & {"grid", "bufs2", "bufs3"})


def test_a_short_nbr_t_is_a_sanitizer_report(emu):
    _sanitizer_report(emu, "short_nbrt", lambda c: c.tags & {"int32", "int16edge", "tail"})


def test_short_rows_are_a_sanitizer_report(emu):
    """rows one row short: the case that marks every well of its last tile writes the last row."""
    _sanitizer_report(emu, "short_rows", lambda c: "allmarked" in c.tags)


def test_a_scratch_word_left_out_of_the_clear_is_noticed(emu):
    """The first counter slot and the first mask word of every part dirty again after dense_clear_scratch: MISMATCH in
    the tile counters of the cases that run parts on dirty, reused scratch sets."""
    exe, files, _ = emu
    sel = [c for c in dc.cases() if "dirty" in c.tags]
    out = _run(exe, [files[c.name] for c in sel], "skip_clear")
    assert out.returncode == 1
    kinds, _ = _mismatches(out)
    for c in sel:
        assert "out_tile" in kinds.get(c.name, set()), (c.name, kinds.get(c.name))
