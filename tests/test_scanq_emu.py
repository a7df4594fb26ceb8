"""k_scan_q (csrc/scan_queue.inc) run on the CPU under shuffled schedules: tools/scan_queue_emu.cpp compiles the kernel as
it stands, plays the 256 lanes of a workgroup with fibers (tools/wave_emu.h), launches every case of
tests/scanq_cases.py as launch_queue_t / launch_queue_lev_t do - the grid walked through the kernel's own XCD mapping,
the LDS bytes of the host's own scan_q_lds_dwords - and lets the schedule hand over to another lane at every atomic:
never, always, with probability 1/3 under eight seeds, lanes in reverse, workgroups permuted (all eleven schedules for
every case: none was cut).  Every buffer, the LDS block and the kernel's argument block included, is a heap allocation
of exactly its size, and the emulator is built with the address and undefined-behaviour sanitizers: a clamp of the
kernel's unconditional loads that is off by one, a carve-up of LDS longer than the host's figure or a late_arg offset
behind the struct is a sanitizer report, not a silent read of a neighbouring allocation.  Under each schedule the tile
counters, the per-target counts, the status word, the hit count and the hit records must be the CPU oracle's.

Three control builds prove that the test can fail: an add that another fiber may cut in two (the per-target counters in
LDS, the hit log's place claim), an LDS block without the last wave's second queue buffer, and nbr one entry short.
The emulator is a stand-alone program; no GPU is involved, and the emulation is sequentially consistent and says
nothing about caches, time or the memory model."""
import os
import re
import subprocess

import scanq_cases as qc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
         "-I" + os.path.join(REPO, "include")]
SRC = os.path.join(REPO, "tools", "scan_queue_emu.cpp")
NAMES = ("n", "tiles", "T", "levels", "L", "k", "tpb", "schedules", "launches", "points", "mid_drains", "drains", "in_place",
         "finish_all", "pushes", "hits", "orders")
LINE = re.compile(r"case (\w+) ok: kernel (k_scan_q<\w+, \d, -?\d, \d>) " + " ".join(r"%s (-?\d+)" % name for name in NAMES) +
                  r" mid_qn ([\d,]+|-)")


def _constant(name, source):
    text = open(os.path.join(REPO, "well_duplicates_amd", "csrc", source)).read()
    m = re.search(r"constexpr int %s = (\w+);" % name, text).group(1)
    return int(m if m.isdigit() else re.search(r"#define %s (\d+)" % m, text).group(1))


def _build(tmp_path, name, *defines):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++"] + FLAGS + list(defines) + [SRC, "-o", exe])
    return exe


def _files(tmp_path, select=lambda c: True):
    paths = []
    for case in qc.cases():
        if select(case):
            paths.append(str(tmp_path / (case.name + ".sqc")))
            qc.write_case(paths[-1], case)
    return paths


def test_every_schedule_gives_the_oracles_counts(tmp_path):
    assert (_constant("kPass", "wd_shared.h"), _constant("kMaxPasses", "wd_shared.h"), _constant("kQCap", "scan_queue.inc"),
            _constant("kFinishInPlace", "scan_queue.inc"), _constant("kFinishAllMax", "scan_queue.inc")) == \
        (qc.K_PASS, qc.K_MAX_PASSES, qc.K_QCAP, qc.K_FINISH_IN_PLACE, qc.K_FINISH_ALL_MAX)
    exe = _build(tmp_path, "scan_queue_emu")
    out = subprocess.run([exe] + _files(tmp_path), capture_output=True, text=True, timeout=900)
    print(out.stdout)                                     # per case: the instantiation, the schedules run, the queues' events
    assert out.returncode == 0 and "MISMATCH" not in out.stdout, (out.stdout[-3000:], out.stderr[-3000:])
    rows = {row[0]: dict(zip(("kernel",) + NAMES, (row[1],) + tuple(int(v) for v in row[2:-1]))) for row in LINE.findall(out.stdout)}
    mid_qn = {row[0]: {int(v) for v in row[-1].split(",")} if row[-1] != "-" else set() for row in LINE.findall(out.stdout)}
    assert list(rows) == [c.name for c in qc.cases()] and len(out.stdout.strip().split("\n")) == len(rows)
    for case in qc.cases():
        r = rows[case.name]
        assert r["kernel"] == case.kernel, (case.name, r["kernel"])
        assert (r["n"], r["tiles"], r["T"], r["levels"], r["L"], r["k"], r["tpb"]) == \
            (case.n, len(case.tiles), case.T, case.levels, case.L, case.kk, case.tpb)
        # never, reverse, always and eight seeds at 1/3, a launch each; the tallies alone are atomics
        assert r["schedules"] == 11 and r["launches"] == 11 and r["points"] > 0, (case.name, r)
        assert r["hits"] == (qc.truth(case)["hits"].shape[0] if case.hit_cap >= 0 else -1)
        if "queue" in case.tags:                          # a drain with items still to come, under every schedule
            assert r["mid_drains"] >= 11 and r["pushes"] > r["drains"], (case.name, r)
            # the occupancy at those drains: the queue at exactly kQCap (wave 0), at one below (wave 1) and at 117 (wave 2)
            assert {qc.K_QCAP, qc.K_QCAP - 1, 117} <= mid_qn[case.name], (case.name, mid_qn[case.name])
        if "lowdiv" in case.tags:
            assert r["in_place"] >= 11, (case.name, r)
    # every instantiation the launchers can launch for the two families ran
    assert len({c.kernel for c in qc.cases()}) == 16 + 1 + 6 + 1
    # the order of the hit records is the schedule's: where the log is too small, different schedules keep different
    # records in a different order - otherwise the schedules tested nothing there
    for case in qc.cases():
        if case.name.endswith("equal_K127"):
            assert 0 < case.hit_cap < rows[case.name]["hits"] and rows[case.name]["orders"] >= 2, (case.name, rows[case.name])


def _run_control(tmp_path, exe, select):
    files = _files(tmp_path, select)
    assert files
    out = subprocess.run([exe] + files, capture_output=True, text=True, timeout=900)
    print(out.stdout[-3000:], out.stderr[:1500])
    return out


def test_a_torn_add_is_noticed(tmp_path):
    """-DWAVE_EMU_TORN_ADD: the adds on the per-target counters in LDS and the hit log's place claim may be cut in two.
    Every equal-reads case - every pair a duplicate - must end in MISMATCH on its per-target counts or its hit records
    (the emulator prints every kind that differs under the failing schedule: the tile counters, which the same build
    tears in the tally phase, do not count here), and both kinds must show among the cases."""
    exe = _build(tmp_path, "scan_queue_emu_torn", "-DWAVE_EMU_TORN_ADD")
    out = _run_control(tmp_path, exe, lambda c: "equal" in c.tags)
    assert out.returncode == 1, (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    failed = {}
    for name, kind in re.findall(r"MISMATCH case (\w+) schedule \d+ \(\w+\): ([a-z_ ]+?)(?: \(| \d+:)", out.stdout):
        failed.setdefault(name, set()).add(kind)
    seen = set()
    for case in qc.cases():
        if "equal" in case.tags:
            kinds = failed.get(case.name, set()) & {"out_per_target", "hit record"}
            assert kinds, (case.name, failed.get(case.name))
            seen |= kinds
    assert seen == {"out_per_target", "hit record"}, seen


def test_a_short_lds_block_is_a_sanitizer_report(tmp_path):
    """-DSCANQ_EMU_SHORT_LDS: the LDS block lacks the last wave's second queue buffer.  The case whose last wave drains
    with survivors that live through a round must end in a report of the address sanitizer."""
    exe = _build(tmp_path, "scan_queue_emu_short_lds", "-DSCANQ_EMU_SHORT_LDS")
    for case in qc.cases():
        if "lastdrain" in case.tags:
            out = _run_control(tmp_path, exe, lambda c: c.name == case.name)
            assert out.returncode != 0 and "AddressSanitizer: heap-buffer-overflow" in out.stderr and " ok:" not in out.stdout, \
                (case.name, out.returncode, out.stdout[-2000:], out.stderr[-2000:])


def test_a_short_nbr_is_a_sanitizer_report(tmp_path):
    """-DSCANQ_EMU_SHORT_NBR: nbr is one entry short.  The cases whose last target reads nbr's last entry - through the
    clamped, unconditional index loads - must end in a report of the address sanitizer."""
    exe = _build(tmp_path, "scan_queue_emu_short_nbr", "-DSCANQ_EMU_SHORT_NBR")
    for case in qc.cases():
        if "bufend" in case.tags:
            out = _run_control(tmp_path, exe, lambda c: c.name == case.name)
            assert out.returncode != 0 and "AddressSanitizer: heap-buffer-overflow" in out.stderr and " ok:" not in out.stdout, \
                (case.name, out.returncode, out.stdout[-2000:], out.stderr[-2000:])
