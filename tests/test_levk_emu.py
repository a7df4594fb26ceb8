"""The three kernels of Levenshtein <= k by the banded DP run on the CPU under shuffled schedules: tools/scan_lev_emu.cpp
compiles k_scan_q with LEVH 1 .. 3 (csrc/scan_queue.inc), k_scan<LevState<H>, ..> (csrc/scan_sequential.inc) and
k_scan_lev_generic (csrc/scan_lev_generic.inc) as they stand, plays the lanes of a workgroup with fibers
(tools/wave_emu.h), launches every case of tests/levk_cases.py as the launchers do - the grids, the lanes, the LDS bytes
of the host's own scan_q_lds_dwords(levels, tpb, 4) and lev_generic_lds_bytes(L, H) - and lets the schedule hand over to
another lane at every atomic: all eleven schedules for every case.  Every buffer, the dynamic LDS blocks and k_scan_q's
argument block included, is a heap allocation of exactly its size, and the emulator is built with the address and
undefined-behaviour sanitizers.  Under each schedule the tile counters, the per-target counts, the status word, the hit
count and the hit records with their distances must be the CPU oracle's.

`--state` checks the state alone: LevState<H>, and lev_pack / lev_unpack between the rounds for H <= 3, against the
textbook distance on every ordered pair over {A, C, N} of up to 6 cycles and on every pair of the cases, both orders.

Four control builds prove that the test can fail; what each breaks is said in its docstring.  The emulator is a
stand-alone program; no GPU is involved, and the emulation is sequentially consistent: it says nothing about caches,
time, the memory model, or what the device compiler makes of the same source (tests/test_gpu_levk_cases.py does)."""
import os
import re
import subprocess

import pytest

import levk_cases as lc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
         "-I" + os.path.join(REPO, "include")]
SRC = os.path.join(REPO, "tools", "scan_lev_emu.cpp")
NAMES = ("n", "tiles", "T", "levels", "L", "k", "tpb", "early", "schedules", "launches", "points", "mid_drains", "drains", "compactions",
         "pushes", "hits", "orders")
LINE = re.compile(r"case (\w+) ok: kernel (k_scan\w*<[\w<>, ]+>) " + " ".join(r"%s (-?\d+)" % name for name in NAMES) + r"\n")
MISMATCH = re.compile(r"MISMATCH case (\w+) schedule \d+ \(\w+\): ([a-z_ ]+?)(?: \(| \d+:)")


def _build(tmp_path, name, *defines):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++"] + FLAGS + list(defines) + [SRC, "-o", exe])
    return exe


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """the uncontrolled build, shared by the kernels' test and the state's"""
    return _build(tmp_path_factory.mktemp("levk_emu"), "scan_lev_emu")


def _files(tmp_path, select=lambda c: True):
    paths = []
    for case in lc.cases():
        if select(case):
            paths.append(str(tmp_path / (case.name + ".sqc")))
            lc.write_case(paths[-1], case)
    return paths


def _band_edge_pairs(case):
    cen, nb, dist = lc.pairs_of(case)
    return int(((dist <= case.kk) & (lc.restricted_distance(cen, nb, case.kk // 2 - 1) > case.kk)).sum())


def test_every_schedule_gives_the_oracles_counts(emu, tmp_path):
    out = subprocess.run([emu] + _files(tmp_path), capture_output=True, text=True, timeout=900)
    print(out.stdout)                                     # per case: the instantiation, the schedules run, the queues' events
    assert out.returncode == 0 and "MISMATCH" not in out.stdout and "Sanitizer" not in out.stderr, (out.stdout[-3000:], out.stderr[-3000:])
    rows = {row[0]: dict(zip(("kernel",) + NAMES, (row[1],) + tuple(int(v) for v in row[2:]))) for row in LINE.findall(out.stdout)}
    assert list(rows) == [c.name for c in lc.cases()] and len(out.stdout.strip().split("\n")) == len(rows)
    for case in lc.cases():
        r = rows[case.name]
        assert r["kernel"] == case.kernel, (case.name, r["kernel"])
        assert (r["n"], r["tiles"], r["T"], r["levels"], r["L"], r["k"], r["tpb"], r["early"]) == \
            (case.n, len(case.tiles), case.T, case.levels, case.L, case.kk, case.tpb, case.early)
        assert r["schedules"] == 11 and r["launches"] == 11 and r["points"] > 0, (case.name, r)
        assert r["hits"] == (lc.truth(case)["hits"].shape[0] if case.hit_cap >= 0 else -1)
        if case.kind == "queue" and case.L > case.B1:
            # survivors of the first round went through the queue entries under every schedule: packed, unpacked, compacted
            assert r["pushes"] >= 11 and r["drains"] >= 11, (case.name, r)
            if case.L > case.B1 + (4 if case.layout == "il" else 1):
                assert r["compactions"] >= 11, (case.name, r)
        else:
            assert r["pushes"] == r["drains"] == 0, (case.name, r)
    # every instantiation the launchers have ran: thirteen of k_scan_q, twelve of k_scan, two of the generic kernel
    ran = {r["kernel"] for r in rows.values()}
    assert len([k for k in ran if k.startswith("k_scan_q<")]) == 13 and len([k for k in ran if k.startswith("k_scan<LevState<")]) == 12 and \
        len([k for k in ran if k.startswith("k_scan_lev_generic<")]) == 2 and len(ran) == 27, sorted(ran)
    # a drain with entries still to come (the queue over its cap) happened somewhere: the mid-scan drain of the lev branch
    assert sum(r["mid_drains"] for r in rows.values()) > 0
    # the order of the hit records is the schedule's
    assert max(r["orders"] for r in rows.values()) >= 2


def test_the_state_alone_is_the_textbooks(emu, tmp_path):
    """LevState<H> for every H of the launchers, k = 2 H and 2 H + 1, every schedule of rounds: all ordered pairs over
    {A, C, N} of 1 .. 6 cycles, then every pair of every case in both orders, with a lev_pack / lev_unpack round trip
    behind every round for H <= 3.  dup() is (distance <= k), dist() the distance where it is within k, and no alive() on
    the way was false for a pair within k."""
    files = _files(tmp_path, lambda c: c.kind != "generic")
    out = subprocess.run([emu, "--state"] + files, capture_output=True, text=True, timeout=900)
    print(out.stdout[:300], "..", out.stdout[-600:])
    assert out.returncode == 0 and "MISMATCH" not in out.stdout and "Sanitizer" not in out.stderr, (out.stdout[-3000:], out.stderr[-3000:])
    runs = int(re.search(r"state exhaustive ok: pairs over \{A, C, N\} of 1 \.\. 6 cycles, runs (\d+)", out.stdout).group(1))
    pairs = sum(9 ** L for L in range(1, 7))
    # per H two thresholds; H = 1: three schedules (planes, interleaved, k_scan), H = 2, 3: two, H = 4, 6, 8: k_scan's
    assert runs == pairs * 2 * (3 + 2 + 2 + 1 + 1 + 1)
    done = dict(re.findall(r"state (\w+) ok: band \d+ k \d+ L \d+ runs (\d+)", out.stdout))
    for case in lc.cases():
        if case.kind != "generic":
            assert int(done[case.name]) == 2 * case.nbr.shape[0] * len(case.tiles), case.name


def _run_control(tmp_path, exe, select):
    files = _files(tmp_path, select)
    assert files
    out = subprocess.run([exe] + files, capture_output=True, text=True, timeout=900)
    print(out.stdout[-3000:], out.stderr[:1500])
    return out


def test_a_band_one_diagonal_short_is_noticed(tmp_path):
    """-DLEVK_EMU_NARROW: the kernels are handed k / 2 - 1 where the launchers hand k / 2 - the templated ones are
    instantiated with H - 1, the generic one gets H - 1 as its argument.  This breaks the emulator's own launch, not the
    library's source: it stands for a launcher or a kernel that is one diagonal out.  A case of every kind that has
    band-edge pairs (within k, but not by |j - i| <= H - 1: counted here from the oracle's distances) must end in MISMATCH on
    its per-target counts.  (k = 10, 11, 14, 15 are no such cases: launch_lev rounds their band up, and one diagonal less
    is still theirs.)"""
    names = ("queue_plane_k4_L37", "queue_ptr_k7_L64", "seq_plane_k8_L37_early1", "seq_ptr_k13_L37_early0", "seq_plane_k16_L37_early0",
             "generic_plane_k18_L40", "generic_ptr_k63_L64")
    exe = _build(tmp_path, "scan_lev_emu_narrow", "-DLEVK_EMU_NARROW")
    out = _run_control(tmp_path, exe, lambda c: c.name in names)
    assert out.returncode == 1, (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    failed = {}
    for name, kind in MISMATCH.findall(out.stdout):
        failed.setdefault(name, set()).add(kind)
    for name in names:
        case = lc.case(name)
        assert case.band == case.kk // 2 and _band_edge_pairs(case) >= 4, name
        assert "out_per_target" in failed.get(name, set()), (name, failed.get(name))


def test_a_cell_of_three_bits_is_noticed(tmp_path):
    """-DWD_LEV_CELL_MASK=7: lev_pack (the library's source, through the seam it has for this) keeps three bits of a band
    cell.  At k = 7 the cells saturate at 8, which then travels as 0: every k = 7 case that packs a state - L beyond the
    first round - must end in MISMATCH.  At k = 6 the cells saturate at 7 and three bits hold them: those cases must still
    pass, which is asserted too (so a mask that lost more than the fourth bit would show)."""
    exe = _build(tmp_path, "scan_lev_emu_pack3", "-DWD_LEV_CELL_MASK=7", "-DLEVK_EMU_KINDS=1")
    packs = lambda c: c.kind == "queue" and c.L > c.B1
    out = _run_control(tmp_path, exe, lambda c: packs(c) and c.kk in (6, 7))
    assert out.returncode == 1, (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    failed = {name for name, _ in MISMATCH.findall(out.stdout)}
    passed = {row[0] for row in LINE.findall(out.stdout)}
    seven = {c.name for c in lc.cases() if packs(c) and c.kk == 7}
    six = {c.name for c in lc.cases() if packs(c) and c.kk == 6}
    assert len(seven) >= 8 and len(six) >= 8 and failed == seven and passed == six, (sorted(seven - failed), sorted(six - passed))


def test_a_short_lds_block_of_the_generic_kernel_is_a_sanitizer_report(tmp_path):
    """-DLEVK_EMU_SHORT_LDS: the generic kernel's LDS block is kWave bytes shorter than lev_generic_lds_bytes(L, H) - the
    emulator's own launch, standing for a host figure that forgot a part of the carve-up.  The centre's codes lie at the
    block's end: a report of the address sanitizer, in both layouts."""
    exe = _build(tmp_path, "scan_lev_emu_short_lds", "-DLEVK_EMU_SHORT_LDS", "-DLEVK_EMU_KINDS=4")
    for name in ("generic_plane_k18_L40", "generic_ptr_k19_L64"):
        out = _run_control(tmp_path, exe, lambda c: c.name == name)
        assert out.returncode != 0 and "AddressSanitizer: heap-buffer-overflow" in out.stderr and " ok:" not in out.stdout, \
            (name, out.returncode, out.stdout[-2000:], out.stderr[-2000:])


def test_a_short_nbr_is_a_sanitizer_report(tmp_path):
    """-DSCANQ_EMU_SHORT_NBR: nbr is one entry short (tools/scan_emu_common.h: the emulator's own buffer).  The k_scan case
    whose last target is valid and reads nbr's last entry must end in a report of the address sanitizer."""
    exe = _build(tmp_path, "scan_lev_emu_short_nbr", "-DSCANQ_EMU_SHORT_NBR", "-DLEVK_EMU_KINDS=2")
    tagged = [c.name for c in lc.cases() if "bufend" in c.tags]
    assert tagged == ["seq_plane_k8_L37_early1"]
    case = lc.case(tagged[0])
    assert case.lvl_off[-1, -1] == case.nbr.shape[0] and (case.tiles[0][1][case.centre[-1]] & 1) == 1
    out = _run_control(tmp_path, exe, lambda c: c.name == tagged[0])
    assert out.returncode != 0 and "AddressSanitizer: heap-buffer-overflow" in out.stderr and " ok:" not in out.stdout, \
        (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
