"""A lane's reported base quality against its duplicate copies, without a GPU: the host reference the GPU tests compare
against on a hand-worked lane and against the header's identities, the C ABI and its workspace and scratch arithmetic,
the CLI's flag checks, the report block and the fit check."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from lanedups_ref import lane_dups
from lanemismatch_ref import lane_mismatches, lane_pairs
from lanenear_ref import HAND, hand_made_lane, lane_near_dups
from lanequality_ref import (LANE_COLS, MAX_BINS, MAX_D, TILE_COLS, VALUES, bin_table, check_quality_identities,
                             lane_qualities)
from well_duplicates_amd import _lib, report
from well_duplicates_amd import count_well_duplicates as cwd

HEADER = os.path.join(_lib.INCLUDE, "welldup_lanequality.h")

# ---- the host reference -------------------------------------------------------------------------
# lanenear_ref.hand_made_lane: a base's byte fixes its quality there - A 16, C 32, G 48, T 8, N 0 - but for well 18
# (AAAAAA on tile index 4), whose bytes carry 20 at the even cycles and 31 at the odd ones.  With the edges below the
# bins are N 0, T 1, A (and 20) 2, 31 3, C 4, G 5.  The pairs (tests/test_lanemismatch_host.py lists them), root <-
# member, and what they add to Obs (a * marks a cycle where the bases differ: Mis):
#   K = 2   0 AAAAAA <- 4 CAAAAA    (2,4)* (2,2) x 5
#           1 NAGGTT <- 6 NAGGTC    (0,0) (2,2) (5,5) x 2 (1,1) (1,4)*
#           3 GGGGGG <- 7 GGGGGT    (5,5) x 5 (5,1)*
#           0 AAAAAA <- 8 CCAAAA    (2,4)* x 2 (2,2) x 4
#           1 NAGGTT <- 9 AAGGTA    (0,2)* (2,2) (5,5) x 2 (1,1) (1,2)*
#           2 CGCGCG <- 17 CGCGCG   (4,4) x 3 (5,5) x 3
#           0 AAAAAA <- 18 AAAAAA   (2,2) x 3 (2,3) x 3
#           3 <- 10 and 3 <- 11 lie three and four cycles from their root: not profiled at max_d = 2
EDGES = [0, 8, 16, 21, 32, 48]
HAND_QHIST = {0: 2, 8: 17, 16: 24, 20: 3, 31: 3, 32: 12, 48: 29}       # the 15 PF reads letter by letter: 90 bases
HAND_OBS = {(2, 2): 14, (2, 4): 3, (0, 0): 1, (5, 5): 12, (1, 1): 2, (1, 4): 1, (5, 1): 1, (0, 2): 1, (1, 2): 1, (4, 4): 3,
            (2, 3): 3}
HAND_MIS = {(2, 4): 3, (1, 4): 1, (5, 1): 1, (0, 2): 1, (1, 2): 1}


def _matrix(cells):
    m = np.zeros((MAX_BINS, MAX_BINS), dtype=np.int64)
    for at, n in cells.items():
        m[at] = n
    return m


def _hand(k, max_d, edges=EDGES):
    tiles = hand_made_lane()
    labels = lane_near_dups(tiles, 4, 5, k)[2] if k else lane_dups(tiles, 4, 5)[2]
    assert labels.tolist() == HAND[k]["labels"]
    return tiles, labels, lane_qualities(tiles, 4, 5, labels, max_d, edges)


def test_reference_gives_the_hand_worked_answer():
    tiles, labels, (lane, trow, qhist, obs, mis) = _hand(2, 2)
    assert lane.tolist() == [9, 7, 42, 7]
    assert trow.tolist() == [[0] * 4, [3, 3, 18, 3], [4, 2, 12, 4], [0] * 4, [2, 2, 12, 0]]
    assert {q: int(n) for q, n in enumerate(qhist) if n} == HAND_QHIST
    assert (obs == _matrix(HAND_OBS)).all() and (mis == _matrix(HAND_MIS)).all()
    check_quality_identities(lane, trow, qhist, obs, mis, 2, 6, len(EDGES), mismatch=lane_mismatches(tiles, 4, 5, labels, 2),
                             pf_wells=15)
    # every pair profiled: 3 <- 10 (GGGTTT) and 3 <- 11 (GGTTTT) add (5,5) x 5 and (5,1) x 7, all but the first five Mis
    lane7, _, qhist7, obs7, mis7 = _hand(2, 7)[2]
    assert lane7.tolist() == [9, 9, 54, 14] and (qhist7 == qhist).all()
    assert (obs7 - obs == _matrix({(5, 5): 5, (5, 1): 7})).all() and (mis7 - mis == _matrix({(5, 1): 7})).all()
    # one bin: everything in cell (0, 0)
    one = _hand(2, 2, [0])[2]
    assert (one[3] == _matrix({(0, 0): 42})).all() and (one[4] == _matrix({(0, 0): 7})).all()
    # by equality: 2 <- 17 and 0 <- 18
    tiles, labels, eq = _hand(0, 5)
    assert eq[0].tolist() == [2, 2, 12, 0] and (eq[3] == _matrix({(4, 4): 3, (5, 5): 3, (2, 2): 3, (2, 3): 3})).all()
    check_quality_identities(*eq, 5, 6, len(EDGES), mismatch=lane_mismatches(tiles, 4, 5, labels, 5), pf_wells=15, equality=True)


def test_bin_table_is_the_largest_edge_not_above():
    t = bin_table([0, 2, 10, 20, 25, 30, 35, 40])
    assert t[[0, 1, 2, 9, 10, 19, 20, 24, 25, 29, 30, 34, 35, 39, 40, 63]].tolist() == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7]
    assert bin_table([0]).tolist() == [0] * 64 and bin_table([0, 63]).tolist() == [0] * 63 + [1]
    assert bin_table([0, 5, 5, 9])[[4, 5, 8, 9]].tolist() == [0, 2, 2, 3]      # equal edges: the earlier bin is empty
    for bad in ([], [1], [0, 64], [0, 9, 8], list(range(9))):
        with pytest.raises(AssertionError):
            bin_table(bad)


def test_reference_identities_on_a_random_lane():
    n, max_tiles, L = 300, 6, 24
    rng = np.random.default_rng(12)
    index = [4, 0, 3, 1]
    m = len(index) * n
    levels = np.array([2, 12, 23, 37, 40, 41, 63], dtype=np.uint8)
    reads = (levels[rng.integers(0, levels.size, (m, L))] << 2 | rng.integers(0, 4, (m, L))).astype(np.uint8)
    reads[rng.random(reads.shape) < 0.02] = 0
    for spread in (0, 1, 2, 3):                                        # copies at 0..3 cycles, with qualities of their own
        src, dst = rng.choice(m, m // 8, replace=False), rng.choice(m, m // 8, replace=False)
        copy = (reads[src] & 3) | (levels[rng.integers(0, levels.size, (dst.size, L))] << 2)
        copy[reads[src] == 0] = 0
        reads[dst] = copy
        for w in dst.tolist():
            for c in rng.choice(L, spread, replace=False).tolist():
                reads[w, c] = 0 if rng.random() < 0.1 else (int(reads[w, c]) & 0xFC) | ((int(reads[w, c]) + 1) & 3) | 4
    filt = (rng.random(m) < 0.9).astype(np.uint8)
    tiles = [(ti, [np.ascontiguousarray(reads[i * n:(i + 1) * n, c]) for c in range(L)], filt[i * n:(i + 1) * n])
             for i, ti in enumerate(index)]
    pf = int(filt.sum())
    edges = [0, 2, 12, 23, 37, 40, 41, 63]
    eq_labels = lane_dups(tiles, n, max_tiles)[2]
    got = lane_qualities(tiles, n, max_tiles, eq_labels, 3, edges)
    check_quality_identities(*got, 3, L, 8, mismatch=lane_mismatches(tiles, n, max_tiles, eq_labels, 3), pf_wells=pf, equality=True)
    seen = np.bincount((reads[filt.astype(bool)] >> 2).reshape(-1), minlength=64)
    assert (got[2] == seen).all() and 8 <= (seen > 0).sum() < 20      # QHist: zero outside the values that occur
    for k in (1, 2):
        labels = lane_near_dups(tiles, n, max_tiles, k)[2]
        before = None
        for max_d in range(MAX_D + 1):
            got = lane_qualities(tiles, n, max_tiles, labels, max_d, edges)
            check_quality_identities(*got, max_d, L, 8, mismatch=lane_mismatches(tiles, n, max_tiles, labels, max_d),
                                     pf_wells=pf, shallower=before)
            before = got
        assert got[0][0] > 30 and got[4].sum() > 10 and (got[3] > 0).sum() > 40
        few = lane_qualities(tiles, n, max_tiles, labels, k, edges[:3])
        check_quality_identities(*few, k, L, 3)
        assert few[3][:3, :3].sum() == few[0][2] and (few[2] == got[2]).all()      # QHist does not depend on the bins
        # the same read off pair by pair
        ids, roots, a, b = lane_pairs(tiles, n, max_tiles, labels)
        table, qual = bin_table(edges), reads >> 2
        where = {ti * n: i * n for i, ti in enumerate(index)}          # global id of a tile's first well -> its row in reads
        row = lambda g: where[g // n * n] + g % n
        obs, mis = np.zeros((8, 8), dtype=np.int64), np.zeros((8, 8), dtype=np.int64)
        for p in range(ids.size):
            if (a[:, p] != b[:, p]).sum() <= k:
                for c in range(L):
                    cell = table[qual[row(int(roots[p])), c]], table[qual[row(int(ids[p])), c]]
                    obs[cell] += 1
                    mis[cell] += a[c, p] != b[c, p]
        want = lane_qualities(tiles, n, max_tiles, labels, k, edges)
        assert (obs == want[3]).all() and (mis == want[4]).all()


# ---- C ABI --------------------------------------------------------------------------------------
def test_lanequality_header_and_binding_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert '#include "welldup_lanedistance.h"' in text
    syms = sorted(set(re.findall(r"\b(wd_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.LANEQUALITY_PROTOTYPES) == ["wd_lane_qual_add", "wd_lane_qual_begin", "wd_lane_qual_scratch",
                                                           "wd_lane_qual_workspace", "wd_lane_qualities"]
    assert int(re.search(r"#define WD_LANEQUALITY_MAX_BINS\s+(\d+)", text).group(1)) == _lib.LANEQUALITY_MAX_BINS == MAX_BINS
    assert int(re.search(r"#define WD_LANEQUALITY_VALUES\s+(\d+)", text).group(1)) == _lib.LANEQUALITY_VALUES == VALUES
    assert re.search(r"#define WD_LANEQUALITY_MAX_D\s+WD_LANEMISMATCH_MAX_D", text) and _lib.LANEQUALITY_MAX_D == MAX_D == 7
    assert int(re.search(r"#define WD_LANEQUALITY_LANE_COLS\s+(\d+)", text).group(1)) == _lib.LANEQUALITY_LANE_COLS == LANE_COLS
    assert int(re.search(r"#define WD_LANEQUALITY_TILE_COLS\s+(\d+)", text).group(1)) == _lib.LANEQUALITY_TILE_COLS == TILE_COLS
    assert report.LANE_QUALITY_COLS == LANE_COLS == TILE_COLS and report.LANE_QUALITY_MAX_BINS == MAX_BINS
    assert report.LANE_QUALITY_VALUES == VALUES and report.LANE_QUALITY_MAX_D == MAX_D
    taken = set()
    for table in (_lib.PROTOTYPES, _lib.SETS_PROTOTYPES, _lib.TILEDUPS_PROTOTYPES, _lib.TILENEAR_PROTOTYPES,
                  _lib.LANEDUPS_PROTOTYPES, _lib.LANENEAR_PROTOTYPES, _lib.LANEINDEX_PROTOTYPES, _lib.LANEMISMATCH_PROTOTYPES,
                  _lib.LANEDISTANCE_PROTOTYPES):
        taken |= set(table)
    assert not set(_lib.LANEQUALITY_PROTOTYPES) & taken
    source = open(os.path.join(_lib.CSRC, "lane_quality.inc")).read()
    assert "k_lq_tally" in source and "k_lq_pack" in source and _lib.unit_of_kernel("k_lq_tally") == "tiledups"
    assert "lm_compare(" in source and "lm_fold(" in source and "ld_store_staged(" in source      # used, not copied
    assert "lm_compare(const" not in source and "lm_fold(uint32_t x" not in source
    deps = {os.path.basename(f) for f in _lib._deps(os.path.join(_lib.CSRC, "welldup_tiledups.hip"))}
    assert {"lane_quality.inc", "welldup_lanequality.h", "lane_distance.inc", "lane_mismatch.inc", "lane_dups.inc"} <= deps
    unit = open(os.path.join(_lib.CSRC, "welldup_tiledups.hip")).read()
    assert unit.index('#include "lane_distance.inc"') < unit.index('#include "lane_quality.inc"')
    assert unit.rstrip().splitlines()[-1].startswith('#include "lane_quality.inc"')
    _lib.build()
    lib = _lib.load()
    for s in syms:                                                     # exported, and bound as the table says
        assert getattr(lib, s).argtypes == _lib.LANEQUALITY_PROTOTYPES[s][1]
    ids = _lib.build_ids()
    assert ids["tiledups"] == _lib.source_unit_ids()["tiledups"] and ids["all"] == _lib.source_build_id()


def _up(v):
    return (v + 255) // 256 * 256


def _workspace_formula(n, tiles, L):
    """The arithmetic include/welldup_lanequality.h states."""
    return 32768 + _up(8 * tiles * L) + _up(8 * tiles) + _up(4 * tiles) + _up(4 * ((L + 9) // 10) * tiles * n)


def _scratch_formula(tiles):
    return _up(2048 * tiles) + 65536 + _up(4 * tiles)


def _size(fn, *args):
    b = ctypes.c_size_t()
    rc = fn(*args, ctypes.byref(b))
    return rc, b.value


def test_workspace_and_scratch_sizes_need_no_gpu_and_match_the_header():
    _lib.build()
    lib = _lib.load()
    text = open(HEADER).read()
    for piece in ("32768 ", "+ 8 * max_tiles * L", "+ 8 * max_tiles ", "+ 4 * max_tiles ", "+ 4 * R * W", "R = ceil(L / 10)",
                  "rounded up to 256 bytes", "11.6 GB at 51 cycles, 30.9 GB at 151", "2048 * max_tiles", "+ 65536", "295 KB"):
        assert piece in text, piece
    for tiles in (0, 1, 3, 7, 112):
        assert _size(lib.wd_lane_qual_scratch, tiles) == (0, _scratch_formula(tiles))
        for n in (0, 1, 601, 2640, 4309253):
            for L in (0, 1, 10, 11, 37, 83, 151, 1024):
                assert _size(lib.wd_lane_qual_workspace, n, tiles, L) == (0, _workspace_formula(n, tiles, L)), (n, tiles, L)
    assert _size(lib.wd_lane_qual_scratch, 112) == (0, 295424)         # the header's HiSeq 4000 lane
    assert round(_size(lib.wd_lane_qual_workspace, 4309253, 112, 51)[1] / 1e9, 1) == 11.6
    assert round(_size(lib.wd_lane_qual_workspace, 4309253, 112, 151)[1] / 1e9, 1) == 30.9
    lanedups = lambda *a: _size(lib.wd_lane_dups_workspace, *a)[0]      # limits and error codes are the accumulator's
    for bad in ((-1, 3, 10), (10, -1, 10), (10, 3, -1), (10, 3, 1025), (10, 65536, 10), (1 << 31, 2, 10)):
        rc = _size(lib.wd_lane_qual_workspace, *bad)[0]
        assert rc == lanedups(*bad) and rc in (_lib.ERR_ARG, _lib.ERR_UNSUPPORTED), bad
    assert _size(lib.wd_lane_qual_scratch, 65536)[0] == _lib.ERR_UNSUPPORTED and _size(lib.wd_lane_qual_scratch, -1)[0] == _lib.ERR_ARG
    assert lib.wd_lane_qual_workspace(10, 3, 10, None) == _lib.ERR_ARG and lib.wd_lane_qual_scratch(3, None) == _lib.ERR_ARG
    row = (ctypes.c_int64 * 64)()                                      # a null handle is refused before anything is looked at
    assert lib.wd_lane_qualities(None, 1, None, 0, row, row, row, row, row) == _lib.ERR_ARG
    assert lib.wd_lane_qual_begin(None, 1, (ctypes.c_int * 1)(0), None, 0) == _lib.ERR_ARG
    assert lib.wd_lane_qual_add(None, 0, None, None, None) == _lib.ERR_ARG


# ---- CLI ----------------------------------------------------------------------------------------
def test_cli_flag_checks(tmp_path, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["-s", "hiseq_4000", "-r", str(tmp_path), "--all-wells"]
    lane = ["--lane-dups"]
    near = ["--lane-dups", "--lane-dups-hamming", "2"]
    args = cwd.parse_args(base + lane + ["--lane-dups-quality"])       # without --lane-dups-hamming: allowed
    assert args.lane_dups_quality and args.lane_dups_quality_max_d is None
    assert args.lane_dups_quality_edges == cwd.DEFAULT_QUALITY_BINS == [0, 2, 10, 20, 25, 30, 35, 40]
    args = cwd.parse_args(base + near + ["--lane-dups-quality", "--lane-dups-quality-bins", "0,2,12,23,37",
                                         "--lane-dups-quality-max-d", "0"])
    assert args.lane_dups_quality_edges == [0, 2, 12, 23, 37] and args.lane_dups_quality_max_d == 0
    assert cwd.parse_args(base + near + ["--lane-dups-quality", "--lane-dups-quality-bins", "0"]).lane_dups_quality_edges == [0]
    assert not cwd.parse_args(base + near).lane_dups_quality
    q = ["--lane-dups-quality"]
    for extra, message in ((q, "--lane-dups-quality needs --lane-dups"),
                           (["--tile-dups"] + q, "--lane-dups-quality needs --lane-dups"),
                           (near + ["--lane-dups-quality-bins", "0,5"], "--lane-dups-quality-bins needs --lane-dups-quality"),
                           (near + ["--lane-dups-quality-max-d", "1"], "--lane-dups-quality-max-d needs --lane-dups-quality"),
                           (near + q + ["--lane-dups-quality-max-d", "8"], "--lane-dups-quality-max-d takes 0..7, not 8"),
                           (near + q + ["--lane-dups-quality-max-d", "-1"], "--lane-dups-quality-max-d takes 0..7, not -1"),
                           (near + q + ["--lane-dups-quality-bins", "2,10"], "--lane-dups-quality-bins: the first edge is 0"),
                           (near + q + ["--lane-dups-quality-bins", "0,10,9"], "--lane-dups-quality-bins: the edges ascend"),
                           (near + q + ["--lane-dups-quality-bins", "0,64"], "--lane-dups-quality-bins: a quality is at most 63"),
                           (near + q + ["--lane-dups-quality-bins", "0,1,2,3,4,5,6,7,8"],
                            "--lane-dups-quality-bins: 1..8 lower edges, not 9"),
                           (near + q + ["--lane-dups-quality-bins", "0,x"],
                            "--lane-dups-quality-bins: a comma-separated list of integers")):
        with pytest.raises(SystemExit):
            cwd.parse_args(base + extra)
        assert message in " ".join(capsys.readouterr().err.split()), message
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cwd.parse_args(base + near + q)
    assert "--lane-dups runs in a single process only" in " ".join(capsys.readouterr().err.split())


def test_cli_help_names_the_new_options(capsys):
    with pytest.raises(SystemExit):
        cwd.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--lane-dups-quality " in text and "--lane-dups-quality-bins E0,E1,.." in text
    assert "--lane-dups-quality-max-d D" in text and "default 0,2,10,20,25,30,35,40" in text
    assert "truncated from above" in text and "distinct molecules within K inflate them" in text


def test_the_quality_workspace_counts_when_a_lane_is_fitted():
    cwd.check_lane_dups_fits(1000, 2900, 2, 3, 4, scratch=500, index=300, mismatch=100, quality=1000)
    with pytest.raises(MemoryError) as e:
        cwd.check_lane_dups_fits(1000, 2900, 2, 3, 4, scratch=500, index=300, mismatch=100, quality=1001)
    msg = str(e.value)
    assert ("2901 bytes, 500 of them for --lane-dups-hamming, 300 of them for --lane-dups-index, 100 of them for "
            "--lane-dups-mismatches, 1001 of them for --lane-dups-quality)") in msg and "2900 bytes" in msg
    with pytest.raises(MemoryError) as e:                              # without the flag the message is what it was
        cwd.check_lane_dups_fits(1000, 1400, 2, 3, 4, scratch=401)
    assert "(1401 bytes, 401 of them for --lane-dups-hamming)" in str(e.value)


# ---- report -------------------------------------------------------------------------------------
CAVEAT = "(rates are truncated from above: clusters only link within 2; distinct molecules within 2 inflate them)"
SUMMARY = (
    "LaneQualitiesSummary: 3\tTiles: 4\tHamming: 2\tMaxD: 2\tPairs: 9\tProfiled: 7 (0.77778)\tObservations: 42\tMismatches: 7\t"
    + CAVEAT + "\n"
    "LaneQualities: 3\tBin: 0-7\tValues: 0\tPF share: 0.02222\tRoots: 0.04762\tMembers: 0.02381\tMean Q: 0.00\t"
    "Error rate: 0.000e+00 (Q inf)\tAgainst top bin: - (Q -)\n"
    "LaneQualities: 3\tBin: 8-15\tValues: 8\tPF share: 0.18889\tRoots: 0.09524\tMembers: 0.07143\tMean Q: 8.00\t"
    "Error rate: 0.000e+00 (Q inf)\tAgainst top bin: 1.000e+00 (Q 0.0)\n"
    "LaneQualities: 3\tBin: 16-20\tValues: 16,20\tPF share: 0.30000\tRoots: 0.47619\tMembers: 0.38095\tMean Q: 16.44\t"
    "Error rate: 0.000e+00 (Q inf)\tAgainst top bin: - (Q -)\n"
    "LaneQualities: 3\tBin: 21-31\tValues: 31\tPF share: 0.03333\tRoots: 0.00000\tMembers: 0.07143\tMean Q: 31.00\t"
    "Error rate: - (Q -)\tAgainst top bin: - (Q -)\n"
    "LaneQualities: 3\tBin: 32-47\tValues: 32\tPF share: 0.13333\tRoots: 0.07143\tMembers: 0.16667\tMean Q: 32.00\t"
    "Error rate: 0.000e+00 (Q inf)\tAgainst top bin: - (Q -)\n"
    "LaneQualities: 3\tBin: 48-63\tValues: 48\tPF share: 0.32222\tRoots: 0.30952\tMembers: 0.28571\tMean Q: 48.00\t"
    "Error rate: 0.000e+00 (Q inf)\tAgainst top bin: - (Q -)\n")
TILE_LINES = (
    "LaneQualities: 3\tTile: 1101\tPairs: 0\tProfiled: 0\tObservations: 0\tMismatches: 0\n"
    "LaneQualities: 3\tTile: 1102\tPairs: 3\tProfiled: 3\tObservations: 18\tMismatches: 3\n"
    "LaneQualities: 3\tTile: 1103\tPairs: 4\tProfiled: 2\tObservations: 12\tMismatches: 4\n"
    "LaneQualities: 3\tTile: 1105\tPairs: 2\tProfiled: 2\tObservations: 12\tMismatches: 0\n")
MATRICES = (
    "LaneQualities: 3\tObs root bin 0-7:\t1\t0\t1\t0\t0\t0\n"
    "LaneQualities: 3\tObs root bin 8-15:\t0\t2\t1\t0\t1\t0\n"
    "LaneQualities: 3\tObs root bin 16-20:\t0\t0\t14\t3\t3\t0\n"
    "LaneQualities: 3\tObs root bin 21-31:\t0\t0\t0\t0\t0\t0\n"
    "LaneQualities: 3\tObs root bin 32-47:\t0\t0\t0\t0\t3\t0\n"
    "LaneQualities: 3\tObs root bin 48-63:\t0\t1\t0\t0\t0\t12\n"
    "LaneQualities: 3\tMis root bin 0-7:\t0\t0\t1\t0\t0\t0\n"
    "LaneQualities: 3\tMis root bin 8-15:\t0\t0\t1\t0\t1\t0\n"
    "LaneQualities: 3\tMis root bin 16-20:\t0\t0\t0\t0\t3\t0\n"
    "LaneQualities: 3\tMis root bin 21-31:\t0\t0\t0\t0\t0\t0\n"
    "LaneQualities: 3\tMis root bin 32-47:\t0\t0\t0\t0\t0\t0\n"
    "LaneQualities: 3\tMis root bin 48-63:\t0\t1\t0\t0\t0\t0\n")


def test_the_hand_worked_lane_as_a_report():
    """K = 2, max_d = 2, tile index 3 never a tile of the lane."""
    names = ["1101", "1102", "1103", None, "1105"]
    c = report.LaneQualityCounts.from_rows(*_hand(2, 2)[2], names, 2, 2, EDGES)
    assert (c.pairs, c.profiled, c.observations, c.mismatches) == (9, 7, 42, 7) and c.occupied() == [0, 1, 2, 3, 4, 5]
    assert c.values(2) == [16, 20] and c.seen(2) == 27 and c.roots(2) == 20 and c.members(2) == 16
    assert c.error_rate(3) is None and c.error_rate(5) == 0.0 and c.error_rate_against_top(1) == 1.0
    assert c.error_rate_against_top(5) is None and c.error_rate_against_top(2) is None
    out = io.StringIO()
    report.write_lane_qualities("3", c, verbose=True, out=out)
    assert out.getvalue() == "\n" + TILE_LINES + SUMMARY + MATRICES
    out = io.StringIO()
    report.write_lane_qualities("3", c, out=out)                       # -S: the summary line and the bins
    assert out.getvalue() == "\n" + SUMMARY


def test_rates_of_a_table_with_errors():
    """Two bins, low (0-29) and high (30-63): 1000 observations high against high with 2 mismatches, 200 low against
    high (either way round) with 11, 50 low against low with 5."""
    obs, mis = np.zeros((8, 8), dtype=np.int64), np.zeros((8, 8), dtype=np.int64)
    obs[1, 1], mis[1, 1], obs[0, 1], mis[0, 1], obs[1, 0], mis[1, 0], obs[0, 0], mis[0, 0] = 1000, 2, 120, 7, 80, 4, 50, 5
    qhist = np.zeros(64, dtype=np.int64)
    qhist[[12, 37]] = 300, 2700
    c = report.LaneQualityCounts.from_rows([30, 25, 1250, 18], [[30, 25, 1250, 18]], qhist, obs, mis, ["1101"], 1, 1, [0, 30])
    assert c.error_rate(1) == 2 / 2000 and c.error_rate(0) == 5 / 100
    assert c.error_rate_against_top(0) == 11 / 200 - 0.001 and c.error_rate_against_top(1) is None
    out = io.StringIO()
    report.write_lane_qualities("1", c, out=out)
    assert out.getvalue() == (
        "\nLaneQualitiesSummary: 1\tTiles: 1\tHamming: 1\tMaxD: 1\tPairs: 30\tProfiled: 25 (0.83333)\tObservations: 1250\t"
        "Mismatches: 18\t(rates are truncated from above: clusters only link within 1; distinct molecules within 1 inflate them)\n"
        "LaneQualities: 1\tBin: 0-29\tValues: 12\tPF share: 0.10000\tRoots: 0.13600\tMembers: 0.10400\tMean Q: 12.00\t"
        "Error rate: 5.000e-02 (Q 13.0)\tAgainst top bin: 5.400e-02 (Q 12.7)\n"
        "LaneQualities: 1\tBin: 30-63\tValues: 37\tPF share: 0.90000\tRoots: 0.86400\tMembers: 0.89600\tMean Q: 37.00\t"
        "Error rate: 1.000e-03 (Q 30.0)\tAgainst top bin: - (Q -)\n")
    mis[0, 1] = 0                                                      # below the top bin's own rate: clamped at 0
    obs[0, 1], obs[1, 0], mis[1, 0] = 4000, 10, 1
    c = report.LaneQualityCounts.from_rows([30, 25, 5060, 8], [[30, 25, 5060, 8]], qhist, obs, mis, ["1101"], 1, 1, [0, 30])
    assert c.error_rate_against_top(0) == 0.0


def test_an_empty_lane_as_a_report():
    zeros = np.zeros((8, 8), dtype=np.int64)
    c = report.LaneQualityCounts.from_rows([0] * 4, [[0] * 4], [0] * 64, zeros, zeros, ["1101"], 0, 0, [0, 2, 10])
    out = io.StringIO()
    report.write_lane_qualities("1", c, verbose=True, out=out)
    assert out.getvalue() == (
        "\nLaneQualities: 1\tTile: 1101\tPairs: 0\tProfiled: 0\tObservations: 0\tMismatches: 0\n"
        "LaneQualitiesSummary: 1\tTiles: 1\tHamming: 0\tMaxD: 0\tPairs: 0\tProfiled: 0 (0.00000)\tObservations: 0\tMismatches: 0\t"
        "(under equality every copy is identical: only the reported qualities of copies against the lane's are shown)\n"
        "LaneQualities: 1\tObs root bin 0-1:\t0\t0\t0\n"
        "LaneQualities: 1\tObs root bin 2-9:\t0\t0\t0\n"
        "LaneQualities: 1\tObs root bin 10-63:\t0\t0\t0\n"
        "LaneQualities: 1\tMis root bin 0-1:\t0\t0\t0\n"
        "LaneQualities: 1\tMis root bin 2-9:\t0\t0\t0\n"
        "LaneQualities: 1\tMis root bin 10-63:\t0\t0\t0\n")
    for bad in (dict(lane=[0] * 5), dict(max_d=8), dict(edges=[1, 2]), dict(edges=[0, 64]), dict(edges=[0, 9, 8]),
                dict(qhist=[0] * 63)):
        a = dict(lane=[0] * 4, qhist=[0] * 64, max_d=0, edges=[0])
        a.update(bad)
        with pytest.raises(AssertionError):
            report.LaneQualityCounts.from_rows(a["lane"], [[0] * 4], a["qhist"], zeros, zeros, ["1101"], 0, a["max_d"], a["edges"])
