"""Where a lane's duplicate copies differ, without a GPU: the host reference the GPU tests compare against on a
hand-worked lane and against the header's identities, the C ABI and its scratch arithmetic, the CLI's flag checks,
the report block and the fit check."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from lanedups_ref import lane_dups
from lanemismatch_ref import (DIST_BINS, LANE_COLS, MAX_D, TILE_COLS, check_mismatch_identities, lane_mismatches,
                              lane_pairs)
from lanenear_ref import HAND, hand_made_lane, lane_near_dups
from well_duplicates_amd import _lib, report
from well_duplicates_amd import count_well_duplicates as cwd

HEADER = os.path.join(_lib.INCLUDE, "welldup_lanemismatch.h")
A, C, G, T, N_ = range(5)


# ---- the host reference -------------------------------------------------------------------------
# lanenear_ref.hand_made_lane, worked by hand (ids in brackets there; root <- member: the cycles where they differ):
#   K = 0   0 <- 18 and 2 <- 17: equal reads
#   K = 1   0 <- 4 (CAAAAA: cycle 0 A>C), 0 <- 8 (CCAAAA: cycles 0 and 1 A>C: two from the root, linked through 4),
#           1 <- 6 (NAGGTC: cycle 5 T>C; N == N), 3 <- 7 (GGGGGT: cycle 5 G>T), 10 <- 11 (GGTTTT: cycle 2 G>T), and K = 0's
#   K = 2   K = 1's with 10 and 11 now under root 3 (GGGGGG): 3 <- 10 (GGGTTT: cycles 3 4 5 G>T), 3 <- 11 (cycles
#           2 3 4 5 G>T), and 1 <- 9 (AAGGTA against NAGGTT: cycle 0 N>A, cycle 5 T>A)
HAND_MISMATCH = {
    (0, 7): dict(lane=[2, 2, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0], tiles=[[0] * 4, [0] * 4, [0] * 4, [0] * 4, [2, 2, 0, 0]], sub={}),
    (1, 0): dict(lane=[7, 2, 0, 0, 2, 4, 1, 0, 0, 0, 0, 0, 0], tiles=[[0] * 4, [3, 0, 0, 0], [2, 0, 0, 0], [0] * 4, [2, 2, 0, 0]],
                 sub={}),
    (1, 1): dict(lane=[7, 6, 4, 0, 2, 4, 1, 0, 0, 0, 0, 0, 0], tiles=[[0] * 4, [3, 3, 3, 0], [2, 1, 1, 0], [0] * 4, [2, 2, 0, 0]],
                 sub={(0, A, C): 1, (2, G, T): 1, (5, G, T): 1, (5, T, C): 1}),
    (1, 2): dict(lane=[7, 7, 6, 0, 2, 4, 1, 0, 0, 0, 0, 0, 0], tiles=[[0] * 4, [3, 3, 3, 0], [2, 2, 3, 0], [0] * 4, [2, 2, 0, 0]],
                 sub={(0, A, C): 2, (1, A, C): 1, (2, G, T): 1, (5, G, T): 1, (5, T, C): 1}),
    (2, 2): dict(lane=[9, 7, 7, 1, 2, 3, 2, 1, 1, 0, 0, 0, 0], tiles=[[0] * 4, [3, 3, 3, 0], [4, 2, 4, 1], [0] * 4, [2, 2, 0, 0]],
                 sub={(0, A, C): 2, (0, N_, A): 1, (1, A, C): 1, (5, G, T): 1, (5, T, A): 1, (5, T, C): 1}),
    (2, 7): dict(lane=[9, 9, 14, 1, 2, 3, 2, 1, 1, 0, 0, 0, 0], tiles=[[0] * 4, [3, 3, 3, 0], [4, 4, 11, 1], [0] * 4, [2, 2, 0, 0]],
                 sub={(0, A, C): 2, (0, N_, A): 1, (1, A, C): 1, (2, G, T): 1, (3, G, T): 2, (4, G, T): 2, (5, G, T): 3,
                      (5, T, A): 1, (5, T, C): 1}),
}


def _hand(k, max_d):
    tiles = hand_made_lane()
    labels = lane_near_dups(tiles, 4, 5, k)[2] if k else lane_dups(tiles, 4, 5)[2]
    assert labels.tolist() == HAND[k]["labels"]
    return lane_mismatches(tiles, 4, 5, labels, max_d)


@pytest.mark.parametrize("k,max_d", sorted(HAND_MISMATCH))
def test_reference_gives_the_hand_worked_answer(k, max_d):
    want = HAND_MISMATCH[(k, max_d)]
    lane, trow, sub = _hand(k, max_d)
    assert lane.tolist() == want["lane"] and trow.tolist() == want["tiles"]
    want_sub = np.zeros((6, 5, 5), dtype=np.int64)
    for at, n in want["sub"].items():
        want_sub[at] = n
    assert (sub == want_sub).all()
    finish = HAND[k]["lane"][:6] + HAND[k]["lane"][7:]                 # (HAND's lane rows carry NearPairs)
    check_mismatch_identities(lane, trow, sub, max_d, finish, HAND[k]["tiles"], equality=k == 0)


def test_reference_identities_on_a_random_lane():
    n, max_tiles, L = 300, 6, 24
    rng = np.random.default_rng(12)
    index = [4, 0, 3, 1]
    m = len(index) * n
    reads = rng.integers(1, 256, (m, L)).astype(np.uint8)
    reads[rng.random(reads.shape) < 0.02] = 0
    for spread in (0, 1, 2, 3):                                        # copies at 0..3 cycles, and copies of copies
        src, dst = rng.choice(m, m // 8, replace=False), rng.choice(m, m // 8, replace=False)
        reads[dst] = reads[src]
        for w in dst.tolist():
            for c in rng.choice(L, spread, replace=False).tolist():
                reads[w, c] = 0 if rng.random() < 0.1 else (int(reads[w, c]) & 0xFC) | ((int(reads[w, c]) + 1) & 3) | 4
    filt = (rng.random(m) < 0.9).astype(np.uint8)
    tiles = [(ti, [np.ascontiguousarray(reads[i * n:(i + 1) * n, c]) for c in range(L)], filt[i * n:(i + 1) * n])
             for i, ti in enumerate(index)]
    eq_lane, eq_tiles, eq_labels = lane_dups(tiles, n, max_tiles)
    got = lane_mismatches(tiles, n, max_tiles, eq_labels, 3)
    check_mismatch_identities(*got, 3, eq_lane, eq_tiles, equality=True)
    assert got[0][0] > 30                                              # (of the 150 equal copies: PF, and not written over)
    for k in (1, 2):
        near_lane, near_tiles, labels = lane_near_dups(tiles, n, max_tiles, k)
        finish = np.concatenate([near_lane[:6], near_lane[7:]])
        subs, got_dist = [], lane_mismatches(tiles, n, max_tiles, labels, 0)[0][4:]
        for max_d in range(MAX_D + 1):
            lane, trow, sub = lane_mismatches(tiles, n, max_tiles, labels, max_d)
            check_mismatch_identities(lane, trow, sub, max_d, finish, near_tiles)
            subs.append(sub)
            assert (lane[4:] == got_dist).all()                        # Dist does not depend on max_d
        assert all((a <= b).all() for a, b in zip(subs, subs[1:]))
        assert got_dist[:k + 2].all() and subs[-1][:, 4, :].sum() + subs[-1][:, :, 4].sum() > 0
        # the same read off pair by pair
        ids, roots, a, b = lane_pairs(tiles, n, max_tiles, labels)
        literal = np.zeros_like(subs[k])
        for p in range(ids.size):
            where = np.flatnonzero(a[:, p] != b[:, p])
            if where.size <= k:
                for c in where.tolist():
                    literal[c, a[c, p], b[c, p]] += 1
        assert (literal == subs[k]).all()


# ---- C ABI --------------------------------------------------------------------------------------
def test_lanemismatch_header_and_binding_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert '#include "welldup_laneindex.h"' in text
    syms = sorted(set(re.findall(r"\b(wd_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.LANEMISMATCH_PROTOTYPES) == ["wd_lane_mismatch_scratch", "wd_lane_mismatches"]
    assert int(re.search(r"#define WD_LANEMISMATCH_MAX_D\s+(\d+)", text).group(1)) == _lib.LANEMISMATCH_MAX_D == MAX_D
    assert int(re.search(r"#define WD_LANEMISMATCH_DIST_BINS\s+(\d+)", text).group(1)) == _lib.LANEMISMATCH_DIST_BINS == DIST_BINS
    assert re.search(r"#define WD_LANEMISMATCH_LANE_COLS\s+\(4 \+ WD_LANEMISMATCH_DIST_BINS\)", text)
    assert int(re.search(r"#define WD_LANEMISMATCH_TILE_COLS\s+(\d+)", text).group(1)) == _lib.LANEMISMATCH_TILE_COLS == TILE_COLS
    assert _lib.LANEMISMATCH_LANE_COLS == LANE_COLS == report.LANE_MISMATCH_LANE_COLS == 13
    assert report.LANE_MISMATCH_TILE_COLS == TILE_COLS and report.LANE_MISMATCH_MAX_D == MAX_D
    assert len(report.LANE_MISMATCH_DIST_NAMES) == DIST_BINS
    assert not set(_lib.LANEMISMATCH_PROTOTYPES) & set(_lib.PROTOTYPES)      # PROTOTYPES stays welldup.h's
    source = open(os.path.join(_lib.CSRC, "lane_mismatch.inc")).read()
    assert "k_lm_tally" in source and _lib.unit_of_kernel("k_lm_tally") == "tiledups"
    deps = {os.path.basename(f) for f in _lib._deps(os.path.join(_lib.CSRC, "welldup_tiledups.hip"))}
    assert {"lane_mismatch.inc", "welldup_lanemismatch.h", "lane_index.inc", "lane_near.inc", "lane_dups.inc"} <= deps
    unit = open(os.path.join(_lib.CSRC, "welldup_tiledups.hip")).read()
    assert unit.index('#include "lane_index.inc"') < unit.index('#include "lane_mismatch.inc"')
    _lib.build()
    lib = _lib.load()
    for s in syms:                                                     # exported, and bound as the table says
        assert getattr(lib, s).argtypes == _lib.LANEMISMATCH_PROTOTYPES[s][1]
    ids = _lib.build_ids()
    assert ids["tiledups"] == _lib.source_unit_ids()["tiledups"] and ids["all"] == _lib.source_build_id()


def _formula(tiles, L):
    """The arithmetic include/welldup_lanemismatch.h states."""
    up = lambda v: (v + 255) // 256 * 256
    return up(2048 * tiles) + 8192 + up(4 * tiles) + up(200 * L)


def _scratch(lib, tiles, L):
    b = ctypes.c_size_t()
    rc = lib.wd_lane_mismatch_scratch(tiles, L, ctypes.byref(b))
    return rc, b.value


def test_scratch_size_needs_no_gpu_and_matches_the_header():
    _lib.build()
    lib = _lib.load()
    text = open(HEADER).read()
    for piece in ("2048 * max_tiles", "+ 8192", "+ 4 * max_tiles", "+ 200 * L", "rounded up to 256 bytes", "268 KB"):
        assert piece in text, piece
    for tiles in (0, 1, 3, 7, 64, 65, 112, 65535):
        for L in (0, 1, 9, 10, 37, 83, 151, 302, 1024):
            assert _scratch(lib, tiles, L) == (0, _formula(tiles, L)), (tiles, L)
    assert _scratch(lib, 112, 151) == (0, 268288)                      # the header's HiSeq 4000 lane
    assert _scratch(lib, 65536, 10)[0] == _lib.ERR_UNSUPPORTED and _scratch(lib, 3, 1025)[0] == _lib.ERR_UNSUPPORTED
    assert _scratch(lib, -1, 10)[0] == _lib.ERR_ARG and _scratch(lib, 3, -1)[0] == _lib.ERR_ARG
    assert lib.wd_lane_mismatch_scratch(3, 10, None) == _lib.ERR_ARG
    row = (ctypes.c_int64 * 32)()                                      # a null handle is refused before anything is looked at
    assert lib.wd_lane_mismatches(None, 1, None, 0, row, row, row) == _lib.ERR_ARG


# ---- CLI ----------------------------------------------------------------------------------------
def test_cli_flag_checks(tmp_path, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["-s", "hiseq_4000", "-r", str(tmp_path), "--all-wells"]
    near = ["--lane-dups", "--lane-dups-hamming", "2"]
    args = cwd.parse_args(base + near + ["--lane-dups-mismatches"])
    assert args.lane_dups_mismatches and args.lane_dups_mismatches_max_d is None      # (D defaults to K where it is used)
    assert cwd.parse_args(base + near + ["--lane-dups-mismatches", "--lane-dups-mismatches-max-d", "0"]).lane_dups_mismatches_max_d == 0
    assert cwd.parse_args(base + near + ["--lane-dups-mismatches", "--lane-dups-mismatches-max-d", "7"]).lane_dups_mismatches_max_d == 7
    assert not cwd.parse_args(base + near).lane_dups_mismatches
    for extra, message in ((["--lane-dups", "--lane-dups-mismatches"], "--lane-dups-mismatches needs --lane-dups-hamming K"),
                           (["--lane-dups-mismatches"], "--lane-dups-mismatches needs --lane-dups-hamming K"),
                           (["--tile-dups", "--tile-dups-hamming", "1", "--lane-dups-mismatches"],
                            "--lane-dups-mismatches needs --lane-dups-hamming K"),
                           (near + ["--lane-dups-mismatches-max-d", "1"],
                            "--lane-dups-mismatches-max-d needs --lane-dups-mismatches"),
                           (near + ["--lane-dups-mismatches", "--lane-dups-mismatches-max-d", "8"],
                            "--lane-dups-mismatches-max-d takes 0..7, not 8"),
                           (near + ["--lane-dups-mismatches", "--lane-dups-mismatches-max-d", "-1"],
                            "--lane-dups-mismatches-max-d takes 0..7, not -1")):
        with pytest.raises(SystemExit):
            cwd.parse_args(base + extra)
        assert message in " ".join(capsys.readouterr().err.split())
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cwd.parse_args(base + near + ["--lane-dups-mismatches"])
    assert "--lane-dups runs in a single process only" in " ".join(capsys.readouterr().err.split())


def test_cli_help_names_the_new_options(capsys):
    with pytest.raises(SystemExit):
        cwd.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--lane-dups-mismatches " in text and "--lane-dups-mismatches-max-d D" in text
    assert "Mismatches / (2 x Profiled x cycles)" in text and "truncated from above" in text


def test_the_mismatch_scratch_counts_when_a_lane_is_fitted():
    cwd.check_lane_dups_fits(1000, 1900, 2, 3, 4, scratch=500, index=300, mismatch=100)
    with pytest.raises(MemoryError) as e:
        cwd.check_lane_dups_fits(1000, 1900, 2, 3, 4, scratch=500, index=300, mismatch=101)
    msg = str(e.value)
    assert ("1901 bytes, 500 of them for --lane-dups-hamming, 300 of them for --lane-dups-index, 101 of them for "
            "--lane-dups-mismatches)") in msg and "1900 bytes" in msg
    with pytest.raises(MemoryError) as e:                              # without the flag the message is what it was
        cwd.check_lane_dups_fits(1000, 1400, 2, 3, 4, scratch=401)
    assert "(1401 bytes, 401 of them for --lane-dups-hamming)" in str(e.value)


# ---- report -------------------------------------------------------------------------------------
SUMMARY = (
    "LaneMismatchesSummary: 3\tTiles: 4\tHamming: 2\tMaxD: 2\tPairs: 9\tProfiled: 7 (0.77778)\tMismatches: 7\tWithN: 1\n"
    "Dist: 0: 2 (0.22222)\t1: 3 (0.33333)\t2: 2 (0.22222)\t3: 1 (0.11111)\t4: 1 (0.11111)\t5: 0 (0.00000)\t6: 0 (0.00000)\t"
    "7: 0 (0.00000)\t>=8: 0 (0.00000)\n"
    "Mismatches per profiled pair: 1.00000\n"
    "Implied error rate per base (Mismatches / (2 x Profiled x 6 cycles)): 8.333e-02\n"
    "Substitution: A<>C\t3 (0.42857 of Mismatches)\n"
    "Substitution: A<>G\t0 (0.00000 of Mismatches)\n"
    "Substitution: A<>T\t1 (0.14286 of Mismatches)\n"
    "Substitution: C<>G\t0 (0.00000 of Mismatches)\n"
    "Substitution: C<>T\t1 (0.14286 of Mismatches)\n"
    "Substitution: G<>T\t1 (0.14286 of Mismatches)\n"
    "Substitution: A<>N\t1 (0.14286 of Mismatches)\n"
    "Substitution: C<>N\t0 (0.00000 of Mismatches)\n"
    "Substitution: G<>N\t0 (0.00000 of Mismatches)\n"
    "Substitution: T<>N\t0 (0.00000 of Mismatches)\n"
    "Pairs at distance 2, the last the clusters link: 2 (0.40000 of the pairs at 1..2, 0.22222 of Pairs)\n")
VERBOSE = (
    "LaneMismatches: 3\tTile: 1101\tPairs: 0\tProfiled: 0\tMismatches: 0\tWithN: 0\n"
    "LaneMismatches: 3\tTile: 1102\tPairs: 3\tProfiled: 3\tMismatches: 3\tWithN: 0\n"
    "LaneMismatches: 3\tTile: 1103\tPairs: 4\tProfiled: 2\tMismatches: 4\tWithN: 1\n"
    "LaneMismatches: 3\tTile: 1105\tPairs: 2\tProfiled: 2\tMismatches: 0\tWithN: 0\n"
    "LaneMismatches: 3\tCycle: 20\tMismatches: 3 (0.428571 per profiled pair)\tWithN: 1\n"
    "LaneMismatches: 3\tCycle: 21\tMismatches: 1 (0.142857 per profiled pair)\tWithN: 0\n"
    "LaneMismatches: 3\tCycle: 22\tMismatches: 0 (0.000000 per profiled pair)\tWithN: 0\n"
    "LaneMismatches: 3\tCycle: 50\tMismatches: 0 (0.000000 per profiled pair)\tWithN: 0\n"
    "LaneMismatches: 3\tCycle: 51\tMismatches: 0 (0.000000 per profiled pair)\tWithN: 0\n"
    "LaneMismatches: 3\tCycle: 52\tMismatches: 3 (0.428571 per profiled pair)\tWithN: 0\n")


def test_the_hand_worked_lane_as_a_report():
    """K = 2, max_d = 2, the cycles those of --cycles 20-23,50-53, tile index 3 never a tile of the lane."""
    names = ["1101", "1102", "1103", None, "1105"]
    c = report.LaneMismatchCounts.from_rows(*_hand(2, 2), names, 2, 2, [20, 21, 22, 50, 51, 52])
    assert (c.pairs, c.profiled, c.mismatches, c.with_n) == (9, 7, 7, 1) and c.dist == [2, 3, 2, 1, 1, 0, 0, 0, 0]
    assert c.per_cycle() == [(3, 1), (1, 0), (0, 0), (0, 0), (0, 0), (3, 0)]
    assert c.symmetric(A, C) == c.symmetric(C, A) == 3 and c.symmetric(A, N_) == 1 and c.per_pair() == 1.0
    assert c.error_rate() == 7 / (2 * 7 * 6)
    out = io.StringIO()
    report.write_lane_mismatches("3", c, verbose=True, out=out)
    assert out.getvalue() == "\n" + VERBOSE + SUMMARY
    out = io.StringIO()
    report.write_lane_mismatches("3", c, out=out)                      # -S: the summary alone
    assert out.getvalue() == "\n" + SUMMARY
    assert out.getvalue().count("Substitution: ") == 10 and "N<>N" not in out.getvalue()


def test_an_empty_lane_as_a_report():
    c = report.LaneMismatchCounts.from_rows([0] * 13, [[0] * 4], np.zeros((2, 5, 5), dtype=np.int64), ["1101"], 3, 3)
    out = io.StringIO()
    report.write_lane_mismatches("1", c, verbose=True, out=out)
    text = out.getvalue()
    assert "LaneMismatches: 1\tCycle: 1\tMismatches: 0 (0.000000 per profiled pair)\tWithN: 0\n" in text
    assert "Implied error rate per base (Mismatches / (2 x Profiled x 2 cycles)): 0.000e+00\n" in text
    assert text.endswith("Pairs at distance 3, the last the clusters link: 0 (0.00000 of the pairs at 1..3, 0.00000 of Pairs)\n")
    with pytest.raises(AssertionError):
        report.LaneMismatchCounts.from_rows([0] * 12, [[0] * 4], np.zeros((2, 5, 5)), ["1101"], 3, 3)
    with pytest.raises(AssertionError):
        report.LaneMismatchCounts.from_rows([0] * 13, [[0] * 4], np.zeros((2, 5, 5)), ["1101"], 3, 8)
