"""Which libraries a lane's duplicate copies join, without a GPU: the two host references the GPU tests compare
against on a pooled lane and on a hand-worked one, the report block line by line, the Expected column as exact
fractions, the C ABI and its scratch arithmetic, and the CLI's flag checks."""
import ctypes
import io
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from lanedups_ref import lane_dups
from lanehops_ref import (LANE_COLS, MAX_E, MAX_LISTED, TILE_COLS, check_hop_identities, lane_hops, lane_hops_literal)
from laneindex_ref import index_keys, key_of
from lanenear_ref import lane_near_dups
from tiledups_ref import INVALID
from well_duplicates_amd import _lib, report
from well_duplicates_amd import count_well_duplicates as cwd

HEADER = os.path.join(_lib.INCLUDE, "welldup_lanehops.h")
_BYTE = {"A": 0x40, "C": 0x41, "G": 0x42, "T": 0x43, "N": 0}


# ---- the host references ------------------------------------------------------------------------
def _pool(seed, n, max_tiles, index, L, I, libraries):
    """A small pooled lane: reads copied within and across tiles, the copies' index reads kept, hit by one error, or
    replaced in the first part, the second, or both."""
    rng = np.random.default_rng(seed)
    m = len(index) * n
    reads = rng.integers(1, 256, (m, L)).astype(np.uint8)
    lib = rng.integers(1, 256, (libraries, I)).astype(np.uint8)
    idx = lib[rng.integers(0, libraries, m)]
    idx[rng.random(idx.shape) < 0.01] = 0
    for kind in range(5):
        src, dst = rng.choice(m, m // 10, replace=False), rng.choice(m, m // 10, replace=False)
        reads[dst] = reads[src]
        idx[dst] = idx[src]
        other = lib[rng.integers(0, libraries, dst.size)]
        if kind == 1:
            col = rng.integers(0, I, dst.size)
            idx[dst, col] = (idx[dst, col] + 1) & 3 | 4
        elif kind == 2:
            idx[dst, :I // 2] = other[:, :I // 2]
        elif kind == 3:
            idx[dst, I // 2:] = other[:, I // 2:]
        elif kind == 4:
            idx[dst] = other
    filt = (rng.random(m) < 0.9).astype(np.uint8)
    tiles = [(ti, [np.ascontiguousarray(reads[i * n:(i + 1) * n, c]) for c in range(L)], filt[i * n:(i + 1) * n])
             for i, ti in enumerate(index)]
    itiles = [(ti, [np.ascontiguousarray(idx[i * n:(i + 1) * n, c]) for c in range(I)]) for i, ti in enumerate(index)]
    return tiles, itiles


@pytest.mark.parametrize("I,split", [(8, 8), (16, 8), (20, 13), (11, 1)])
def test_the_two_references_agree_on_a_pooled_lane(I, split):
    n, max_tiles, index = 300, 6, [4, 0, 3, 1]
    tiles, itiles = _pool(7 + I, n, max_tiles, index, 20, I, 6)
    eq_lane, eq_tiles, eq_labels = lane_dups(tiles, n, max_tiles)
    near_lane, near_tiles, near_labels = lane_near_dups(tiles, n, max_tiles, 1)
    keys = index_keys(itiles, n, max_tiles)[0]
    pf_keys, count = np.unique(keys[eq_labels.reshape(-1) != INVALID], return_counts=True)
    top3 = pf_keys[np.argsort(-count, kind="stable")[:3]]
    for labels, lane_row, tile_rows in ((eq_labels, eq_lane, eq_tiles),
                                        (near_labels, np.concatenate([near_lane[:6], near_lane[7:]]), near_tiles)):
        for max_e in range(MAX_E + 1):
            for listed, all_listed in ((pf_keys[::-1], True), (top3, False), ([], False)):
                got = lane_hops(itiles, labels, n, max_tiles, I, split, max_e, listed)
                lit = lane_hops_literal(itiles, labels, n, max_tiles, I, split, max_e, listed)
                for g, w in zip(got, lit):
                    assert g.shape == w.shape and (g == w).all()
                check_hop_identities(got, lane_row, tile_rows, I, split, max_e, all_listed=all_listed)
        full = lane_hops(itiles, labels, n, max_tiles, I, split, 1, pf_keys)
        assert full[0][0] > 80 and full[0][4] > 20 and full[0][2] > 10 and (split in (1, I) or full[0][3] > 5)      # (a part of one cycle is never Far at E = 1)
        assert np.count_nonzero(full[2]) > 12


# Twelve wells on three tiles (ids in brackets; [3] fails the filter), four index cycles split 2 + 2, E = 1; the
# listing is AC+GT and CA+GT: two libraries with one i5.  root <- copy:
#   tile 0   [0] AC+GT root   [1] AC+GT <- 0  the same index          [2] CA+GT root   [3] -
#   tile 1   [4] AC+GA <- 0   one error in the second read: Same/Near, an unlisted key
#            [5] CA+GT <- 0   the first read swapped: Far/Same, into the listed library CA+GT
#            [6] CA+GT <- 2   the same index, across tiles
#            [7] CA+TG <- 2   the second read swapped (two cycles): Same/Far, into a combination nobody listed
#   tile 2   [8] TT+AA <- 0   both reads: Far/Far       [9] AC+GT root   [10] AC+GN <- 9  T > N: Same/Near, on its root's tile
#            [11] GG+GG, a well of its own
HAND_READS = ["ACGT", "ACGT", "CAGT", "AAAA", "ACGA", "CAGT", "CAGT", "CATG", "TTAA", "ACGT", "ACGN", "GGGG"]
HAND_LABELS = [[0, 0, 2, INVALID], [0, 0, 2, 2], [0, 9, 9, 11]]
HAND_LISTED = ["ACGT", "CAGT"]
HAND_LANE = [7, 2, 2, 1, 2, 2, 1, 0, 0, 0, 1, 0, 1]
HAND_TILES = [[1, 1, 0, 0], [4, 0, 2, 0], [2, 1, 0, 1]]
HAND_MATRIX = [[1, 1, 3], [0, 1, 1], [0, 0, 0]]
HAND_PF = [3, 3, 5]                                                    # AC+GT: 0 1 9; CA+GT: 2 5 6; the rest: 4 7 8 10 11
HAND_TEXT = """
LaneHops: 1\tIndex1: Same\tIndex2: Same\tPairs: 2 (0.28571)
LaneHops: 1\tIndex1: Same\tIndex2: Near\tPairs: 2 (0.28571)
LaneHops: 1\tIndex1: Same\tIndex2: Far\tPairs: 1 (0.14286)
LaneHops: 1\tIndex1: Near\tIndex2: Same\tPairs: 0 (0.00000)
LaneHops: 1\tIndex1: Near\tIndex2: Near\tPairs: 0 (0.00000)
LaneHops: 1\tIndex1: Near\tIndex2: Far\tPairs: 0 (0.00000)
LaneHops: 1\tIndex1: Far\tIndex2: Same\tPairs: 1 (0.14286)
LaneHops: 1\tIndex1: Far\tIndex2: Near\tPairs: 0 (0.00000)
LaneHops: 1\tIndex1: Far\tIndex2: Far\tPairs: 1 (0.14286)
LaneHopsTile: 1\tTile: 1101\tPairs: 1\tSameTile: 1\tHop1: 0\tHop2: 0
LaneHopsTile: 1\tTile: 1102\tPairs: 4\tSameTile: 0\tHop1: 2\tHop2: 0
LaneHopsTile: 1\tTile: 1103\tPairs: 2\tSameTile: 1\tHop1: 0\tHop2: 1
LaneHopLibrary: 1\tIndex: AC+GT\tPF wells: 3\tWithin: 1\tExchanged: 4 (1.333333 of PF)
LaneHopLibrary: 1\tIndex: CA+GT\tPF wells: 3\tWithin: 1\tExchanged: 2 (0.666667 of PF)
LaneHopLibrary: 1\tIndex: Other\tPF wells: 5\tWithin: 0\tExchanged: 4 (0.800000 of PF)
LaneHopPair: 1\tIndex: AC+GT\tIndex: Other\tPairs: 3 (0.60000)\tExpected: 1.92\tRatio: 1.560
LaneHopPair: 1\tIndex: AC+GT\tIndex: CA+GT\tPairs: 1 (0.20000)\tExpected: 1.15\tRatio: 0.867
LaneHopPair: 1\tIndex: CA+GT\tIndex: Other\tPairs: 1 (0.20000)\tExpected: 1.92\tRatio: 0.520
LaneHopsSummary: 1\tSplit: 2\tMaxE: 1\tListed: 2\tPairs: 7\tSame index: 2 (0.28571)\tIndex-read errors only: 2 (0.28571)\t\
One index read swapped: 2 (0.285714 per pair)\tBoth: 1\tInto a listed library: 1\tInto an unlisted combination: 4\tSameTile: 2
"""
HAND_TSV = """lane\tindex_a\tindex_b\tpairs
1\tAC+GT\tAC+GT\t1
1\tAC+GT\tCA+GT\t1
1\tAC+GT\tOther\t3
1\tCA+GT\tCA+GT\t1
1\tCA+GT\tOther\t1
"""


def _hand():
    itiles = [(ti, [np.array([_BYTE[HAND_READS[ti * 4 + w][c]] for w in range(4)], dtype=np.uint8) for c in range(4)])
              for ti in range(3)]
    labels = np.array(HAND_LABELS, dtype=np.uint32)
    return itiles, labels, [key_of(k) for k in HAND_LISTED]


def _hand_counts(n_pairs=10):
    itiles, labels, listed = _hand()
    return report.LaneHopCounts.from_rows(*lane_hops(itiles, labels, 4, 3, 4, 2, 1, listed), listed, HAND_PF, [2, 2],
                                          ["1101", "1102", "1103"], 1, n_pairs=n_pairs)


def test_hand_made_lane():
    itiles, labels, listed = _hand()
    for fn in (lane_hops, lane_hops_literal):
        lane, tile_rows, matrix = fn(itiles, labels, 4, 3, 4, 2, 1, listed)
        assert lane.tolist() == HAND_LANE and tile_rows.tolist() == HAND_TILES and matrix.tolist() == HAND_MATRIX
    # the finish these labels would belong to: 11 PF wells, 3 classes of 8 wells, 7 redundant; LaneRedundant per tile
    check_hop_identities((lane, tile_rows, matrix), [11, 3, 10, 7], [[0, 0, 0, 0, 1], [0, 0, 0, 0, 4], [0, 0, 0, 0, 2]], 4, 2, 1)
    # E = 0: the two errors are other indexes; E = 2: a part of two cycles is never Far
    assert lane_hops(itiles, labels, 4, 3, 4, 2, 0, listed)[0].tolist() == [7, 2, 4, 1, 2, 0, 3, 0, 0, 0, 1, 0, 1]
    assert lane_hops(itiles, labels, 4, 3, 4, 2, 2, listed)[0].tolist() == [7, 2, 0, 0, 2, 3, 0, 1, 1, 0, 0, 0, 0]
    # a single index of four cycles, E = 1
    single = lane_hops(itiles, labels, 4, 3, 4, 4, 1, listed)
    assert single[0].tolist() == [7, 2, 3, 0, 2, 0, 0, 2, 0, 0, 3, 0, 0] and single[2].tolist() == HAND_MATRIX
    assert lane_hops(itiles, labels, 4, 3, 4, 2, 1, [])[2].tolist() == [[7]]
    # the listing the other way round: the ranks follow it
    swapped = lane_hops(itiles, labels, 4, 3, 4, 2, 1, listed[::-1])[2]
    assert swapped.tolist() == [[1, 0, 1], [1, 1, 3], [0, 0, 0]]


def test_hand_made_block_line_by_line():
    c = _hand_counts()
    assert (c.pairs, c.same_tile, c.hop1, c.hop2, c.errors_only, c.off_diagonal) == (7, 2, 2, 1, 2, 5)
    assert c.names == ["AC+GT", "CA+GT", "Other"] and not c.single and c.split == 2
    assert [c.exchanged(a) for a in range(3)] == [4, 2, 4] and c.into_listed() == 1 and c.into_unlisted() == 4
    assert key_of("CAGT") < key_of("ACGT")                             # the tie of the two pairs of one: by the keys
    assert c.top_pairs() == [(0, 2, 3), (0, 1, 1), (1, 2, 1)]
    text = io.StringIO()
    report.write_lane_hops("1", c, verbose=True, out=text)
    assert text.getvalue() == HAND_TEXT
    text = io.StringIO()
    report.write_lane_hops("1", _hand_counts(n_pairs=1), verbose=False, out=text)
    want = [line for line in HAND_TEXT.splitlines() if not line.startswith("LaneHopsTile")]
    assert text.getvalue().splitlines() == want[:14] + want[16:]       # one pair listed, no tile lines
    text = io.StringIO()
    report.write_lane_hops_tsv("1", c, text)
    assert text.getvalue() == HAND_TSV
    text = io.StringIO()
    report.write_lane_hops_tsv("2", c, text, header=False)
    assert text.getvalue() == "".join(line.replace("1\t", "2\t", 1) + "\n" for line in HAND_TSV.splitlines()[1:])


def test_expected_column_as_exact_fractions():
    """H = 5 pairs between libraries, PF shares 3/11, 3/11, 5/11: 1 - sum p^2 = 78/121."""
    c = _hand_counts()
    assert c.expected(0, 1) == Fraction(5 * 2 * 3 * 3, 121 - 43) == Fraction(15, 13)
    assert c.expected(0, 2) == c.expected(1, 2) == Fraction(25, 13)
    assert c.expected(0, 1) + c.expected(0, 2) + c.expected(1, 2) == c.off_diagonal      # they share out H
    one = report.LaneHopCounts.from_rows([4, 4, 0, 0, 4] + [0] * 8, [[4, 4, 0, 0]], [[0, 0], [0, 4]], [key_of("ACGT")], [0, 9], [4],
                                         ["1101"], 0)
    assert one.expected(0, 1) is None                                  # every PF well in one library: nothing to exchange


def test_report_for_a_single_index_and_for_no_pairs():
    itiles, labels, listed = _hand()
    c = report.LaneHopCounts.from_rows(*lane_hops(itiles, labels, 4, 3, 4, 4, 1, listed), listed, HAND_PF, [4],
                                       ["1101", "1102", "1103"], 1, k=2)
    text = io.StringIO()
    report.write_lane_hops("3", c, out=text)
    lines = text.getvalue().splitlines()
    assert lines[:4] == ["", "LaneHops: 3\tHamming: 2\tIndex1: Same\tIndex2: -\tPairs: 2 (0.28571)",
                         "LaneHops: 3\tHamming: 2\tIndex1: Near\tIndex2: -\tPairs: 2 (0.28571)",
                         "LaneHops: 3\tHamming: 2\tIndex1: Far\tIndex2: -\tPairs: 3 (0.42857)"]
    assert lines[4] == "LaneHopLibrary: 3\tHamming: 2\tIndex: ACGT\tPF wells: 3\tWithin: 1\tExchanged: 4 (1.333333 of PF)"
    assert lines[-1].startswith("LaneHopsSummary: 3\tHamming: 2\tSplit: single\tMaxE: 1\tListed: 2\tPairs: 7\t")
    assert "\tOne index read swapped: 3 (0.428571 per pair)\tBoth: 0\t" in lines[-1] and len(lines) == 11
    none = report.LaneHopCounts.from_rows([0] * 13, np.zeros((3, 4), dtype=np.int64), [[0]], [], [11], [2, 2],
                                          ["1101", None, "1103"], 1)
    text = io.StringIO()
    report.write_lane_hops("1", none, verbose=True, out=text)
    lines = text.getvalue().splitlines()
    assert len(lines) == 1 + 9 + 2 + 1 + 1 and lines[1] == "LaneHops: 1\tIndex1: Same\tIndex2: Same\tPairs: 0 (0.00000)"
    assert lines[12] == "LaneHopLibrary: 1\tIndex: Other\tPF wells: 11\tWithin: 0\tExchanged: 0 (0.000000 of PF)"
    assert lines[13] == ("LaneHopsSummary: 1\tSplit: 2\tMaxE: 1\tListed: 0\tPairs: 0\tSame index: 0 (0.00000)\t"
                         "Index-read errors only: 0 (0.00000)\tOne index read swapped: 0 (0.000000 per pair)\tBoth: 0\t"
                         "Into a listed library: 0\tInto an unlisted combination: 0\tSameTile: 0")
    text = io.StringIO()
    report.write_lane_hops_tsv("1", none, text)
    assert text.getvalue() == "lane\tindex_a\tindex_b\tpairs\n"


# ---- C ABI --------------------------------------------------------------------------------------
def test_lanehops_header_and_binding_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert '#include "welldup_laneindex.h"' in text
    syms = sorted(set(re.findall(r"\b(wd_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.LANEHOPS_PROTOTYPES) == ["wd_lane_hops", "wd_lane_hops_scratch"]
    assert int(re.search(r"#define WD_LANEHOPS_MAX_E\s+(\d+)", text).group(1)) == _lib.LANEHOPS_MAX_E == MAX_E == report.LANE_HOPS_MAX_E
    assert int(re.search(r"#define WD_LANEHOPS_TILE_COLS\s+(\d+)", text).group(1)) == _lib.LANEHOPS_TILE_COLS == TILE_COLS
    assert int(re.search(r"#define WD_LANEHOPS_STATES\s+(\d+)", text).group(1)) == _lib.LANEHOPS_STATES == 9
    assert int(re.search(r"#define WD_LANEHOPS_MAX_LISTED\s+(\d+)", text).group(1)) == _lib.LANEHOPS_MAX_LISTED == MAX_LISTED
    assert _lib.LANEHOPS_LANE_COLS == LANE_COLS == report.LANE_HOPS_LANE_COLS == 13
    assert report.LANE_HOPS_TILE_COLS == TILE_COLS and report.LANE_HOPS_MAX_LISTED == MAX_LISTED
    assert not set(_lib.LANEHOPS_PROTOTYPES) & set(_lib.PROTOTYPES)
    source = open(os.path.join(_lib.CSRC, "lane_hops.inc")).read()
    assert "k_lh_tally" in source and _lib.unit_of_kernel("k_lh_tally") == "tiledups"
    assert "binary search" in source and "does not depend on the order of execution" in source
    deps = {os.path.basename(f) for f in _lib._deps(os.path.join(_lib.CSRC, "welldup_tiledups.hip"))}
    assert {"lane_hops.inc", "welldup_lanehops.h", "lane_index.inc", "lane_pass.inc"} <= deps
    unit = open(os.path.join(_lib.CSRC, "welldup_tiledups.hip")).read()
    assert unit.index('#include "lane_index.inc"') < unit.index('#include "lane_hops.inc"')
    assert "k_lh_tally (lane_hops.inc)" in open(os.path.join(_lib.CSRC, "lane_mismatch.inc")).read()
    assert "lane_hops_emu.cpp" in open(os.path.join(_lib.REPO, "tools", "wave_emu.h")).read()
    _lib.build()
    lib = _lib.load()
    for s in syms:                                                     # exported, and bound as the table says
        assert getattr(lib, s).argtypes == _lib.LANEHOPS_PROTOTYPES[s][1]
    ids = _lib.build_ids()
    assert ids["tiledups"] == _lib.source_unit_ids()["tiledups"] and ids["all"] == _lib.source_build_id()


def _formula(tiles, M):
    """The arithmetic include/welldup_lanehops.h states."""
    up = lambda v: (v + 255) // 256 * 256
    return up(2048 * tiles) + 8192 + up(4 * tiles) + up(8 * M) + up(2 * M) + up(8 * (M + 1) * (M + 1))


def _scratch(lib, tiles, M):
    b = ctypes.c_size_t()
    rc = lib.wd_lane_hops_scratch(tiles, M, ctypes.byref(b))
    return rc, b.value


def test_scratch_size_needs_no_gpu_and_matches_the_header():
    _lib.build()
    lib = _lib.load()
    text = open(HEADER).read()
    for piece in ("2048 * max_tiles", "+ 8192", "+ 4 * max_tiles", "+ 8 * M", "+ 2 * M", "+ 8 * (M + 1) * (M + 1)",
                  "rounded up to 256 bytes", "8.4 MB and 2 KB per tile"):
        assert piece in text, piece
    for tiles in (0, 1, 3, 7, 64, 65, 112, 65535):
        for M in (0, 1, 3, 31, 32, 96, 1023, 1024):
            assert _scratch(lib, tiles, M) == (0, _formula(tiles, M)), (tiles, M)
    assert 8.4e6 < _formula(0, 1024) < 8.5e6 and _formula(112, 1024) - _formula(0, 1024) == 112 * 2048 + 512
    assert _scratch(lib, 65536, 10)[0] == _lib.ERR_UNSUPPORTED
    for tiles, M in ((-1, 10), (3, -1), (3, 1025)):
        assert _scratch(lib, tiles, M)[0] == _lib.ERR_ARG
    assert lib.wd_lane_hops_scratch(3, 10, None) == _lib.ERR_ARG
    row = (ctypes.c_int64 * 32)()                                      # a null handle is refused before anything is looked at
    assert lib.wd_lane_hops(None, 1, 1, 0, None, None, 0, row, row, row) == _lib.ERR_ARG


def test_fit_check_counts_the_scratch():
    cwd.check_lane_dups_fits(1000, 1000 + 8_500_000, 4, 100, 10, hops=8_500_000)
    with pytest.raises(MemoryError) as e:
        cwd.check_lane_dups_fits(1000, 1000 + 8_499_999, 4, 100, 10, index=500, hops=8_500_000)
    assert "8500000 of them for --lane-dups-hops" in str(e.value) and "500 of them for --lane-dups-index" in str(e.value)


# ---- CLI ----------------------------------------------------------------------------------------
def test_cli_flag_checks(tmp_path, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["-s", "hiseq_4000", "-r", str(tmp_path), "--all-wells"]
    index = ["--lane-dups", "--lane-dups-index", "151-159,159-167"]
    args = cwd.parse_args(base + index + ["--lane-dups-hops"])
    assert args.lane_dups_hops == 10 and args.lane_dups_hops_mismatches is None and args.lane_dups_hops_out is None
    assert cwd.parse_args(base + index + ["--lane-dups-hops", "25"]).lane_dups_hops == 25
    assert cwd.parse_args(base + index + ["--lane-dups-hops", "0"]).lane_dups_hops == 0
    assert cwd.parse_args(base + index).lane_dups_hops is None
    for e in (0, 3):
        assert cwd.parse_args(base + index + ["--lane-dups-hops", "--lane-dups-hops-mismatches", str(e)]).lane_dups_hops_mismatches == e
    assert cwd.parse_args(base + index + ["--lane-dups-hops", "--lane-dups-hops-out", "x.tsv"]).lane_dups_hops_out == "x.tsv"
    for extra, message in ((["--lane-dups", "--lane-dups-hops"], "--lane-dups-hops needs --lane-dups-index"),
                           (["--lane-dups-hops", "5"], "--lane-dups-hops needs --lane-dups-index"),
                           (index + ["--lane-dups-hops", "-1"], "--lane-dups-hops takes the number of library pairs to list, not -1"),
                           (index + ["--lane-dups-hops-mismatches", "1"], "--lane-dups-hops-mismatches needs --lane-dups-hops"),
                           (index + ["--lane-dups-hops", "--lane-dups-hops-mismatches", "4"],
                            "--lane-dups-hops-mismatches takes 0..3, not 4"),
                           (index + ["--lane-dups-hops", "--lane-dups-hops-mismatches", "-1"],
                            "--lane-dups-hops-mismatches takes 0..3, not -1"),
                           (index + ["--lane-dups-hops-out", "x.tsv"], "--lane-dups-hops-out needs --lane-dups-hops"),
                           (["--lane-dups-index", "151-159", "--lane-dups-hops"], "--lane-dups-index needs --lane-dups")):
        with pytest.raises(SystemExit):
            cwd.parse_args(base + extra)
        assert message in " ".join(capsys.readouterr().err.split())


def test_cli_help_names_the_new_options(capsys):
    with pytest.raises(SystemExit):
        cwd.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--lane-dups-hops [N]" in text and "--lane-dups-hops-mismatches E" in text and "--lane-dups-hops-out FILE" in text
    assert "an index combination nobody used" in text
