"""A lane's errors against its families' vote without a GPU: the header against the binding, the scratch formula and
its error codes, the parser's refusals, the fit check, the reference on hand-worked lanes with every figure worked out
by hand, the identities, and the report block and the TSV."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from laneconsensus_ref import (DIST, LANE_COLS, MAX_D, MAX_FAMILY, TILE_COLS, check_consensus_identities, families_of,
                               lane_consensus, vote)
from tiledups_ref import INVALID
from well_duplicates_amd import _lib, report
from well_duplicates_amd import count_well_duplicates as cwd

HEADER = os.path.join(_lib.INCLUDE, "welldup_laneconsensus.h")
BYTE = {"A": 0x40, "C": 0x81, "G": 0xC2, "T": 0x23, "N": 0x00}


# ---- C ABI --------------------------------------------------------------------------------------
def test_laneconsensus_header_and_binding_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(wd_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.LANECONSENSUS_PROTOTYPES) == ["wd_lane_consensus", "wd_lane_consensus_scratch"]
    define = lambda name: int(re.search(r"#define WD_LANECONSENSUS_%s\s+(.+)" % name, text).group(1).strip())
    assert define("MAX_D") == _lib.LANECONSENSUS_MAX_D == MAX_D == report.LANE_CONSENSUS_MAX_D
    assert define("MAX_FAMILY") == _lib.LANECONSENSUS_MAX_FAMILY == MAX_FAMILY == report.LANE_CONSENSUS_MAX_FAMILY
    assert define("LANE_COLS") == _lib.LANECONSENSUS_LANE_COLS == LANE_COLS == report.LANE_CONSENSUS_LANE_COLS
    assert define("TILE_COLS") == _lib.LANECONSENSUS_TILE_COLS == TILE_COLS == report.LANE_CONSENSUS_TILE_COLS
    assert define("DIST_BINS") == _lib.LANECONSENSUS_DIST_BINS == len(report.LANE_CONSENSUS_DIST_NAMES)
    source = open(os.path.join(_lib.CSRC, "lane_consensus.inc")).read()
    for kernel in ("k_lc_reserve", "k_lc_scatter", "k_lc_vote"):
        assert kernel in source and _lib.unit_of_kernel(kernel) == "tiledups"
        assert kernel in open(os.path.join(_lib.CSRC, "lane_mismatch.inc")).read()         # listed among the readers
    assert "asm" not in source                                         # plain C++ and vector atomics only
    deps = {os.path.basename(f) for f in _lib._deps(os.path.join(_lib.CSRC, "welldup_tiledups.hip"))}
    assert {"lane_consensus.inc", "welldup_laneconsensus.h"} <= deps
    _lib.build()
    lib = _lib.load()
    for s in syms:                                                     # exported, and bound as the table says
        assert getattr(lib, s).argtypes == _lib.LANECONSENSUS_PROTOTYPES[s][1]


def _scratch(lib, tiles, wells, cycles):
    b = ctypes.c_size_t()
    rc = lib.wd_lane_consensus_scratch(tiles, wells, cycles, ctypes.byref(b))
    return rc, b.value


def test_scratch_size_needs_no_gpu_and_matches_the_header():
    _lib.build()
    lib = _lib.load()
    text = open(HEADER).read()
    for piece in ("2048 * max_tiles", "+ 8192", "+ 256 ", "+ 4 * max_tiles", "+ 200 * L", "+ 4 * W", "rounded up to 256 bytes",
                  "8 bytes per well of the lane"):
        assert piece in text, piece
    up = lambda v: (v + 255) // 256 * 256
    for tiles in (0, 1, 7, 112, 65535):
        for wells in (0, 1, 2640, 8449):
            for cycles in (0, 1, 37, 151, 1024):
                w = tiles * wells
                want = 2048 * tiles + 8192 + 256 + up(4 * tiles) + up(200 * cycles) + 2 * up(4 * w)
                assert _scratch(lib, tiles, wells, cycles) == (0, want)
                assert want <= 8 * w + 2048 * tiles + 200 * cycles + 4 * tiles + 8192 + 256 + 4 * 256      # 8 bytes per well, and counters
    rc, nbytes = _scratch(lib, 112, 4300000, 151)                       # the header's lane
    assert rc == 0 and 3.85e9 < nbytes < 3.86e9
    assert _scratch(lib, 65536, 10, 10)[0] == _lib.ERR_UNSUPPORTED and _scratch(lib, 3, 10, 1025)[0] == _lib.ERR_UNSUPPORTED
    assert _scratch(lib, 1024, 1 << 22, 10)[0] == _lib.ERR_UNSUPPORTED   # 2^32 wells: a global id no longer fits a label
    assert _scratch(lib, -1, 10, 10)[0] == _lib.ERR_ARG and _scratch(lib, 3, -1, 10)[0] == _lib.ERR_ARG
    assert _scratch(lib, 3, 10, -1)[0] == _lib.ERR_ARG and lib.wd_lane_consensus_scratch(3, 10, 10, None) == _lib.ERR_ARG
    row = (ctypes.c_int64 * 64)()                                      # a null handle is refused before anything is looked at
    assert lib.wd_lane_consensus(None, 0, 256, None, 0, row, row, row) == _lib.ERR_ARG


# ---- CLI ----------------------------------------------------------------------------------------
def test_cli_flag_checks(tmp_path, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["-s", "hiseq_4000", "-r", str(tmp_path), "--all-wells"]
    args = cwd.parse_args(base + ["--lane-dups", "--lane-dups-consensus"])
    assert args.lane_dups_consensus
    assert (args.lane_dups_consensus_max_d, args.lane_dups_consensus_max_family, args.lane_dups_consensus_out) == (None,) * 3
    assert not cwd.parse_args(base + ["--lane-dups"]).lane_dups_consensus
    args = cwd.parse_args(base + ["--lane-dups", "--lane-dups-hamming", "2", "--lane-dups-consensus",
                                  "--lane-dups-consensus-max-d", "7", "--lane-dups-consensus-max-family", "4096",
                                  "--lane-dups-consensus-out", "c.tsv"])
    assert (args.lane_dups_consensus_max_d, args.lane_dups_consensus_max_family, args.lane_dups_consensus_out) == (7, 4096, "c.tsv")
    args = cwd.parse_args(base + ["--lane-dups", "--lane-dups-consensus", "--lane-dups-consensus-max-d", "0",
                                  "--lane-dups-consensus-max-family", "3"])
    assert (args.lane_dups_consensus_max_d, args.lane_dups_consensus_max_family) == (0, 3)
    on = ["--lane-dups", "--lane-dups-consensus"]
    for extra, message in ((["--lane-dups-consensus"], "--lane-dups-consensus needs --lane-dups"),
                           (["--tile-dups", "--lane-dups-consensus"], "--lane-dups-consensus needs --lane-dups"),
                           (["--lane-dups", "--lane-dups-consensus-max-d", "0"],
                            "--lane-dups-consensus-max-d needs --lane-dups-consensus"),
                           (["--lane-dups", "--lane-dups-consensus-max-family", "10"],
                            "--lane-dups-consensus-max-family needs --lane-dups-consensus"),
                           (["--lane-dups", "--lane-dups-consensus-out", "x.tsv"],
                            "--lane-dups-consensus-out needs --lane-dups-consensus"),
                           (on + ["--lane-dups-consensus-max-d", "8"], "--lane-dups-consensus-max-d takes 0..7, not 8"),
                           (on + ["--lane-dups-consensus-max-d", "-1"], "--lane-dups-consensus-max-d takes 0..7, not -1"),
                           (on + ["--lane-dups-consensus-max-family", "2"],
                            "--lane-dups-consensus-max-family takes 3..4096, not 2"),
                           (on + ["--lane-dups-consensus-max-family", "4097"],
                            "--lane-dups-consensus-max-family takes 3..4096, not 4097")):
        with pytest.raises(SystemExit):
            cwd.parse_args(base + extra)
        assert message in " ".join(capsys.readouterr().err.split())
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cwd.parse_args(base + on)
    assert "--lane-dups runs in a single process only" in " ".join(capsys.readouterr().err.split())


def test_cli_help_and_docstring_name_the_new_options(capsys):
    with pytest.raises(SystemExit):
        cwd.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for piece in ("--lane-dups-consensus", "--lane-dups-consensus-max-d D", "--lane-dups-consensus-max-family M",
                  "--lane-dups-consensus-out FILE", "3..4096, default 256",
                  "Without --lane-dups-hamming every copy is identical: no well disagrees"):
        assert piece in text, piece
    for flag in ("--lane-dups-consensus,", "--lane-dups-consensus-max-d", "--lane-dups-consensus-max-family",
                 "--lane-dups-consensus-out", "report.write_lane_consensus"):
        assert flag in cwd.__doc__, flag


def test_the_consensus_scratch_counts_when_a_lane_is_fitted():
    cwd.check_lane_dups_fits(1000, 2000, 2, 3, 4, scratch=500, gc=200, consensus=300)
    with pytest.raises(MemoryError) as e:
        cwd.check_lane_dups_fits(1000, 2000, 2, 3, 4, scratch=500, gc=200, consensus=301)
    assert ("(2001 bytes, 500 of them for --lane-dups-hamming, 200 of them for --lane-dups-gc, 301 of them for "
            "--lane-dups-consensus), and 0.00 GB (2000 bytes) are free") in str(e.value)
    with pytest.raises(MemoryError) as e:
        cwd.check_lane_dups_fits(1000, 999, 2, 3, 4)
    assert "(1000 bytes), and" in str(e.value) and "consensus" not in str(e.value)


# ---- the reference on hand-worked lanes -----------------------------------------------------------
def hand_made_lane():
    """Two tiles of 8 wells (indices 0 and 1 of 2), 4 cycles; global id = 8 x tile + well.  Well 8 fails the filter.
      family A, root 0: wells 0, 1, 9 read ACGT, ACGT, ACTT - the vote is ACGT, well 9 calls T for G at cycle 2;
      family B, root 2: wells 2, 3, 10, 11 read AAAA, AAAA, CAAA, CAAN - cycle 0 is 2 against 2 and undecided, at
                        cycle 3 three of four say A and well 11 calls N for A;
      family C, root 4: wells 4 and 12, a pair;
      family D, root 5: wells 5, 6, 7, 13, 14 read TGGG, GGGG, GGGG, GGGG, GGGG - the FIRST well calls T for G;
      well 15 is single.
    -> (tiles, labels): the labels are the clusters a finish at K = 1 would leave, written down."""
    reads = {0: "ACGT", 1: "ACGT", 9: "ACTT", 2: "AAAA", 3: "AAAA", 10: "CAAA", 11: "CAAN", 4: "CCCC", 12: "CCCC",
             5: "TGGG", 6: "GGGG", 7: "GGGG", 13: "GGGG", 14: "GGGG", 15: "TTTT", 8: "ACAC"}
    root = {0: 0, 1: 0, 9: 0, 2: 2, 3: 2, 10: 2, 11: 2, 4: 4, 12: 4, 5: 5, 6: 5, 7: 5, 13: 5, 14: 5, 15: 15}
    tiles = []
    for t in range(2):
        planes = [np.array([BYTE[reads[8 * t + w][c]] for w in range(8)], dtype=np.uint8) for c in range(4)]
        filt = np.array([0 if 8 * t + w == 8 else 1 for w in range(8)], dtype=np.uint8)
        tiles.append((t, planes, filt))
    labels = np.full((2, 8), INVALID, dtype=np.uint32)
    for g, r in root.items():
        labels[g // 8, g % 8] = r
    return tiles, labels


def _cells(calls):
    return {(c, "ACGTN"[a], "ACGTN"[b]): int(calls[c, a, b]) for c, a, b in np.argwhere(calls)}


def test_reference_on_a_hand_worked_lane():
    tiles, labels = hand_made_lane()
    assert [(r, m.tolist()) for r, m in families_of(labels)] == [(0, [0, 1, 9]), (2, [2, 3, 10, 11]), (4, [4, 12]),
                                                                 (5, [5, 6, 7, 13, 14])]
    lane, trow, calls = lane_consensus(tiles, 8, 2, labels, 1, 256)
    #                      Fam Wells Prof Mis WithN Und UndCalls FirstOff Pairs Large LargeWells Dist
    assert lane.tolist() == [3, 12, 12, 3, 1, 1, 4, 1, 1, 0, 0] + [9, 3, 0, 0, 0, 0, 0, 0, 0]
    assert trow.tolist() == [[7, 7, 1, 0], [5, 5, 2, 1]]
    assert _cells(calls) == {(0, "A", "A"): 3, (0, "G", "G"): 4, (0, "G", "T"): 1,
                             (1, "C", "C"): 3, (1, "A", "A"): 4, (1, "G", "G"): 5,
                             (2, "G", "G"): 2 + 5, (2, "G", "T"): 1, (2, "A", "A"): 4,
                             (3, "T", "T"): 3, (3, "A", "A"): 3, (3, "A", "N"): 1, (3, "G", "G"): 5}
    assert calls.sum() == 12 * 4 - 4
    check_consensus_identities(lane, trow, calls, 1, finish_lane=[15, 4, 14, 10])
    # max_d = 0: the three wells that err are counted by distance and kept out of calls; B's undecided cycle now weighs 3
    lane0, trow0, calls0 = lane_consensus(tiles, 8, 2, labels, 0, 256)
    assert lane0.tolist() == [3, 12, 9, 0, 0, 1, 3, 1, 1, 0, 0] + [9, 3, 0, 0, 0, 0, 0, 0, 0]
    assert trow0.tolist() == [[7, 6, 0, 0], [5, 3, 0, 0]] and calls0.sum() == 9 * 4 - 3
    assert _cells(calls0)[(2, "G", "G")] == 2 + 4 and (0, "G", "T") not in _cells(calls0)
    check_consensus_identities(lane0, trow0, calls0, 0, finish_lane=[15, 4, 14, 10], wider=None)
    check_consensus_identities(lane, trow, calls, 1, lower=(lane0, trow0, calls0))
    # max_family = 4: D is large, and with it the first well that was off
    lane4, trow4, calls4 = lane_consensus(tiles, 8, 2, labels, 1, 4)
    assert lane4.tolist() == [2, 7, 7, 2, 1, 1, 4, 0, 1, 1, 5] + [5, 2, 0, 0, 0, 0, 0, 0, 0]
    check_consensus_identities(lane4, trow4, calls4, 1, finish_lane=[15, 4, 14, 10], wider=(lane, trow, calls))
    lane3, _, calls3 = lane_consensus(tiles, 8, 2, labels, 1, 3)
    assert lane3[:2].tolist() == [1, 3] and lane3[9:11].tolist() == [2, 9] and calls3.sum() == 12


def test_the_vote_needs_strictly_more_than_half():
    code = lambda reads: np.array([["ACGTN".index(b) for b in r] for r in reads], dtype=np.uint8).T
    cons, decided = vote(code(["AC", "AG", "CT"]))                      # three codes in three wells at the second cycle
    assert decided.tolist() == [True, False] and cons[0] == 0
    cons, decided = vote(code(["A", "A", "C", "C", "G"]))               # 2 / 2 / 1
    assert decided.tolist() == [False]
    cons, decided = vote(code(["N", "N", "A"]))                         # N votes like a base
    assert decided.tolist() == [True] and cons[0] == 4
    cons, decided = vote(code(["T", "T", "T", "A", "C"]))               # 3 of 5
    assert decided.tolist() == [True] and cons[0] == 3


def test_under_equality_labels_nothing_disagrees():
    tiles, labels = hand_made_lane()
    planes = [np.array([BYTE["ACGT"[(w // 3 + c) % 4]] for w in range(8)], dtype=np.uint8) for c in range(4)]
    tiles = [(1, planes, np.ones(8, dtype=np.uint8))]                   # wells 0-2, 3-5 equal, 6-7 a pair; tile index 1 of 2
    labels = np.full((2, 8), INVALID, dtype=np.uint32)
    labels[1] = [8, 8, 8, 11, 11, 11, 14, 14]
    lane, trow, calls = lane_consensus(tiles, 8, 2, labels, 0, 256)
    assert lane.tolist() == [2, 6, 6, 0, 0, 0, 0, 0, 1, 0, 0] + [6] + [0] * 8 and not trow[0].any()
    check_consensus_identities(lane, trow, calls, 0, finish_lane=[8, 3, 8, 5], equality=True)
    with pytest.raises(AssertionError):
        bad = calls.copy()
        bad[0, 0, 1] += 1
        check_consensus_identities(lane, trow, bad, 0, equality=True)


# ---- the report ---------------------------------------------------------------------------------
def _counts(max_d=1):
    tiles, labels = hand_made_lane()
    return report.LaneConsensusCounts.from_rows(*lane_consensus(tiles, 8, 2, labels, max_d, 256), ["1101", "1102"], 1, max_d,
                                                256, 15, [10, 11, 12, 13])


def _text(counts, verbose=True):
    out = io.StringIO()
    report.write_lane_consensus("1", counts, verbose=verbose, out=out)
    return out.getvalue()


def test_write_lane_consensus_lines():
    lines = _text(_counts()).split("\n")
    assert lines[0] == "" and lines[-1] == "" and len(lines) == 1 + 2 + 4 + 1 + 1 + 12 + 1 + 1
    assert lines[1] == "LaneConsensus: 1\tTile: 1101\tWells: 7\tProfiled: 7\tMismatches: 1\tWithN: 0"
    assert lines[2] == "LaneConsensus: 1\tTile: 1102\tWells: 5\tProfiled: 5\tMismatches: 2\tWithN: 1"
    assert lines[3] == "LaneConsensus: 1\tCycle: 10\tCalls: 8\tErrors: 1\tRate: 1.250e-01\tMost frequent: G>T (1)"
    assert lines[4] == "LaneConsensus: 1\tCycle: 11\tCalls: 12\tErrors: 0\tRate: 0.000e+00\tMost frequent: -"
    assert lines[6] == "LaneConsensus: 1\tCycle: 13\tCalls: 12\tErrors: 1\tRate: 8.333e-02\tMost frequent: A>N (1)"
    assert lines[7] == ("LaneConsensusSummary: 1\tTiles: 2\tHamming: 1\tMaxD: 1\tMaxFamily: 256\tFamilies: 3\t"
                        "Wells: 12 (0.80000 of PF)\tProfiled: 12 (1.00000)\tMismatches: 3\tWithN: 1\t"
                        "Errors per called base: 6.818e-02 (Q 11.7)\tUndecided: 1\tFirstWellOff: 1 (0.33333 of Families)\t"
                        "Pairs left out: 1\tLarge left out: 0 (0 wells)")
    assert lines[8] == "ConsensusDist: 0: 9 (0.75000)\t1: 3 (0.25000)\t" + "\t".join(
        "%s: 0 (0.00000)" % n for n in ("2", "3", "4", "5", "6", "7", ">=8"))
    table = lines[9:21]
    assert [l.split("\t")[0] for l in table] == ["Consensus: %s>%s" % (a, b) for a in "ACGT" for b in "ACGT" if a != b]
    # the direction: G>T twice among 23 calls of a G molecule, T>G never among 3 calls of a T molecule
    assert table[8] == "Consensus: G>T\t2 (0.66667 of Mismatches)\tRate: 8.696e-02\tReverse T>G: 0\tRatio: inf"
    assert table[11] == "Consensus: T>G\t0 (0.00000 of Mismatches)\tRate: 0.000e+00\tReverse G>T: 2\tRatio: 0.000"
    assert table[0] == "Consensus: A>C\t0 (0.00000 of Mismatches)\tRate: 0.000e+00\tReverse C>A: 0\tRatio: n/a"
    assert lines[21] == "Consensus: N\tmolecule>N: 1\tN>call: 0\t(0.33333 of Mismatches)"
    short = _text(_counts(), verbose=False).split("\n")
    assert short == [""] + lines[7:]                                    # -S: the summary lines alone


def test_write_lane_consensus_of_an_empty_lane():
    empty = report.LaneConsensusCounts.from_rows([0] * 20, [[0] * 4], np.zeros((3, 5, 5), dtype=np.int64), ["1101"], 0, 0, 256, 0)
    lines = _text(empty).split("\n")
    assert lines[4].startswith("LaneConsensus: 1\tCycle: 2\tCalls: 0\tErrors: 0\tRate: n/a\tMost frequent: -")
    assert "Errors per called base: n/a (Q -)" in lines[5] and "FirstWellOff: 0 (0.00000 of Families)" in lines[5]
    assert lines[7].endswith("Rate: n/a\tReverse C>A: 0\tRatio: n/a")


def test_write_lane_consensus_tsv():
    out = io.StringIO()
    report.write_lane_consensus_tsv("1", _counts(), out)
    lines = out.getvalue().split("\n")
    assert lines[0] == "lane\tcycle\tconsensus\tcall\tcount" and lines[-1] == "" and len(lines) == 1 + 13 + 1
    assert lines[1:4] == ["1\t10\tA\tA\t3", "1\t10\tG\tG\t4", "1\t10\tG\tT\t1"]
    assert "1\t13\tA\tN\t1" in lines and sum(int(l.split("\t")[4]) for l in lines[1:-1]) == 44
    out = io.StringIO()
    report.write_lane_consensus_tsv("2", _counts(), out, header=False)
    assert out.getvalue().split("\n")[0] == "2\t10\tA\tA\t3"
