"""A lane's most frequent reads and their spread without a GPU: the header against the binding, the scratch formula,
the parser's refusals, the fit check, the report block and the reference on a hand-worked lane."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from lanetop_ref import EDGES, HEAD_COLS, LEVELS, MAX_PASSES, MAX_TOP, check_top_identities, decode, lane_top, level_of
from tiledups_ref import INVALID
from well_duplicates_amd import _lib, report
from well_duplicates_amd import count_well_duplicates as cwd

HEADER = os.path.join(_lib.INCLUDE, "welldup_lanetop.h")


# ---- C ABI --------------------------------------------------------------------------------------
def test_lanetop_header_and_binding_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert '#include "welldup_lanesaturation.h"' in text
    syms = sorted(set(re.findall(r"\b(wd_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.LANETOP_PROTOTYPES) == ["wd_lane_top", "wd_lane_top_scratch"]
    define = lambda name: re.search(r"#define WD_LANETOP_%s\s+(.+)" % name, text).group(1).strip()
    assert int(define("MAX")) == _lib.LANETOP_MAX == MAX_TOP == report.LANE_TOP_MAX
    assert int(define("LEVELS")) == _lib.LANETOP_LEVELS == LEVELS == len(EDGES)
    assert int(define("HEAD_COLS")) == _lib.LANETOP_HEAD_COLS == HEAD_COLS
    assert int(define("MAX_PASSES")) == _lib.LANETOP_MAX_PASSES == MAX_PASSES
    assert int(define("DEFAULT_CAPACITY")) == _lib.LANETOP_DEFAULT_CAPACITY == 65536
    edges = tuple(int(v) for v in define("EDGES").strip("{}").split(","))
    assert edges == _lib.LANETOP_EDGES == EDGES == report.LANE_TOP_EDGES
    taken = set()
    for table in (_lib.PROTOTYPES, _lib.SETS_PROTOTYPES, _lib.TILEDUPS_PROTOTYPES, _lib.TILENEAR_PROTOTYPES,
                  _lib.LANEDUPS_PROTOTYPES, _lib.LANENEAR_PROTOTYPES, _lib.LANEINDEX_PROTOTYPES, _lib.LANEMISMATCH_PROTOTYPES,
                  _lib.LANEDISTANCE_PROTOTYPES, _lib.LANEQUALITY_PROTOTYPES, _lib.LANESATURATION_PROTOTYPES):
        taken |= set(table)
    assert not set(_lib.LANETOP_PROTOTYPES) & taken
    source = open(os.path.join(_lib.CSRC, "lane_top.inc")).read()
    for kernel in ("k_lt_hist", "k_lt_collect", "k_lt_spread", "k_lt_rows"):
        assert kernel in source and _lib.unit_of_kernel(kernel) == "tiledups"
    assert "asm" not in source                                         # plain C++ and vector atomics only
    assert "kLaneTopMaxPasses, \"the bound on the passes\"" in source  # the bound is derived from the bin counts
    deps = {os.path.basename(f) for f in _lib._deps(os.path.join(_lib.CSRC, "welldup_tiledups.hip"))}
    assert {"lane_top.inc", "welldup_lanetop.h", "lane_saturation.inc", "welldup_lanesaturation.h"} <= deps
    sat = open(os.path.join(_lib.CSRC, "lane_saturation.inc")).read()  # included at the end of the file before it
    assert sat.rstrip().splitlines()[-2:] == ['#include "lane_top.inc"', "#endif"]
    assert "tiledups" in _lib.UNITS and "lanetop" not in _lib.UNITS and len(_lib.UNITS) == 8
    _lib.build()
    lib = _lib.load()
    for s in syms:                                                     # exported, and bound as the table says
        assert getattr(lib, s).argtypes == _lib.LANETOP_PROTOTYPES[s][1]
    ids = _lib.build_ids()
    assert ids["tiledups"] == _lib.source_unit_ids()["tiledups"] and ids["all"] == _lib.source_build_id()


def _formula(tiles, cycles, n_top, cap):
    """The arithmetic include/welldup_lanetop.h states."""
    up = lambda v: (v + 255) // 256 * 256
    c = cap if cap else max(65536, n_top)
    return (up(64 * 2082 * 8) + up(8 * c) + 256 + 16384 + up(4 * n_top) + up(4 * n_top * tiles) + up(4 * n_top) +
            up(4 * n_top * ((cycles + 9) // 10)) + up(4 * tiles))


def _scratch(lib, n, tiles, cycles, n_top, cap):
    b = ctypes.c_size_t()
    rc = lib.wd_lane_top_scratch(n, tiles, cycles, n_top, cap, ctypes.byref(b))
    return rc, b.value


def test_scratch_size_needs_no_gpu_and_matches_the_header():
    _lib.build()
    lib = _lib.load()
    text = open(HEADER).read()
    for piece in ("1 065 984", "+ 8 * C", "+ 256", "+ 16384", "+ 4 * n_top * max_tiles", "+ 4 * n_top * ceil(L / 10)",
                  "+ 4 * max_tiles", "rounded up to 256 bytes", "1 659 648 bytes"):
        assert piece in text, piece
    for n in (0, 2640, 4309650):
        for tiles in (0, 1, 7, 64, 65, 112, 4096):
            for cycles in (0, 1, 10, 37, 151, 1024):
                for n_top, cap in ((1, 0), (1, 1), (5, 9), (100, 0), (100, 100), (1024, 0), (1024, 1024), (1024, 1 << 20)):
                    assert _scratch(lib, n, tiles, cycles, n_top, cap) == (0, _formula(tiles, cycles, n_top, cap))
    assert _scratch(lib, 4309650, 112, 151, 100, 0) == (0, 1659648)    # the header's HiSeq 4000 lane
    assert _scratch(lib, 10, 65535, 10, 1, 0)[0] == 0 and _scratch(lib, 10, 65536, 10, 1, 0)[0] == _lib.ERR_UNSUPPORTED
    assert _scratch(lib, 10, 3, 1025, 1, 0)[0] == _lib.ERR_UNSUPPORTED
    for bad in ((-1, 3, 10, 1, 0), (10, -1, 10, 1, 0), (10, 3, -1, 1, 0), (10, 3, 10, 0, 0), (10, 3, 10, 1025, 0),
                (10, 3, 10, 5, -1), (10, 3, 10, 5, 4)):
        assert _scratch(lib, *bad)[0] == _lib.ERR_ARG, bad
    assert lib.wd_lane_top_scratch(10, 3, 10, 1, 0, None) == _lib.ERR_ARG
    row = (ctypes.c_int64 * 64)()                                      # a null handle is refused before anything is looked at
    assert lib.wd_lane_top(None, 5, 0, None, 0, row, row, row, row, row, row, row) == _lib.ERR_ARG


# ---- CLI ----------------------------------------------------------------------------------------
def test_cli_flag_checks(tmp_path, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["-s", "hiseq_4000", "-r", str(tmp_path), "--all-wells"]
    args = cwd.parse_args(base + ["--lane-dups", "--lane-dups-top", "100"])
    assert args.lane_dups_top == 100 and args.lane_dups_top_out is None
    assert cwd.parse_args(base + ["--lane-dups"]).lane_dups_top is None
    args = cwd.parse_args(base + ["--lane-dups", "--lane-dups-hamming", "2", "--lane-dups-top", "1024", "--lane-dups-top-out", "x.tsv"])
    assert (args.lane_dups_top, args.lane_dups_top_out) == (1024, "x.tsv")
    assert cwd.parse_args(base + ["--lane-dups", "--lane-dups-top", "1"]).lane_dups_top == 1
    for extra, message in ((["--lane-dups-top", "5"], "--lane-dups-top needs --lane-dups"),
                           (["--tile-dups", "--lane-dups-top", "5"], "--lane-dups-top needs --lane-dups"),
                           (["--lane-dups", "--lane-dups-top-out", "x.tsv"], "--lane-dups-top-out needs --lane-dups-top"),
                           (["--lane-dups", "--lane-dups-top", "0"], "--lane-dups-top takes 1..1024, not 0"),
                           (["--lane-dups", "--lane-dups-top", "1025"], "--lane-dups-top takes 1..1024, not 1025")):
        with pytest.raises(SystemExit):
            cwd.parse_args(base + extra)
        assert message in " ".join(capsys.readouterr().err.split())
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cwd.parse_args(base + ["--lane-dups", "--lane-dups-top", "5"])
    assert "--lane-dups runs in a single process only" in " ".join(capsys.readouterr().err.split())


def test_cli_help_and_docstring_name_the_new_options(capsys):
    with pytest.raises(SystemExit):
        cwd.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for piece in ("--lane-dups-top N", "--lane-dups-top-out FILE", "(1..1024)", "duplication levels"):
        assert piece in text, piece
    assert "--lane-dups-top" in cwd.__doc__ and "report.write_lane_top" in cwd.__doc__


def test_the_top_scratch_counts_when_a_lane_is_fitted():
    cwd.check_lane_dups_fits(1000, 2000, 2, 3, 4, scratch=500, saturation=300, top=200)
    with pytest.raises(MemoryError) as e:
        cwd.check_lane_dups_fits(1000, 2000, 2, 3, 4, scratch=500, saturation=300, top=201)
    msg = str(e.value)
    assert ("2001 bytes, 500 of them for --lane-dups-hamming, 300 of them for --lane-dups-saturation, 201 of them for "
            "--lane-dups-top)") in msg and "2000 bytes" in msg
    with pytest.raises(MemoryError) as e:                              # without the flag the message is what it was
        cwd.check_lane_dups_fits(1000, 1400, 2, 3, 4, scratch=401)
    assert "(1401 bytes, 401 of them for --lane-dups-hamming)" in str(e.value)


# ---- the reference, on a hand-worked lane -----------------------------------------------------------
def _hand_lane():
    """two tiles of six wells (tile indices 0 and 2 of three), four cycles; A C G T = bytes 0x40 0x41 0x42 0x43"""
    a, c, g, t, n_ = 0x40, 0x41, 0x42, 0x43, 0
    tile0 = np.array([[a, a, a, a], [c, g, t, a], [a, a, a, a], [g, g, g, g], [c, g, t, a], [n_, n_, n_, n_]], dtype=np.uint8)
    tile2 = np.array([[a, a, a, a], [c, g, t, a], [t, t, t, t], [a, a, a, c], [n_, n_, n_, n_], [g, g, g, g]], dtype=np.uint8)
    filt0 = np.array([1, 1, 1, 1, 1, 1], dtype=np.uint8)
    filt2 = np.array([1, 1, 1, 1, 1, 0], dtype=np.uint8)              # the second GGGG did not pass
    tiles = [(idx, [np.ascontiguousarray(r[:, cyc]) for cyc in range(4)], f) for idx, r, f in ((0, tile0, filt0), (2, tile2, filt2))]
    labels = np.full((3, 6), INVALID, dtype=np.uint32)
    labels[0] = [0, 1, 0, 3, 1, 5]
    labels[2] = [0, 1, 14, 15, 5, INVALID]
    return tiles, labels


def test_reference_on_a_hand_worked_lane():
    tiles, labels = _hand_lane()
    # AAAA: wells 0, 2, 12 (size 3); CGTA: 1, 4, 13 (size 3); NNNN: 5, 16 (size 2); GGGG, TTTT, AAAC alone
    head, levels, root, size, exact, tile_count, reads = lane_top(labels, tiles, 6, 3, 10)
    assert head.tolist() == [11, 3, 3, 8]
    assert levels[0].tolist() == [3, 1, 2] + [0] * 13 and levels[1].tolist() == [3, 2, 6] + [0] * 13
    assert root.tolist() == [0, 1, 5] and size.tolist() == [3, 3, 2] and exact.tolist() == [3, 3, 2]
    assert tile_count.tolist() == [[2, 0, 1], [2, 0, 1], [1, 0, 1]] and reads == ["AAAA", "CGTA", "NNNN"]
    check_top_identities(head, levels, root, size, exact, tile_count, reads, n=6, n_top=10, equality=True, cycles=4,
                         finish_lane=[11, 3, 8, 5, 3, 6, 1, 2, 0, 0, 0, 0, 0, 0])
    two = lane_top(labels, tiles, 6, 3, 2)                             # the tie of size 3 is cut by the root
    assert two[0].tolist() == [11, 3, 2, 6] and two[2].tolist() == [0, 1]
    check_top_identities(*two, n=6, n_top=2, longer=(head, levels, root, size, exact, tile_count, reads))
    one = lane_top(labels, tiles, 6, 3, 1)
    assert one[2].tolist() == [0] and one[6] == ["AAAA"]
    near = labels.copy()                                               # a cluster: AAAC joins AAAA
    near[2][3] = 0
    got = lane_top(near, tiles, 6, 3, 1)
    assert got[3].tolist() == [4] and got[4].tolist() == [3] and got[5].tolist() == [[2, 0, 2]]
    assert level_of([1, 2, 9, 10, 49, 50, 99, 100, 499, 500, 999, 1000, 4999, 5000, 9999, 10000, 1 << 31]).tolist() == \
        [0, 1, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13, 14, 14, 15, 15]
    assert decode([0x40, 0x81, 0xC2, 0x23, 0]) == "ACGTN"


# ---- the report ---------------------------------------------------------------------------------
class _Final:
    def __init__(self, pf, redundant):
        self.pf, self.redundant = pf, redundant


def _counts(k=0, n_top=10):
    """a lane of 1000 PF wells on tiles 1101 1102 1103 (100 wells each): six listed groups, one per note"""
    reads = ["G" * 19 + "A", "N" * 20, "ACGTN" * 4, "ACGT" * 5, "ACGTA" * 4, "TTGCA" * 4]
    size = [400, 50, 20, 12, 9, 2]
    exact = [390, 50, 20, 12, 9, 1]
    tile_count = [[100, 200, 100], [50, 0, 0], [0, 10, 10], [0, 0, 12], [9, 0, 0], [1, 1, 0]]
    root = [3, 17, 101, 250, 40, 99]
    groups = [507, 1, 0, 0, 0, 0, 0, 0, 1, 2, 1, 1, 0, 0, 0, 0]
    wells = [507, 2, 0, 0, 0, 0, 0, 0, 9, 32, 50, 400, 0, 0, 0, 0]
    head = [1000, 6, 6, 493]
    return report.LaneTopCounts.from_rows(head, [groups, wells], root, size, exact, tile_count, reads, n_top, 100,
                                          ["1101", "1102", "1103"], _Final(1000, 487), k)


def _text(counts, verbose=True):
    out = io.StringIO()
    report.write_lane_top("3", counts, verbose=verbose, out=out)
    return out.getvalue()


def test_write_lane_top_levels_list_notes_and_closing_line():
    text = _text(_counts())
    lines = text.split("\n")
    assert lines[0] == "" and text.count("LaneTopLevel: 3\t") == 6 and text.count("LaneTop: 3\tRank: ") == 6
    assert "LaneTopLevel: 3\tSize: 1\tGroups: 507\tWells: 507\tOf distinct: %.5f\tOf PF: 0.50700" % (507 / 513) in text
    assert "LaneTopLevel: 3\tSize: 10-49\tGroups: 2\tWells: 32\t" in text and "\tSize: 100-499\tGroups: 1\tWells: 400\t" in text
    assert "\tSize: 9\tGroups: 1\tWells: 9\t" in text and "\tSize: 50-99\t" in text and "Size: 3\t" not in text
    assert ("LaneTop: 3\tRank: 1\tSize: 400\tOf PF: 0.40000\tRoot: 1101:3\tTiles: 3\tLargest tile share: 0.50000\tRead: "
            + "G" * 19 + "A\tNote: poly-G") in text
    notes = re.findall(r"Rank: (\d)\t.*\tNote: (.*)", text)
    assert notes == [("1", "poly-G"), ("2", "all N"), ("3", "N-rich"), ("4", "one tile"), ("5", "-"), ("6", "-")]
    assert "Root: 1102:1\t" in text and "Root: 1103:50\tTiles: 1\tLargest tile share: 1.00000" in text
    assert "Exact:" not in text and "consensus" not in text
    assert lines[-2] == ("LaneTopSummary: 3\tAsked: 10\tListed: 6\tHamming: 0\tPF wells: 1000\tGroups: 6\tCovered: 493 "
                         "(0.49300 of PF)\tRedundant in listed: 487 of 487 (1.00000)")
    assert report.lane_top_note("A" * 18 + "CN", 5, 2) == "poly-A" and report.lane_top_note("A" * 17 + "CCN", 5, 2) == ""
    assert report.lane_top_note("ACGT" * 4 + "NNNN", 5, 2) == "N-rich" and report.lane_top_note("ACGT" * 4 + "NNN", 5, 2) == ""
    assert report.lane_top_note("ACGT", 10, 1) == "one tile" and report.lane_top_note("ACGT", 9, 1) == ""
    assert [report.lane_top_note(b * 10, 2, 2) for b in "ACGT"] == ["poly-A", "poly-C", "poly-G", "poly-T"]


def test_write_lane_top_on_clusters_and_in_summary():
    text = _text(_counts(k=2))
    assert "\tExact: 390/400\tRead: " in text and "\tExact: 1/2\t" in text and "Hamming: 2\t" in text
    assert "LaneTop: 3\tthe read shown is that of the cluster's first well (Hamming <= 2), not a consensus" in text
    short = _text(_counts(), verbose=False)
    assert short.count("LaneTopLevel: 3\t") == 1 and "Size: 100-499" in short and short.count("\tRank: ") == 5
    assert "Rank: 6" not in short and "LaneTopSummary: 3\tAsked: 10\tListed: 6\t" in short


def test_write_lane_top_with_an_empty_list():
    empty = report.LaneTopCounts.from_rows([700, 0, 0, 0], [[700] + [0] * 15, [700] + [0] * 15], [], [], [], [], [], 5, 100,
                                           ["1101"], _Final(700, 0), 2)
    text = _text(empty)
    assert text == ("\nLaneTopLevel: 3\tSize: 1\tGroups: 700\tWells: 700\tOf distinct: 1.00000\tOf PF: 1.00000\n"
                    "LaneTopSummary: 3\tAsked: 5\tListed: 0\tHamming: 2\tPF wells: 700\tGroups: 0\tCovered: 0 (0.00000 of PF)\t"
                    "Redundant in listed: 0 of 0 (0.00000)\n")
    last = report.LaneTopCounts.from_rows([20000, 1, 1, 20000], [[0] * 15 + [1], [0] * 15 + [20000]], [0], [20000], [20000],
                                          [[20000]], ["ACGT"], 1, 20000, ["1101"], _Final(20000, 19999), 0)
    assert "LaneTopLevel: 3\tSize: >=10000\tGroups: 1\tWells: 20000\t" in _text(last)


def test_write_lane_top_tsv():
    out = io.StringIO()
    report.write_lane_top_tsv("3", _counts(), out)
    lines = out.getvalue().rstrip("\n").split("\n")
    assert lines[0] == "lane\trank\tsize\texact\ttiles\troot_tile\troot_well\tread" and len(lines) == 7
    assert lines[1] == "3\t1\t400\t390\t3\t1101\t3\t" + "G" * 19 + "A\t1101=100\t1102=200\t1103=100"
    assert lines[6] == "3\t6\t2\t1\t2\t1101\t99\t" + "TTGCA" * 4 + "\t1101=1\t1102=1"
    out = io.StringIO()
    report.write_lane_top_tsv("4", _counts(), out, header=False)
    assert out.getvalue().startswith("4\t1\t400\t")
    with pytest.raises(AssertionError):                                # rows that contradict each other are refused
        report.LaneTopCounts.from_rows([1000, 6, 6, 493], [[0] * 16, [0] * 16], [], [], [], [], [], 10, 100, ["1101"],
                                       _Final(1000, 487))
