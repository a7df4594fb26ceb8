"""A lane's duplication against its reads' GC content without a GPU: the header against the binding, the scratch
formula and its error codes, the parser's refusals, the fit check, the reference in its two versions on a hand-worked
lane, and the report block and the TSV spelled out."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from lanedups_ref import lane_dups
from lanegc_ref import HIST_COLS, LANE_COLS, TILE_COLS, check_gc_identities, lane_gc, lane_gc_literal
from lanenear_ref import lane_near_dups
from well_duplicates_amd import _lib, report
from well_duplicates_amd import count_well_duplicates as cwd

HEADER = os.path.join(_lib.INCLUDE, "welldup_lanegc.h")


# ---- C ABI --------------------------------------------------------------------------------------
def test_lanegc_header_and_binding_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(wd_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.LANEGC_PROTOTYPES) == ["wd_lane_gc", "wd_lane_gc_scratch"]
    define = lambda name: int(re.search(r"#define WD_LANEGC_%s\s+(.+)" % name, text).group(1).strip())
    assert define("HIST_COLS") == _lib.LANEGC_HIST_COLS == HIST_COLS == report.LANE_GC_HIST_COLS
    assert define("LANE_COLS") == _lib.LANEGC_LANE_COLS == LANE_COLS == report.LANE_GC_LANE_COLS
    assert define("TILE_COLS") == _lib.LANEGC_TILE_COLS == TILE_COLS == report.LANE_GC_TILE_COLS
    taken = set()
    for table in (_lib.PROTOTYPES, _lib.SETS_PROTOTYPES, _lib.TILEDUPS_PROTOTYPES, _lib.TILENEAR_PROTOTYPES,
                  _lib.LANEDUPS_PROTOTYPES, _lib.LANENEAR_PROTOTYPES, _lib.LANEINDEX_PROTOTYPES, _lib.LANEMISMATCH_PROTOTYPES,
                  _lib.LANEDISTANCE_PROTOTYPES, _lib.LANEQUALITY_PROTOTYPES, _lib.LANESATURATION_PROTOTYPES,
                  _lib.LANETOP_PROTOTYPES, _lib.LANEHOPS_PROTOTYPES):
        taken |= set(table)
    assert not set(_lib.LANEGC_PROTOTYPES) & taken
    source = open(os.path.join(_lib.CSRC, "lane_gc.inc")).read()
    assert "k_lgc_tally" in source and _lib.unit_of_kernel("k_lgc_tally") == "tiledups"
    assert "asm" not in source                                         # plain C++ and vector atomics only
    assert "k_ln_members" in source and "k_ln_compress" in source      # where the near finish writes members is said
    assert "k_lgc_tally" in open(os.path.join(_lib.CSRC, "lane_mismatch.inc")).read()      # listed among the readers
    deps = {os.path.basename(f) for f in _lib._deps(os.path.join(_lib.CSRC, "welldup_tiledups.hip"))}
    assert {"lane_gc.inc", "welldup_lanegc.h"} <= deps
    _lib.build()
    lib = _lib.load()
    for s in syms:                                                     # exported, and bound as the table says
        assert getattr(lib, s).argtypes == _lib.LANEGC_PROTOTYPES[s][1]


def _scratch(lib, tiles, cycles):
    b = ctypes.c_size_t()
    rc = lib.wd_lane_gc_scratch(tiles, cycles, ctypes.byref(b))
    return rc, b.value


def test_scratch_size_needs_no_gpu_and_matches_the_header():
    _lib.build()
    lib = _lib.load()
    text = open(HEADER).read()
    for piece in ("5120 * max_tiles", "+ 2048 * (L + 1)", "+ 4 * max_tiles", "rounded up to 256 bytes", "885 248 bytes"):
        assert piece in text, piece
    up = lambda v: (v + 255) // 256 * 256
    for tiles in (0, 1, 7, 64, 65, 112, 4096, 65535):
        for cycles in (0, 1, 10, 37, 151, 1024):
            assert _scratch(lib, tiles, cycles) == (0, 5120 * tiles + 2048 * (cycles + 1) + up(4 * tiles))
    assert _scratch(lib, 112, 151) == (0, 885248)                      # the header's HiSeq 4000 lane
    assert _scratch(lib, 65536, 10)[0] == _lib.ERR_UNSUPPORTED and _scratch(lib, 3, 1025)[0] == _lib.ERR_UNSUPPORTED
    assert _scratch(lib, -1, 10)[0] == _lib.ERR_ARG and _scratch(lib, 3, -1)[0] == _lib.ERR_ARG
    assert lib.wd_lane_gc_scratch(3, 10, None) == _lib.ERR_ARG
    row = (ctypes.c_int64 * 64)()                                      # a null handle is refused before anything is looked at
    assert lib.wd_lane_gc(None, 0, None, 0, row, row, row) == _lib.ERR_ARG


# ---- CLI ----------------------------------------------------------------------------------------
def test_cli_flag_checks(tmp_path, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["-s", "hiseq_4000", "-r", str(tmp_path), "--all-wells"]
    args = cwd.parse_args(base + ["--lane-dups", "--lane-dups-gc"])
    assert args.lane_dups_gc and (args.lane_dups_gc_bins, args.lane_dups_gc_max_n, args.lane_dups_gc_out) == (None,) * 3
    assert not cwd.parse_args(base + ["--lane-dups"]).lane_dups_gc
    args = cwd.parse_args(base + ["--lane-dups", "--lane-dups-hamming", "2", "--lane-dups-gc", "--lane-dups-gc-bins", "100",
                                  "--lane-dups-gc-max-n", "3", "--lane-dups-gc-out", "gc.tsv"])
    assert (args.lane_dups_gc_bins, args.lane_dups_gc_max_n, args.lane_dups_gc_out) == (100, 3, "gc.tsv")
    assert cwd.parse_args(base + ["--lane-dups", "--lane-dups-gc", "--lane-dups-gc-bins", "2"]).lane_dups_gc_bins == 2
    for extra, message in ((["--lane-dups-gc"], "--lane-dups-gc needs --lane-dups"),
                           (["--tile-dups", "--lane-dups-gc"], "--lane-dups-gc needs --lane-dups"),
                           (["--lane-dups", "--lane-dups-gc-bins", "10"], "--lane-dups-gc-bins needs --lane-dups-gc"),
                           (["--lane-dups", "--lane-dups-gc-max-n", "0"], "--lane-dups-gc-max-n needs --lane-dups-gc"),
                           (["--lane-dups", "--lane-dups-gc-out", "x.tsv"], "--lane-dups-gc-out needs --lane-dups-gc"),
                           (["--lane-dups", "--lane-dups-gc", "--lane-dups-gc-bins", "1"], "--lane-dups-gc-bins takes 2..100, not 1"),
                           (["--lane-dups", "--lane-dups-gc", "--lane-dups-gc-bins", "101"], "--lane-dups-gc-bins takes 2..100, not 101"),
                           (["--lane-dups", "--lane-dups-gc", "--lane-dups-gc-max-n", "-1"],
                            "--lane-dups-gc-max-n takes 0..the number of scanned cycles, not -1")):
        with pytest.raises(SystemExit):
            cwd.parse_args(base + extra)
        assert message in " ".join(capsys.readouterr().err.split())
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cwd.parse_args(base + ["--lane-dups", "--lane-dups-gc"])
    assert "--lane-dups runs in a single process only" in " ".join(capsys.readouterr().err.split())


def test_cli_help_and_docstring_name_the_new_options(capsys):
    with pytest.raises(SystemExit):
        cwd.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for piece in ("--lane-dups-gc", "--lane-dups-gc-bins B", "--lane-dups-gc-max-n M", "--lane-dups-gc-out FILE", "2..100",
                  "min(B - 1, g * B // L)"):
        assert piece in text, piece
    for flag in ("--lane-dups-gc,", "--lane-dups-gc-bins", "--lane-dups-gc-max-n", "--lane-dups-gc-out", "report.write_lane_gc"):
        assert flag in cwd.__doc__, flag


def test_the_gc_scratch_counts_when_a_lane_is_fitted():
    cwd.check_lane_dups_fits(1000, 2000, 2, 3, 4, scratch=500, top=300, gc=200)
    with pytest.raises(MemoryError) as e:
        cwd.check_lane_dups_fits(1000, 2000, 2, 3, 4, scratch=500, top=300, gc=201)
    msg = str(e.value)
    assert ("2001 bytes, 500 of them for --lane-dups-hamming, 300 of them for --lane-dups-top, 201 of them for "
            "--lane-dups-gc)") in msg and "2000 bytes" in msg
    with pytest.raises(MemoryError) as e:                              # without the flag the message is what it was
        cwd.check_lane_dups_fits(1000, 1400, 2, 3, 4, scratch=401)
    assert str(e.value) == ("--lane-dups needs 0.00 GB of device memory for a lane of 2 tiles x 3 wells x 4 cycles "
                            "(1401 bytes, 401 of them for --lane-dups-hamming), and 0.00 GB (1400 bytes) are free")
    with pytest.raises(MemoryError) as e:
        cwd.check_lane_dups_fits(1000, 999, 2, 3, 4)
    assert "(1000 bytes), and" in str(e.value) and "gc" not in str(e.value)


# ---- the reference on a hand-worked lane ----------------------------------------------------------
BYTE = {"A": 0x40, "C": 0x81, "G": 0xC2, "T": 0x23, "N": 0x00}
# Tile indices 0 and 2 of a lane with room for three, six wells each, ten cycles (g, n; what the well is by equality):
#   index 0  [0] CGAAAAAAAA 2,0 root of 3   [1] AAAAAAAAAA 0,0 single   [2] CCCCGGGGTT 8,0 single
#            [3] CGAAAAAAAA 2,0 copy of 0   [4] NNCGCGATAT 4,2 root of 2, skipped below max_n = 2   [5] not PF
#   index 2 [12] GGGGGGGGGG 10,0 single    [13] CGAAAAAAAA 2,0 copy of 0   [14] NNCGCGATAT 4,2 copy of 4, skipped
#           [15] CGCGCATATA 5,0 root of 2  [16] CGCGCATATA 5,0 copy of 15  [17] NAAAAAAAAC 1,1 single, skipped at max_n = 0
# With five bins the bin of g is g // 2 (g = 10 joins bin 4): g = 2 lies on the edge of bin 1, g = 1 below it.
READS = {0: ["CGAAAAAAAA", "AAAAAAAAAA", "CCCCGGGGTT", "CGAAAAAAAA", "NNCGCGATAT", "GGGGGGGGGG"],
         2: ["GGGGGGGGGG", "CGAAAAAAAA", "NNCGCGATAT", "CGCGCATATA", "CGCGCATATA", "NAAAAAAAAC"]}
FILT = {0: [1, 1, 1, 1, 1, 0], 2: [1, 1, 1, 1, 1, 3]}


def hand_made_lane():
    return [(ti, [np.array([BYTE[r[c]] for r in READS[ti]], dtype=np.uint8) for c in range(10)],
             np.array(FILT[ti], dtype=np.uint8)) for ti in (2, 0)]


def _rows(hist):
    return {g: row.tolist() for g, row in enumerate(hist) if row.any()}


def test_reference_on_a_hand_worked_lane():
    tiles = hand_made_lane()
    fin_lane, fin_tiles, labels = lane_dups(tiles, 6, 3)
    I = 0xFFFFFFFF
    assert labels.tolist() == [[0, 1, 2, 0, 4, I], [I] * 6, [12, 0, 4, 15, 15, 17]]
    lane, trow, hist = lane_gc(tiles, 6, 3, labels, 0)
    assert lane.tolist() == [11, 4, 3, 4, 1, 1, 1, 2]
    assert trow.tolist() == [[5, 4, 12, 1, 2], [0] * 5, [6, 4, 22, 2, 7]]
    assert _rows(hist) == {0: [1, 0, 0, 0], 2: [0, 1, 2, 3], 5: [0, 1, 1, 2], 8: [1, 0, 0, 0], 10: [1, 0, 0, 0]}
    one = lane_gc(tiles, 6, 3, labels, 1)                              # the single read with one N comes in at g = 1
    assert one[0].tolist() == [11, 4, 3, 4, 0, 1, 1, 2] and one[1].tolist() == [[5, 4, 12, 1, 2], [0] * 5, [6, 5, 23, 2, 7]]
    assert _rows(one[2]) == {**_rows(hist), 1: [1, 0, 0, 0]}
    two = lane_gc(tiles, 6, 3, labels, 2)                              # and the skipped pair at g = 4
    assert two[0].tolist() == [11, 4, 3, 4, 0, 0, 0, 0] and two[1].tolist() == [[5, 5, 16, 1, 2], [0] * 5, [6, 6, 27, 3, 11]]
    assert _rows(two[2]) == {**_rows(one[2]), 4: [0, 1, 1, 2]}
    full = lane_gc(tiles, 6, 3, labels, 10)
    assert all((a == b).all() for a, b in zip(two, full))
    results = {0: (lane, trow, hist), 1: one, 2: two, 10: full}
    for max_n, res in results.items():                                 # the two versions, and the identities
        lit = lane_gc_literal(tiles, 6, 3, labels, max_n)
        assert all(a.shape == b.shape and (a == b).all() for a, b in zip(res, lit)), max_n
        check_gc_identities(*res, max_n, fin_lane, fin_tiles, equality=True, wider=full)
    with pytest.raises(AssertionError):                                # an identity that fails is noticed
        bad = hist.copy()
        bad[2, 3] += 1
        check_gc_identities(lane, trow, bad, 0, fin_lane, fin_tiles, equality=True)
    with pytest.raises(AssertionError):
        check_gc_identities(lane, trow, hist, 10)                      # max_n = L skips nothing
    # on clusters (K = 1: CGCGCATATA has no neighbour, nothing links) the labels are the classes; at K = 10 everything
    # is one cluster of 11 wells whose root is well 0: one root, ten copies by their own reads
    near = lane_near_dups(tiles, 6, 3, 1)
    assert (near[2] == labels).all()
    near_lane, near_tiles, all_one = lane_near_dups(tiles, 6, 3, 10)
    got = lane_gc(tiles, 6, 3, all_one, 10)
    assert got[0].tolist() == [11, 0, 1, 10, 0, 0, 0, 0] and got[2][2].tolist() == [0, 1, 2, 11]
    assert got[2][:, 2].tolist() == [1, 1, 2, 0, 2, 2, 0, 0, 1, 0, 1]
    lit = lane_gc_literal(tiles, 6, 3, all_one, 10)
    assert all((a == b).all() for a, b in zip(got, lit))
    check_gc_identities(*got, 10, np.concatenate([near_lane[:6], near_lane[7:]]), near_tiles)
    with pytest.raises(AssertionError):                                # a copy's read is not its root's there
        check_gc_identities(*got, 10, equality=True)


# ---- the report -----------------------------------------------------------------------------------
def _counts(max_n=0, bins=5, k=0):
    tiles = hand_made_lane()
    labels = lane_dups(tiles, 6, 3)[2]
    return report.LaneGCCounts.from_rows(*lane_gc(tiles, 6, 3, labels, max_n), ["1101", None, "1103"], max_n, bins, k)


def _text(counts, verbose=True):
    out = io.StringIO()
    report.write_lane_gc("3", counts, verbose=verbose, out=out)
    return out.getvalue()


BLOCK = [
    "",
    "LaneGC: 3\tBin: 0\tGC: 0-1\tDistinct: 1 (0.20000)\tReads: 1\tRedundant: 0\tDuplication: 0.00000\tRelative: 0.000\t"
    "MeanFamily: n/a\tCopies: 0\tLibrarySize: n/a",
    "LaneGC: 3\tBin: 1\tGC: 2-3\tDistinct: 1 (0.20000)\tReads: 3\tRedundant: 2\tDuplication: 0.66667\tRelative: 1.778\t"
    "MeanFamily: 3.000\tCopies: 2\tLibrarySize: 1",
    "LaneGC: 3\tBin: 2\tGC: 4-5\tDistinct: 1 (0.20000)\tReads: 2\tRedundant: 1\tDuplication: 0.50000\tRelative: 1.333\t"
    "MeanFamily: 2.000\tCopies: 1\tLibrarySize: 1",
    "LaneGC: 3\tBin: 3\tGC: 6-7\tDistinct: 0 (0.00000)\tReads: 0\tRedundant: 0\tDuplication: 0.00000\tRelative: 0.000\t"
    "MeanFamily: n/a\tCopies: 0\tLibrarySize: n/a",
    "LaneGC: 3\tBin: 4\tGC: 8-10\tDistinct: 2 (0.40000)\tReads: 2\tRedundant: 0\tDuplication: 0.00000\tRelative: 0.000\t"
    "MeanFamily: n/a\tCopies: 0\tLibrarySize: n/a",
    "LaneGCTile: 3\tTile: 1101\tPF: 5\tCounted: 4\tMeanGC: 0.30000\tCopies: 1\tCopiesMeanGC: 0.20000",
    "LaneGCTile: 3\tTile: 1103\tPF: 6\tCounted: 4\tMeanGC: 0.55000\tCopies: 2\tCopiesMeanGC: 0.35000",
    # both tiles lie 0.125 from the lane's 34 / 80: the first in sorted order is named
    "LaneGCTiles: 3\tLaneMeanGC: 0.42500\tFurthest: 1101 (0.30000, -0.12500)",
    # distinct molecules at g = 0, 2, 5, 8, 10: mean 0.5; copies at 2, 2, 5: 0.3.  Quartiles: 4 x 2 >= 5 at g = 2,
    # 4 x 4 >= 15 at g = 8.  g <= 2: 4 reads, 2 redundant; 2 < g <= 8: 3 reads, 1 redundant; g = 10: 1 read.
    "LaneGCSummary: 3\tMaxN: 0\tCycles: 10\tBins: 5\tCounted: 8\tSkipped: 3\tDistinct: 5\tDuplication: 0.37500\t"
    "MeanGC distinct: 0.50000\tMeanGC redundant: 0.30000\tShift: -0.20000\tQ1: 2\tQ3: 8\t"
    "Duplication at or below Q1: 0.50000\tbetween: 0.33333\tabove Q3: 0.00000\tHighest: bin 1 (GC 2-3, 0.66667)",
    "",
]


def test_write_lane_gc_every_line():
    assert _text(_counts()).split("\n") == BLOCK
    short = _text(_counts(), verbose=False).split("\n")
    assert short == BLOCK[:6] + BLOCK[9:]                              # the summary flag drops the tiles' lines
    ham = _text(_counts(k=2))
    assert ham.count("\tHamming: 2\t") == 6 and "LaneGCSummary: 3\tHamming: 2\tMaxN: 0\t" in ham
    assert ham.replace("\tHamming: 2", "") == "\n".join(BLOCK)
    # max_n = 2: the pair at g = 4 joins bin 2, the single at g = 1 bin 0; nothing is skipped: 11 reads, 4 redundant
    wide = _text(_counts(max_n=2))
    assert ("LaneGC: 3\tBin: 2\tGC: 4-5\tDistinct: 2 (0.28571)\tReads: 4\tRedundant: 2\tDuplication: 0.50000\tRelative: 1.375\t"
            "MeanFamily: 2.000\tCopies: 2\tLibrarySize: 3") in wide
    assert "\tMaxN: 2\tCycles: 10\tBins: 5\tCounted: 11\tSkipped: 0\tDistinct: 7\tDuplication: 0.36364\t" in wide
    # more bins than values of g: a bin that no g falls into is printed empty, and g = L closes the last one
    many = _text(_counts(bins=20), verbose=False).split("\n")
    assert len(many) == 1 + 20 + 2 and many[2].startswith("LaneGC: 3\tBin: 1\tGC: -\tDistinct: 0 ")
    assert many[5].startswith("LaneGC: 3\tBin: 4\tGC: 2-2\tDistinct: 1 ") and many[20].startswith("LaneGC: 3\tBin: 19\tGC: 10-10\t")
    assert "Highest: bin 4 (GC 2-2, 0.66667)" in many[21]
    two = _counts(bins=2)
    assert [two.bin_of(g) for g in range(11)] == [0] * 5 + [1] * 6
    assert [_counts(bins=3).bin_of(g) for g in range(11)] == [0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2]


def test_write_lane_gc_of_an_empty_lane_and_of_a_lane_without_groups():
    empty = report.LaneGCCounts.from_rows([0] * 8, [[0] * 5], [[0] * 4] * 11, ["1101"], 0, 2)
    lines = _text(empty).split("\n")
    assert lines[1] == ("LaneGC: 3\tBin: 0\tGC: 0-4\tDistinct: 0 (0.00000)\tReads: 0\tRedundant: 0\tDuplication: 0.00000\t"
                        "Relative: n/a\tMeanFamily: n/a\tCopies: 0\tLibrarySize: n/a")
    assert lines[3] == "LaneGCTile: 3\tTile: 1101\tPF: 0\tCounted: 0\tMeanGC: n/a\tCopies: 0\tCopiesMeanGC: n/a"
    assert lines[4] == ("LaneGCSummary: 3\tMaxN: 0\tCycles: 10\tBins: 2\tCounted: 0\tSkipped: 0\tDistinct: 0\tDuplication: 0.00000\t"
                        "MeanGC distinct: n/a\tMeanGC redundant: n/a\tShift: n/a\tQ1: 0\tQ3: 0\tDuplication at or below Q1: 0.00000\t"
                        "between: 0.00000\tabove Q3: 0.00000\tHighest: n/a")
    assert report.library_size(0, 0) is None and report.library_size(5, 5) is None      # an empty bin, a bin without a copy
    hist = [[0] * 4 for _ in range(11)]
    hist[3][0], hist[7][0] = 30, 10
    lone = report.LaneGCCounts.from_rows([40, 40, 0, 0, 0, 0, 0, 0], [[40, 40, 160, 0, 0]], hist, ["1101"], 0, 2)
    text = _text(lone, verbose=False)
    assert "Bin: 0\tGC: 0-4\tDistinct: 30 (0.75000)\tReads: 30\tRedundant: 0\tDuplication: 0.00000\tRelative: n/a\t" in text
    assert "MeanGC distinct: 0.40000\tMeanGC redundant: n/a\tShift: n/a\tQ1: 3\tQ3: 3\t" in text
    assert "Highest: bin 0 (GC 0-4, 0.00000)" in text                  # a tie goes to the lower bin
    with pytest.raises(AssertionError):
        report.LaneGCCounts.from_rows([0] * 8, [[0] * 5], [[0] * 4] * 11, ["1101"], 0, 1)
    with pytest.raises(AssertionError):
        report.LaneGCCounts.from_rows([0] * 8, [[0] * 5], [[0] * 4] * 11, ["1101"], 11, 5)


def test_the_quartile_cut_on_ties():
    q = report.gc_quartiles
    assert q([0] * 11) == (0, 0)
    assert q([0, 0, 0, 8]) == (3, 3)                                   # every molecule at one g: both cuts there
    assert q([1, 1, 1, 1]) == (0, 2) and q([1, 1, 1, 1, 1]) == (1, 3)  # 4 x 1 >= 4; 4 x 2 >= 5 and 4 x 4 >= 15
    assert q([2, 0, 0, 6]) == (0, 3)                                   # exactly a quarter at g = 0
    assert q([1, 0, 0, 7]) == (3, 3)                                   # less than a quarter below the tie: it takes both
    assert q([3, 0, 5, 0, 0, 4]) == (0, 5) and q([3, 0, 6, 0, 0, 3]) == (0, 2)       # exactly three quarters at g = 2
    # at or below Q1 holds at least a quarter of the molecules, above Q3 at most a quarter
    rng = np.random.default_rng(4)
    for _ in range(50):
        d = rng.integers(0, 5, 12).tolist()
        q1, q3 = q(d)
        if sum(d):
            assert q1 <= q3 and 4 * sum(d[:q1 + 1]) >= sum(d) > 4 * sum(d[:q1]) and 4 * sum(d[q3 + 1:]) <= sum(d)
            assert 4 * sum(d[:q3 + 1]) >= 3 * sum(d) > 4 * sum(d[:q3])


def test_write_lane_gc_tsv():
    out = io.StringIO()
    report.write_lane_gc_tsv("3", _counts(), out)
    assert out.getvalue().split("\n") == [
        "lane\tgc\tsingle\troots\tcopies\tfamily_wells", "3\t0\t1\t0\t0\t0", "3\t1\t0\t0\t0\t0", "3\t2\t0\t1\t2\t3",
        "3\t3\t0\t0\t0\t0", "3\t4\t0\t0\t0\t0", "3\t5\t0\t1\t1\t2", "3\t6\t0\t0\t0\t0", "3\t7\t0\t0\t0\t0", "3\t8\t1\t0\t0\t0",
        "3\t9\t0\t0\t0\t0", "3\t10\t1\t0\t0\t0", ""]
    out = io.StringIO()
    report.write_lane_gc_tsv("4", _counts(), out, header=False)
    assert out.getvalue().startswith("4\t0\t1\t0\t0\t0\n")
