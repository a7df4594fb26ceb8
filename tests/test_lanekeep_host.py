"""The best well of each of a lane's families without a GPU: the header against the binding, the scratch formula and
its error codes, the parser's refusals, the fit check, the reference in its two versions on hand-made families - ties,
the best on another tile, every weight zero -, the filter writer's round trip through bcl.Tile, and the report block
spelled out."""
import ctypes
import io
import os
import re
import struct

import numpy as np
import pytest

from lanedups_ref import lane_dups
from lanekeep_ref import (GAIN_BINS, LANE_COLS, TILE_COLS, bin_table, check_keep_identities, gain_bin, lane_keep,
                          lane_keep_literal, quality_weight, weights_of)
from lanenear_ref import lane_near_dups
from well_duplicates_amd import _lib, bcl, report
from well_duplicates_amd import count_well_duplicates as cwd

HEADER = os.path.join(_lib.INCLUDE, "welldup_lanekeep.h")


# ---- C ABI --------------------------------------------------------------------------------------
def test_lanekeep_header_and_binding_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(wd_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.LANEKEEP_PROTOTYPES) == ["wd_lane_keep", "wd_lane_keep_scratch"]
    define = lambda name: int(re.search(r"#define WD_LANEKEEP_%s\s+(.+)" % name, text).group(1).strip())
    assert define("LANE_COLS") == _lib.LANEKEEP_LANE_COLS == LANE_COLS == report.LANE_KEEP_LANE_COLS == 17
    assert define("TILE_COLS") == _lib.LANEKEEP_TILE_COLS == TILE_COLS == report.LANE_KEEP_TILE_COLS == 6
    assert define("GAIN_BINS") == _lib.LANEKEEP_GAIN_BINS == GAIN_BINS == len(report.LANE_KEEP_GAIN_NAMES) == 8
    assert define("MAX_Q") == _lib.LANEKEEP_MAX_Q == 63 and _lib.LANEKEEP_DEFAULT_MIN_Q == 15
    assert _lib.LANEKEEP_GAIN_NAMES == report.LANE_KEEP_GAIN_NAMES
    taken = set()
    for name in dir(_lib):
        if name.endswith("PROTOTYPES") and name != "LANEKEEP_PROTOTYPES":
            taken |= set(getattr(_lib, name))
    assert not set(_lib.LANEKEEP_PROTOTYPES) & taken
    source = open(os.path.join(_lib.CSRC, "lane_keep.inc")).read()
    for kernel in ("k_lk_score", "k_lk_mark"):
        assert kernel in source and _lib.unit_of_kernel(kernel) == "tiledups"
        assert kernel in open(os.path.join(_lib.CSRC, "lane_mismatch.inc")).read()         # listed among the readers
    assert "asm" not in source                                         # plain C++ and vector atomics only
    assert "static_assert(WD_LANEKEEP_MAX_Q * kMaxCycles <= (int)kLkMaxScore" in source   # the 16-bit score is held to its bound
    assert "lgc_piece(" in source and "lgc_piece(const" not in source  # the piece loads are lane_gc.inc's, used, not copied
    assert "Why the read before the atomic is safe" in source and "does not depend on the order of execution" in source
    deps = {os.path.basename(f) for f in _lib._deps(os.path.join(_lib.CSRC, "welldup_tiledups.hip"))}
    assert {"lane_keep.inc", "welldup_lanekeep.h", "lane_quality.inc", "lane_gc.inc"} <= deps
    top = open(os.path.join(_lib.CSRC, "lane_top.inc")).read()         # included after everything of lane_quality.inc
    assert top.rstrip().splitlines()[-2:] == ['#include "lane_keep.inc"', "#endif"]
    assert "lane_keep_emu.cpp" in open(os.path.join(_lib.REPO, "tools", "wave_emu.h")).read()
    _lib.build()
    lib = _lib.load()
    for s in syms:                                                     # exported, and bound as the table says
        assert getattr(lib, s).argtypes == _lib.LANEKEEP_PROTOTYPES[s][1]


def _scratch(lib, tiles, wells):
    b = ctypes.c_size_t()
    rc = lib.wd_lane_keep_scratch(tiles, wells, ctypes.byref(b))
    return rc, b.value


def test_scratch_size_needs_no_gpu_and_matches_the_header():
    _lib.build()
    lib = _lib.load()
    text = open(HEADER).read()
    for piece in ("8 * W", "+ 2 * W", "+ 3072 * max_tiles", "+ 5632", "+ 4 * max_tiles", "+ 8 * max_tiles",
                  "rounded up to 256 bytes", "4.83 GB"):
        assert piece in text, piece
    up = lambda v: (v + 255) // 256 * 256
    for tiles in (0, 1, 7, 64, 65, 112, 4096, 65535):
        for wells in (0, 1, 127, 128, 700, 8193, 65536):
            w = tiles * wells
            assert _scratch(lib, tiles, wells) == (0, up(8 * w) + up(2 * w) + 3072 * tiles + 5632 + up(4 * tiles) + up(8 * tiles))
    rc, hiseq = _scratch(lib, 112, 4309253)                            # the header's HiSeq 4000 lane
    assert rc == 0 and round(hiseq / 1e9, 2) == 4.83
    assert _scratch(lib, 65536, 10)[0] == _lib.ERR_UNSUPPORTED
    assert _scratch(lib, 1, (1 << 32) - 2)[0] == 0 and _scratch(lib, 1, (1 << 32) - 1)[0] == _lib.ERR_UNSUPPORTED
    assert _scratch(lib, 2, 1 << 31)[0] == _lib.ERR_UNSUPPORTED        # the limits of a lane's accumulator
    assert _scratch(lib, -1, 10)[0] == _lib.ERR_ARG and _scratch(lib, 3, -1)[0] == _lib.ERR_ARG
    assert lib.wd_lane_keep_scratch(3, 10, None) == _lib.ERR_ARG
    row = (ctypes.c_int64 * 64)()                                      # a null handle is refused before anything is looked at
    assert lib.wd_lane_keep(None, 15, None, 0, row, row, None) == _lib.ERR_ARG


# ---- CLI ----------------------------------------------------------------------------------------
def test_cli_flag_checks(tmp_path, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["-s", "hiseq_4000", "-r", str(tmp_path), "--all-wells"]
    args = cwd.parse_args(base + ["--lane-dups", "--lane-dups-keep"])
    assert args.lane_dups_keep and (args.lane_dups_keep_min_q, args.lane_dups_keep_out) == (None, None)
    assert not args.lane_dups_quality and args.lane_dups_quality_edges == cwd.DEFAULT_QUALITY_BINS
    assert not cwd.parse_args(base + ["--lane-dups"]).lane_dups_keep
    args = cwd.parse_args(base + ["--lane-dups", "--lane-dups-hamming", "2", "--lane-dups-keep", "--lane-dups-keep-min-q", "0",
                                  "--lane-dups-keep-out", "dedup", "--lane-dups-quality-bins", "0,10,20,30"])
    assert (args.lane_dups_keep_min_q, args.lane_dups_keep_out, args.lane_dups_quality_edges) == (0, "dedup", [0, 10, 20, 30])
    assert cwd.parse_args(base + ["--lane-dups", "--lane-dups-keep", "--lane-dups-keep-min-q", "63"]).lane_dups_keep_min_q == 63
    both = cwd.parse_args(base + ["--lane-dups", "--lane-dups-keep", "--lane-dups-quality", "--lane-dups-quality-bins", "0,7"])
    assert both.lane_dups_quality and both.lane_dups_keep and both.lane_dups_quality_edges == [0, 7]
    for extra, message in ((["--lane-dups-keep"], "--lane-dups-keep needs --lane-dups"),
                           (["--tile-dups", "--lane-dups-keep"], "--lane-dups-keep needs --lane-dups"),
                           (["--lane-dups", "--lane-dups-keep-min-q", "15"], "--lane-dups-keep-min-q needs --lane-dups-keep"),
                           (["--lane-dups", "--lane-dups-keep-out", "d"], "--lane-dups-keep-out needs --lane-dups-keep"),
                           (["--lane-dups", "--lane-dups-keep", "--lane-dups-keep-min-q", "64"],
                            "--lane-dups-keep-min-q takes 0..63, not 64"),
                           (["--lane-dups", "--lane-dups-keep", "--lane-dups-keep-min-q", "-1"],
                            "--lane-dups-keep-min-q takes 0..63, not -1"),
                           (["--lane-dups", "--lane-dups-quality-bins", "0,7"],
                            "--lane-dups-quality-bins needs --lane-dups-quality"),
                           (["--lane-dups", "--lane-dups-keep", "--lane-dups-quality-bins", "1,7"],
                            "--lane-dups-quality-bins: the first edge is 0")):
        with pytest.raises(SystemExit):
            cwd.parse_args(base + extra)
        assert message in " ".join(capsys.readouterr().err.split())
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cwd.parse_args(base + ["--lane-dups", "--lane-dups-keep"])
    assert "--lane-dups runs in a single process only" in " ".join(capsys.readouterr().err.split())


def test_cli_help_and_docstring_name_the_new_options(capsys):
    with pytest.raises(SystemExit):
        cwd.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for piece in ("--lane-dups-keep", "--lane-dups-keep-min-q Q", "--lane-dups-keep-out DIR", "0..63, default 15",
                  "MarkDuplicates", "L00<lane>"):
        assert piece in text, piece
    for flag in ("--lane-dups-keep,", "--lane-dups-keep-min-q", "--lane-dups-keep-out", "report.write_lane_keep"):
        assert flag in cwd.__doc__, flag


def test_the_keep_scratch_counts_when_a_lane_is_fitted():
    cwd.check_lane_dups_fits(1000, 2000, 2, 3, 4, scratch=500, quality=300, keep=200)
    with pytest.raises(MemoryError) as e:
        cwd.check_lane_dups_fits(1000, 2000, 2, 3, 4, scratch=500, quality=300, keep=201)
    msg = str(e.value)
    assert ("2001 bytes, 500 of them for --lane-dups-hamming, 300 of them for --lane-dups-quality, 201 of them for "
            "--lane-dups-keep)") in msg and "2000 bytes" in msg
    with pytest.raises(MemoryError) as e:                              # without the flag the message is what it was
        cwd.check_lane_dups_fits(1000, 1400, 2, 3, 4, scratch=401)
    assert str(e.value) == ("--lane-dups needs 0.00 GB of device memory for a lane of 2 tiles x 3 wells x 4 cycles "
                            "(1401 bytes, 401 of them for --lane-dups-hamming), and 0.00 GB (1400 bytes) are free")


# ---- the reference on hand-made families ----------------------------------------------------------
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
EDGES = [0, 10, 20, 30]            # with min_q 15 the bins weigh 0, 0, 20, 30
# Tile indices 0 and 2 of a lane with room for three, six wells each, four cycles: (read, qualities, PF) and, with
# min_q 15, the score; what the well is by equality.
#   index 0  [0] ACGT 12 12 12 12    0  root of A (3, 13, 16)        [1] AAAA 35 35 35 35  120  single
#            [2] CCCC 25 25 25 25   80  root of B (14), tied with it  [3] ACGT 30 30 20  5   80  copy in A
#            [4] GGGG 40 40 40 40  120  root of C (15), the best      [5] ACGT, not PF
#   index 2 [12] TTTT 20 20 20 20   80  single                       [13] ACGT 30 30 30 20  110  copy in A: its best
#           [14] CCCC 25 25 25 25   80  copy in B: the root wins     [15] GGGG 20 20 10 10   40  copy in C
#           [16] ACGT 30 30 30 20  110  copy in A, tied with 13       [17] NNNN (bytes 0)     0  single
WELLS = {0: [("ACGT", [12] * 4, 1), ("AAAA", [35] * 4, 1), ("CCCC", [25] * 4, 1), ("ACGT", [30, 30, 20, 5], 1),
             ("GGGG", [40] * 4, 1), ("ACGT", [40] * 4, 0)],
         2: [("TTTT", [20] * 4, 1), ("ACGT", [30, 30, 30, 20], 1), ("CCCC", [25] * 4, 3), ("GGGG", [20, 20, 10, 10], 1),
             ("ACGT", [30, 30, 30, 20], 1), ("NNNN", [0] * 4, 3)]}


def hand_made_lane():
    byte = lambda read, quals, c: 0 if read[c] == "N" else CODE[read[c]] | quals[c] << 2
    return [(ti, [np.array([byte(r, q, c) for r, q, _ in WELLS[ti]], dtype=np.uint8) for c in range(4)],
             np.array([f for _, _, f in WELLS[ti]], dtype=np.uint8)) for ti in (2, 0)]


def test_bins_weights_and_gain_bins():
    assert bin_table(EDGES).tolist() == [0] * 10 + [1] * 10 + [2] * 10 + [3] * 34
    assert bin_table([0, 7, 7, 33])[6:8].tolist() == [0, 2] and bin_table([0]).tolist() == [0] * 64      # an empty bin
    assert weights_of(EDGES, 15).tolist() == [0, 0, 20, 30] and weights_of(EDGES, 0).tolist() == EDGES
    assert weights_of(EDGES, 30).tolist() == [0, 0, 0, 30] and not weights_of(EDGES, 31).any()
    assert quality_weight(EDGES, 15)[[0, 14, 19, 20, 29, 30, 63]].tolist() == [0, 0, 0, 20, 20, 30, 30]
    assert [gain_bin(g) for g in (0, 1, 9, 10, 19, 20, 49, 50, 99, 100, 199, 200, 499, 500, 64512)] == \
        [0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7]


def test_reference_on_hand_made_families():
    tiles = hand_made_lane()
    fin_lane, fin_tiles, labels = lane_dups(tiles, 6, 3)
    I = 0xFFFFFFFF
    assert labels.tolist() == [[0, 1, 2, 0, 4, I], [I] * 6, [12, 0, 2, 4, 0, 17]]
    lane, trow, masks, singles = lane_keep(tiles, 6, 3, labels, EDGES, 15)
    #                      PF K  D  In SumK SumD F  M  SumR gains: two of 0 (B tied, C the root), A's 110 in 100-199
    assert lane.tolist() == [11, 6, 5, 1, 510, 310, 3, 1, 200, 2, 0, 0, 0, 0, 1, 0, 0]
    assert trow.tolist() == [[5, 3, 2, 0, 320, 80], [0] * 6, [6, 3, 3, 1, 190, 230]]
    assert masks[0].tolist() == [0, 1, 1, 0, 1, 0] and masks[2].tolist() == [1, 1, 0, 0, 0, 1] and sorted(masks) == [0, 2]
    assert singles == 200
    # min_q 0: every edge weighs - [0] scores 40, [3] 30 + 30 + 20 + 0, [13] and [16] 110, B 80 = 80, C 160 > 40 + 20
    zero = lane_keep(tiles, 6, 3, labels, EDGES, 0)
    assert zero[0].tolist() == [11, 6, 5, 1, 120 + 80 + 0 + 110 + 80 + 120, 40 + 80 + 110 + 80 + 60, 3, 1, 40 + 80 + 120,
                                2, 0, 0, 0, 1, 0, 0, 0]
    assert all((zero[2][t] == masks[t]).all() for t in masks)
    # min_q 30: [3] scores 60 and [13], [16] 90; min_q 31, above every edge: every weight is zero and the roots stay
    thirty = lane_keep(tiles, 6, 3, labels, EDGES, 30)
    assert thirty[0].tolist() == [11, 6, 5, 1, 120 + 90 + 0 + 120, 60 + 90, 3, 1, 120, 2, 0, 0, 0, 1, 0, 0, 0]
    none = lane_keep(tiles, 6, 3, labels, EDGES, 31)
    assert none[0].tolist() == [11, 6, 5, 0, 0, 0, 3, 0, 0, 3, 0, 0, 0, 0, 0, 0, 0]
    assert none[1].tolist() == [[5, 4, 1, 0, 0, 0], [0] * 6, [6, 2, 4, 0, 0, 0]]           # per tile Dropped differs from min_q 15's
    assert none[2][0].tolist() == [1, 1, 1, 0, 1, 0] and none[2][2].tolist() == [1, 0, 0, 0, 0, 1]
    # QHist of the PF wells, as LaneDups.qualities would count it, for identity 4
    qhist = np.zeros(64, dtype=np.int64)
    for _, planes, filt in tiles:
        for p in planes:
            qhist += np.bincount((p >> 2)[(filt & 1) != 0], minlength=64)
    for min_q, res in ((15, (lane, trow, masks, singles)), (0, zero), (30, thirty), (31, none), (63, lane_keep(tiles, 6, 3, labels, EDGES, 63))):
        lit = lane_keep_literal(tiles, 6, 3, labels, EDGES, min_q)
        assert (res[0] == lit[0]).all() and (res[1] == lit[1]).all() and res[3] == lit[3], min_q
        assert all((res[2][t] == lit[2][t]).all() for t in (0, 2))
        check_keep_identities(res[0], res[1], EDGES, min_q, fin_lane, fin_tiles, qhist=qhist, sum_singles=res[3],
                              masks=res[2], labels=labels)
    with pytest.raises(AssertionError):                                # an identity that fails is noticed
        bad = lane.copy()
        bad[4] += 1
        check_keep_identities(bad, trow, EDGES, 15, fin_lane, fin_tiles, qhist=qhist)
    with pytest.raises(AssertionError):
        bad = lane.copy()
        bad[7] += 1
        check_keep_identities(bad, trow, EDGES, 15)
    # clusters: at K = 4 everything is one cluster of 11 wells rooted at well 0; wells 1 and 4 tie at 120, well 1 wins
    near_lane, near_tiles, all_one = lane_near_dups(tiles, 6, 3, 4)
    got = lane_keep(tiles, 6, 3, all_one, EDGES, 15)
    assert got[0].tolist() == [11, 1, 10, 1, 120, 700, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0]
    assert got[2][0].tolist() == [0, 1, 0, 0, 0, 0] and not got[2][2].any()
    lit = lane_keep_literal(tiles, 6, 3, all_one, EDGES, 15)
    assert (got[0] == lit[0]).all() and (got[1] == lit[1]).all()
    check_keep_identities(got[0], got[1], EDGES, 15, np.concatenate([near_lane[:6], near_lane[7:]]), near_tiles, qhist=qhist,
                          sum_singles=got[3])


# ---- the filter writer ----------------------------------------------------------------------------
def test_filter_writer_round_trip_through_bcl_tile(tmp_path):
    lane_dir = tmp_path / "run" / "Data" / "Intensities" / "BaseCalls" / "L003"
    lane_dir.mkdir(parents=True)
    rng = np.random.default_rng(3)
    filt = rng.integers(0, 4, 1001).astype(np.uint8)                   # bit 1 is kept as it is
    filt[:4] = [0, 1, 2, 3]
    with open(lane_dir / "s_3_1101.filter", "wb") as fh:
        fh.write(struct.pack("<III", 0, 3, filt.size) + filt.tobytes())
    tile = bcl.Tile(str(lane_dir), "1101")
    mask = ((filt & 1) & rng.integers(0, 2, filt.size)).astype(np.uint8)
    mask[:4] = [0, 0, 0, 1]
    paths = cwd.write_lane_keep_filters(str(tmp_path / "out"), "3", {"1101": tile}, {"1101": mask})
    assert paths == [str(tmp_path / "out" / "L003" / "s_3_1101.filter")]
    raw = open(paths[0], "rb").read()
    assert raw[:12] == struct.pack("<III", 0, 3, 1001) and len(raw) == 12 + 1001
    back = bcl.Tile(str(tmp_path / "out" / "L003"), "1101")
    assert back.num_clusters == 1001
    got = back.read_filter()
    assert (got & 1 == mask).all() and (got & 0xFE == filt & 0xFE).all() and got[:4].tolist() == [0, 0, 2, 3]
    assert cwd.write_lane_keep_filters(str(tmp_path / "out"), "L003", {"1101": tile}, {"1101": mask}) == paths
    with pytest.raises(ValueError):
        cwd.write_keep_filter(str(tmp_path / "x.filter"), filt, mask[:-1])


# ---- the report -----------------------------------------------------------------------------------
def _counts(min_q=15, k=0):
    tiles = hand_made_lane()
    labels = lane_dups(tiles, 6, 3)[2]
    lane, trow, _, _ = lane_keep(tiles, 6, 3, labels, EDGES, min_q)
    return report.LaneKeepCounts.from_rows(lane, trow, ["1101", None, "1103"], k, min_q, EDGES, 4)


def _text(counts, verbose=True):
    out = io.StringIO()
    report.write_lane_keep("3", counts, verbose=verbose, out=out)
    return out.getvalue()


BLOCK = [
    "",
    # tile 1101: 320 / (3 x 4) and 80 / (2 x 4); tile 1103: 190 / 12 and 230 / 12
    "LaneKeep: 3\tTile: 1101\tPF: 5\tKept: 3\tDropped: 2 (0.40000)\tMovedIn: 0\tMeanScore kept: 26.667\tdropped: 10.000",
    "LaneKeep: 3\tTile: 1103\tPF: 6\tKept: 3\tDropped: 3 (0.50000)\tMovedIn: 1\tMeanScore kept: 15.833\tdropped: 19.167",
    "LaneKeepSummary: 3\tTiles: 2\tHamming: 0\tMinQ: 15\tCycles: 4\tWeights: 0,0,20,30\tPF: 11\tKept: 6 (0.54545)\t"
    "Dropped: 5 (0.45455)\tFamilies: 3\tMoved: 1 (0.33333 of Families)",
    # 510 / (6 x 4), 200 / (3 x 4), 310 / (5 x 4)
    "Mean score per base\tkept wells: 21.250\tfirst wells of families: 16.667\tdropped wells: 15.500",
    "FamiliesByGain: 0: 2\t1-9: 0\t10-19: 0\t20-49: 0\t50-99: 0\t100-199: 1\t200-499: 0\t500+: 0",
    "",
]


def test_write_lane_keep_every_line():
    assert _text(_counts()).split("\n") == BLOCK
    short = _text(_counts(), verbose=False).split("\n")
    assert short == [line for line in BLOCK if not line.startswith("LaneKeep: ")]
    ham = _text(_counts(k=2))
    assert "\tHamming: 2\t" in ham
    c = _counts()
    assert c.weights == [0, 0, 20, 30] and (c.pf, c.kept, c.dropped, c.moved_in) == (11, 6, 5, 1)
    assert c.gains == [2, 0, 0, 0, 0, 1, 0, 0] and c.tiles["1103"] == [6, 3, 3, 1, 190, 230] and sorted(c.tiles) == ["1101", "1103"]


def test_write_lane_keep_of_an_empty_lane():
    empty = report.LaneKeepCounts.from_rows([0] * 17, [[0] * 6], ["1101"], 0, 15, [0], 0)
    lines = _text(empty).split("\n")
    assert lines[1] == "LaneKeep: 3\tTile: 1101\tPF: 0\tKept: 0\tDropped: 0 (0.00000)\tMovedIn: 0\tMeanScore kept: n/a\tdropped: n/a"
    assert "Kept: 0 (0.00000)" in lines[2] and "Moved: 0 (0.00000 of Families)" in lines[2] and "Weights: 0\t" in lines[2]
    assert lines[3] == "Mean score per base\tkept wells: n/a\tfirst wells of families: n/a\tdropped wells: n/a"
