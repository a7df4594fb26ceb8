"""How far apart a lane's duplicate copies lie, without a GPU: the host reference the GPU tests compare against on a
hand-made lane whose every output is written out and against the header's identities, the C ABI and its scratch
arithmetic, the CLI's flag checks, the report block and the fit check."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from lanedistance_ref import (DIST_BINS, EDGES, LANE_COLS, MAX_COORD, MAX_RADIUS, TILE_COLS, check_distance_identities,
                              dist_bin, lane_distances)
from well_duplicates_amd import _lib, report, workload
from well_duplicates_amd import count_well_duplicates as cwd

HEADER = os.path.join(_lib.INCLUDE, "welldup_lanedistance.h")
NO = 0xFFFFFFFF


# ---- the host reference -------------------------------------------------------------------------
# Three tile indices of six wells; index 1 was never added.  The wells lie at
#   well   0        1         2          3           4            5
#   (x,y)  (0, 0)   (10, 0)   (100, 0)   (1000, 0)   (20000, 0)   (40, 30)
# tile 0 (ids 0..5):    1, 2 and 4 are copies of 0: q = 100 (bin 0), 10 000 (bin 2: 4096 <= q < 16 384) and 4 x 10^8
#                       (bin 10: >= 2^28); 3 is not PF; 5 is its own root.
# tile 2 (ids 12..17):  12 is a copy of 0 and 13 of 5: cross-tile, roots on tile 0; 14 is its own root; 15 and 17 are
#                       copies of 14 (well 2): q = 900^2 = 810 000 (bin 5: 2^18 <= q < 2^20) and 60^2 + 30^2 = 4500
#                       (bin 2); 16 is not PF.
HAND_X = [0, 10, 100, 1000, 20000, 40]
HAND_Y = [0, 0, 0, 0, 0, 30]
HAND_LABELS = [0, 0, 0, NO, 0, 5] + [NO] * 6 + [0, 5, 14, 14, NO, 14]
HAND_DIST = [1, 0, 2, 0, 0, 1, 0, 0, 0, 0, 1]
HAND_PAIRS = [[3, 0, 2], [0, 0, 0], [0, 0, 2]]
HAND = {      # radius -> (Local of the lane, tile rows): q < R^2, strictly
    0: (0, [[3, 3, 0], [0, 0, 0], [4, 2, 0]]),
    10: (0, [[3, 3, 0], [0, 0, 0], [4, 2, 0]]),                        # q = 100 is not < 100
    11: (1, [[3, 3, 1], [0, 0, 0], [4, 2, 0]]),
    100: (2, [[3, 3, 1], [0, 0, 0], [4, 2, 1]]),                       # 100 and 4500; q = 10 000 is not < 10 000
    101: (3, [[3, 3, 2], [0, 0, 0], [4, 2, 1]]),
    2500: (4, [[3, 3, 2], [0, 0, 0], [4, 2, 2]]),                      # and 810 000
    MAX_RADIUS: (5, [[3, 3, 3], [0, 0, 0], [4, 2, 2]]),
}


@pytest.mark.parametrize("radius", sorted(HAND))
def test_reference_gives_the_hand_worked_answer(radius):
    local, tiles = HAND[radius]
    lane, trow, pairs = lane_distances(HAND_LABELS, 6, 3, HAND_X, HAND_Y, radius)
    assert lane.tolist() == [7, 5, local] + HAND_DIST and trow.tolist() == tiles and pairs.tolist() == HAND_PAIRS
    # (the rows of the finish these labels belong to: ten PF wells in three classes, all ten in them, Redundant 7; on
    # tile 2 wells 12 and 13 have no classmate before them: TileRedundant 2 of LaneRedundant 4)
    check_distance_identities(lane, trow, pairs, radius, [10, 3, 10, 7, 2, 5], [[5, 5, 4, 3, 3], [0] * 5, [5, 5, 3, 2, 4]],
                              local_at=lambda r: lane_distances(HAND_LABELS, 6, 3, HAND_X, HAND_Y, r)[0][2])


def test_the_bins_by_their_edges():
    assert dist_bin([0, 1023, 1024, 4095, 4096, (1 << 28) - 1, 1 << 28, (1 << 49) - 1]).tolist() == [0, 0, 1, 1, 2, 9, 10, 10]
    for j, edge in enumerate(EDGES):                                   # a distance of 32 x 2^j is the first of bin j + 1
        assert dist_bin([edge * edge - 1, edge * edge]).tolist() == [j, j + 1]
    assert len(EDGES) == DIST_BINS - 1 and EDGES[-1] == 16384


def test_reference_identities_on_a_random_lane():
    n, max_tiles = 500, 5
    rng = np.random.default_rng(21)
    x, y = rng.integers(0, 40000, n), rng.integers(0, 90000, n)
    x[:3], y[:3] = [0, MAX_COORD, 5], [0, MAX_COORD, 5]
    labels = np.full(max_tiles * n, NO, dtype=np.uint32)
    for ti in (0, 2, 3):
        ids = np.arange(ti * n, (ti + 1) * n)
        pf = rng.random(n) < 0.9
        labels[ids[pf]] = ids[pf]
    labels[0], labels[1] = 0, 0                                        # the longest distance there is: q = 2 (2^24 - 1)^2
    for g in np.flatnonzero(labels != NO)[::7].tolist():               # pairs only: a root stays a root
        r = int(rng.integers(0, g)) if g else 0
        if labels[r] == r and r != g and labels[g] == g and not (labels == g).sum() > 1:
            labels[g] = r
    got = {r: lane_distances(labels, n, max_tiles, x, y, r) for r in (0, 32, 33, 2500, 40000, MAX_RADIUS)}
    local_at = lambda r: lane_distances(labels, n, max_tiles, x, y, r)[0][2]
    for r, res in got.items():
        check_distance_identities(*res, r, local_at=local_at)
        assert (res[0][3:] == got[0][0][3:]).all() and (res[2] == got[0][2]).all()      # Dist does not depend on the radius
    lane = got[2500][0]
    assert lane[0] > 100 and 0 < lane[1] < lane[0] and lane[13] >= 1 and np.triu(got[0][2], 1).sum() == lane[0] - lane[1]
    literal = sum(1 for g in np.flatnonzero((labels != NO) & (labels != np.arange(labels.size))).tolist()
                  if g // n == labels[g] // n and
                  (int(x[g % n]) - int(x[labels[g] % n])) ** 2 + (int(y[g % n]) - int(y[labels[g] % n])) ** 2 < 2500 ** 2)
    assert literal == lane[2]                                          # the same read off pair by pair


# ---- C ABI --------------------------------------------------------------------------------------
def test_lanedistance_header_and_binding_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert '#include "welldup_lanemismatch.h"' in text
    syms = sorted(set(re.findall(r"\b(wd_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.LANEDISTANCE_PROTOTYPES) == ["wd_lane_distance_scratch", "wd_lane_distances"]
    assert int(re.search(r"#define WD_LANEDISTANCE_DIST_BINS\s+(\d+)", text).group(1)) == _lib.LANEDISTANCE_DIST_BINS == DIST_BINS
    assert re.search(r"#define WD_LANEDISTANCE_LANE_COLS\s+\(3 \+ WD_LANEDISTANCE_DIST_BINS\)", text)
    assert int(re.search(r"#define WD_LANEDISTANCE_TILE_COLS\s+(\d+)", text).group(1)) == _lib.LANEDISTANCE_TILE_COLS == TILE_COLS
    assert re.search(r"#define WD_LANEDISTANCE_MAX_COORD\s+\(\(1 << 24\) - 1\)", text) and _lib.LANEDISTANCE_MAX_COORD == MAX_COORD
    assert re.search(r"#define WD_LANEDISTANCE_MAX_RADIUS\s+\(1 << 25\)", text) and _lib.LANEDISTANCE_MAX_RADIUS == MAX_RADIUS
    assert int(re.search(r"#define WD_LANEDISTANCE_MATRIX_MAX_TILES\s+(\d+)", text).group(1)) == _lib.LANEDISTANCE_MATRIX_MAX_TILES
    assert _lib.LANEDISTANCE_LANE_COLS == LANE_COLS == report.LANE_DISTANCE_LANE_COLS == 14
    assert report.LANE_DISTANCE_TILE_COLS == TILE_COLS and report.LANE_DISTANCE_MAX_RADIUS == MAX_RADIUS
    assert len(report.LANE_DISTANCE_DIST_NAMES) == DIST_BINS and report.LANE_DISTANCE_EDGES == EDGES
    taken = set()
    for table in (_lib.PROTOTYPES, _lib.SETS_PROTOTYPES, _lib.TILEDUPS_PROTOTYPES, _lib.TILENEAR_PROTOTYPES,
                  _lib.LANEDUPS_PROTOTYPES, _lib.LANENEAR_PROTOTYPES, _lib.LANEINDEX_PROTOTYPES, _lib.LANEMISMATCH_PROTOTYPES):
        taken |= set(table)
    assert not set(_lib.LANEDISTANCE_PROTOTYPES) & taken and "wd_lane_distances" not in _lib.PROTOTYPES
    source = open(os.path.join(_lib.CSRC, "lane_distance.inc")).read()
    assert "k_lg_tally" in source and _lib.unit_of_kernel("k_lg_tally") == "tiledups"
    deps = {os.path.basename(f) for f in _lib._deps(os.path.join(_lib.CSRC, "welldup_tiledups.hip"))}
    assert {"lane_distance.inc", "welldup_lanedistance.h", "lane_mismatch.inc", "welldup_lanemismatch.h", "lane_dups.inc"} <= deps
    unit = open(os.path.join(_lib.CSRC, "welldup_tiledups.hip")).read()
    assert unit.index('#include "lane_mismatch.inc"') < unit.index('#include "lane_distance.inc"')
    assert "lane_distance.inc\n// (last)" in unit and "lane_mismatch.inc (last)" not in unit      # the unit's head comment
    _lib.build()
    lib = _lib.load()
    for s in syms:                                                     # exported, and bound as the table says
        assert getattr(lib, s).argtypes == _lib.LANEDISTANCE_PROTOTYPES[s][1]
    ids = _lib.build_ids()
    assert ids["tiledups"] == _lib.source_unit_ids()["tiledups"] and ids["all"] == _lib.source_build_id()


def _formula(n, tiles, matrix):
    """The arithmetic include/welldup_lanedistance.h states."""
    up = lambda v: (v + 255) // 256 * 256
    return up(8 * n) + up(1536 * tiles) + 8192 + up(4 * tiles) + (up(8 * tiles * tiles) if matrix else 0)


def _scratch(lib, n, tiles, matrix):
    b = ctypes.c_size_t()
    rc = lib.wd_lane_distance_scratch(n, tiles, matrix, ctypes.byref(b))
    return rc, b.value


def test_scratch_size_needs_no_gpu_and_matches_the_header():
    _lib.build()
    lib = _lib.load()
    text = open(HEADER).read()
    for piece in ("8 * N", "+ 1536 * max_tiles", "+ 8192", "+ 4 * max_tiles", "+ 8 * max_tiles * max_tiles",
                  "rounded up to 256 bytes", "34 758 400 bytes"):
        assert piece in text, piece
    for n in (0, 1, 31, 32, 33, 2640, 9000, 4309650, (1 << 32) - 2):
        for tiles in (0, 1, 3, 7, 64, 65, 112, 4096):
            for matrix in (0, 1):
                assert _scratch(lib, n, tiles, matrix) == (0, _formula(n, tiles, matrix)), (n, tiles, matrix)
    assert _scratch(lib, 4309650, 112, 1) == (0, 34758400)             # the header's HiSeq 4000 lane
    assert _scratch(lib, 10, 4097, 0) == (0, _formula(10, 4097, 0)) and _scratch(lib, 10, 65535, 0)[0] == 0
    assert _scratch(lib, 10, 4097, 1)[0] == _lib.ERR_UNSUPPORTED and _scratch(lib, 10, 65536, 0)[0] == _lib.ERR_UNSUPPORTED
    assert _scratch(lib, -1, 3, 0)[0] == _lib.ERR_ARG and _scratch(lib, 10, -1, 1)[0] == _lib.ERR_ARG
    assert lib.wd_lane_distance_scratch(10, 3, 1, None) == _lib.ERR_ARG
    row = (ctypes.c_int64 * 32)()                                      # a null handle is refused before anything is looked at
    xy = (ctypes.c_int32 * 8)()
    assert lib.wd_lane_distances(None, xy, xy, 5, None, 0, row, row, row) == _lib.ERR_ARG


# ---- CLI ----------------------------------------------------------------------------------------
def test_cli_flag_checks(tmp_path, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["-s", "hiseq_4000", "-r", str(tmp_path), "--all-wells"]
    args = cwd.parse_args(base + ["--lane-dups", "--lane-dups-distance"])
    assert args.lane_dups_distance and args.lane_dups_distance_radius == 2500
    assert cwd.parse_args(base + ["--lane-dups", "--lane-dups-hamming", "2", "--lane-dups-distance",
                                  "--lane-dups-distance-radius", "0"]).lane_dups_distance_radius == 0
    assert cwd.parse_args(base + ["--lane-dups", "--lane-dups-distance", "--lane-dups-distance-radius",
                                  str(1 << 25)]).lane_dups_distance_radius == 1 << 25
    assert not cwd.parse_args(base + ["--lane-dups"]).lane_dups_distance
    for extra, message in ((["--lane-dups-distance"], "--lane-dups-distance needs --lane-dups"),
                           (["--tile-dups", "--lane-dups-distance"], "--lane-dups-distance needs --lane-dups"),
                           (["--lane-dups", "--lane-dups-distance", "--lane-dups-distance-radius", "-1"],
                            "--lane-dups-distance-radius takes 0..33554432, not -1"),
                           (["--lane-dups", "--lane-dups-distance", "--lane-dups-distance-radius", str((1 << 25) + 1)],
                            "--lane-dups-distance-radius takes 0..33554432, not 33554433")):
        with pytest.raises(SystemExit):
            cwd.parse_args(base + extra)
        assert message in " ".join(capsys.readouterr().err.split())
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cwd.parse_args(base + ["--lane-dups", "--lane-dups-distance"])
    assert "--lane-dups runs in a single process only" in " ".join(capsys.readouterr().err.split())


def test_cli_help_names_the_new_options(capsys):
    with pytest.raises(SystemExit):
        cwd.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--lane-dups-distance " in text and "--lane-dups-distance-radius R" in text
    assert "OPTICAL_DUPLICATE_PIXEL_DISTANCE" in text and "int(10 x the s.locs position + 1000.5)" in text
    assert "(default: 2500)" in text


def test_the_distance_scratch_counts_when_a_lane_is_fitted():
    cwd.check_lane_dups_fits(1000, 2000, 2, 3, 4, scratch=500, index=300, mismatch=100, distance=100)
    with pytest.raises(MemoryError) as e:
        cwd.check_lane_dups_fits(1000, 2000, 2, 3, 4, scratch=500, index=300, mismatch=100, distance=101)
    msg = str(e.value)
    assert ("2001 bytes, 500 of them for --lane-dups-hamming, 300 of them for --lane-dups-index, 100 of them for "
            "--lane-dups-mismatches, 101 of them for --lane-dups-distance)") in msg and "2000 bytes" in msg
    with pytest.raises(MemoryError) as e:
        cwd.check_lane_dups_fits(1000, 1050, 2, 3, 4, distance=51)
    assert "(1051 bytes, 51 of them for --lane-dups-distance)" in str(e.value)
    with pytest.raises(MemoryError) as e:                              # without the flag the message is what it was
        cwd.check_lane_dups_fits(1000, 1400, 2, 3, 4, scratch=401)
    assert "(1401 bytes, 401 of them for --lane-dups-hamming)" in str(e.value)


# ---- report -------------------------------------------------------------------------------------
# Six tile indices of a hiseq_4000 lane, index 2 never a tile of it.  Seen from 1101: 1102 is the adjacent tile of its
# swath, 1128 the same swath further on, 1201 the same surface, 2101 the other surface.
NAMES = ["1101", "1102", None, "1128", "1201", "2101"]
FINAL = report.LaneDupCounts(1000, 50, 120, 70, 10, 65, [40, 5, 3, 1, 1, 0, 0, 0],
                             {"1101": [300, 40, 30, 15, 15], "1102": [200, 30, 24, 12, 17], "1128": [100, 15, 12, 8, 10],
                              "1201": [250, 20, 16, 10, 16], "2101": [150, 15, 8, 5, 12]})
LANE_ROW = [70, 50, 42, 20, 6, 4, 0, 3, 2, 5, 4, 3, 2, 1]
TILE_ROWS = [[15, 15, 13], [17, 12, 10], [0, 0, 0], [10, 8, 7], [16, 10, 8], [12, 5, 4]]
TILE_PAIRS = [[15, 5, 0, 1, 3, 4], [0, 12, 0, 1, 2, 1], [0] * 6, [0, 0, 0, 8, 1, 0], [0, 0, 0, 0, 10, 2], [0, 0, 0, 0, 0, 5]]
# uniform~ over an area of 10^8: pi x 1024 / 10^8 = 0.00003, x 3 for the next bin, then x 4 each; 4096-8192 would be
# 1.58 and takes what is left of 1.  By PF wells: 300 x 200 = 60 000 of the 387 500 that all pairs of tiles make;
# 30 000 + 20 000 + 75 000 + 50 000 + 25 000 = 200 000; 150 x 850 = 127 500.
SUMMARY = (
    "LaneDistancesSummary: 3\tTiles: 5\tR: 2500\tPairs: 70\tSameTile: 50 (0.71429)\tLocal: 42 (0.60000)\t"
    "SameTile of the wells with an earlier classmate on their tile: 0.90909\n"
    "Dist (share of SameTile; uniform~: a copy placed uniformly over the tile, an approximation without edges): "
    "<32: 20 (0.40000, uniform~ 0.00003)\t32-64: 6 (0.12000, uniform~ 0.00010)\t64-128: 4 (0.08000, uniform~ 0.00039)\t"
    "128-256: 0 (0.00000, uniform~ 0.00154)\t256-512: 3 (0.06000, uniform~ 0.00618)\t512-1024: 2 (0.04000, uniform~ 0.02471)\t"
    "1024-2048: 5 (0.10000, uniform~ 0.09883)\t2048-4096: 4 (0.08000, uniform~ 0.39530)\t4096-8192: 3 (0.06000, uniform~ 0.47293)\t"
    "8192-16384: 2 (0.04000, uniform~ 0.00000)\t>=16384: 1 (0.02000, uniform~ 0.00000)\n"
    "Cross-tile pairs: 20\tadjacent tile of the swath: 5 (0.25000, by PF wells 0.15484)\t"
    "same surface otherwise: 8 (0.40000, by PF wells 0.51613)\tother surface: 7 (0.35000, by PF wells 0.32903)\n"
    "Estimated library size without local copies (R = 2500; distinct/X = 1 - exp(-(PF - Local)/X)): %s\n")
VERBOSE = (
    "LaneDistances: 3\tTile: 1101\tPairs: 15\tSameTile: 15\tLocal: 13\n"
    "LaneDistances: 3\tTile: 1102\tPairs: 17\tSameTile: 12\tLocal: 10\n"
    "LaneDistances: 3\tTile: 1128\tPairs: 10\tSameTile: 8\tLocal: 7\n"
    "LaneDistances: 3\tTile: 1201\tPairs: 16\tSameTile: 10\tLocal: 8\n"
    "LaneDistances: 3\tTile: 2101\tPairs: 12\tSameTile: 5\tLocal: 4\n")


def test_fixed_counts_as_a_report():
    check_distance_identities(LANE_ROW, TILE_ROWS, TILE_PAIRS, 2500, FINAL.to_rows()[0])
    assert all(n in workload.tiles_for_stype(workload.HISEQ_4000) for n in NAMES if n)
    c = report.LaneDistanceCounts.from_rows(LANE_ROW, TILE_ROWS, TILE_PAIRS, NAMES, 2500, FINAL, 1e8)
    assert (c.pairs, c.same_tile, c.local, c.cross_tile) == (70, 50, 42, 20) and c.dist == LANE_ROW[3:]
    assert c.cross == [5, 8, 7] and sum(c.cross) == c.cross_tile and c.coverage() == 50 / 55
    assert c.cross_by_pf == [60000 / 387500, 200000 / 387500, 127500 / 387500]
    shares = c.uniform_shares()
    assert abs(sum(shares) - 1.0) < 1e-12 and shares[0] == np.pi * 1024 / 1e8 and shares[-2:] == [0.0, 0.0]
    # the corrected estimate is the Lander-Waterman one on PF - Local reads; it lies above the uncorrected one
    size = report.library_size(1000 - 42, 1000 - 70)
    assert c.library_size_without_local() == size and size > FINAL.library_size() > 0
    out = io.StringIO()
    report.write_lane_distances("3", c, verbose=True, out=out)
    assert out.getvalue() == "\n" + VERBOSE + SUMMARY % ("%.0f" % size)
    out = io.StringIO()
    report.write_lane_distances("3", c, out=out)                       # -S: the summary alone
    assert out.getvalue() == "\n" + SUMMARY % ("%.0f" % size)
    nomatrix = report.LaneDistanceCounts.from_rows(LANE_ROW, TILE_ROWS, None, NAMES, 2500, FINAL, 1e8)
    out = io.StringIO()
    report.write_lane_distances("3", nomatrix, out=out)
    assert out.getvalue() == "\n" + "".join(ln + "\n" for ln in (SUMMARY % ("%.0f" % size)).splitlines()
                                            if not ln.startswith("Cross-tile pairs"))


def test_the_cross_tile_categories_on_hiseq_4000_names():
    tiles = workload.tiles_for_stype(workload.HISEQ_4000)
    seen = {0: 0, 1: 0, 2: 0}
    for i, a in enumerate(tiles):
        for b in tiles[i + 1:]:
            cat = report.cross_tile_category(a, b)
            assert cat == report.cross_tile_category(b, a)
            assert cat == (2 if a[0] != b[0] else 0 if a[1] == b[1] and abs(int(a[2:]) - int(b[2:])) == 1 else 1)
            seen[cat] += 1
    assert seen == {0: 4 * 27, 1: 2 * (56 * 55 // 2) - 4 * 27, 2: 56 * 56}
    assert report.cross_tile_category("1101", "1102") == 0 and report.cross_tile_category("1128", "1201") == 1
    assert report.cross_tile_category("1101", "1103") == 1 and report.cross_tile_category("1228", "2228") == 2
    assert report.cross_tile_category("a", "1101") == 2


def test_an_empty_lane_as_a_report():
    c = report.LaneDistanceCounts.from_rows([0] * 14, [[0] * 3], [[0]], ["1101"], 0, report.LaneDupCounts(pf=10), 0.0)
    out = io.StringIO()
    report.write_lane_distances("1", c, verbose=True, out=out)
    text = out.getvalue()
    assert "LaneDistances: 1\tTile: 1101\tPairs: 0\tSameTile: 0\tLocal: 0\n" in text
    assert "\tPairs: 0\tSameTile: 0 (0.00000)\tLocal: 0 (0.00000)\t" in text and "<32: 0 (0.00000, uniform~ 0.00000)" in text
    assert "Cross-tile pairs: 0\tadjacent tile of the swath: 0 (0.00000, by PF wells 0.00000)" in text
    assert text.endswith("Estimated library size without local copies (R = 0; distinct/X = 1 - exp(-(PF - Local)/X)): n/a\n")
    with pytest.raises(AssertionError):
        report.LaneDistanceCounts.from_rows([0] * 13, [[0] * 3], None, ["1101"], 0, report.LaneDupCounts(), 0.0)
    with pytest.raises(AssertionError):
        report.LaneDistanceCounts.from_rows([0] * 14, [[0] * 3], None, ["1101"], (1 << 25) + 1, report.LaneDupCounts(), 0.0)
