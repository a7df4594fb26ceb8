"""Near-duplicate read clusters of a lane without a GPU: the host reference the GPU tests compare against (its
two edge methods and two row methods against each other and against a hand-worked lane), the C ABI and its
scratch arithmetic, the CLI's flag checks, the report block and the TSV."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from lanedups_ref import lane_dups
from lanenear_ref import (HAND, NEAR_LANE_COLS, NEAR_PAIRS, check_near_identities, coarser, hand_made_lane,
                          lane_near_dups, near_row)
from tiledups_ref import INVALID
from well_duplicates_amd import _lib, report
from well_duplicates_amd import count_well_duplicates as cwd

HEADER = os.path.join(_lib.INCLUDE, "welldup_lanenear.h")


# ---- the host reference -------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2])
def test_references_give_the_hand_worked_answer(k):
    tiles = hand_made_lane()
    for order in (tiles, tiles[::-1]):
        for method in ("all_pairs",) + (("deletion",) if k else ()):
            for rows in ("arrays", "literal"):
                lane, trow, labels = lane_near_dups(order, 4, 5, k, method=method, rows=rows)
                assert lane.tolist() == HAND[k]["lane"]
                assert trow.tolist() == HAND[k]["tiles"]
                assert labels.tolist() == HAND[k]["labels"]
                check_near_identities(lane, trow)
    assert coarser(HAND[0]["labels"], HAND[1]["labels"]) and coarser(HAND[1]["labels"], HAND[2]["labels"])
    assert not coarser(HAND[2]["labels"], HAND[1]["labels"])


def _random_lane(seed, n, L, n_tiles, max_tiles):
    """Random reads, copies at 0..3 mismatches planted anywhere on the lane (chains included), N calls, a filter."""
    rng = np.random.default_rng(seed)
    index = sorted(rng.choice(max_tiles, n_tiles, replace=False).tolist())
    m = n_tiles * n
    reads = rng.integers(1, 256, (m, L)).astype(np.uint8)
    reads[rng.random(reads.shape) < 0.01] = 0
    for d in (0, 1, 2, 3, 1):
        src, dst = rng.choice(m, m // 12, replace=False), rng.choice(m, m // 12, replace=False)
        reads[dst] = reads[src]
        for c in range(d):                                             # up to d cycles moved to another base
            col = rng.integers(0, L, dst.size)
            reads[dst, col] = (reads[dst, col] & 0xFC) | ((reads[dst, col] + 1) & 3) | 4
    filt = (rng.random(m) < 0.85).astype(np.uint8) | (rng.integers(0, 2, m).astype(np.uint8) << 1)
    return [(ti, [np.ascontiguousarray(reads[i * n:(i + 1) * n, c]) for c in range(L)], filt[i * n:(i + 1) * n])
            for i, ti in enumerate(index)]


@pytest.mark.parametrize("L", [4, 9, 25])
def test_the_methods_agree_on_random_lanes(L):
    n, max_tiles = 250, 6
    tiles = _random_lane(11 + L, n, L, 4, max_tiles)
    eq_lane, eq_tiles, eq_labels = lane_dups(tiles, n, max_tiles)
    got0 = lane_near_dups(tiles, n, max_tiles, 0)
    assert (got0[0] == near_row(eq_lane, 0)).all() and (got0[1] == eq_tiles).all() and (got0[2] == eq_labels).all()
    last = eq_labels
    for k in (1, 2):
        results = [lane_near_dups(tiles, n, max_tiles, k, method=m, rows=r)
                   for m in ("all_pairs", "deletion") for r in ("arrays", "literal")]
        for lane, trow, labels in results[1:]:
            assert (lane == results[0][0]).all() and (trow == results[0][1]).all() and (labels == results[0][2]).all()
        lane, trow, labels = results[0]
        assert lane.shape == (NEAR_LANE_COLS,)
        check_near_identities(lane, trow)
        assert coarser(last, labels)
        if L > 4:                                                      # (four cycles: nearly everything is within one)
            assert lane[NEAR_PAIRS] > 20 and lane[4] > 20 and lane[3] > got0[0][3]
        last = labels
    never = sorted(set(range(max_tiles)) - {t[0] for t in tiles})
    assert (trow[never] == 0).all() and (labels[never] == INVALID).all()


# ---- C ABI --------------------------------------------------------------------------------------
def test_lanenear_header_and_binding_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert '#include "welldup_lanedups.h"' in text
    syms = sorted(set(re.findall(r"\b(wd_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.LANENEAR_PROTOTYPES) == ["wd_lane_near_dups_finish", "wd_lane_near_dups_scratch"]
    assert int(re.search(r"#define WD_LANENEAR_MAX_K (\d+)", text).group(1)) == _lib.LANENEAR_MAX_K == _lib.TILENEAR_MAX_K
    assert "#define WD_LANENEAR_LANE_COLS (7 + WD_DUPSET_SIZE_BINS)" in text
    assert _lib.LANENEAR_LANE_COLS == NEAR_LANE_COLS == report.LANE_NEAR_ROW_COLS
    for kernel in ("k_ln_bucket", "k_ln_bound", "k_ln_scatter", "k_ln_pairs", "k_ln_pairs_long", "k_ln_compress",
                   "k_ln_members"):
        assert _lib.unit_of_kernel(kernel) == "tiledups"
    deps = {os.path.basename(f) for f in _lib._deps(os.path.join(_lib.CSRC, "welldup_tiledups.hip"))}
    assert {"lane_near.inc", "welldup_lanenear.h", "lane_dups.inc", "tile_near.inc", "near_core.inc", "read_classes.inc"} <= deps
    _lib.build()
    lib = _lib.load()
    for s in syms:
        assert getattr(lib, s).argtypes == _lib.LANENEAR_PROTOTYPES[s][1]
    assert _lib.build_ids()["tiledups"] == _lib.source_unit_ids()["tiledups"]


def _formula(N, tiles, k):
    """The arithmetic include/welldup_lanenear.h states."""
    up = lambda v: (v + 255) // 256 * 256
    return 0 if k == 0 else up(64) + up(512) + up(4 * tiles * N)


def _scratch(lib, N, tiles, L, k):
    b = ctypes.c_size_t()
    rc = lib.wd_lane_near_dups_scratch(N, tiles, L, k, ctypes.byref(b))
    return rc, b.value


def test_scratch_size_needs_no_gpu_and_matches_the_header():
    _lib.build()
    lib = _lib.load()
    text = open(HEADER).read()
    for piece in ("k == 0:  0", "64 ", "+ 512", "+ 4 * W", "W = max_tiles * N", "rounded up to 256 bytes"):
        assert piece in text, piece
    for N, tiles, L in [(2640, 7, 40), (1000, 3, 4), (1001, 3, 151), (4309253, 112, 151), (7, 1, 10), (0, 3, 5), (5, 0, 5)]:
        for k in range(4):
            assert _scratch(lib, N, tiles, L, k) == (0, _formula(N, tiles, k)), (N, tiles, L, k)
    # the HiSeq 4000 lane, 151 cycles, K = 2: 112 x 4 309 253 wells of four bytes, and 768 bytes in front of them
    W = 112 * 4309253
    assert W == 482636336
    assert _scratch(lib, 4309253, 112, 151, 2) == (0, 1930546176) and 1930546176 == 768 + (4 * W + 255) // 256 * 256
    # errors as wd_lane_dups_workspace, and k outside 0..3
    assert _scratch(lib, 4309253, 997, 50, 1)[0] == _lib.ERR_UNSUPPORTED
    assert _scratch(lib, 10, 2, 1025, 1)[0] == _lib.ERR_UNSUPPORTED
    assert _scratch(lib, 65537, 65535, 10, 1)[0] == _lib.ERR_UNSUPPORTED
    for bad in ((-1, 2, 10, 1), (10, -1, 10, 1), (10, 2, -1, 1), (10, 2, 10, -1), (10, 2, 10, 4)):
        assert _scratch(lib, *bad)[0] == _lib.ERR_ARG, bad
    assert lib.wd_lane_near_dups_scratch(10, 1, 10, 1, None) == _lib.ERR_ARG
    # a null handle or row is refused before anything is looked at
    row = (ctypes.c_int64 * 64)()
    assert lib.wd_lane_near_dups_finish(None, 1, None, 0, 0, row, row, None, row, row, None) == _lib.ERR_ARG


# ---- CLI ----------------------------------------------------------------------------------------
def test_cli_flag_checks(tmp_path, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["-s", "hiseq_4000", "-r", str(tmp_path), "--all-wells"]
    args = cwd.parse_args(base + ["--lane-dups", "--lane-dups-hamming", "2", "--lane-dups-pair-budget", "5000"])
    assert args.lane_dups and args.lane_dups_hamming == 2 and args.lane_dups_pair_budget == 5000
    args = cwd.parse_args(base + ["--lane-dups"])
    assert args.lane_dups_hamming is None and args.lane_dups_pair_budget == 0
    for extra, message in ((["--lane-dups-hamming", "1"], "--lane-dups-hamming needs --lane-dups"),
                           (["--tile-dups", "--lane-dups-hamming", "1"], "--lane-dups-hamming needs --lane-dups"),
                           (["--lane-dups", "--lane-dups-hamming", "0"], "--lane-dups-hamming takes 1..3"),
                           (["--lane-dups", "--lane-dups-hamming", "4"], "--lane-dups-hamming takes 1..3"),
                           (["--lane-dups", "--lane-dups-pair-budget", "9"],
                            "--lane-dups-pair-budget needs --lane-dups-hamming"),
                           (["--lane-dups", "--lane-dups-hamming", "1", "--lane-dups-pair-budget", "-1"],
                            "--lane-dups-pair-budget must not be negative")):
        with pytest.raises(SystemExit):
            cwd.parse_args(base + extra)
        assert message in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cwd.parse_args(base + ["--lane-dups", "--lane-dups-hamming", "1"])
    err = " ".join(capsys.readouterr().err.split())
    assert "--lane-dups runs in a single process only" in err and "WORLD_SIZE" in err


def test_cli_help_names_the_new_options(capsys):
    with pytest.raises(SystemExit):
        cwd.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--lane-dups-hamming K" in text and "--lane-dups-pair-budget N" in text and "cluster_tile" in text


def test_the_scratch_counts_when_a_lane_is_fitted():
    cwd.check_lane_dups_fits(1000, 1500, 2, 3, 4, scratch=500)
    with pytest.raises(MemoryError) as e:
        cwd.check_lane_dups_fits(1000, 1500, 2, 3, 4, scratch=501)
    msg = str(e.value)
    assert "1501 bytes, 501 of them for --lane-dups-hamming" in msg and "1500 bytes" in msg


# ---- report -------------------------------------------------------------------------------------
NAMES = ["1101", "1102", "1103", None, "1105"]


def test_lane_near_counts_decode():
    c = report.LaneNearCounts.from_rows(HAND[1]["lane"], HAND[1]["tiles"], NAMES)
    assert (c.pf, c.classes, c.in_classes, c.redundant, c.cross_tile_classes, c.tile_spans, c.near_pairs) == \
        (15, 5, 12, 7, 4, 11, 5)
    assert c.sizes == [4, 0, 1, 0, 0, 0, 0, 0] and sorted(c.tiles) == ["1101", "1102", "1103", "1105"]
    assert (c.within_tiles, c.across_tiles) == (1, 6) and c.lane_duplication() == 7 / 15
    assert c.to_rows() == (HAND[1]["lane"], [HAND[1]["tiles"][i] for i in (0, 1, 2, 4)])
    with pytest.raises(AssertionError):
        report.LaneNearCounts.from_rows(HAND[1]["lane"][:-1], HAND[1]["tiles"], NAMES)


def test_write_lane_near_dups_text():
    near = report.LaneNearCounts.from_rows(HAND[1]["lane"], HAND[1]["tiles"], NAMES)
    eq0 = HAND[0]["lane"]
    equal = report.LaneDupCounts.from_rows(eq0[:NEAR_PAIRS] + eq0[NEAR_PAIRS + 1:], HAND[0]["tiles"], NAMES)
    out = io.StringIO()
    report.write_lane_near_dups("3", 1, near, verbose=True, out=out, equal=equal)
    size = report.library_size(15, 8)
    assert out.getvalue() == (
        "\n"
        "LaneNearDups: 3\tTile: 1101\tHamming: 1\tPF wells: 4\tInLane: 4\tInTile: 0\tTileRedundant: 0\tLaneRedundant: 0\n"
        "LaneNearDups: 3\tTile: 1102\tHamming: 1\tPF wells: 4\tInLane: 3\tInTile: 0\tTileRedundant: 0\tLaneRedundant: 3\n"
        "LaneNearDups: 3\tTile: 1103\tHamming: 1\tPF wells: 4\tInLane: 3\tInTile: 2\tTileRedundant: 1\tLaneRedundant: 2\n"
        "LaneNearDups: 3\tTile: 1105\tHamming: 1\tPF wells: 3\tInLane: 2\tInTile: 0\tTileRedundant: 0\tLaneRedundant: 2\n"
        "LaneNearDupsSummary: 3\tTiles: 4\tHamming: 1\tPF wells: 15\tClusters: 5\tInClusters: 12 (0.80000)\t"
        "Redundant: 7 (0.46667)\tCrossTileClusters: 4\tTileSpans: 11\tNearPairs: 5\n"
        "ClusterSizes: 2: 4\t3: 0\t4: 1\t5: 0\t6: 0\t7: 0\t8: 0\t>=9: 0\n"
        "Redundant within tiles: 1 (0.14286 of Redundant)\tacross tiles: 6 (0.85714 of Redundant)\n"
        "Lane duplication at Hamming <= 1 (Redundant/PF wells): 46.67%\tby equality: 13.33%\n"
        "Estimated library size (distinct/X = 1 - exp(-PF/X)): " + "%.0f" % size + "\n")
    out = io.StringIO()
    report.write_lane_near_dups("1", 2, report.LaneNearCounts.from_rows([500] + [0] * 14, [[500, 0, 0, 0, 0]], ["1101"]),
                                verbose=False, out=out)
    assert out.getvalue() == (
        "\n"
        "LaneNearDupsSummary: 1\tTiles: 1\tHamming: 2\tPF wells: 500\tClusters: 0\tInClusters: 0 (0.00000)\t"
        "Redundant: 0 (0.00000)\tCrossTileClusters: 0\tTileSpans: 0\tNearPairs: 0\n"
        "ClusterSizes: 2: 0\t3: 0\t4: 0\t5: 0\t6: 0\t7: 0\t8: 0\t>=9: 0\n"
        "Redundant within tiles: 0 (0.00000 of Redundant)\tacross tiles: 0 (0.00000 of Redundant)\n"
        "Lane duplication at Hamming <= 2 (Redundant/PF wells): 0.00%\n"
        "Estimated library size (distinct/X = 1 - exp(-PF/X)): n/a\n")


# ---- TSV ----------------------------------------------------------------------------------------
def test_lane_cluster_members_tsv(tmp_path):
    classes = np.array(HAND[0]["labels"], dtype=np.uint32)
    clusters = np.array(HAND[1]["labels"], dtype=np.uint32)
    got = cwd.lane_cluster_members(classes, clusters)
    assert got[0].tolist() == [0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 4, 4]
    assert got[1].tolist() == [0, 1, 2, 3, 0, 2, 3, 0, 2, 3, 1, 2]
    path = str(tmp_path / "lane.tsv")
    cwd.write_lane_members(path, {"2": (NAMES,) + got})
    assert open(path).read().splitlines() == [
        "lane\ttile\twell\tclass_tile\tclass_well\tcluster_tile\tcluster_well",
        "2\t1101\t0\t1101\t0\t1101\t0", "2\t1101\t1\t1101\t1\t1101\t1", "2\t1101\t2\t1101\t2\t1101\t2",
        "2\t1101\t3\t1101\t3\t1101\t3", "2\t1102\t0\t1102\t0\t1101\t0", "2\t1102\t2\t1102\t2\t1101\t1",
        "2\t1102\t3\t1102\t3\t1101\t3", "2\t1103\t0\t1103\t0\t1101\t0", "2\t1103\t2\t1103\t2\t1103\t2",
        "2\t1103\t3\t1103\t3\t1103\t2", "2\t1105\t1\t1101\t2\t1101\t2", "2\t1105\t2\t1101\t0\t1101\t0"]
    # without cluster columns the file is what it was
    cwd.write_lane_members(path, {"2": (NAMES,) + cwd.lane_members(classes)})
    assert open(path).read().splitlines() == ["lane\ttile\twell\tclass_tile\tclass_well", "2\t1101\t0\t1101\t0",
                                              "2\t1101\t2\t1101\t2", "2\t1105\t1\t1101\t2", "2\t1105\t2\t1101\t0"]
