"""Near-duplicate read clusters per tile without a GPU: the host reference the GPU tests compare against (its two
methods against each other and against a hand-worked tile), the C ABI of include/welldup_tilenear.h, the CLI's
flag checks, the report block and the TSV."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from tiledups_ref import INVALID, codes_of, tile_dups
from tilenear_ref import (HAND, distinct_reads, edges_all_pairs, edges_by_deletion, grid_rings, hand_made_tile,
                          tile_near_dups)
from well_duplicates_amd import _lib, report
from well_duplicates_amd import count_well_duplicates as cwd

HEADER = os.path.join(_lib.INCLUDE, "welldup_tilenear.h")

@pytest.mark.parametrize("k", [1, 2])
def test_both_references_give_the_hand_worked_answer(k):
    planes, filt, (lvl_off, nbr) = hand_made_tile()
    want = HAND[k]
    for method in ("all_pairs", "deletion"):
        row, labels = tile_near_dups(planes, filt, lvl_off, nbr, k, method=method)
        assert labels.tolist() == want["labels"], method
        assert row[:5].tolist() == want["head"], method              # PF, Clusters, InClusters, Redundant, NearPairs
        assert row[5:7].tolist() == want["local"] and row[7:9].tolist() == want["ring_wells"], method
        assert row[9:].tolist() == want["bins"], method


def test_reference_at_k0_is_the_class_reference():
    planes, filt, (lvl_off, nbr) = hand_made_tile()
    row, labels = tile_near_dups(planes, filt, lvl_off, nbr, 0)
    eq_row, eq_labels = tile_dups(planes, filt, lvl_off, nbr)
    assert (labels == eq_labels).all() and row[4] == 0
    assert (np.delete(row, 4) == eq_row).all()
    assert eq_row[:4].tolist() == [23, 2, 5, 3]                        # {3, 9, 21} and {14, 19}


def _random_tile(seed, n, L, near1, near2):
    rng = np.random.default_rng(seed)
    reads = rng.integers(1, 256, (n, L)).astype(np.uint8)
    reads[rng.random((n, L)) < 0.01] = 0
    src = rng.choice(n, near1 + near2, replace=False)
    dst = rng.choice(np.setdiff1d(np.arange(n), src), near1 + near2, replace=False)
    reads[dst] = reads[src]
    for i, w in enumerate(dst.tolist()):
        for c in rng.choice(L, 1 if i < near1 else 2, replace=False).tolist():
            b = int(reads[w, c])
            reads[w, c] = (b & 0xFC | ((b + 1) & 3)) or 0x41   # another base (or N -> a base)
    exact = rng.choice(n, 40, replace=False)
    reads[exact[20:]] = reads[exact[:20]]
    filt = (rng.random(n) < 0.8).astype(np.uint8)
    return [np.ascontiguousarray(reads[:, c]) for c in range(L)], filt


@pytest.mark.parametrize("k,L", [(1, 2), (1, 25), (2, 3), (2, 25)])
def test_the_two_references_agree_on_random_tiles(k, L):
    n = 1500
    planes, filt = _random_tile(11 * k + L, n, L, 60, 60)
    lvl_off, nbr = grid_rings(30, 50)
    codes = codes_of(planes, n)
    _, reps = distinct_reads(codes, (filt & 1).astype(bool))
    ea, eb = edges_all_pairs(codes, reps, k), edges_by_deletion(codes, reps, k)
    assert sorted(map(tuple, ea.tolist())) == sorted(map(tuple, eb.tolist()))
    if L == 25:
        assert 20 < ea.shape[0] < 200                                  # the planted pairs that passed the filter
    row_a, lab_a = tile_near_dups(planes, filt, lvl_off, nbr, k, method="all_pairs")
    row_b, lab_b = tile_near_dups(planes, filt, lvl_off, nbr, k, method="deletion")
    assert (row_a == row_b).all() and (lab_a == lab_b).all()
    row_0, lab_0 = tile_near_dups(planes, filt, lvl_off, nbr, k - 1)
    same = lab_0[:, None] == lab_0[None, :]                            # clusters at k coarsen those at k - 1
    assert (lab_a[:, None] == lab_a[None, :])[same].all() and row_a[3] >= row_0[3]


# ---- C ABI --------------------------------------------------------------------------------------
def test_tilenear_header_and_binding_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert '#include "welldup_tiledups.h"' in text
    syms = sorted(set(re.findall(r"\b(wd_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.TILENEAR_PROTOTYPES) == ["wd_tile_near_dups", "wd_tile_near_dups_workspace"]
    assert not set(syms) & (set(_lib.PROTOTYPES) | set(_lib.SETS_PROTOTYPES) | set(_lib.TILEDUPS_PROTOTYPES))
    assert int(re.search(r"#define WD_TILENEAR_MAX_K (\d+)", text).group(1)) == _lib.TILENEAR_MAX_K == 3
    for kernel in ("k_tn_fingerprint<true>", "k_tn_bucket", "k_tn_pairs", "k_tn_pairs_long"):
        assert _lib.unit_of_kernel(kernel) == "tiledups"
    _lib.build()
    lib = _lib.load()
    for s in syms:
        assert getattr(lib, s).argtypes == _lib.TILENEAR_PROTOTYPES[s][1]


def test_build_id_covers_the_new_sources():
    deps = {os.path.basename(f) for f in _lib._deps(os.path.join(_lib.CSRC, "welldup_tiledups.hip"))}
    assert {"tile_near.inc", "near_core.inc", "read_classes.inc", "welldup_tilenear.h", "welldup_tiledups.h"} <= deps
    for u in _lib.UNITS[:-1]:
        other = {os.path.basename(f) for f in _lib._deps(os.path.join(_lib.CSRC, "welldup_%s.hip" % u))}
        assert not {"tile_near.inc", "welldup_tilenear.h"} & other
    _lib.build()
    assert _lib.build_ids()["all"] == _lib.source_build_id()
    assert _lib.build_ids()["tiledups"] == _lib.source_unit_ids()["tiledups"]


def test_near_workspace_size_needs_no_gpu():
    _lib.build()
    lib = _lib.load()
    sizes = []
    for k in range(4):
        b = ctypes.c_size_t()
        assert lib.wd_tile_near_dups_workspace(100000, 3, k, ctypes.byref(b)) == 0
        sizes.append(b.value)
    eq = ctypes.c_size_t()
    assert lib.wd_tile_dups_workspace(100000, 3, ctypes.byref(eq)) == 0
    assert sizes[0] == eq.value                                        # k = 0 runs wd_tile_dups
    assert sizes[0] < sizes[1] < sizes[2] < sizes[3]
    for k in (1, 2, 3):                                                # 4 (k + 1) bytes per well on top, and little else
        assert 0 <= sizes[k] - eq.value - 4 * (k + 1) * 300000 < 4096
    b = ctypes.c_size_t()
    for bad in (dict(N=-1), dict(k=-1), dict(k=4), dict(tiles=-1)):
        assert lib.wd_tile_near_dups_workspace(bad.get("N", 10), bad.get("tiles", 1), bad.get("k", 1),
                                               ctypes.byref(b)) == _lib.ERR_ARG
    assert lib.wd_tile_near_dups_workspace(10, 1, 1, None) == _lib.ERR_ARG


# ---- CLI ----------------------------------------------------------------------------------------
def test_cli_flag_checks(tmp_path, capsys):
    base = ["-s", "hiseq_4000", "-r", str(tmp_path), "--all-wells"]
    args = cwd.parse_args(base + ["--tile-dups", "--tile-dups-hamming", "2", "--tile-dups-pair-budget", "5000"])
    assert args.tile_dups_hamming == 2 and args.tile_dups_pair_budget == 5000
    args = cwd.parse_args(base + ["--tile-dups"])
    assert args.tile_dups_hamming is None and args.tile_dups_pair_budget == 0
    for extra, message in ((["--tile-dups-hamming", "1"], "--tile-dups-hamming needs --tile-dups"),
                           (["--tile-dups", "--tile-dups-hamming", "0"], "--tile-dups-hamming takes 1..3"),
                           (["--tile-dups", "--tile-dups-hamming", "4"], "--tile-dups-hamming takes 1..3"),
                           (["--tile-dups", "--tile-dups-hamming", "1", "--tile-dups-pair-budget", "-1"],
                            "--tile-dups-pair-budget must not be negative"),
                           (["--tile-dups", "--tile-dups-pair-budget", "9"],
                            "--tile-dups-pair-budget needs --tile-dups-hamming")):
        with pytest.raises(SystemExit):
            cwd.parse_args(base + extra)
        assert message in capsys.readouterr().err


def test_cli_help_points_to_the_new_option(capsys):
    with pytest.raises(SystemExit):
        cwd.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--tile-dups-hamming K" in text and "--tile-dups-pair-budget N" in text
    assert "a different algorithm and are not offered" not in text            # the old sentence of --tile-dups
    assert "are what --tile-dups-hamming adds" in text
    assert "by edit distance over a whole tile are not offered" in text


# ---- report -------------------------------------------------------------------------------------
def _two_tiles():
    a = report.TileNearCounts.from_block([1000, 22, 50, 28, 6, 12, 33, 300, 900, 18, 3, 0, 0, 0, 0, 0, 1], 2, wells=2001)
    b = report.TileNearCounts.from_block([500, 1, 2, 1, 1, 2, 2, 12, 36, 1, 0, 0, 0, 0, 0, 0, 0], 2, wells=2001)
    return {"1102": b, "1101": a}


def test_tilenear_counts_decode_and_add():
    row = [1000, 22, 50, 28, 6, 12, 33, 300, 900, 18, 3, 0, 0, 0, 0, 0, 1]
    c = report.TileNearCounts.from_block(np.array(row), 2, wells=2001)
    assert (c.pf, c.clusters, c.in_clusters, c.redundant, c.near_pairs) == (1000, 22, 50, 28, 6)
    assert c.local == [12, 33] and c.ring_wells == [300, 900] and c.sizes == [18, 3, 0, 0, 0, 0, 0, 1]
    assert c.even_den == 50 * 2000 and c.to_block() == row
    s = c + _two_tiles()["1102"]
    assert (s.pf, s.clusters, s.in_clusters, s.redundant, s.near_pairs) == (1500, 23, 52, 29, 7)
    assert s.tile_duplication() == 29 / 1500 and s.local_share() == 35 / 52
    z = report.TileNearCounts.zeros(3)
    assert z.levels == 3 and z.tile_duplication() == 0.0 and z.local_share() == 0.0
    with pytest.raises(ValueError):
        c + z
    with pytest.raises(AssertionError):
        report.TileNearCounts.from_block(row[:-1], 2)


def test_write_tile_near_dups_text():
    out = io.StringIO()
    equal = report.TileDupCounts.from_block([1500, 21, 47, 26, 12, 32, 282, 846, 18, 2, 0, 0, 0, 0, 0, 1], 2)
    report.write_tile_near_dups("3", 2, _two_tiles(), verbose=True, out=out, equal=equal)
    assert out.getvalue() == (
        "\n"
        "TileNearDups: 3\tTile: 1101\tHamming: 2\tPF wells: 1000\tClusters: 22\tInClusters: 50\tRedundant: 28\tNearPairs: 6\n"
        "Level: 1\tLocal: 12\tRingWells: 300\n"
        "Level: 2\tLocal: 33\tRingWells: 900\n"
        "TileNearDups: 3\tTile: 1102\tHamming: 2\tPF wells: 500\tClusters: 1\tInClusters: 2\tRedundant: 1\tNearPairs: 1\n"
        "Level: 1\tLocal: 2\tRingWells: 12\n"
        "Level: 2\tLocal: 2\tRingWells: 36\n"
        "TileNearDupsSummary: 3\tTiles: 2\tHamming: 2\tPF wells: 1500\tClusters: 23\tInClusters: 52 (0.03467)\t"
        "Redundant: 29 (0.01933)\tNearPairs: 7\n"
        "Level: 1\tLocal: 14 (0.26923 of InClusters)\tEvenly spread: 0.00300\n"
        "Level: 2\tLocal: 35 (0.67308 of InClusters)\tEvenly spread: 0.00900\n"
        "ClusterSizes: 2: 19\t3: 3\t4: 0\t5: 0\t6: 0\t7: 0\t8: 0\t>=9: 1\n"
        "Tile duplication at Hamming <= 2 (Redundant/PF wells): 1.93%\tby equality: 1.73%\n"
        "Local share at level 2 (Local/InClusters): 67.31%\n")
    out = io.StringIO()
    report.write_tile_near_dups("1", 1, {"1101": report.TileNearCounts.zeros(1)}, verbose=False, out=out)
    assert out.getvalue() == (
        "\n"
        "TileNearDupsSummary: 1\tTiles: 1\tHamming: 1\tPF wells: 0\tClusters: 0\tInClusters: 0 (0.00000)\t"
        "Redundant: 0 (0.00000)\tNearPairs: 0\n"
        "Level: 1\tLocal: 0 (0.00000 of InClusters)\tEvenly spread: 0.00000\n"
        "ClusterSizes: 2: 0\t3: 0\t4: 0\t5: 0\t6: 0\t7: 0\t8: 0\t>=9: 0\n"
        "Tile duplication at Hamming <= 1 (Redundant/PF wells): 0.00%\n"
        "Local share at level 1 (Local/InClusters): 0.00%\n")


def test_cluster_members_tsv(tmp_path):
    planes, filt, (lvl_off, nbr) = hand_made_tile()
    _, classes = tile_dups(planes, filt, lvl_off, nbr)
    _, clusters = tile_near_dups(planes, filt, lvl_off, nbr, 1)
    wells, cl = cwd.set_members(clusters)
    path = str(tmp_path / "clusters.tsv")
    cwd.write_cluster_members(path, {("1", "1101"): (wells, classes[wells], cl)})
    assert open(path).read().splitlines() == [
        "lane\ttile\twell\tclass\tcluster", "1\t1101\t0\t0\t0", "1\t1101\t1\t1\t0", "1\t1101\t3\t3\t3",
        "1\t1101\t5\t5\t5", "1\t1101\t6\t6\t3", "1\t1101\t7\t7\t0", "1\t1101\t9\t3\t3", "1\t1101\t12\t12\t12",
        "1\t1101\t13\t13\t12", "1\t1101\t14\t14\t14", "1\t1101\t16\t16\t16", "1\t1101\t17\t17\t16",
        "1\t1101\t19\t14\t14", "1\t1101\t21\t3\t3", "1\t1101\t23\t23\t5"]
