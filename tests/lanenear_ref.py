"""Host reference of the near-duplicate read clusters of a lane (include/welldup_lanenear.h) in numpy.  The
lane's tiles are laid end to end as one "tile" of max_tiles * n wells (a well's place is its global id; a tile
index never added is n wells that fail the filter), the distinct reads and the edges between them come from
tests/tilenear_ref.py (`edges_all_pairs`, `edges_by_deletion`: neither is the segment scheme of the device) and
`cluster_labels` unites them.  Rows follow from the cluster labels by the arithmetic of tests/lanedups_ref.py with
NearPairs inserted: once in arrays (`rows_from_labels`), once cluster by cluster (`rows_literal`).
Test plumbing only: what LaneDups.finish(hamming=K) computes on the GPU is compared against this."""
from __future__ import annotations

import numpy as np

from lanedups_ref import LANE_COLS, TILE_COLS
from tiledups_ref import INVALID, SIZE_BINS, codes_of
from tilenear_ref import cluster_labels, distinct_reads, edges_all_pairs, edges_by_deletion

NEAR_LANE_COLS = LANE_COLS + 1     # PF, Clusters, InClusters, Redundant, CrossTileClusters, TileSpans, NearPairs, bins
NEAR_PAIRS = 6


def lay_end_to_end(tiles, n, max_tiles):
    """-> (codes uint8 [L, max_tiles * n], pf bool [max_tiles * n]) of the lane as one tile."""
    assert len({t[0] for t in tiles}) == len(tiles) and all(0 <= t[0] < max_tiles for t in tiles)
    L = len(tiles[0][1]) if tiles else 0
    codes = np.zeros((L, max_tiles * n), dtype=np.uint8)
    pf = np.zeros(max_tiles * n, dtype=bool)
    for ti, planes, filt in tiles:
        codes[:, ti * n:(ti + 1) * n] = codes_of(planes, n)
        pf[ti * n:(ti + 1) * n] = (np.asarray(filt, dtype=np.uint8)[:n] & 1).astype(bool)
    return codes, pf


def near_row(lane, near_pairs):
    """the lane row of lanedups_ref with NearPairs in front of the size bins"""
    lane = np.asarray(lane, dtype=np.int64)
    return np.concatenate([lane[:NEAR_PAIRS], [int(near_pairs)], lane[NEAR_PAIRS:]]).astype(np.int64)


def rows_from_labels(flat, n, max_tiles):
    """labels uint32 [max_tiles * n] (the smallest global id of a well's group, INVALID for no vertex) -> (lane row
    [LANE_COLS], tile rows [max_tiles, TILE_COLS]) in array arithmetic, as lanedups_ref.lane_dups."""
    lane = np.zeros(LANE_COLS, dtype=np.int64)
    trow = np.zeros((max_tiles, TILE_COLS), dtype=np.int64)
    ids = np.flatnonzero(flat != INVALID).astype(np.int64)
    if ids.size == 0:
        return lane, trow
    lab = flat[ids].astype(np.int64)
    tile = ids // n
    size = np.bincount(lab, minlength=flat.size)
    in_group = size[lab] >= 2
    lane[0] = ids.size
    lane[1] = int((size >= 2).sum())
    lane[2] = int(in_group.sum())
    lane[3] = lane[2] - lane[1]
    lane[6:] = np.bincount(np.minimum(size[size >= 2], SIZE_BINS + 1) - 2, minlength=SIZE_BINS)[:SIZE_BINS]
    pairs, held = np.unique(lab[in_group] * max_tiles + tile[in_group], return_counts=True)
    lane[5] = pairs.size
    lane[4] = int((np.unique(pairs // max_tiles, return_counts=True)[1] >= 2).sum()) if pairs.size else 0
    pair_tile = pairs % max_tiles
    trow[:, 0] = np.bincount(tile, minlength=max_tiles)
    trow[:, 1] = np.bincount(tile[in_group], minlength=max_tiles)
    trow[:, 2] = np.bincount(pair_tile[held >= 2], weights=held[held >= 2], minlength=max_tiles).astype(np.int64)
    trow[:, 3] = np.bincount(pair_tile, weights=held - 1, minlength=max_tiles).astype(np.int64)
    trow[:, 4] = np.bincount(tile[in_group & (ids != lab)], minlength=max_tiles)
    return lane, trow


def rows_literal(flat, n, max_tiles):
    """rows_from_labels, read off the header's definitions one cluster at a time (small lanes)."""
    lane = np.zeros(LANE_COLS, dtype=np.int64)
    trow = np.zeros((max_tiles, TILE_COLS), dtype=np.int64)
    ids = np.flatnonzero(flat != INVALID)
    np.add.at(trow[:, 0], ids // n, 1)
    lane[0] = ids.size
    for root in sorted(set(flat[ids].tolist())):
        members = np.sort(ids[flat[ids] == root])
        if members.size < 2:
            continue
        assert members[0] == root
        tiles_of = members // n
        touched = sorted(set(tiles_of.tolist()))
        lane[1] += 1
        lane[2] += members.size
        lane[4] += len(touched) >= 2
        lane[5] += len(touched)
        lane[6 + min(members.size, SIZE_BINS + 1) - 2] += 1
        for t in touched:
            here = members[tiles_of == t]
            trow[t, 1] += here.size
            if here.size >= 2:
                trow[t, 2] += here.size
            trow[t, 3] += here.size - 1
            trow[t, 4] += int((here != root).sum())
    lane[3] = lane[2] - lane[1]
    return lane, trow


def lane_near_dups(tiles, n, max_tiles, k, method="all_pairs", rows="arrays"):
    """tiles: [(tile_index, [L planes of n bytes], filter bytes)] -> (near lane row int64 [NEAR_LANE_COLS], near tile
    rows int64 [max_tiles, TILE_COLS], labels uint32 [max_tiles, n]) at Hamming distance <= k."""
    codes, pf = lay_end_to_end(tiles, n, max_tiles)
    class_lab, reps = distinct_reads(codes, pf)
    if k == 0 or reps.size < 2:
        edges = np.zeros((0, 2), dtype=np.int64)
    elif method == "all_pairs":
        edges = edges_all_pairs(codes, reps, k)
    else:
        edges = edges_by_deletion(codes, reps, k)
    labels = cluster_labels(class_lab, reps, edges)
    lane, trow = (rows_from_labels if rows == "arrays" else rows_literal)(labels, n, max_tiles)
    return near_row(lane, edges.shape[0]), trow, labels.reshape(max_tiles, n)


def check_near_identities(near_lane, trow):
    """lanedups_ref.check_identities on the cluster rows (NearPairs taken out)."""
    from lanedups_ref import check_identities
    near_lane = np.asarray(near_lane)
    check_identities(np.concatenate([near_lane[:NEAR_PAIRS], near_lane[NEAR_PAIRS + 1:]]), np.asarray(trow))
    assert near_lane[NEAR_PAIRS] >= 0


def coarser(fine, coarse):
    """equal labels in `fine` imply equal labels in `coarse` (both uint32, same shape), and the vertices are the same"""
    fine, coarse = np.asarray(fine).reshape(-1), np.asarray(coarse).reshape(-1)
    if not ((fine == INVALID) == (coarse == INVALID)).all():
        return False
    v = fine != INVALID
    pairs = np.unique(np.stack([fine[v], coarse[v]], axis=1), axis=0)
    return pairs.shape[0] == np.unique(fine[v]).shape[0]


# ---- a hand-made lane and its hand-worked answer (host and GPU tests) -----------------------------
_A, _C, _G, _T = 0x40, 0x81, 0xC2, 0x23
_BASE = {"A": _A, "C": _C, "G": _G, "T": _T, "N": 0}


def hand_made_lane():
    """Tile indices 0, 1, 2 and 4 of a lane with room for five tiles, four wells each, six cycles (ids in brackets):
         index 0   [0] AAAAAA   [1] NAGGTT   [2] CGCGCG   [3] GGGGGG
         index 1   [4] CAAAAA   [5] TATATA   [6] NAGGTC   [7] GGGGGT
         index 2   [8] CCAAAA   [9] AAGGTA  [10] GGGTTT  [11] GGTTTT
         index 4  [16] GGGGTT* [17] CGCGCG  [18] AAAAAA  [19] CTAGCT          * fails the filter (byte 2)
    chain    0 ~ 4 ~ 8 on three tiles (0 and 8 differ in two cycles); 18 on a fourth tile equals 0
    N        1 ~ 6 (N == N); 9 is two cycles from both (N against A counts): it joins them at K = 2 only
    bridge   3 ~ 7 and 10 ~ 11; 16 is one cycle from 7 and from 10 but fails the filter: two clusters at K = 1;
             at K = 2 well 7 reaches 10 itself
    class    2 == 17 across tiles; 5 and 19 are at least three cycles from everything."""
    reads = {0: "AAAAAA", 1: "NAGGTT", 2: "CGCGCG", 3: "GGGGGG", 4: "CAAAAA", 5: "TATATA", 6: "NAGGTC", 7: "GGGGGT",
             8: "CCAAAA", 9: "AAGGTA", 10: "GGGTTT", 11: "GGTTTT", 16: "GGGGTT", 17: "CGCGCG", 18: "AAAAAA", 19: "CTAGCT"}
    tiles = []
    for ti in (0, 1, 2, 4):
        planes = [np.array([_BASE[reads[ti * 4 + w][c]] for w in range(4)], dtype=np.uint8) for c in range(6)]
        filt = np.ones(4, dtype=np.uint8)
        if ti == 4:
            filt[0] = 2                                                # only bit 0 counts
            for c in range(6):
                planes[c][2] |= 0x3C if c % 2 else 0x10                # (the same bases, other quality bits)
        tiles.append((ti, planes, filt))
    return tiles


I = INVALID
HAND = {
    # K = 0: classes {0, 18} and {2, 17}
    0: dict(labels=[[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11], [I] * 4, [I, 2, 0, 19]],
            lane=[15, 2, 4, 2, 2, 4, 0, 2, 0, 0, 0, 0, 0, 0, 0],
            tiles=[[4, 2, 0, 0, 0], [4, 0, 0, 0, 0], [4, 0, 0, 0, 0], [0] * 5, [3, 2, 0, 0, 2]]),
    # K = 1: {0, 4, 8, 18}, {1, 6}, {2, 17}, {3, 7}, {10, 11}; pairs of distinct reads 0-4, 4-8, 1-6, 3-7, 10-11
    1: dict(labels=[[0, 1, 2, 3], [0, 5, 1, 3], [0, 9, 10, 10], [I] * 4, [I, 2, 0, 19]],
            lane=[15, 5, 12, 7, 4, 11, 5, 4, 0, 1, 0, 0, 0, 0, 0],
            tiles=[[4, 4, 0, 0, 0], [4, 3, 0, 0, 3], [4, 3, 2, 1, 2], [0] * 5, [3, 2, 0, 0, 2]]),
    # K = 2: {0, 4, 8, 18}, {1, 6, 9}, {2, 17}, {3, 7, 10, 11}; K = 1's pairs and 0-8, 1-9, 6-9, 7-10 (3-10 and 7-11
    # differ in three cycles, 3-11 in four)
    2: dict(labels=[[0, 1, 2, 3], [0, 5, 1, 3], [0, 1, 3, 3], [I] * 4, [I, 2, 0, 19]],
            lane=[15, 4, 13, 9, 4, 12, 9, 1, 1, 2, 0, 0, 0, 0, 0],
            tiles=[[4, 4, 0, 0, 0], [4, 3, 0, 0, 3], [4, 4, 2, 1, 4], [0] * 5, [3, 2, 0, 0, 2]]),
}
