"""Host reference of the best well of each of a lane's families (include/welldup_lanekeep.h) in numpy: the lane's tiles
laid end to end as lanenear_ref does, the score of every PF well summed from the host tiles' bytes through the bins'
lower edges, the population of a well read off the labels - group sizes by bincount of the labels, never from a
members array -, the best of a family by the smallest (0xFFFF - score, id), and the header's rows and masks read off
that.  The labels come from lanedups_ref.lane_dups or lanenear_ref.lane_near_dups - the device's own labels are never
used.  lane_keep_literal says the same family by family in plain Python.
Test plumbing only: what LaneDups.keep computes on the GPU is compared against this."""
from __future__ import annotations

import numpy as np

from tiledups_ref import INVALID

LANE_COLS = 17                 # PF, Kept, Dropped, MovedIn, SumKept, SumDropped, Families, Moved, SumRoots, GainBins[8]
TILE_COLS = 6                  # the first six, by the well's own tile
GAIN_BINS = 8
GAIN_EDGES = (1, 10, 20, 50, 100, 200, 500)       # a gain below GAIN_EDGES[i] and not below the edge before lies in bin i
MAX_SCORE = 63 * 1024


def bin_table(edges):
    """bin(q) for q = 0..63: the largest i with edges[i] <= q"""
    edges = [int(e) for e in edges]
    assert 1 <= len(edges) <= 8 and edges[0] == 0 and all(a <= b for a, b in zip(edges, edges[1:])) and edges[-1] <= 63
    return np.array([max(i for i, e in enumerate(edges) if e <= q) for q in range(64)], dtype=np.int64)


def weights_of(edges, min_q):
    """the weight of every bin: its lower edge if that is at least min_q, else 0"""
    return np.array([int(e) if int(e) >= min_q else 0 for e in edges], dtype=np.int64)


def quality_weight(edges, min_q):
    """weight[bin(q)] for q = 0..63"""
    return weights_of(edges, min_q)[bin_table(edges)]


def gain_bin(gain):
    return int(np.searchsorted(np.array(GAIN_EDGES), int(gain), side="right"))


def scores_of(tiles, n, max_tiles, edges, min_q):
    """-> int64 [max_tiles * n]: the score of every well of the tiles given (PF or not), 0 elsewhere"""
    wq = quality_weight(edges, min_q)
    score = np.zeros(max_tiles * n, dtype=np.int64)
    for ti, planes, _ in tiles:
        s = np.zeros(n, dtype=np.int64)
        for p in planes:
            s += wq[np.asarray(p, dtype=np.uint8) >> 2]
        score[ti * n:(ti + 1) * n] = s
    assert score.max(initial=0) <= MAX_SCORE
    return score


def lane_keep(tiles, n, max_tiles, labels, edges, min_q):
    """tiles: [(tile_index, [L planes of n bytes], filter bytes)], labels uint32 [max_tiles, n] -> (lane row int64
    [LANE_COLS], tile rows int64 [max_tiles, TILE_COLS], masks {tile index: uint8 [n]} for the tiles given, and the
    sum of the Singles' scores (identity 5))."""
    flat = np.asarray(labels, dtype=np.uint32).reshape(-1)
    assert flat.size == max_tiles * n
    pf = np.zeros(flat.size, dtype=bool)
    for ti, _, filt in tiles:
        pf[ti * n:(ti + 1) * n] = (np.asarray(filt) & 1) != 0
    assert ((flat != INVALID) == pf).all()
    score = scores_of(tiles, n, max_tiles, edges, min_q)
    ids = np.flatnonzero(pf).astype(np.int64)
    lab = flat[ids].astype(np.int64)
    assert (lab <= ids).all() and (flat[lab] == lab).all()             # a root is the smallest id, and its own root
    size = np.bincount(lab, minlength=flat.size)[lab]
    copy, root, single = lab != ids, (lab == ids) & (size > 1), (lab == ids) & (size == 1)
    fam = copy | root
    key = ((0xFFFF - score[ids]).astype(np.uint64) << np.uint64(32)) | ids.astype(np.uint64)
    best = np.full(flat.size, np.iinfo(np.uint64).max, dtype=np.uint64)
    np.minimum.at(best, lab[fam], key[fam])
    best_id = (best[lab] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    best_score = 0xFFFF - (best[lab] >> np.uint64(32)).astype(np.int64)
    kept = single | (fam & (best_id == ids))
    sc = score[ids]
    lane = np.zeros(LANE_COLS, dtype=np.int64)
    lane[:6] = [ids.size, kept.sum(), (~kept).sum(), (kept & copy).sum(), sc[kept].sum(), sc[~kept].sum()]
    lane[6] = root.sum()
    lane[7] = (root & ~kept).sum()
    lane[8] = sc[root].sum()
    gains = (best_score - sc)[root]
    assert (gains >= 0).all()
    lane[9:] = np.bincount(np.searchsorted(np.array(GAIN_EDGES), gains, side="right"), minlength=GAIN_BINS)
    tile = ids // n
    trow = np.zeros((max_tiles, TILE_COLS), dtype=np.int64)
    trow[:, 0] = np.bincount(tile, minlength=max_tiles)
    trow[:, 1] = np.bincount(tile[kept], minlength=max_tiles)
    trow[:, 2] = np.bincount(tile[~kept], minlength=max_tiles)
    trow[:, 3] = np.bincount(tile[kept & copy], minlength=max_tiles)
    trow[:, 4] = np.bincount(tile[kept], weights=sc[kept], minlength=max_tiles).astype(np.int64)
    trow[:, 5] = np.bincount(tile[~kept], weights=sc[~kept], minlength=max_tiles).astype(np.int64)
    full = np.zeros(flat.size, dtype=np.uint8)
    full[ids[kept]] = 1
    masks = {ti: full[ti * n:(ti + 1) * n].copy() for ti, _, _ in tiles}
    return lane, trow, masks, int(sc[single].sum())


def lane_keep_literal(tiles, n, max_tiles, labels, edges, min_q):
    """lane_keep, read off the header's definitions one family at a time from the bytes (small lanes)."""
    flat = [int(v) for v in np.asarray(labels, dtype=np.uint32).reshape(-1)]
    edges = [int(e) for e in edges]
    weight = [e if e >= min_q else 0 for e in edges]
    score, family = {}, {}
    for ti, planes, filt in tiles:
        for w in range(n):
            if not filt[w] & 1:
                continue
            gid = ti * n + w
            s = 0
            for p in planes:
                q = int(p[w]) >> 2
                s += weight[max(i for i, e in enumerate(edges) if e <= q)]
            score[gid] = s
            family.setdefault(flat[gid], []).append(gid)
    lane, trow = [0] * LANE_COLS, [[0] * TILE_COLS for _ in range(max_tiles)]
    masks = {ti: np.zeros(n, dtype=np.uint8) for ti, _, _ in tiles}
    singles = 0
    for root, wells in family.items():
        assert root == min(wells)
        best = max(wells, key=lambda g: (score[g], -g))                # the largest score, the smallest id among equals
        if len(wells) > 1:
            lane[6] += 1
            lane[7] += best != root
            lane[8] += score[root]
            lane[9 + gain_bin(score[best] - score[root])] += 1
        else:
            singles += score[root]
        for g in wells:
            t = trow[g // n]
            kept = g == best
            for row in (lane, t):
                row[0] += 1
                row[1 if kept else 2] += 1
                row[3] += kept and g != root
                row[4 if kept else 5] += score[g]
            if kept:
                masks[g // n][g % n] = 1
    return np.array(lane, dtype=np.int64), np.array(trow, dtype=np.int64).reshape(max_tiles, TILE_COLS), masks, singles


def check_keep_identities(lane, trow, edges, min_q, finish_lane=None, finish_tiles=None, qhist=None, sum_singles=None,
                          masks=None, labels=None):
    """Identities 1 - 6 of the header, of any result.  finish_lane, finish_tiles: the rows of the finish the labels
    came from (PF and Redundant are columns 0 and 3 of the lane row, PF column 0 of a tile row); qhist: QHist of
    LaneDups.qualities on the same accumulator; sum_singles: the Singles' summed scores; masks {tile index: uint8 [n]}
    and labels uint32 [max_tiles, n]: identity 6."""
    lane, trow = np.asarray(lane), np.asarray(trow)
    assert lane.shape == (LANE_COLS,) and trow.shape[1] == TILE_COLS
    assert (lane >= 0).all() and (trow >= 0).all()
    pf, kept, dropped, moved_in, sum_kept, sum_dropped, families, moved, sum_roots = (int(v) for v in lane[:9])
    gains = lane[9:]
    assert pf == kept + dropped and kept >= families                                        # 1
    if finish_lane is not None:
        assert pf == finish_lane[0] and dropped == finish_lane[3]
    assert (trow.sum(axis=0) == lane[:6]).all()                                             # 2
    assert (trow[:, 0] == trow[:, 1] + trow[:, 2]).all() and (trow[:, 3] <= trow[:, 1]).all()
    if finish_tiles is not None:
        assert (trow[:, 0] == np.asarray(finish_tiles)[:, 0]).all()
    assert moved == families - gains[0] == moved_in and gains.sum() == families             # 3
    if qhist is not None:                                                                   # 4
        assert sum_kept + sum_dropped == int((quality_weight(edges, min_q) * np.asarray(qhist)).sum())
    if sum_singles is not None:                                                             # 5
        assert sum_kept - sum_singles >= sum_roots and (sum_kept - sum_singles == sum_roots) == (moved == 0)
        lo = np.array((0,) + GAIN_EDGES)                               # the gains' sum lies between the bins' bounds
        assert (gains * lo).sum() <= sum_kept - sum_singles - sum_roots
    if min_q > max(int(e) for e in edges):                                                  # 6
        assert moved == 0 and sum_kept == sum_dropped == sum_roots == 0 and gains[0] == families
        if masks is not None and labels is not None:
            lab = np.asarray(labels, dtype=np.uint32)
            n = lab.shape[1]
            for ti, m in masks.items():
                assert (m == (lab[ti] == ti * n + np.arange(n, dtype=np.uint32))).all()
