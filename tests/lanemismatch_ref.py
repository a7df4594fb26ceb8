"""Host reference of where a lane's duplicate copies differ (include/welldup_lanemismatch.h) in numpy: the lane's
tiles laid end to end as lanenear_ref does, every PF well that is not its own root compared with its root code by
code, and the header's definitions read off the comparison.  The labels come from lanedups_ref.lane_dups or
lanenear_ref.lane_near_dups - the device's own labels are never used.
Test plumbing only: what LaneDups.mismatches computes on the GPU is compared against this."""
from __future__ import annotations

import numpy as np

from lanenear_ref import lay_end_to_end
from tiledups_ref import INVALID

MAX_D = 7
DIST_BINS = 9
LANE_COLS = 4 + DIST_BINS      # Pairs, Profiled, Mismatches, WithN, Dist d = 0..7 and >= 8
TILE_COLS = 4                  # Pairs, Profiled, Mismatches, WithN
N_CODE = 4


def lane_pairs(tiles, n, max_tiles, labels):
    """-> (member ids int64 [P], root ids int64 [P], root codes uint8 [L, P], member codes uint8 [L, P])"""
    codes, pf = lay_end_to_end(tiles, n, max_tiles)
    flat = np.asarray(labels, dtype=np.uint32).reshape(-1)
    assert flat.size == max_tiles * n and ((flat != INVALID) == pf).all()
    ids = np.flatnonzero((flat != INVALID) & (flat != np.arange(flat.size, dtype=np.uint32))).astype(np.int64)
    roots = flat[ids].astype(np.int64)
    assert (roots < ids).all() and (flat[roots] == roots).all()       # a root is the smallest id, and its own root
    return ids, roots, codes[:, roots], codes[:, ids]


def lane_mismatches(tiles, n, max_tiles, labels, max_d):
    """tiles: [(tile_index, [L planes of n bytes], filter bytes)], labels uint32 [max_tiles, n] -> (lane row int64
    [LANE_COLS], tile rows int64 [max_tiles, TILE_COLS], sub int64 [L, 5, 5])."""
    assert 0 <= max_d <= MAX_D
    ids, roots, a, b = lane_pairs(tiles, n, max_tiles, labels)
    L = a.shape[0]
    differ = a != b
    d = differ.sum(axis=0).astype(np.int64)
    profiled = d <= max_d
    counted = differ & profiled[None, :]
    with_n = (counted & ((a == N_CODE) | (b == N_CODE))).sum(axis=0).astype(np.int64)
    sub = np.zeros((L, 5, 5), dtype=np.int64)
    c, p = np.nonzero(counted)
    np.add.at(sub, (c, a[c, p], b[c, p]), 1)
    tile = ids // n
    trow = np.zeros((max_tiles, TILE_COLS), dtype=np.int64)
    trow[:, 0] = np.bincount(tile, minlength=max_tiles)
    trow[:, 1] = np.bincount(tile[profiled], minlength=max_tiles)
    trow[:, 2] = np.bincount(tile, weights=d * profiled, minlength=max_tiles).astype(np.int64)
    trow[:, 3] = np.bincount(tile, weights=with_n, minlength=max_tiles).astype(np.int64)
    dist = np.bincount(np.minimum(d, DIST_BINS - 1), minlength=DIST_BINS).astype(np.int64)
    return np.concatenate([trow.sum(axis=0), dist]).astype(np.int64), trow, sub


def check_mismatch_identities(lane, trow, sub, max_d, finish_lane=None, finish_tiles=None, equality=False):
    """What the header promises of any result.  finish_lane, finish_tiles: the rows of the finish the labels came
    from (Redundant is column 3 of the lane row, LaneRedundant column 4 of a tile row); equality: the labels are
    classes."""
    lane, trow, sub = np.asarray(lane), np.asarray(trow), np.asarray(sub)
    pairs, profiled, mismatches, with_n = (int(v) for v in lane[:4])
    dist = lane[4:]
    assert lane.shape == (LANE_COLS,) and trow.shape[1] == TILE_COLS and sub.shape[1:] == (5, 5)
    assert dist.sum() == pairs
    assert profiled == dist[:max_d + 1].sum()
    assert mismatches == (np.arange(max_d + 1) * dist[:max_d + 1]).sum()
    assert (trow.sum(axis=0) == lane[:4]).all()
    assert sub.sum() == mismatches and (sub >= 0).all()
    assert all(sub[:, a, a].sum() == 0 for a in range(5))
    assert sub[:, N_CODE, :].sum() + sub[:, :, N_CODE].sum() == with_n
    assert (trow[:, 1] <= trow[:, 0]).all() and (trow[:, 3] <= trow[:, 2]).all()
    if finish_lane is not None:
        assert pairs == finish_lane[3]
    if finish_tiles is not None:
        assert (trow[:, 0] == np.asarray(finish_tiles)[:, 4]).all()
    if equality:
        assert dist[0] == pairs and not dist[1:].any() and not sub.any() and mismatches == 0 and profiled == pairs
