"""Host reference of which libraries a lane's duplicate copies join (include/welldup_lanehops.h) in numpy: the index
key of every redundant well held against its root's under a label array - the classes of lanedups_ref or the clusters
of lanenear_ref - and the keys of laneindex_ref.index_keys.  Twice: in array arithmetic (lane_hops), and read off the
header's definitions one well and one cycle at a time (lane_hops_literal).
Test plumbing only: what LaneDups.hops computes on the GPU is compared against this."""
from __future__ import annotations

import numpy as np

from laneindex_ref import index_keys
from tiledups_ref import INVALID

TILE_COLS = 4                  # Pairs, SameTile, Hop1, Hop2
LANE_COLS = 13                 # the four, then State[0..8]
MAX_E = 3
MAX_LISTED = 1024


def _code(keys, c):
    return (keys >> np.uint64(32 * (c // 10) + 3 * (c % 10))) & np.uint64(7)


def lane_hops(index_tiles, labels, n, max_tiles, I, split, max_e, listed):
    """labels uint32 [max_tiles, n] (INVALID: no PF well); listed: M distinct keys -> (lane row int64 [13], tile rows
    int64 [max_tiles, 4], matrix int64 [M + 1, M + 1])."""
    assert 1 <= split <= I and 0 <= max_e <= MAX_E
    listed = np.asarray(listed, dtype=np.uint64).reshape(-1)
    M = listed.size
    assert M <= MAX_LISTED and np.unique(listed).size == M
    flat = np.asarray(labels, dtype=np.uint32).reshape(-1)
    keys, given = index_keys(index_tiles, n, max_tiles)
    ids = np.flatnonzero(flat != INVALID)
    assert given[np.unique(ids // n)].all()
    copy = ids[flat[ids] != ids]
    root = flat[copy].astype(np.int64)
    d = np.zeros((2, copy.size), dtype=np.int64)
    for c in range(I):
        d[0 if c < split else 1] += _code(keys[root], c) != _code(keys[copy], c)
    state = np.where(d == 0, 0, np.where(d <= max_e, 1, 2))
    pair_state = 3 * state[0] + state[1]
    far = (state == 2).sum(axis=0)
    tile = copy // n
    tile_rows = np.zeros((max_tiles, TILE_COLS), dtype=np.int64)
    tile_rows[:, 0] = np.bincount(tile, minlength=max_tiles)
    tile_rows[:, 1] = np.bincount(tile[root // n == tile], minlength=max_tiles)
    tile_rows[:, 2] = np.bincount(tile[far == 1], minlength=max_tiles)
    tile_rows[:, 3] = np.bincount(tile[far == 2], minlength=max_tiles)
    lane = np.concatenate([tile_rows.sum(axis=0), np.bincount(pair_state, minlength=9)]).astype(np.int64)

    def rank(k):
        if M == 0:
            return np.zeros(k.size, dtype=np.int64)
        order = np.argsort(listed)
        at = np.minimum(np.searchsorted(listed[order], k), M - 1)
        return np.where(listed[order][at] == k, order[at], M).astype(np.int64)
    matrix = np.bincount(rank(keys[root]) * (M + 1) + rank(keys[copy]), minlength=(M + 1) ** 2).reshape(M + 1, M + 1)
    return lane, tile_rows, matrix.astype(np.int64)


def lane_hops_literal(index_tiles, labels, n, max_tiles, I, split, max_e, listed):
    """lane_hops, one well at a time (small lanes)."""
    flat = np.asarray(labels, dtype=np.uint32).reshape(-1).tolist()
    keys = index_keys(index_tiles, n, max_tiles)[0].tolist()
    listed = [int(k) for k in listed]
    M = len(listed)
    lane, tile_rows = [0] * LANE_COLS, [[0] * TILE_COLS for _ in range(max_tiles)]
    matrix = [[0] * (M + 1) for _ in range(M + 1)]
    for g, r in enumerate(flat):
        if r == INVALID or r == g:
            continue
        d = [0, 0]
        for c in range(I):
            at = 32 * (c // 10) + 3 * (c % 10)
            d[0 if c < split else 1] += (keys[r] >> at) & 7 != (keys[g] >> at) & 7
        s = [0 if v == 0 else 1 if v <= max_e else 2 for v in d]
        row = tile_rows[g // n]
        row[0] += 1
        row[1] += r // n == g // n
        row[2] += s.count(2) == 1
        row[3] += s.count(2) == 2
        lane[4 + 3 * s[0] + s[1]] += 1
        matrix[listed.index(keys[r]) if keys[r] in listed else M][listed.index(keys[g]) if keys[g] in listed else M] += 1
    for f in range(TILE_COLS):
        lane[f] = sum(row[f] for row in tile_rows)
    return np.array(lane, dtype=np.int64), np.array(tile_rows, dtype=np.int64).reshape(max_tiles, TILE_COLS), \
        np.array(matrix, dtype=np.int64)


def check_hop_identities(result, eq_lane, eq_tiles, I, split, max_e, all_listed=False, subset_of_scanned=False):
    """What the header promises of any result; eq_lane, eq_tiles: the lane row and the tile rows (classes or clusters)
    the labels belong to - [PF, Classes, InClasses, Redundant, ...] and [.., LaneRedundant]; all_listed: every PF
    well's key is in the listing; subset_of_scanned: equality labels and index cycles among the scanned ones."""
    lane, tile_rows, matrix = (np.asarray(v) for v in result)
    M = matrix.shape[0] - 1
    state = lane[4:]
    assert lane.shape == (LANE_COLS,) and tile_rows.shape[1] == TILE_COLS and matrix.shape == (M + 1, M + 1)
    assert (lane >= 0).all() and (tile_rows >= 0).all() and (matrix >= 0).all()
    assert state.sum() == lane[0] == int(eq_lane[3])
    assert lane[2] == state[2] + state[5] + state[6] + state[7] and lane[3] == state[8]
    assert (tile_rows.sum(axis=0) == lane[:4]).all()
    assert (tile_rows[:, 0] == np.asarray(eq_tiles)[:, 4]).all()
    assert (tile_rows[:, 1] <= tile_rows[:, 0]).all() and (tile_rows[:, 2] + tile_rows[:, 3] <= tile_rows[:, 0]).all()
    assert matrix.sum() == lane[0]
    if all_listed:
        assert not matrix[M].any() and not matrix[:, M].any() and np.trace(matrix) == state[0]
    else:
        assert np.trace(matrix[:M, :M]) <= state[0]
    if split == I:
        assert not state[[1, 2, 4, 5, 7, 8]].any()
    if max_e >= split:
        assert not state[6:].any()
    if max_e >= I - split:
        assert not state[[2, 5, 8]].any()
    if subset_of_scanned:
        assert state[0] == lane[0]
    if M == 0:
        assert matrix.tolist() == [[int(lane[0])]]
