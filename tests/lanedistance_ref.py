"""Host reference of how far apart a lane's duplicate copies lie (include/welldup_lanedistance.h) in numpy, computed
directly from the labels, N and the coordinates: every PF well that is not its own root against its root.  The
labels come from lanedups_ref.lane_dups or lanenear_ref.lane_near_dups - the device's own labels are never used.
Test plumbing only: what LaneDups.distances computes on the GPU is compared against this."""
from __future__ import annotations

import numpy as np

from tiledups_ref import INVALID

DIST_BINS = 11
LANE_COLS = 3 + DIST_BINS      # Pairs, SameTile, Local, Dist[0..10]
TILE_COLS = 3                  # Pairs, SameTile, Local
MAX_COORD = (1 << 24) - 1
MAX_RADIUS = 1 << 25
EDGES = [32 << j for j in range(10)]      # Local at these radii is a prefix sum of Dist


def dist_bin(q):
    """The bin of squared distances, by the header's compares: the number of thresholds 2^10, 2^12, .., 2^28 that q
    has reached (int64 holds q < 2^49 exactly)."""
    return np.searchsorted(np.array([1 << (10 + 2 * b) for b in range(DIST_BINS - 1)], dtype=np.int64),
                           np.asarray(q, dtype=np.int64), side="right")


def lane_distances(labels, n, max_tiles, x, y, radius):
    """labels uint32 [max_tiles, n] (or flat), x, y: n coordinates -> (lane row int64 [LANE_COLS], tile rows int64
    [max_tiles, TILE_COLS], tile pairs int64 [max_tiles, max_tiles]: [root's tile][member's tile])."""
    assert 0 <= radius <= MAX_RADIUS
    flat = np.asarray(labels, dtype=np.uint32).reshape(-1)
    xs, ys = np.asarray(x).astype(np.int64), np.asarray(y).astype(np.int64)
    assert flat.size == max_tiles * n and xs.shape == ys.shape == (n,)
    assert n == 0 or (min(xs.min(), ys.min()) >= 0 and max(xs.max(), ys.max()) <= MAX_COORD)
    ids = np.flatnonzero((flat != INVALID) & (flat != np.arange(flat.size, dtype=np.uint32))).astype(np.int64)
    roots = flat[ids].astype(np.int64)
    assert (roots < ids).all() and (flat[roots] == roots).all()       # a root is the smallest id, and its own root
    tile, root_tile = ids // n, roots // n
    same = tile == root_tile
    w, r = ids[same] % n, roots[same] % n
    q = (xs[w] - xs[r]) ** 2 + (ys[w] - ys[r]) ** 2
    trow = np.zeros((max_tiles, TILE_COLS), dtype=np.int64)
    trow[:, 0] = np.bincount(tile, minlength=max_tiles)
    trow[:, 1] = np.bincount(tile[same], minlength=max_tiles)
    trow[:, 2] = np.bincount(tile[same][q < int(radius) * int(radius)], minlength=max_tiles)
    pairs = np.zeros((max_tiles, max_tiles), dtype=np.int64)
    np.add.at(pairs, (root_tile, tile), 1)
    dist = np.bincount(dist_bin(q), minlength=DIST_BINS).astype(np.int64)
    return np.concatenate([trow.sum(axis=0), dist]).astype(np.int64), trow, pairs


def check_distance_identities(lane, trow, pairs, radius, finish_lane=None, finish_tiles=None, local_at=None,
                              classes_of_two=False):
    """What the header promises of any result.  pairs may be None (no matrix).  finish_lane, finish_tiles: the rows
    of the finish the labels came from (Redundant is column 3 of the lane row; TileRedundant and LaneRedundant are
    columns 3 and 4 of a tile row).  local_at(R) -> the lane's Local at radius R, from the same source as the result:
    the identities that tie Local to the radius are checked through it.  classes_of_two: no class has more than two
    members."""
    lane, trow = np.asarray(lane), np.asarray(trow)
    n_pairs, same, local = (int(v) for v in lane[:3])
    dist = lane[3:]
    assert lane.shape == (LANE_COLS,) and trow.shape[1] == TILE_COLS and (lane >= 0).all() and (trow >= 0).all()
    assert dist.sum() == same
    assert (trow.sum(axis=0) == lane[:3]).all()
    assert (trow[:, 2] <= trow[:, 1]).all() and (trow[:, 1] <= trow[:, 0]).all()
    for j, edge in enumerate(EDGES):
        if radius == edge:
            assert local == dist[:j + 1].sum()
    if radius == 0:
        assert local == 0
    if radius == MAX_RADIUS:
        assert local == same
    if pairs is not None:
        pairs = np.asarray(pairs)
        assert pairs.shape == (trow.shape[0], trow.shape[0]) and (pairs >= 0).all()
        assert (pairs.sum(axis=0) == trow[:, 0]).all()                 # column b: the pairs whose member lies on b
        assert (np.diagonal(pairs) == trow[:, 1]).all()
        assert not np.tril(pairs, -1).any()                            # the root is the smallest global id
    if finish_lane is not None:
        assert n_pairs == finish_lane[3]
    if finish_tiles is not None:
        finish_tiles = np.asarray(finish_tiles)
        assert (trow[:, 0] == finish_tiles[:, 4]).all()
        assert (trow[:, 1] <= finish_tiles[:, 3]).all()
        assert not classes_of_two or (trow[:, 1] == finish_tiles[:, 3]).all()
    if local_at is not None:
        at = {r: int(local_at(r)) for r in [0, 1] + EDGES + [e + 1 for e in EDGES] + [MAX_RADIUS]}
        assert at[0] == 0 and at[MAX_RADIUS] == same
        for j, edge in enumerate(EDGES):
            assert at[edge] == dist[:j + 1].sum()
        order = sorted(at)
        assert all(at[a] <= at[b] for a, b in zip(order, order[1:]))   # monotone in the radius
        assert radius not in at or at[radius] == local
