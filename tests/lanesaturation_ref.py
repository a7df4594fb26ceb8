"""Host reference of a lane's distinct reads against its depth (include/welldup_lanesaturation.h) in numpy, computed
directly from the labels, N, max_tiles and the coordinates: the step of every well in uint64 arithmetic, the dropped
wells by the header's integer test, the class minima with np.minimum.at.  The labels come from lanedups_ref.lane_dups
or lanenear_ref.lane_near_dups - the device's own labels are never used.  Test plumbing only: what
LaneDups.saturation computes on the GPU is compared against this; it shares no code with the library."""
from __future__ import annotations

import numpy as np

from tiledups_ref import INVALID

MAX_STEPS = 64
HEAD_COLS = 2                  # PF, Dropped
MAX_COORD = (1 << 24) - 1
MAX_RADIUS = 1 << 25
MASK = np.uint64(0xFFFFFFFF)


def step_of(g, seed, steps):
    """The step of global ids g (any integers below 2^32) for a uint32 seed: uint64 arithmetic, masked to 32 bits
    after every add and multiply."""
    assert 1 <= steps <= MAX_STEPS and 0 <= seed < 1 << 32
    u = lambda v: np.uint64(v)
    h = (np.asarray(g).astype(np.uint64) + u((seed * 0x9E3779B9) & 0xFFFFFFFF)) & MASK
    h ^= h >> u(16)
    h = (h * u(0x85EBCA6B)) & MASK
    h ^= h >> u(13)
    h = (h * u(0xC2B2AE35)) & MASK
    h ^= h >> u(16)
    return ((h * u(steps)) >> u(32)).astype(np.int64)


def dropped_wells(labels, n, max_tiles, x=None, y=None, radius=0):
    """-> bool [max_tiles * n]: the same-tile pairs with q < radius^2 (none without coordinates or with radius 0)"""
    assert 0 <= radius <= MAX_RADIUS
    flat = np.asarray(labels, dtype=np.uint32).reshape(-1)
    assert flat.size == max_tiles * n
    out = np.zeros(flat.size, dtype=bool)
    if x is None or radius == 0:
        assert y is None or radius == 0
        return out
    xs, ys = np.asarray(x).astype(np.int64), np.asarray(y).astype(np.int64)
    assert xs.shape == ys.shape == (n,)
    assert n == 0 or (min(xs.min(), ys.min()) >= 0 and max(xs.max(), ys.max()) <= MAX_COORD)
    ids = np.flatnonzero((flat != INVALID) & (flat != np.arange(flat.size, dtype=np.uint32))).astype(np.int64)
    roots = flat[ids].astype(np.int64)
    same = ids // n == roots // n
    w, r = ids[same] % n, roots[same] % n
    q = (xs[w] - xs[r]) ** 2 + (ys[w] - ys[r]) ** 2
    out[ids[same][q < int(radius) * int(radius)]] = True
    return out


def lane_saturation(labels, n, max_tiles, steps, seed=0, x=None, y=None, radius=0):
    """labels uint32 [max_tiles, n] (or flat) -> (head int64 [2]: [PF, Dropped], new reads int64 [steps], new distinct
    int64 [steps])."""
    flat = np.asarray(labels, dtype=np.uint32).reshape(-1)
    ids = np.arange(flat.size, dtype=np.int64)
    pf = flat != INVALID
    dropped = dropped_wells(flat, n, max_tiles, x, y, radius)
    assert not (dropped & ~pf).any() and not (dropped & (flat == ids)).any()      # a root is never dropped
    counted = pf & ~dropped
    step = step_of(ids, seed, steps)
    roots = flat[counted].astype(np.int64)
    assert (flat[roots] == roots).all()                                # a root is its own root
    class_step = np.full(flat.size, steps, dtype=np.int64)
    np.minimum.at(class_step, roots, step[counted])                    # (a root counts itself: its own step is in)
    own = pf & (flat == ids)
    new_reads = np.bincount(step[counted], minlength=steps).astype(np.int64)
    new_distinct = np.bincount(class_step[own], minlength=steps).astype(np.int64)
    assert new_distinct.size == steps                                  # every own well got a step below `steps`
    return np.array([pf.sum(), dropped.sum()], dtype=np.int64), new_reads, new_distinct


def coarsen(arr):
    """steps 2j and 2j + 1 added"""
    arr = np.asarray(arr)
    assert arr.size % 2 == 0
    return arr.reshape(-1, 2).sum(axis=1)


def check_saturation_identities(head, new_reads, new_distinct, finish_lane=None, local=None, finer=None, no_class=False,
                                other_seed=None):
    """What the header promises of any result.  finish_lane: the lane row of the finish the labels came from (PF is
    column 0, Redundant column 3); local: Local of wd_lane_distances at the same radius; finer: the result for twice
    the steps, same seed and radius, from the same source; no_class: the lane has no class; other_seed: a result for
    the same steps and radius under another seed."""
    head, r, d = (np.asarray(v) for v in (head, new_reads, new_distinct))
    assert head.shape == (HEAD_COLS,) and r.shape == d.shape and 1 <= r.size <= MAX_STEPS
    assert (head >= 0).all() and (r >= 0).all() and (d >= 0).all()
    pf, dropped = int(head[0]), int(head[1])
    assert r.sum() == pf - dropped
    assert (np.cumsum(d) <= np.cumsum(r)).all()
    if finish_lane is not None:
        assert pf == finish_lane[0] and d.sum() == pf - finish_lane[3]
    if local is not None:
        assert dropped == local
    if finer is not None:
        assert (np.asarray(finer[0]) == head).all()
        assert (coarsen(finer[1]) == r).all() and (coarsen(finer[2]) == d).all()
    if no_class:
        assert (r == d).all() and dropped == 0
    if other_seed is not None:
        assert (np.asarray(other_seed[0]) == head).all()
        assert np.asarray(other_seed[1]).sum() == r.sum() and np.asarray(other_seed[2]).sum() == d.sum()
