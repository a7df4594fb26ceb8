"""Host reference of a lane's reported base quality against its duplicate copies (include/welldup_lanequality.h) in
numpy: the lane's tiles laid end to end as lanenear_ref does, the qualities (byte >> 2) binned by the caller's edges,
every PF well that is not its own root held against its root cycle by cycle, and the header's definitions read off
that.  The labels come from lanedups_ref.lane_dups or lanenear_ref.lane_near_dups - the device's own labels are never
used.  Test plumbing only: what LaneDups.qualities computes on the GPU is compared against this."""
from __future__ import annotations

import numpy as np

from lanemismatch_ref import lane_pairs

MAX_D = 7
MAX_BINS = 8
VALUES = 64
LANE_COLS = 4                  # Pairs, Profiled, Observations, Mismatches
TILE_COLS = 4


def bin_table(edges):
    """-> uint8 [64]: bin(q) = the largest i with edges[i] <= q"""
    edges = [int(e) for e in edges]
    assert 1 <= len(edges) <= MAX_BINS and edges[0] == 0 and all(0 <= e < VALUES for e in edges)
    assert all(a <= b for a, b in zip(edges, edges[1:]))
    return np.array([max(i for i, e in enumerate(edges) if e <= q) for q in range(VALUES)], dtype=np.uint8)


def qualities_end_to_end(tiles, n, max_tiles):
    """-> uint8 [L, max_tiles * n]: byte >> 2 of the lane as one tile (zero for an index never added)"""
    L = len(tiles[0][1]) if tiles else 0
    q = np.zeros((L, max_tiles * n), dtype=np.uint8)
    for ti, planes, _ in tiles:
        for c, p in enumerate(planes):
            q[c, ti * n:(ti + 1) * n] = np.asarray(p, dtype=np.uint8)[:n] >> 2
    return q


def lane_qualities(tiles, n, max_tiles, labels, max_d, edges):
    """tiles: [(tile_index, [L planes of n bytes], filter bytes)], labels uint32 [max_tiles, n] -> (lane row int64 [4],
    tile rows int64 [max_tiles, 4], qhist int64 [64], obs int64 [8, 8], mis int64 [8, 8])."""
    assert 0 <= max_d <= MAX_D
    table = bin_table(edges)
    ids, roots, a, b = lane_pairs(tiles, n, max_tiles, labels)
    L = a.shape[0]
    qual = qualities_end_to_end(tiles, n, max_tiles)
    qhist = np.zeros(VALUES, dtype=np.int64)
    for ti, _, filt in tiles:
        pf = (np.asarray(filt, dtype=np.uint8)[:n] & 1).astype(bool)
        qhist += np.bincount(qual[:, ti * n:(ti + 1) * n][:, pf].reshape(-1), minlength=VALUES)
    differ = a != b
    d = differ.sum(axis=0).astype(np.int64)
    profiled = d <= max_d
    qa, qb = table[qual[:, roots[profiled]]], table[qual[:, ids[profiled]]]
    cell = qa.astype(np.int64) * MAX_BINS + qb
    obs = np.bincount(cell.reshape(-1), minlength=MAX_BINS * MAX_BINS).reshape(MAX_BINS, MAX_BINS).astype(np.int64)
    mis = np.bincount(cell[differ[:, profiled]], minlength=MAX_BINS * MAX_BINS).reshape(MAX_BINS, MAX_BINS).astype(np.int64)
    tile = ids // n
    trow = np.zeros((max_tiles, TILE_COLS), dtype=np.int64)
    trow[:, 0] = np.bincount(tile, minlength=max_tiles)
    trow[:, 1] = np.bincount(tile[profiled], minlength=max_tiles)
    trow[:, 2] = trow[:, 1] * L
    trow[:, 3] = np.bincount(tile, weights=d * profiled, minlength=max_tiles).astype(np.int64)
    return trow.sum(axis=0).astype(np.int64), trow, qhist, obs, mis


def check_quality_identities(lane, trow, qhist, obs, mis, max_d, L, n_bins, mismatch=None, pf_wells=None, equality=False,
                             shallower=None):
    """What the header promises of any result.  mismatch: (lane row, tile rows, ...) of the mismatch pass at the same
    max_d; pf_wells: the PF wells of the added tiles; equality: the labels are classes; shallower: (.., obs, mis) of the
    same lane at max_d - 1."""
    lane, trow, qhist, obs, mis = (np.asarray(v) for v in (lane, trow, qhist, obs, mis))
    pairs, profiled, observations, mismatches = (int(v) for v in lane)
    assert lane.shape == (LANE_COLS,) and trow.shape[1] == TILE_COLS and qhist.shape == (VALUES,)
    assert obs.shape == mis.shape == (MAX_BINS, MAX_BINS)
    assert (trow.sum(axis=0) == lane).all() and (trow[:, 1] <= trow[:, 0]).all()
    assert observations == profiled * L == obs.sum() and (trow[:, 2] == trow[:, 1] * L).all()
    assert mis.sum() == mismatches and (mis >= 0).all() and (mis <= obs).all()
    assert mismatches <= profiled * max_d
    assert not obs[n_bins:].any() and not obs[:, n_bins:].any()
    assert (qhist >= 0).all()
    if mismatch is not None:
        m_lane, m_tiles = np.asarray(mismatch[0]), np.asarray(mismatch[1])
        assert (lane[[0, 1, 3]] == m_lane[:3]).all() and (trow[:, [0, 1, 3]] == m_tiles[:, :3]).all()
    if pf_wells is not None:
        assert qhist.sum() == L * int(pf_wells)
    if equality:
        assert not mis.any() and mismatches == 0 and profiled == pairs and obs.sum() == pairs * L
    if shallower is not None:
        assert (np.asarray(shallower[-2]) <= obs).all() and (np.asarray(shallower[-1]) <= mis).all()
