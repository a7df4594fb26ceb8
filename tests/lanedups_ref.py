"""Host reference of the read classes across the tiles of a lane (include/welldup_lanedups.h) in numpy, over a
list of (tile_index, planes, filter).  The reads are decoded to codes and the PF wells of the whole lane grouped
by their rows, by two independent methods: np.unique over the coded rows, and a dict keyed by a row's bytes.
Rows and labels follow from the groups by the header's definitions: once class by class (lane_dups_literal, a
Python set of tiles per class), once in array arithmetic for lanes of full tiles (lane_dups).
Test plumbing only: what the LaneDups accumulator computes on the GPU is compared against this."""
from __future__ import annotations

import numpy as np

from tiledups_ref import INVALID, SIZE_BINS, codes_of

LANE_COLS = 6 + SIZE_BINS      # PF, Classes, InClasses, Redundant, CrossTileClasses, TileSpans, size bins
TILE_COLS = 5                  # PF, InLane, InTile, TileRedundant, LaneRedundant


def _lane_rows(tiles, n):
    """-> (global ids int64 [m], coded rows uint8 [m, L]) of the PF wells of the lane, by global id."""
    ids, rows = [], []
    for ti, planes, filt in sorted(tiles, key=lambda t: t[0]):
        pf = np.flatnonzero(np.asarray(filt, dtype=np.uint8)[:n] & 1)
        ids.append(int(ti) * n + pf)
        rows.append(np.ascontiguousarray(codes_of(planes, n)[:, pf].T))
    L = len(tiles[0][1]) if tiles else 0
    if not ids:
        return np.zeros(0, dtype=np.int64), np.zeros((0, L), dtype=np.uint8)
    return np.concatenate(ids).astype(np.int64), np.concatenate(rows, axis=0)


def groups_by_unique(ids, rows):
    """group number per PF well: np.unique(axis=0) over the coded rows (21 codes of 3 bits to a uint64, nothing
    lost: sorting 13 million rows of three words takes a fraction of what rows of 50 bytes take)"""
    if rows.shape[0] == 0:
        return np.zeros(0, dtype=np.int64)
    if rows.shape[1] == 0:
        return np.zeros(rows.shape[0], dtype=np.int64)
    words = np.zeros((rows.shape[0], (rows.shape[1] + 20) // 21), dtype=np.uint64)
    for c in range(rows.shape[1]):
        words[:, c // 21] |= rows[:, c].astype(np.uint64) << np.uint64(3 * (c % 21))
    _, inverse = np.unique(words, axis=0, return_inverse=True)
    return np.asarray(inverse).reshape(-1).astype(np.int64)


def groups_by_dict(ids, rows):
    """group number per PF well: a dict of row bytes, in order of first appearance"""
    seen, out = {}, np.zeros(rows.shape[0], dtype=np.int64)
    for i in range(rows.shape[0]):
        out[i] = seen.setdefault(rows[i].tobytes(), len(seen))
    return out


def lane_dups(tiles, n, max_tiles, method="unique"):
    """tiles: [(tile_index, [L planes of n bytes], filter bytes)] -> (lane row int64 [LANE_COLS], tile rows int64
    [max_tiles, TILE_COLS], labels uint32 [max_tiles, n]).  Array arithmetic over the groups (a lane of full
    tiles has millions of classes); lane_dups_literal below says the same class by class."""
    assert len({t[0] for t in tiles}) == len(tiles) and all(0 <= t[0] < max_tiles for t in tiles)
    ids, rows = _lane_rows(tiles, n)
    group = (groups_by_unique if method == "unique" else groups_by_dict)(ids, rows)
    labels = np.full(max_tiles * n, INVALID, dtype=np.uint32)
    lane = np.zeros(LANE_COLS, dtype=np.int64)
    trow = np.zeros((max_tiles, TILE_COLS), dtype=np.int64)
    if ids.size == 0:
        return lane, trow, labels.reshape(max_tiles, n)
    tile = ids // n
    size = np.bincount(group)
    rep = np.full(size.shape[0], np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(rep, group, ids)                      # the smallest global id of every group
    in_class = size[group] >= 2
    labels[ids] = np.where(in_class, rep[group], ids)
    lane[0] = ids.size
    lane[1] = int((size >= 2).sum())
    lane[2] = int(in_class.sum())
    lane[3] = lane[2] - lane[1]
    lane[6:] = np.bincount(np.minimum(size[size >= 2], SIZE_BINS + 1) - 2, minlength=SIZE_BINS)[:SIZE_BINS]
    # the (class, tile) pairs and how many wells each holds
    pairs, held = np.unique(group[in_class] * max_tiles + tile[in_class], return_counts=True)
    lane[5] = pairs.size
    lane[4] = int((np.bincount(pairs // max_tiles) >= 2).sum()) if pairs.size else 0
    pair_tile = pairs % max_tiles
    trow[:, 0] = np.bincount(tile, minlength=max_tiles)
    trow[:, 1] = np.bincount(tile[in_class], minlength=max_tiles)
    trow[:, 2] = np.bincount(pair_tile[held >= 2], weights=held[held >= 2], minlength=max_tiles).astype(np.int64)
    trow[:, 3] = np.bincount(pair_tile, weights=held - 1, minlength=max_tiles).astype(np.int64)
    trow[:, 4] = np.bincount(tile[in_class & (ids != rep[group])], minlength=max_tiles)
    return lane, trow, labels.reshape(max_tiles, n)


def lane_dups_literal(tiles, n, max_tiles, method="dict"):
    """lane_dups, read off the header's definitions one class at a time (small lanes)."""
    ids, rows = _lane_rows(tiles, n)
    group = (groups_by_unique if method == "unique" else groups_by_dict)(ids, rows)
    labels = np.full(max_tiles * n, INVALID, dtype=np.uint32)
    lane = np.zeros(LANE_COLS, dtype=np.int64)
    trow = np.zeros((max_tiles, TILE_COLS), dtype=np.int64)
    labels[ids] = ids                                   # PF wells: their own id unless a class says otherwise
    np.add.at(trow[:, 0], ids // n, 1)
    lane[0] = ids.size
    for g in sorted(set(group.tolist())):
        members = np.sort(ids[group == g])
        if members.size < 2:
            continue
        rep = int(members[0])
        labels[members] = rep
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
            trow[t, 3] += here.size - 1                 # all but the smallest well index of the class on this tile
            trow[t, 4] += int((here != rep).sum())
    lane[3] = lane[2] - lane[1]
    return lane, trow, labels.reshape(max_tiles, n)


def check_identities(lane, trow):
    """What the header promises of any result."""
    assert lane[3] == lane[2] - lane[1]
    assert trow[:, 4].sum() == lane[3]                  # sum of LaneRedundant = Redundant
    assert trow[:, 3].sum() == lane[2] - lane[5]        # within tiles: InClasses - TileSpans
    assert lane[5] - lane[1] >= 0                       # across tiles: TileSpans - Classes
    assert (lane[2] - lane[5]) + (lane[5] - lane[1]) == lane[3]
    assert trow[:, 0].sum() == lane[0] and trow[:, 1].sum() == lane[2]
    assert lane[6:].sum() == lane[1] and lane[4] <= lane[1] <= lane[5]
    assert (trow[:, 2] <= trow[:, 1]).all() and (trow[:, 3] <= trow[:, 4]).all()


def members_of(labels, n):
    """labels [max_tiles, n] -> (tile index, well, class tile index, class well) int64 arrays of every well in a
    class, by global id."""
    flat = labels.reshape(-1)
    valid = np.flatnonzero(flat != INVALID)
    size = np.bincount(flat[valid].astype(np.int64), minlength=flat.size)
    g = valid[size[flat[valid].astype(np.int64)] >= 2]
    lab = flat[g].astype(np.int64)
    return g // n, g % n, lab // n, lab % n
