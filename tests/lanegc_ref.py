"""Host reference of a lane's duplication against its reads' GC content (include/welldup_lanegc.h) in numpy: the
lane's tiles laid end to end as lanenear_ref does, g and n of every PF well counted from the host tiles' bytes, the
population of a well read off the labels - group sizes by bincount of the labels, never from a members array -, and
the header's definitions read off that.  The labels come from lanedups_ref.lane_dups or lanenear_ref.lane_near_dups -
the device's own labels are never used.  lane_gc_literal says the same well by well in plain Python.
Test plumbing only: what LaneDups.gc computes on the GPU is compared against this."""
from __future__ import annotations

import numpy as np

from lanenear_ref import lay_end_to_end
from tiledups_ref import INVALID

HIST_COLS = 4                  # Single, Roots, Copies, FamilyWells
LANE_COLS = 8                  # PF, Single, Roots, Copies, SkipSingle, SkipRoots, SkipCopies, SkipFamilyWells
TILE_COLS = 5                  # PF, Counted, GC, CopiesCounted, CopiesGC
SINGLE, ROOT, COPY = 0, 1, 2


def wells_of(tiles, n, max_tiles, labels):
    """-> (global ids int64 [P] of the PF wells, g int64 [P], n int64 [P], population int64 [P], group size int64 [P]
    - of the well's group, whatever the well is in it -, L)"""
    codes, pf = lay_end_to_end(tiles, n, max_tiles)
    flat = np.asarray(labels, dtype=np.uint32).reshape(-1)
    assert flat.size == max_tiles * n and ((flat != INVALID) == pf).all()
    ids = np.flatnonzero(pf).astype(np.int64)
    lab = flat[ids].astype(np.int64)
    assert (lab <= ids).all() and (flat[lab] == lab).all()             # a root is the smallest id, and its own root
    size = np.bincount(lab, minlength=flat.size)[lab].astype(np.int64)
    pop = np.where(lab != ids, COPY, np.where(size > 1, ROOT, SINGLE)).astype(np.int64)
    mine = codes[:, ids]
    g = ((mine == 1) | (mine == 2)).sum(axis=0).astype(np.int64)
    nn = (mine == 4).sum(axis=0).astype(np.int64)
    return ids, g, nn, pop, size, codes.shape[0]


def lane_gc(tiles, n, max_tiles, labels, max_n):
    """tiles: [(tile_index, [L planes of n bytes], filter bytes)], labels uint32 [max_tiles, n] -> (lane row int64
    [LANE_COLS], tile rows int64 [max_tiles, TILE_COLS], hist int64 [L + 1, HIST_COLS])."""
    ids, g, nn, pop, size, L = wells_of(tiles, n, max_tiles, labels)
    assert 0 <= max_n <= L
    skip = nn > max_n
    lane = np.zeros(LANE_COLS, dtype=np.int64)
    hist = np.zeros((L + 1, HIST_COLS), dtype=np.int64)
    lane[0] = ids.size
    for p in (SINGLE, ROOT, COPY):
        lane[1 + p] = (pop == p).sum()
        lane[4 + p] = ((pop == p) & skip).sum()
        hist[:, p] = np.bincount(g[(pop == p) & ~skip], minlength=L + 1)
    roots = pop == ROOT
    lane[7] = size[roots & skip].sum()
    hist[:, 3] = np.bincount(g[roots & ~skip], weights=size[roots & ~skip], minlength=L + 1).astype(np.int64)
    tile = ids // n
    copies = (pop == COPY) & ~skip
    trow = np.zeros((max_tiles, TILE_COLS), dtype=np.int64)
    trow[:, 0] = np.bincount(tile, minlength=max_tiles)
    trow[:, 1] = np.bincount(tile[~skip], minlength=max_tiles)
    trow[:, 2] = np.bincount(tile[~skip], weights=g[~skip], minlength=max_tiles).astype(np.int64)
    trow[:, 3] = np.bincount(tile[copies], minlength=max_tiles)
    trow[:, 4] = np.bincount(tile[copies], weights=g[copies], minlength=max_tiles).astype(np.int64)
    return lane, trow, hist


def lane_gc_literal(tiles, n, max_tiles, labels, max_n):
    """lane_gc, read off the header's definitions one well at a time from the bytes (small lanes)."""
    flat = [int(v) for v in np.asarray(labels, dtype=np.uint32).reshape(-1)]
    L = len(tiles[0][1]) if tiles else 0
    lane, trow, hist = [0] * LANE_COLS, [[0] * TILE_COLS for _ in range(max_tiles)], [[0] * HIST_COLS for _ in range(L + 1)]
    wells = {}
    for lab in flat:
        if lab != INVALID:
            wells[lab] = wells.get(lab, 0) + 1
    for ti, planes, filt in tiles:
        for w in range(n):
            if not filt[w] & 1:
                continue
            gid = ti * n + w
            read = [int(planes[c][w]) for c in range(L)]
            g = sum(1 for b in read if b != 0 and (b & 3) in (1, 2))
            nn = sum(1 for b in read if b == 0)
            pop = COPY if flat[gid] != gid else ROOT if wells[gid] > 1 else SINGLE
            lane[0] += 1
            lane[1 + pop] += 1
            trow[ti][0] += 1
            if nn > max_n:
                lane[4 + pop] += 1
                if pop == ROOT:
                    lane[7] += wells[gid]
                continue
            hist[g][pop] += 1
            if pop == ROOT:
                hist[g][3] += wells[gid]
            trow[ti][1] += 1
            trow[ti][2] += g
            if pop == COPY:
                trow[ti][3] += 1
                trow[ti][4] += g
    return np.array(lane, dtype=np.int64), np.array(trow, dtype=np.int64).reshape(max_tiles, TILE_COLS), \
        np.array(hist, dtype=np.int64).reshape(L + 1, HIST_COLS)


def check_gc_identities(lane, trow, hist, max_n, finish_lane=None, finish_tiles=None, equality=False, wider=None):
    """What the header promises of any result.  finish_lane, finish_tiles: the rows of the finish the labels came from
    (PF, Classes and Redundant are columns 0, 1 and 3 of the lane row, PF column 0 of a tile row); equality: the labels
    are classes; wider: the result of the same lane at a larger max_n (identity 5)."""
    lane, trow, hist = np.asarray(lane), np.asarray(trow), np.asarray(hist)
    assert lane.shape == (LANE_COLS,) and trow.shape[1] == TILE_COLS and hist.shape[1] == HIST_COLS
    L = hist.shape[0] - 1
    g = np.arange(L + 1)
    pf, single, roots, copies = (int(v) for v in lane[:4])
    assert (lane >= 0).all() and (trow >= 0).all() and (hist >= 0).all()
    assert pf == single + roots + copies                                                   # 1
    if finish_lane is not None:
        assert pf == finish_lane[0] and roots == finish_lane[1] and copies == finish_lane[3]
    if finish_tiles is not None:
        assert (trow[:, 0] == np.asarray(finish_tiles)[:, 0]).all()
    assert (hist[:, :3].sum(axis=0) == lane[1:4] - lane[4:7]).all()                        # 2
    assert hist[:, 3].sum() + lane[7] == roots + copies
    assert (hist[:, 3] >= 2 * hist[:, 1]).all() and lane[7] >= 2 * lane[5]
    assert (hist[:, 3][hist[:, 1] == 0] == 0).all()                                        # 3
    if max_n == L:                                                                         # 4
        assert not lane[4:].any()
    if wider is not None:                                                                  # 5
        wl, wt, wh = (np.asarray(a) for a in wider)
        assert (wl[:4] == lane[:4]).all() and (wl[4:] <= lane[4:]).all()
        assert (wh >= hist).all() and (wt >= trow).all()
    if equality:                                                                           # 6
        assert (hist[:, 2] == hist[:, 3] - hist[:, 1]).all() and lane[6] == lane[7] - lane[5]
    elif not lane[4:].any():
        assert hist[:, 2].sum() == hist[:, 3].sum() - hist[:, 1].sum()
    counted = hist[:, :3].sum(axis=1)                                                      # 7
    want = [pf, counted.sum(), (g * counted).sum(), hist[:, 2].sum(), (g * hist[:, 2]).sum()]
    assert trow.sum(axis=0).tolist() == [int(v) for v in want]
    assert (trow[:, 1] <= trow[:, 0]).all() and (trow[:, 3] <= trow[:, 1]).all() and (trow[:, 4] <= trow[:, 2]).all()
    assert (trow[:, 2] <= L * trow[:, 1]).all() and (trow[:, 4] <= L * trow[:, 3]).all()
