"""Host reference of a lane's duplication by insert length (include/welldup_laneadapter.h) in numpy, straight from
the definitions: the lane's tiles laid end to end as lanenear_ref does, a(w) of every PF well found by a loop over the
positions p - o(p), mism(p) and allowed(p) as the header writes them -, the population of a well read off the labels -
group sizes by bincount of the labels, never from a members array -, and the rows and the histogram read off that.  The
labels come from lanedups_ref.lane_dups or lanenear_ref.lane_near_dups - the device's own labels are never used.
first_match_literal says the same for one read char by char in plain Python.
Test plumbing only: what LaneDups.adapter computes on the GPU is compared against this."""
from __future__ import annotations

import numpy as np

from lanenear_ref import lay_end_to_end
from tiledups_ref import INVALID

HIST_COLS = 4                  # Single, Roots, Copies, FamilyWells
LANE_COLS = 10                 # PF, Single, Roots, Copies, AdSingle, AdRoots, AdCopies, AdFamilyWells, Inexact, Partial
TILE_COLS = 5                  # PF, Adapter, Copies, CopiesAdapter, SumA
SINGLE, ROOT, COPY = 0, 1, 2
MIN_LEN, MAX_LEN, MAX_E, MIN_OVERLAP = 8, 32, 3, 3
NAMES = {"truseq": "AGATCGGAAGAGC", "nextera": "CTGTCTCTTATACACATCT", "smallrna": "TGGAATTCTCGG"}


def codes_of(seq):
    return np.array(["ACGT".index(ch) for ch in seq.upper()], dtype=np.uint8)


def allowed(L, m, e, o, p):
    """allowed(p) of the header; -1 where p cannot match (L - p < O)"""
    over = min(m, L - p)
    return -1 if over < o else e if over == m else e * over // m


def ge_vectors(L, m, e, o):
    """The bit vectors over positions the kernel matches by, as Python integers: ge[x] has bit p set where
    allowed(p) >= x and p <= L - O, for x = 0 .. 3."""
    ge = [0, 0, 0, 0]
    for p in range(L - o + 1):
        for x in range(allowed(L, m, e, o, p) + 1):
            ge[x] |= 1 << p
    return ge


def first_matches(reads, codes, e, o):
    """reads: codes uint8 [L, P] (A 0, C 1, G 2, T 3, N 4) -> (a int64 [P], L where nothing matches; mism int64 [P]
    of the first match, 0 where none)"""
    reads, codes = np.asarray(reads), np.asarray(codes, dtype=np.uint8)
    L, P = reads.shape
    m = codes.size
    assert MIN_LEN <= m <= MAX_LEN and 0 <= e <= MAX_E and MIN_OVERLAP <= o <= min(m, L) and (codes <= 3).all()
    a = np.full(P, L, dtype=np.int64)
    mism = np.zeros(P, dtype=np.int64)
    for p in range(L - o + 1):
        over = min(m, L - p)
        mm = (reads[p:p + over] != codes[:over, None]).sum(axis=0)
        hit = (a == L) & (mm <= allowed(L, m, e, o, p))
        a[hit] = p
        mism[hit] = mm[hit]
    return a, mism


def first_match_literal(read, codes, e, o):
    """(a, mism of the first match) of one read, char by char"""
    L, m = len(read), len(codes)
    for p in range(L):
        if L - p < o:
            break
        over = m if m < L - p else L - p
        mm = 0
        for j in range(over):
            if int(read[p + j]) != int(codes[j]):
                mm += 1
        if mm <= (e if over == m else (e * over) // m):
            return p, mm
    return L, 0


def wells_of(tiles, n, max_tiles, labels, codes, e, o):
    """-> (global ids int64 [P] of the PF wells, a int64 [P], mism int64 [P], population int64 [P], group size int64
    [P] - of the well's group, whatever the well is in it -, L)"""
    reads, pf = lay_end_to_end(tiles, n, max_tiles)
    flat = np.asarray(labels, dtype=np.uint32).reshape(-1)
    assert flat.size == max_tiles * n and ((flat != INVALID) == pf).all()
    ids = np.flatnonzero(pf).astype(np.int64)
    lab = flat[ids].astype(np.int64)
    assert (lab <= ids).all() and (flat[lab] == lab).all()             # a root is the smallest id, and its own root
    size = np.bincount(lab, minlength=flat.size)[lab].astype(np.int64)
    pop = np.where(lab != ids, COPY, np.where(size > 1, ROOT, SINGLE)).astype(np.int64)
    a, mism = first_matches(reads[:, ids], codes, e, o)
    return ids, a, mism, pop, size, reads.shape[0]


def lane_adapter(tiles, n, max_tiles, labels, codes, e, o):
    """tiles: [(tile_index, [L planes of n bytes], filter bytes)], labels uint32 [max_tiles, n], codes: the adapter,
    0 .. 3 -> (lane row int64 [LANE_COLS], tile rows int64 [max_tiles, TILE_COLS], hist int64 [L + 1, HIST_COLS])."""
    ids, a, mism, pop, size, L = wells_of(tiles, n, max_tiles, labels, codes, e, o)
    m = len(codes)
    ad = a < L
    lane = np.zeros(LANE_COLS, dtype=np.int64)
    hist = np.zeros((L + 1, HIST_COLS), dtype=np.int64)
    lane[0] = ids.size
    for p in (SINGLE, ROOT, COPY):
        lane[1 + p] = (pop == p).sum()
        lane[4 + p] = ((pop == p) & ad).sum()
        hist[:, p] = np.bincount(a[pop == p], minlength=L + 1)
    roots = pop == ROOT
    lane[7] = size[roots & ad].sum()
    lane[8] = (ad & (mism >= 1)).sum()
    lane[9] = (ad & (L - a < m)).sum()
    hist[:, 3] = np.bincount(a[roots], weights=size[roots], minlength=L + 1).astype(np.int64)
    tile = ids // n
    copies = pop == COPY
    trow = np.zeros((max_tiles, TILE_COLS), dtype=np.int64)
    trow[:, 0] = np.bincount(tile, minlength=max_tiles)
    trow[:, 1] = np.bincount(tile[ad], minlength=max_tiles)
    trow[:, 2] = np.bincount(tile[copies], minlength=max_tiles)
    trow[:, 3] = np.bincount(tile[copies & ad], minlength=max_tiles)
    trow[:, 4] = np.bincount(tile[ad], weights=a[ad], minlength=max_tiles).astype(np.int64)
    return lane, trow, hist


def check_adapter_identities(lane, trow, hist, m, e, o, finish_lane=None, finish_tiles=None, equality=False,
                             looser=None):
    """What the header promises of any result.  finish_lane, finish_tiles: the rows of the finish the labels came from
    (PF, Classes and Redundant are columns 0, 1 and 3 of the lane row, PF column 0 of a tile row); equality: the labels
    are classes; looser: the result of the same lane and adapter at an E at least as large and an O at most as large
    (identity 7)."""
    lane, trow, hist = np.asarray(lane), np.asarray(trow), np.asarray(hist)
    assert lane.shape == (LANE_COLS,) and trow.shape[1] == TILE_COLS and hist.shape[1] == HIST_COLS
    L = hist.shape[0] - 1
    pos = np.arange(L + 1)
    pf, single, roots, copies = (int(v) for v in lane[:4])
    assert (lane >= 0).all() and (trow >= 0).all() and (hist >= 0).all()
    assert pf == single + roots + copies                                                   # 1
    if finish_lane is not None:
        assert pf == finish_lane[0] and roots == finish_lane[1] and copies == finish_lane[3]
    if finish_tiles is not None:
        assert (trow[:, 0] == np.asarray(finish_tiles)[:, 0]).all()
    assert (hist[:, :3].sum(axis=0) == lane[1:4]).all()                                    # 2
    assert (hist[:L, :3].sum(axis=0) == lane[4:7]).all() and hist[:L, 3].sum() == lane[7]  # 3
    assert hist[:, 3].sum() == roots + copies and (hist[:, 3] >= 2 * hist[:, 1]).all()     # 4
    assert (hist[:, 3][hist[:, 1] == 0] == 0).all()
    assert not hist[L - o + 1:L].any()                                                     # (no position beyond L - O)
    if equality:                                                                           # 5
        assert (hist[:, 2] == hist[:, 3] - hist[:, 1]).all()
    wells = hist[:, :3].sum(axis=1)                                                        # 6
    want = [pf, lane[4:7].sum(), copies, lane[6], (pos[:L] * wells[:L]).sum()]
    assert trow.sum(axis=0).tolist() == [int(v) for v in want]
    assert (trow[:, 1] <= trow[:, 0]).all() and (trow[:, 3] <= trow[:, 1]).all() and (trow[:, 3] <= trow[:, 2]).all()
    assert (trow[:, 4] <= (L - o) * trow[:, 1]).all()
    if looser is not None:                                                                 # 7
        ll, lt, lh = (np.asarray(v) for v in looser)
        assert (ll[:4] == lane[:4]).all()
        assert (np.cumsum(lh[:L, :3].sum(axis=1)) >= np.cumsum(wells[:L])).all()
    with_ad = int(lane[4:7].sum())                                                         # 8
    assert 0 <= lane[8] <= with_ad and 0 <= lane[9] <= with_ad
    if e == 0:
        assert lane[8] == 0
    if o == m:
        assert lane[9] == 0
