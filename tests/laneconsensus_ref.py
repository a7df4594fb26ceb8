"""Host reference of a lane's errors against its families' vote (include/welldup_laneconsensus.h) in numpy: the lane's
tiles laid end to end as lanenear_ref does, the families read off the labels - their members by sorting the labels,
never from a members array or a list in any order but ascending -, the vote per cycle by counting the five codes, and
the header's definitions read off that, family by family.  The labels come from lanedups_ref.lane_dups or
lanenear_ref.lane_near_dups - the device's own labels are never used.
Test plumbing only: what LaneDups.consensus computes on the GPU is compared against this."""
from __future__ import annotations

import numpy as np

from lanenear_ref import lay_end_to_end
from tiledups_ref import INVALID

LANE_COLS = 20                 # Families, Wells, Profiled, Mismatches, WithN, Undecided, UndecidedCalls, FirstWellOff,
TILE_COLS = 4                  # PairFamilies, LargeFamilies, LargeWells, Dist[9]; Wells, Profiled, Mismatches, WithN
DIST_BINS = 9
MAX_D = 7
MIN_FAMILY, MAX_FAMILY = 3, 4096
FAMILIES, WELLS, PROFILED, MISMATCHES, WITH_N, UNDECIDED, UNDECIDED_CALLS, FIRST_OFF, PAIRS, LARGE, LARGE_WELLS, DIST = range(12)


def families_of(labels):
    """labels uint32 [max_tiles, n] -> [(root, members int64 ascending, the root first)] for every group of two or more"""
    flat = np.asarray(labels, dtype=np.uint32).reshape(-1)
    ids = np.flatnonzero(flat != INVALID).astype(np.int64)
    lab = flat[ids].astype(np.int64)
    assert (lab <= ids).all() and (flat[lab] == lab).all()             # a root is the smallest id, and its own root
    order = np.argsort(lab, kind="stable")
    lab, ids = lab[order], ids[order]
    cut = np.flatnonzero(np.diff(lab)) + 1
    return [(int(m[0]), m) for m in np.split(ids, cut) if m.size >= 2]


def vote(sub):
    """sub uint8 [L, n]: the codes of a family's wells -> (consensus int64 [L], decided bool [L]): the code strictly
    more than half of the n wells hold"""
    counts = (sub[:, :, None] == np.arange(5)[None, None, :]).sum(axis=1)
    return counts.argmax(axis=1), 2 * counts.max(axis=1) > sub.shape[1]


def lane_consensus(tiles, n, max_tiles, labels, max_d, max_family):
    """tiles: [(tile_index, [L planes of n bytes], filter bytes)], labels uint32 [max_tiles, n] -> (lane row int64
    [LANE_COLS], tile rows int64 [max_tiles, TILE_COLS], calls int64 [L, 5, 5])."""
    assert 0 <= max_d <= MAX_D and MIN_FAMILY <= max_family <= MAX_FAMILY
    codes, pf = lay_end_to_end(tiles, n, max_tiles)
    L = codes.shape[0]
    lane = np.zeros(LANE_COLS, dtype=np.int64)
    trow = np.zeros((max_tiles, TILE_COLS), dtype=np.int64)
    calls = np.zeros((L, 5, 5), dtype=np.int64)
    cyc = np.arange(L)
    for root, m in families_of(labels):
        assert pf[m].all()
        if m.size == 2:
            lane[PAIRS] += 1
            continue
        if m.size > max_family:
            lane[LARGE] += 1
            lane[LARGE_WELLS] += m.size
            continue
        sub = codes[:, m]
        cons, decided = vote(sub)
        off = (sub != cons[:, None]) & decided[:, None]
        with_n = off & ((sub == 4) | (cons[:, None] == 4))
        d = off.sum(axis=0)
        prof = d <= max_d
        lane[FAMILIES] += 1
        lane[UNDECIDED] += int((~decided).sum())
        lane[UNDECIDED_CALLS] += int((~decided).sum()) * int(prof.sum())
        lane[FIRST_OFF] += int(d[0] >= 1)
        lane[DIST:] += np.bincount(np.minimum(d, DIST_BINS - 1), minlength=DIST_BINS)
        tile = m // n
        trow[:, 0] += np.bincount(tile, minlength=max_tiles)
        trow[:, 1] += np.bincount(tile[prof], minlength=max_tiles)
        trow[:, 2] += np.bincount(tile[prof], weights=d[prof], minlength=max_tiles).astype(np.int64)
        trow[:, 3] += np.bincount(tile[prof], weights=with_n.sum(axis=0)[prof], minlength=max_tiles).astype(np.int64)
        own = sub[decided][:, prof]                                        # [decided cycles, profiled wells]
        np.add.at(calls, (np.broadcast_to(cyc[decided][:, None], own.shape),
                          np.broadcast_to(cons[decided][:, None], own.shape), own), 1)
    lane[WELLS:WITH_N + 1] = trow.sum(axis=0)
    return lane, trow, calls


def check_consensus_identities(lane, trow, calls, max_d, finish_lane=None, equality=False, wider=None, lower=None):
    """What the header promises of any result.  finish_lane: the lane row of the finish the labels came from (Classes
    and Redundant are columns 1 and 3); equality: the labels are classes; wider: the result of the same lane at a
    larger max_family, lower: at a smaller max_d (identity 10)."""
    lane, trow, calls = np.asarray(lane), np.asarray(trow), np.asarray(calls)
    assert lane.shape == (LANE_COLS,) and trow.shape[1] == TILE_COLS and calls.shape[1:] == (5, 5)
    assert (lane >= 0).all() and (trow >= 0).all() and (calls >= 0).all()
    L = calls.shape[0]
    dist = lane[DIST:]
    if finish_lane is not None:
        assert lane[PAIRS] + lane[FAMILIES] + lane[LARGE] == finish_lane[1]                # 1
        assert 2 * lane[PAIRS] + lane[WELLS] + lane[LARGE_WELLS] == finish_lane[1] + finish_lane[3]      # 2
    assert dist.sum() == lane[WELLS]                                                       # 3
    assert lane[PROFILED] == dist[:max_d + 1].sum()                                        # 4
    assert lane[MISMATCHES] == (np.arange(max_d + 1) * dist[:max_d + 1]).sum()             # 5
    diag = calls[:, np.arange(5), np.arange(5)]
    assert lane[MISMATCHES] == calls.sum() - diag.sum()
    assert lane[WITH_N] == calls[:, 4, :4].sum() + calls[:, :4, 4].sum()
    assert calls.sum() == lane[PROFILED] * L - lane[UNDECIDED_CALLS]                       # 6
    assert (trow.sum(axis=0) == lane[WELLS:WITH_N + 1]).all()                              # 7
    assert (trow[:, 1] <= trow[:, 0]).all() and (trow[:, 3] <= trow[:, 2]).all()
    rows = calls.sum(axis=2)
    assert (diag[rows > 0] > 0).all()                                                      # 8
    if lane[PROFILED] == lane[WELLS]:
        assert (2 * diag[rows > 0] > rows[rows > 0]).all()
    assert lane[FAMILIES] * 3 <= lane[WELLS] and lane[FIRST_OFF] <= lane[FAMILIES]
    assert lane[UNDECIDED] <= lane[FAMILIES] * L and lane[LARGE_WELLS] >= 4 * lane[LARGE]
    if equality:                                                                           # 9
        assert dist[0] == lane[WELLS] and lane[UNDECIDED] == lane[MISMATCHES] == lane[FIRST_OFF] == 0
        assert calls.sum() == diag.sum()
    if wider is not None:                                                                  # 10
        wl, wt, wc = (np.asarray(a) for a in wider)
        assert wl[FAMILIES] >= lane[FAMILIES] and wl[WELLS] >= lane[WELLS] and (wc >= calls).all() and (wt >= trow).all()
        assert wl[LARGE] <= lane[LARGE] and wl[PAIRS] == lane[PAIRS]
    if lower is not None:
        ll, lt, lc = (np.asarray(a) for a in lower)
        assert (lc <= calls).all() and (ll[DIST:] == dist).all() and ll[PROFILED] <= lane[PROFILED]
