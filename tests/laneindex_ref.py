"""Host reference of a lane's duplication per index read (include/welldup_laneindex.h) in numpy: the PF wells of a
lane grouped by the bases of their index cycles, and a label array - the classes of lanedups_ref or the clusters of
lanenear_ref - counted per group.  Twice: in array arithmetic (lane_index), and read off the header's definitions
one well at a time with dicts and sets (lane_index_literal).
Test plumbing only: what LaneDups.index_finish computes on the GPU is compared against this."""
from __future__ import annotations

import numpy as np

from tiledups_ref import INVALID, codes_of

GROUP_COLS = 5                 # PF, InLane, InGroup, GroupRedundant, Mixed
LANE_COLS = 5                  # Groups, Listed, GroupSpans, MixedClasses, MixedWells
MAX_CYCLES = 20


def index_keys(index_tiles, n, max_tiles):
    """index_tiles: [(tile_index, [I planes of n bytes])] -> (keys uint64 [max_tiles * n], given bool [max_tiles]):
    ten 3-bit codes per 32-bit word, the first word low; 0 for the wells of a tile index that got no planes."""
    keys = np.zeros(max_tiles * n, dtype=np.uint64)
    given = np.zeros(max_tiles, dtype=bool)
    for ti, planes in index_tiles:
        assert 1 <= len(planes) <= MAX_CYCLES and not given[ti]
        given[ti] = True
        codes = codes_of(planes, n).astype(np.uint64)
        k = np.zeros(n, dtype=np.uint64)
        for c in range(len(planes)):
            k |= codes[c] << np.uint64(32 * (c // 10) + 3 * (c % 10))
        keys[ti * n:(ti + 1) * n] = k
    return keys, given


def key_of(bases: str) -> int:
    """the key of an index read written as bases"""
    key = 0
    for c, b in enumerate(bases):
        key |= "ACGTN".index(b) << (32 * (c // 10) + 3 * (c % 10))
    return key


def _listing(keys, rows, min_pf):
    """all groups' keys and rows -> (Other row, listed rows by (-PF, key), their keys)"""
    keys, rows = np.asarray(keys, dtype=np.uint64), np.asarray(rows, dtype=np.int64).reshape(-1, GROUP_COLS)
    listed = rows[:, 0] >= min_pf
    other = rows[~listed].sum(axis=0).astype(np.int64)
    rows, keys = rows[listed], keys[listed]
    order = np.lexsort((keys, -rows[:, 0]))
    return other, rows[order], keys[order]


def lane_index(index_tiles, labels, n, max_tiles, min_pf=1):
    """labels uint32 [max_tiles, n] (INVALID: no PF well) -> (lane index row int64 [LANE_COLS], Other row int64
    [GROUP_COLS], listed group rows int64 [listed, GROUP_COLS] by (-PF, key), their keys uint64 [listed])."""
    flat = np.asarray(labels, dtype=np.uint32).reshape(-1)
    keys, given = index_keys(index_tiles, n, max_tiles)
    ids = np.flatnonzero(flat != INVALID)
    assert given[np.unique(ids // n)].all()
    lane = np.zeros(LANE_COLS, dtype=np.int64)
    if ids.size == 0:
        return lane, np.zeros(GROUP_COLS, dtype=np.int64), np.zeros((0, GROUP_COLS), dtype=np.int64), np.zeros(0, dtype=np.uint64)
    ukeys, group = np.unique(keys[ids], return_inverse=True)
    group = np.asarray(group).reshape(-1).astype(np.int64)
    G = ukeys.size
    lab = flat[ids].astype(np.int64)
    class_size = np.bincount(lab, minlength=flat.size)[lab]
    c = class_size >= 2                                   # the wells in a class
    pairs, sub, held = np.unique(lab[c] * G + group[c], return_inverse=True, return_counts=True)
    sub = np.asarray(sub).reshape(-1)
    first = np.full(pairs.size, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(first, sub, ids[c])                     # the smallest global id of every subgroup
    gc = group[c]
    rows = np.zeros((G, GROUP_COLS), dtype=np.int64)
    rows[:, 0] = np.bincount(group, minlength=G)
    rows[:, 1] = np.bincount(gc, minlength=G)
    rows[:, 2] = np.bincount(gc[held[sub] >= 2], minlength=G)
    rows[:, 3] = np.bincount(gc[ids[c] != first[sub]], minlength=G)
    rows[:, 4] = np.bincount(gc[held[sub] < class_size[c]], minlength=G)
    other, listed, lkeys = _listing(ukeys, rows, min_pf)
    lane[0] = G
    lane[1] = listed.shape[0]
    lane[2] = pairs.size
    lane[3] = int((np.bincount(pairs // G) >= 2).sum()) if pairs.size else 0
    lane[4] = rows[:, 4].sum()
    return lane, other, listed, lkeys


def lane_index_literal(index_tiles, labels, n, max_tiles, min_pf=1):
    """lane_index, one well at a time (small lanes)."""
    flat = np.asarray(labels, dtype=np.uint32).reshape(-1).tolist()
    keys, given = index_keys(index_tiles, n, max_tiles)
    keys = keys.tolist()
    classes, groups = {}, {}
    for g, lab in enumerate(flat):
        if lab == INVALID:
            continue
        assert given[g // n]
        classes.setdefault(lab, []).append(g)
        groups.setdefault(keys[g], []).append(g)
    rows = {k: [len(wells), 0, 0, 0, 0] for k, wells in groups.items()}
    spans = mixed_classes = 0
    for lab, wells in classes.items():
        if len(wells) < 2:
            continue
        touched = sorted({keys[g] for g in wells})
        spans += len(touched)
        mixed_classes += len(touched) >= 2
        for k in touched:
            here = sorted(g for g in wells if keys[g] == k)             # the subgroup
            rows[k][1] += len(here)
            if len(here) >= 2:
                rows[k][2] += len(here)
            rows[k][3] += len(here) - 1
            if len(touched) >= 2:
                rows[k][4] += len(here)
    ks = sorted(rows)
    other, listed, lkeys = _listing(ks, [rows[k] for k in ks], min_pf)
    lane = np.array([len(rows), listed.shape[0], spans, mixed_classes, sum(r[4] for r in rows.values())], dtype=np.int64)
    return lane, other, listed, lkeys


def check_index_identities(result, eq_lane):
    """What the header promises of any result; eq_lane: the lane row (classes or clusters, NearPairs or not) the
    labels belong to - [PF, Classes, InClasses, Redundant, ...]."""
    lane, other, rows, keys = result
    total = rows.sum(axis=0) + other
    pf, classes, in_classes = int(eq_lane[0]), int(eq_lane[1]), int(eq_lane[2])
    assert lane[1] == rows.shape[0] == keys.shape[0] <= lane[0]
    assert total[0] == pf and total[1] == in_classes
    assert total[3] == in_classes - lane[2]               # the redundancy within libraries
    assert lane[2] >= classes and total[4] == lane[4]
    assert (lane[2] == classes) == (lane[3] == 0) == (lane[4] == 0)
    assert (rows[:, 2] <= rows[:, 1]).all() and (rows[:, 3] <= rows[:, 2]).all() and (rows[:, 1] <= rows[:, 0]).all()
    assert (rows[:, 4] <= rows[:, 1]).all() and lane[3] <= classes
    if rows.shape[0] > 1:
        order = np.lexsort((keys, -rows[:, 0]))
        assert (order == np.arange(rows.shape[0])).all() and np.unique(keys).size == keys.size
    if lane[0] == 1 and rows.shape[0] == 1:               # a single index read
        assert rows[0].tolist() == [pf, in_classes, in_classes, int(eq_lane[3]), 0]


# ---- the index reads of lanenear_ref.hand_made_lane and the hand-worked answer ----------------------
_BYTE = {"A": 0x40, "C": 0x81, "G": 0xC2, "T": 0x23, "N": 0}


def hand_made_index():
    """Two index cycles for the sixteen wells of lanenear_ref.hand_made_lane (ids in brackets; 16 fails the filter):
         index 0   [0] AC   [1] AC   [2] AC   [3] GT
         index 1   [4] AC   [5] GT   [6] GT   [7] NN
         index 2   [8] AC   [9] AC  [10] GT  [11] NN
         index 4  [16] AC* [17] GT  [18] AC  [19] NN
    Groups: AC {0, 1, 2, 4, 8, 9, 18}, GT {3, 5, 6, 10, 17}, NN {7, 11, 19}.
    Classes (K = 0): {0, 18} lies in AC; {2, 17} has 2 in AC and 17 in GT: mixed.
    Clusters (K = 1): {0, 4, 8, 18} lies in AC; {1, 6} and {2, 17} are AC + GT, {3, 7} and {10, 11} GT + NN."""
    reads = {0: "AC", 1: "AC", 2: "AC", 3: "GT", 4: "AC", 5: "GT", 6: "GT", 7: "NN", 8: "AC", 9: "AC", 10: "GT", 11: "NN",
             16: "AC", 17: "GT", 18: "AC", 19: "NN"}
    return [(ti, [np.array([_BYTE[reads[ti * 4 + w][c]] | (0 if reads[ti * 4 + w][c] == "N" else 4 * w)
                            for w in range(4)], dtype=np.uint8) for c in range(2)]) for ti in (0, 1, 2, 4)]


HAND_KEYS = {"AC": 0o10, "GT": 0o32, "NN": 0o44}          # A C G T N = 0 1 2 3 4, the first cycle lowest
HAND_INDEX = {
    # K -> min_pf -> the answer; rows in the order AC (7 PF wells), GT (5), NN (3)
    0: {1: dict(lane=[3, 3, 3, 1, 2], other=[0, 0, 0, 0, 0], keys=["AC", "GT", "NN"],
                rows=[[7, 3, 2, 1, 1], [5, 1, 0, 0, 1], [3, 0, 0, 0, 0]]),
        4: dict(lane=[3, 2, 3, 1, 2], other=[3, 0, 0, 0, 0], keys=["AC", "GT"],
                rows=[[7, 3, 2, 1, 1], [5, 1, 0, 0, 1]]),
        8: dict(lane=[3, 0, 3, 1, 2], other=[15, 4, 2, 1, 2], keys=[], rows=[])},
    1: {1: dict(lane=[3, 3, 9, 4, 8], other=[0, 0, 0, 0, 0], keys=["AC", "GT", "NN"],
                rows=[[7, 6, 4, 3, 2], [5, 4, 0, 0, 4], [3, 2, 0, 0, 2]]),
        6: dict(lane=[3, 1, 9, 4, 8], other=[8, 6, 0, 0, 6], keys=["AC"], rows=[[7, 6, 4, 3, 2]])},
}
