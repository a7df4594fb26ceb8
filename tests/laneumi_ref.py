"""Host reference of a lane's duplicates split by molecular identifier (include/welldup_laneumi.h) in numpy and plain
Python, straight from the definitions: the families read off the labels - their members by sorting the labels, never
from a members array or a list in any order but ascending -, the UMI read of a well its codes over the UMI planes, a
molecule a connected component of a family's wells under "at most E cycles differ", found by a union by brute force
over all pairs of the family.  The labels come from lanedups_ref.lane_dups or lanenear_ref.lane_near_dups - the
device's own labels are never used.
Test plumbing only: what LaneDups.umi computes on the GPU is compared against this."""
from __future__ import annotations

import numpy as np

from laneconsensus_ref import families_of
from tiledups_ref import INVALID, codes_of

LANE_COLS = 27
TILE_COLS = 3                  # Wells, UmiRedundant, Lone
BINS = 8
MAX_CYCLES, MAX_E, MAX_FAMILY = 20, 3, 1024
(WELLS, REDUNDANT, LONE, FAMILIES, MOLECULES, DISTINCT, SPLIT_FAMILIES, SPLIT_WELLS, WITH_N, LARGE, LARGE_WELLS, PER_FAMILY) = range(12)
SIZE = PER_FAMILY + BINS
BIN_NAMES = ("1", "2", "3", "4", "5-8", "9-16", "17-64", "65+")


def bin_of(v: int) -> int:
    """the bin of a count >= 1: 1, 2, 3, 4, 5-8, 9-16, 17-64, 65 or more"""
    assert v >= 1
    return v - 1 if v <= 4 else 4 if v <= 8 else 5 if v <= 16 else 6 if v <= 64 else 7


def umi_codes(umi_tiles, n, max_tiles):
    """umi_tiles: [(tile_index, [U planes of n bytes], ...)] -> (codes uint8 [max_tiles * n, U], given bool [max_tiles])"""
    U = len(umi_tiles[0][1]) if umi_tiles else 1
    assert 1 <= U <= MAX_CYCLES
    codes = np.zeros((max_tiles * n, U), dtype=np.uint8)
    given = np.zeros(max_tiles, dtype=bool)
    for entry in umi_tiles:
        ti, planes = entry[0], entry[1]
        assert len(planes) == U and not given[ti]
        given[ti] = True
        codes[ti * n:(ti + 1) * n] = codes_of(planes, n).T
    return codes, given


def umi_keys(umi_tiles, n, max_tiles):
    """the keys as the library packs them: uint64 [max_tiles * n], ten 3-bit codes per 32-bit word, the first word low"""
    codes, _ = umi_codes(umi_tiles, n, max_tiles)
    keys = np.zeros(codes.shape[0], dtype=np.uint64)
    for c in range(codes.shape[1]):
        keys |= codes[:, c].astype(np.uint64) << np.uint64(32 * (c // 10) + 3 * (c % 10))
    return keys


def molecules_of(codes, max_e):
    """codes uint8 [m, U]: the UMI reads of a family's wells, ids ascending -> a list of molecules, each the ascending
    list of its wells' positions: the connected components under d <= max_e, by a union over every pair"""
    m = codes.shape[0]
    root = list(range(m))

    def find(x):
        while root[x] != x:
            x = root[x]
        return x

    d = (codes[:, None, :] != codes[None, :, :]).sum(axis=2)
    for i in range(m):
        for j in np.flatnonzero(d[i, :i] <= max_e).tolist():
            a, b = find(i), find(j)
            if a != b:
                root[max(a, b)] = min(a, b)
    comp = {}
    for i in range(m):
        comp.setdefault(find(i), []).append(i)
    return list(comp.values())


def lane_umi(tiles, umi_tiles, n, max_tiles, labels, max_e, max_family):
    """tiles: [(tile_index, [L planes of n bytes], filter bytes)] (looked at for the tile indices alone), umi_tiles:
    [(tile_index, [U planes of n bytes])], labels uint32 [max_tiles, n] -> (lane row int64 [LANE_COLS], tile rows int64
    [max_tiles, TILE_COLS])."""
    assert 0 <= max_e <= MAX_E and 2 <= max_family <= MAX_FAMILY
    codes, given = umi_codes(umi_tiles, n, max_tiles)
    assert sorted(t[0] for t in tiles) == np.flatnonzero(given).tolist()
    lane = np.zeros(LANE_COLS, dtype=np.int64)
    trow = np.zeros((max_tiles, TILE_COLS), dtype=np.int64)
    for root, m in families_of(labels):
        if m.size > max_family:
            lane[LARGE] += 1
            lane[LARGE_WELLS] += m.size
            continue
        sub = codes[m]
        mols = molecules_of(sub, max_e)
        lane[FAMILIES] += 1
        lane[MOLECULES] += len(mols)
        lane[DISTINCT] += len({r.tobytes() for r in sub})
        if len(mols) >= 2:
            lane[SPLIT_FAMILIES] += 1
            lane[SPLIT_WELLS] += m.size
        lane[WITH_N] += int((sub == 4).any(axis=1).sum())
        lane[PER_FAMILY + bin_of(len(mols))] += 1
        for mol in mols:
            lane[SIZE + bin_of(len(mol))] += 1
            for j, pos in enumerate(mol):                               # (positions ascend with the ids: mol[0] is the first well)
                t = int(m[pos]) // n
                trow[t, 0] += 1
                trow[t, 1] += j > 0
                trow[t, 2] += len(mol) == 1
    lane[:TILE_COLS] = trow.sum(axis=0)
    return lane, trow


def check_umi_identities(lane, trow, max_e, U=None, finish_lane=None, lower_e=None, at_e0=None, subset_equality=False,
                         group_spans=None):
    """What the header promises of any result.  finish_lane: the lane row of the finish the labels came from (Classes
    and Redundant are columns 1 and 3: the groups of two or more wells and their wells beyond the first); lower_e: the
    result of the same lane and max_family at a smaller E; at_e0: at E = 0; subset_equality: equality labels and UMI
    cycles among the scanned ones; group_spans: GroupSpans of index_finish over the same cycles, for a result at E = 0
    with no large family."""
    lane, trow = np.asarray(lane), np.asarray(trow)
    assert lane.shape == (LANE_COLS,) and trow.shape[1] == TILE_COLS
    assert (lane >= 0).all() and (trow >= 0).all()
    per_family, size = lane[PER_FAMILY:SIZE], lane[SIZE:]
    if finish_lane is not None:
        assert lane[FAMILIES] + lane[LARGE] == finish_lane[1]                              # 1
        assert lane[WELLS] + lane[LARGE_WELLS] == finish_lane[1] + finish_lane[3]          # 2
    assert lane[FAMILIES] <= lane[MOLECULES] <= lane[DISTINCT] <= lane[WELLS]              # 3
    assert lane[REDUNDANT] == lane[WELLS] - lane[MOLECULES]                                # 4
    assert per_family.sum() == lane[FAMILIES]                                              # 5
    assert size.sum() == lane[MOLECULES]                                                   # 6
    assert size[0] == lane[LONE]                                                           # 7
    assert lane[SPLIT_FAMILIES] == lane[FAMILIES] - per_family[0]                          # 8
    assert (trow.sum(axis=0) == lane[:TILE_COLS]).all()                                    # 9
    assert (trow[:, 1] <= trow[:, 0]).all() and (trow[:, 2] <= trow[:, 0]).all()
    assert 2 * lane[SPLIT_FAMILIES] <= lane[SPLIT_WELLS] <= lane[WELLS] and lane[WITH_N] <= lane[WELLS]
    assert 2 * lane[FAMILIES] <= lane[WELLS] and lane[LARGE_WELLS] >= 3 * lane[LARGE]
    if lower_e is not None:                                                                # 10, 11
        ll = np.asarray(lower_e[0])
        assert ll[MOLECULES] >= lane[MOLECULES] and ll[SPLIT_FAMILIES] >= lane[SPLIT_FAMILIES]
        assert ll[DISTINCT] == lane[DISTINCT] and ll[WELLS] == lane[WELLS] and ll[FAMILIES] == lane[FAMILIES]
    if at_e0 is not None:
        assert np.asarray(at_e0[0])[MOLECULES] == lane[DISTINCT]
    if max_e == 0:                                                                         # 12
        assert lane[MOLECULES] == lane[DISTINCT]
    if U is not None and max_e >= U:                                                       # 13
        assert lane[MOLECULES] == lane[FAMILIES] and lane[LONE] == 0 and lane[SPLIT_FAMILIES] == 0
    if subset_equality:                                                                    # 14
        assert lane[MOLECULES] == lane[FAMILIES] and lane[LONE] == 0
    if group_spans is not None:                                                            # 15
        assert max_e == 0 and lane[LARGE] == 0 and lane[MOLECULES] == group_spans
