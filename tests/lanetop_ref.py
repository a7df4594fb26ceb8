"""Host reference for a lane's most frequent reads and their spread (include/welldup_lanetop.h): the definitions in
plain numpy, from the label arrays of lanedups_ref.lane_dups / lanenear_ref.lane_near_dups and the host reads."""
import numpy as np

from tiledups_ref import INVALID

MAX_TOP = 1024
LEVELS = 16
HEAD_COLS = 4
EDGES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 50, 100, 500, 1000, 5000, 10000)
MAX_PASSES = 8


def level_of(sizes):
    """the duplication level of each size >= 1"""
    return np.searchsorted(np.asarray(EDGES), np.asarray(sizes), side="right") - 1


def decode(read_bytes):
    """a read's BCL bytes -> its bases: 0 is a no-call, else the low two bits"""
    b = np.asarray(read_bytes)
    return "".join("N" if v == 0 else "ACGT"[v & 3] for v in b.tolist())


def lane_reads(tiles, n, max_tiles):
    """tiles: (tile index, planes, filter) as lanedups_ref takes them -> uint8 [max_tiles * n, L] by global id"""
    cycles = len(tiles[0][1])
    out = np.zeros((max_tiles * n, cycles), dtype=np.uint8)
    for idx, planes, _ in tiles:
        out[idx * n:(idx + 1) * n] = np.stack([np.asarray(p, dtype=np.uint8) for p in planes], axis=1)
    return out


def lane_top(labels, tiles, n, max_tiles, n_top):
    """-> (head int64 [4]: [PF, Groups2, Listed, Covered], levels int64 [2, 16], root uint32 [k], size uint32 [k],
    exact uint32 [k], tile_count uint32 [k, max_tiles], reads: list of k str), k = Listed"""
    assert 1 <= n_top <= MAX_TOP
    flat = np.asarray(labels).reshape(-1).astype(np.int64)
    assert flat.size == max_tiles * n
    pf = np.flatnonzero(flat != INVALID)
    sizes = np.bincount(flat[pf], minlength=flat.size)                  # at the roots; 1 at a PF well in no group
    roots = np.flatnonzero(sizes)
    assert (flat[roots] == roots).all()
    levels = np.zeros((2, LEVELS), dtype=np.int64)
    lev = level_of(sizes[roots])
    np.add.at(levels[0], lev, 1)
    np.add.at(levels[1], lev, sizes[roots])
    grouped = roots[sizes[roots] >= 2]
    order = grouped[np.lexsort((grouped, -sizes[grouped]))]             # size descending, then root ascending
    listed = order[:n_top]
    codes = lane_reads(tiles, n, max_tiles)
    codes = np.where(codes == 0, 4, codes & 3)                          # what the packed rows hold
    exact = np.zeros(listed.size, dtype=np.uint32)
    tile_count = np.zeros((listed.size, max_tiles), dtype=np.uint32)
    reads = []
    for r, root in enumerate(listed.tolist()):
        wells = pf[flat[pf] == root]
        exact[r] = int((codes[wells] == codes[root]).all(axis=1).sum())
        tile_count[r] = np.bincount(wells // n, minlength=max_tiles)
        reads.append("".join("ACGTN"[c] for c in codes[root].tolist()))
    head = np.array([pf.size, grouped.size, listed.size, int(sizes[listed].sum())], dtype=np.int64)
    return head, levels, listed.astype(np.uint32), sizes[listed].astype(np.uint32), exact, tile_count, reads


def check_top_identities(head, levels, root, size, exact, tile_count, reads, n, n_top, finish_lane=None, equality=False,
                         longer=None, cycles=None):
    """the identities include/welldup_lanetop.h states; finish_lane: the lane row of the finish that ran last ([PF,
    Classes, InClasses, Redundant, CrossTile, Spans, bins 2 .. 8, >= 9]); longer: the result for a larger n_top"""
    groups, wells = levels
    pf, groups2, listed, covered = (int(v) for v in head)
    assert wells.sum() == pf and groups[0] == wells[0] and groups[1:].sum() == groups2
    assert (wells[:9] == np.arange(1, 10) * groups[:9]).all()
    for i in range(9, LEVELS):                                          # a level's wells lie between its edges
        hi = EDGES[i + 1] - 1 if i + 1 < LEVELS else pf
        assert EDGES[i] * groups[i] <= wells[i] <= hi * groups[i]
    assert listed == min(n_top, groups2) == len(root) == len(size) == len(exact) == len(tile_count) == len(reads)
    assert covered == int(size.astype(np.int64).sum())
    if finish_lane is not None:
        assert pf == finish_lane[0] and groups2 == finish_lane[1] and wells[1:].sum() == finish_lane[2]
        assert groups[0] == pf - finish_lane[2]
        assert (groups[1:8] == finish_lane[6:13]).all() and groups[8:].sum() == finish_lane[13]
    key = list(zip((-size.astype(np.int64)).tolist(), root.tolist()))
    assert key == sorted(key) and len(set(root.tolist())) == listed    # the order, and it is total
    if listed:
        assert size.min() >= 2 and (tile_count.astype(np.int64).sum(axis=1) == size).all()
        assert (exact >= 1).all() and (exact <= size).all()
        assert (tile_count[np.arange(listed), root // n] >= 1).all()
        if equality:
            assert (exact == size).all()
        if cycles is not None:
            assert all(len(r) == cycles and set(r) <= set("ACGTN") for r in reads)
    if longer is not None:                                              # the list for a is the head of the list for b > a
        assert (longer[0][:2] == head[:2]).all() and (longer[1] == levels).all()
        for a, b in zip((root, size, exact, tile_count), longer[2:6]):
            assert (b[:listed] == a).all()
        assert longer[6][:listed] == reads
