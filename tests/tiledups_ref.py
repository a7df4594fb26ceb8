"""Host reference of the read classes of a tile (include/welldup_tiledups.h) in numpy: the reads decoded to
codes, the PF wells grouped by their rows (pre-grouped by a host hash, every group confirmed by comparing the
rows themselves), labels, size bins, Local by the symmetric ring rule from lvl_off / nbr, RingWells.
Test plumbing only: what wd_tile_dups computes on the GPU is compared against this."""
from __future__ import annotations

import numpy as np

INVALID = 0xFFFFFFFF
SIZE_BINS = 8            # sizes 2..8, >= 9


def codes_of(planes, n):
    """[L planes of n bytes] -> uint8 [L, n] (a plane per cycle, as the input): 4 for byte 0 (N), else
    byte & 3 (bcl_direct_reader.py:352-361)."""
    out = np.zeros((len(planes), n), dtype=np.uint8)
    for c, p in enumerate(planes):
        p = np.asarray(p, dtype=np.uint8)[:n]
        out[c] = np.where(p == 0, 4, p & 3)
    return out


def class_labels(codes, pf):
    """labels uint32 [n]: the smallest well index of the well's class, its own index for a PF well in no
    class, INVALID for a non-PF well."""
    L, n = codes.shape
    pf = np.asarray(pf).astype(bool)
    labels = np.full(n, INVALID, dtype=np.uint32)
    wells = np.flatnonzero(pf)
    if wells.size == 0:
        return labels
    labels[wells] = wells
    # a host hash first (a polynomial over the codes, nothing the device uses) ...
    h = np.zeros(wells.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for c in range(L):
            h = h * np.uint64(1099511628211) + codes[c][wells].astype(np.uint64) + np.uint64(7)
    order = np.argsort(h, kind="stable")                  # (stable: wells of a hash stay in index order)
    hs = h[order]
    starts = np.flatnonzero(np.concatenate([[True], hs[1:] != hs[:-1]]))
    ends = np.concatenate([starts[1:], [hs.size]])
    for s, e in zip(starts.tolist(), ends.tolist()):
        if e - s < 2:
            continue
        # ... then every group of one hash is split by the rows themselves
        group = wells[order[s:e]]
        rows = np.ascontiguousarray(codes[:, group].T)
        _, inverse = np.unique(rows, axis=0, return_inverse=True)
        inverse = np.asarray(inverse).reshape(-1)
        for g in np.unique(inverse).tolist():
            members = group[inverse == g]
            assert (codes[:, members] == codes[:, members[:1]]).all()
            labels[members] = members.min()
    return labels


def tile_dups(planes, filt, lvl_off, nbr):
    """-> (row [PF, Classes, InClasses, Redundant, Local[levels], RingWells[levels], 8 size bins] int64,
    labels uint32 [n]).  Target t is well t: lvl_off [n, levels + 1], nbr [P]."""
    filt = np.asarray(filt, dtype=np.uint8)
    n = filt.shape[0]
    lvl_off = np.asarray(lvl_off, dtype=np.int64)
    nbr = np.asarray(nbr, dtype=np.int64)
    assert lvl_off.shape[0] == n
    levels = lvl_off.shape[1] - 1
    pf = (filt & 1).astype(bool)
    labels = class_labels(codes_of(planes, n), pf)
    size = np.bincount(labels[pf].astype(np.int64), minlength=n)
    in_class = np.zeros(n, dtype=bool)
    in_class[pf] = size[labels[pf].astype(np.int64)] >= 2
    reps = np.flatnonzero(size >= 2)
    classes, in_classes = int(reps.size), int(in_class.sum())
    bins = np.bincount(np.minimum(size[reps], SIZE_BINS + 1) - 2, minlength=SIZE_BINS)[:SIZE_BINS]
    # the first level at which a well meets a classmate, from either end of the pair
    first = np.full(n, levels, dtype=np.int64)
    ring_wells = np.zeros(levels, dtype=np.int64)
    for w in np.flatnonzero(in_class).tolist():
        o = lvl_off[w]
        for l in range(levels):
            ring_wells[l] += o[l + 1] - o[0]
            m = nbr[o[l]:o[l + 1]]
            m = m[(m != w) & (labels[m] == labels[w])]
            if m.size:
                first[w] = min(first[w], l)
                np.minimum.at(first, m, l)
    local = np.array([(first <= l).sum() for l in range(levels)], dtype=np.int64)
    row = np.concatenate([[int(pf.sum()), classes, in_classes, in_classes - classes], local, ring_wells,
                          bins]).astype(np.int64)
    return row, labels
