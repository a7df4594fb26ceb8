"""Host reference of the duplicate sets (include/welldup_sets.h): a plain sequential union-find over
explicit edges, and the edges themselves from the reads (through the oracle's distances) or from the
scan's hit log.  Test plumbing only: what wd_dup_sets computes on the GPU is compared against this."""
from __future__ import annotations

import numpy as np

INVALID = 0xFFFFFFFF
SIZE_BINS = 8            # sizes 2..8, >= 9


def levels_of_slots(lvl_off, targets, slots):
    """Ring (0-based) of each neighbour slot in its target's row of lvl_off."""
    lvl_off = np.asarray(lvl_off)
    levels = lvl_off.shape[1] - 1
    rows = lvl_off[np.asarray(targets, dtype=np.int64)]
    slots = np.asarray(slots, dtype=np.int64)
    lev = np.zeros(slots.shape[0], dtype=np.int64)
    for l in range(1, levels):
        lev += slots >= rows[:, l]
    return lev


def dup_sets(n, pf, a, b, lev, levels):
    """Single-linkage sets of the PF wells over edges (a[i], b[i]) of level lev[i]; an edge with an end that
    fails the filter, or from a well to itself, is dropped.  -> (row [PF, Sets[levels], InSets[levels], Redundant[levels], 8 size bins],
    labels uint32[n]: smallest well of the outermost-level set, own index in no set, INVALID if not PF)."""
    pf = np.asarray(pf).astype(bool)
    a = np.asarray(a, dtype=np.int64)
    b = np.asarray(b, dtype=np.int64)
    lev = np.asarray(lev, dtype=np.int64)
    keep = pf[a] & pf[b] & (a != b)               # (a well that names itself is no pair: a set has two wells)
    a, b, lev = a[keep], b[keep], lev[keep]
    parent = list(range(n))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    merges = [0] * levels
    order = np.argsort(lev, kind="stable")
    for i in order.tolist():
        ra, rb = find(int(a[i])), find(int(b[i]))
        if ra != rb:
            if ra < rb:
                ra, rb = rb, ra
            parent[ra] = rb                       # the smaller index stays the root
            merges[int(lev[i])] += 1
    par = np.array(parent, dtype=np.int64)
    while True:                                   # pointer jumping to the roots
        nxt = par[par]
        if (nxt == par).all():
            break
        par = nxt
    first = np.full(n, levels, dtype=np.int64)
    np.minimum.at(first, a, lev)
    np.minimum.at(first, b, lev)
    in_sets = np.array([(first <= l).sum() for l in range(levels)], dtype=np.int64)
    redundant = np.cumsum(np.array(merges, dtype=np.int64))
    size = np.bincount(par[pf], minlength=n)
    roots = np.flatnonzero((size >= 2) & (par == np.arange(n)))
    bins = np.bincount(np.minimum(size[roots], SIZE_BINS + 1) - 2, minlength=SIZE_BINS)[:SIZE_BINS]
    row = np.concatenate([[int(pf.sum())], in_sets - redundant, in_sets, redundant, bins]).astype(np.int64)
    labels = np.where(pf, par, INVALID).astype(np.uint32)
    return row, labels


def read_strings(planes, n):
    """[L planes of n bytes] -> n strings as the reference decodes them (0 -> N, else ACGT[b & 3])."""
    rows = np.stack([np.asarray(p, dtype=np.uint8)[:n] for p in planes], axis=1)
    lut = np.frombuffer(b"NACGT", dtype="S1")
    codes = lut[np.where(rows == 0, 0, (rows & 3) + 1)]
    return [r.tobytes().decode() for r in codes]


def edges_from_reads(seqs, pf, lvl_off, nbr, mode, k, dist_fn):
    """Every (a, b, level) with b in ring `level` of a, both PF and dist(a, b) <= k (mode 0: equal reads).
    Targets are the wells themselves (target t is well t).  dist_fn(x, y): the metric of modes 1 and 2."""
    levels = lvl_off.shape[1] - 1
    memo = {}
    ea, eb, el = [], [], []
    for t in range(lvl_off.shape[0]):
        if not pf[t]:
            continue
        for l in range(levels):
            for s in range(int(lvl_off[t, l]), int(lvl_off[t, l + 1])):
                w = int(nbr[s])
                if not pf[w]:
                    continue
                key = (min(t, w), max(t, w))
                d = memo.get(key)
                if d is None:
                    d = (0 if seqs[t] == seqs[w] else k + 1) if mode == 0 else dist_fn(seqs[t], seqs[w])
                    memo[key] = d
                if d <= k:
                    ea.append(t)
                    eb.append(w)
                    el.append(l)
    return np.array(ea, dtype=np.int64), np.array(eb, dtype=np.int64), np.array(el, dtype=np.int64)


def edges_from_hits(hits, lvl_off, nbr):
    """Hit records {tile, target, slot, dist} of one tile -> (a, b, level)."""
    t = hits["target"].astype(np.int64)
    s = hits["slot"].astype(np.int64)
    return t, np.asarray(nbr)[s].astype(np.int64), levels_of_slots(lvl_off, t, s)
