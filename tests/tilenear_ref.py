"""Host reference of the near-duplicate read clusters of a tile (include/welldup_tilenear.h) in numpy.  Two
independent ways to the edges between distinct reads, neither of them the segment scheme of the device:
  (a) `edges_all_pairs`: every pair, in blocks, the distance counted as L minus the matching cycles (one
      matrix product per letter) - tiles of a few thousand distinct reads, any K;
  (b) `edges_by_deletion`: the deletion neighbourhood - for every choice of K cycles a polynomial hash of the
      read without the terms of those cycles, sorted; every run of equal keys confirmed on the rows with those
      cycles masked - large tiles, K = 1 (L sorts) or K = 2 (L (L - 1) / 2 sorts).
Clusters by a sequential union-find on the host; the rest of the row as tests/tiledups_ref.py.
Test plumbing only: what wd_tile_near_dups computes on the GPU is compared against this."""
from __future__ import annotations

import itertools

import numpy as np

from tiledups_ref import INVALID, SIZE_BINS, class_labels, codes_of


def distinct_reads(codes, pf):
    """-> (class labels uint32 [n], reps int64 [r]): one well per distinct read of the PF wells (the smallest)."""
    labels = class_labels(codes, pf)
    n = labels.shape[0]
    reps = np.flatnonzero(labels == np.arange(n, dtype=np.uint32))
    return labels, reps


def edges_all_pairs(codes, reps, k, block=1024):
    """Pairs (i < j, indices into reps) of distinct reads at Hamming distance <= k, as an int64 [e, 2] array."""
    L = codes.shape[0]
    rows = codes[:, reps].T                                           # [r, L]
    onehot = [(rows == v).astype(np.float32) for v in range(5)]
    out = []
    for b0 in range(0, rows.shape[0], block):
        match = np.zeros((min(block, rows.shape[0] - b0), rows.shape[0]), dtype=np.float32)
        for h in onehot:
            match += h[b0:b0 + block] @ h.T
        i, j = np.nonzero(L - match <= k + 0.5)
        keep = i + b0 < j
        out.append(np.stack([i[keep] + b0, j[keep]], axis=1))
    e = np.concatenate(out) if out else np.zeros((0, 2), dtype=np.int64)
    # (the distances once more, in integers, on the pairs found)
    d = (rows[e[:, 0]] != rows[e[:, 1]]).sum(axis=1)
    assert ((d >= 1) & (d <= k)).all()
    return e.astype(np.int64)


def edges_by_deletion(codes, reps, k):
    """The same edges from the deletion neighbourhood (k = 1 or 2)."""
    assert k in (1, 2)
    L = codes.shape[0]
    rows = codes[:, reps]                                             # [L, r]
    r = rows.shape[1]
    base = np.uint64(1099511628211)
    power = np.ones(L, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for c in range(1, L):
            power[c] = power[c - 1] * base
        term = lambda p: (rows[p].astype(np.uint64) + np.uint64(1)) * power[p]
        whole = np.zeros(r, dtype=np.uint64)
        for c in range(L):
            whole += term(c)
    found = []
    for cut in itertools.combinations(range(L), k):
        with np.errstate(over="ignore"):
            key = whole.copy()
            for p in cut:
                key -= term(p)
        order = np.argsort(key, kind="stable")
        ks = key[order]
        starts = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
        ends = np.concatenate([starts[1:], [r]])
        size = ends - starts
        keep = np.ones(L, dtype=bool)
        keep[list(cut)] = False
        two = starts[size == 2]
        if two.size:                                                  # runs of two: confirmed in one go
            a, b = order[two], order[two + 1]
            same = (rows[:, a] == rows[:, b])[keep].all(axis=0)
            a, b = a[same], b[same]
            found.append(np.stack([np.minimum(a, b), np.maximum(a, b)], axis=1))
        for s, e in zip(starts[size > 2].tolist(), ends[size > 2].tolist()):
            group = order[s:e]
            _, inverse = np.unique(np.ascontiguousarray(rows[:, group][keep].T), axis=0, return_inverse=True)
            inverse = np.asarray(inverse).reshape(-1)
            for g in np.unique(inverse).tolist():
                m = np.sort(group[inverse == g])
                if m.size >= 2:
                    found.append(np.array(list(itertools.combinations(m.tolist(), 2)), dtype=np.int64))
    if not found:
        return np.zeros((0, 2), dtype=np.int64)
    e = np.concatenate(found).astype(np.int64)
    packed = np.unique(e[:, 0] * r + e[:, 1])                         # (a pair turns up once per cut that hides its mismatches)
    return np.stack([packed // r, packed % r], axis=1)


def cluster_labels(class_lab, reps, edges):
    """Single linkage over the edges between distinct reads -> labels uint32 [n]: the smallest well of the
    cluster, the well's own index in none, INVALID for a non-PF well."""
    parent = list(range(reps.shape[0]))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    for a, b in edges.tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)                         # reps ascend: the smaller index is the smaller well
    root_well = reps.copy()
    for i in np.unique(edges).tolist():                               # (a read with no edge is its own root)
        root_well[i] = reps[find(i)]
    n = class_lab.shape[0]
    of_rep = np.zeros(n, dtype=np.int64)
    of_rep[reps] = root_well
    labels = np.full(n, INVALID, dtype=np.uint32)
    pf = class_lab != INVALID
    labels[pf] = of_rep[class_lab[pf].astype(np.int64)]
    return labels


def row_of(labels, near_pairs, lvl_off, nbr):
    """[PF, Clusters, InClusters, Redundant, NearPairs, Local[levels], RingWells[levels], 8 size bins] int64 from
    cluster labels: sizes, and Local by the symmetric ring rule (target t is well t)."""
    n = labels.shape[0]
    lvl_off = np.asarray(lvl_off, dtype=np.int64)
    nbr = np.asarray(nbr, dtype=np.int64)
    assert lvl_off.shape[0] == n
    levels = lvl_off.shape[1] - 1
    pf = labels != INVALID
    size = np.bincount(labels[pf].astype(np.int64), minlength=n)
    inside = np.zeros(n, dtype=bool)
    inside[pf] = size[labels[pf].astype(np.int64)] >= 2
    roots = np.flatnonzero(size >= 2)
    bins = np.bincount(np.minimum(size[roots], SIZE_BINS + 1) - 2, minlength=SIZE_BINS)[:SIZE_BINS]
    first = np.full(n, levels, dtype=np.int64)
    ring_wells = np.zeros(levels, dtype=np.int64)
    for w in np.flatnonzero(inside).tolist():
        o = lvl_off[w]
        for l in range(levels):
            ring_wells[l] += o[l + 1] - o[0]
            m = nbr[o[l]:o[l + 1]]
            m = m[(m != w) & (labels[m] == labels[w])]
            if m.size:
                first[w] = min(first[w], l)
                np.minimum.at(first, m, l)
    local = np.array([(first <= l).sum() for l in range(levels)], dtype=np.int64)
    n_in = int(inside.sum())
    return np.concatenate([[int(pf.sum()), roots.size, n_in, n_in - roots.size, int(near_pairs)], local, ring_wells,
                           bins]).astype(np.int64)


def tile_near_dups(planes, filt, lvl_off, nbr, k, method="all_pairs"):
    """-> (row, labels uint32 [n]) of one tile at Hamming distance <= k."""
    filt = np.asarray(filt, dtype=np.uint8)
    n = filt.shape[0]
    codes = codes_of(planes, n)
    class_lab, reps = distinct_reads(codes, (filt & 1).astype(bool))
    if k == 0 or reps.size < 2:
        edges = np.zeros((0, 2), dtype=np.int64)
    elif method == "all_pairs":
        edges = edges_all_pairs(codes, reps, k)
    else:
        edges = edges_by_deletion(codes, reps, k)
    labels = cluster_labels(class_lab, reps, edges)
    return row_of(labels, edges.shape[0], lvl_off, nbr), labels


# ---- a hand-made tile and its hand-worked answer (host and GPU tests) ---------------------------
A, C, G, T = 0x40, 0x81, 0xC2, 0x23          # quality bits on top of the base's two low bits
BASE = {"A": A, "C": C, "G": G, "T": T, "N": 0}


def grid_rings(rows, cols):
    """Level 1: the wells left, right, above and below; level 2: the diagonal ones."""
    lvl_off, nbr = [], []
    for r in range(rows):
        for c in range(cols):
            row = [len(nbr)]
            for ring in ([(0, -1), (0, 1), (-1, 0), (1, 0)], [(-1, -1), (-1, 1), (1, -1), (1, 1)]):
                for dr, dc in ring:
                    if 0 <= r + dr < rows and 0 <= c + dc < cols:
                        nbr.append((r + dr) * cols + c + dc)
                row.append(len(nbr))
            lvl_off.append(row)
    return np.array(lvl_off), np.array(nbr)


def hand_made_tile():
    """4 x 6 wells, six cycles:
          0  1  2  3  4  5       chain   0 AAAAAA ~ 1 CAAAAA ~ 7 CCAAAA (0 and 7 differ in two cycles)
          6  7  8  9 10 11       N       5 NAGGTT ~ 23 NAGGTC (N == N); 11 AAGGTA is two cycles from both
         12 13 14 15 16 17               (N against A counts), so it joins them at K = 2 only
         18 19 20 21 22 23       bridge  12 GGGGGG ~ 13 GGGGGT and 16 GGGTTT ~ 17 GGTTTT; 15 GGGGTT is one cycle
    from 13 and from 16 but fails the filter (byte 2): two clusters at K = 1; at K = 2 well 13 reaches 16 itself
    quality  14 and 19 read TGTGTG with different quality bits: a class, diagonal neighbours (level 2)
    class    3, 9, 21 read ACGTAC (3 above 9; 21 far off); 6 ACGTAA, far from all three, is one cycle away
    the other wells read something at least three cycles from everything else."""
    reads = {0: "AAAAAA", 1: "CAAAAA", 7: "CCAAAA", 5: "NAGGTT", 23: "NAGGTC", 11: "AAGGTA",
             12: "GGGGGG", 13: "GGGGGT", 15: "GGGGTT", 16: "GGGTTT", 17: "GGTTTT",
             14: "TGTGTG", 19: "TGTGTG", 3: "ACGTAC", 9: "ACGTAC", 21: "ACGTAC", 6: "ACGTAA",
             2: "CGCGCG", 4: "GCGCGC", 8: "TATATA", 10: "ATCTAT", 18: "CTAGCT", 20: "CATTCA", 22: "GAGAGA"}
    planes = [np.array([BASE[reads[w][c]] for w in range(24)], dtype=np.uint8) for c in range(6)]
    for c in range(6):
        planes[c][19] |= 0x3C if c % 2 else 0x10                       # (the same bases: the low two bits stay)
        planes[c][9] ^= 0x04
    filt = np.ones(24, dtype=np.uint8)
    filt[15] = 2                                                       # only bit 0 counts
    filt[3] = 0x81
    return planes, filt, grid_rings(4, 6)


HAND = {
    1: dict(labels=[0, 0, 2, 3, 4, 5, 3, 0, 8, 3, 10, 11, 12, 12, 14, INVALID, 16, 16, 18, 14, 20, 3, 22, 5],
            head=[23, 6, 15, 9, 6], local=[9, 11], ring_wells=[47, 84], bins=[4, 1, 1, 0, 0, 0, 0, 0]),
    2: dict(labels=[0, 0, 2, 3, 4, 5, 3, 0, 8, 3, 10, 5, 12, 12, 14, INVALID, 12, 12, 18, 14, 20, 3, 22, 5],
            head=[23, 5, 16, 11, 10], local=[11, 13], ring_wells=[50, 89], bins=[1, 2, 2, 0, 0, 0, 0, 0]),
}


# ---- reads at the boundary between the chain walk and the rank path (GPU tests of both near passes) ----
LONG_GROUPS = (31, 32, 33, 34)      # a slot of up to 32 distinct reads is walked as a chain, a larger one goes by ranks


def long_boundary_reads(seed=23, n=256, cycles=20):
    """-> (reads uint8 [n, cycles], groups: the wells of each), for K = 1 (segments: cycles 0..9 and 10..19).
    Four groups of 31, 32, 33 and 34 distinct reads at random wells; a group shares its own cycles 0..9 - one slot
    of segment 0 - and is random in cycles 10..19 but for five planted pairs, which differ in exactly one cycle
    of 10..19.  The other wells are random; no two reads of the tile are equal.
    What the tests built on this cannot see: which path a group went down on the GPU.  A random well whose segment
    fingerprint falls into a group's slot makes 32 vertices 33, and a chain's order is the order of arrival, so the
    planted pairs lie at arbitrary steps of a walk: a bound one step short would be caught only by chance."""
    rng = np.random.default_rng(seed)
    half = cycles // 2
    reads = (0x40 | rng.integers(0, 4, (n, cycles))).astype(np.uint8)
    wells = rng.permutation(n)
    groups, at = [], 0
    for size in LONG_GROUPS:
        g = wells[at:at + size]
        at += size
        reads[g, :half] = reads[g[0], :half]
        for a, b in ((0, 1), (2, 3), (4, 5), (size - 4, size - 3), (size - 2, size - 1)):
            reads[g[b], half:] = reads[g[a], half:]
            reads[g[b], half + a % half] ^= 1                          # another base, the same quality bits
        groups.append(g)
    assert np.unique(reads, axis=0).shape[0] == n
    return reads, groups


def long_boundary_check(labels, groups):
    """labels [n]: the reference's cluster label of every read above.  Every group holds a near pair and no near
    pair joins two groups, so each of the four slots is decided on its own path."""
    owner = {}
    for i, g in enumerate(groups):
        labs, count = np.unique(labels[g], return_counts=True)
        assert (count >= 2).any(), i
        for lab in labs.tolist():
            assert owner.setdefault(lab, i) == i, (lab, i)
