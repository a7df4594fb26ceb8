"""A small lane for the adapter pass (tests/test_gpu_laneadapter.py, tests/test_laneadapter_host.py): the N, MAX_TILES
and INDEX of tests/test_gpu_lanemismatch.py, random reads, one tile without a PF well, and a scripted part whose wells
carry the plants tools/lane_adapter_emu.cpp lists - for each of the three (m, E, O) of PARAMS, whose adapters are
prefixes of one another: the adapter at every p in 0 .. L - O, 0, 1, E and E + 1 substitutions that include its first
base, its last (of those that fit) and a middle one, an N inside the match, overlaps of O - 1, O, m - 1 and m at the
read's end with allowed(p) and allowed(p) + 1 mismatches, two matches in one read, and for every adapter base j the
plant that puts it on cycle 9, 10, 19, 20, 63 and 64 with that base substituted alone and with E more.  Every third
plant is copied once to three times onto other tiles (families among the plants, singles besides), and copies of reads
that end in the adapter carry one substitution inside it: one mismatch from their root, so its cluster under K = 2, with
another a.  check_coverage asserts from the reference that the lane holds what the tests are to see."""
from __future__ import annotations

import numpy as np

from laneadapter_ref import COPY, allowed, codes_of, first_match_literal, wells_of

ROWS, COLS = 44, 60
N = ROWS * COLS                                    # test_gpu_lanemismatch.py's
INDEX = [5, 0, 3, 6, 1]                            # slot -> tile index in a lane of MAX_TILES
MAX_TILES = 7
DEAD = 1                                           # the slot without a PF well
ADAPTER = codes_of("AGATCGGAAGAGCACACGTCTGAACTCCAGTC")      # TruSeq's 13 bases and the 19 that follow them in the read
PARAMS = [(13, 1, 8), (8, 0, 3), (32, 3, 32)]      # (m, E, O); the adapter of each is ADAPTER[:m]
EDGES = (9, 10, 19, 20, 63, 64)


def bytes_of(codes, rng):
    """plane bytes of codes: N is byte 0, a base its code under a quality that is not 0"""
    codes = np.asarray(codes, dtype=np.uint8)
    q = rng.integers(1, 64, codes.shape).astype(np.uint8)
    return np.where(codes == 4, 0, codes | (q << 2)).astype(np.uint8)


def _plant(read, codes, p, subs=(), n_at=None, rng=None):
    for j in range(len(codes)):
        if p + j >= len(read):
            break
        read[p + j] = 4 if j == n_at else (int(codes[j]) + 1 + int(rng.integers(3))) % 4 if j in subs else codes[j]


def _subs_with(over, must, count):
    """`count` bases of 0 .. over - 1 that include `must`"""
    return {(must + i) % over for i in range(min(count, over))}


def scripted(L, rng, params=PARAMS):
    """-> [(read codes uint8 [L], what)]: the plants of every (m, E, O) of params.  An exact plant at p is kept free
    of a match before p under every one of params (an N goes into any that a random background brings)."""
    out = []

    def clean(read, p):
        for m, e, o in params:
            if p > L - o:
                continue
            while True:
                a, _ = first_match_literal(read, ADAPTER[:m], e, o)
                if a >= p:
                    break
                j = next(j for j in range(a, p) if read[j] != 4)
                read[j] = 4

    for m, e, o in params:
        codes = ADAPTER[:m]

        def add(p, what, subs=(), n_at=None, full=False):
            if not 0 <= p < L:
                return
            read = rng.integers(0, 4, L).astype(np.uint8)
            _plant(read, ADAPTER if full else codes, p, subs, n_at, rng)
            if full:
                clean(read, p)
            out.append((read, what))

        if (m, e, o) == params[0]:
            for p in range(L - MIN_O + 1):
                add(p, "exact", full=True)
        for p in (0, (L - m) // 2, L - m, L - (m + o) // 2):
            if p < 0 or p + o > L:
                continue
            over = min(m, L - p)
            for must in (0, over - 1, over // 2):
                for count in (0, 1, e, e + 1):
                    add(p, "subs", _subs_with(over, must, count))
            add(p, "n", n_at=over // 2)
            add(p, "n", _subs_with(over, 0, e), n_at=over - 1)
        for over in (o - 1, o, m - 1, m):
            if not 1 <= over <= L:
                continue
            p = L - over
            ok = e if over == m else e * over // m
            for count in (ok, ok + 1, 0):
                for must in (0, over - 1):
                    if count <= over:
                        add(p, "end", _subs_with(over, must, count))
        if L >= 2 * m + 4:
            read = rng.integers(0, 4, L).astype(np.uint8)
            _plant(read, codes, 1, rng=rng)
            _plant(read, codes, m + 3, rng=rng)
            out.append((read, "two"))
            read = read.copy()
            _plant(read, codes, 1, _subs_with(m, 1, e + 1), rng=rng)
            out.append((read, "two"))
        for edge in EDGES:
            for j in range(m):
                p = edge - j
                if p < 0 or p + o > L or edge >= L:
                    continue
                over = min(m, L - p)
                add(p, "edge", {j})
                add(p, "edge", {(j + i) % over for i in range(e + 1)})
    return out


MIN_O = min(o for _, _, o in PARAMS)


def small_lane(cycles, seed=23):
    """-> (reads: per slot uint8 [N, cycles] plane bytes, filts: per slot uint8 [N])"""
    rng = np.random.default_rng(seed + cycles)
    L = cycles
    codes = [rng.integers(0, 4, (N, L)).astype(np.uint8) for _ in INDEX]
    for c in codes:
        c[rng.random(c.shape) < 0.004] = 4
    filts = [(rng.random(N) < 0.9).astype(np.uint8) for _ in INDEX]
    filts[DEAD][:] = 0
    live = [s for s in range(len(INDEX)) if s != DEAD]
    free = {s: list(rng.permutation(N)) for s in live}

    def place(slot, read):
        w = free[slot].pop()
        codes[slot][w] = read
        filts[slot][w] = 1
        return w

    for i, (read, what) in enumerate(scripted(L, rng)):
        slot = live[i % len(live)]
        place(slot, read)
        if i % 3 == 0:                                                 # a family: equal reads on the other tiles
            for j in range(1 + i // 3 % 3):
                place(live[(i + 1 + j) % len(live)], read)
    # reads that end in the adapter, each with a copy one substitution inside the adapter away: over allowed(p)
    for m, e, o in PARAMS:
        for i in range(40):
            over = o + i % max(1, min(m, L) - o)                       # overlaps of O .. below m, where allowed(p) is smallest
            p = L - over
            read = rng.integers(0, 4, L).astype(np.uint8)
            _plant(read, ADAPTER[:m], p, rng=rng)
            ok = allowed(L, m, e, o, p)
            other = read.copy()
            for j in range(ok + 1):
                other[p + j] = (other[p + j] + 1 + j) % 4
            if ok + 1 <= 2:                                            # (within K = 2 of the root)
                place(live[i % len(live)], read)
                place(live[(i + 1) % len(live)], other)
    return [bytes_of(c, rng) for c in codes], filts


def check_coverage(tiles, labels, k, cycles):
    """The ground the lane covers, from the reference: every a in 0 .. L - O is hit; every population is present with
    and without adapter; Inexact and Partial occur where E and O let them; under K = 2 at least 20 copies' a is not
    their root's."""
    for m, e, o in PARAMS:
        ids, a, mism, pop, size, L = wells_of(tiles, N, MAX_TILES, labels, ADAPTER[:m], e, o)
        assert L == cycles and set(range(L - o + 1)) <= set(a.tolist()), (m, e, o, sorted(set(range(L - o + 1)) - set(a.tolist())))
        for p in range(3):
            assert ((pop == p) & (a < L)).sum() >= 10 and ((pop == p) & (a == L)).sum() >= 10, (m, e, o, p)
        assert (e == 0 or ((a < L) & (mism > 0)).sum() >= 10) and (o == m or ((a < L) & (L - a < m)).sum() >= 10)
        if k == 2:
            flat = np.asarray(labels).reshape(-1).astype(np.int64)
            at = np.full(flat.size, -1, dtype=np.int64)
            at[ids] = np.arange(ids.size)
            copies = np.flatnonzero(pop == COPY)
            other = int((a[copies] != a[at[flat[ids[copies]]]]).sum())
            assert other >= 20 or (m, e, o) != PARAMS[0], (m, e, o, other)
