"""Scripted indel pairs for the dense Levenshtein <= 2 chain (numpy only, seeded).

A 12 x 200 honeycomb, every well a centre, 3 levels (2 400 wells, symmetric rings, most 64-target groups window
groups - test_dense_tiles_per_wave's targets).  For a read length L, `generate(L)` gives three tiles of planes and
filters and the list of scripted pairs: a well w and one well v of w's own rings, alternately below and above w,
where v's read is a script of w's read.  The first mismatch p and the last mismatch t of every script run over all
p < t of the boundary set B(L): the 8 + 2 split of sig_codes, the end of the signature word (9 | 10), of the screen
word (15 | 16), the row's chunks (10 + 8c) and groups (10 + 32k), the ballot words of lev2_gather (63 | 64,
127 | 128), the read's last chunk and last cycle.

Kinds (read a at w, read b at v):
  up, down                    b[i] = a[i+1] on [p, t), b[t] drawn / b[i] = a[i-1] on (p, t], b[p] drawn
  up+out, down+out            ... plus one substitution outside [p, t]: at 0, p - 1, t + 1 or L - 1     (intended 3)
  up+in, down+in              ... plus one substitution strictly inside                                 (intended 3)
  up-nocall                   up over a no-call inside a's stretch                                      (still 2)
  up-nocall-A                 ... and that no-call an A in b only: equal to the screen, N != A exactly  (intended 3)
  two-stretches               [p, m] and [m + 2, t] shifted separately: 4 that looks like 2 locally
  subs2, subs3                substitutions at p, t (and one cycle between)
  up-two-letters, down-...    the stretch drawn from two letters: fewer cycles mismatch in place than the shift spans
  tail                        (L > 16) substitutions at cycles >= 16 only: equal reads to the screen
  late-third                  (L > 16) within 2 on the first 16 cycles, a third error behind them
"up or down" kinds alternate their direction from one (p, t) to the next.  The intended distance is a label; what
a pair's distance is, the oracle decides (tests/test_lev2_scripts_host.py).

Background: random reads over five symbols with 2 % no-calls; 3 % of the wells fail the filter, never a scripted
one.  On tile 2 a third of the wells share their first 16 cycles (a scripted w among them keeps them where its
script allows), so the screen passes non-duplicates in bulk.
Reads are redrawn under the seed until no pair of neighbours outside the scripts (and outside tile 2's shared
prefix) is within distance 2, by the closed form restated here on symbol arrays (`closed_form`)."""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from well_duplicates_amd import cluster_indexes, synth, workload

ROWS, COLS, LEVELS = 12, 200, 3
N_TILES = 3
LENGTHS = (9, 10, 11, 16, 17, 43, 75, 129, 160)
SCREEN = 16
GATHER_TILES = (0, 1)                        # without tile 2's shared prefix: no survivor queue of theirs overflows
QUEUE_MAX = 64                               # the largest survivor queue per 64 targets ("dense_queue_cap")
N_SYM = 4                                    # symbols 0..3 = A, C, G, T; 4 = N (a no-call)


def boundary_set(L):
    cand = (0, 1, 7, 8, 9, 10, 11, 15, 16, 17, 18, 41, 42, 63, 64, 73, 74, 127, 128, L - 9, L - 8, L - 2, L - 1)
    return sorted({v for v in cand if 0 <= v < L})


@lru_cache(maxsize=None)
def targets():
    n = ROWS * COLS
    x, y = synth.honeycomb_pixels(ROWS, COLS)
    return workload.targets_to_csr(cluster_indexes.generate(x, y, range(n), LEVELS))


def closed_form(a, b):
    """min(Levenshtein distance, 3) of equal-length reads, rows of a against rows of b ([P, L] symbol arrays):
    at most two mismatches, or one read the other shifted by one cycle between the first and the last mismatch."""
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    P, L = a.shape
    m = a != b
    h = m.sum(axis=1)
    p = m.argmax(axis=1)
    t = L - 1 - m[:, ::-1].argmax(axis=1)
    mu = np.ones((P, L + 1), dtype=np.int16)                # b[i] != a[i+1]
    md = np.ones((P, L + 1), dtype=np.int16)                # b[i] != a[i-1]
    mu[:, :L - 1] = b[:, :L - 1] != a[:, 1:]
    md[:, 1:L] = b[:, 1:] != a[:, :L - 1]
    cu = np.concatenate([np.zeros((P, 1), np.int16), np.cumsum(mu, axis=1, dtype=np.int16)], axis=1)
    cd = np.concatenate([np.zeros((P, 1), np.int16), np.cumsum(md, axis=1, dtype=np.int16)], axis=1)
    r = np.arange(P)
    up = cu[r, t] - cu[r, p] == 0                           # [p, t)
    down = cd[r, t + 1] - cd[r, p + 1] == 0                 # (p, t]
    return np.where(h <= 2, h, np.where(up | down, 2, 3))


def screen_words(codes):
    """k_dense_sig's screen word per read: byte & 3 of the first 16 cycles, 2 bits each - a no-call reads as A."""
    c = np.where(codes[:, :SCREEN] == 4, 0, codes[:, :SCREEN]).astype(np.uint32)
    return (c << (2 * np.arange(c.shape[1], dtype=np.uint32))[None, :]).sum(axis=1).astype(np.uint32)


def screen_passes(a, b):
    """lev2_screen(a, a >> 2, a << 2, b) <= 1 on arrays of screen words: what the compare stage queues."""
    def fold(x):
        return (x | (x >> np.uint32(1))) & np.uint32(0x55555555)

    def pop(x):
        return np.unpackbits(x.view(np.uint8).reshape(-1, 4), axis=1).sum(axis=1)
    a, b = a.astype(np.uint32), b.astype(np.uint32)
    m0 = fold(a ^ b)
    up = (((a >> np.uint32(2)) ^ b) | (((a >> np.uint32(2)) ^ b) >> np.uint32(1))) & m0
    dn = (((a << np.uint32(2)) ^ b) | (((a << np.uint32(2)) ^ b) >> np.uint32(1))) & m0
    first = (pop(m0).astype(np.int64) - 1) % (1 << 32)              # popc(m0) - 1 as an unsigned word
    return np.minimum(np.minimum(first, pop(up)), pop(dn)) <= 1


def queue_bound(case, tile):
    """The most survivors one group of 64 targets can queue on this tile: its (target, slot) pairs that pass the
    screen, seen from both ends (the two-ended compare; the one-ended one queues half of them)."""
    centre, lvl_off, nbr = case.csr
    slot_c = np.searchsorted(lvl_off[:, 0], np.arange(nbr.shape[0]), side="right") - 1
    w = screen_words(case.tiles[tile].codes)
    passes = screen_passes(w[slot_c], w[nbr])
    return int(np.bincount(slot_c[passes] // 64, minlength=1).max())


def shifted(a, p, t, up, drawn):
    b = a.copy()
    if up:
        b[p:t] = a[p + 1:t + 1]
        b[t] = drawn
    else:
        b[p + 1:t + 1] = a[p:t]
        b[p] = drawn
    return b


class Pair:
    __slots__ = ("tile", "w", "v", "kind", "p", "t", "direction", "intended")

    def __init__(self, tile, w, v, kind, p, t, direction, intended):
        self.tile, self.w, self.v, self.kind, self.p, self.t = tile, w, v, kind, p, t
        self.direction, self.intended = direction, intended

    def __repr__(self):
        return "Pair(tile %d, %d -> %d, %s, p %d, t %d)" % (self.tile, self.w, self.v, self.kind, self.p, self.t)


class Tile:
    def __init__(self, codes, planes, filt, shared):
        self.codes, self.planes, self.filt, self.shared = codes, planes, filt, shared


class Case:
    def __init__(self, L, csr, tiles, pairs):
        self.L, self.csr, self.tiles, self.pairs = L, csr, tiles, pairs


def _random_read(rng, L):
    c = rng.integers(0, N_SYM, size=L)
    return np.where(rng.random(L) < 0.02, 4, c).astype(np.int8)


def _substitute(rng, b, at):
    b[at] = (int(b[at]) + int(rng.integers(1, 5))) % 5


def _plan(L):
    """[(kind, p, t, direction, intended)] - every kind for every p < t of B(L), then the two kinds behind the screen."""
    B = boundary_set(L)
    plan = []
    i = 0
    for p in B:
        for t in B:
            if p >= t:
                continue
            d, e = ("up", "down")[i % 2], ("up", "down")[(i + 1) % 2]
            plan.append(("up", p, t, "up", 2))
            plan.append(("down", p, t, "down", 2))
            if [at for at in (0, p - 1, t + 1, L - 1) if 0 <= at < L and (at < p or at > t)]:
                plan.append((d + "+out", p, t, d, 3))
            if t - p >= 2:
                plan.append((e + "+in", p, t, e, 3))
                plan.append(("two-stretches", p, t, d, 4))
                plan.append(("subs3", p, t, None, 3))
            plan.append(("up-nocall", p, t, "up", 2))
            plan.append(("up-nocall-A", p, t, "up", 3))
            plan.append(("subs2", p, t, None, 2))
            plan.append((e + "-two-letters", p, t, e, 2))
            i += 1
    if L > SCREEN:
        for j in range(40):
            plan.append(("tail", SCREEN, L - 1, None, min(1 + j % 3, L - SCREEN)))
            plan.append(("late-third", 0, L - 1, None, 3))
    return plan


def _script(rng, L, kind, p, t, direction, intended, serial, prefix=None):
    """(a, b, whether a was drawn behind `prefix`) of one scripted pair; a begins with `prefix` where the script can
    live with it."""
    up = direction == "up"
    for attempt in range(1000):
        a = _random_read(rng, L)
        kept = prefix is not None and attempt < 50
        if kept:
            a[:prefix.shape[0]] = prefix
        if kind in ("up", "down"):
            b = shifted(a, p, t, up, int(rng.integers(0, 5)))
            if a[p] == b[p] or a[t] == b[t]:                # the first and the last mismatch where they are planned
                continue
            if t - p >= 4 and (a != b).sum() < 3:           # a shift that shows as one: more mismatches than a
                continue                                    # pair of substitutions has
        elif kind.endswith("+out"):
            b = shifted(a, p, t, up, int(rng.integers(0, 5)))
            ats = [at for at in (0, p - 1, t + 1, L - 1) if 0 <= at < L and (at < p or at > t)]
            _substitute(rng, b, ats[serial % len(ats)])
        elif kind.endswith("+in"):
            b = shifted(a, p, t, up, int(rng.integers(0, 5)))
            _substitute(rng, b, int(rng.integers(p + 1, t)))
        elif kind in ("up-nocall", "up-nocall-A"):
            m = int(rng.integers(p + 1, t + 1))
            a[m] = 4
            b = shifted(a, p, t, True, int(rng.integers(0, 5)))
            if kind == "up-nocall-A":
                b[m - 1] = 0
        elif kind == "two-stretches":
            m = int(rng.integers(p, t - 1))
            b = shifted(a, p, m, up, int(rng.integers(0, 5)))
            b = shifted(b, m + 2, t, bool(rng.integers(0, 2)), int(rng.integers(0, 5)))
        elif kind in ("subs2", "subs3"):
            b = a.copy()
            _substitute(rng, b, p)
            _substitute(rng, b, t)
            if kind == "subs3":
                _substitute(rng, b, int(rng.integers(p + 1, t)))
        elif kind.endswith("-two-letters"):
            x = int(rng.integers(0, 4))
            y = (x + int(rng.integers(1, 4))) % 4
            a[p:t + 1] = np.where(rng.integers(0, 2, size=t + 1 - p) == 1, x, y)
            b = shifted(a, p, t, up, (x, y)[int(rng.integers(0, 2))])
        elif kind == "tail":
            b = a.copy()
            for at in rng.choice(np.arange(SCREEN, L), size=intended, replace=False):
                _substitute(rng, b, int(at))
        elif kind == "late-third":
            b = a.copy()
            for at in rng.choice(SCREEN, size=2, replace=False):
                _substitute(rng, b, int(at))
            _substitute(rng, b, int(rng.integers(SCREEN, L)))
            fa, fb = np.where(a[:SCREEN] == 4, 0, a[:SCREEN]), np.where(b[:SCREEN] == 4, 0, b[:SCREEN])
            if closed_form(a, b)[0] < 3 or closed_form(fa, fb)[0] > 2:
                continue
        else:
            raise ValueError(kind)
        return a, b, kept
    raise RuntimeError("no script for %s p %d t %d" % (kind, p, t))


def codes_to_bytes(rng, codes):
    """BCL bytes: a no-call is 0, else random non-zero quality bits above the base."""
    q = rng.integers(1, 41, size=codes.shape)
    return np.where(codes == 4, 0, (q << 2) | (codes & 3)).astype(np.uint8)


@lru_cache(maxsize=None)
def generate(L, seed=20):
    rng = np.random.default_rng([seed, L])
    csr = targets()
    centre, lvl_off, nbr = csr
    n = centre.shape[0]
    assert (centre == np.arange(n)).all()
    # the plain shifts go to tiles 0 and 1, whose survivor queues must not overflow (queue_bound): a batch in which
    # one queue overflows settles every survivor on packed rows, and lev2_gather would never see a pair
    per_tile = [[] for _ in range(N_TILES)]
    n_plain = n_other = 0
    for entry in _plan(L):
        if entry[0] in ("up", "down"):
            per_tile[GATHER_TILES[n_plain % 2]].append(entry)
            n_plain += 1
        else:
            per_tile[2 if n_other % 20 < 9 else GATHER_TILES[n_other & 1]].append(entry)
            n_other += 1
    slots = np.arange(nbr.shape[0])
    slot_c = (np.searchsorted(lvl_off[:, 0], slots, side="right") - 1).astype(np.int64)      # every slot's centre
    slot_v = nbr.astype(np.int64)
    tiles, pairs = [], []
    for ti in range(N_TILES):
        codes = np.where(rng.random((n, L)) < 0.02, 4, rng.integers(0, N_SYM, size=(n, L))).astype(np.int8)
        shared, prefix = np.zeros(n, dtype=bool), None
        if ti == 2:
            shared = rng.random(n) < 1 / 3
            prefix = rng.integers(0, N_SYM, size=min(SCREEN, L)).astype(np.int8)
            codes[shared, :SCREEN] = prefix
        bad = rng.random(n) < 0.03
        # placement: w and one well of w's own rings, alternately below and above w; scripted wells distinct
        free = ~bad
        order = rng.permutation(n)
        owner = np.full(n, -1, dtype=np.int64)                       # scripted well -> index into `mine`
        mine = []
        at = 0
        for serial, (kind, p, t, direction, intended) in enumerate(per_tile[ti]):
            want_lower = serial % 2 == 0
            while True:
                assert at < n, "not enough wells for the scripts of L = %d" % L
                w = int(order[at])
                at += 1
                if not free[w]:
                    continue
                ring = nbr[lvl_off[w, 0]:lvl_off[w, -1]]
                ring = ring[free[ring] & ((ring < w) if want_lower else (ring > w))]
                if ring.size:
                    break
            v = int(ring[rng.integers(0, ring.size)])
            free[w] = free[v] = False
            owner[w] = owner[v] = len(mine)
            mine.append(Pair(ti, w, v, kind, p, t, direction, intended))

        def write(j):
            pr = mine[j]
            a, b, kept = _script(rng, L, pr.kind, pr.p, pr.t, pr.direction, pr.intended, j, prefix if shared[pr.w] else None)
            codes[pr.w], codes[pr.v] = a, b
            shared[pr.w] = shared[pr.v] = kept                       # (b: the prefix with a script's edits in it)
        for j in range(len(mine)):
            write(j)
        # the background: no neighbours within distance 2 but the scripts and tile 2's shared prefix
        own = (owner[slot_c] >= 0) & (owner[slot_c] == owner[slot_v])
        for _ in range(200):
            near = closed_form(codes[slot_c], codes[slot_v]) <= 2
            near &= ~own & ~(shared[slot_c] & shared[slot_v])
            if not near.any():
                break
            redone = set()
            for c, v in zip(slot_c[near], slot_v[near]):
                x = c if owner[c] < 0 else v                         # a background well if there is one
                if x in redone or c in redone:
                    continue
                redone.add(x)
                if owner[x] < 0:
                    codes[x] = _random_read(rng, L)
                    shared[x] = False
                else:
                    write(int(owner[x]))
        else:
            raise RuntimeError("background of L = %d keeps pairs within distance 2" % L)
        b = codes_to_bytes(rng, codes)
        filt = ((rng.integers(0, 128, size=n) << 1) | 1).astype(np.uint8)   # bit 0 is the filter, the rest noise
        filt[bad] &= 0xFE
        tiles.append(Tile(codes, [np.ascontiguousarray(b[:, c]) for c in range(L)], filt, shared))
        pairs += mine
    return Case(L, csr, tiles, pairs)


@lru_cache(maxsize=None)
def expected(L):
    """The oracle's answer per tile, computed once: [(valid, dups, lens, dist)] for Levenshtein <= 2."""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import oracle
    case = generate(L)
    oracle.lib()
    with ThreadPoolExecutor(N_TILES) as pool:             # (the C oracle runs outside the interpreter's lock)
        return list(pool.map(lambda t: oracle.count_tile(t.planes, t.filt, *case.csr, mode=2, k=2, want_dist=True),
                             case.tiles))


def slot_of(case, w, v):
    """v's slot in w's rings."""
    centre, lvl_off, nbr = case.csr
    lo, hi = int(lvl_off[w, 0]), int(lvl_off[w, -1])
    return lo + int(np.flatnonzero(nbr[lo:hi] == v)[0])
