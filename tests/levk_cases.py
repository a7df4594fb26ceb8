"""The cases of Levenshtein <= k by the banded DP, k >= 2, that tests/test_levk_emu.py (the kernels' source on the CPU
under shuffled schedules, tools/scan_lev_emu.cpp) and tests/test_gpu_levk_cases.py (the kernels on the GPU, through
Scanner) hold to one truth: the CPU oracle's counts, tallies and distances (scanq_cases.truth).  Plain numpy, no GPU.

Three kernel kinds run such a scan (wd_scan_async, csrc/welldup_scan.hip):
  "queue"    k_scan_q<S, B1, LEVH, WS>, LEVH = 1 .. 3: k = 2 (with lev2_closed = 0) .. 7, the DP state in 16-byte queue entries;
  "seq"      k_scan<LevState<H>, S, lev_first(H), kLevB2>, H in {1, 2, 3, 4, 6, 8}: k = 8 .. 17, any k >= 2 with queue_kernel = 0
             or early_exit = 0, and any target of more than 508 slots;
  "generic"  k_scan_lev_generic<S>: k >= 18 (band half-width k / 2 > 8), DP row and codes in LDS.
A case names its kind, the layout ("ptr", "plane", "il") and the options that select the kernel; `kernel` is the name both
the emulator and wd_last_kernel() must report.

Built on tests/scanq_cases.py (Case, truth, write_case, cuts_of) and tests/survival_ref.py (codes, bytes, filters).  What
is new here is the reads: a neighbour is its centre with s substitutions, i insertions and i deletions at scripted places
(2 i + s from k - 1 to k + 2), so that pairs lie AT the threshold, one above it, and on the band's outermost diagonal.
An edit script states an intention - an inserted letter may repeat its neighbour, two edits may cancel; the oracle alone
decides the distance, and tests/test_levk_cases_host.py asserts from the oracle's distances that the set still holds
what it is meant to hold."""
from __future__ import annotations

import numpy as np

import scanq_cases as qc
import survival_ref as sr
from scanq_cases import LAYOUTS, INVALID, truth, cuts_of            # noqa: F401  (the test modules' names)

KINDS = ("queue", "seq", "generic")
SEQ_H = (1, 2, 3, 4, 6, 8)                    # launch_lev's instantiations (csrc/welldup_scan.hip)
LEV_FIRST = {1: 7, 2: 10, 3: 13, 4: 16, 6: 20, 8: 24}         # lev_first(H), csrc/wd_shared.h
LEV_B2 = 8                                    # kLevB2, csrc/welldup_scan.hip: cycles of k_scan's later batches
SEQ_MAX_SLOTS = 2048                          # (no limit of k_scan's; the most a case here asks for is 509)


def seq_h(h):
    """the band half-width launch_lev instantiates for h = k / 2 (csrc/welldup_scan.hip: the chain of h <= ..)"""
    return h if h <= 4 else 6 if h <= 6 else 8


def queue_first(layout, k):
    """B1 as launch_queue_lev_t (csrc/welldup_queue.hip) chooses it: first_even / first_odd of lev_first(H), 8 interleaved"""
    H = k // 2
    if layout == "il":
        return 8
    if k & 1:
        return LEV_FIRST[H] + 1 - (2 if H == 1 else 0)
    return LEV_FIRST[H] - (2 if H <= 2 else 0)


def boundaries(kind, layout, B1, L):
    """The cycles behind which the kernel at hand decides who lives on (alive()): the end of the first round, then
    q_drain_lev's rounds of 1, 2, 4, 8, 8 .. cycles (4, 8, 8 .. interleaved), k_scan's batches of kLevB2."""
    if kind == "generic":
        return [L // 2]
    out, j = [], B1
    nb = LEV_B2 if kind == "seq" else 4 if layout == "il" else 1
    while j < L:
        out.append(j)
        j += nb
        nb = LEV_B2 if kind == "seq" else min(8, nb * 2)
    return out


class Case(qc.Case):
    MAX_SLOTS = SEQ_MAX_SLOTS

    def __init__(self, name, kind, layout, k, L, tpb, levels, n, lists, tiles, codes, early=1, queue_kernel=1, sort=False,
                 hit_cap=-1, tags=()):
        self.kind, self.early, self.queue_kernel, self.codes = kind, early, queue_kernel, codes
        assert kind in KINDS and (layout != "il" or kind == "queue") and 2 <= k
        super().__init__(name, "lev", layout, k, L, tpb, levels, n, lists, tiles, sort=sort, per_target=True, hit_cap=hit_cap, tags=tags)
        slots = int(np.diff(self.lvl_off[:, [0, -1]], axis=1).max())
        assert k < L or hit_cap > 0           # (k >= L without a hit log is a Hamming scan)
        assert (kind == "queue") == (self.kk // 2 <= 3 and early == 1 and queue_kernel == 1 and slots <= qc.K_MAX_PASSES * qc.K_PASS)
        assert (kind == "generic") == (self.kk // 2 > 8)

    def instantiation(self):
        S = "false" if self.layout == "ptr" else "true"
        H = self.kk // 2
        if self.kind == "queue":
            B1 = queue_first(self.layout, self.kk)
            return B1, "k_scan_q<%s, %d, %d, %d>" % (S, B1, H, 4 if self.layout == "il" else 1)
        if self.kind == "seq":
            return LEV_FIRST[seq_h(H)], "k_scan<LevState<%d>, %s, %d, %d>" % (seq_h(H), S, LEV_FIRST[seq_h(H)], LEV_B2)
        return 0, "k_scan_lev_generic<%s>" % S

    @property
    def band(self):
        """the band half-width the kernel runs with (the launcher's figure)"""
        return seq_h(self.kk // 2) if self.kind == "seq" else self.kk // 2

    @property
    def group(self):
        """(the instantiation, the threshold the kernel is given): what the conditions of the case set are counted by"""
        return self.kernel, self.kk


def write_case(path, case):
    """scanq_cases.write_case with the family word 2 and, behind the hit records, {kind, band half-width, early}"""
    qc.write_case(path, case, extra=[KINDS.index(case.kind), case.band, case.early])


# ---- reads -----------------------------------------------------------------------------------------------------------
def centre_read(rng, L, kind):
    """codes 0 = N, 1 .. 4 = A C G T.  "random": 6 % no-calls; "two": two letters, where many alignments tie; "runs":
    homopolymer runs of 2 .. 6; "nocall": random with a no-call at every fifth cycle."""
    if kind == "two":
        a, b = rng.choice(4, size=2, replace=False) + 1
        return [int(a if v else b) for v in rng.random(L) < 0.5]
    if kind == "runs":
        out = []
        while len(out) < L:
            out += [int(rng.integers(1, 5))] * int(rng.integers(2, 7))
        return out[:L]
    c = sr.random_codes(rng, (L,)).tolist()
    if kind == "nocall":
        c[::5] = [0] * len(c[::5])
    return c


def apply_script(rng, c, ins, dele, sub, nocall=False):
    """The centre's read c with a letter inserted before each position of `ins` (L: behind the end; a position may
    repeat), the positions of `dele` deleted and those of `sub` substituted (by a no-call, where the centre has a base
    there and nocall is set).  As many insertions as deletions: the length is kept."""
    L, out = len(c), []
    assert len(ins) == len(dele) and not (set(dele) & set(sub))
    for p in range(L + 1):
        for _ in range(ins.count(p)):
            out.append((c[min(p, L - 1)] + int(rng.integers(1, 5))) % 5)      # (not the letter it pushes along)
        if p < L and p not in dele:
            if p in sub:
                out.append(0 if nocall and c[p] else (c[p] + int(rng.integers(1, 5))) % 5)
            else:
                out.append(c[p])
    assert len(out) == L
    return out


def _window(rng, lo, hi, m, L):
    """m distinct positions of [lo, hi), the window grown to the left (then to the right) until it holds them"""
    lo, hi = max(lo, 0), min(hi, L)
    while hi - lo < m and lo > 0:
        lo -= 1
    while hi - lo < m:
        hi += 1
    assert hi <= L
    return [int(v) for v in rng.choice(np.arange(lo, hi), size=m, replace=False)]


def scripts(rng, kind, layout, k, H, B1, L):
    """Every (placement, 2 i + s, i) of the issue's list that fits L -> [(placement, ins, dele, sub, nocall)].
    a+ / a-  all insertions at cycle 0 and all deletions at cycle L - 1 (a-: the other direction - the deletions first, the
             insertions behind the end), the path on diagonal +-i for the whole read; i up to H + 1 (one past the band)
    c        every edit inside the first round
    d        edits about a boundary of the schedule, every boundary in turn
    e        edits in the last H cycles, the rows finish() runs
    f        insertions in the first three cycles, their deletions at the end, the substitutions early: the pair is at its
             dearest from the start, and within k only behind its last cycle
    g        as d, the substitutions by no-calls on the neighbour's side alone (the centres carry the shared ones)"""
    out = []
    bnds = [b for b in boundaries(kind, layout, B1, L) if 0 < b < L] or [max(L // 2, 1)]
    turn = 0
    for tot in (k - 1, k, k + 1, k + 2):
        for i in range(0, min(H + 1, tot // 2, L // 2) + 1):
            s = tot - 2 * i
            if i + s > L or s < 0:
                continue
            if i:
                mid = _window(rng, i, L - i, s, L) if s <= L - 2 * i else None
                if mid is not None:
                    out.append(("a+", [0] * i, list(range(L - i, L)), mid, False))
                    out.append(("a-", [L] * i, list(range(i)), mid, False))
                    early = _window(rng, 3, max(B1, 4), s, L) if s <= L - i - 3 and not set(range(3, 3 + s)) & set(range(L - i, L)) else None
                    if early is not None and not set(early) & set(range(L - i, L)):
                        out.append(("f", [int(v) for v in rng.integers(0, 3, size=i)], list(range(L - i, L)), early, False))
            b = bnds[turn % len(bnds)]
            turn += 1
            for name, lo, hi in (("c", 0, max(min(B1, L), 1)), ("d", b - 1 - (i + s) // 2, b + 1 + (i + s) // 2), ("e", L - max(H, 1), L),
                                 ("g", b - 1 - (i + s) // 2, b + 1 + (i + s) // 2)):
                at = _window(rng, lo, hi, i + s, L)
                dele, sub = at[:i], at[i:]
                ins = [int(v) for v in rng.integers(max(min(at) - 1, 0), min(max(at) + 2, L + 1), size=i)] if at else []
                out.append((name, ins, dele, sub, name == "g"))
    return out


def restricted_distance(a, b, band):
    """The textbook DP of rows a [P, L] against b [P, L], restricted to |j - i| <= band (band < 0: nothing is inside - every
    pair is `big`): int64 [P].  With band >= L it is the edit distance.  A row at a time over all pairs: the step along
    the row, cur[j] = min over j' <= j of tmp[j'] + (j - j'), is a running minimum of tmp[j'] - j'."""
    P, L = a.shape
    big = 1 << 20
    if band < 0:
        return np.full(P, big, dtype=np.int64)
    j = np.arange(L + 1, dtype=np.int64)
    prev = np.where(j <= band, j, big)[None, :].repeat(P, axis=0)
    for i in range(1, L + 1):
        inside = np.abs(j - i) <= band
        tmp = np.full((P, L + 1), big, dtype=np.int64)
        tmp[:, 1:] = np.minimum(prev[:, :-1] + (a[:, i - 1:i] != b), prev[:, 1:] + 1)
        tmp[:, 0] = i
        tmp[:, ~inside] = big
        cur = np.minimum.accumulate(tmp - j, axis=1) + j
        cur[:, ~inside] = big
        prev = np.minimum(cur, big)
    return prev[:, L]


def pairs_of(case):
    """-> (centre codes [P', L], neighbour codes [P', L]) of every pair of a valid centre, all tiles, and the oracle's
    distances [P'] in the same order"""
    slots = np.arange(case.nbr.shape[0])
    tgt = np.searchsorted(case.lvl_off[:, 0], slots, side="right") - 1
    t = truth(case)
    cen, nb, dist = [], [], []
    for i, ((planes, filt), codes) in enumerate(zip(case.tiles, case.codes)):
        valid = (filt[case.centre[tgt]] & 1) == 1
        cen.append(codes[case.centre[tgt]][valid])
        nb.append(codes[case.nbr][valid])
        dist.append(t["dist"][i][valid])
    return np.concatenate(cen), np.concatenate(nb), np.concatenate(dist)


def _whole_read_target(rng, L, K):
    """k = L - 1, the widest threshold a scan has: what 2 i + s about k cannot script, since no pair lies above L.
    The centre is A^H u, H = (L - 1) / 2, u random over {G, T, N}; the neighbours, in turn:
      u' C^H, u' = u with one substitution or none: H deletions and H insertions, 2 H (+ 1) <= k, on the outermost diagonal
              for the whole read - and every cycle a mismatch in place (Hamming distance L);
      C^L: distance L = k + 1, no letter shared;  C^L with one cycle the centre's: distance L - 1 = k.
    -> (centre, [K reads])"""
    H = (L - 1) // 2
    # (u opens with no-calls and closes with bases: where its two copies meet, on the diagonals about the main one, nothing matches)
    u = [0] * 4 + [int(v) for v in rng.choice([0, 3, 4], size=L - H - 10)] + [int(v) for v in rng.choice([3, 4], size=6)]
    c = [1] * H + u
    reads = []
    for e in range(K):
        if e % 3 == 0:
            v = list(u)
            if e % 2:
                at = int(rng.integers(L - 2 * H, L - H))           # (not a cycle that meets u again in place)
                v[at] = [x for x in (0, 3, 4) if x != v[at]][int(rng.integers(0, 2))]
            reads.append(v + [2] * H)
        else:
            v = [2] * L
            if e % 3 == 2:
                at = int(rng.integers(0, L))
                v[at] = c[at]
            reads.append(v)
    return c, reads


# ---- the cases -------------------------------------------------------------------------------------------------------
CENTRES = ("random", "two", "random", "runs", "nocall", "random")


def _tile(rng, kind, layout, k, H, B1, L, Ks, levels, bad=(), where=None):
    """Targets of Ks[t] slots, the wells disjoint and in a random order of the tile: target t's neighbours are the scripts
    of its centre, taken in turn from scripts() (a target of more slots than scripts goes round).
    -> (n, lists, where - the wells' order, for the next tile -, codes [n, L], planes, filt)"""
    n = max(sum(K + 1 for K in Ks), 257)
    where = rng.permutation(n) if where is None else where
    codes = sr.random_codes(rng, (n, L))
    lists, at = [], 0
    for t, K in enumerate(Ks):
        if t == 0 and k == L - 1 and kind == "generic":
            c, reads = _whole_read_target(rng, L, K)
        else:
            c = centre_read(rng, L, CENTRES[t % len(CENTRES)])
            sc = scripts(rng, kind, layout, k, H, B1, L)
            start = int(rng.integers(0, len(sc)))
            reads = [apply_script(rng, c, *sc[(start + e) % len(sc)][1:]) for e in range(K)]
        codes[where[at]] = c
        codes[where[at + 1:at + 1 + K]] = reads
        wells = [int(w) for w in where[at + 1:at + 1 + K]]
        lists.append((int(where[at]), wells, cuts_of(K, levels)))
        at += K + 1
    is_bad = np.zeros(n, dtype=bool)
    is_bad[[lists[t][0] for t in bad]] = True
    nbrs = np.array([w for _, ws, _ in lists for w in ws])
    is_bad[nbrs[rng.random(nbrs.shape[0]) < 0.02]] = True             # neighbours that fail the filter: must not matter
    b = sr.codes_to_bytes(rng, codes)
    return n, lists, where, codes, [np.ascontiguousarray(b[:, c]) for c in range(L)], sr.filter_bytes(rng, n, is_bad)


def _lengths(kind, layout, k, B1):
    """L of the issue's list for the kernel at hand: k + 1, B1 - 1, B1, B1 + 1, the ends of the second and third round
    behind the first, 37 and 64 - those a Levenshtein scan can be launched at (k < L)"""
    if kind == "generic":
        return [40, 64]
    step = (8, 16) if kind == "seq" else (12, 20) if layout == "il" else (3, 7)
    Ls = [k + 1, B1 - 1, B1, B1 + 1, B1 + step[0], B1 + step[1], 37, 64]
    return sorted({L for L in Ls if L > k})


def not_launchable():
    """(kind, layout, k, L) of the issue's list that wd_scan_async does not run as a Levenshtein scan: k >= L is a
    Hamming problem there (csrc/welldup_scan.hip: `if (k >= L)`), the hit log apart"""
    out = []
    for kind, layout, k, early, qk in _plan_groups():
        B1 = queue_first(layout, k) if kind == "queue" else LEV_FIRST[seq_h(k // 2)] if kind == "seq" else 0
        for L in (B1 - 1, B1, B1 + 1):
            if kind != "generic" and L <= k:
                out.append((kind, layout, k, L))
    return sorted(set(out))


def _plan_groups():
    """(kind, layout, k, early_exit, queue_kernel) of every instantiation the launchers have, at every threshold that maps
    to it.  k_scan runs where the queue kernel is switched off (early_exit = 1) and where early_exit = 0."""
    out = []
    for layout in ("ptr", "plane"):
        for k in range(2, 8):
            out.append(("queue", layout, k, 1, 1))
    out += [("queue", "il", 2, 1, 1), ("queue", "il", 3, 1, 1)]
    for layout in ("ptr", "plane"):
        for k in range(2, 18):
            out.append(("seq", layout, k, 1, 0))
            out.append(("seq", layout, k, 0, 1))
    for layout in ("ptr", "plane"):
        for k in (18, 19, -1):
            out.append(("generic", layout, k, 1, 1))
    return out


def planned_names():
    """The names of every case, from the plan alone (tests/test_levk_cases_host.py: none is dropped after generation)"""
    return [name for name, _ in _plan()]


def _plan():
    out = []
    for g, (kind, layout, k, early, qk) in enumerate(_plan_groups()):
        H = k // 2 if kind != "seq" else seq_h(k // 2)
        B1 = queue_first(layout, k) if kind == "queue" else LEV_FIRST[H] if kind == "seq" else 0
        Ls = _lengths(kind, layout, k, B1)
        if kind == "seq":
            # the two ways into k_scan share the list: the lengths in turn, both at 37
            Ls = [L for j, L in enumerate(Ls) if L == 37 or j % 2 == early]
        for j, L in enumerate(Ls):
            kk = L - 1 if k < 0 else k
            name = "%s_%s_k%d_L%d%s" % (kind, layout, kk, L, "" if kind != "seq" else "_early%d" % early)
            out.append((name, dict(kind=kind, layout=layout, k=kk, L=L, early=early, queue_kernel=qk, seed=[g, j])))
    # more slots than the queue kernel's four passes hold: the first target it hands over to k_scan
    for layout, k in (("plane", 4), ("ptr", 7)):
        out.append(("seq_%s_k%d_L37_slots509" % (layout, k), dict(kind="seq", layout=layout, k=k, L=37, early=1, queue_kernel=1, seed=[900, k], slots509=True)))
    # k >= L with the hit log on: the log wants the true distances, so the DP runs with k = L (every pair a duplicate)
    for layout in ("ptr", "plane"):
        out.append(("seq_%s_k16_L16_hitlog" % layout, dict(kind="seq", layout=layout, k=16, L=16, early=1, queue_kernel=1, seed=[901], hitlog=True)))
        out.append(("generic_%s_k25_L20_hitlog" % layout, dict(kind="generic", layout=layout, k=25, L=20, early=1, queue_kernel=1, seed=[902], hitlog=True)))
    return out


def _build(name, kind, layout, k, L, early, queue_kernel, seed, slots509=False, hitlog=False):
    rng = np.random.default_rng([77, KINDS.index(kind), LAYOUTS.index(layout)] + list(seed))
    kk = min(k, L)
    H = kk // 2 if kind != "seq" else seq_h(kk // 2)
    B1 = queue_first(layout, kk) if kind == "queue" else LEV_FIRST[H] if kind == "seq" else 0
    j = seed[-1]
    tags = []
    if slots509:
        Ks, levels, tpb, n_tiles = [509, 40, 127], 3, 2, 1
    elif L == 37 or (kind == "generic" and L == 40):
        # slot counts at 1, 64, 127, 128 and a ragged block; one level (a target of one slot has one ring)
        Ks, levels, tpb, n_tiles = [128, 1, 64, 127, 200, 97, 33, 255], 1, 3, 1
        tags.append("main")
    elif L == 64:
        Ks, levels, tpb, n_tiles = [130, 97, 65, 255, 40], 8, 16, 2
        tags.append("main")
    else:
        Ks, levels, tpb, n_tiles = [90, 70, 45], 2 + j % 4, (1, 64)[j % 2], 1
    if kind == "generic":
        Ks = [min(K, 130) for K in Ks]        # (a lane per slot, 64 slots a pass, no early exit: correct, not fast)
    bad = (2,) if len(Ks) > 2 and not slots509 else ()
    tiles, codes = [], []
    where = lists = n = None
    for _ in range(n_tiles):                  # (every tile the same wells - the targets are the scan's -, other reads)
        n, lists, where, c, planes, filt = _tile(rng, kind, layout, kk, H, B1, L, Ks, levels, bad=bad, where=where)
        tiles.append((planes, filt))
        codes.append(c)
    if "main" in tags or hitlog or slots509:
        tags.append("hitlog")
    if early == 1 and kind == "seq" and L == 37 and layout == "plane" and k == 8 and not slots509:
        # (the last target is valid, and its last slot is nbr's last entry)
        tags.append("bufend")
    return Case(name, kind, layout, k, L, tpb, levels, n, lists, tiles, codes, early=early, queue_kernel=queue_kernel,
                sort=bool(j % 2) and kind == "queue",         # (the sorted view is the queue kernels': queue_view, csrc/welldup_scan.hip)
                hit_cap=1 << 20 if "hitlog" in tags else -1, tags=tags)


_cases = []


def cases():
    """Built once per process and shared; nothing changes a case after it is built."""
    if not _cases:
        for name, kw in _plan():
            _cases.append(_build(name, **kw))
        assert len({c.name for c in _cases}) == len(_cases)
    return _cases


def case(name):
    return {c.name: c for c in cases()}[name]
