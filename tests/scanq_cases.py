"""The cases of k_scan_q that tests/test_scanq_emu.py (the kernel's source on the CPU under shuffled schedules,
tools/scan_queue_emu.cpp) and tests/test_gpu_scanq_cases.py (the kernel on the GPU, through Scanner) hold to one truth:
the CPU oracle's counts, tallies and distances.  Plain numpy, no GPU.

The reads come from tests/survival_ref.py: scripted survival (sr.build: the test decides at which cycle a neighbour
stops matching its centre), its edit scripts for the Levenshtein family, and its code / byte / filter helpers for the
unscripted reads (random, every read equal, every base a no-call).  What is new here is the geometry: tiles of 257 to
4099 wells, targets of ragged slot counts in one block, wells at the buffers' ends, and the launch parameters.

A case names the family ("ham": equality / Hamming, "lev2": Levenshtein <= 2 by the closed form), the layout ("ptr": a
pointer per cycle, "plane": strided planes, "il": cycles interleaved by four) and the options that select the
instantiation; `kernel` is the name both the emulator and wd_last_kernel() must report."""
from __future__ import annotations

import numpy as np

import survival_ref as sr
from oracle import oracle

K_PASS, K_MAX_PASSES, K_QCAP = sr.K_PASS, sr.K_MAX_PASSES, sr.K_QCAP
K_FINISH_IN_PLACE, K_FINISH_ALL_MAX = sr.K_FINISH_IN_PLACE, sr.K_FINISH_ALL_MAX
INVALID = 0xFFFFFFFF                          # WD_INVALID_TARGET
FAMILIES, LAYOUTS = ("ham", "lev2"), ("ptr", "plane", "il")
ALL_FAMILIES = FAMILIES + ("lev",)            # "lev": Levenshtein <= k by the banded DP - tests/levk_cases.py's, not a family of cases()
# slots per target at the pass boundaries (127 a pass, lane 63 of the second slot shadows the centre)
K_EDGES = (1, 63, 64, 65, 126, 127, 128, 253, 254, 255, 381, 382, 507, 508)


def first_round(fam, layout, k, queue_first):
    """B1 as launch_queue_t / launch_queue_lev_t (csrc/welldup_queue.hip) choose it."""
    if fam == "ham":
        return 4 if layout == "il" else (queue_first or sr.auto_first(k))
    return 8 if layout == "il" else (queue_first if queue_first in (4, 6) else 5)


class Case:
    MAX_SLOTS = K_MAX_PASSES * K_PASS         # the most slots of a target (tests/linewalk_cases.py: the line walk takes more)

    def instantiation(self):
        """-> (first round, the kernel's name as wd_last_kernel() reports it)"""
        B1 = first_round(self.fam, self.layout, self.kk, self.queue_first)
        return B1, "k_scan_q<%s, %d, %d, %d>" % ("false" if self.layout == "ptr" else "true", B1, -1 if self.fam == "lev2" else 0,
                                                 4 if self.layout == "il" else 1)

    def __init__(self, name, fam, layout, k, L, tpb, levels, n, lists, tiles, queue_first=0, sort=False, per_target=True,
                 hit_cap=1 << 20, check_empty=False, tags=()):
        """lists: per target (centre, [neighbour wells], level cuts [levels + 1] into them); tiles: [(planes, filt)]"""
        self.name, self.fam, self.layout, self.k, self.L, self.tpb, self.levels, self.n = name, fam, layout, k, L, tpb, levels, n
        self.mode = 2 if fam in ("lev2", "lev") else (0 if k == 0 else 1)
        self.queue_first, self.sort, self.per_target, self.hit_cap, self.check_empty = queue_first, sort, per_target, hit_cap, check_empty
        self.tags = set(tags)
        self.kk = min(k, L)                   # what the kernel is given: wd_scan_async caps the threshold at the read's length
        self.B1, self.kernel = self.instantiation()
        self.centre = np.array([c for c, _, _ in lists], dtype=np.int32)
        off, nbr, at = [], [], 0
        for _, wells, cuts in lists:
            assert len(cuts) == levels + 1 and cuts[0] == 0 and cuts[-1] == len(wells) <= self.MAX_SLOTS
            off.append([at + c for c in cuts])
            nbr += list(wells)
            at += len(wells)
        self.lvl_off = np.array(off, dtype=np.int32).reshape(len(lists), levels + 1)
        self.nbr = np.array(nbr, dtype=np.int32)
        self.tiles = tiles
        self.T = len(lists)
        assert 257 <= n <= 4099 and all(f.shape[0] == n and len(p) == L for p, f in tiles)
        assert self.nbr.shape[0] and 0 <= self.nbr.min() and self.nbr.max() < n and self.centre.max() < n

    def csr(self):
        return self.centre, self.lvl_off, self.nbr

    def view(self):
        """(centre, lvl_off, perm or None) as the kernel reads them: sorted by centre if asked for and not sorted already
        (install_sorted_view, csrc/welldup_scan.hip, without its strips: any order gives the same sums)."""
        order = np.argsort(self.centre, kind="stable")
        if not self.sort or (order == np.arange(self.T)).all():
            return self.centre, self.lvl_off, None
        return self.centre[order], self.lvl_off[order], order.astype(np.int32)


def truth(case):
    """-> dict(out_tile int64 [tiles, 1 + 5 levels] as the kernel counts - first / last as histograms -, out_pt uint32
    [tiles, T, levels] with INVALID rows, hits int32 [H, 4] {tile, target, slot, dist}, status).  Computed once, and kept
    with the case (not by its name: tests/linewalk_cases.py has cases of the same names)."""
    if getattr(case, "_truth", None) is not None:
        return case._truth
    levels, T = case.levels, case.T
    empty = (np.diff(case.lvl_off, axis=1) <= 0).any(axis=1)
    slots = np.arange(case.nbr.shape[0])
    tgt = np.searchsorted(case.lvl_off[:, 0], slots, side="right") - 1
    out_tile, out_pt, hits, dists, status = [], [], [], [], 0
    for i, (planes, filt) in enumerate(case.tiles):
        f = filt
        if case.check_empty and empty.any():
            # a valid centre with an empty level: the kernel sets the status bit and counts the target as invalid - the
            # oracle (which refuses such a file as the reference does) is asked about the tile with those centres filtered
            status |= int(((filt[case.centre] & 1) == 1)[empty].any())
            f = filt.copy()
            f[case.centre[empty]] &= 0xFE
        valid, dups, lens, dist = oracle.count_tile(planes, f, case.centre, case.lvl_off, case.nbr, case.mode, case.k, want_dist=True)
        row = oracle.tally_tile(valid, dups, lens).astype(np.int64)
        acco, acci = row[1 + 3 * levels:1 + 4 * levels].copy(), row[1 + 4 * levels:].copy()
        row[1 + 3 * levels:1 + 4 * levels] = np.diff(np.concatenate([[0], acco]))
        row[1 + 4 * levels:] = acci - np.concatenate([acci[1:], [0]])
        out_tile.append(row)
        out_pt.append(np.where(valid[:, None] == 1, dups, -1).astype(np.int64) & 0xFFFFFFFF)
        ok = (valid[tgt] == 1) & (dist <= (0 if case.mode == 0 else case.k))
        hits.append(np.stack([np.full(ok.sum(), i), tgt[ok], slots[ok], dist[ok]], axis=1))
        dists.append(dist)                    # (every pair's, per tile; -1 where the centre is invalid)
    case._truth = dict(out_tile=np.array(out_tile, dtype=np.int64), out_pt=np.array(out_pt).astype(np.uint32),
                       hits=np.concatenate(hits).astype(np.int32), status=status, dist=dists)
    return case._truth


def write_case(path, case, line_pairs=0, extra=()):
    """The file tools/scan_queue_emu.cpp reads (tools/scan_emu_common.h says how); line_pairs and extra - int32 words behind
    the hit records - are the line walk's (tests/linewalk_cases.py, tools/scan_lines_emu.cpp)."""
    t = truth(case)
    centre, lvl_off, perm = case.view()
    extra = np.asarray(extra, dtype="<i4")
    head = np.array([0x31435153, ALL_FAMILIES.index(case.fam), LAYOUTS.index(case.layout), case.B1, case.n, len(case.tiles), case.T,
                     case.levels, case.L, case.kk, case.tpb, perm is not None, case.per_target, case.check_empty, case.hit_cap,
                     t["hits"].shape[0], case.nbr.shape[0], t["status"], line_pairs, extra.shape[0]], dtype="<i4")
    with open(path, "wb") as fh:
        for a in (head, centre.astype("<i4"), lvl_off.astype("<i4"), case.nbr.astype("<i4")):
            fh.write(a.tobytes())
        if perm is not None:
            fh.write(perm.astype("<i4").tobytes())
        for planes, filt in case.tiles:
            fh.write(np.ascontiguousarray(filt, dtype=np.uint8).tobytes())
            for p in planes:
                fh.write(np.ascontiguousarray(p, dtype=np.uint8).tobytes())
        fh.write(t["out_tile"].astype("<i8").tobytes())
        if case.per_target:
            fh.write(t["out_pt"].astype("<u4").tobytes())
        fh.write(t["hits"].astype("<i4").tobytes())
        fh.write(extra.tobytes())


# ---- geometry ------------------------------------------------------------------------------------------------------
def cuts_of(K, levels):
    c = np.linspace(0, K, levels + 1).astype(int)
    assert (np.diff(c) > 0).all(), (K, levels)
    return [int(v) for v in c]


class Wells:
    """What sr.finish wants of a geometry: the tile's size, the centres, every neighbour."""

    def __init__(self, n, lists):
        self.n = n
        self.centre = np.array([c for c, _, _ in lists], dtype=np.int32)
        self.nbr = np.array([w for _, ws, _ in lists for w in ws], dtype=np.int32)


def shared_lists(rng, n, Ks, levels):
    """Targets whose neighbours are drawn from the whole tile (wells shared between targets).  The ends: the first
    centre is well n - 1; well 0 and (with two targets or more) well n - 1 are neighbours, and the last target's last
    neighbour - nbr's last entry - is well 0."""
    T = len(Ks)
    centres = [n - 1] + [int(v) for v in rng.choice(n - 1, size=T - 1, replace=False)]
    lists = []
    for t, K in enumerate(Ks):
        pool = np.setdiff1d(np.arange(n), [centres[t]])
        wells = [int(v) for v in rng.choice(pool, size=K, replace=False)]
        if t == min(1, T - 1) and centres[t] != n - 1:
            wells[0] = n - 1
        if t == T - 1 and (K > 1 or T == 1):
            wells[-1] = 0
        lists.append((centres[t], wells, cuts_of(K, levels)))
    return lists


def unscripted(rng, n, lists, L, kind, tiles=1, bad=()):
    """Tiles of random reads with planted near copies ("random"), of one read ("equal") or of no-calls ("nocall")."""
    g = Wells(n, lists)
    out = []
    for _ in range(tiles):
        if kind == "random":
            codes = sr.random_codes(rng, (n, L))
            fam = sr.random_codes(rng, (6, L))                     # six families: copies with 0 .. 3 substitutions
            near = rng.random(n) < 0.5
            cp = fam[rng.integers(0, 6, size=n)]
            for _s in range(3):
                at, on = rng.integers(0, L, size=n), rng.random(n) < 0.5
                cp[np.arange(n)[on], at[on]] = rng.integers(0, 5, size=int(on.sum()))
            codes[near] = cp[near]
        elif kind == "equal":
            codes = np.repeat(sr.random_codes(rng, (1, L)), n, axis=0)
        else:
            codes = np.zeros((n, L), dtype=np.int8)
        s = sr.finish(rng, g, L, 0, codes, bad_centres=bad)
        out.append((s.planes, s.filt))
    return out


def dead_in_first_round(rng, s, B1):
    """For the Levenshtein family: a pair the script lets die in the first round (death <= B1) gets, at each of the
    round's cycles, a code that is none of the centre's codes of that cycle and of the two beside it.  Neither the read in
    place nor either shift of it then matches anywhere in the round, so the closed form drops the pair where the Hamming
    count does, and the number of survivors of a pass is the script's under both families."""
    g, L = s.geom, s.L
    codes = s.codes.copy()
    cen = codes[g.centre]
    for t, e in zip(*np.nonzero((s.death > 0) & (s.death <= B1))):
        for j in range(B1):
            ban = {int(cen[t, i]) for i in (j - 1, j, j + 1) if 0 <= i < L}
            codes[g.nbr[t * g.K + e], j] = min(set(range(5)) - ban)
    b = sr.codes_to_bytes(rng, codes)
    return sr.Script(g, L, s.k, codes, [np.ascontiguousarray(b[:, c]) for c in range(L)], s.filt, s.death)


def scripted(rng, T, K, levels, L, k, deaths, Ks=None, flip=False, bad=(), edits=False, tiles=1, dead_first=0):
    """sr.build on T targets of K disjoint slots, `deaths(rng)` -> [T, K]; target t keeps its first Ks[t] slots.  flip
    turns the tile round: the first centre becomes well n - 1 and the last target's last neighbour well 0 (unflipped, that
    neighbour is well n - 1).  -> (n, lists, tiles)"""
    geom = sr.Geometry(T, K, levels)
    n = geom.n
    out = []
    for _ in range(tiles):
        s = sr.build(rng, geom, L, k, deaths(rng), bad)
        if dead_first:
            s = dead_in_first_round(rng, s, dead_first)
        if edits:
            s = sr.add_edit_scripts(rng, s)
        planes, filt = s.planes, s.filt
        if flip:
            planes, filt = [np.ascontiguousarray(p[::-1]) for p in planes], np.ascontiguousarray(filt[::-1])
        out.append((planes, filt))
    lists = []
    for t in range(T):
        Kt = K if Ks is None else Ks[t]
        wells = geom.nbr[t * K:t * K + Kt].astype(np.int64)
        c = int(geom.centre[t])
        if flip:
            wells, c = n - 1 - wells, n - 1 - c
        lists.append((c, [int(w) for w in wells], cuts_of(Kt, levels)))
    return n, lists, out


def spread_deaths(T, K, L, B1, alive=0.3):
    """a share `alive` of the pairs survives the first round and dies anywhere behind it (a quarter of those never);
    the others die inside the first round"""
    def f(rng):
        d = rng.integers(1, max(min(B1, L), 1) + 1, size=(T, K))
        late = rng.random((T, K)) < alive
        if L > B1:
            d[late] = rng.integers(B1 + 1, L + 1, size=int(late.sum()))
        d[late & (rng.random((T, K)) < 0.25)] = 0
        return d.astype(np.int32)
    return f


def survivors(T, K, L, k, B1, counts, kinds):
    """counts[t] pairs of target t survive the first round, at random slots, the others die in it (their (k + 1)-th
    mismatch lies in it); kinds[t]: "never", "late" (alive at the last cycle but one), "early" (dead within three cycles
    of the drain, before finish_from(k)), "rounds" (dying one, two, four, eight .. cycles into the drain, in turn), "spread"."""
    assert k + 1 <= B1 and B1 + 3 < sr.finish_from(k) < L
    def f(rng):
        d = rng.integers(k + 1, B1 + 1, size=(T, K)).astype(np.int32)
        for t in range(T):
            at = rng.choice(K, size=counts[t], replace=False)
            kind = kinds[t]
            if kind == "never":
                v = np.zeros(counts[t])
            elif kind == "late":
                v = rng.choice([0, L, L - 1], size=counts[t])
            elif kind == "early":
                v = rng.integers(B1 + 1, B1 + 4, size=counts[t])
            elif kind == "rounds":
                v = B1 + np.array([1, 2, 3, 4, 6, 8, 12, 16, 0])[np.arange(counts[t]) % 9]
                v = np.where(v == B1, 0, np.minimum(v, L))
            else:
                v = np.where(rng.random(counts[t]) < 0.25, 0, rng.integers(B1 + 1, L + 1, size=counts[t]))
            d[t, at] = v
        return d
    return f


# ---- the cases -----------------------------------------------------------------------------------------------------
def _family_layout_cases(fam, layout):
    """Every edge of the issue's list in at least one case of this family and this layout."""
    out = []
    seed = [FAMILIES.index(fam), LAYOUTS.index(layout)]
    lev2 = fam == "lev2"
    k0 = 2 if lev2 else 1
    ks = (2,) * 4 if lev2 else (0, 1, 2, 3)

    def add(name, *a, **kw):
        out.append(Case("%s_%s_%s" % (fam, layout, name), fam, layout, *a, **kw))

    def rng_of(*extra):
        return np.random.default_rng(seed + list(extra))

    # slots per target: the pass boundaries, ragged in one block; wells shared, the buffers' ends; perm given
    rng = rng_of(1)
    lists = shared_lists(rng, 4099, list(K_EDGES), 1)
    add("ragged_K", k0, 37, 3, 1, 4099, lists, unscripted(rng, 4099, lists, 37, "random", bad=(3,)), sort=True, tags=("bufend",))
    rng = rng_of(2)
    Ks = [int(v) for v in rng.permutation(K_EDGES[1:])]
    lists = shared_lists(rng, 2500, Ks, 3)
    add("ragged_K_levels3", ks[2], 30, 16, 3, 2500, lists, unscripted(rng, 2500, lists, 30, "random"), per_target=False, hit_cap=-1)

    # targets, grid and levels: tpb 1, 3, 16, 64; T = 1, tpb, tpb + 1, 65; tiles x chunks = 1, 7, 8, 9, 17; levels 1, 3, 8, 9, 32
    for i, (tpb, T, tiles, levels, K) in enumerate(((1, 1, 1, 1, 5), (3, 3, 7, 3, 40), (3, 4, 4, 8, 70), (16, 16, 9, 9, 30),
                                                    (1, 1, 17, 32, 130), (64, 65, 1, 3, 20), (16, 17, 1, 32, 33), (64, 64, 1, 1, 9),
                                                    (1, 2, 1, 9, 128), (16, 65, 1, 8, 16), (3, 65, 1, 1, 3), (1, 65, 1, 3, 4))):
        rng = rng_of(3, i)
        n = 257 + 97 * i
        lists = shared_lists(rng, n, [K] * T, levels)
        bad = (T // 2,) if T > 2 else ()
        add("grid%d_tpb%d_T%d_tiles%d_levels%d" % (len(range(0, T, tpb)) * tiles, tpb, T, tiles, levels), ks[i % 4], 21, tpb, levels, n, lists,
            unscripted(rng, n, lists, 21, "random", tiles=tiles, bad=bad), sort=bool(i % 2), per_target=i % 3 != 2,
            hit_cap=(1 << 20, -1, 0)[i % 3])

    # L against the first round, finish_from(k) and the 64-cycle ballots; the interleaved groups
    B1s = {}
    for qf, k in ((0, ks[0]), (0, ks[1]), (0, ks[2]), (0, ks[3])) + (((4, 2), (6, 2)) if lev2 else tuple((q, (q + 1) % 4) for q in range(1, 9))):
        if layout == "il" and qf:
            continue
        B1s[(qf, k)] = first_round(fam, layout, k, qf)
    Ls = {}
    for (qf, k), B1 in B1s.items():
        F = sr.finish_from(k)
        for L in (B1 - 1, B1, B1 + 1) if qf == 0 else (F + 5,):
            if L >= 1:
                Ls[(qf, k, L)] = B1
    for k, L in ((ks[1], sr.finish_from(ks[1]) - 1), (ks[2], sr.finish_from(ks[2])), (ks[3], sr.finish_from(ks[3]) + 1), (ks[0], 64),
                 (ks[1], 65), (ks[2], 100)) + (tuple((ks[j % 4], L) for j, L in enumerate((1, 3, 4, 5, 8, 9, 23, 50))) if layout == "il" else ()):
        Ls[(0, k, L)] = first_round(fam, layout, k, 0)
    if not lev2:
        Ls[(0, 5, 4)] = first_round(fam, layout, 5, 0)            # k >= L
        Ls[(0, 40, 37)] = first_round(fam, layout, 40, 0)
    for j, ((qf, k, L), B1) in enumerate(sorted(Ls.items())):
        rng = rng_of(4, j)
        T, K = 5, 127 if j % 2 else 140
        if (layout == "ptr" and L == 1) or (lev2 and L <= k):
            # what the launchers cannot launch: one plane per tile is strided to the host, whatever its address, and
            # Levenshtein <= k on reads of k cycles or fewer is a Hamming scan (wd_scan_async, csrc/welldup_scan.hip)
            continue
        # (two planes of one tile are a stride too: a second tile, whose planes lie elsewhere, makes it a pointer table)
        n, lists, tiles = scripted(rng, T, K, 2, L, k, spread_deaths(T, K, L, B1), flip=bool(j % 2), bad=(2,), edits=lev2 and L >= 3,
                                   tiles=2 if layout == "ptr" and L == 2 else 1)
        add("L%d_k%d_qf%d" % (L, k, qf), k, L, 3, 2, n, lists, tiles, queue_first=qf, sort=False, tags=("bufend",) if j == 0 else ())

    # reads: equal, no-calls; the in-place threshold from both sides; the queue at its cap; 64 and 65 late survivors
    for kind, K, cap in (("equal", 127, 100), ("equal", 39, 1 << 20), ("nocall", 200, 1 << 20)):
        rng = rng_of(5, K)
        lists = shared_lists(rng, 1031, [K] * 6, 2)
        add("%s_K%d" % (kind, K), k0, 29, 3, 2, 1031, lists, unscripted(rng, 1031, lists, 29, kind, bad=(4,)), hit_cap=cap,
            tags=("equal", "hitcap") + (("lowdiv",) if K >= K_FINISH_IN_PLACE and (not lev2 or layout != "il") else ()))
    k, L = k0, 37
    B1 = first_round(fam, layout, k, 0)
    rng = rng_of(6)
    n, lists, tiles = scripted(rng, 4, 127, 3, L, k, survivors(4, 127, L, k, B1, [39, 40, 41, 127], ["spread", "spread", "late", "rounds"]), dead_first=B1 if lev2 else 0)
    add("in_place_39_40", k, L, 1, 3, n, lists, tiles, tags=() if (lev2 and layout == "il") else ("lowdiv",))
    # 32 targets of one pass, one block: wave w takes targets w, w + 4, ..  Wave 0 fills its queue to exactly kQCap and
    # drains before the next push; wave 1 drains at one below; wave 2 at 117; wave 3 fills to kQCap and drains at the end
    # (the last wave's second buffer: the end of the LDS block).  Then 64 late survivors in wave 0 and 65 in wave 1.
    counts, kinds = [0] * 32, ["rounds"] * 32
    for w, (cs, late) in enumerate((((32, 32, 32, 32, 30, 4, 32, 32), (6, 7)), ((32, 32, 32, 31, 30, 3, 32, 33), (6, 7)),
                                    ((39, 39, 39, 30, 38, 38, 38, 14), ()), ((38, 38, 38, 14, 10, 20, 30, 39), ()))):
        for i, c in enumerate(cs):
            counts[w + 4 * i] = c
            kinds[w + 4 * i] = "never" if i in late else "early" if late and i in (4, 5) else ("rounds" if i % 2 else "spread")
    rng = rng_of(7)
    n, lists, tiles = scripted(rng, 32, 127, 1, L, k, survivors(32, 127, L, k, B1, counts, kinds), flip=True, dead_first=B1 if lev2 else 0)
    add("queue_at_cap", k, L, 32, 1, n, lists, tiles, tags=("queue", "lastdrain"))
    # an empty level under check_empty: the status bit, the target invalid
    rng = rng_of(8)
    lists = shared_lists(rng, 700, [30] * 5, 3)
    lists[2] = (lists[2][0], lists[2][1], [0, 12, 12, 30])
    add("empty_level", k0, 25, 3, 3, 700, lists, unscripted(rng, 700, lists, 25, "random"), check_empty=True, tags=("empty",))
    return out


_cases = []


def cases():
    """Built once per process and shared; nothing changes a case after it is built."""
    if not _cases:
        for fam in FAMILIES:
            for layout in LAYOUTS:
                _cases.extend(_family_layout_cases(fam, layout))
        assert len({c.name for c in _cases}) == len(_cases)
    return _cases


def case(name):
    return {c.name: c for c in cases()}[name]
