"""The cases of k_scan_lines (csrc/scan_lines.inc) that tests/test_linewalk_emu.py (the kernel's source on the CPU under
shuffled schedules, tools/scan_lines_emu.cpp) and tests/test_gpu_linewalk_cases.py (the kernel on the GPU, through
Scanner) hold to one truth: the CPU oracle's counts, tallies and distances (scanq_cases.truth).  Plain numpy, no GPU.

Built on tests/scanq_cases.py (Case, truth, scripted, unscripted, shared_lists) and tests/survival_ref.py (scripted
survival, the edit scripts, the striped input).  What is new here is what the line walk adds to a scan: the tables -
every (target, slot) pair sorted by its neighbour well and cut into blocks of at most line_pairs pairs and 256 targets
(line_tables: the reference the library's make_line_tables, csrc/line_tables.inc, is held to, element by element) - and
with them targets whose pairs lie in several blocks, blocks that end inside a step of 128 pairs, local target 255,
slot 4094 of 4095.

A case names its line_pairs and the kernel both sides must report; the first round is 2, 3, 5, 6, 8 cycles for
k = 0, 1, 2, 3, >= 4 (wd_scan_async), 5 for Levenshtein <= 2, and one dword (4) or two (8) in the interleaved layout."""
from __future__ import annotations

import numpy as np

import scanq_cases as qc
import survival_ref as sr
from scanq_cases import FAMILIES, LAYOUTS, INVALID, truth, cuts_of            # noqa: F401  (the test modules' names)

K_LW_TARGETS, K_LW_PAIRS, K_LW_STEP, K_LW_QCAP, K_LW_IN_PLACE = sr.K_LW_TARGETS, sr.K_LW_PAIRS, sr.K_LW_STEP, sr.K_LW_QCAP, sr.K_LW_IN_PLACE
K_LW_MAX_SLOTS = 4095                         # a slot must fit the 12 bits the entry's tag leaves it beside the Levenshtein state
TAGS = ("split", "negdelta", "sharedword", "lastword", "bufend", "cut256", "slot4095", "notapply", "filters", "equal", "hitcap", "striped", "queue",
        "lastdrain", "short", "k254", "grid", "ties")


def first_round(fam, layout, k):
    """B1 as wd_scan_async and launch_lines_t (csrc/welldup_scan.hip, csrc/welldup_lines.hip) choose it."""
    if layout == "il":
        return 8 if fam == "lev2" else 4
    return 5 if fam == "lev2" else sr.auto_first(k)


def line_tables(centre, lvl_off, nbr, line_pairs):
    """The line walk's tables, or None where the walk does not apply (an empty ring, a target of more than 4095 slots, no
    pair): the pairs in (target, slot) order, a numpy stable argsort by neighbour well - equal wells stay in
    target-then-slot order -, then the greedy cut: a block takes pairs until it holds line_pairs of them or the next pair
    would bring its 257th target.  -> dict(pw int32 [P], pm uint32 [P] (target within the block << 16 | slot), blk int32
    [B, 4] {first pair, pairs, first entry of btgt, targets}, btgt uint32 (index in the file | owner << 31: the first
    block in block order that holds a pair of the target), bcen, boff [.., levels + 1], tmax)."""
    T = lvl_off.shape[0]
    sizes = (lvl_off[:, -1] - lvl_off[:, 0]).astype(np.int64)
    if (np.diff(lvl_off, axis=1) <= 0).any() or sizes.max() > K_LW_MAX_SLOTS or sizes.sum() < 1:
        return None
    tgt = np.repeat(np.arange(T), sizes)
    slot = np.concatenate([np.arange(s) for s in sizes])
    well = nbr[lvl_off[tgt, 0] + slot]
    order = np.argsort(well, kind="stable")
    well, tgt, slot = well[order], tgt[order], slot[order]
    P = well.shape[0]
    per_block = line_pairs or K_LW_PAIRS
    pm = np.zeros(P, dtype=np.uint32)
    blk, btgt, owned, first = [], [], set(), 0
    while first < P:
        local, i = {}, first
        while i < P and i - first < per_block:
            t = int(tgt[i])
            if t not in local:
                if len(local) == K_LW_TARGETS:
                    break
                local[t] = len(local)
            pm[i] = (local[t] << 16) | int(slot[i])
            i += 1
        blk.append((first, i - first, len(btgt), len(local)))
        for t in local:                                            # (in the order the block met them)
            btgt.append(t | (0 if t in owned else 1 << 31))
            owned.add(t)
        first = i
    blk = np.array(blk, dtype=np.int32)
    btgt = np.array(btgt, dtype=np.uint32)
    file_t = (btgt & 0x7FFFFFFF).astype(np.int64)
    return dict(pw=well.astype(np.int32), pm=pm, blk=blk, btgt=btgt, bcen=centre[file_t].astype(np.int32),
                boff=lvl_off[file_t].astype(np.int32), tmax=(int(blk[:, 3].max()) + 3) & ~3)


class Case(qc.Case):
    MAX_SLOTS = K_LW_MAX_SLOTS + 1            # (one more than the walk takes: the case where it does not apply)

    def __init__(self, name, fam, layout, k, L, levels, n, lists, tiles, line_pairs, per_target=True, hit_cap=1 << 14, tags=()):
        self.line_pairs = line_pairs
        assert line_pairs >= 1 and levels <= 8 and set(tags) <= set(TAGS), tags
        super().__init__(name, fam, layout, k, L, 1, levels, n, lists, tiles, per_target=per_target, hit_cap=hit_cap, tags=tags)
        self.tables = line_tables(self.centre, self.lvl_off, self.nbr, line_pairs)
        self.blocks = 0 if self.tables is None else int(self.tables["blk"].shape[0])
        if self.tables is None:
            self.kernel = None                # (whatever the dispatch falls back to: not k_scan_lines)

    def instantiation(self):
        B1 = first_round(self.fam, self.layout, self.kk)
        levh = -1 if self.fam == "lev2" else 0
        if self.layout == "il":
            return B1, "k_scan_lines<true, %d, %d, 4>" % (B1, levh)
        return B1, "k_scan_lines<%s, %d, %d>" % ("false" if self.layout == "ptr" else "true", B1, levh)

    def split_targets(self):
        """targets whose pairs lie in more than one block"""
        t = (self.tables["btgt"] & 0x7FFFFFFF).astype(np.int64)
        return int((np.bincount(t, minlength=self.T) > 1).sum())


def expectation(case):
    """The tables as the case file carries them (tools/scan_lines_emu.cpp: `extra`)."""
    tb = case.tables
    if tb is None:
        return np.zeros(1, dtype=np.int32)
    parts = [np.array([tb["blk"].shape[0], tb["tmax"], tb["btgt"].shape[0]], dtype=np.int32), tb["pw"], tb["pm"].view(np.int32),
             tb["blk"].reshape(-1), tb["btgt"].view(np.int32), tb["bcen"], tb["boff"].reshape(-1)]
    return np.concatenate([np.ascontiguousarray(p, dtype=np.int32) for p in parts])


def write_case(path, case):
    qc.write_case(path, case, line_pairs=case.line_pairs, extra=expectation(case))


# ---- reads -----------------------------------------------------------------------------------------------------------
def planted(rng, n, lists, L, plants, bad=(), tiles=1, bad_nbr=0.0):
    """Tiles of random reads in which neighbour `slot` of target t, for every (t, slot) of `plants`, is its centre's read
    with substitutions at the cycles plants[(t, slot)] (none: a copy).  bad: centres that fail the filter, per tile if a
    list of lists."""
    g = qc.Wells(n, lists)
    out = []
    for i in range(tiles):
        codes = sr.random_codes(rng, (n, L))
        for (t, slot), cycles in plants.items():
            r = codes[g.centre[t]].copy()
            for c in cycles:
                r[c] = (r[c] + rng.integers(1, 5)) % 5
            codes[lists[t][1][slot]] = r
        b = bad[i] if len(bad) and isinstance(bad[0], (list, tuple)) else bad
        s = sr.finish(rng, g, L, 0, codes, bad_centres=b, bad_nbr_frac=bad_nbr)
        out.append((s.planes, s.filt))
    return out


def random_lists(rng, n, Ks, levels, centres_from, wells_from, fixed=None):
    """Targets with centres drawn from the wells centres_from and neighbours from wells_from (shared between targets:
    ties); fixed: {t: [wells]} for the targets whose neighbours the caller chose."""
    fixed = fixed or {}
    centres = [int(v) for v in rng.choice(np.asarray(centres_from), size=len(Ks), replace=False)]
    lists = []
    for t, K in enumerate(Ks):
        wells = fixed[t] if t in fixed else [int(v) for v in rng.choice(np.setdiff1d(wells_from, [centres[t]]), size=K, replace=False)]
        assert len(wells) == K == len(set(wells)) and centres[t] not in wells
        lists.append((centres[t], list(wells), cuts_of(K, levels)))
    return lists


def _split_case(rng, levels, k, L, T=125, line_pairs=4):
    """Target A = 4m + 1 of `levels` rings whose only duplicates arrive, in block order, at levels 3, 5, 1, 7, 0 (8 rings:
    the first hit moves down twice, the last up twice), each in a block of its own; B = 4m with duplicates on the wells
    on both sides of A's (the same mask word in the same blocks), 4m + 2 without a duplicate, 4m + 3 filtered; Z = T - 1, split
    too, alone in the mask's last word (T = 125: 32 words, mask_stride's multiple).  With 8 rings a second pair, A2 = 4m2 + 1
    and B2 = 4m2, meets in twelve blocks, at the outermost levels in turn: every level of theirs is come back to (with
    one ring A and B do that themselves, in twelve blocks).  -> (n, lists, tiles, (A, B, F, Z))"""
    n, m, m2 = 4099, 10, 20
    A, B, F, Z, A2, B2 = 4 * m + 1, 4 * m, 4 * m + 3, T - 1, 4 * m2 + 1, 4 * m2
    ends = [(0, levels - 1)[i % 2] for i in range(12)]
    if levels == 8:
        script = [(A, 16, 500, [(i, 0) for i in range(5)], [3, 5, 1, 7, 0]),
                  (B, 16, 500, [(i, d) for i in range(5) for d in (-1, 1)], [2, 2, 6, 6, 0, 0, 4, 4, 1, 1]),
                  (A2, 48, 200, [(i, 50) for i in range(12)], ends),
                  (B2, 96, 200, [(i, 50 + d) for i in range(12) for d in (-1, 1)], [l for l in ends for _ in (0, 1)])]
    else:
        script = [(A, 24, 200, [(i, 0) for i in range(12)], [i % levels for i in range(12)]),
                  (B, 24, 200, [(i, d) for i in range(12) for d in (-1, 1)], [i % levels for i in range(12) for _ in (0, 1)])]
    script.append((Z, 16, 500, [(i, 7) for i in range(5)], [levels - 1, 0, levels // 2, 0, levels - 1]))
    Ks = [levels] * T
    reserved = set()
    fixed, plants = {}, {}
    free = iter(range(3300, 3600))                                 # wells nobody else is given
    # (B's duplicates lie on the wells on both sides of A's, two of one level: whatever the cut, one of them is in A's block)
    for t, big, step, places, order in script:
        Ks[t] = big
        cuts = cuts_of(big, levels)
        wells, used = [None] * big, {}
        for (i, d), l in zip(places, order):
            s = cuts[l] + used.get(l, 0)                           # the next slot of level l
            used[l] = used.get(l, 0) + 1
            assert s < cuts[l + 1]
            wells[s] = step * (i + 1) + d
            plants[(t, s)] = [L - 1] if (k >= 1 and i % 2 and L > 1) else []
        fixed[t] = [w if w is not None else next(free) for w in wells]
        reserved |= set(fixed[t])
    pool = np.setdiff1d(np.arange(3300), sorted(reserved))
    lists = random_lists(rng, n, Ks, levels, np.arange(3600, n), pool, fixed)
    return n, lists, planted(rng, n, lists, L, plants, bad=(F,)), (A, B, F, Z)


def _family_layout_cases(fam, layout):
    out = []
    seed = [77, FAMILIES.index(fam), LAYOUTS.index(layout)]
    lev2, il = fam == "lev2", layout == "il"
    k0 = 2 if lev2 else 1
    ks = (2,) * 5 if lev2 else (0, 1, 2, 3, 4)

    def add(name, *a, **kw):
        out.append(Case("lw_%s_%s_%s" % (fam, layout, name), fam, layout, *a, **kw))

    def rng_of(*extra):
        return np.random.default_rng(seed + list(extra))

    # ---- split targets
    rng = rng_of(1)
    n, lists, tiles, _ = _split_case(rng, 8, ks[1], 30)
    add("split8", ks[1], 30, 8, n, lists, tiles, 4, tags=("split", "negdelta", "sharedword", "lastword"))
    rng = rng_of(2)
    n, lists, tiles, _ = _split_case(rng, 1, ks[0], 22)
    add("split1", ks[0], 22, 1, n, lists, tiles, 4, tags=("split", "sharedword", "lastword"))
    rng = rng_of(3)
    lists = random_lists(rng, 700, [40, 4, 4, 4, 4], 2, np.arange(600, 700), np.arange(600))
    plants = {(0, s): ([] if s % 2 else [20][:min(ks[2], 1)]) for s in (0, 3, 19, 20, 21, 39)}
    add("split_line_pairs1", ks[2], 21, 2, 700, lists, planted(rng, 700, lists, 21, plants), 1, tags=("split", "negdelta"))

    # ---- blocks that end inside a step; a last block of one pair (pw's last entry); nbr's last entry is the last target's last slot
    for i, lp in enumerate((127, 129, 511, 513)):
        rng = rng_of(4, lp)
        P = 3 * lp + 1
        Ks = [P // 9 + (1 if t < P % 9 else 0) for t in range(9)]
        n = 2500 + 97 * i
        lists = qc.shared_lists(rng, n, Ks, 3)
        add("ends_in_step_%d" % lp, ks[i], 26, 3, n, lists, qc.unscripted(rng, n, lists, 26, "random", bad=(4,)), lp, tags=("bufend",))

    # ---- the cut at 256 targets: 600 targets of one or two slots on neighbouring wells; local target 255 in blocks 0 and 1
    rng = rng_of(5)
    T = 600
    Ks = [1 + (t % 3 == 0) for t in range(T)]
    lists = [(t, [1000 + 2 * t + j for j in range(Ks[t])], [0, Ks[t]]) for t in range(T)]
    plants = {(255, 0): [], (511, 0): [25][:min(k0, 1)], (256, 0): [], (599, 0): []}
    add("cut_at_256_targets", k0, 26, 1, 2300, lists, planted(rng, 2300, lists, 26, plants, bad=(254, 300)), 5000, tags=("cut256",))

    # ---- slot 4094 of 4095: the tag's low 24 bits are the slot and the Levenshtein state (the Hamming count above it)
    rng = rng_of(6)
    wells = [int(v) for v in rng.permutation(4098)[:4095]]
    lists = [(4098, wells, cuts_of(4095, 2))]
    late = [33][:min(k0, 1)]
    add("slot_4094", k0, 34, 2, 4099, lists, planted(rng, 4099, lists, 34, {(0, 0): late, (0, 4093): [], (0, 4094): late}), K_LW_PAIRS,
        tags=("slot4095",))
    if not il:                                                     # (interleaved, nothing else reads the layout: an error, not a fall-back)
        rng = rng_of(7)
        wells = [int(v) for v in rng.permutation(4098)[:4096]]
        lists = [(4098, wells, cuts_of(4096, 2))]
        add("slots_4096_not_the_walks", k0, 12, 2, 4099, lists, planted(rng, 4099, lists, 12, {(0, 4095): [], (0, 7): []}), K_LW_PAIRS,
            tags=("notapply",))

    # ---- filters: target 0's twelve neighbours are wells 0 .. 11 and nobody else's - with four pairs a block, blocks 0 .. 2
    # hold a filtered target alone, whose first pair is the idle well; target 1, filtered too, is split; tile 1 filters others
    rng = rng_of(8)
    lists = random_lists(rng, 900, [12, 12, 6, 6, 6, 6], 2, np.arange(800, 900), np.arange(12, 800), fixed={0: list(range(12))})
    plants = {(0, 3): [], (1, 2): [], (1, 11): [], (2, 0): [], (3, 5): []}
    add("filtered_blocks", ks[3], 24, 2, 900, lists, planted(rng, 900, lists, 24, plants, bad=[[0, 1], [3]], tiles=2), 4, tags=("filters", "split"))

    # ---- low diversity
    for K, cap in ((100, 100), (30, 1 << 14)):
        rng = rng_of(9, K)
        lists = qc.shared_lists(rng, 1031, [K] * 6, 2)
        add("equal_K%d" % K, k0, 29, 2, 1031, lists, qc.unscripted(rng, 1031, lists, 29, "equal", bad=(4,)), 513, hit_cap=cap,
            tags=("equal", "hitcap"))
    L = 37
    B1 = first_round(fam, layout, k0)
    rng = rng_of(10)
    g = sr.Geometry(12, 128, 4)
    n, lists, tiles = qc.scripted(rng, 12, 128, 4, L, k0, lambda r: sr.scripted_deaths(r, g, L, k0, B1, None, K_LW_IN_PLACE, K_LW_QCAP, striped=True),
                                  dead_first=B1 if lev2 else 0)
    add("striped_42_43", k0, L, 4, n, lists, tiles, 512, tags=("striped",))
    # 31 windows of 128 pairs in one block: wave w takes windows w, w + 4, ..  Wave 0 fills its queue to exactly kLwQCap and
    # drains before the next push, wave 1 would pass it by one (127 + 2), wave 2 drains at 117, wave 3 - the last: its
    # second buffer is the end of the LDS block - fills to kLwQCap, drains and ends with survivors that live through rounds
    counts, kinds = [0] * 32, ["rounds"] * 32
    for w, (cs, late) in enumerate((((32, 32, 32, 32, 30, 4, 32, 32), (6, 7)), ((32, 32, 32, 31, 2, 3, 32, 33), (6, 7)),
                                    ((39, 39, 39, 30, 38, 38, 38, 14), ()), ((38, 38, 38, 14, 10, 20, 30, 39), ()))):
        for i, c in enumerate(cs):
            counts[w + 4 * i] = c
            kinds[w + 4 * i] = "never" if i in late else "early" if late and i in (4, 5) else ("rounds" if i % 2 else "spread")
    rng = rng_of(11)
    n, lists, tiles = qc.scripted(rng, 31, 128, 1, L, k0, qc.survivors(31, 128, L, k0, B1, counts[:31], kinds[:31]), dead_first=B1 if lev2 else 0)
    add("queue_at_cap", k0, L, 1, n, lists, tiles, 4096, tags=("queue", "lastdrain"))

    # ---- short and ragged reads
    Ls = {}
    for k in ks:
        B1 = first_round(fam, layout, k)
        for L in (1, B1 - 1, B1, B1 + 1):
            Ls[(k, L)] = B1
    if il:
        for j, L in enumerate((1, 3, 4, 5, 7, 8, 9)):
            Ls[(ks[j % 5], L)] = first_round(fam, layout, ks[j % 5])
    if not lev2:
        Ls[(5, 4)] = first_round(fam, layout, 4)                  # k >= L: capped at L
        Ls[(40, 37)] = first_round(fam, layout, 37)
    for j, ((k, L), B1) in enumerate(sorted(Ls.items())):
        if L < 1 or (layout == "ptr" and L == 1) or (lev2 and L <= k):
            continue                                               # (what the launchers cannot launch: scanq_cases says why)
        rng = rng_of(12, j)
        n, lists, tiles = qc.scripted(rng, 5, 140, 2, L, k, qc.spread_deaths(5, 140, L, B1), flip=bool(j % 2), bad=(2,),
                                      edits=lev2 and L >= 3, tiles=2 if layout == "ptr" and L == 2 else 1)
        add("L%d_k%d" % (L, k), k, L, 2, n, lists, tiles, 300, tags=("short",))
    if not lev2:
        # 254 mismatches allowed in 300 cycles: a neighbour at exactly 254 and one at 255 (the tag's count stops at 255)
        rng = rng_of(13)
        lists = random_lists(rng, 257, [9, 9], 1, np.arange(250, 257), np.arange(250))
        plants = {(0, 2): [int(v) for v in rng.choice(300, size=254, replace=False)], (0, 5): [int(v) for v in rng.choice(300, size=255, replace=False)],
                  (1, 8): [int(v) for v in rng.choice(300, size=254, replace=False)], (1, 0): list(range(255))}
        add("k254_L300", 254, 300, 1, 257, lists, planted(rng, 257, lists, 300, plants), 7, tags=("k254",))

    # ---- the grid: one block on one tile; blocks x tiles = 7, 9, 17 (no multiple of the 8 XCDs); three tiles, three filters
    for i, (blocks, n_tiles) in enumerate(((1, 1), (7, 1), (3, 3), (17, 1), (1, 17))):
        rng = rng_of(14, i)
        lp = 40
        P = lp * blocks - 3
        Ks = [P // 3 + (1 if t < P % 3 else 0) for t in range(3)]
        n = 300 + 31 * i
        lists = qc.shared_lists(rng, n, Ks, 2)
        tiles = []
        for j in range(n_tiles):
            tiles += qc.unscripted(rng, n, lists, 19, "random", bad=((), (0,), (1, 2))[j % 3])
        add("grid%d_blocks%d_tiles%d" % (blocks * n_tiles, blocks, n_tiles), ks[i], 19, 2, n, lists, tiles, lp, tags=("grid",))

    # ---- ties: well 100 wanted by five targets at slots that differ; target 1's centre is target 0's neighbour; no per-target
    # counts and no hit log
    rng = rng_of(15)
    lists = random_lists(rng, 400, [7] * 6, 2, np.arange(300, 400), np.setdiff1d(np.arange(300), [100]))
    for t in range(5):
        lists[t][1][(2 * t + 1) % 7] = 100
    lists[0][1][0] = lists[1][0]
    plants = {(0, 0): [], (2, 5): []}
    add("ties", ks[2], 23, 2, 400, lists, planted(rng, 400, lists, 23, plants), 6, per_target=False, hit_cap=-1, tags=("ties", "split"))
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
