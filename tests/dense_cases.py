"""The cases of the dense chain (csrc/scan_dense.inc) that tests/test_dense_emu.py (the chain's source on the CPU: exact
buffers, the LDS-DMA model, shuffled schedules - tools/scan_dense_emu.cpp) and tests/test_gpu_dense_cases.py (the chain
on the GPU, through Scanner) hold to one truth: the CPU oracle's counts, tallies and distances (tests/scanq_cases.py:
truth).  Plain numpy, no GPU.

Also here: the reference of the dense path's device tables, written from the definitions in the comments of
k_transpose_nbr, k_dense_symcheck and k_dense_windows (tables_ref), with the properties a table has by definition
asserted on it (check_table_properties).  The emulator compares every element the kernels write with it.

A case file is tests/scanq_cases.py's (write_case) with `extra` = the options of the case, the constants it assumes and
the expected tables (extra_words)."""
from __future__ import annotations

import numpy as np

import scanq_cases as qc
import survival_ref as sr
from well_duplicates_amd import cluster_indexes, synth, workload

# the constants the cases assume (tests/test_dense_emu.py compares them with the source)
K_WAVE = 64
K_SIG_CYCLES, K_SCREEN_CYCLES, K_MAX_SEG, K_WIN_MAX_K, K_WIN_GAP, K_WIN_DWORDS, K_MARK_BLOCK = 10, 16, 16, 128, 24, 1024, 256
K_WIN_BUFS, K_WIN_BUFS_SYM, K_ROW_GROUPS, K_ROW_CYCLES = 2, 3, 4, 160
CONSTANTS = (K_SIG_CYCLES, K_MAX_SEG, K_WIN_MAX_K, K_WIN_GAP, K_WIN_DWORDS, K_MARK_BLOCK, K_WIN_BUFS, K_WIN_BUFS_SYM)
MAGIC = 0x31534E44
OPTION_DEFAULTS = dict(dense_sym=1, dense_windows=1, dense_pack=-1, dense_queue_cap=0, dense_tile_chunk=16, dense_nt=1,
                       dense_overlap=0, dense_part_tiles=0, dense_pack_blocks=1024)
OPTION_ORDER = ("dense_sym", "dense_windows", "dense_pack", "dense_queue_cap", "dense_tile_chunk", "dense_nt", "dense_overlap",
                "dense_part_tiles", "dense_pack_blocks")
# (behind the options in a case file: misalign - a pointer table whose planes lie 1 to 3 bytes off alignment)


# ---- the tables, from their definitions ------------------------------------------------------------------------------
def kpad_of(k_max):
    kpad = min(K_WIN_MAX_K, (2 * k_max + 8 + 31) & ~31)
    return kpad if 1 <= k_max <= kpad else 0


def _window_group(g, centre, lvl_off, nbr, T, levels, kpad, half):
    """k_dense_windows for group g -> None (the group keeps the gathers) or its tables."""
    lanes = range(g * K_WAVE, min(T, (g + 1) * K_WAVE))
    c0 = int(centre[g * K_WAVE])
    if any(int(centre[t]) != c0 + (t - g * K_WAVE) for t in lanes):
        return None                                           # centres not consecutive
    lists = []                                                # per lane: [(ring, offset)] in slot order
    for t in lanes:
        o = lvl_off[t]
        lst = []
        for q in range(int(o[levels] - o[0])):
            lev = sum(1 for l in range(1, levels) if o[0] + q >= o[l])
            lst.append((lev, int(nbr[o[0] + q]) - int(centre[t])))
        lists.append(lst)
    union = sorted({e for lst in lists for e in lst})         # (ring, offset) order
    if not union or len(union) > kpad:
        return None
    place = {e: u for u, e in enumerate(union)}
    mask = np.zeros((kpad // 32, K_WAVE), dtype=np.uint32)
    for i, lst in enumerate(lists):
        us = [place[e] for e in lst]
        if any(b <= a for a, b in zip(us, us[1:])):
            return None                                       # a ring out of order, or a well listed twice
        for u in us:
            mask[u >> 5, i] |= np.uint32(1 << (u & 31))
    walked = [(u, e) for u, e in enumerate(union) if not half or e[1] > 0]
    n_el = len(walked)
    if n_el == 0 or (half and n_el >= kpad):
        return None
    if half:
        walked.append((0, (0, 0)))                            # the centres' own signatures
    sd = [e[1] for _, e in walked]
    n = len(sd)
    start = [not any((v < sd[p] and sd[p] - v <= K_WIN_GAP) or (v == sd[p] and f < p) for f, v in enumerate(sd)) for p in range(n)]
    starts = sorted(sd[p] for p in range(n) if start[p])
    lo = [max(s for s in starts if s <= sd[p]) for p in range(n)]
    runs, base = [], 0
    for s in starts:
        hi = max(sd[p] for p in range(n) if lo[p] == s)
        runs.append((s, base, K_WAVE + hi - s))
        base += K_WAVE + hi - s
    if len(runs) > K_MAX_SEG or base > K_WIN_DWORDS:
        return None
    run_base = {s: b for s, b, _ in runs}
    uoff = np.zeros(kpad, dtype=np.int64)
    wdelta, wlev, wfull = np.zeros(kpad, dtype=np.int64), np.zeros(kpad, dtype=np.int64), np.zeros(kpad, dtype=np.int64)
    for p, (u, (lev, d)) in enumerate(walked):
        uoff[p] = 4 * (run_base[lo[p]] + d - lo[p])
        wdelta[p], wlev[p], wfull[p] = d, lev, u
    return dict(ginfo=n_el | (len(runs) << 9) | (base << 14), useg=[(s, b | (ln << 16)) for s, b, ln in runs], uoff=uoff, wdelta=wdelta,
                wlev=wlev, wfull=wfull, wmask=mask, total=base, n_el=n_el, n=n, union=union, lists=lists, c0=c0)


def tables_ref(centre, lvl_off, nbr, levels, sym_option=1):
    """The dense path's tables for a targets set, by their definitions."""
    T = centre.shape[0]
    groups = (T + K_WAVE - 1) // K_WAVE
    K = (lvl_off[:, levels] - lvl_off[:, 0]).astype(np.int64)
    gbase = np.zeros(groups + 1, dtype=np.int64)
    for g in range(groups):
        gbase[g + 1] = gbase[g] + K_WAVE * max(1, int(K[g * K_WAVE:(g + 1) * K_WAVE].max()))
    total = int(gbase[-1])
    # the q-th neighbour of a group's lanes, the centre itself behind a lane's last; lanes past the last target: centre 0
    wells = np.zeros(total, dtype=np.int64)
    cen = np.zeros(total, dtype=np.int64)
    udelta = np.zeros(total // K_WAVE, dtype=np.int64)
    guni = np.zeros(groups, dtype=np.int64)
    for g in range(groups):
        kmax = int(gbase[g + 1] - gbase[g]) // K_WAVE
        lanes = np.arange(g * K_WAVE, (g + 1) * K_WAVE)
        inn = lanes < T
        tt = np.minimum(lanes, T - 1)
        c = np.where(inn, centre[tt], 0).astype(np.int64)
        uniform = bool(inn.all() and (np.diff(c) == 1).all())
        for q in range(kmax):
            have = inn & (q < K[tt])
            w = np.where(have, nbr[np.minimum(lvl_off[tt, 0] + q, nbr.shape[0] - 1)], c)
            at = int(gbase[g]) + q * K_WAVE
            wells[at:at + K_WAVE], cen[at:at + K_WAVE] = w, c
            same = bool(have.all() and ((w - c) == (w - c)[0]).all())
            udelta[int(gbase[g]) // K_WAVE + q] = (w - c)[0] if same else 0
            uniform = uniform and same
        guni[g] = int(uniform)
    idx16 = bool((np.abs(wells - cen) <= 32767).all())
    nbr_t = (wells - cen) if idx16 else wells
    rel_t = (lvl_off[:, 1:] - lvl_off[:, :1]).T.reshape(-1).astype(np.int64)
    # the symmetric verdict
    sym_on = False
    if sym_option and T >= 2:
        c0 = int(centre[0])
        sym_on = bool((centre == c0 + np.arange(T)).all())
        rings = {}
        for t in range(T if sym_on else 0):
            for l in range(levels):
                r = nbr[lvl_off[t, l]:lvl_off[t, l + 1]].astype(np.int64)
                rings[t, l] = r
                if r.size == 0 or (np.diff(r) <= 0).any() or (r == centre[t]).any() or (r < c0).any() or (r >= c0 + T).any():
                    sym_on = False
        for (t, l), r in rings.items() if sym_on else ():
            for w in r:
                if int(centre[t]) not in rings[int(w) - c0, l]:
                    sym_on = False
    kpad = kpad_of(int(K.max()))
    wins = [None] * groups
    if kpad:
        wins = [_window_group(g, centre, lvl_off, nbr, T, levels, kpad, sym_on) for g in range(groups)]
    ginfo = np.array([w["ginfo"] if w else 0 for w in wins], dtype=np.int64)
    win_max = max([w["total"] for w in wins if w] + [0])
    return dict(T=T, levels=levels, groups=groups, total=total, gbase=gbase, guni=guni, ginfo=ginfo, nbr_t=nbr_t, udelta=udelta, rel_t=rel_t,
                idx16=idx16, sym_on=sym_on, kpad=kpad, win_max=win_max, wins=wins,
                window_groups=int((ginfo != 0).sum()), uniform_groups=int(guni.sum()),
                window_dwords=(win_max + K_WAVE - 1) // K_WAVE * K_WAVE)


def check_table_properties(tb, centre, lvl_off, nbr):
    """What the window tables are by definition, whatever the reference's own arithmetic thinks."""
    T, levels, kpad = tb["T"], tb["levels"], tb["kpad"]
    for g, w in enumerate(tb["wins"]):
        if not w:
            continue
        n_el, nrun, total = w["ginfo"] & 0x1FF, (w["ginfo"] >> 9) & 31, w["ginfo"] >> 14
        assert 1 <= n_el <= kpad and 1 <= nrun <= K_MAX_SEG and 64 <= total <= K_WIN_DWORDS and total == w["total"]
        # useg: ascending, back to back, lengths 64 + hi - lo, split exactly where two offsets are more than kWinGap apart
        offs = sorted(set(int(d) for d in w["wdelta"][:w["n"]]))
        cuts = [offs[0]] + [b for a, b in zip(offs, offs[1:]) if b - a > K_WIN_GAP]
        assert [s for s, _ in w["useg"]] == cuts, (g, w["useg"], cuts)
        at = 0
        for i, (s, word) in enumerate(w["useg"]):
            hi = max(d for d in offs if d >= s and (i + 1 == len(cuts) or d < cuts[i + 1]))
            assert (word & 0xFFFF, word >> 16) == (at, K_WAVE + hi - s)
            at += K_WAVE + hi - s
        assert at == total
        # uoff: every lane's dword of every element inside the window, and the source of that dword the element's well
        for p in range(w["n"]):
            assert w["uoff"][p] % 4 == 0 and 0 <= w["uoff"][p] // 4 and w["uoff"][p] // 4 + 63 < total
            run = max(i for i, (s, word) in enumerate(w["useg"]) if (word & 0xFFFF) <= w["uoff"][p] // 4)
            s, word = w["useg"][run]
            assert s + (w["uoff"][p] // 4 - (word & 0xFFFF)) == w["wdelta"][p]
        # wdelta / wlev: in (ring, offset) order; wfull: the place in the whole union
        walked = [(int(w["wlev"][p]), int(w["wdelta"][p])) for p in range(n_el)]
        assert walked == sorted(walked) and [w["union"][int(w["wfull"][p])] for p in range(n_el)] == walked
        assert (w["uoff"][w["n"]:] == 0).all() and (w["wdelta"][w["n"]:] == 0).all()
        # wmask: a lane's slot of an element equals the number of its members below it
        for i, lst in enumerate(w["lists"]):
            bits = [u for u in range(len(w["union"])) if (int(w["wmask"][u >> 5, i]) >> (u & 31)) & 1]
            assert [w["union"][u] for u in bits] == lst, (g, i)
        assert (w["wmask"][:, len(w["lists"]):] == 0).all()
    assert tb["win_max"] == max([w["total"] for w in tb["wins"] if w] + [0])


def extra_words(case):
    tb = case.tables()
    words = [MAGIC] + [case.options[name] for name in OPTION_ORDER] + [int(case.misalign)] + list(CONSTANTS) + \
        [int(tb["idx16"]), int(tb["sym_on"]), tb["kpad"], tb["win_max"], tb["groups"], tb["total"]]
    parts = [np.array(words, dtype=np.int64), tb["gbase"], tb["guni"], tb["ginfo"], tb["nbr_t"], tb["udelta"], tb["rel_t"]]
    for w in tb["wins"]:
        if w:
            parts += [np.array(w["useg"], dtype=np.int64).reshape(-1), w["uoff"], w["wdelta"], w["wlev"], w["wfull"],
                      w["wmask"].astype(np.int64).reshape(-1)]
    out = np.concatenate([np.asarray(p, dtype=np.int64).reshape(-1) for p in parts])
    return (out & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


# ---- a case ----------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, fam, k, L, levels, n, csr, tiles, layout="plane", per_target=True, hit_cap=1 << 20, check_empty=False,
                 tags=(), expect=(), misalign=False, **options):
        self.name, self.fam, self.k, self.kk, self.L, self.levels, self.n = name, fam, k, min(k, L), L, levels, n
        self.mode = 2 if fam == "lev2" else (0 if k == 0 else 1)
        self.layout, self.per_target, self.hit_cap = layout, per_target, hit_cap
        self.tags, self.expect, self.misalign = set(tags), tuple(expect), misalign
        assert not misalign or layout == "ptr"
        self.options = dict(OPTION_DEFAULTS)
        assert set(options) <= set(OPTION_DEFAULTS), options
        self.options.update(options)
        self.centre, self.lvl_off, self.nbr = (np.ascontiguousarray(a, dtype=np.int32) for a in csr)
        self.T, self.tiles = self.centre.shape[0], tiles
        self.tpb, self.B1, self.sort, self.queue_first = 1, 0, False, 0
        self._tables = None
        assert all(f.shape[0] == n and len(p) == L for p, f in tiles) and self.nbr.min() >= 0 and self.nbr.max() < n
        assert not (layout == "ptr" and L == 1)               # (one plane per tile is a stride to the host)
        # (wd_set_targets notes an empty ring itself, and the scan then checks for it: no case has one by accident)
        self.check_empty = bool((np.diff(self.lvl_off, axis=1) <= 0).any())
        assert self.check_empty == check_empty, name

    def csr(self):
        return self.centre, self.lvl_off, self.nbr

    def view(self):
        return self.centre, self.lvl_off, None

    def tables(self):
        if self._tables is None:
            self._tables = tables_ref(self.centre, self.lvl_off, self.nbr, self.levels, self.options["dense_sym"])
            check_table_properties(self._tables, self.centre, self.lvl_off, self.nbr)
        return self._tables


def write_case(path, case):
    qc.write_case(path, case, extra=extra_words(case))


# ---- geometry --------------------------------------------------------------------------------------------------------
def honeycomb_csr(rows, cols, levels):
    """Every well of a rows x cols honeycomb a centre (synth.honeycomb_pixels, cluster_indexes.generate)."""
    x, y = synth.honeycomb_pixels(rows, cols)
    return rows * cols, workload.targets_to_csr(cluster_indexes.generate(x, y, list(range(rows * cols)), levels))


def comb_csr(n, rings, centres=None, keep=lambda c, d, l: True, order=None):
    """Centre c has in ring l the wells c + d, d in rings[l], that lie in the tile (and that `keep` keeps), ascending -
    or in the order `order(c, l, wells)` gives.  centres: default every well."""
    centres = list(range(n)) if centres is None else list(centres)
    off, nb = [], []
    for c in centres:
        row = [len(nb)]
        for l, ds in enumerate(rings):
            wells = sorted(c + d for d in ds if 0 <= c + d < n and d != 0 and keep(c, d, l))
            if order:
                wells = order(c, l, wells)
            nb += wells
            row.append(len(nb))
        off.append(row)
    return np.array(centres), np.array(off), np.array(nb)


def sym(ds):
    return sorted(set(ds) | {-d for d in ds})


# ---- reads -----------------------------------------------------------------------------------------------------------
def make_tiles(rng, n, L, csr, tiles=1, kind="random", pf="mixed", nocall=True, plant=0.3, lev=False):
    """Random reads with planted copies of a neighbour (0 to 3 substitutions, for lev an insertion or a deletion too) and
    of a far well; every read equal; reads of two letters.  -> [(planes, filt)]"""
    centre, lvl_off, nbr = csr
    out = []
    for _ in range(tiles):
        if kind == "equal":
            codes = np.repeat(sr.random_codes(rng, (1, L)), n, axis=0)
        elif kind == "two":
            codes = (rng.integers(0, 2, size=(n, L)) * 2 + 1).astype(np.int8)     # (A and G; survival_ref's codes: 0 = no-call, 1..4)
        else:
            codes = sr.random_codes(rng, (n, L))
            if not nocall:
                codes[codes == 0] = 1
            for t in rng.permutation(centre.shape[0])[:int(plant * centre.shape[0])]:
                K = int(lvl_off[t, -1] - lvl_off[t, 0])
                if K == 0:
                    continue
                src = int(nbr[lvl_off[t, 0] + rng.integers(0, K)]) if rng.random() < 0.8 else int(rng.integers(0, n))
                r = codes[src].copy()
                if lev and L > 3 and rng.random() < 0.5:
                    at = int(rng.integers(0, L - 1))
                    r = np.concatenate([r[:at], r[at + 1:], [rng.integers(1, 5)]]) if rng.random() < 0.5 else \
                        np.concatenate([r[:at], [rng.integers(1, 5)], r[at:-1]])
                for _s in range(int(rng.integers(0, 4))):
                    r[rng.integers(0, L)] = rng.integers(0 if nocall else 1, 5)
                codes[int(centre[t])] = r
        b = sr.codes_to_bytes(rng, codes.astype(np.int8))
        filt = (rng.integers(0, 128, size=n) * 2).astype(np.uint8)
        filt |= {"all": 1, "none": 0}.get(pf, (rng.random(n) < 0.85).astype(np.uint8))
        out.append(([np.ascontiguousarray(b[:, c]) for c in range(L)], filt))
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------
_cases = []


def _build():
    out = []

    def add(name, fam, k, L, levels, n, csr, seed, layout="plane", tiles=1, kind="random", pf="mixed", nocall=True, **kw):
        rng = np.random.default_rng([77, seed])
        out.append(Case(name, fam, k, L, levels, n, csr, make_tiles(rng, n, L, csr, tiles, kind, pf, nocall, lev=fam == "lev2"),
                        layout=layout, **kw))

    # -- grids: every well a centre.  Wide (rows of 200: most groups window groups), narrow (rows of 60: every group
    # straddles a row end); the levels pick the window size and with it the pieces per window (NPC 4, 5, 6; 8 comes with a crafted comb below)
    wide = {lv: honeycomb_csr(5, 200, lv) for lv in (1, 3, 4, 5)}
    for i, (fam, k, lv, L, npc) in enumerate((("ham", 0, 1, 41, 4), ("ham", 2, 3, 42, 5), ("lev2", 2, 4, 43, 6), ("ham", 1, 5, 17, 6),
                                              ("lev2", 2, 1, 16, 4), ("ham", 0, 3, 150, 5))):
        n, csr = wide[lv]
        mode = 2 if fam == "lev2" else (0 if k == 0 else 1)
        add("wide_%s%d_lv%d_L%d" % (fam, k, lv, L), fam, k, L, lv, n, csr, 100 + i, tiles=3 if i < 4 else 1, dense_tile_chunk=(16, 2, 3, 1, 16, 16)[i],
            tags=("grid", "win"), expect=("k_dense_pairs_win<%d, true, %d>" % (mode, npc),))
    # ... and the other (mode, pieces) pairs of the fixed-piece kernel on the same grids, one tile each
    for i, (fam, k, lv, npc) in enumerate((("lev2", 2, 3, 5), ("ham", 0, 4, 6), ("ham", 1, 4, 6))):
        n, csr = wide[lv]
        mode = 2 if fam == "lev2" else (0 if k == 0 else 1)
        add("wide_more_%s%d_lv%d" % (fam, k, lv), fam, k, 19, lv, n, csr, 106 + i, tiles=2, tags=("grid", "win"),
            expect=("k_dense_pairs_win<%d, true, %d>" % (mode, npc),))
    n, csr = honeycomb_csr(17, 60, 2)
    add("narrow_ham1_L15", "ham", 1, 15, 2, n, csr, 110, layout="ptr", tiles=2, tags=("grid", "straddle"))
    n, csr = honeycomb_csr(17, 60, 2)
    add("narrow_lev2_L11", "lev2", 2, 11, 2, n, csr, 111, dense_sym=0, tiles=3, dense_tile_chunk=3, tags=("grid", "straddle", "twoended"),
        expect=("k_dense_pairs_win<2, false, 0>",))
    # -- N % 64 != 0 with N % 4 = 1, 2, 3: a partial last group, the dword / byte tail (pointer table: aligned planes),
    # plane bases 1 to 3 bytes off alignment (strided planes)
    comb = [sym([1, 2]), sym([70, 71, 140])]
    for i, (n, layout, fam, k, L) in enumerate(((453, "ptr", "ham", 1, 9), (454, "plane", "ham", 2, 10), (455, "ptr", "lev2", 2, 17),
                                                (453, "plane", "lev2", 2, 42), (458, "plane", "ham", 0, 11), (455, "ptr", "ham", 2, 43),
                                                (454, "ptr", "lev2", 2, 20))):
        add("tail_n%d_%s_%s%d_L%d" % (n, layout, fam, k, L), fam, k, L, 2, n, comb_csr(n, comb), 120 + i, layout=layout, tiles=2,
            dense_pack=(1, -1, -1, 1, 0, 1, -1)[i], dense_nt=i % 2, misalign=i >= 5, tags=("tail",))
    # -- the tile pipeline: n_tl = 1, 2, 3, 4 and 16 + 3 against the windows in flight; tc odd and even
    n, csr = 320, comb_csr(320, [sym([1, 3]), sym([30, 64])])
    for i, (tiles, tc, fam, k) in enumerate(((1, 16, "ham", 1), (2, 16, "ham", 0), (3, 3, "lev2", 2), (4, 4, "ham", 2), (19, 16, "ham", 1), (5, 2, "ham", 1))):
        add("pipe_tiles%d_tc%d_%s%d" % (tiles, tc, fam, k), fam, k, 12, 2, n, csr, 130 + i, tiles=tiles, dense_tile_chunk=tc,
            hit_cap=(1 << 20, 40, -1)[i % 3], tags=("pipe", "win"))
    # -- three windows without a fixed piece count (a window of more than 8 pieces), and two: forced through tile_chunk
    # and dense_queue_cap, so that the LDS bound in the host's choice decides
    n, csr = 900, comb_csr(900, [sym([1]), sym([100 * j for j in range(1, 7)])])
    add("npc8", "ham", 2, 13, 2, n, csr, 139, tiles=3, tags=("win",), expect=("k_dense_pairs_win<1, true, 8>",))
    add("npc8_eq", "ham", 0, 13, 2, n, csr, 137, tiles=4, tags=("win",), expect=("k_dense_pairs_win<0, true, 8>",))
    add("npc8_lev2", "lev2", 2, 13, 2, n, csr, 138, tiles=2, tags=("win",), expect=("k_dense_pairs_win<2, true, 8>",))
    far = [sym([1]), sym([100 * j for j in range(1, 9)])]
    n, csr = 1100, comb_csr(1100, far)
    add("bigwin_three", "ham", 1, 13, 2, n, csr, 140, tiles=5, dense_tile_chunk=5, dense_queue_cap=3, tags=("win", "bufs3"),
        expect=("k_dense_pairs_win<1, true, 0>",))
    add("bigwin_two", "ham", 1, 13, 2, n, csr, 141, tiles=4, dense_tile_chunk=4, dense_queue_cap=64, tags=("win", "bufs2"),
        expect=("k_dense_pairs_win<1, true, 0>",))
    add("bigwin_lev2", "lev2", 2, 20, 2, n, csr, 142, tiles=2, dense_tile_chunk=2, tags=("win",), expect=("k_dense_pairs_win<2, true, 0>",))
    add("bigwin_eq", "ham", 0, 20, 2, n, csr, 143, tiles=2, layout="ptr", tags=("win",), expect=("k_dense_pairs_win<0, true, 0>",))
    # -- gather groups: windows off; asymmetric rings (two-ended); the int32 table (offsets beyond +-32767); centres not
    # consecutive; a ring out of order; a well listed twice
    n, csr = 400, comb_csr(400, [sym([1, 2]), sym([17, 40])])
    for i, (fam, k) in enumerate((("ham", 0), ("ham", 2), ("lev2", 2))):
        add("gather_sym_%s%d" % (fam, k), fam, k, 18, 2, n, csr, 150 + i, dense_windows=0, tiles=(2, 3, 5)[i], dense_tile_chunk=(2, 3, 4)[i],
            tags=("gather",),
            expect=("k_dense_pairs<%d, true, true>" % (2 if fam == "lev2" else (0 if k == 0 else 1)),))
    n, csr = 400, comb_csr(400, [[-2, 1], [-40, 17, 33]])
    for i, (fam, k) in enumerate((("ham", 0), ("ham", 1), ("lev2", 2))):
        mode = 2 if fam == "lev2" else (0 if k == 0 else 1)
        add("asym_%s%d" % (fam, k), fam, k, 16, 2, n, csr, 160 + i, dense_windows=i % 2, tiles=(4, 3, 2)[i], dense_tile_chunk=(4, 3, 16)[i],
            hit_cap=(1 << 20, 30, 1 << 20)[i], tags=("twoended",),
            expect=("k_dense_pairs<%d, true, false>" % mode,) if i % 2 == 0 else ("k_dense_pairs_win<%d, false, 0>" % mode,))
    n = 33100
    csr = comb_csr(n, [sym([1]), sym([32768])], centres=range(100, 240))
    add("wide_offsets_int32_win", "ham", 1, 12, 2, n, csr, 170, tiles=4, dense_tile_chunk=3, tags=("int32", "win", "twoended"),
        expect=("k_dense_pairs_win<1, false, 0>",))
    for i, (fam, k) in enumerate((("ham", 0), ("ham", 1), ("lev2", 2))):
        add("wide_offsets_int32_%s%d" % (fam, k), fam, k, 12, 2, n, csr, 176 + i, dense_windows=0, tiles=(2, 3, 5)[i], dense_tile_chunk=(16, 3, 2)[i],
            tags=("int32", "gather"),
            expect=("k_dense_pairs<%d, false, false>" % (2 if fam == "lev2" else (0 if k == 0 else 1)),))
    csr = comb_csr(n, [sym([1]), sym([32767])], centres=range(100, 240))
    add("wide_offsets_int16", "lev2", 2, 12, 2, n, csr, 171, tiles=2, tags=("int16edge",))
    # a symmetric relation with offsets beyond +-32767, every well a centre (one level: ring {+-1, +-32768} is empty for
    # nobody): the int32 table under the one-ended compare, windows off
    n = 32900
    csr = comb_csr(n, [sym([1, 32768])])
    for i, (fam, k) in enumerate((("ham", 0), ("ham", 1), ("lev2", 2))):
        add("sym_int32_%s%d" % (fam, k), fam, k, 12, 1, n, csr, 190 + i, dense_windows=0, tiles=(1, 2, 1)[i], tags=("int32", "gather", "symint32"),
            expect=("k_dense_pairs<%d, false, true>" % (2 if fam == "lev2" else (0 if k == 0 else 1)),))
    n, csr = 500, comb_csr(500, [sym([1, 2]), sym([9])], centres=[c for c in range(500) if c % 7])
    add("centres_not_consecutive", "ham", 1, 14, 2, n, csr, 172, tiles=3, dense_tile_chunk=2, tags=("gatheronly",))
    n, csr = 300, comb_csr(300, [sym([1, 2]), sym([9, 11])], order=lambda c, l, w: w[::-1] if c == 100 and l == 1 else w)
    add("ring_out_of_order", "ham", 1, 14, 2, n, csr, 173, tiles=3, tags=("unordered",))
    n, csr = 300, comb_csr(300, [sym([1, 2]), sym([9, 11])], order=lambda c, l, w: w + w[-1:] if c == 200 and l == 0 else w)
    add("well_listed_twice", "ham", 0, 14, 2, n, csr, 174, tiles=2, tags=("unordered",))
    # the same offset in two rings (alternate centres see +-5 in ring 0 or in ring 1)
    n, csr = 300, comb_csr(300, [sym([1, 5]), sym([5, 9])], keep=lambda c, d, l: abs(d) != 5 or (c + min(d, 0)) % 2 == l)
    add("offset_in_two_rings", "ham", 1, 14, 2, n, csr, 175, tags=("win",))
    # -- table limits on crafted CSRs with consecutive centres: runs split at kWinGap / kWinGap + 1; kMaxSeg and
    # kMaxSeg + 1 runs; a union of exactly kpad and kpad + 1 elements (kpad 32); a window of kWinDwords and one more
    n = 2400
    add("gap_24_25", "ham", 1, 12, 2, n, comb_csr(n, [[1, 1 + K_WIN_GAP], [60, 60 + K_WIN_GAP + 1]], centres=range(0, 640)), 180, tags=("limits", "win"))
    runs16 = [[1], [100 * j for j in range(1, K_MAX_SEG)]]
    add("runs_16", "ham", 1, 12, 2, n, comb_csr(n, runs16, centres=range(0, 640)), 181, tags=("limits", "win"))
    add("runs_17", "ham", 1, 12, 2, n, comb_csr(n, [[1], [100 * j for j in range(1, K_MAX_SEG + 1)]], centres=range(0, 640)), 182,
        tags=("limits", "gatheronly"))
    # a union of exactly kpad and kpad + 1 elements, for the kpad values 32, 64, 96, 128 (k_max K -> kpad): every lane has
    # K - s offsets all lanes share and s of m more, in turn, so that the union has K - s + m elements
    for kpad, K, sp in ((32, 8, 1), (64, 16, 1), (96, 32, 2), (128, 48, 4)):
        assert kpad_of(K) == kpad
        for extra in (0, 1):
            m = kpad + extra - (K - sp)
            shared = list(range(1, K - sp + 1))
            csr = comb_csr(n, [shared[:2], shared[2:] + list(range(200, 200 + m))], centres=range(0, 128),
                           keep=lambda c, d, l, m=m, sp=sp: d < 200 or (d - 200 - sp * (c % 64)) % m < sp)
            add("union_%d_of_%d" % (kpad + extra, kpad), "ham", 1, 12, 2, n, csr, 300 + kpad + extra,
                tags=("limits",) + (("gatheronly",) if extra else ("win", "fullunion")))
    # one-ended (a symmetric relation, every well a centre) with kpad - 1 and kpad elements above the centres, kpad = 32.
    # A symmetric group's whole union is usually twice what lies above its centres and must itself fit kpad, so the limit
    # is met in the FIRST group alone: every offset is 70 or more, and the wells 0 .. 63 are nobody's upper well.  Every
    # well c is the lower well of the pairs (c, c + s), s in `shared`, and (c, c + 100 + c % 29) - which makes it the upper
    # well of exactly one such pair (29 is odd): at most 2 |shared| + 2 <= 12 neighbours a well, |shared| + 29 offsets
    # above the first group's centres
    for shared in ((70, 80), (70, 80, 90)):
        nn = 640
        lists = {c: set() for c in range(nn)}
        for c in range(nn):
            for w in [c + d for d in shared] + [c + 100 + c % 29]:
                if w < nn:
                    lists[c].add(w)
                    lists[w].add(c)
        off, nb = [], []
        for c in range(nn):
            row = [len(nb)]
            for near in (True, False):
                nb += sorted(w for w in lists[c] if (abs(w - c) in shared) == near)
                row.append(len(nb))
            off.append(row)
        csr = (np.arange(nn), np.array(off), np.array(nb))
        assert kpad_of(max(r[2] - r[0] for r in off)) == 32
        add("one_ended_%d_of_32" % (len(shared) + 29), "ham", 1, 12, 2, nn, csr, 310 + len(shared), tiles=2,
            tags=("limits", "oneended%d" % (len(shared) + 29)))
    # a window of exactly kWinDwords dwords (one run of offsets 1 .. 961: 64 + 960) and one more
    for i, span in enumerate((K_WIN_DWORDS - K_WAVE + 1, K_WIN_DWORDS - K_WAVE + 2)):
        ds = list(range(1, span + 1, K_WIN_GAP)) + [span]
        csr = comb_csr(n, [ds[:2], sorted(set(ds[2:]))], centres=range(0, 128))
        add("window_%d_dwords" % (K_WAVE + span - 1), "ham", 0, 12, 2, n, csr, 186 + i, tags=("limits",) + (("gatheronly",) if i else ("win",)))
    # -- reads: the edges of kSigCycles, kScreenCycles and of a 32-cycle row group; the largest L the rows hold and one above
    n, csr = 384, comb_csr(384, [sym([1, 2]), sym([20, 21])])
    # (launch_dense keeps rows for L <= K_ROW_CYCLES, and Levenshtein <= 2 beyond that length is not the dense path's)
    for i, (L, fam, k) in enumerate(((1, "ham", 1), (9, "lev2", 2), (10, "ham", 2), (11, "ham", 0), (15, "ham", 1), (16, "lev2", 2), (17, "ham", 2),
                                     (41, "lev2", 2), (42, "ham", 1), (43, "lev2", 2), (150, "ham", 2), (150, "lev2", 2), (K_ROW_CYCLES, "lev2", 2),
                                     (K_ROW_CYCLES, "ham", 1), (K_ROW_CYCLES + 1, "ham", 2))):
        add("reads_L%d_%s%d" % (L, fam, k), fam, k, L, 2, n, csr, 200 + i, dense_pack=(1, -1)[i % 2], tags=("reads",))
    add("reads_equal_ham", "ham", 1, 40, 2, n, csr, 220, kind="equal", pf="all", tags=("equal", "overflow"), dense_pack=1)
    add("reads_equal_eq_cap", "ham", 0, 12, 2, n, csr, 221, kind="equal", hit_cap=100, tags=("equal", "overflow", "hitcap"))
    add("reads_equal_lev2", "lev2", 2, 40, 2, n, csr, 222, kind="equal", tags=("equal", "overflow", "levover"))
    add("reads_equal_lev2_gather", "lev2", 2, 40, 2, n, csr, 223, kind="equal", dense_windows=0, tags=("equal", "overflow", "levover"))
    add("reads_equal_ham_gather", "ham", 2, 30, 2, n, csr, 224, kind="equal", dense_windows=0, dense_sym=0, tags=("equal", "overflow"))
    add("reads_two_letters", "ham", 2, 12, 2, n, csr, 225, kind="two", pf="all", dense_queue_cap=3, tags=("overflow",))
    # -- queues: n_q exactly q_per and q_per + 1 come with the caps 1, 3 and 64 on planted reads; dense_pack -1, 0, 1
    for i, (cap, pack, fam, k) in enumerate(((1, -1, "ham", 1), (3, 0, "ham", 2), (64, 1, "ham", 1), (1, -1, "lev2", 2), (3, 0, "lev2", 2), (64, 1, "lev2", 2))):
        add("queue_cap%d_pack%d_%s%d" % (cap, pack + 1, fam, k), fam, k, 37, 2, n, csr, 230 + i, tiles=2, dense_queue_cap=cap, dense_pack=pack, tags=("queue",))
    # n_q exactly q_per and q_per + 1: equality on reads without no-calls, three equal pairs in group 0, four in group 1
    # (the relation is symmetric: a pair is queued once, from its lower well)
    rng = np.random.default_rng([77, 236])
    tiles = make_tiles(rng, n, 14, csr, pf="all", nocall=False, plant=0.0)
    codes = np.stack(tiles[0][0], axis=1)
    for a in (2, 10, 20, 66, 74, 84, 94):
        codes[a + 1] = codes[a]
    out.append(Case("queue_exactly_full", "ham", 0, 14, 2, n, csr, [([np.ascontiguousarray(codes[:, j]) for j in range(14)], tiles[0][1])],
                    dense_queue_cap=3, tags=("queue", "exact")))
    # every well in a survivor pair, no queue over its cap: every well marked, the last row of `rows` in use
    tiles = make_tiles(rng, n, 21, csr, pf="all", nocall=False, plant=0.0)
    codes = np.stack(tiles[0][0], axis=1)
    codes[1::2] = codes[0::2]
    out.append(Case("every_well_marked", "ham", 1, 21, 2, n, csr, [([np.ascontiguousarray(codes[:, j]) for j in range(21)], tiles[0][1])],
                    dense_queue_cap=64, dense_pack=1, dense_nt=0, tags=("allmarked",)))
    # -- filters and edges
    add("no_pf", "ham", 1, 20, 2, n, csr, 240, pf="none", tags=("filters",))
    add("all_pf_no_log", "lev2", 2, 20, 2, n, csr, 241, pf="all", hit_cap=-1, per_target=False, tags=("filters",))
    add("small_log_sym", "ham", 1, 20, 2, n, csr, 242, hit_cap=25, per_target=False, tags=("filters", "hitcap"))
    empty = comb_csr(384, [sym([1, 2]), sym([20, 21])], keep=lambda c, d, l: not (c == 130 and l == 1))
    out.append(Case("empty_ring", "ham", 1, 20, 2, 384, empty, make_tiles(np.random.default_rng([77, 243]), 384, 20, empty, pf="all"),
                    check_empty=True, tags=("empty",)))
    # -- parts: 5 tiles in parts of 2 with a bounded pack grid: tile0, alternating scratch sets, dirty scratch
    for i, (fam, k) in enumerate((("ham", 1), ("lev2", 2))):
        add("parts_5_by_2_%s%d" % (fam, k), fam, k, 37, 2, n, csr, 250 + i, tiles=5, dense_overlap=1, dense_part_tiles=2, dense_pack_blocks=2,
            dense_pack=1, tags=("parts", "dirty"))
    n, csr = 400, comb_csr(400, [[-2, 1], [-40, 17, 33]])
    add("parts_5_by_2_two_ended", "lev2", 2, 21, 2, n, csr, 252, tiles=5, dense_overlap=1, dense_part_tiles=2, dense_pack_blocks=2,
        tags=("parts", "dirty", "twoended"), expect=("k_dense_pairs_win<2, false, 0>",))
    add("parts_5_by_2_gather", "ham", 1, 21, 2, n, csr, 253, tiles=5, dense_overlap=1, dense_part_tiles=2, dense_pack_blocks=2, dense_windows=0,
        dense_pack=1, tags=("parts", "dirty", "twoended", "gather"), expect=("k_dense_pairs<1, true, false>",))
    return out


def cases():
    """Built once per process and shared; nothing changes a case after it is built."""
    if not _cases:
        _cases.extend(_build())
        assert len({c.name for c in _cases}) == len(_cases)
    return _cases
