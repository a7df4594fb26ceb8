"""GPU parity tests with scripted survival (tests/survival_ref.py): inputs on which the test decides, pair by pair, at
which cycle a neighbour stops matching its centre - so that the survivor queues of k_scan_q, k_scan_lines and the
dense chain fill to their caps, overflow, drain with entries dying in every round and finish both ways.
tests/test_survival_host.py proves (on the host) which of those decisions each input drives.

Every comparison here is exact and against the CPU oracle alone: per-target counts (INVALID_TARGET rows where the
centre fails the filter), the tally block, and the hit log (tile, target, slot, dist) - the log is what catches a
mismatch lost or counted twice in a drain round when the pair still ends within the threshold.  The Levenshtein and
dense cases have no model of their own: only the oracle decides."""
import numpy as np
import pytest

import survival_ref as sr
from helpers import blocks_to_reference
from oracle import oracle
from well_duplicates_amd import cluster_indexes, synth, workload
from well_duplicates_amd.scanner import INVALID_TARGET, Scanner, TileBatch

pytestmark = pytest.mark.gpu

OPTIONS = ("early_exit", "batch_first", "batch_next", "targets_per_block", "queue_kernel", "queue_first", "dense_kernel",
           "dense_pack", "dense_queue_cap", "dense_sym", "line_walk", "line_pairs", "sort_targets", "lev2_closed")

Q_CASES = sorted(n for n, s in sr.CASES.items() if s[0] == "queue")
LW_CASES = sorted(n for n, s in sr.CASES.items() if s[0] == "lines")


@pytest.fixture(scope="module")
def sc():
    s = Scanner(0)
    s.defaults = [(name, s.get_option(name)) for name in OPTIONS]      # the library's own, read back - not restated
    yield s
    s.close()


def restore(sc):
    sc.hitlog_enable(0)
    for name, v in sc.defaults:
        sc.set_option(name, v)


# ---- the oracle, once per (input, mode, k) ------------------------------------------------------------------------
_want = {}


def want(key, scripts, csr, mode, k):
    """-> per tile (valid, dups, lens, dist), and the hit records [(tile, target, slot, dist)] of all tiles"""
    kk = (key, mode, k)
    if kk not in _want:
        centre, lvl_off, nbr = csr
        tiles, hits = [], []
        slots = np.arange(nbr.shape[0])
        tgt = np.searchsorted(lvl_off[:, 0], slots, side="right") - 1
        for i, s in enumerate(scripts):
            valid, dups, lens, dist = oracle.count_tile(s.planes, s.filt, centre, lvl_off, nbr, mode, k, want_dist=True)
            tiles.append((valid, dups, lens))
            ok = (valid[tgt] == 1) & (slots < lvl_off[tgt, -1]) & (dist <= (0 if mode == 0 else k))
            hits.append(np.stack([np.full(ok.sum(), i), tgt[ok], slots[ok], dist[ok]], axis=1))
        _want[kk] = (tiles, np.concatenate(hits).astype(np.int64))
    return _want[kk]


def sort_rows(a):
    return a[np.lexsort(a.T[::-1])] if a.shape[0] else a


def check(sc, run, key, scripts, csr, mode, k, what):
    """run() -> (blocks, per_target) of one scan; counts, tallies and the hit log against the oracle, exactly"""
    tiles, want_hits = want(key, scripts, csr, mode, k)
    levels = csr[1].shape[1] - 1
    cap = int(csr[2].shape[0]) * len(scripts) + 16
    sc.hitlog_enable(cap)
    blocks, pt = run()
    hits, total = sc.hitlog_fetch(cap)
    sc.hitlog_enable(0)
    n_dup = 0
    for i, (valid, dups, lens) in enumerate(tiles):
        got = pt[i].astype(np.int64)
        got[got == INVALID_TARGET] = -1
        bad = np.flatnonzero((got != np.where(valid[:, None] == 1, dups, -1)).any(axis=1))
        assert bad.shape[0] == 0, (what, mode, k, "tile", i, "targets", bad[:8], got[bad[:3]], dups[bad[:3]])
        assert (blocks_to_reference(blocks[i], levels) == oracle.tally_tile(valid, dups, lens)).all(), (what, mode, k, i)
        n_dup += int(dups[valid == 1].sum())
    assert total == want_hits.shape[0] == n_dup, (what, mode, k, total, want_hits.shape[0])
    got_hits = np.stack([hits["tile"], hits["target"], hits["slot"], hits["dist"]], axis=1).astype(np.int64)
    assert (sort_rows(got_hits) == sort_rows(want_hits)).all(), (what, mode, k)
    return n_dup


class Resident:
    """The tiles of an input on the device: a plane per cycle, the same planes behind a scrambled pointer table with
    odd alignments, and interleaved by four."""

    def __init__(self, sc, scripts, geom, pointer_table=False):
        self.sc, self.n, self.L = sc, geom.n, scripts[0].L
        self.plane = TileBatch(sc, len(scripts), self.L, self.n)
        self.il = TileBatch(sc, len(scripts), self.L, self.n, interleave=4)
        for i, s in enumerate(scripts):
            self.plane.upload_tile(i, s.planes, s.filt)
            self.il.upload_tile(i, s.planes, s.filt)
        self.slab, self.ptrs = 0, None
        if pointer_table:
            self.slab = sc.malloc(len(scripts) * self.L * (self.n + 13) + 64)
            order = np.random.default_rng(3).permutation(len(scripts) * self.L)
            self.ptrs = [[0] * self.L for _ in scripts]
            for j, o in enumerate(order):
                i, c = divmod(int(o), self.L)
                self.ptrs[i][c] = self.slab + 1 + j * (self.n + 13)
                sc.h2d(self.ptrs[i][c], scripts[i].planes[c])

    def batch(self, layout):
        return self.il if layout == "il" else self.plane

    def count_ptrs(self, mode, k):
        return self.sc.count_tiles(self.ptrs, self.plane.filter_ptrs(), self.n, mode, k, per_target=True)

    def free(self):
        self.plane.free()
        self.il.free()
        if self.slab:
            self.sc.free(self.slab)


def queue_name(strided, B1, levh, ws):
    return "k_scan_q<%s, %d, %d, %d>" % ("true" if strided else "false", B1, levh, ws)


# ---- k_scan_q --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Q_CASES)
def test_queue_kernel_scripted(sc, name):
    """The case's own threshold in its own layout at 64 targets per block in file order - the run the model speaks
    for - then the same scan behind a pointer table, in the other layout, at 7 and 1 targets per block and with the
    targets sorted by centre; the other thresholds of the Hamming family on the same input."""
    c = sr.case(name)
    csr = c.geom.csr()
    res = Resident(sc, c.tiles, c.geom, pointer_table=True)
    try:
        sc.set_targets(*csr)
        sc.set_option("line_walk", 0)
        sc.set_option("sort_targets", 0)
        assert sc.get_option("targets_per_block") == c.tpb == 64 and sc.get_option("queue_first") == 0
        n = check(sc, lambda: res.batch(c.layout).count(c.mode, c.k, per_target=True), name, c.tiles, csr, c.mode, c.k, name)
        assert n > 0
        assert sc.last_kernel() == queue_name(True, c.B1, 0, 4 if c.layout == "il" else 1), sc.last_kernel()
        for mode, k in ((0, 0), (1, 1), (1, 2), (1, 3)):
            for layout in ("plane", "il"):
                check(sc, lambda: res.batch(layout).count(mode, k, per_target=True), name, c.tiles, csr, mode, k, (name, layout))
                assert sc.last_kernel() == queue_name(True, sr.first_round(k, layout), 0, 4 if layout == "il" else 1)
            check(sc, lambda: res.count_ptrs(mode, k), name, c.tiles, csr, mode, k, (name, "pointer table"))
            assert sc.last_kernel() == queue_name(False, sr.auto_first(k), 0, 1), sc.last_kernel()
        for tpb in (7, 1):
            sc.set_option("targets_per_block", tpb)
            for layout in ("plane", "il"):
                check(sc, lambda: res.batch(layout).count(c.mode, c.k, per_target=True), name, c.tiles, csr, c.mode, c.k, (name, layout, tpb))
                assert sc.last_kernel().startswith("k_scan_q<")
        sc.set_option("targets_per_block", 64)
        sc.set_option("sort_targets", 1)
        sc.set_targets(*csr)                                     # (the sorted view is made when the targets are installed)
        check(sc, lambda: res.batch(c.layout).count(c.mode, c.k, per_target=True), name, c.tiles, csr, c.mode, c.k, (name, "sorted"))
        assert sc.last_kernel().startswith("k_scan_q<")
    finally:
        restore(sc)
        res.free()


@pytest.mark.parametrize("name", [n for n in Q_CASES if "_plane_L37" in n or "_plane_L14" in n])
def test_queue_first_round_depths(sc, name):
    """queue_first 1..8 in the plane layout: the first round ends elsewhere, so other pairs are queued and the drain's
    rounds start at other cycles (a first round of 8 or more of L = 14's cycles leaves one short round)."""
    c = sr.case(name)
    csr = c.geom.csr()
    res = Resident(sc, c.tiles, c.geom)
    try:
        sc.set_targets(*csr)
        sc.set_option("line_walk", 0)
        sc.set_option("sort_targets", 0)
        for qf in range(1, 9):
            sc.set_option("queue_first", qf)
            for mode, k in {(c.mode, c.k), (1, 2)}:
                check(sc, lambda: res.plane.count(mode, k, per_target=True), name, c.tiles, csr, mode, k, (name, qf))
                assert sc.last_kernel() == queue_name(True, qf, 0, 1), sc.last_kernel()
    finally:
        restore(sc)
        res.free()


def test_queue_kernel_large_threshold(sc):
    """k = 30 at L = 37: the first round (8 cycles) kills nobody, finish_from(k) >= L so no drain ends all at once,
    and the mismatch count in the tag (min(mm, 255)) is carried across every round.  Targets of 30 slots - under
    kFinishInPlace, so the passes are queued, four to a queue before it overflows - and random reads, whose
    distances (about 28) lie on both sides of the threshold; k = 36 and 37 on the same input."""
    geom = sr.Geometry(300, 30, 3)
    scripts = []
    for i in range(2):
        rng = np.random.default_rng([77, i])
        codes = sr.random_codes(rng, (geom.n, 37))
        near = rng.random(geom.nbr.shape[0]) < 0.3                 # a few near copies among the random reads
        src = np.repeat(geom.centre, geom.K)[near]
        cp = codes[src].copy()
        flip = rng.random(cp.shape) < 0.5
        cp[flip] = (cp[flip] + rng.integers(1, 5, size=int(flip.sum()))) % 5
        codes[geom.nbr[near]] = cp
        scripts.append(sr.finish(rng, geom, 37, 30, codes, bad_centres=(5, 17, 299)))
    csr = geom.csr()
    res = Resident(sc, scripts, geom, pointer_table=True)
    try:
        sc.set_targets(*csr)
        sc.set_option("line_walk", 0)
        for k in (30, 36, 37, 20):
            for layout in ("plane", "il"):
                n = check(sc, lambda: res.batch(layout).count(1, k, per_target=True), "large_k", scripts, csr, 1, k, layout)
                assert sc.last_kernel().startswith(queue_name(True, 4 if layout == "il" else 8, 0, 4 if layout == "il" else 1))
            check(sc, lambda: res.count_ptrs(1, k), "large_k", scripts, csr, 1, k, "pointer table")
        dist = np.concatenate([oracle.count_tile(s.planes, s.filt, *csr, 1, 30, want_dist=True)[3] for s in scripts])
        assert 0.2 < (dist <= 30).mean() < 0.95 and (dist > 30).any() and n > 0      # both sides of the threshold
    finally:
        restore(sc)
        res.free()


# ---- Levenshtein: the closed form for k = 2, the banded kernels for k = 3, 4, 5 ---------------------------------
@pytest.mark.parametrize("name", ["q_k2_plane_L37", "q_k2_il_L37", "q_k3_plane_L37", "q_k0_plane_L14", "q_k2_plane_K254",
                                  "q_k1_il_K300", "lw_k2_plane_L37"])
def test_levenshtein_scripted(sc, name):
    """The scripted inputs, and the same with every 7th neighbour a shift of its centre (edit distance <= 2, large
    Hamming distance) or its centre with an insertion and a deletion.  No model speaks for edit distance: the oracle
    alone decides."""
    c = sr.case(name)
    csr = c.geom.csr()
    edited = [sr.add_edit_scripts(np.random.default_rng([9, i]), s) for i, s in enumerate(c.tiles)]
    try:
        for key, scripts in ((name, c.tiles), (name + "+edits", edited)):
            res = Resident(sc, scripts, c.geom)
            try:
                sc.set_targets(*csr)
                sc.set_option("line_walk", 0)
                for layout in ("plane", "il"):
                    ws = 4 if layout == "il" else 1
                    run = lambda k: (lambda: res.batch(layout).count(2, k, per_target=True))
                    n = check(sc, run(2), key, scripts, csr, 2, 2, (key, layout))
                    assert n > 0 and sc.last_kernel() == queue_name(True, 8 if ws == 4 else 5, -1, ws), sc.last_kernel()
                    sc.set_option("lev2_closed", 0)                   # k = 2 through the banded DP
                    check(sc, run(2), key, scripts, csr, 2, 2, (key, layout, "banded"))
                    assert sc.last_kernel().startswith("k_scan_q<true") and ", 1, %d>" % ws in sc.last_kernel(), sc.last_kernel()
                    sc.set_option("lev2_closed", 1)
                    check(sc, run(3), key, scripts, csr, 2, 3, (key, layout))
                    assert sc.last_kernel().startswith("k_scan_q<true") and ", 1, %d>" % ws in sc.last_kernel(), sc.last_kernel()
                    if layout == "plane":
                        for qf in (4, 5, 6):
                            sc.set_option("queue_first", qf)
                            check(sc, run(2), key, scripts, csr, 2, 2, (key, "queue_first", qf))
                            assert sc.last_kernel() == queue_name(True, qf, -1, 1), sc.last_kernel()
                        sc.set_option("queue_first", 0)
                        for k in (4, 5):                              # (wider bands read planes only)
                            check(sc, run(k), key, scripts, csr, 2, k, (key, layout))
                            assert sc.last_kernel().startswith("k_scan_q<true") and ", 2, 1>" in sc.last_kernel(), sc.last_kernel()
            finally:
                res.free()
    finally:
        restore(sc)


# ---- the line walk ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LW_CASES)
def test_line_walk_scripted(sc, name):
    """k_scan_lines on inputs whose windows of 128 pairs are scripted (a window is a target: K = 128), in blocks of
    512 pairs (a window per wave) and of 12288 (24 per wave: the queue fills, overflows and drains as the model
    says); the striped cases hold 42 or 43 survivors in ANY 128 consecutive pairs - both sides of kLwInPlace."""
    c = sr.case(name)
    csr = c.geom.csr()
    res = Resident(sc, c.tiles, c.geom, pointer_table=True)
    try:
        sc.set_targets(*csr)
        sc.set_option("line_walk", 1)
        for pairs in (512, 12288):
            sc.set_option("line_pairs", pairs)
            for mode, k in ((0, 0), (1, 1), (1, 2), (1, 3), (2, 2)):        # (the case's own threshold is one of them)
                for layout in ("plane", "il"):
                    check(sc, lambda: res.batch(layout).count(mode, k, per_target=True), name, c.tiles, csr, mode, k, (name, pairs, layout))
                    assert sc.last_kernel().startswith("k_scan_lines"), sc.last_kernel()
                    assert sc.get_option("line_walk_blocks") == -(-c.geom.T * c.geom.K // pairs)
            check(sc, lambda: res.count_ptrs(c.mode, c.k), name, c.tiles, csr, c.mode, c.k, (name, pairs, "pointer table"))
            assert sc.last_kernel().startswith("k_scan_lines<false"), sc.last_kernel()
    finally:
        restore(sc)
        res.free()


# ---- the sequential kernel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Q_CASES)
def test_sequential_kernel_scripted(sc, name):
    """queue_kernel = 0, with and without the early exit: the same oracle result."""
    c = sr.case(name)
    csr = c.geom.csr()
    res = Resident(sc, c.tiles, c.geom)
    try:
        sc.set_targets(*csr)
        sc.set_option("queue_kernel", 0)
        sc.set_option("line_walk", 0)
        for early in (0, 1):
            sc.set_option("early_exit", early)
            for mode, k in {(c.mode, c.k), (2, 2)}:
                check(sc, lambda: res.plane.count(mode, k, per_target=True), name, c.tiles, csr, mode, k, (name, "sequential", early))
                assert not sc.last_kernel().startswith(("k_scan_q", "k_scan_lines")), sc.last_kernel()
    finally:
        restore(sc)
        res.free()


# ---- shared prefixes: primer or adaptor, then divergence --------------------------------------------------------
@pytest.mark.parametrize("which", range(6))
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_shared_prefix(sc, k, which):
    """Every read of the tile shares its first p cycles and is random after that: every pair survives p cycles and
    dies soon after - all of a pass in one drain round.  p around the first round, around finish_from(k), and L - 1."""
    L, B1, F = 37, sr.auto_first(k), sr.finish_from(k)
    p = (B1 - 1, B1, B1 + 1, F - 1, F, L - 1)[which]
    geom = sr.Geometry(150, 127, 5)
    scripts = [sr.shared_prefix(np.random.default_rng([k, p, i]), geom, L, p, bad_centres=(3, 77)) for i in range(2)]
    csr = geom.csr()
    key = ("prefix", k, p)
    mode = 0 if k == 0 else 1
    res = Resident(sc, scripts, geom)
    try:
        sc.set_targets(*csr)
        for walk in (0, 1):
            sc.set_option("line_walk", walk)
            for layout in ("plane", "il"):
                for m, kk in ((mode, k), (2, 2)):
                    check(sc, lambda: res.batch(layout).count(m, kk, per_target=True), key, scripts, csr, m, kk, (key, walk, layout))
                    assert sc.last_kernel().startswith("k_scan_lines" if walk else "k_scan_q"), sc.last_kernel()
    finally:
        restore(sc)
        res.free()


# ---- the dense chain ---------------------------------------------------------------------------------------------
_dense_targets = {}


def dense_targets():
    if not _dense_targets:
        rows, cols, levels = 30, 200, 3
        x, y = synth.honeycomb_pixels(rows, cols)
        _dense_targets["csr"] = workload.targets_to_csr(cluster_indexes.generate(x, y, range(rows * cols), levels))
    return _dense_targets["csr"]


class DenseTile:
    def __init__(self, planes, filt):
        self.planes, self.filt, self.L = planes, filt, len(planes)


def dense_tile(rng, csr, L, f, p):
    """A fraction f of the wells shares its first p cycles (the signature is the first 5: with f = 1 every pair passes
    the signature round, real non-duplicates in bulk); on top, copies with 0..3 mismatches behind the prefix planted on
    a well's own neighbours."""
    centre, lvl_off, nbr = csr
    n = centre.shape[0]
    codes = sr.random_codes(rng, (n, L), nocall=0.02)
    share = rng.random(n) < f
    codes[share, :p] = sr.random_codes(rng, (1, p), nocall=0.0)
    for w in rng.choice(n, size=n // 12, replace=False):
        slot = int(rng.integers(lvl_off[w, 0], lvl_off[w, -1]))
        cp = codes[w].copy()
        for _ in range(int(rng.integers(0, 4))):
            at = int(rng.integers(min(p, L - 1), L))
            cp[at] = (cp[at] + int(rng.integers(1, 5))) % 5
        codes[nbr[slot]] = cp
    b = sr.codes_to_bytes(rng, codes)
    bad = rng.random(n) < 0.03
    return DenseTile([np.ascontiguousarray(b[:, c]) for c in range(L)], sr.filter_bytes(rng, n, bad))


@pytest.mark.parametrize("p", [5, 8, 16])
@pytest.mark.parametrize("f", [0.3, 1.0])
@pytest.mark.parametrize("L", [24, 17])
def test_dense_chain_shared_prefix(sc, L, f, p):
    """A 30 x 200 honeycomb, every well a centre, 3 levels: the dense chain's survivor regions (16 entries per 64
    targets, 32 for Levenshtein) at their default size under a signature round that lets non-duplicates through."""
    csr = dense_targets()
    n = csr[0].shape[0]
    tiles = [dense_tile(np.random.default_rng([L, int(f * 10), p, i]), csr, L, f, p) for i in range(2)]
    key = ("dense", L, f, p)
    tb = TileBatch(sc, len(tiles), L, n)
    try:
        for i, t in enumerate(tiles):
            tb.upload_tile(i, t.planes, t.filt)
        assert sc.get_option("dense_queue_cap") == 0
        for sym in (1, 0):
            sc.set_option("dense_sym", sym)
            sc.set_targets(*csr)
            sc.set_option("dense_kernel", 1)
            for pack in (-1, 0, 1):
                sc.set_option("dense_pack", pack)
                for mode, k in ((0, 0), (1, 2), (2, 2)):
                    nd = check(sc, lambda: tb.count(mode, k, per_target=True), key, tiles, csr, mode, k, (key, sym, pack))
                    assert nd > 0
                    assert sc.last_kernel().startswith("dense chain"), sc.last_kernel()
                    assert sc.get_option("dense_window_groups") > ((n + 63) // 64) // 4        # the path under test ran
                    assert sc.get_option("dense_sym_on") == sym
    finally:
        restore(sc)
        tb.free()
