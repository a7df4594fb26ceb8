"""The cases of tests/levk_cases.py on the GPU: what tests/test_levk_emu.py runs through the kernels' source on the CPU
(exact buffers, shuffled schedules) goes here through Scanner / TileBatch to the kernels themselves - k_scan_q with the
banded DP in its queue entries (k = 2 with lev2_closed = 0, .. 7), k_scan<LevState<H>, ..> (k = 8 .. 17; any k with the
queue kernel or the early exit switched off; a target of 509 slots) and k_scan_lev_generic (k >= 18) - so that emulator
and hardware are held to one truth: the CPU oracle's tile counters, per-target counts (INVALID_TARGET rows included) and
hit records with their distances.  Integers, compared exactly.  wd_last_kernel() must name the very instantiation the
emulator ran for the case.  The pairs are scripted to lie at the threshold, one above it and on the band's outermost
diagonal (tests/test_levk_cases_host.py asserts that they do).  The tiles are small (257 to 4099 wells): a kind and a
layout - some fifty to a hundred and fifty cases - take a second or two."""
import numpy as np
import pytest

import levk_cases as lc
from oracle import oracle
from well_duplicates_amd.scanner import Scanner, TileBatch

pytestmark = pytest.mark.gpu

OPTIONS = ("queue_kernel", "queue_first", "targets_per_block", "lev2_closed", "sort_targets", "line_walk", "early_exit")


@pytest.fixture(scope="module")
def sc():
    s = Scanner(0)
    s.defaults = [(name, s.get_option(name)) for name in OPTIONS]      # the library's own, read back - not restated
    yield s
    s.hitlog_enable(0)
    for name, v in s.defaults:
        s.set_option(name, v)
    s.close()


def sort_rows(a):
    return a[np.lexsort(a.T[::-1])] if a.shape[0] else a


def run_case(sc, case):
    want = lc.truth(case)
    n_tiles = len(case.tiles)
    sc.set_option("queue_kernel", case.queue_kernel)
    sc.set_option("early_exit", case.early)
    sc.set_option("line_walk", 0)
    sc.set_option("lev2_closed", 0)                             # (k = 2 by the banded DP, not by the closed form)
    sc.set_option("queue_first", 0)
    sc.set_option("targets_per_block", case.tpb)
    sc.set_option("sort_targets", int(case.sort))
    sc.set_targets(*case.csr())                                 # (the sorted view is made when the targets are installed)
    tb, slab = None, 0
    try:
        if case.layout == "ptr":
            # a pointer per cycle, the planes scattered with odd alignments: no stride describes them
            tb = TileBatch(sc, n_tiles, 1, case.n)              # (the filters' home)
            slab = sc.malloc(n_tiles * case.L * (case.n + 13) + 64)
            order = np.random.default_rng(3).permutation(n_tiles * case.L)
            ptrs = [[0] * case.L for _ in case.tiles]
            for j, o in enumerate(order):
                i, c = divmod(int(o), case.L)
                ptrs[i][c] = slab + 1 + j * (case.n + 13) + (7 if c == 1 and i % 2 == 0 else 0)
                sc.h2d(ptrs[i][c], case.tiles[i][0][c])
            for i, (_, filt) in enumerate(case.tiles):
                sc.h2d(tb.filter_ptr(i), np.ascontiguousarray(filt, dtype=np.uint8))
            run = lambda: sc.count_tiles(ptrs, tb.filter_ptrs(), case.n, case.mode, case.k, per_target=True)
        else:
            tb = TileBatch(sc, n_tiles, case.L, case.n, interleave=4 if case.layout == "il" else 1)
            for i, (planes, filt) in enumerate(case.tiles):
                tb.upload_tile(i, planes, filt)
            run = lambda: tb.count(case.mode, case.k, per_target=True)
        sc.hitlog_enable(max(case.hit_cap, 0))
        blocks, pt = run()
        assert sc.last_kernel().startswith(case.kernel), (case.name, sc.last_kernel())
        assert (blocks == want["out_tile"]).all(), (case.name, blocks, want["out_tile"])
        assert (pt == want["out_pt"]).all(), (case.name, np.argwhere(pt != want["out_pt"])[:8])
        if case.hit_cap > 0:
            hits, total = sc.hitlog_fetch(case.hit_cap)
            got = np.stack([hits["tile"], hits["target"], hits["slot"], hits["dist"]], axis=1).astype(np.int64)
            oracle_hits = want["hits"].astype(np.int64)
            assert total == oracle_hits.shape[0] == got.shape[0], (case.name, total, got.shape)
            assert (sort_rows(got) == sort_rows(oracle_hits)).all(), case.name      # the oracle's true distances
    finally:
        sc.hitlog_enable(0)
        if tb is not None:
            tb.free()
        if slab:
            sc.free(slab)


@pytest.mark.parametrize("kind,layout", [("queue", "ptr"), ("queue", "plane"), ("queue", "il"), ("seq", "ptr"), ("seq", "plane"),
                                         ("generic", "ptr"), ("generic", "plane")])
def test_the_emulators_cases_on_the_kernels(sc, kind, layout):
    ran = set()
    for case in lc.cases():
        if case.kind == kind and case.layout == layout:
            run_case(sc, case)
            ran.add(case.kernel)
    assert len(ran) == {"queue": 1 if layout == "il" else 6, "seq": 6, "generic": 1}[kind], ran


def test_a_threshold_beyond_the_lds_is_refused_and_the_context_lives_on(sc):
    """L = 400, k = 398: the generic kernel would need (2 * 199 + 1) * 128 + 65 * 400 + 8 bytes of LDS, more than 64 KB - the
    host refuses (WD_ERR_UNSUPPORTED) before any launch.  The next scan on the same context answers, and rightly."""
    rng = np.random.default_rng(11)
    n, L = 300, 400
    centre = np.array([5, 17], dtype=np.int32)
    nbr = np.array([int(v) for v in rng.choice(np.arange(20, n), size=40, replace=False)], dtype=np.int32)
    lvl_off = np.array([[0, 10, 20], [20, 30, 40]], dtype=np.int32)
    codes = lc.sr.random_codes(rng, (n, L))
    codes[nbr[::2]] = codes[centre[0]]                          # copies of the first centre, some with an edit or two
    codes[nbr[::4], 7] = (codes[nbr[::4], 7] + 1) % 5
    b = lc.sr.codes_to_bytes(rng, codes)
    planes = [np.ascontiguousarray(b[:, c]) for c in range(L)]
    filt = lc.sr.filter_bytes(rng, n, np.zeros(n, dtype=bool))
    for name, v in sc.defaults:
        sc.set_option(name, v)
    sc.set_option("line_walk", 0)
    sc.set_targets(centre, lvl_off, nbr)
    tb = TileBatch(sc, 1, L, n)
    try:
        tb.upload_tile(0, planes, filt)
        assert (2 * 199 + 1) * 128 + 65 * 400 + 8 > 64 * 1024
        with pytest.raises(RuntimeError, match="64 KB of LDS"):
            tb.count(2, 398, per_target=True)
        for k in (2, 5, 20):
            blocks, pt = tb.count(2, k, per_target=True)
            valid, dups, lens, _ = oracle.count_tile(planes, filt, centre, lvl_off, nbr, 2, k)
            assert (pt[0].astype(np.int64) == np.where(valid[:, None] == 1, dups, -1).astype(np.int64) & 0xFFFFFFFF).all(), k
            assert blocks[0, 0] == valid.sum() and dups.sum() > 0
    finally:
        tb.free()
