"""The cases of tests/linewalk_cases.py on the GPU: what tests/test_linewalk_emu.py runs through k_scan_lines' source on the
CPU (the library's own tables, exact buffers, shuffled schedules, the workgroups permuted) goes here through Scanner /
TileBatch to the kernel itself, with line_walk = 1 and the case's line_pairs, so that emulator and hardware are held to
one truth - the CPU oracle's tile counters, per-target counts (INVALID_TARGET rows included) and hit records.
wd_last_kernel() must name the very instantiation the emulator ran for the case, and line_walk_blocks must be the block
count of the Python reference of the tables (0, and another kernel, for the target of 4096 slots).  The tiles are small
(257 to 4099 wells): a family and a layout - some thirty to forty-five cases - take a second or two.  No kernel is added
or changed for this."""
import numpy as np
import pytest

import linewalk_cases as lc
from well_duplicates_amd.scanner import Scanner, TileBatch

pytestmark = pytest.mark.gpu

OPTIONS = ("queue_kernel", "queue_first", "targets_per_block", "lev2_closed", "sort_targets", "line_walk", "line_pairs", "early_exit",
           "dense_kernel")


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
    sc.set_option("queue_kernel", 1)
    sc.set_option("early_exit", 1)
    sc.set_option("lev2_closed", 1)
    sc.set_option("dense_kernel", 0)                            # (the dense path has its own tests: here the sampled scan is meant)
    sc.set_option("sort_targets", 0)
    sc.set_option("line_walk", 1)
    sc.set_option("line_pairs", case.line_pairs)
    sc.set_targets(*case.csr())                                 # (the tables are built by the first scan that wants them)
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
                # (7 more bytes for cycle 1 of the even tiles: the planes of a tile are then no arithmetic sequence)
                ptrs[i][c] = slab + 1 + j * (case.n + 13) + (7 if c == 1 and i % 2 == 0 else 0)
                sc.h2d(ptrs[i][c], case.tiles[i][0][c])
            for i, (_, filt) in enumerate(case.tiles):
                sc.h2d(tb.filter_ptr(i), np.ascontiguousarray(filt, dtype=np.uint8))
            run = lambda: sc.count_tiles(ptrs, tb.filter_ptrs(), case.n, case.mode, case.k, per_target=case.per_target)
        else:
            tb = TileBatch(sc, n_tiles, case.L, case.n, interleave=4 if case.layout == "il" else 1)
            for i, (planes, filt) in enumerate(case.tiles):
                tb.upload_tile(i, planes, filt)
            run = lambda: tb.count(case.mode, case.k, per_target=case.per_target)
        sc.hitlog_enable(max(case.hit_cap, 0))                  # (no log and a log without room are one to the library)
        blocks, pt = run()
        ran = sc.last_kernel()
        if case.kernel is None:                                 # the walk does not apply: it stands aside
            assert sc.get_option("line_walk_blocks") == 0 and not ran.startswith("k_scan_lines"), (case.name, ran)
        else:
            assert ran.startswith(case.kernel), (case.name, ran)
            assert sc.get_option("line_walk_blocks") == case.blocks, (case.name, sc.get_option("line_walk_blocks"), case.blocks)
        assert (blocks == want["out_tile"]).all(), (case.name, blocks, want["out_tile"])
        if case.per_target:
            assert (pt == want["out_pt"]).all(), (case.name, np.argwhere(pt != want["out_pt"])[:8])
        else:
            assert pt is None
        if case.hit_cap > 0:
            hits, total = sc.hitlog_fetch(case.hit_cap)
            got = np.stack([hits["tile"], hits["target"], hits["slot"], hits["dist"]], axis=1).astype(np.int64)
            oracle_hits = want["hits"].astype(np.int64)
            assert total == oracle_hits.shape[0] and got.shape[0] == min(total, case.hit_cap), (case.name, total, got.shape)
            if total <= case.hit_cap:
                assert (sort_rows(got) == sort_rows(oracle_hits)).all(), case.name
            else:
                # the log is too small: what it kept are distinct records of the oracle's
                have = {tuple(r) for r in oracle_hits.tolist()}
                kept = {tuple(r) for r in got.tolist()}
                assert len(kept) == case.hit_cap and kept <= have, case.name
    finally:
        sc.hitlog_enable(0)
        if tb is not None:
            tb.free()
        if slab:
            sc.free(slab)


@pytest.mark.parametrize("layout", lc.LAYOUTS)
@pytest.mark.parametrize("fam", lc.FAMILIES)
def test_the_emulators_cases_on_the_kernel(sc, fam, layout):
    ran = set()
    for case in lc.cases():
        if case.fam == fam and case.layout == layout:
            run_case(sc, case)
            ran.add(case.kernel)
    ran.discard(None)
    assert len(ran) == (1 if layout == "il" or fam == "lev2" else 5), ran
