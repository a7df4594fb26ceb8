"""The cases of tests/dense_cases.py on the GPU: what tests/test_dense_emu.py runs through the dense chain's source on the
CPU (exact buffers, the LDS-DMA model, shuffled schedules) goes here through Scanner to the kernels themselves, with the
options a case names, so that emulator and hardware are held to one truth - the CPU oracle's tile counters, per-target
counts (INVALID_TARGET rows included), status and hit records - and the tables' summary the library reports
(dense_sym_on, dense_window_groups, dense_uniform_groups, dense_window_dwords) to the numpy reference of the tables.

The planes are placed as the emulator places them: "plane" is a stride of exactly N bytes (so planes lie 1 to 3 bytes off
alignment where N % 4 != 0), "ptr" a scattered pointer table (off alignment where the case asks for it).  The tiles are
a few hundred to a few thousand wells: the file takes seconds."""
import numpy as np
import pytest

import dense_cases as dc
from well_duplicates_amd.scanner import Scanner

pytestmark = pytest.mark.gpu

OPTIONS = ("dense_kernel",) + dc.OPTION_ORDER


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


def place(sc, case):
    """-> (slab, plane addresses [tile][cycle], filter addresses)"""
    n, L, n_tiles = case.n, case.L, len(case.tiles)
    if case.layout == "plane":
        step = L * n
        slab = sc.malloc(n_tiles * (step + n) + 256)
        ptrs = [[slab + i * step + c * n for c in range(L)] for i in range(n_tiles)]
        filt0 = slab + n_tiles * step
    else:
        slot = (n + 15) // 16 * 16 + 32
        slab = sc.malloc(n_tiles * (L * slot + n) + 256)
        order = np.random.default_rng(5).permutation(n_tiles * L)
        ptrs = [[0] * L for _ in range(n_tiles)]
        for j, o in enumerate(order):
            i, c = divmod(int(o), L)
            # (16 more bytes for cycle 1 of the even tiles: whatever the permutation, no tile's planes are a stride)
            ptrs[i][c] = slab + j * slot + (16 if c == 1 and i % 2 == 0 else 0) + ((1 + j % 3) if case.misalign else 0)
        filt0 = slab + n_tiles * L * slot
    filters = [filt0 + i * n for i in range(n_tiles)]
    for i, (planes, filt) in enumerate(case.tiles):
        for c in range(L):
            sc.h2d(ptrs[i][c], planes[c])
        sc.h2d(filters[i], np.ascontiguousarray(filt, dtype=np.uint8))
    return slab, ptrs, filters


@pytest.mark.parametrize("name", [c.name for c in dc.cases()])
def test_the_emulators_case_on_the_chain(sc, name):
    case = {c.name: c for c in dc.cases()}[name]
    want, tb = dc.qc.truth(case), case.tables()
    slab = 0
    try:
        sc.set_option("dense_kernel", 1)
        for opt in dc.OPTION_ORDER:
            sc.set_option(opt, case.options[opt])
        sc.set_targets(*case.csr())
        slab, ptrs, filters = place(sc, case)
        sc.hitlog_enable(max(case.hit_cap, 0))                  # (no log and a log without room are one to the library)
        run = lambda: sc.count_tiles(ptrs, filters, case.n, case.mode, case.k, per_target=case.per_target)
        if "empty" in case.tags:
            # The status bit, read back by the library, is what Scanner raises on; count_tiles raises before it returns,
            # so the counters of such a scan cannot be had here.  That the target's row is INVALID_TARGET and the other
            # targets' counts are right is checked on the CPU side (tests/test_dense_emu.py), as for k_scan_q's case.
            assert want["status"] == 1
            with pytest.raises(AssertionError, match="empty level"):
                run()
            assert sc.last_kernel().startswith("dense chain"), sc.last_kernel()
            return
        blocks, pt = run()
        assert sc.last_kernel().startswith("dense chain"), (case.name, sc.last_kernel())
        assert ("pairs from one end" in sc.last_kernel()) == tb["sym_on"], sc.last_kernel()
        assert (sc.get_option("dense_sym_on"), sc.get_option("dense_window_groups"), sc.get_option("dense_uniform_groups")) == \
            (int(tb["sym_on"]), tb["window_groups"] if case.options["dense_windows"] else 0, tb["uniform_groups"]), case.name
        # (with dense_windows off the library reports no window group: the path that ran, not the one the tables allow)
        if tb["kpad"]:
            assert sc.get_option("dense_window_dwords") == tb["window_dwords"], case.name
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
        for opt, v in sc.defaults:
            sc.set_option(opt, v)
        if slab:
            sc.free(slab)
