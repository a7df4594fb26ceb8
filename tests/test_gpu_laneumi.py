"""A lane's duplicates split by molecular identifier on the GPU (LaneDups.umi_begin / umi_add / umi,
include/welldup_laneumi.h) against the host reference of tests/laneumi_ref.py on the labels of tests/lanedups_ref.py /
lanenear_ref.py - lane row and tile rows equal cell by cell, nothing approximate - however the tiles and their UMI
planes are fed and whatever hash_bits, and against the identities the header states.  Every test first asserts on the
reference that its ground is covered."""
import ctypes
import io
import os
import shutil
from contextlib import redirect_stdout

import numpy as np
import pytest

from laneconsensus_ref import families_of
from lanedups_ref import lane_dups
from lanenear_ref import lane_near_dups
from laneumi_ref import (DISTINCT, FAMILIES, LANE_COLS, LARGE, LARGE_WELLS, LONE, MOLECULES, PER_FAMILY, REDUNDANT, SIZE,
                         SPLIT_FAMILIES, TILE_COLS, WELLS, WITH_N, check_umi_identities, lane_umi, umi_keys)
from test_gpu_lanemismatch import INDEX, MAX_TILES, N, WAYS, _finish, _host_tiles, _small_lane, _upload
from well_duplicates_amd import _lib
from well_duplicates_amd import count_well_duplicates as cwd
from well_duplicates_amd import report, synth
from well_duplicates_amd.scanner import LaneDups, Scanner, TileBatch

pytestmark = pytest.mark.gpu

BYTE = np.array([0x40, 0x81, 0xC2, 0x23, 0x00], dtype=np.uint8)        # a byte of every code A C G T N
U = 9


@pytest.fixture(scope="module")
def sc():
    s = Scanner(0)
    yield s
    s.close()


def _same(got, want):
    for g, w, name in zip(got, want, ("lane row", "tile rows")):
        assert g.shape == w.shape and (g == w).all(), (name, g[g != w], w[g != w], np.argwhere(g != w)[:8])


def _labels(tiles, n, max_tiles, k):
    """-> (the finish's lane row in lane_dups' columns, labels) of the reference"""
    if k == 0:
        lane, _, labels = lane_dups(tiles, n, max_tiles)
        return lane, labels
    near_lane, _, labels = lane_near_dups(tiles, n, max_tiles, k)
    return np.concatenate([near_lane[:6], near_lane[7:]]), labels


def _bytes(rng, codes):
    """codes 0..4 -> plane bytes: the base under a random quality that is not 0, byte 0 for N"""
    codes = np.asarray(codes)
    q = (rng.integers(1, 64, codes.shape) << 2).astype(np.uint8)
    return np.where(codes == 4, 0, BYTE[codes] | q).astype(np.uint8)


def _umis_for(rng, labels, n, index, u):
    """UMI codes per slot, uint8 [n, u]: every well a random UMI (one code in 40 an N); a copy gets its root's UMI with
    probability about one half, the same with one cycle changed with probability about one eighth, else keeps its own."""
    flat = np.asarray(labels, dtype=np.uint32).reshape(-1)
    codes = np.where(rng.random((flat.size, u)) < 0.025, 4, rng.integers(0, 4, (flat.size, u))).astype(np.uint8)
    for root, m in families_of(labels):
        for g in m[1:].tolist():
            p = rng.random()
            if p < 0.5:
                codes[g] = codes[root]
            elif p < 0.625:
                codes[g] = codes[root]
                c = int(rng.integers(0, u))
                codes[g, c] = (codes[g, c] + 1 + int(rng.integers(0, 3))) % 4
    return [codes[ti * n:(ti + 1) * n] for ti in index]


def _umi_batch(sc, umi_bytes, filts):
    n, u = umi_bytes[0].shape
    utb = TileBatch(sc, len(umi_bytes), u, n)
    for i, (r, f) in enumerate(zip(umi_bytes, filts)):
        utb.upload_tile(i, [np.ascontiguousarray(r[:, c]) for c in range(u)], f)
    return utb


def _umi_tiles(umi_bytes, index):
    return [(index[s], [np.ascontiguousarray(r[:, c]) for c in range(r.shape[1])]) for s, r in enumerate(umi_bytes)]


def _tables(tb, slots):
    ptrs = tb.plane_ptrs()
    return Scanner._tables([ptrs[s] for s in slots], [tb.filter_ptr(s) for s in slots], tb.L)


def _lane(sc, tb, utb, index, max_tiles, calls, order="after", hash_bits=0):
    """A lane fed call by call; the UMI planes of a call before its reads, after them, or all of them first"""
    ld = LaneDups(sc, tb.N, max_tiles, tb.L, hash_bits=hash_bits)
    try:
        ld.umi_begin(utb.L)
        if order == "first":
            for slots in reversed(calls):
                ld.umi_add(_tables(utb, slots), [index[s] for s in slots])
        for slots in calls:
            if order == "before":
                ld.umi_add(_tables(utb, slots), [index[s] for s in slots])
            ld.add_tables([index[s] for s in slots], _tables(tb, slots))
            if order == "after":
                ld.umi_add(_tables(utb, slots), [index[s] for s in slots])
    except Exception:
        ld.close()
        raise
    return ld


# ---- 1: the small lane ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 2])
def test_lane_umi_matches_reference_however_the_tiles_are_fed(sc, k):
    cycles = 37
    reads, filts = _small_lane(k, cycles)
    tiles = _host_tiles(reads, filts, INDEX)
    fin_lane, labels = _labels(tiles, N, MAX_TILES, k)
    rng = np.random.default_rng(900 + k)
    umi_bytes = [_bytes(rng, c) for c in _umis_for(rng, labels, N, INDEX, U)]
    umi_tiles = _umi_tiles(umi_bytes, INDEX)
    combos = [(e, mf) for e in (0, 1, 3) for mf in (2, 3, 256)]
    want = {c: lane_umi(tiles, umi_tiles, N, MAX_TILES, labels, *c) for c in combos}
    for (e, mf), w in want.items():
        check_umi_identities(*w, e, U=U, finish_lane=fin_lane, lower_e=want[(0, mf)] if e else None, at_e0=want[(0, mf)])
    check_umi_identities(*want[(3, 256)], 3, lower_e=want[(1, 256)])
    lane = want[(1, 256)][0]
    print("k %d: lane row at E 1, max_family 256: %s" % (k, lane.tolist()))
    # the ground: families of three or more beside the pairs, families that split and families that do not, UMI reads
    # merged as read errors at E = 1 and more at E = 3, lone wells, wells with N, families across tiles, and families
    # that max_family 2 and 3 leave out
    assert lane[FAMILIES] > 300 and lane[PER_FAMILY:SIZE].sum() == lane[FAMILIES] and lane[SIZE + 2:].sum() > 0
    assert 0 < lane[SPLIT_FAMILIES] < lane[FAMILIES] and lane[LONE] > 50 and lane[WITH_N] > 20
    assert want[(0, 256)][0][MOLECULES] > lane[MOLECULES] >= want[(3, 256)][0][MOLECULES] > lane[FAMILIES]
    assert want[(1, 2)][0][LARGE] > want[(1, 3)][0][LARGE] >= want[(1, 256)][0][LARGE]
    assert want[(1, 2)][0][FAMILIES] > 100 and want[(1, 3)][0][FAMILIES] > want[(1, 2)][0][FAMILIES]
    assert sum(1 for _, m in families_of(labels) if len(set((m // N).tolist())) > 1) > (100 if k else 30)
    tb = _upload(sc, reads, filts)
    utb = _umi_batch(sc, umi_bytes, filts)
    try:
        for bits in (0, 1):
            for i, calls in enumerate(WAYS.values()):
                ld = _lane(sc, tb, utb, INDEX, MAX_TILES, calls, order=("before", "after", "first")[(i + bits) % 3], hash_bits=bits)
                try:
                    rows = _finish(ld, k, bits)
                    for (e, mf), w in want.items():
                        got = ld.umi(e, mf)
                        _same(got, w)
                        check_umi_identities(*got, e, U=U, finish_lane=rows[0])
                finally:
                    ld.close()
    finally:
        utb.free()
        tb.free()


# ---- 2: the edges of the grouping -------------------------------------------------------------------
def _chain(rng, u, n):
    """n UMIs, each one cycle from the last"""
    out = np.zeros((n, u), dtype=np.uint8)
    out[0] = rng.integers(0, 4, u)
    for i in range(1, n):
        out[i] = out[i - 1]
        out[i, i % u] = (out[i, i % u] + 1 + rng.integers(0, 3)) % 4
    return out


def test_families_at_the_wave_at_the_chunk_and_at_the_cap(sc):
    """Two tiles of 2640 wells, 20 cycles of random reads, 12 UMI cycles, equality labels.  Planted families of 2, 3,
    63, 64, 65, 200 and 1024 identical reads: the family of 64 has its halves on the two tiles; those of 65 and 200 are
    chains of UMIs one apart with the wells permuted along the chain - one molecule at E = 1 that only the closure
    joins, 65 and 200 at E = 0; the family of 1024 holds eight UMIs and their one-cycle errors, with N among them; the
    family of 63 three.  max_family 1023 turns the largest family into Large."""
    n, cycles, u = N, 20, 12
    rng = np.random.default_rng(1024)
    codes = [rng.integers(0, 4, (n, cycles)) for _ in range(2)]
    reads = [_bytes(rng, c) for c in codes]
    filts = [(rng.random(n) < 0.9).astype(np.uint8) for _ in range(2)]
    umi = [rng.integers(0, 4, (n, u)).astype(np.uint8) for _ in range(2)]
    spots = [rng.permutation(n) for _ in range(2)]
    at = [0, 0]

    def take(tile, count):
        w = spots[tile][at[tile]:at[tile] + count]
        at[tile] += count
        return tile * n + w

    sizes = (2, 3, 63, 64, 65, 200, 1024)
    for size in sizes:
        wells = np.concatenate([take(0, 32), take(1, 32)]) if size == 64 else take(0, size)
        wells = rng.permutation(wells)                                 # (the wells' order along a chain is any)
        read = _bytes(rng, rng.integers(0, 4, cycles))
        if size in (65, 200):
            us = _chain(rng, u, size)
        else:
            centres = rng.integers(0, 4, (8 if size == 1024 else 3, u)).astype(np.uint8)
            us = centres[rng.integers(0, len(centres), size)]
            for j in np.flatnonzero(rng.random(size) < 0.3).tolist():
                us[j, rng.integers(0, u)] = rng.integers(0, 5)
            if size == 2:
                us[1] = us[0]
        for g, uu in zip(wells.tolist(), us):
            reads[g // n][g % n] = read
            filts[g // n][g % n] = 1
            umi[g // n][g % n] = uu
    index, max_tiles = [2, 0], 3
    tiles = _host_tiles(reads, filts, index)
    fin_lane, labels = _labels(tiles, n, max_tiles, 0)
    got_sizes = sorted(m.size for _, m in families_of(labels))
    assert got_sizes[-5:] == list(sizes[2:]) and set(got_sizes[:-5]) <= {2, 3}
    umi_bytes = [_bytes(rng, c) for c in umi]
    umi_tiles = _umi_tiles(umi_bytes, index)
    combos = [(0, 1024), (1, 1024), (2, 1024), (0, 1023), (1, 1023)]
    want = {c: lane_umi(tiles, umi_tiles, n, max_tiles, labels, *c) for c in combos}
    for (e, mf), w in want.items():
        check_umi_identities(*w, e, U=u, finish_lane=fin_lane, at_e0=want[(0, mf)], lower_e=want[(0, mf)] if e else None)
    l0, l1, capped = want[(0, 1024)][0], want[(1, 1024)][0], want[(1, 1023)][0]
    assert l0[LARGE] == l1[LARGE] == 0 and capped[LARGE] == 1 and capped[LARGE_WELLS] == 1024
    assert capped[WELLS] == l1[WELLS] - 1024 and capped[FAMILIES] == l1[FAMILIES] - 1
    assert l0[SIZE + 7] + 2 <= l1[SIZE + 7]                            # the two chains: molecules of 65 and 200 wells at E = 1
    assert l0[PER_FAMILY + 7] >= 2 and l0[MOLECULES] > l1[MOLECULES] + 200 and l1[WITH_N] > 20
    assert want[(1, 1024)][1][0, 0] >= 32 and want[(1, 1024)][1][2, 0] >= 1024      # wells on both tile indices
    tb = _upload(sc, reads, filts)
    utb = _umi_batch(sc, umi_bytes, filts)
    ld = _lane(sc, tb, utb, index, max_tiles, [[1], [0]], order="before")
    try:
        rows = _finish(ld, 0)
        for (e, mf), w in want.items():
            got = ld.umi(e, mf)
            _same(got, w)
            check_umi_identities(*got, e, U=u, finish_lane=rows[0])
    finally:
        ld.close()
        utb.free()
        tb.free()


# ---- 3, 4: against the index part; UMI cycles among the scanned ones ----------------------------------
@pytest.mark.parametrize("k", [0, 2])
def test_molecules_at_e0_are_the_group_spans_of_the_index_part(sc, k):
    cycles = 37
    reads, filts = _small_lane(k, cycles)
    tiles = _host_tiles(reads, filts, INDEX)
    fin_lane, labels = _labels(tiles, N, MAX_TILES, k)
    rng = np.random.default_rng(77 + k)
    umi_bytes = [_bytes(rng, c) for c in _umis_for(rng, labels, N, INDEX, U)]
    umi_tiles = _umi_tiles(umi_bytes, INDEX)
    want = lane_umi(tiles, umi_tiles, N, MAX_TILES, labels, 0, 1024)
    assert want[0][LARGE] == 0 and want[0][FAMILIES] < want[0][MOLECULES] < want[0][WELLS]
    tb = _upload(sc, reads, filts)
    utb = _umi_batch(sc, umi_bytes, filts)
    ld = LaneDups(sc, N, MAX_TILES, cycles)
    try:
        ld.index_begin(U)
        ld.umi_begin(U)
        for slots in WAYS["2 + 3"]:
            ld.index_add(_tables(utb, slots), [INDEX[s] for s in slots])
            ld.add_tables([INDEX[s] for s in slots], _tables(tb, slots))
            ld.umi_add(_tables(utb, slots), [INDEX[s] for s in slots])
        rows = _finish(ld, k)
        got = ld.umi(0, 1024)
        spans = int(ld.index_finish(min_pf=1)[0][2])
        _same(got, want)
        check_umi_identities(*got, 0, U=U, finish_lane=rows[0], group_spans=spans)
        _same(ld.umi(0, 1024), want)                                   # after the index finish, which used the lane's table
        keys = ld.umi_keys()
        given = np.repeat(np.isin(np.arange(MAX_TILES), INDEX), N)
        assert (keys[given] == ld.index_keys()[given]).all() and (keys[given] == umi_keys(umi_tiles, N, MAX_TILES)[given]).all()
    finally:
        ld.close()
        utb.free()
        tb.free()


def test_umi_cycles_among_the_scanned_ones_split_nothing(sc):
    cycles, at = 37, list(range(3, 12))
    reads, filts = _small_lane(0, cycles)
    tiles = _host_tiles(reads, filts, INDEX)
    fin_lane, labels = _labels(tiles, N, MAX_TILES, 0)
    umi_bytes = [np.ascontiguousarray(r[:, at]) for r in reads]
    umi_tiles = _umi_tiles(umi_bytes, INDEX)
    want = {e: lane_umi(tiles, umi_tiles, N, MAX_TILES, labels, e, 256) for e in (0, 1)}
    assert want[0][0][FAMILIES] > 300 and want[0][0][WELLS] > 2 * want[0][0][FAMILIES]
    tb = _upload(sc, reads, filts)
    utb = _umi_batch(sc, umi_bytes, filts)
    ld = _lane(sc, tb, utb, INDEX, MAX_TILES, WAYS["a tile per call"], order="first")
    try:
        rows = _finish(ld, 0)
        for e in (0, 1):
            got = ld.umi(e, 256)
            _same(got, want[e])
            check_umi_identities(*got, e, U=len(at), finish_lane=rows[0], subset_equality=True)
            assert got[0][REDUNDANT] == got[0][WELLS] - got[0][FAMILIES] and got[0][DISTINCT] == got[0][FAMILIES]
    finally:
        ld.close()
        utb.free()
        tb.free()


# ---- 5: call discipline -----------------------------------------------------------------------------
def _raw(sc, ld, max_e, max_family, scratch, scratch_bytes, missing=None):
    """wd_lane_umi itself -> (rc, lane row, tile rows); missing: the output pointer passed as null"""
    out = [np.full(LANE_COLS, -1, dtype=np.int64), np.full((ld.max_tiles, TILE_COLS), -1, dtype=np.int64)]
    ptr = [None if i == missing else a.ctypes.data_as(ctypes.c_void_p) for i, a in enumerate(out)]
    rc = sc._lib.wd_lane_umi(ld._h, max_e, max_family, ctypes.c_void_p(scratch), scratch_bytes, *ptr)
    return (rc,) + tuple(out)


def _untouched(res):
    return all((a == -1).all() for a in res[1:])


def test_call_discipline(sc):
    k, cycles, e, mf = 2, 37, 1, 256
    reads, filts = _small_lane(k, cycles)
    tiles = _host_tiles(reads, filts, INDEX)
    fin_lane, labels = _labels(tiles, N, MAX_TILES, k)
    rng = np.random.default_rng(55)
    umi_bytes = [_bytes(rng, c) for c in _umis_for(rng, labels, N, INDEX, U)]
    umi_tiles = _umi_tiles(umi_bytes, INDEX)
    want = lane_umi(tiles, umi_tiles, N, MAX_TILES, labels, e, mf)
    want_03 = lane_umi(tiles, umi_tiles, N, MAX_TILES, labels, 0, 3)
    assert want[0][MOLECULES] < want[0][DISTINCT] and want_03[0][LARGE] > 0
    need = sc.lane_umi_scratch_bytes(MAX_TILES, N)
    d_scratch = sc.malloc(need)
    sc.memset(d_scratch, 0xA5, need)                                   # whatever it holds: nothing is assumed of it
    host = np.zeros(need, dtype=np.uint8)
    tb = _upload(sc, reads, filts)
    utb = _umi_batch(sc, umi_bytes, filts)
    idx = TileBatch(sc, len(reads), 8, N)                              # index reads: the first eight cycles, again
    for i, r in enumerate(reads):
        idx.upload_tile(i, [np.ascontiguousarray(r[:, c]) for c in range(8)], filts[i])
    last = None
    ld = LaneDups(sc, N, MAX_TILES, cycles)
    try:
        with pytest.raises(ValueError) as err:                         # add before begin
            ld.umi_add(_tables(utb, [0]), [INDEX[0]])
        assert "wd_lane_umi_begin" in str(err.value)
        for bad in (0, 21):
            with pytest.raises(ValueError):
                ld.umi_begin(bad)
        assert ld.U == 0
        ld.index_begin(8)
        ld.umi_begin(U)
        with pytest.raises(ValueError):                                # begin is called once
            ld.umi_begin(U)
        assert sc._lib.wd_lane_umi_begin(ld._h, U, ctypes.c_void_p(ld.d_umi), ld.umi_bytes) == _lib.ERR_ARG
        assert b"lane umi: begin is called once" in sc._lib.wd_last_error(sc._ctx)
        for slots in WAYS["2 + 3"]:
            ld.add_tables([INDEX[s] for s in slots], _tables(tb, slots))
        ld.index_add(idx, INDEX)
        ld.umi_add(_tables(utb, [2, 0]), [INDEX[2], INDEX[0]])
        # refused adds: a tile again, twice in one call, out of range, the interleaved layout, planes in host memory
        for bad in ([INDEX[0]], [INDEX[1], INDEX[2]], [INDEX[3], INDEX[3]], [INDEX[3], MAX_TILES], [-1, INDEX[3]]):
            with pytest.raises(ValueError) as err:
                ld.umi_add(_tables(utb, [3, 4][:len(bad)]), bad)
            assert str(err.value).startswith(_lib.strerror(_lib.ERR_ARG)) and "lane umi: tile index" in str(err.value)
        with pytest.raises(ValueError):
            ld.umi_add(_tables(utb, [3]), [INDEX[3]], well_stride=4)
        assert sc.get_option("well_stride") == 1
        with pytest.raises(ValueError):                                # a batch of another shape (checked in Python)
            ld.umi_add(tb, INDEX)
        plane = np.zeros(N, dtype=np.uint8)
        table = (ctypes.c_void_p * U)(*[plane.ctypes.data] * U)
        with pytest.raises(ValueError) as err:
            ld.umi_add((table, None), [INDEX[3]])
        assert "device memory" in str(err.value)
        res = _raw(sc, ld, e, mf, d_scratch, need)                     # before any finish
        assert res[0] == _lib.ERR_ARG and _untouched(res)
        assert b"lane umi comes after a successful finish of the lane" in sc._lib.wd_last_error(sc._ctx)
        with pytest.raises(ValueError):
            ld.umi(e, mf)
        ld.umi_add(_tables(utb, [1, 3]), [INDEX[1], INDEX[3]])         # the refused adds changed nothing: these go in
        with pytest.raises(RuntimeError):                              # a near finish refused over budget is no finish
            ld.finish(hamming=k, pair_budget=3)
        res = _raw(sc, ld, e, mf, d_scratch, need)
        assert res[0] == _lib.ERR_ARG and _untouched(res) and b"finish" in sc._lib.wd_last_error(sc._ctx)
        rows = _finish(ld, k)
        res = _raw(sc, ld, e, mf, d_scratch, need)                     # tile INDEX[4] has reads and no UMI planes
        assert res[0] == _lib.ERR_ARG and _untouched(res)
        assert ("lane umi: tile index %d was added without UMI planes" % INDEX[4]).encode() in sc._lib.wd_last_error(sc._ctx)
        with pytest.raises(ValueError):                                # and after a finish nothing is added
            ld.umi_add(_tables(utb, [4]), [INDEX[4]])
        # the same lane again, every tile with its UMI planes
        ld.restart()
        for slots in WAYS["descending indices"]:
            ld.add_tables([INDEX[s] for s in slots], _tables(tb, slots))
        ld.index_add(idx, INDEX)
        ld.umi_add(utb, INDEX)
        rows = _finish(ld, k)
        for bad in ((-1, mf, d_scratch, need), (4, mf, d_scratch, need), (e, 1, d_scratch, need), (e, 1025, d_scratch, need),
                    (e, mf, 0, need), (e, mf, d_scratch, need - 1), (e, mf, d_scratch, 0), (e, mf, host.ctypes.data, need)):
            res = _raw(sc, ld, *bad)
            assert res[0] == _lib.ERR_ARG and _untouched(res), bad
        for missing in range(2):
            res = _raw(sc, ld, e, mf, d_scratch, need, missing=missing)
            assert res[0] == _lib.ERR_ARG and _untouched(res)
        for bad in ((-1, mf), (4, mf), (e, 1), (e, 1025)):
            with pytest.raises(ValueError):
                ld.umi(*bad)
        first = _raw(sc, ld, e, mf, d_scratch, need)                   # the caller's scratch, dirty from nothing
        assert first[0] == _lib.OK
        _same(first[1:], want)
        _same(_raw(sc, ld, e, mf, d_scratch, need)[1:], want)          # twice in a row, on the scratch the first call left
        _same(_raw(sc, ld, 0, 3, d_scratch, need)[1:], want_03)
        _same(_raw(sc, ld, e, mf, d_scratch, need)[1:], want)          # and on the scratch another max_family left
        _same(ld.umi(e, mf), want)
        listing = ld.index_finish(min_pf=1)
        keys = listing[3][:_lib.LANEHOPS_MAX_LISTED]
        before = ld.consensus(k, 256), ld.hops(8, 1, keys), listing
        _same(ld.umi(e, mf), want)                                     # after consensus, hops and the index finish
        again = ld.consensus(k, 256), ld.hops(8, 1, keys), ld.index_finish(min_pf=1)      # which find the accumulator as they left it
        for a, b in zip(before, again):
            assert all(np.array_equal(u, v) for u, v in zip(a, b))
        check_umi_identities(*ld.umi(e, mf), e, U=U, finish_lane=rows[0])
        # a lane without a UMI part; a lane without a tile: zeros
        ld2 = LaneDups(sc, N, MAX_TILES, cycles)
        try:
            ld2.add_tables([INDEX[0]], _tables(tb, [0]))
            _finish(ld2, 0)
            res = _raw(sc, ld2, e, mf, d_scratch, need)
            assert res[0] == _lib.ERR_ARG and _untouched(res) and b"wd_lane_umi_begin" in sc._lib.wd_last_error(sc._ctx)
            with pytest.raises(ValueError):                            # begin comes before any finish
                ld2.umi_begin(U)
        finally:
            ld2.close()
        ld.restart()
        _finish(ld, 0)
        res = _raw(sc, ld, 0, mf, d_scratch, need)
        assert res[0] == _lib.OK and not any(a.any() for a in res[1:])
        ld.close()
        with pytest.raises(ValueError):
            ld.umi(e, mf)
    finally:
        ld.close()
        idx.free()
        utb.free()
        tb.free()
        sc.free(d_scratch)


# ---- 6: the CLI -------------------------------------------------------------------------------------
def _main(argv):
    out = io.StringIO()
    with redirect_stdout(out):
        assert cwd.main(argv) == 0
    return out.getvalue()


def test_cli_lane_umi_block(tmp_path):
    """The run directory of test_gpu_lanemismatch.py's CLI test, one lane: tile 1103's files are tile 1101's but for the
    last cycle, which is tile 1102's.  Cycles 0-15 are scanned, 15-24 are the UMI: every well of 1103 is a copy of its
    well on 1101 whose UMI differs at the last cycle or not at all.  The new block closes the lane's output, equals
    write_lane_umi of the reference's rows and is all the flag adds, under another --tile-batch too; the TSV parses
    back to the rows."""
    rows, cols, levels, L, scan, lane = 36, 70, 3, 24, 15, 1
    n = rows * cols
    x, y = synth.honeycomb_pixels(rows, cols)
    spec = synth.SynthSpec(seed=35, n_clusters=n, row=cols, plant_per_64k=8000, nocall_per_64k=500, plant_far=True)
    run_dir = str(tmp_path / "run")
    names = ["1101", "1102", "1103", "1104"]
    synth.write_run_dir(spec, run_dir, [lane], names, list(range(L)), slocs=synth.slocs_bytes(x, y))
    source = lambda t, c: "1101" if t == "1103" and c < L - 1 else "1102" if t == "1103" else t
    ldir = os.path.join(run_dir, "Data", "Intensities", "BaseCalls", "L%03d" % lane)
    shutil.copy(os.path.join(ldir, "s_%d_1101.filter" % lane), os.path.join(ldir, "s_%d_1103.filter" % lane))
    for c in range(L):
        cdir = os.path.join(ldir, "C%d.1" % (c + 1))
        shutil.copy(os.path.join(cdir, "s_%d_%s.bcl.gz" % (lane, source("1103", c))),
                    os.path.join(cdir, "s_%d_1103.bcl.gz" % lane))
    argv = ["-s", "hiseq_x", "-r", run_dir, "-t", "1101,1102,1103,1104", "-i", str(lane), "-l", str(levels),
            "--cycles", "0-%d" % scan, "-q", "--all-wells", "--lane-dups"]
    planes = lambda t, cs: [synth.plane_bytes(spec, lane, int(source(t, c)), c) for c in cs]
    tiles = [(i, planes(t, range(scan)), synth.filter_bytes(spec, lane, int(t if t != "1103" else "1101")))
             for i, t in enumerate(names)]
    umi_tiles = [(i, planes(t, range(scan, L))) for i, t in enumerate(names)]
    finish = {0: lane_dups(tiles, n, 4), 2: lane_near_dups(tiles, n, 4, 2)}

    def block(k, e, max_family, summary):
        res = lane_umi(tiles, umi_tiles, n, 4, finish[k][2], e, max_family)
        counts = report.LaneUmiCounts.from_rows(*res, names, k, e, max_family, L - scan, int(finish[k][0][0]), int(finish[k][0][3]))
        text, tsv = io.StringIO(), io.StringIO()
        report.write_lane_umi(str(lane), counts, verbose=not summary, out=text)
        report.write_lane_umi_tsv(str(lane), counts, tsv)
        return text.getvalue(), tsv.getvalue(), counts, res

    want, tsv, counts, res = block(0, 1, 256, False)
    at_e0 = block(0, 0, 256, False)[2]
    pf_1101 = int((tiles[0][2] & 1).sum())
    assert counts.wells >= 2 * pf_1101 and counts.molecules < at_e0.molecules and counts.distinct_umis == at_e0.molecules
    # (a copy differs from its original at the UMI's last cycle or nowhere: at the default E = 1 nothing splits, the
    # UMI reads that differ are merged as read errors; at E = 0 they are molecules of their own)
    assert counts.split_families == 0 and counts.distinct_umis > counts.molecules == counts.families
    assert at_e0.split_families > 500 and at_e0.redundant_with_umi < at_e0.redundant == counts.redundant_with_umi
    small = block(2, 0, 3, True)[2]
    assert small.large > 0 and small.k == 2 and small.split_families > 500
    plain = _main(argv)
    assert want.count("LaneUmi: 1\tTile: ") == 4 and "LaneUmiSummary: 1\tTiles: 4\tHamming: 0\tUmiCycles: 9\tMismatches: 1\tMaxFamily: 256\t" in want
    out_file = str(tmp_path / "umi.tsv")
    got = _main(argv + ["--tile-batch", "1", "--lane-dups-umi", "%d-%d" % (scan, L), "--lane-dups-umi-out", out_file])
    assert got == plain + want                                         # the new block is all the flag adds
    assert open(out_file).read() == tsv
    parsed = [ln.split("\t") for ln in tsv.strip("\n").split("\n")[1:]]
    assert [int(r[3]) for r in parsed if r[1] == "per_family"] == res[0][PER_FAMILY:SIZE].tolist()
    assert [int(r[3]) for r in parsed if r[1] == "size"] == res[0][SIZE:].tolist()
    assert {r[2]: [int(v) for v in r[3:]] for r in parsed if r[1] == "tile"} == {t: res[1][i].tolist() for i, t in enumerate(names)}
    # on the clusters, after every other pass of the lane, the summary alone, E = 0 and a small max_family; with an
    # index part over other cycles beside the UMI part
    others = ["--lane-dups-hamming", "2", "-S", "--lane-dups-mismatches", "--lane-dups-index", "0-6", "--lane-dups-top", "5",
              "--lane-dups-consensus"]
    want, tsv, counts, res = block(2, 0, 3, True)
    assert counts.large > 0 and counts.k == 2 and "\tTile: " not in want
    got = _main(argv + others + ["--lane-dups-umi", "%d-%d" % (scan, L), "--lane-dups-umi-mismatches", "0",
                                 "--lane-dups-umi-max-family", "3", "--lane-dups-umi-out", out_file])
    assert got.endswith(want) and got.count(want) == 1 and got.count("LaneUmi") == want.count("LaneUmi")
    assert got.index("LaneConsensusSummary: 1") < got.index("LaneUmiSummary: 1")       # after every other block of the lane
    assert open(out_file).read() == tsv
