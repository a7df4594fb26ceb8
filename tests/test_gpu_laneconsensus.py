"""A lane's errors against its families' vote on the GPU (LaneDups.consensus, include/welldup_laneconsensus.h) against
the host reference of tests/laneconsensus_ref.py on the labels of tests/lanedups_ref.py / lanenear_ref.py - lane row,
tile rows and the call matrix equal cell by cell, nothing approximate - however the tiles are fed and whatever
hash_bits, and against the identities the header states.  Every test first asserts on the reference that its ground
is covered."""
import ctypes
import io
import os
import shutil
from contextlib import redirect_stdout

import numpy as np
import pytest

from laneconsensus_ref import (DIST, FAMILIES, FIRST_OFF, LANE_COLS, LARGE, LARGE_WELLS, MISMATCHES, PAIRS, PROFILED,
                               TILE_COLS, UNDECIDED, WELLS, WITH_N, check_consensus_identities, families_of, lane_consensus)
from lanedups_ref import lane_dups
from lanenear_ref import lane_near_dups
from test_gpu_lanemismatch import INDEX, MAX_TILES, N, RUN, WAYS, WINDOW, _finish, _host_tiles, _lane, _small_lane, _upload
from well_duplicates_amd import _lib
from well_duplicates_amd import count_well_duplicates as cwd
from well_duplicates_amd import report, synth
from well_duplicates_amd.scanner import Scanner

pytestmark = pytest.mark.gpu

BYTE = np.array([0x40, 0x81, 0xC2, 0x23, 0x00], dtype=np.uint8)        # a byte of every code A C G T N
PAIRS12 = [(a, b) for a in range(4) for b in range(4) if a != b]       # the ordered pairs of bases


@pytest.fixture(scope="module")
def sc():
    s = Scanner(0)
    yield s
    s.close()


def _same(got, want):
    for g, w, name in zip(got, want, ("lane row", "tile rows", "calls")):
        assert g.shape == w.shape and (g == w).all(), (name, g[g != w], w[g != w], np.argwhere(g != w)[:8])


def _labels(tiles, n, max_tiles, k):
    """-> (the finish's lane row in lane_dups' columns, its tile rows, labels) of the reference"""
    if k == 0:
        return lane_dups(tiles, n, max_tiles)
    near_lane, near_tiles, labels = lane_near_dups(tiles, n, max_tiles, k)
    return np.concatenate([near_lane[:6], near_lane[7:]]), near_tiles, labels


def _random_reads(rng, n, cycles):
    """uint8 [n, cycles]: bytes of random bases under random qualities, never a no-call"""
    return (BYTE[rng.integers(0, 4, (n, cycles))] | (rng.integers(1, 64, (n, cycles)) << 2).astype(np.uint8)).astype(np.uint8)


def _bytes(codes):
    return BYTE[np.asarray(codes)]


def _reference(reads, filts, index, max_tiles, k, combos):
    """-> (tiles, the finish's lane row, labels, {(max_d, max_family): the reference's result}), the identities checked"""
    n = reads[0].shape[0]
    tiles = _host_tiles(reads, filts, index)
    fin_lane, _, labels = _labels(tiles, n, max_tiles, k)
    want = {c: lane_consensus(tiles, n, max_tiles, labels, *c) for c in combos}
    for (d, mf), w in want.items():
        check_consensus_identities(*w, d, fin_lane, equality=k == 0)
    return tiles, fin_lane, labels, want


def _on_gpu(sc, reads, filts, index, max_tiles, k, want, calls=None, equality=None, extra=None):
    """One lane on the GPU: every combination of want against the reference and the identities; extra(ld) afterwards."""
    tb = _upload(sc, reads, filts)
    ld = _lane(sc, tb, index, max_tiles, calls or [list(range(len(reads)))])
    try:
        rows = _finish(ld, k)
        for (d, mf), w in want.items():
            got = ld.consensus(d, mf)
            _same(got, w)
            check_consensus_identities(*got, d, rows[0], equality=(k == 0) if equality is None else equality)
        if extra:
            extra(ld)
    finally:
        ld.close()
        tb.free()


# ---- 1: the small lane ------------------------------------------------------------------------------
@pytest.mark.parametrize("cycles", [37, 83])         # four words with a partial last one; nine words
@pytest.mark.parametrize("k", [0, 2])
def test_lane_consensus_matches_reference_however_the_tiles_are_fed(sc, k, cycles):
    reads, filts = _small_lane(k, cycles)
    combos = [(d, mf) for d in sorted({0, k, 7}) for mf in (3, 256)]
    tiles, fin_lane, labels, want = _reference(reads, filts, INDEX, MAX_TILES, k, combos)
    lane = want[(7, 256)][0]
    print("k %d cycles %d: lane row at max_d 7, max_family 256: %s" % (k, cycles, lane.tolist()))
    if k == 2:
        # the ground, as measured on the reference: families that vote, first wells that are off - the error the
        # mismatch pass misattributes -, a cycle without a majority, wells at d = 0, 1 and 2
        assert lane[FAMILIES] >= 50 and lane[FIRST_OFF] >= 30 and lane[UNDECIDED] >= 1, lane
        assert (lane[DIST:DIST + 3] > 0).all() and lane[PAIRS] > 100, lane
        assert want[(0, 256)][0][PROFILED] < want[(2, 256)][0][PROFILED] <= lane[PROFILED]
    else:
        assert lane[FAMILIES] >= 5 and lane[DIST] == lane[WELLS] and lane[MISMATCHES] == 0        # identity 9
    for d in sorted({0, k, 7}):
        assert want[(d, 3)][0][LARGE] > want[(d, 256)][0][LARGE] or k == 0                       # (the copies planted by equality are triples)
        assert want[(d, 3)][0][FAMILIES] > 0
        check_consensus_identities(*want[(d, 3)], d, fin_lane, wider=want[(d, 256)])              # identity 10
    check_consensus_identities(*want[(7, 256)], 7, fin_lane, lower=want[(0, 256)])
    tb = _upload(sc, reads, filts)
    try:
        for bits in (0, 1):
            for calls in WAYS.values():
                ld = _lane(sc, tb, INDEX, MAX_TILES, calls, hash_bits=bits)
                try:
                    rows = _finish(ld, k, bits)
                    for (d, mf), w in want.items():
                        got = ld.consensus(d, mf)
                        _same(got, w)
                        check_consensus_identities(*got, d, rows[0], equality=k == 0)
                finally:
                    ld.close()
    finally:
        tb.free()


# ---- 2: the direction -------------------------------------------------------------------------------
def test_the_direction_of_a_substitution(sc):
    """One tile of 2640 wells, 30 cycles, random reads, and 100 planted families of 5 identical wells at ascending
    wells; in family i the member i % 5 has one cycle changed from X to Y, the cycle and (X, Y) spread over the twelve
    ordered pairs.  The vote says X>Y in every family; the comparison with the first well says Y>X in the 20 families
    whose first well is the one that erred, four times each."""
    n, cycles, k = N, 30, 2
    rng = np.random.default_rng(2640)
    reads = [_random_reads(rng, n, cycles)]
    filts = [np.ones(n, dtype=np.uint8)]
    planted = np.zeros((cycles, 5, 5), dtype=np.int64)
    for i in range(100):
        wells = 26 * i + np.array([0, 5, 9, 14, 22])
        c, (x, y) = (7 * i) % cycles, PAIRS12[i % 12]
        base = rng.integers(0, 4, cycles)
        base[c] = x
        reads[0][wells] = _bytes(base)
        reads[0][wells[i % 5], c] = BYTE[y]
        planted[c, x, y] += 1
    assert len({(7 * i % cycles, i % 12) for i in range(100)}) >= 50 and (planted.sum(axis=0) >= 8)[tuple(zip(*PAIRS12))].all()
    assert not ((planted > 0) & (planted.transpose(0, 2, 1) > 0)).any()      # no cycle holds a pair and its reverse
    tiles, fin_lane, labels, want = _reference(reads, filts, [0], 1, k, [(0, 256), (2, 256)])
    lane, _, calls = want[(2, 256)]
    off = calls.copy()
    off[:, np.arange(5), np.arange(5)] = 0
    assert lane[FAMILIES] == 100 and lane[WELLS] == 500 and lane[MISMATCHES] == 100 and lane[FIRST_OFF] == 20
    assert (off == planted).all() and lane[UNDECIDED] == 0 and calls.sum() == 500 * cycles
    assert want[(0, 256)][0][PROFILED] == 400 and want[(0, 256)][0][DIST:DIST + 2].tolist() == [400, 100]

    def first_well_view(ld):
        m_lane, _, sub = ld.mismatches(2)
        reversed_ = np.zeros_like(planted)
        for i in range(0, 100, 5):                                     # the first well erred: its four copies "differ" from it
            reversed_[(7 * i) % cycles, PAIRS12[i % 12][1], PAIRS12[i % 12][0]] += 4
        forward = planted.copy()
        for i in range(0, 100, 5):
            forward[(7 * i) % cycles][PAIRS12[i % 12]] -= 1
        assert m_lane[2] == 80 + 4 * 20 == 160 and (sub == forward + reversed_).all()
        assert reversed_.sum() == 80 and (sub != planted).any()        # what the feature adds: calls is `planted` itself

    _on_gpu(sc, reads, filts, [0], 1, k, want, extra=first_well_view)


# ---- 3: ties and N ------------------------------------------------------------------------------------
def test_ties_no_calls_and_a_chain(sc):
    """One tile of 600 random reads of 30 cycles and five planted families (K = 2):
      wells 10..13   R, R, R', R' (cycle 3 changed): 2 / 2, undecided there and decided elsewhere;
      wells 20..24   R, R, R', R', R'' (cycle 4): 2 / 2 / 1;
      wells 30..32   A, C, G at cycle 5: three codes in three wells;
      wells 40..42   N, N, A at cycle 6: the consensus is N, the third well calls A;
      wells 50..58   five equal reads and a chain leading 2, 4, 6 and 8 cycles away: the five hold the majority at
                     every cycle, the last link lands in the open bin and is never profiled."""
    n, cycles, k = 600, 30, 2
    rng = np.random.default_rng(33)
    reads = [_random_reads(rng, n, cycles)]
    filts = [np.ones(n, dtype=np.uint8)]
    base = lambda: rng.integers(0, 4, cycles)
    put = lambda w, codes: reads[0].__setitem__(w, _bytes(codes))
    r = base()
    r[3] = 0
    for w, code in zip(range(10, 14), (0, 0, 1, 1)):
        put(w, np.where(np.arange(cycles) == 3, code, r))
    r = base()
    for w, code in zip(range(20, 25), (0, 0, 1, 1, 2)):
        put(w, np.where(np.arange(cycles) == 4, code, r))
    r = base()
    for w, code in zip(range(30, 33), (0, 1, 2)):
        put(w, np.where(np.arange(cycles) == 5, code, r))
    r = base()
    for w, code in zip(range(40, 43), (4, 4, 0)):
        put(w, np.where(np.arange(cycles) == 6, code, r))
    r = base()
    for w in range(50, 55):
        put(w, r)
    link = r.copy()
    for step, w in enumerate(range(55, 59)):
        for c in (2 * step + 10, 2 * step + 11):
            link[c] = (link[c] + 1) % 4
        put(w, link)
    combos = [(0, 256), (2, 256), (7, 256), (7, 4)]
    tiles, fin_lane, labels, want = _reference(reads, filts, [0], 1, k, combos)
    fams = {root: m.tolist() for root, m in families_of(labels)}
    assert [fams[w] for w in (10, 20, 30, 40, 50)] == [list(range(10, 14)), list(range(20, 25)), list(range(30, 33)),
                                                       list(range(40, 43)), list(range(50, 59))]
    lane, _, calls = want[(7, 256)]
    assert lane[FAMILIES] == len(fams) - int(lane[PAIRS]) and lane[UNDECIDED] == 3 and lane[LARGE] == 0
    assert calls[3].sum() == lane[PROFILED] - 4 and calls[4].sum() == lane[PROFILED] - 5 and calls[5].sum() == lane[PROFILED] - 3
    assert calls[6, 4].tolist() == [1, 0, 0, 0, 2] and lane[WITH_N] == 1
    assert lane[DIST:].tolist()[2:] == [1, 0, 1, 0, 1, 0, 1] and lane[PROFILED] == lane[WELLS] - 1      # d = 2, 4, 6 and the open bin
    assert want[(2, 256)][0][PROFILED] == lane[WELLS] - 3 and want[(7, 4)][0][LARGE_WELLS] == 5 + 9
    _on_gpu(sc, reads, filts, [0], 1, k, want)


# ---- 4: wave and cap boundaries -----------------------------------------------------------------------
def test_families_at_the_wave_and_at_the_cap(sc):
    """Three tiles of 8449 wells (a run of kLaneRun and a bit).  Families of 63, 64 and 65 wells with one erring member
    each and families of exactly 4096 and 4097 equal reads, every one spread over the three tiles and over both runs of
    a tile; a tenth of the other wells pass the filter.  max_family 64: the family of 65 is Large; 4096: the family
    of 4097 alone is."""
    n, cycles, k = 8449, 30, 1
    assert RUN < n < 2 * RUN
    rng = np.random.default_rng(4096)
    reads = [_random_reads(rng, n, cycles) for _ in range(3)]
    filts = [(rng.random(n) < 0.1).astype(np.uint8) for _ in range(3)]
    early = rng.permutation(np.concatenate([t * n + np.arange(RUN) for t in range(3)]))      # the first runs' wells
    late = [t * n + rng.permutation(np.arange(RUN, n)) for t in range(3)]                    # each tile's second run
    at = 0
    sizes = (63, 64, 65, 4096, 4097)
    for f, size in enumerate(sizes):
        wells = np.sort(np.concatenate([early[at:at + size - 6], [l[2 * f + j] for l in late for j in range(2)]]))
        at += size - 6
        base = rng.integers(0, 4, cycles)
        for j, g in enumerate(wells.tolist()):
            reads[g // n][g % n] = _bytes(base)
            filts[g // n][g % n] = 1
        if size < 100:                                                 # one member errs: the last but one
            g = int(wells[-2])
            reads[g // n][g % n, size % cycles] = BYTE[(base[size % cycles] + 1) % 4]
        assert len(set((wells // n).tolist())) == 3 and (wells % n >= RUN).any() and (wells % n < RUN).any()
    combos = [(1, 64), (1, 4096), (0, 4096)]
    tiles, fin_lane, labels, want = _reference(reads, filts, [0, 1, 2], 3, k, combos)
    got_sizes = sorted(m.size for _, m in families_of(labels) if m.size >= 60)
    assert got_sizes == list(sizes)
    small = sum(m.size for _, m in families_of(labels) if 3 <= m.size < 60)
    l64, l4096 = want[(1, 64)][0], want[(1, 4096)][0]
    assert l64[WELLS] == small + 63 + 64 and l64[LARGE] == 3 and l64[LARGE_WELLS] == 65 + 4096 + 4097
    assert l4096[WELLS] == small + 63 + 64 + 65 + 4096 and l4096[LARGE] == 1 and l4096[LARGE_WELLS] == 4097
    assert l64[MISMATCHES] >= 2 and l4096[MISMATCHES] == l64[MISMATCHES] + 1 and want[(0, 4096)][0][DIST + 1] >= 3
    check_consensus_identities(*want[(1, 64)], 1, fin_lane, wider=want[(1, 4096)])
    _on_gpu(sc, reads, filts, [0, 1, 2], 3, k, want, calls=[[2], [0, 1]])


# ---- 5: row geometry ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cycles", [9, 10, 25, 51, 151])      # rows of 1 (partial), 1 (full), 3, 6 and 16 words
def test_rows_of_every_geometry(sc, cycles):
    """Two tiles of 8449 wells at tile indices 1 and 2 of 3: with an odd number of words per row the tiles' first rows
    lie off a 16-byte boundary.  One well in twenty passes the filter (few enough that random reads of nine cycles
    seldom lie within one substitution of each other), and 120 planted families of 3, 4 and 5 wells spread over both
    tiles and both runs, one member of each with one cycle changed."""
    n, k = 8449, 1
    words = (cycles + 9) // 10
    rng = np.random.default_rng(8449 + cycles)
    reads = [_random_reads(rng, n, cycles) for _ in range(2)]
    filts = [(rng.random(n) < 0.05).astype(np.uint8) for _ in range(2)]
    free = rng.permutation(2 * n)
    at = 0
    for i in range(120):
        size = 3 + i % 3
        wells = free[at:at + size]
        at += size
        base = rng.integers(0, 4, cycles)
        for g in wells.tolist():
            reads[g // n][g % n] = _bytes(base)
            filts[g // n][g % n] = 1
        g, c = int(wells[i % size]), (11 * i) % cycles
        reads[g // n][g % n, c] = BYTE[(base[c] + 1 + i % 3) % 4]
    if words % 2:
        assert (n * words * 4) % 16 != 0 and (2 * n * words * 4) % 16 != 0
    tiles, fin_lane, labels, want = _reference(reads, filts, [1, 2], 3, k, [(0, 256), (1, 256), (7, 3)])
    lane, trow, calls = want[(1, 256)]
    assert lane[FAMILIES] >= 100 and lane[MISMATCHES] >= 100 and lane[FIRST_OFF] >= 15 and not trow[0].any()
    assert (trow[1:, 2] > 20).all() and (calls.sum(axis=(1, 2)) > 0).all() and want[(7, 3)][0][LARGE] >= 70
    _on_gpu(sc, reads, filts, [1, 2], 3, k, want)


def test_errors_on_both_sides_of_the_lds_window(sc):
    """One tile of 300 wells, 1024 cycles (rows of 103 words); 40 families of 3 with one member changed at one cycle,
    the cycles spread over the whole read: inside the window of the LDS histogram and beyond it."""
    n, cycles, k = 300, 1024, 2
    rng = np.random.default_rng(1024)
    reads = [_random_reads(rng, n, cycles)]
    filts = [np.ones(n, dtype=np.uint8)]
    at = []
    for i in range(40):
        base = rng.integers(0, 4, cycles)
        reads[0][6 * i:6 * i + 3] = _bytes(base)
        c = (i * 27 + 5) % cycles
        reads[0][6 * i + i % 3, c] = BYTE[(base[c] + 2) % 4]
        at.append(c)
    assert sum(c < WINDOW for c in at) >= 5 and sum(c >= WINDOW for c in at) >= 30 and max(at) > 1000
    tiles, fin_lane, labels, want = _reference(reads, filts, [0], 1, k, [(0, 256), (2, 256)])
    lane, _, calls = want[(2, 256)]
    off = calls.sum(axis=(1, 2)) - calls[:, np.arange(5), np.arange(5)].sum(axis=1)
    assert lane[FAMILIES] == 40 and lane[MISMATCHES] == 40 and sorted(np.flatnonzero(off).tolist()) == sorted(at)
    assert (calls.sum(axis=(1, 2)) == 120).all()
    _on_gpu(sc, reads, filts, [0], 1, k, want)


# ---- 6: degenerate lanes ------------------------------------------------------------------------------
def test_a_lane_of_equal_reads_is_one_large_family(sc):
    """Three tiles of 9000 equal reads: one family of every PF well, above any max_family - it is counted, and neither
    gathered nor walked: the call returns at once (it reads two words per well)."""
    n, cycles = 9000, 40
    read = BYTE[np.arange(cycles) % 4] | 4
    reads = [np.tile(read, (n, 1)) for _ in range(3)]
    filts = [np.ones(n, dtype=np.uint8) for _ in range(3)]
    for f in filts:
        f[::9] = 2                                                     # (only bit 0 counts: every ninth well fails)
    pf = 3 * int((filts[0] & 1).sum())
    combos = [(0, 256), (7, 4096)]
    tiles, fin_lane, labels, want = _reference(reads, filts, [0, 1, 2], 3, 0, combos)
    for w in want.values():
        assert w[0].tolist() == [0] * 9 + [1, pf] + [0] * 9 and not w[1].any() and not w[2].any()
    for k in (0, 1):
        _on_gpu(sc, reads, filts, [0, 1, 2], 3, k, want, equality=True)


def test_a_lane_without_a_group_and_a_lane_of_pairs(sc):
    n, cycles = 2000, 30
    rng = np.random.default_rng(30)
    reads = [_random_reads(rng, n, cycles) for _ in range(2)]
    filts = [(rng.random(n) < 0.9).astype(np.uint8) for _ in range(2)]
    tiles, fin_lane, labels, want = _reference(reads, filts, [1, 0], 2, 0, [(0, 256)])
    assert fin_lane[1] == 0 and fin_lane[0] > 3000 and not any(a.any() for a in want[(0, 256)])
    _on_gpu(sc, reads, filts, [1, 0], 2, 0, want, calls=[[0], [1]])
    reads[1][:] = reads[0]                                             # every read twice, on two tiles: pairs only
    filts[1][:] = filts[0]
    tiles, fin_lane, labels, want = _reference(reads, filts, [1, 0], 2, 0, [(0, 256), (3, 3)])
    pairs = int(filts[0].sum())
    for w in want.values():
        assert w[0].tolist() == [0] * 8 + [pairs, 0, 0] + [0] * 9 and not w[1].any() and not w[2].any()
    _on_gpu(sc, reads, filts, [1, 0], 2, 0, want)


# ---- 7: call discipline -----------------------------------------------------------------------------
def _raw(sc, ld, max_d, max_family, scratch, scratch_bytes, missing=None):
    """wd_lane_consensus itself -> (rc, lane row, tile rows, calls); missing: the output pointer passed as null"""
    out = [np.full(LANE_COLS, -1, dtype=np.int64), np.full((ld.max_tiles, TILE_COLS), -1, dtype=np.int64),
           np.full((ld.L, 5, 5), -1, dtype=np.int64)]
    ptr = [None if i == missing else a.ctypes.data_as(ctypes.c_void_p) for i, a in enumerate(out)]
    rc = sc._lib.wd_lane_consensus(ld._h, max_d, max_family, ctypes.c_void_p(scratch), scratch_bytes, *ptr)
    return (rc,) + tuple(out)


def _untouched(res):
    return all((a == -1).all() for a in res[1:])


def _tables_of(tb, slots):
    ptrs = tb.plane_ptrs()
    return Scanner._tables([ptrs[s] for s in slots], [tb.filter_ptr(s) for s in slots], tb.L)


def test_call_discipline(sc):
    k, cycles, d, mf = 2, 37, 2, 256
    reads, filts = _small_lane(k, cycles)
    tiles = _host_tiles(reads, filts, INDEX)
    want = lane_consensus(tiles, N, MAX_TILES, lane_near_dups(tiles, N, MAX_TILES, k)[2], d, mf)
    want_eq = lane_consensus(tiles, N, MAX_TILES, lane_dups(tiles, N, MAX_TILES)[2], d, mf)
    assert want[0][MISMATCHES] > 50 and want_eq[0][FAMILIES] >= 5 and want_eq[0][MISMATCHES] == 0
    need = sc.lane_consensus_scratch_bytes(MAX_TILES, N, cycles)
    d_scratch = sc.malloc(need)
    sc.memset(d_scratch, 0xA5, need)                                   # whatever it holds: nothing is assumed of it
    host = np.zeros(need, dtype=np.uint8)
    tb = _upload(sc, reads, filts)
    x, y = synth.honeycomb_pixels(44, 60)
    ld = _lane(sc, tb, INDEX, MAX_TILES, WAYS["2 + 3"])
    try:
        res = _raw(sc, ld, d, mf, d_scratch, need)                     # before any finish
        assert res[0] == _lib.ERR_ARG and _untouched(res)
        assert b"lane consensus comes after a successful finish of the lane" in sc._lib.wd_last_error(sc._ctx)
        with pytest.raises(ValueError):
            ld.consensus(d, mf)
        with pytest.raises(RuntimeError):                              # a near finish refused over budget is no finish
            ld.finish(hamming=k, pair_budget=3)
        res = _raw(sc, ld, d, mf, d_scratch, need)
        assert res[0] == _lib.ERR_ARG and _untouched(res) and b"finish" in sc._lib.wd_last_error(sc._ctx)
        rows = _finish(ld, k)
        for bad in ((-1, mf, d_scratch, need), (8, mf, d_scratch, need), (d, 2, d_scratch, need), (d, 4097, d_scratch, need),
                    (d, mf, 0, need), (d, mf, d_scratch, need - 1), (d, mf, d_scratch, 0), (d, mf, host.ctypes.data, need)):
            res = _raw(sc, ld, *bad)
            assert res[0] == _lib.ERR_ARG and _untouched(res), bad
        for missing in range(3):
            res = _raw(sc, ld, d, mf, d_scratch, need, missing=missing)
            assert res[0] == _lib.ERR_ARG and _untouched(res)
        for bad in ((-1, mf), (8, mf), (d, 2), (d, 4097)):
            with pytest.raises(ValueError):
                ld.consensus(*bad)
        first = _raw(sc, ld, d, mf, d_scratch, need)                   # the caller's scratch, dirty from nothing
        assert first[0] == _lib.OK
        _same(first[1:], want)
        _same(_raw(sc, ld, d, mf, d_scratch, need)[1:], want)          # twice in a row, on the scratch the first call left
        _same(_raw(sc, ld, 0, 3, d_scratch, need)[1:], lane_consensus(tiles, N, MAX_TILES, lane_near_dups(tiles, N, MAX_TILES, k)[2], 0, 3))
        _same(_raw(sc, ld, d, mf, d_scratch, need)[1:], want)          # and on the scratch another max_family left
        _same(ld.consensus(d, mf), want)
        before = ld.mismatches(k), ld.top(20), ld.distances(x, y, 100), ld.gc(1)
        _same(ld.consensus(d, mf), want)                               # after mismatches, top, distances and gc
        again = ld.mismatches(k), ld.top(20), ld.distances(x, y, 100), ld.gc(1)      # which find the accumulator as they left it
        for a, b in zip(before, again):
            assert all(np.array_equal(u, v) for u, v in zip(a, b))
        check_consensus_identities(*ld.consensus(d, mf), d, rows[0])
        # another lane in the same workspace, by equality; and one without a tile: zeros
        ld.restart()
        with pytest.raises(ValueError):
            ld.consensus(d, mf)
        for slots in WAYS["descending indices"]:
            ld.add_tables([INDEX[s] for s in slots], _tables_of(tb, slots))
        rows = _finish(ld, 0)
        got = ld.consensus(d, mf)
        _same(got, want_eq)
        check_consensus_identities(*got, d, rows[0], equality=True)
        ld.restart()
        _finish(ld, 0)
        res = _raw(sc, ld, 0, mf, d_scratch, need)
        assert res[0] == _lib.OK and not any(a.any() for a in res[1:])
        ld.close()
        with pytest.raises(ValueError):
            ld.consensus(d, mf)
    finally:
        ld.close()
        tb.free()
        sc.free(d_scratch)


# ---- 8: the CLI -------------------------------------------------------------------------------------
def _main(argv):
    out = io.StringIO()
    with redirect_stdout(out):
        assert cwd.main(argv) == 0
    return out.getvalue()


def test_cli_lane_consensus_block(tmp_path):
    """The run directory of test_gpu_lanegc.py's CLI test: tile 1103's files are tile 1101's but for the last cycle,
    which is tile 1102's.  The new block closes the lane's output, equals write_lane_consensus of the reference's
    counts and is all the flag adds, also under another --tile-batch; with --lane-dups-hamming it is on the clusters,
    after every other pass; the TSV is write_lane_consensus_tsv of the same counts."""
    rows, cols, levels, L, lane = 36, 70, 3, 24, 1
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
            "--cycles", "0-%d" % L, "-q", "--all-wells", "--lane-dups"]
    tiles = [(i, [synth.plane_bytes(spec, lane, int(source(t, c)), c) for c in range(L)],
              synth.filter_bytes(spec, lane, int(t if t != "1103" else "1101"))) for i, t in enumerate(names)]
    finish = {0: lane_dups(tiles, n, 4), 2: lane_near_dups(tiles, n, 4, 2)}

    def block(k, max_d, max_family, summary):
        counts = report.LaneConsensusCounts.from_rows(*lane_consensus(tiles, n, 4, finish[k][2], max_d, max_family), names, k,
                                                      max_d, max_family, int(finish[k][0][0]), list(range(L)))
        text, tsv = io.StringIO(), io.StringIO()
        report.write_lane_consensus(str(lane), counts, verbose=not summary, out=text)
        report.write_lane_consensus_tsv(str(lane), counts, tsv)
        return text.getvalue(), tsv.getvalue(), counts

    plain = _main(argv)
    want, tsv, counts = block(0, 0, 256, False)
    assert counts.families >= 40 and counts.pairs > 300 and counts.mismatches == 0
    assert want.count("LaneConsensus: 1\tTile: ") == 4 and want.count("LaneConsensus: 1\tCycle: ") == L
    assert "LaneConsensusSummary: 1\tTiles: 4\tHamming: 0\tMaxD: 0\tMaxFamily: 256\t" in want
    out_file = str(tmp_path / "consensus.tsv")
    got = _main(argv + ["--tile-batch", "1", "--lane-dups-consensus", "--lane-dups-consensus-out", out_file])
    assert got == plain + want                                         # the new block is all the flag adds
    assert "".join(line for line in got.splitlines(True)
                   if not line.startswith(("LaneConsensus", "Consensus"))).rstrip("\n") == plain.rstrip("\n")
    assert open(out_file).read() == tsv
    # on the clusters, after every other pass of the lane, the summary alone, another max_d and max_family
    others = ["--lane-dups-hamming", "2", "-S", "--lane-dups-mismatches", "--lane-dups-distance", "--lane-dups-top", "5",
              "--lane-dups-gc"]
    want, tsv, counts = block(2, 1, 5, True)
    assert counts.mismatches >= 30 and counts.undecided > 20 and counts.large > 0 and counts.dist[2] == 0
    assert block(2, 2, 256, True)[2].dist[2] > 0                       # (the default max_d = K would let that well in)
    out_file = str(tmp_path / "consensus2.tsv")
    got = _main(argv + others + ["--lane-dups-consensus", "--lane-dups-consensus-max-d", "1",
                                 "--lane-dups-consensus-max-family", "5", "--lane-dups-consensus-out", out_file])
    assert got == _main(argv + others) + want and open(out_file).read() == tsv
    assert "LaneConsensus: 1\t" not in want and "\tHamming: 2\tMaxD: 1\tMaxFamily: 5\t" in want
