"""A lane's duplication per index read on the GPU (LaneDups.index_begin / index_add / index_finish,
include/welldup_laneindex.h) against the host reference of tests/laneindex_ref.py - the lane index row, the Other row,
the listed groups' rows and their keys equal, nothing approximate - however the tiles and their index planes are fed,
on the classes and on the clusters."""
import ctypes
import gzip
import io
import math
import os
import time
from contextlib import redirect_stdout

import numpy as np
import pytest

from contention_inputs import LI_PROBE, li_home, probe_edge_index
from laneindex_ref import check_index_identities, index_keys, key_of, lane_index
from lanedups_ref import lane_dups
from lanenear_ref import lane_near_dups
from tiledups_ref import INVALID
from well_duplicates_amd import _lib
from well_duplicates_amd import count_well_duplicates as cwd
from well_duplicates_amd import report, synth, workload
from well_duplicates_amd.scanner import LaneDups, Scanner, TileBatch

pytestmark = pytest.mark.gpu

ROWS, COLS, L = 44, 60, 40
N = ROWS * COLS
INDEX = [5, 0, 3, 6, 1]                                               # slot -> tile index in a lane of MAX_TILES
MAX_TILES = 7                                                         # (indices 2 and 4 are never added)
DEAD = 1                                                              # the slot of the tile without a PF well


@pytest.fixture(scope="module")
def sc():
    s = Scanner(0)
    yield s
    s.close()


def _upload(sc, reads, filts=None):
    """reads: per tile uint8 [n, cycles] (well, cycle); -> a resident TileBatch (filters of ones if none are given)"""
    n, cycles = reads[0].shape
    tb = TileBatch(sc, len(reads), cycles, n)
    for i, r in enumerate(reads):
        tb.upload_tile(i, [np.ascontiguousarray(r[:, c]) for c in range(cycles)],
                       filts[i] if filts is not None else np.ones(n, dtype=np.uint8))
    return tb


def _tables(tb, slots, shift=0, cycles=None):
    ptrs = tb.plane_ptrs()
    cycles = range(tb.L) if cycles is None else cycles
    return Scanner._tables([[ptrs[s][c] + shift for c in cycles] for s in slots], [tb.filter_ptr(s) + shift for s in slots],
                           len(cycles))


def _planes(tb, slots=None, cycles=None):
    slots = range(tb.n_tiles) if slots is None else slots
    cycles = range(tb.L) if cycles is None else cycles
    return [[tb.download_plane(s, c) for c in cycles] for s in slots]


def _reference(tb, itb, index, max_tiles, hamming=0, min_pf=1, index_cycles=None):
    """The host reference from the bytes resident on the GPU -> (lane row of the labels, labels, index result)."""
    tiles = [(index[s], p, tb.download_filter(s)) for s, p in enumerate(_planes(tb))]
    itiles = [(index[s], p) for s, p in enumerate(_planes(itb, cycles=index_cycles))]
    if hamming:
        lane, _, labels = lane_near_dups(tiles, tb.N, max_tiles, hamming)
    else:
        lane, _, labels = lane_dups(tiles, tb.N, max_tiles)
    return lane, labels, itiles, lane_index(itiles, labels, tb.N, max_tiles, min_pf)


def _feed(sc, tb, itb, index, max_tiles, ops, hash_bits=0, hamming=0, finishes=((1, 1 << 16),), index_cycles=None, I=None):
    """ops: [("add" | "index", [batch slots])], one call each; then the finish, then an index_finish per entry of
    finishes -> (what finish returned, [what each index_finish returned])"""
    ld = LaneDups(sc, tb.N, max_tiles, tb.L, hash_bits=hash_bits)
    try:
        ld.index_begin(I or (len(index_cycles) if index_cycles is not None else itb.L))
        for what, slots in ops:
            if what == "add":
                ld.add_tables([index[s] for s in slots], _tables(tb, slots))
            else:
                ld.index_add(_tables(itb, slots, cycles=index_cycles), [index[s] for s in slots])
        got = ld.finish(labels=True, hamming=hamming)
        return got, [ld.index_finish(min_pf, cap) for min_pf, cap in finishes]
    finally:
        ld.close()


def _same(got, want):
    for g, w, name in zip(got, want, ("lane index row", "Other", "group rows", "keys")):
        assert np.asarray(g).shape == np.asarray(w).shape and (np.asarray(g) == np.asarray(w)).all(), (name, g, w)


def _pooled_lane(seed=23, n=N, cycles=L, I=8, n_tiles=5, libraries=12, dead=DEAD, near=False):
    """A lane of n_tiles tiles (one of them without a PF well) whose wells come from `libraries` libraries of skewed
    shares.  A few per cent of the index reads carry one random error, some an N.  Reads are copied within a library
    on one tile, within a library across tiles, and across libraries (the read without its index); near: copies at
    one and two mismatches too.  -> (reads, filters, index reads), per tile [n, cycles] / [n] / [n, I]."""
    rng = np.random.default_rng(seed)
    reads = [rng.integers(1, 256, (n, cycles)).astype(np.uint8) for _ in range(n_tiles)]
    lib = rng.integers(1, 256, (libraries, I)).astype(np.uint8)
    share = 0.6 ** np.arange(libraries) + 0.01
    idx = []
    for r in reads:
        r[rng.random(r.shape) < 0.004] = 0
        x = lib[rng.choice(libraries, n, p=share / share.sum())]
        x = (x & 3) | (rng.integers(1, 64, x.shape).astype(np.uint8) << 2)             # the same bases, other quality bits
        err, col = rng.random(n) < 0.04, rng.integers(0, I, n)
        x[err, col[err]] = ((x[err, col[err]] + rng.integers(1, 4, int(err.sum()))) & 3) | 8
        x[rng.random(x.shape) < 0.003] = 0
        idx.append(x)
    for src, dst, count, same_library in ((0, 0, 200, True), (2, 2, 150, True), (0, 2, 300, True), (2, 3, 200, True),
                                          (0, 4, 150, False), (3, 4, 100, False), (3, 3, 80, False), (0, 3, 60, True)):
        src, dst = src % n_tiles, dst % n_tiles
        a, b = rng.choice(n, count, replace=False), rng.choice(n, count, replace=False)
        reads[dst][b] = reads[src][a]                                  # (chains: a copy of a copy)
        if same_library:
            idx[dst][b] = idx[src][a]
    if near:
        for src, dst, count, d in ((0, 2, 200, 1), (2, 4, 150, 2), (3, 3, 100, 1), (4, 0, 100, 2)):
            src, dst = src % n_tiles, dst % n_tiles
            a, b = rng.choice(n, count, replace=False), rng.choice(n, count, replace=False)
            reads[dst][b] = reads[src][a]
            for _ in range(d):
                col = rng.integers(0, cycles, count)
                reads[dst][b, col] = (reads[dst][b, col] & 0xFC) | ((reads[dst][b, col] + 1) & 3) | 4
    filts = [(rng.random(n) < 0.9).astype(np.uint8) | (rng.integers(0, 2, n).astype(np.uint8) << 1) for _ in range(n_tiles)]
    if dead is not None:
        filts[dead][:] = 2                                             # (only bit 0 counts)
    return reads, filts, idx


ALL = [0, 1, 2, 3, 4]
WAYS = {
    "one call each": [("add", ALL), ("index", ALL)],
    "index first, a tile per call": [("index", [s]) for s in ALL] + [("add", ALL)],
    "2 + 3": [("add", [0, 1]), ("index", [0, 1]), ("add", [2, 3, 4]), ("index", [2, 3, 4])],
    "descending indices": [("add", ALL)] + [("index", [s]) for s in (3, 0, 2, 4, 1)],
    "one call, descending": [("index", [3, 0, 2, 4, 1]), ("add", [3, 0, 2, 4, 1])],
    "interleaved differently from add": [("index", [4, 0]), ("add", [1]), ("add", [0, 2, 3]), ("index", [2]), ("add", [4]),
                                         ("index", [3, 1])],
}


def test_lane_index_matches_reference_however_the_tiles_are_fed(sc):
    reads, filts, idx = _pooled_lane()
    tb, itb = _upload(sc, reads, filts), _upload(sc, idx)
    try:
        eq_lane, labels, itiles, want = _reference(tb, itb, INDEX, MAX_TILES, min_pf=20)
        lane, other, rows, keys = want
        check_index_identities(want, eq_lane)
        # twelve libraries and the keys with an error or an N around them; classes inside a library and across two
        assert 12 <= lane[1] <= 14 and lane[0] > 150 and other[0] > 100 and lane[3] > 150 and rows[:, 3].sum() > 300
        assert rows[0, 0] > 10 * rows[11, 0] and rows[:, 4].sum() > 300 and (rows[:12, 2] > 0).sum() >= 6
        assert np.isin(index_keys(itiles, N, MAX_TILES)[0][INDEX[DEAD] * N:(INDEX[DEAD] + 1) * N], keys).sum() > N // 2
        assert (labels[INDEX[DEAD]] == INVALID).all() and (labels[[2, 4]] == INVALID).all()
        everything = lane_index(itiles, labels, N, MAX_TILES, 1)
        assert everything[0][1] == everything[0][0] == lane[0] and not everything[1].any()
        for bits in (0, 4, 1):
            for name, ops in WAYS.items():
                if bits and name not in ("one call each", "interleaved differently from add"):
                    continue
                got, (listed, full) = _feed(sc, tb, itb, INDEX, MAX_TILES, ops, hash_bits=bits,
                                            finishes=((20, 64), (1, 1 << 16)))
                assert (got[0] == eq_lane).all() and (got[2] == labels).all(), name
                _same(listed, want)
                _same(full, everything)
    finally:
        tb.free()
        itb.free()


@pytest.mark.parametrize("I", [1, 8, 10, 11, 16, 20])
def test_lane_index_shapes(sc, I):
    """Keys of one word, of exactly one, of one and a cycle, of two; tiles of 1001 wells (the last well goes through
    the tail of k_li_pack) and index planes that start on an odd address; index cycles disjoint from the scanned
    ones, inside them, and equal to them."""
    n, cycles = 1001, 24
    reads, filts, idx = _pooled_lane(seed=100 + I, n=n, cycles=cycles, I=I, n_tiles=3, libraries=5, dead=None)
    tb, itb = _upload(sc, reads, filts), _upload(sc, idx)
    index, ops = [2, 0, 1], [("index", [1]), ("add", [0, 1, 2]), ("index", [2, 0])]
    try:
        # disjoint from the scanned cycles
        eq_lane, labels, itiles, want = _reference(tb, itb, index, 3, min_pf=10)
        check_index_identities(want, eq_lane)
        assert want[0][3] > 20 and want[0][1] >= 4 and want[1][0] > 0
        for bits in (0, 1):
            _same(_feed(sc, tb, itb, index, 3, ops, hash_bits=bits, finishes=((10, 1001),))[1][0], want)
        # inside the scanned cycles: the index planes ARE scanned planes, and no class is mixed
        inside = list(range(2, 2 + I))
        eq_lane, labels, _, want_in = _reference(tb, tb, index, 3, min_pf=1, index_cycles=inside)
        check_index_identities(want_in, eq_lane)
        assert want_in[0][3] == 0 and want_in[0][4] == 0 and not want_in[2][:, 4].any() and want_in[0][2] == eq_lane[1]
        _same(_feed(sc, tb, tb, index, 3, ops, index_cycles=inside)[1][0], want_in)
        # the same tiles less their first well: every plane starts one byte after a 256-byte boundary
        tiles1 = [(i, [p[1:] for p in planes], tb.download_filter(s)[1:]) for i, (s, planes) in enumerate(zip(range(3), _planes(tb)))]
        itiles1 = [(i, [p[1:] for p in planes]) for i, planes in enumerate(_planes(itb))]
        lane1, _, labels1 = lane_dups(tiles1, n - 1, 3)
        want1 = lane_index(itiles1, labels1, n - 1, 3, 3)
        ld = LaneDups(sc, n - 1, 3, cycles)
        try:
            ld.index_begin(I)
            ld.add_tables([0, 1, 2], _tables(tb, [0, 1, 2], shift=1))
            ld.index_add(_tables(itb, [0, 1, 2], shift=1), [0, 1, 2])
            assert (ld.finish()[0] == lane1).all()
            _same(ld.index_finish(3), want1)
        finally:
            ld.close()
    finally:
        tb.free()
        itb.free()


def test_lane_index_on_the_scanned_cycles_themselves(sc):
    """Index cycles equal to the scanned cycles: a group is a distinct read, every class is one subgroup."""
    reads, filts, _ = _pooled_lane(seed=5, n=1500, cycles=12, I=4, n_tiles=3, libraries=3, dead=None)
    tb = _upload(sc, reads, filts)
    try:
        eq_lane, labels, _, want = _reference(tb, tb, [0, 1, 2], 3, min_pf=2)
        lane, other, rows, keys = want
        check_index_identities(want, eq_lane)
        assert lane[0] == eq_lane[0] - eq_lane[3] and lane[1] == lane[2] == eq_lane[1] > 100 and lane[3] == 0
        assert (rows[:, 0] == rows[:, 1]).all() and (rows[:, 0] == rows[:, 2]).all() and (rows[:, 3] == rows[:, 0] - 1).all()
        assert other.tolist() == [eq_lane[0] - eq_lane[2], 0, 0, 0, 0]
        _same(_feed(sc, tb, tb, [0, 1, 2], 3, [("add", [0, 1, 2]), ("index", [0, 1, 2])], finishes=((2, 4500),))[1][0], want)
    finally:
        tb.free()


@pytest.mark.parametrize("k", [1, 2])
def test_lane_index_after_the_near_finish(sc, k):
    n = 700
    reads, filts, idx = _pooled_lane(seed=40 + k, n=n, cycles=30, I=8, n_tiles=5, near=True)
    tb, itb = _upload(sc, reads, filts), _upload(sc, idx)
    try:
        near_lane, near_labels, itiles, want = _reference(tb, itb, INDEX, MAX_TILES, hamming=k, min_pf=8)
        eq_lane, eq_labels, _, want_eq = _reference(tb, itb, INDEX, MAX_TILES, min_pf=8)
        check_index_identities(want, near_lane)
        # clusters reach further than classes: more wells in them, more of them mixed
        assert want[2][:, 1].sum() > want_eq[2][:, 1].sum() + 100 and want[0][3] > want_eq[0][3] + 20
        assert near_lane[6] > 200 and 12 <= want[0][1] <= 16
        for bits in (0, 1):
            got, (res,) = _feed(sc, tb, itb, INDEX, MAX_TILES, WAYS["2 + 3"], hash_bits=bits, hamming=k, finishes=((8, 100),))
            assert (got[3] == near_lane).all() and (got[5] == near_labels).all() and (got[2] == eq_labels).all()
            _same(res, want)
        if k == 1:
            # K = 0 through the near finish gives the rows of the equality finish
            ld = LaneDups(sc, n, MAX_TILES, 30)
            try:
                ld.index_begin(8)
                ld.add_tables([INDEX[s] for s in ALL], _tables(tb, ALL))
                ld.index_add(itb, [INDEX[s] for s in ALL])
                lane_row = np.zeros(_lib.LANEDUPS_LANE_COLS, dtype=np.int64)
                tile_rows = np.zeros((MAX_TILES, 5), dtype=np.int64)
                near_row = np.zeros(_lib.LANENEAR_LANE_COLS, dtype=np.int64)
                p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
                sc._ck(sc._lib.wd_lane_near_dups_finish(ld._h, 0, None, 0, 0, p(lane_row), p(tile_rows), None, p(near_row),
                                                        p(tile_rows.copy()), None))
                assert (lane_row == eq_lane).all() and near_row[6] == 0
                _same(ld.index_finish(8, 100), want_eq)
            finally:
                ld.close()
    finally:
        tb.free()
        itb.free()


def test_single_index_lanes(sc, capsys):
    """One index read on the whole lane: one row [PF, InClasses, InClasses, Redundant, 0].  Then the hottest case:
    every read equal too - one class, one group, every counter on one row.  It must finish; its time is printed."""
    reads, filts, _ = _pooled_lane(seed=8, n_tiles=3, dead=None)
    one = [np.tile(np.array([0x42 + 4 * (c % 3) for c in range(8)], dtype=np.uint8), (N, 1)) for _ in range(3)]
    for x in one:
        x[::7] ^= 0xF0                                                 # (quality bits do not matter)
    tb, itb = _upload(sc, reads, filts), _upload(sc, one)
    try:
        eq_lane, labels, _, want = _reference(tb, itb, [0, 1, 2], 3)
        assert want[0].tolist() == [1, 1, eq_lane[1], 0, 0] and want[3].tolist() == [key_of("G" * 8)]
        assert want[2].tolist() == [[eq_lane[0], eq_lane[2], eq_lane[2], eq_lane[3], 0]] and eq_lane[3] > 300
        check_index_identities(want, eq_lane)
        for bits in (0, 1):
            _same(_feed(sc, tb, itb, [0, 1, 2], 3, [("add", [0, 1, 2]), ("index", [0, 1, 2])], hash_bits=bits)[1][0], want)
    finally:
        tb.free()
    equal = [np.tile(np.array([0x42 + (c % 4) for c in range(L)], dtype=np.uint8), (N, 1)) for _ in range(3)]
    tb = _upload(sc, equal, filts)
    try:
        total = int(sum((f & 1).sum() for f in filts))
        t0 = time.perf_counter()
        got, (res,) = _feed(sc, tb, itb, [0, 1, 2], 3, [("add", [0, 1, 2]), ("index", [0, 1, 2])])
        with capsys.disabled():
            print("\nevery read and every index equal, 3 x %d wells: %.1f ms" % (N, (time.perf_counter() - t0) * 1e3))
        assert got[0][:4].tolist() == [total, 1, total, total - 1]
        assert res[0].tolist() == [1, 1, 1, 0, 0] and not res[1].any()
        assert res[2].tolist() == [[total, total, total, total - 1, 0]] and res[3].tolist() == [key_of("G" * 8)]
    finally:
        tb.free()
        itb.free()


def test_more_groups_than_the_lds_table_holds(sc):
    """Uniform random index reads of 8 cycles: a workgroup's run of wells meets thousands of distinct keys, far more
    than its LDS table holds, and the adds that find it full go to memory.  Then a lane on which every key is unique:
    with min_pf = 2 everything lands in Other and Groups = PF."""
    rng = np.random.default_rng(77)
    n, tiles = 20000, 3
    reads, filts, _ = _pooled_lane(seed=9, n=n, cycles=16, n_tiles=tiles, dead=None)
    idx = [rng.integers(0, 256, (n, 8)).astype(np.uint8) for _ in range(tiles)]
    tb, itb = _upload(sc, reads, filts), _upload(sc, idx)
    try:
        eq_lane, labels, itiles, want = _reference(tb, itb, [0, 1, 2], tiles, min_pf=3)
        check_index_identities(want, eq_lane)
        run = index_keys(itiles, n, tiles)[0][:8192]
        assert np.unique(run).size > 4 * 512                           # one workgroup's run of wells
        assert want[0][0] > 30000 and want[0][1] > 1000 and want[1][0] > 10000 and want[0][3] > 100
        _same(_feed(sc, tb, itb, [0, 1, 2], tiles, [("add", [0, 1, 2]), ("index", [0, 1, 2])], finishes=((3, 60000),))[1][0],
              want)
    finally:
        itb.free()
    # every key unique: the global id in base 4 over 10 cycles, then its low digits again
    gid = np.arange(tiles * n)
    digits = np.stack([(gid >> (2 * c)) & 3 for c in range(10)] + [(gid >> (2 * c)) & 3 for c in range(2)], axis=1)
    uniq = (digits | 0x40).astype(np.uint8).reshape(tiles, n, 12)
    itb = _upload(sc, [uniq[t] for t in range(tiles)])
    try:
        eq_lane, labels, _, want = _reference(tb, itb, [0, 1, 2], tiles, min_pf=2)
        pf = int(eq_lane[0])
        assert want[0].tolist() == [pf, 0, eq_lane[2], eq_lane[1], eq_lane[2]] and want[2].shape == (0, 5)
        assert want[1].tolist() == [pf, eq_lane[2], 0, 0, eq_lane[2]]
        got, (res, res1) = _feed(sc, tb, itb, [0, 1, 2], tiles, [("index", [0, 1, 2]), ("add", [0, 1, 2])],
                                 finishes=((2, 0), (1, tiles * n)))
        _same(res, want)
        assert res1[0][1] == pf and (res1[2][:, 0] == 1).all() and np.unique(res1[3]).size == pf
    finally:
        tb.free()
        itb.free()


def _copied_reads(seed, n, cycles, tiles=2, copies=1500):
    """random reads, `copies` of them copied to other wells of the lane: classes of two and a few larger ones"""
    rng = np.random.default_rng(seed)
    reads = rng.integers(1, 256, (tiles * n, cycles)).astype(np.uint8)
    reads[rng.integers(0, tiles * n, copies)] = reads[rng.integers(0, tiles * n, copies)]
    return [reads[t * n:(t + 1) * n] for t in range(tiles)]


@pytest.mark.parametrize("I", [8, 20])
def test_groups_that_share_a_home_entry_of_the_lds_table(sc, I):
    """As many groups as a probe path of k_li_tally's table is long, one more and four more, their representatives all
    beginning at one entry (tests/contention_inputs.py; tests/test_laneindex_emu.py holds its copy of the home entry
    against the kernel's): the last group that comes finds the path's last entry, or none and adds to memory."""
    n = 9000
    reads = _copied_reads(50 + I, n, 12)
    tb = _upload(sc, reads)                                            # (the filters come with each lane of index reads)
    try:
        for extra in (0, 1, 4):
            idx, filts, reps, slot = probe_edge_index(300 + extra, n, I, LI_PROBE + extra)
            assert (li_home(reps) == slot).all() and reps.size == LI_PROBE + extra
            for s in range(2):
                sc.h2d(tb.filter_ptr(s), filts[s])
            itb = _upload(sc, idx)
            try:
                eq_lane, labels, itiles, want = _reference(tb, itb, [0, 1], 2)
                check_index_identities(want, eq_lane)
                assert want[0][0] == want[0][1] == LI_PROBE + extra and want[0][3] > 500 and (want[2][:, 0] > 500).all()
                got, (res,) = _feed(sc, tb, itb, [0, 1], 2, [("add", [0, 1]), ("index", [0, 1])])
                assert (got[0] == eq_lane).all() and (got[2] == labels).all()
                _same(res, want)
            finally:
                itb.free()
    finally:
        tb.free()


@pytest.mark.parametrize("n", [8192, 8193])
def test_a_run_of_one_group_and_one_class_fills_the_fields(sc, n):
    """One index read, every well PF, every read equal: a workgroup of k_li_tally adds a whole run of 8192 wells into
    each 16-bit field of one entry.  After the equality finish and after the near finish at K = 1."""
    equal = [np.tile(np.array([0x42 + (c % 4) for c in range(12)], dtype=np.uint8), (n, 1)) for _ in range(2)]
    one = [np.tile(np.array([0x41 + 4 * (c % 5) for c in range(8)], dtype=np.uint8), (n, 1)) for _ in range(2)]
    tb, itb = _upload(sc, equal), _upload(sc, one)
    try:
        total = 2 * n
        for k in (0, 1):
            lane_row, labels, _, want = _reference(tb, itb, [0, 1], 2, hamming=k)
            assert (labels == 0).all()
            assert want[0].tolist() == [1, 1, 1, 0, 0] and not want[1].any() and want[3].tolist() == [key_of("C" * 8)]
            assert want[2].tolist() == [[total, total, total, total - 1, 0]]
            got, (res,) = _feed(sc, tb, itb, [0, 1], 2, [("add", [0, 1]), ("index", [0, 1])], hamming=k)
            assert (got[5 if k else 2] == labels).all()
            _same(res, want)
    finally:
        tb.free()
        itb.free()


def test_min_pf_and_cap(sc):
    reads, filts, idx = _pooled_lane(seed=61)
    tb, itb = _upload(sc, reads, filts), _upload(sc, idx)
    ld = LaneDups(sc, N, MAX_TILES, L)
    try:
        eq_lane, labels, itiles, _ = _reference(tb, itb, INDEX, MAX_TILES)
        ld.index_begin(8)
        ld.index_add(itb, INDEX)
        ld.add(tb, INDEX)
        assert (ld.finish()[0] == eq_lane).all()
        wants = {m: lane_index(itiles, labels, N, MAX_TILES, m) for m in (0, 1, 2, 5, 50, 400, 2000, 10 ** 7)}
        assert len({w[0][1] for w in wants.values()}) >= 6 and wants[10 ** 7][0][1] == 0 and wants[2000][0][1] in (1, 2, 3)
        for _ in range(2):                                             # repeatable, in any order of min_pf
            for m in (50, 1, 10 ** 7, 2, 400, 0, 5, 2000):
                _same(ld.index_finish(m, max(1, int(wants[m][0][1]))), wants[m])
                check_index_identities(wants[m], eq_lane)
        # one group too many for the cap: refused with the count, nothing delivered
        listed = int(wants[5][0][1])
        with pytest.raises(RuntimeError) as e:
            ld.index_finish(5, listed - 1)
        assert str(e.value).startswith(_lib.strerror(_lib.ERR_UNSUPPORTED)) and "%d groups" % listed in str(e.value)
        assert ld.index_listed == listed
        lane_row, other = np.full(5, -7, dtype=np.int64), np.full(5, -7, dtype=np.int64)
        rows, keys = np.full((listed, 5), -7, dtype=np.int64), np.full(listed, 7, dtype=np.uint64)
        count = ctypes.c_int64(-1)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rc = sc._lib.wd_lane_index_finish(ld._h, 5, listed - 1, p(lane_row), p(other), p(rows), p(keys), ctypes.byref(count))
        assert rc == _lib.ERR_UNSUPPORTED and count.value == listed
        assert (lane_row == -7).all() and (other == -7).all() and (rows == -7).all() and (keys == 7).all()
        with pytest.raises(RuntimeError):
            ld.index_finish(1, 0)
        _same(ld.index_finish(5, listed), wants[5])                    # and the lane is as it was
    finally:
        ld.close()
        tb.free()
        itb.free()


def test_lane_index_errors_leave_the_lane_as_it_was(sc):
    reads, filts, idx = _pooled_lane(seed=62)
    tb, itb = _upload(sc, reads, filts), _upload(sc, idx)
    il = None
    ld = LaneDups(sc, N, MAX_TILES, L)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    try:
        eq_lane, labels, itiles, want = _reference(tb, itb, INDEX, MAX_TILES, min_pf=20)
        with pytest.raises(ValueError):                                # before index_begin
            ld.index_add(_tables(itb, [0]), [INDEX[0]])
        for bad in (0, 21, -1):
            with pytest.raises(ValueError):
                ld.index_begin(bad)
        assert ld.I == 0 and ld.d_index == 0
        ld.add_tables([INDEX[0], INDEX[1]], _tables(tb, [0, 1]))
        ld.index_begin(8)                                              # after the first add
        with pytest.raises(ValueError):                                # twice
            ld.index_begin(8)
        with pytest.raises(ValueError):
            sc._ck(sc._lib.wd_lane_index_begin(ld._h, 8, ctypes.c_void_p(ld.d_index), ld.index_bytes))
        ld.index_add(_tables(itb, [2, 0]), [INDEX[2], INDEX[0]])
        for bad in ([INDEX[0]], [INDEX[1], INDEX[2]], [INDEX[3], INDEX[3]], [INDEX[3], MAX_TILES], [-1, INDEX[3]]):
            with pytest.raises(ValueError) as e:                       # repeated, repeated in the call, out of range
                ld.index_add(_tables(itb, [3, 4][:len(bad)]), bad)
            assert str(e.value).startswith(_lib.strerror(_lib.ERR_ARG))
        with pytest.raises(ValueError):                                # the interleaved layout
            ld.index_add(_tables(itb, [3]), [INDEX[3]], well_stride=4)
        assert sc.get_option("well_stride") == 1
        il = TileBatch(sc, 1, 8, N, interleave=4)
        with pytest.raises(ValueError):
            ld.index_add(il, [INDEX[3]])
        with pytest.raises(ValueError):                                # a batch of another shape (checked in Python)
            ld.index_add(tb, [INDEX[s] for s in ALL])
        host = np.zeros(N, dtype=np.uint8)                             # planes in host memory
        table = (ctypes.c_void_p * 8)(*[host.ctypes.data] * 8)
        with pytest.raises(ValueError) as e:
            ld.index_add((table, None), [INDEX[3]])
        assert "device memory" in str(e.value)
        with pytest.raises(ValueError):                                # a null plane
            ld.index_add(((ctypes.c_void_p * 8)(), None), [INDEX[3]])
        with pytest.raises(ValueError) as e:                           # before any finish of the lane
            ld.index_finish(20)
        assert "after a successful finish" in str(e.value)
        # the tile sets differ: index planes of 5 tiles against 4 added tiles, then the other way round
        ld.index_add(_tables(itb, [1, 3, 4]), [INDEX[1], INDEX[3], INDEX[4]])
        ld.add_tables([INDEX[2], INDEX[3]], _tables(tb, [2, 3]))
        assert (ld.finish(labels=True)[1][INDEX[4]] == 0).all()
        with pytest.raises(ValueError) as e:
            ld.index_finish(20)
        assert "tile index %d got index planes but was never added" % INDEX[4] in str(e.value)
        with pytest.raises(ValueError):                                # index_add after a finish
            ld.index_add(_tables(itb, [4]), [2])
        ld.restart()                                                   # the same workspaces, another lane
        ld.add_tables([INDEX[s] for s in ALL], _tables(tb, ALL))
        ld.index_add(_tables(itb, [0, 1, 2, 3]), [INDEX[s] for s in (0, 1, 2, 3)])
        ld.finish()
        with pytest.raises(ValueError) as e:
            ld.index_finish(20)
        assert "tile index %d was added without index planes" % INDEX[4] in str(e.value)
        with pytest.raises(ValueError):                                # begin after a finish
            sc._ck(sc._lib.wd_lane_index_begin(ld._h, 8, ctypes.c_void_p(ld.d_index), ld.index_bytes))
        # none of the refused calls changed anything: fed in full, the lane gives the right answer
        ld.restart()
        ld.add_tables([INDEX[s] for s in (0, 1)], _tables(tb, [0, 1]))
        ld.index_add(_tables(itb, [2, 0]), [INDEX[2], INDEX[0]])
        with pytest.raises(ValueError):
            ld.index_add(_tables(itb, [0, 3]), [INDEX[0], INDEX[3]])
        ld.index_add(_tables(itb, [1, 3, 4]), [INDEX[1], INDEX[3], INDEX[4]])
        ld.add_tables([INDEX[s] for s in (4, 2, 3)], _tables(tb, [4, 2, 3]))
        assert (ld.finish()[0] == eq_lane).all()
        row = np.zeros(5, dtype=np.int64)
        count = ctypes.c_int64()
        for args in ((None, p(row), None, None, ctypes.byref(count)), (p(row), None, None, None, ctypes.byref(count)),
                     (p(row), p(row), None, None, None)):
            assert sc._lib.wd_lane_index_finish(ld._h, 20, 0, *args) == _lib.ERR_ARG
        assert sc._lib.wd_lane_index_finish(ld._h, 20, -1, p(row), p(row), None, None, ctypes.byref(count)) == _lib.ERR_ARG
        assert sc._lib.wd_lane_index_finish(ld._h, 20, 5, p(row), p(row), None, None, ctypes.byref(count)) == _lib.ERR_ARG
        _same(ld.index_finish(20, 64), want)
        # a workspace too small, or in host memory
        ld2 = LaneDups(sc, N, MAX_TILES, L)
        try:
            assert sc.lane_index_workspace_bytes(N, MAX_TILES, 8) == ld.index_bytes
            rc = sc._lib.wd_lane_index_begin(ld2._h, 8, ctypes.c_void_p(ld.d_index), ld.index_bytes - 256)
            assert rc == _lib.ERR_ARG
            buf = np.zeros(ld.index_bytes, dtype=np.uint8)
            assert sc._lib.wd_lane_index_begin(ld2._h, 8, p(buf), ld.index_bytes) == _lib.ERR_ARG
            assert sc._lib.wd_lane_index_begin(ld2._h, 8, None, ld.index_bytes) == _lib.ERR_ARG
        finally:
            ld2.close()
    finally:
        ld.close()
        ld.close()                                                     # (a second close is a no-op)
        if il is not None:
            il.free()
        tb.free()
        itb.free()


def test_lane_index_full_hiseq4000_tiles(sc):
    """Three tiles of 4 309 253 wells, 50 scanned cycles and 8 index cycles, all from the device generator; the third
    has the first's scanned planes but for one plane whose upper half comes from the second (test_gpu_lanedups), and
    its own index planes: millions of classes across tiles, nearly all of them mixed."""
    n, LL, I = workload.HISEQ4000_ROWS * workload.HISEQ4000_COLS, 50, 8
    assert n == 4309253
    spec = synth.SynthSpec(seed=6, n_clusters=n, row=workload.HISEQ4000_COLS, plant_per_64k=1311, nocall_per_64k=328)
    where = [(1, 1101), (1, 1102), (1, 1103)]
    tb, itb = TileBatch(sc, 3, LL, n), TileBatch(sc, 3, I, n)
    tb.fill_synthetic(spec, where, list(range(LL)))
    itb.fill_synthetic(spec, where, list(range(100, 100 + I)))
    try:
        for c in range(LL):
            plane = tb.download_plane(0, c)
            if c == 17:
                plane[n // 2:] = tb.download_plane(1, c)[n // 2:]
            sc.h2d(tb.plane_ptr(2, c), plane)
        tiles = [(s, p, tb.download_filter(s)) for s, p in enumerate(_planes(tb))]
        eq_lane, _, labels = lane_dups(tiles, n, 3)
        del tiles
        itiles = [(s, p) for s, p in enumerate(_planes(itb))]
        want = lane_index(itiles, labels, n, 3, 130)
        check_index_identities(want, eq_lane)
        assert want[0][0] > 65536 and want[0][1] > 5000 and want[0][3] > 1_000_000 and want[1][0] > 100_000
        ld = LaneDups(sc, n, 3, LL)
        try:
            ld.index_begin(I)
            ld.add_tables([0, 1], _tables(tb, [0, 1]))
            ld.index_add(itb, [0, 1, 2])
            ld.add_tables([2], _tables(tb, [2]))
            assert (ld.finish()[0] == eq_lane).all()
            _same(ld.index_finish(130, 200000), want)
        finally:
            ld.close()
    finally:
        tb.free()
        itb.free()


# ---- the CLI ------------------------------------------------------------------------------------
def _main(argv):
    out = io.StringIO()
    with redirect_stdout(out):
        assert cwd.main(argv) == 0
    return out.getvalue()


def test_cli_lane_index_block_and_tsv(tmp_path):
    """2 lanes x 4 tiles, 30 scanned cycles and 8 + 4 index cycles behind them whose files the test overwrites with
    planted libraries; in each lane tile 1103's scanned cycles are copies of tile 1101's.  The block is the same for
    --tile-batch 1, 2 and the default, equals the reference, and is all the flag adds to the output."""
    rows, cols, levels, cycles = 36, 70, 3, 30
    n = rows * cols
    x, y = synth.honeycomb_pixels(rows, cols)
    spec = synth.SynthSpec(seed=35, n_clusters=n, row=cols, plant_per_64k=8000, nocall_per_64k=500, plant_far=True)
    run_dir = str(tmp_path / "run")
    names = ["1101", "1102", "1103", "1104"]
    index_cycles = list(range(40, 48)) + list(range(50, 54))
    synth.write_run_dir(spec, run_dir, [1, 2], names, list(range(cycles)) + index_cycles, slocs=synth.slocs_bytes(x, y))
    rng = np.random.default_rng(3)
    lib = rng.integers(1, 256, (6, len(index_cycles))).astype(np.uint8)
    planted = {}
    for lane in (1, 2):
        ldir = os.path.join(run_dir, "Data", "Intensities", "BaseCalls", "L%03d" % lane)
        for c in range(cycles):                                        # 1103's reads are 1101's (its filter is its own)
            cdir = os.path.join(ldir, "C%d.1" % (c + 1))
            with open(os.path.join(cdir, "s_%d_1101.bcl.gz" % lane), "rb") as src, \
                    open(os.path.join(cdir, "s_%d_1103.bcl.gz" % lane), "wb") as dst:
                dst.write(src.read())
        for t in names:
            idx = lib[rng.choice(6, n, p=[0.4, 0.3, 0.15, 0.1, 0.04, 0.01])]
            err, col = rng.random(n) < 0.03, rng.integers(0, idx.shape[1], n)
            idx[err, col[err]] = ((idx[err, col[err]] + 1) & 3) | 4
            planted[(lane, t)] = idx
            for j, cyc in enumerate(index_cycles):
                with gzip.open(os.path.join(ldir, "C%d.1" % (cyc + 1), "s_%d_%s.bcl.gz" % (lane, t)), "wb", compresslevel=1) as fh:
                    fh.write(synth.bcl_file_bytes(np.ascontiguousarray(idx[:, j])))
    argv = ["-s", "hiseq_x", "-r", run_dir, "-t", ",".join(names), "-i", "1,2", "-l", str(levels),
            "--cycles", "0-%d" % cycles, "-q", "--all-wells", "-S"]
    flag = ["--lane-dups-index", "40-48,50-54", "--lane-dups-index-min-share", "0.01"]
    for k in (0, 1):
        blocks, want_tsv = {}, []
        for lane in (1, 2):
            src = lambda t: int(t if t != "1103" else "1101")
            tiles = [(i, [synth.plane_bytes(spec, lane, src(t), c) for c in range(cycles)], synth.filter_bytes(spec, lane, int(t)))
                     for i, t in enumerate(names)]
            itiles = [(i, [np.ascontiguousarray(planted[(lane, t)][:, j]) for j in range(12)]) for i, t in enumerate(names)]
            eq_lane, _, eq_labels = lane_dups(tiles, n, 4)
            lane_row, labels = eq_lane, eq_labels
            if k:
                lane_row, _, labels = lane_near_dups(tiles, n, 4, k)
            pf = int(lane_row[0])
            min_pf, cap = math.ceil(0.01 * pf), 101
            assert cwd.index_listing(0.01, pf) == (min_pf, cap)
            got = lane_index(itiles, labels, n, 4, min_pf)
            check_index_identities(got, lane_row)
            counts = report.LaneIndexCounts.from_rows(*got, [8, 4], pf, lane_row[1])
            # five libraries over the share, the sixth and the reads with an error in Other; 1101's twins on 1103 fall
            # into another library more often than not
            assert counts.listed == 5 and counts.other[0] > 100 and counts.mixed_classes > 1000 and counts.within_libraries > 300
            text = io.StringIO()
            report.write_lane_index_dups(str(lane), counts, hamming=k, out=text)
            blocks[lane] = text.getvalue()
            keys = index_keys(itiles, n, 4)[0]
            m = cwd.lane_cluster_members(eq_labels, labels) if k else cwd.lane_members(eq_labels)
            cols_ = [v.tolist() for v in m]
            for r in zip(*cols_):
                read = report.index_bases(keys[r[0] * n + r[1]], [8, 4])
                want_tsv.append("\t".join([str(lane), names[r[0]], str(r[1]), names[r[2]], str(r[3])] +
                                          ([names[r[4]], str(r[5])] if k else []) + [read]))
        base = ["--lane-dups"] + (["--lane-dups-hamming", str(k)] if k else [])
        plain = _main(argv + base)
        tsv = str(tmp_path / "lane.tsv")
        runs = [_main(argv + base + flag + ["--tile-batch", "1"]),
                _main(argv + base + flag + ["--tile-batch", "2", "--lane-dups-out", tsv]),
                _main(argv + base + flag)]
        assert runs[0] == runs[1] == runs[2]
        b1, b2 = blocks[1], blocks[2]
        assert runs[0].count(b1) == 1 and runs[0].endswith(b2)
        assert runs[0].replace(b1, "", 1)[:-len(b2)] == plain          # minus the new blocks: the output without the flag
        assert runs[0].index("LaneDupsSummary: 1") < runs[0].index(b1) < runs[0].index("LaneDupsSummary: 2")
        lines = open(tsv).read().splitlines()
        assert lines[0].split("\t")[-1] == "index" and len(lines[0].split("\t")) == (8 if k else 6)
        assert lines[1:] == want_tsv and len(want_tsv) > 2000
        assert ("LaneIndexDups: 2\tHamming: 1\tIndex: " if k else "LaneIndexDups: 2\tIndex: ") in b2
        assert "+" in b2.splitlines()[1].split("\t")[2 if k else 1] and "LaneIndexDupsSummary: 2" in b2
