"""Which libraries a lane's duplicate copies join on the GPU (LaneDups.hops, include/welldup_lanehops.h) against the
host reference of tests/lanehops_ref.py - the lane row, the tile rows and every cell of the matrix equal, nothing
approximate - and against the header's identities: however the tiles and their index planes are fed, on the classes and
on the clusters, for every index length, split and E, across runs and tiles, with one cell and with a million."""
import ctypes
import gzip
import io
import math
import os
import re
from contextlib import redirect_stdout

import numpy as np
import pytest

from lanedups_ref import lane_dups
from lanehops_ref import LANE_COLS, TILE_COLS, check_hop_identities, lane_hops
from laneindex_ref import index_keys, key_of, lane_index
from lanemismatch_ref import lane_mismatches
from lanenear_ref import lane_near_dups
from tiledups_ref import INVALID
from well_duplicates_amd import _lib
from well_duplicates_amd import count_well_duplicates as cwd
from well_duplicates_amd import report, synth
from well_duplicates_amd.scanner import LaneDups, Scanner, TileBatch

pytestmark = pytest.mark.gpu

ROWS, COLS, L = 44, 60, 30
N = ROWS * COLS
INDEX = [5, 0, 3, 6, 1]                                               # slot -> tile index in a lane of MAX_TILES
MAX_TILES = 7                                                         # (indices 2 and 4 are never added)
DEAD = 1                                                              # the slot of the tile without a PF well
ALL = [0, 1, 2, 3, 4]
WAYS = {                                                              # the index planes never in the order of the reads
    "one call each": [("add", ALL), ("index", [3, 0, 2, 4, 1])],
    "a tile per call": [("index", [s]) for s in (4, 2, 0, 1, 3)] + [("add", [s]) for s in ALL],
    "2 + 3": [("add", [0, 1]), ("index", [2, 3, 4]), ("add", [2, 3, 4]), ("index", [0, 1])],
    "descending indices": [("index", [4, 0]), ("add", [3]), ("add", [0]), ("index", [2]), ("add", [2]), ("add", [4]),
                           ("index", [3, 1]), ("add", [1])],
}

with open(os.path.join(_lib.CSRC, "lane_pass.inc")) as _fh:
    RUN = int(re.search(r"constexpr int kLaneRun = (\d+);", _fh.read()).group(1))         # wells a workgroup takes
with open(os.path.join(_lib.CSRC, "lane_hops.inc")) as _fh:
    SLOTS = int(re.search(r"constexpr int kLhSlots = (\d+);", _fh.read()).group(1))        # matrix cells it counts in LDS


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


def _tables(tb, slots):
    ptrs = tb.plane_ptrs()
    return Scanner._tables([ptrs[s] for s in slots], [tb.filter_ptr(s) for s in slots], tb.L)


def _host(reads, filts, idx, index):
    planes = lambda r: [np.ascontiguousarray(r[:, c]) for c in range(r.shape[1])]
    return ([(index[s], planes(r), f) for s, (r, f) in enumerate(zip(reads, filts))],
            [(index[s], planes(x)) for s, x in enumerate(idx)])


def _labels(tiles, n, max_tiles, k):
    """-> (the lane row and the tile rows of the labels a finish at Hamming distance k leaves, the labels)"""
    if k == 0:
        return lane_dups(tiles, n, max_tiles)
    lane, rows, labels = lane_near_dups(tiles, n, max_tiles, k)
    return np.concatenate([lane[:6], lane[7:]]), rows, labels


def _fed(sc, tb, itb, index, max_tiles, ops, hash_bits=0):
    ld = LaneDups(sc, tb.N, max_tiles, tb.L, hash_bits=hash_bits)
    try:
        ld.index_begin(itb.L)
        for what, slots in ops:
            if what == "add":
                ld.add_tables([index[s] for s in slots], _tables(tb, slots))
            else:
                ld.index_add(_tables(itb, slots), [index[s] for s in slots])
    except Exception:
        ld.close()
        raise
    return ld


def _finish(ld, k, hash_bits=0):
    """-> the lane row and tile rows of the labels the lane is left with"""
    if k == 0:
        got = ld.finish()
        return got[0], got[1]
    got = ld.finish(hamming=k, pair_budget=1 << 27 if hash_bits == 1 else 0)      # (two buckets hold every read)
    return np.concatenate([got[3][:6], got[3][7:]]), got[4]


def _same(got, want):
    for g, w, name in zip(got, want, ("lane row", "tile rows", "matrix")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and (g == w).all(), (name, g[g != w][:8], w[g != w][:8], np.argwhere(g != w)[:8])


def _flip(col):
    """another base at the same place, whatever stood there"""
    return ((col + 1) & 3) | 4


def _hop_lane(seed, n=N, cycles=L, I=16, split=8, n_tiles=5, libraries=12, dead=DEAD, near=False, copies=1.0):
    """A pooled lane: `libraries` distinct index reads of skewed shares, a few per cent of the wells with one index
    read error, some with an N.  Reads are copied within and across tiles; on top of a copy its index read is kept,
    gets one error, gets another library's first part, second part or both, or differs from its original's at one of
    the cycles where the parts and the key's words begin and end: 0, split - 1, split, I - 1, 9, 10.
    -> (reads, filters, index reads), per tile [n, cycles] / [n] / [n, I]."""
    rng = np.random.default_rng(seed)
    reads = [rng.integers(1, 256, (n, cycles)).astype(np.uint8) for _ in range(n_tiles)]
    lib = np.zeros((0, I), dtype=np.uint8)
    while lib.shape[0] < libraries:                                    # distinct as bases
        lib = np.concatenate([lib, rng.integers(0, 4, (libraries, I)).astype(np.uint8)])
        lib = lib[np.sort(np.unique(lib, axis=0, return_index=True)[1])][:libraries]
    lib = lib | 0x40
    share = 0.7 ** np.arange(min(libraries, 40))
    share = np.concatenate([share, np.full(libraries - share.size, share[-1])]) + 0.01
    idx = []
    for r in reads:
        r[rng.random(r.shape) < 0.004] = 0
        x = lib[rng.choice(libraries, n, p=share / share.sum())]
        x = (x & 3) | (rng.integers(1, 64, x.shape).astype(np.uint8) << 2)             # the same bases, other quality bits
        err, col = rng.random(n) < 0.02, rng.integers(0, I, n)
        x[err, col[err]] = _flip(x[err, col[err]])
        x[rng.random(x.shape) < 0.002] = 0
        idx.append(x)
    edges = sorted({c for c in (0, split - 1, split, I - 1, 9, 10) if 0 <= c < I})
    plan = ((0, 0, 200, 0), (2, 2, 150, 1), (0, 2, 300, 2), (2, 3, 200, 3), (0, 4, 150, 4), (3, 4, 100, 5), (3, 3, 80, 2),
            (0, 3, 60, 5), (4, 0, 120, 1), (2, 0, 100, 0))
    for src, dst, count, kind in plan:
        src, dst, count = src % n_tiles, dst % n_tiles, int(count * copies)
        a, b = rng.choice(n, count, replace=False), rng.choice(n, count, replace=False)
        reads[dst][b] = reads[src][a]                                  # (chains: a copy of a copy)
        x = idx[src][a].copy()
        other = lib[rng.integers(0, libraries, count)]
        if kind == 1:
            col = rng.integers(0, I, count)
            x[np.arange(count), col] = _flip(x[np.arange(count), col])
        elif kind == 2:
            x[:, :split] = other[:, :split]
        elif kind == 3:
            x[:, split:] = other[:, split:]
        elif kind == 4:
            x = other.copy()
        elif kind == 5:
            col = np.array(edges)[rng.integers(0, len(edges), count)]
            x[np.arange(count), col] = _flip(x[np.arange(count), col])
        idx[dst][b] = x
    if near:
        for src, dst, count, d in ((0, 2, 200, 1), (2, 4, 150, 2), (3, 3, 100, 1), (4, 0, 100, 2)):
            src, dst = src % n_tiles, dst % n_tiles
            a, b = rng.choice(n, count, replace=False), rng.choice(n, count, replace=False)
            reads[dst][b] = reads[src][a]
            idx[dst][b] = idx[src][a]
            for _ in range(d):
                col = rng.integers(0, cycles, count)
                reads[dst][b, col] = (reads[dst][b, col] & 0xFC) | ((reads[dst][b, col] + 1) & 3) | 4
            swap = rng.random(count) < 0.3
            idx[dst][b[swap], :split] = lib[rng.integers(0, libraries, int(swap.sum()))][:, :split]
    filts = [(rng.random(n) < 0.9).astype(np.uint8) | (rng.integers(0, 2, n).astype(np.uint8) << 1) for _ in range(n_tiles)]
    if dead is not None:
        filts[dead][:] = 2                                             # (only bit 0 counts)
    return reads, filts, idx


def _listings(itiles, labels, n, max_tiles):
    """-> (every key a PF well carries, the three most frequent of them, none)"""
    keys = index_keys(itiles, n, max_tiles)[0][np.asarray(labels).reshape(-1) != INVALID]
    ukeys, count = np.unique(keys, return_counts=True)
    order = np.lexsort((ukeys, -count))
    return ukeys[order], ukeys[order][:3], ukeys[:0]


# ---- 1: feeding orders ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 2])
def test_lane_hops_match_reference_however_the_tiles_are_fed(sc, k):
    I, split, E = 16, 8, 1
    reads, filts, idx = _hop_lane(11 + k, near=k > 0)
    tiles, itiles = _host(reads, filts, idx, INDEX)
    lane_row, tile_rows, labels = _labels(tiles, N, MAX_TILES, k)
    every, top3, none = _listings(itiles, labels, N, MAX_TILES)
    assert 100 < every.size <= 1024
    wants = [lane_hops(itiles, labels, N, MAX_TILES, I, split, E, listed) for listed in (every, top3, none)]
    for want, all_listed in zip(wants, (True, False, False)):
        check_hop_identities(want, lane_row, tile_rows, I, split, E, all_listed=all_listed)
    lane = wants[0][0]
    # every state but the rare ones is there, copies across tiles and on one, into listed libraries and out of them
    assert lane[0] > 800 and lane[1] > 100 and lane[2] > 150 and lane[3] > 50 and (lane[4:] > 0).sum() >= 6
    assert np.count_nonzero(wants[0][2]) > 100 and wants[1][2][3].sum() > 0 and wants[1][2][:3, :3].sum() > 100
    tb, itb = _upload(sc, reads, filts), _upload(sc, idx)
    try:
        for bits in (0, 4, 1):
            for name, ops in WAYS.items():
                if bits and name not in ("one call each", "descending indices"):
                    continue
                ld = _fed(sc, tb, itb, INDEX, MAX_TILES, ops, hash_bits=bits)
                try:
                    rows = _finish(ld, k, bits)
                    assert (rows[0] == lane_row).all() and (rows[1] == tile_rows).all(), name
                    for listed, want in zip((every, top3, none), wants):
                        got = ld.hops(split, E, listed)
                        _same(got, want)
                        check_hop_identities(got, *rows, I, split, E, all_listed=listed is every)
                finally:
                    ld.close()
    finally:
        tb.free()
        itb.free()


# ---- 2: index lengths and splits --------------------------------------------------------------------
@pytest.mark.parametrize("I", [1, 8, 10, 11, 16, 20])
def test_index_lengths_and_splits(sc, I):
    n, cycles, index = 1001, 16, [2, 0, 1]
    splits = sorted({s for s in (1, I // 2, I) if 1 <= s <= I})
    tb = itb = ld = None
    try:
        for split in splits:
            reads, filts, idx = _hop_lane(200 + 20 * I + split, n=n, cycles=cycles, I=I, split=split, n_tiles=3,
                                          libraries=min(6, 4 ** I), dead=None, copies=0.5)
            tiles, itiles = _host(reads, filts, idx, index)
            lane_row, tile_rows, labels = _labels(tiles, n, 3, 0)
            every, top3, _ = _listings(itiles, labels, n, 3)
            tb, itb = _upload(sc, reads, filts), _upload(sc, idx)
            ld = _fed(sc, tb, itb, index, 3, [("index", [1]), ("add", [0, 1, 2]), ("index", [2, 0])])
            rows = _finish(ld, 0)
            seen = np.zeros(9, dtype=np.int64)
            for E in (0, 1, 3):
                for listed in (every[:1024], top3):
                    want = lane_hops(itiles, labels, n, 3, I, split, E, listed)
                    got = ld.hops(split, E, listed)
                    _same(got, want)
                    check_hop_identities(got, *rows, I, split, E, all_listed=listed is not top3 and every.size <= 1024)
                seen += want[0][4:]
                # the pairs planted at the edges of the parts, one cycle apart: Far at E = 0, Near at E >= 1
                assert want[0][0] > 250 and (I == 1 or want[0][4] > 50)
            assert seen[0] > 0 and (seen[[3, 6]] > 0).all() and (split == I or (seen[[1, 2]] > 0).all())
            ld.close()
            tb.free()
            itb.free()
            tb = itb = ld = None
    finally:
        for v in (ld, tb, itb):
            if v is not None:
                (v.close if isinstance(v, LaneDups) else v.free)()


# ---- 3: run and tile boundaries ---------------------------------------------------------------------
def _big_lane(seed, n_tiles, libraries, I, copies, index_random=True):
    """n_tiles tiles of RUN + 300 wells: random reads of 12 cycles; `copies` wells of the later tiles are copies of a
    well of the first, each with the index read of a library drawn anew."""
    rng = np.random.default_rng(seed)
    n = RUN + 300
    reads = [rng.integers(1, 256, (n, 12)).astype(np.uint8) for _ in range(n_tiles)]
    lib = np.zeros((0, I), dtype=np.uint8)
    while lib.shape[0] < libraries:
        lib = np.concatenate([lib, rng.integers(0, 4, (libraries, I)).astype(np.uint8)])
        lib = lib[np.sort(np.unique(lib, axis=0, return_index=True)[1])][:libraries]
    lib = lib | 0x80
    idx = [lib[rng.integers(0, libraries, n)] for _ in range(n_tiles)]
    for t in range(1, n_tiles):
        a, b = rng.choice(n, copies, replace=False), rng.choice(n, copies, replace=False)
        reads[t][b] = reads[0][a]
    filts = [(rng.random(n) < 0.95).astype(np.uint8) for _ in range(n_tiles)]
    return reads, filts, idx, lib


def test_pairs_that_cross_a_run_or_a_tile(sc):
    """2 tiles of a run and 300 wells.  A copy sits in the last, partial trip of the second run of the later tile,
    its root on the other tile, its first index read another library's."""
    I, split, E, index = 16, 8, 1, [2, 0]                              # slot 1 is tile index 0: the smaller ids, the roots
    reads, filts, idx, lib = _big_lane(31, 2, 12, I, 400)
    n = RUN + 300
    w_copy, w_root = n - 5, 7
    assert (w_copy - RUN) // 256 == 1 and (n - RUN) % 256 != 0         # the second trip of the second run, a partial one
    reads[0][w_copy] = reads[1][w_root]
    filts[0][w_copy] = filts[1][w_root] = 1
    idx[1][w_root] = lib[0]
    idx[0][w_copy] = np.concatenate([lib[1][:split], lib[0][split:]])
    tiles, itiles = _host(reads, filts, idx, index)
    lane_row, tile_rows, labels = _labels(tiles, n, 3, 0)
    assert labels[2][w_copy] == w_root                                 # (tile index 0 x n + 7)
    every, top3, none = _listings(itiles, labels, n, 3)
    bases = lambda x: "".join("ACGT"[v & 3] for v in x)
    listed = np.array([key_of(bases(lib[i])) for i in range(12)] + [key_of(bases(idx[0][w_copy]))], dtype=np.uint64)
    wants = [lane_hops(itiles, labels, n, 3, I, split, E, keys) for keys in (listed, none)]
    check_hop_identities(wants[0], lane_row, tile_rows, I, split, E, all_listed=True)
    # the planted pair alone has the combination: library 0's root, Far/Same
    assert wants[0][2][0][12] == 1 == wants[0][2][:, 12].sum() and wants[0][0][10] >= 1 and wants[0][1][2][0] > 300 and wants[0][1][2][1] < 20 and wants[0][1][0][0] > 0
    tb, itb = _upload(sc, reads, filts), _upload(sc, idx)
    ld = _fed(sc, tb, itb, index, 3, [("add", [0, 1]), ("index", [1, 0])])
    try:
        rows = _finish(ld, 0)
        for keys, want in zip((listed, none), wants):
            got = ld.hops(split, E, keys)
            _same(got, want)
            check_hop_identities(got, *rows, I, split, E, all_listed=keys is listed)
    finally:
        ld.close()
        tb.free()
        itb.free()


# ---- 4: one cell ------------------------------------------------------------------------------------
def test_a_lane_of_one_read_and_one_index_is_one_cell(sc):
    n, I = RUN + 300, 8
    rng = np.random.default_rng(4)
    reads = [np.tile(np.array([0x42 + (c % 4) for c in range(12)], dtype=np.uint8), (n, 1)) for _ in range(3)]
    idx = [np.tile(np.array([0x42 + 4 * (c % 3) for c in range(I)], dtype=np.uint8), (n, 1)) for _ in range(3)]
    filts = [(rng.random(n) < 0.9).astype(np.uint8) for _ in range(3)]
    total = int(sum(f.sum() for f in filts))
    first = int(np.flatnonzero(filts[0])[0])                           # the root of everything
    same_tile = int(filts[0].sum()) - 1
    tb, itb = _upload(sc, reads, filts), _upload(sc, idx)
    ld = _fed(sc, tb, itb, [0, 1, 2], 3, [("add", [0, 1, 2]), ("index", [0, 1, 2])])
    try:
        rows = _finish(ld, 0)
        assert rows[0][:4].tolist() == [total, 1, total, total - 1] and first < 64
        for split, E in ((8, 0), (4, 1)):
            lane, tile_rows, matrix = ld.hops(split, E, [key_of("G" * I)])
            assert lane.tolist() == [total - 1, same_tile, 0, 0, total - 1] + [0] * 8
            assert matrix.tolist() == [[total - 1, 0], [0, 0]]
            assert tile_rows[:, 0].tolist() == [int(filts[0].sum()) - 1, int(filts[1].sum()), int(filts[2].sum())]
            check_hop_identities((lane, tile_rows, matrix), *rows, I, split, E, all_listed=True, subset_of_scanned=True)
        lane, _, matrix = ld.hops(8, 1, [])
        assert matrix.tolist() == [[total - 1]] and lane[4] == total - 1
        lane, _, matrix = ld.hops(8, 1, [key_of("A" * I), key_of("C" * I)])
        assert matrix[2][2] == total - 1 == matrix.sum()
    finally:
        ld.close()
        tb.free()
        itb.free()


# ---- 5: many cells ----------------------------------------------------------------------------------
def test_more_cells_in_a_run_than_the_lds_table_holds(sc):
    """(a) 40 listed libraries, thousands of copies whose library is drawn anew: a run meets at least 600 of the 1600
    cells.  (b) 1100 libraries of which the 1024 largest are listed: a run meets more cells than the table has
    entries, the adds that find it full go to memory, and the rest of the groups is Other."""
    n, I = RUN + 300, 8
    for libraries, m, least in ((40, 40, 600), (1100, 1024, SLOTS + 1)):
        reads, filts, idx, lib = _big_lane(50 + libraries, 2, libraries, I, 4000)
        tiles, itiles = _host(reads, filts, idx, [0, 1])
        lane_row, tile_rows, labels = _labels(tiles, n, 2, 0)
        every, _, _ = _listings(itiles, labels, n, 2)
        assert every.size == libraries
        listed = every[:m]
        want = lane_hops(itiles, labels, n, 2, I, 4, 1, listed)
        check_hop_identities(want, lane_row, tile_rows, I, 4, 1, all_listed=m == libraries)
        # the cells one workgroup meets: the pairs of the first run of the second tile
        keys = index_keys(itiles, n, 2)[0]
        ids = n + np.flatnonzero((labels[1][:RUN] != INVALID) & (labels[1][:RUN] != n + np.arange(RUN)))
        rank = {int(key): i for i, key in enumerate(listed.tolist())}
        cells = {(rank.get(int(keys[labels[1][g - n]]), m), rank.get(int(keys[g]), m)) for g in ids.tolist()}
        assert len(cells) >= least and want[0][0] > 3000
        if m < libraries:
            assert want[2][m].sum() > 50 and want[2][:, m].sum() > 50 and want[2][m][m] > 0
        tb, itb = _upload(sc, reads, filts), _upload(sc, idx)
        ld = _fed(sc, tb, itb, [0, 1], 2, [("index", [1, 0]), ("add", [0, 1])])
        try:
            rows = _finish(ld, 0)
            got = ld.hops(4, 1, listed)
            _same(got, want)
            check_hop_identities(got, *rows, I, 4, 1, all_listed=m == libraries)
            _same(ld.hops(4, 1, listed[::-1]), (want[0], want[1], want[2][::-1, ::-1][np.r_[1:m + 1, 0]][:, np.r_[1:m + 1, 0]]))
        finally:
            ld.close()
            tb.free()
            itb.free()


# ---- 6: call discipline -----------------------------------------------------------------------------
def _raw(sc, ld, split, max_e, keys, scratch, scratch_bytes, missing=None, m=None):
    """wd_lane_hops itself -> (rc, lane row, tile rows, matrix); missing: the pointer passed as null (3: the keys)"""
    keys = np.ascontiguousarray(np.asarray(keys, dtype=np.uint64))
    m = keys.size if m is None else m
    out = [np.full(LANE_COLS, -1, dtype=np.int64), np.full((ld.max_tiles, TILE_COLS), -1, dtype=np.int64),
           np.full((max(0, min(m, 1024)) + 1,) * 2, -1, dtype=np.int64)]
    ptr = [None if i == missing else a.ctypes.data_as(ctypes.c_void_p) for i, a in enumerate(out)]
    kp = None if missing == 3 or keys.size == 0 else keys.ctypes.data_as(ctypes.c_void_p)
    rc = sc._lib.wd_lane_hops(ld._h, split, max_e, m, kp, ctypes.c_void_p(scratch), scratch_bytes, *ptr)
    return (rc,) + tuple(out)


def _untouched(res):
    return all((a == -1).all() for a in res[1:])


def test_call_discipline(sc):
    I, split, E, k = 8, 4, 1, 1
    reads, filts, idx = _hop_lane(77, I=I, split=split, near=True)
    tiles, itiles = _host(reads, filts, idx, INDEX)
    lane_row, tile_rows, labels = _labels(tiles, N, MAX_TILES, k)
    every, top3, none = _listings(itiles, labels, N, MAX_TILES)
    want = lane_hops(itiles, labels, N, MAX_TILES, I, split, E, top3)
    want_index = lane_index(itiles, labels, N, MAX_TILES, 5)
    want_mis = lane_mismatches(tiles, N, MAX_TILES, labels, k)
    need = sc.lane_hops_scratch_bytes(MAX_TILES, 3)
    d_scratch = sc.malloc(need)
    host = np.zeros(need, dtype=np.uint8)
    tb, itb = _upload(sc, reads, filts), _upload(sc, idx)
    ld = _fed(sc, tb, itb, INDEX, MAX_TILES, WAYS["2 + 3"])
    bare = LaneDups(sc, N, MAX_TILES, L)                               # a lane without an index part
    last_error = lambda: sc._lib.wd_last_error(sc._ctx).decode()
    try:
        res = _raw(sc, ld, split, E, top3, d_scratch, need)            # before any finish
        assert res[0] == _lib.ERR_ARG and _untouched(res) and "finish" in last_error()
        with pytest.raises(ValueError):
            ld.hops(split, E, top3)
        with pytest.raises(RuntimeError):                              # a near finish refused over budget is no finish
            ld.finish(hamming=k, pair_budget=3)
        res = _raw(sc, ld, split, E, top3, d_scratch, need)
        assert res[0] == _lib.ERR_ARG and _untouched(res)
        rows = _finish(ld, k)
        assert (rows[0] == lane_row).all()
        bare.add_tables([INDEX[s] for s in ALL], _tables(tb, ALL))
        bare.finish()
        res = _raw(sc, bare, split, E, top3, d_scratch, need)
        assert res[0] == _lib.ERR_ARG and _untouched(res) and "no index part" in last_error()
        dup = [int(top3[0]), int(top3[1]), int(top3[0])]
        bad = [(0, E, top3), (I + 1, E, top3), (-1, E, top3), (split, -1, top3), (split, 4, top3), (split, E, dup),
               (split, E, [int(top3[0]), 5]), (split, E, [int(top3[0]), 1 << (3 * I)]), (split, E, [1 << 30]),
               (split, E, [1 << 63])]
        for s, e, keys in bad:
            res = _raw(sc, ld, s, e, keys, d_scratch, need)
            assert res[0] == _lib.ERR_ARG and _untouched(res), (s, e, keys)
            with pytest.raises(ValueError):
                ld.hops(s, e, keys)
        assert _raw(sc, ld, split, E, dup, d_scratch, need)[0] == _lib.ERR_ARG and "0x%016x is given twice" % dup[0] in last_error()
        assert _raw(sc, ld, split, E, [5], d_scratch, need)[0] == _lib.ERR_ARG and "0x%016x is no index read" % 5 in last_error()
        for m in (-1, 1025):                                           # M out of range, whatever the scratch
            res = _raw(sc, ld, split, E, top3, d_scratch, need, m=m)
            assert res[0] == _lib.ERR_ARG and _untouched(res)
        with pytest.raises(ValueError):
            ld.hops(split, E, np.arange(1025, dtype=np.uint64))
        for missing in range(4):
            res = _raw(sc, ld, split, E, top3, d_scratch, need, missing=missing)
            assert res[0] == _lib.ERR_ARG and _untouched(res), missing
        for scratch, nbytes in ((0, need), (d_scratch, need - 256), (d_scratch, 0), (host.ctypes.data, need)):
            res = _raw(sc, ld, split, E, top3, scratch, nbytes)
            assert res[0] == _lib.ERR_ARG and _untouched(res), (scratch, nbytes)
        assert _raw(sc, ld, split, E, every[:200], d_scratch, need)[0] == _lib.ERR_ARG      # the scratch of three keys
        first = _raw(sc, ld, split, E, top3, d_scratch, need)          # the caller's scratch, dirty from nothing
        assert first[0] == _lib.OK
        _same(first[1:], want)
        _same(ld.hops(split, E, top3), want)                           # twice the same, before the index finish
        got_index = ld.index_finish(5)
        got_mis = ld.mismatches(k)
        _same(ld.hops(split, E, top3), want)                           # and after it
        _same(_raw(sc, ld, split, E, top3, d_scratch, need)[1:], want)
        for g, w in zip(ld.index_finish(5), got_index):                # which found its tables as it left them
            assert (g == w).all()
        for g, w in zip(got_index, want_index):
            assert g.shape == w.shape and (g == w).all()
        for g, w in zip(ld.mismatches(k), got_mis):
            assert (g == w).all()
        for g, w in zip(got_mis, want_mis):
            assert (g == w).all()
        # the same lane again without a call of hops: the other passes give what they gave with one in between
        ld.restart()
        for what, slots in WAYS["one call each"]:
            if what == "add":
                ld.add_tables([INDEX[s] for s in slots], _tables(tb, slots))
            else:
                ld.index_add(_tables(itb, slots), [INDEX[s] for s in slots])
        _finish(ld, k)
        for g, w in zip(ld.mismatches(k), got_mis):
            assert (g == w).all()
        for g, w in zip(ld.index_finish(5), got_index):
            assert (g == w).all()
        # the tile sets differ: index_finish's message
        ld.restart()
        ld.add_tables([INDEX[s] for s in ALL], _tables(tb, ALL))
        ld.index_add(_tables(itb, [0, 1, 2, 3]), [INDEX[s] for s in (0, 1, 2, 3)])
        ld.finish()
        res = _raw(sc, ld, split, E, top3, d_scratch, need)
        assert res[0] == _lib.ERR_ARG and _untouched(res)
        assert "tile index %d was added without index planes" % INDEX[4] in last_error()
        ld.close()
        with pytest.raises(ValueError):
            ld.hops(split, E, top3)
    finally:
        ld.close()
        bare.close()
        tb.free()
        itb.free()
        sc.free(d_scratch)


# ---- 7: the CLI -------------------------------------------------------------------------------------
def _main(argv):
    out = io.StringIO()
    with redirect_stdout(out):
        assert cwd.main(argv) == 0
    return out.getvalue()


def test_cli_lane_hops_block_and_tsv(tmp_path):
    """The run directory of test_gpu_laneindex.py's CLI test: 2 lanes x 4 tiles, 30 scanned cycles and 8 + 4 index cycles
    whose files the test overwrites with planted libraries; in each lane tile 1103's scanned cycles are copies of tile
    1101's, its libraries its own.  The new block closes each lane's output, equals write_lane_hops of the reference
    on index_finish's listing, is the same for --tile-batch 1 and the default, and is all the flag adds."""
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
            "--cycles", "0-%d" % cycles, "-q", "--all-wells", "--lane-dups", "--lane-dups-index-min-share", "0.01"]
    two, one = ["--lane-dups-index", "40-48,50-54"], ["--lane-dups-index", "40-48"]
    tsv = str(tmp_path / "hops.tsv")
    # (Hamming K, -S, the index ranges, E, the pairs listed)
    for k, summary, ranges, lengths, E, n_pairs in ((0, False, two, [8, 4], 1, 10), (1, True, two, [8, 4], 0, 3),
                                                    (0, True, one, [8], 1, 10)):
        I = sum(lengths)
        blocks, want_tsv = {}, ["lane\tindex_a\tindex_b\tpairs"]
        for lane in (1, 2):
            src = lambda t: int(t if t != "1103" else "1101")
            tiles = [(i, [synth.plane_bytes(spec, lane, src(t), c) for c in range(cycles)], synth.filter_bytes(spec, lane, int(t)))
                     for i, t in enumerate(names)]
            itiles = [(i, [np.ascontiguousarray(planted[(lane, t)][:, j]) for j in range(I)]) for i, t in enumerate(names)]
            lane_row, tile_rows, labels = _labels(tiles, n, 4, k)
            pf = int(lane_row[0])
            listing = lane_index(itiles, labels, n, 4, math.ceil(0.01 * pf))
            keys, pfs = listing[3], listing[2][:, 0].tolist()
            got = lane_hops(itiles, labels, n, 4, I, lengths[0], E, keys)
            check_hop_identities(got, lane_row, tile_rows, I, lengths[0], E)
            counts = report.LaneHopCounts.from_rows(*got, keys, pfs + [pf - sum(pfs)], lengths, names, E, k, n_pairs)
            # 1101's twins on 1103 fall into another library more often than not
            assert len(keys) >= 5 and counts.pairs > 1500 and counts.hop1 + counts.hop2 > 1000 and counts.into_listed() > 1000
            text = io.StringIO()
            report.write_lane_hops(str(lane), counts, verbose=not summary, out=text)
            blocks[lane] = text.getvalue()
            text = io.StringIO()
            report.write_lane_hops_tsv(str(lane), counts, text, header=False)
            want_tsv += text.getvalue().splitlines()
        base = argv + ranges + (["-S"] if summary else []) + (["--lane-dups-hamming", str(k)] if k else [])
        flag = ["--lane-dups-hops"] + ([str(n_pairs)] if n_pairs != 10 else []) + \
            (["--lane-dups-hops-mismatches", str(E)] if E != 1 else [])
        plain = _main(base)
        runs = [_main(base + flag + ["--tile-batch", "1"]), _main(base + flag + ["--lane-dups-hops-out", tsv])]
        assert runs[0] == runs[1]
        b1, b2 = blocks[1], blocks[2]
        assert runs[0].count(b1) == 1 and runs[0].endswith(b2)
        assert runs[0].replace(b1, "", 1)[:-len(b2)] == plain          # minus the new blocks: the output without the flag
        assert runs[0].index("LaneIndexDupsSummary: 1") < runs[0].index(b1) < runs[0].index("LaneDupsSummary: 2")
        assert open(tsv).read().splitlines() == want_tsv and len(want_tsv) > 20
        assert b2.count("LaneHops: 2\t") == (9 if len(lengths) == 2 else 3) and b2.count("LaneHopPair: 2\t") == n_pairs
        assert ("LaneHops: 2\tHamming: 1\tIndex1: " in b2) == bool(k) and ("LaneHopsTile: 2\t" in b2) == (not summary)
