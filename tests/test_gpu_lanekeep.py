"""The best well of each of a lane's families on the GPU (LaneDups.keep, include/welldup_lanekeep.h) against the host
reference of tests/lanekeep_ref.py on the labels of tests/lanenear_ref.py / lanedups_ref.py - lane row, tile rows and
every mask byte equal, nothing approximate - however the tiles are fed and whatever hash_bits, and against the
identities the header states: QHist of LaneDups.qualities on the same accumulator among them, and the lane rebuilt
from the masks, which has no redundant well left.

Figures of this file's shapes on the reference (so that a change of the inputs that empties a test shows): the fed
lane has more than 350 families at every K, more than 100 of them moved at min_q 15."""
import ctypes
import io
import os
import re
import shutil
from contextlib import redirect_stdout

import numpy as np
import pytest

from lanedups_ref import lane_dups
from lanekeep_ref import LANE_COLS, TILE_COLS, check_keep_identities, lane_keep, quality_weight, scores_of
from lanenear_ref import lane_near_dups
from well_duplicates_amd import _lib
from well_duplicates_amd import count_well_duplicates as cwd
from well_duplicates_amd import bcl, report, synth
from well_duplicates_amd.scanner import LaneDups, Scanner, TileBatch

pytestmark = pytest.mark.gpu

N = 44 * 60
INDEX = [3, 0, 5, 1]                                                  # slot -> tile index in a lane of MAX_TILES
MAX_TILES = 6                                                         # (indices 2 and 4 are never added)
WAYS = {"one call": [[0, 1, 2, 3]], "a tile per call": [[0], [1], [2], [3]], "1 + 3": [[0], [1, 2, 3]],
        "descending indices": [[2], [0], [3], [1]]}
QUAL_WAYS = {"one call": "1 + 3", "a tile per call": "one call", "1 + 3": "descending indices",
             "descending indices": "a tile per call"}                 # the qualities come batched otherwise than the reads
EDGES = [0, 2, 8, 14, 20, 26, 32, 38]
INVALID = 0xFFFFFFFF

with open(os.path.join(_lib.CSRC, "lane_pass.inc")) as _fh:
    RUN = int(re.search(r"constexpr int kLaneRun = (\d+);", _fh.read()).group(1))         # wells a workgroup takes


@pytest.fixture(scope="module")
def sc():
    s = Scanner(0)
    yield s
    s.close()


def _upload(sc, reads, filts):
    """reads: per tile uint8 [n, L] (well, cycle); -> a resident TileBatch"""
    n, cycles = reads[0].shape
    tb = TileBatch(sc, len(reads), cycles, n)
    for i, (r, f) in enumerate(zip(reads, filts)):
        tb.upload_tile(i, [np.ascontiguousarray(r[:, c]) for c in range(cycles)], f)
    return tb


def _host_tiles(reads, filts, index):
    return [(index[s], [np.ascontiguousarray(r[:, c]) for c in range(r.shape[1])], f)
            for s, (r, f) in enumerate(zip(reads, filts))]


def _tables(tb, slots):
    ptrs = tb.plane_ptrs()
    return Scanner._tables([ptrs[s] for s in slots], [tb.filter_ptr(s) for s in slots], tb.L)


def _lane(sc, tb, index, max_tiles, calls, edges, qual_calls=None, hash_bits=0, qual_first=False):
    """an accumulator with a quality part, the reads fed by `calls` and the qualities by `qual_calls`"""
    ld = LaneDups(sc, tb.N, max_tiles, tb.L, hash_bits=hash_bits)
    try:
        ld.qual_begin(edges)
        feeds = [(ld.qual_add, qual_calls if qual_calls is not None else calls),
                 (lambda tables, idx: ld.add_tables(idx, tables), calls)]
        for feed, batches in feeds if qual_first else feeds[::-1]:
            for slots in batches:
                feed(_tables(tb, slots), [index[s] for s in slots])
    except Exception:
        ld.close()
        raise
    return ld


def _finish(ld, k, hash_bits=0):
    """-> the lane row and the tile rows of the labels the lane is left with"""
    if k == 0:
        return ld.finish()[:2]
    got = ld.finish(hamming=k, pair_budget=1 << 27 if hash_bits in (1, 2) else 0)      # (a few buckets hold every read)
    return got[3], got[4]


def _same(got, want, what=""):
    """(lane row, tile rows, masks) of LaneDups.keep against the reference's first three"""
    for g, w, name in zip(got[:2], want[:2], ("lane row", "tile rows")):
        assert g.shape == w.shape and (g == w).all(), (what, name, g[g != w], w[g != w], np.argwhere(g != w)[:8])
    if len(got) > 2:
        assert sorted(got[2]) == sorted(want[2]), what
        for t in want[2]:
            assert got[2][t].dtype == np.uint8 and (got[2][t] == want[2][t]).all(), (what, t, np.flatnonzero(got[2][t] != want[2][t])[:8])


def _other_base(b):
    """the byte with another base and the same quality, never 0 (a no-call becomes a base of quality 0)"""
    b = int(b)
    return (b & 0xFC) | ((b + 1) & 3) if b & 0xFC else 1 + (b & 3) % 3


def _requalify(read, fresh):
    """the read with the quality bits of `fresh`; a no-call stays one, and no base becomes a no-call"""
    new = (read & 3) | (fresh & 0xFC)
    return np.where(read == 0, 0, np.where(new == 0, read, new)).astype(np.uint8)


def _plant(reads, rng, src_tile, dst_tile, count, mismatches):
    """copies of `count` reads of src_tile on dst_tile, copy i with 1 + i % mismatches cycles changed (0: none), each
    called with qualities of its own, 0..63 (a no-call stays one), as test_gpu_lanequality._plant does"""
    n, cycles = reads[0].shape
    a, b = rng.choice(n, count, replace=False), rng.choice(n, count, replace=False)
    reads[dst_tile][b] = _requalify(reads[src_tile][a], rng.integers(0, 64, (count, cycles)).astype(np.uint8) << 2)
    for i, w in enumerate(b.tolist()):
        if mismatches:
            for c in rng.choice(cycles, min(cycles, 1 + i % mismatches), replace=False).tolist():
                reads[dst_tile][w, c] = _other_base(reads[dst_tile][w, c])


def _random_tiles(rng, tiles, n, cycles, pf=0.93):
    reads = [rng.integers(1, 256, (n, cycles)).astype(np.uint8) for _ in range(tiles)]
    for r in reads:
        r[rng.random(r.shape) < 0.005] = 0                            # no-calls
    return reads, [(rng.random(n) < pf).astype(np.uint8) for _ in range(tiles)]


def _fed_lane(k, cycles):
    """Four tiles of 2640 wells, random reads with every quality 0..63 and no-calls; near copies at 1 .. k + 1 mismatches
    planted within tiles and across tiles (chains: a copy of a copy) and equal reads across tiles, every copy with
    qualities of its own."""
    rng = np.random.default_rng(29 + k)
    reads, filts = _random_tiles(rng, 4, N, cycles)
    for src, dst, count in ((0, 2, 300), (2, 3, 200), (0, 1, 150), (3, 1, 100), (0, 0, 120), (3, 3, 120)):
        _plant(reads, rng, src, dst, count, k + 1)
    for src, dst, count in ((2, 1, 150), (1, 3, 150), (0, 3, 100), (1, 1, 80)):      # and equal reads, chains among them
        _plant(reads, rng, src, dst, count, 0)
    return reads, filts


def _labels(tiles, n, max_tiles, k):
    """-> (finish lane row, finish tile rows, labels) of the reference at K = k"""
    return lane_dups(tiles, n, max_tiles) if k == 0 else lane_near_dups(tiles, n, max_tiles, k)


# ---- 1: rows and masks against the reference, however the lane is fed ------------------------------
@pytest.mark.parametrize("cycles", [37, 83])         # a partial last word in 16-byte pieces; nine words
@pytest.mark.parametrize("k", [0, 1, 2])
def test_keep_matches_reference_however_the_tiles_are_fed(sc, k, cycles):
    reads, filts = _fed_lane(k, cycles)
    tiles = _host_tiles(reads, filts, INDEX)
    fin_lane, fin_tiles, labels = _labels(tiles, N, MAX_TILES, k)
    min_qs = (15, 0, 63)                                               # 63: above every edge, identity 6
    want = {q: lane_keep(tiles, N, MAX_TILES, labels, EDGES, q) for q in min_qs}
    # the ground is covered: hundreds of families, many of them moved, kept copies on every tile, every gain bin below
    # 500 among them; nothing moves when nothing weighs
    lane = want[15][0]
    print("families %d moved %d gains %s" % (lane[6], lane[7], lane[9:].tolist()))
    assert lane[6] > 350 and lane[7] > 100 and (want[15][1][INDEX, 3] > 0).all() and (lane[10:16] > 0).all()
    assert want[63][0][7] == 0 and want[0][0][4] > lane[4] > 0
    for q in min_qs:
        check_keep_identities(want[q][0], want[q][1], EDGES, q, fin_lane, fin_tiles, sum_singles=want[q][3],
                              masks=want[q][2], labels=labels)
    tb = _upload(sc, reads, filts)
    try:
        for bits in (0, 2):
            for way, calls in WAYS.items():
                ld = _lane(sc, tb, INDEX, MAX_TILES, calls, EDGES, qual_calls=WAYS[QUAL_WAYS[way]], hash_bits=bits,
                           qual_first=way in ("1 + 3", "one call"))
                try:
                    got_lane, got_tiles = _finish(ld, k, bits)
                    qhist = ld.qualities(0)[2]
                    for q in min_qs:
                        got = ld.keep(q, masks=True)
                        _same(got, want[q], (bits, way, q))
                        check_keep_identities(got[0], got[1], EDGES, q, got_lane, got_tiles, qhist=qhist,      # identity 4
                                              sum_singles=want[q][3], masks=got[2], labels=labels)
                        assert (got[1][[2, 4]] == 0).all()             # a tile index never added
                    _same(ld.keep(15), want[15])                       # without masks: the rows alone
                finally:
                    ld.close()
    finally:
        tb.free()


# ---- 2: the lane rebuilt from the masks (identity 8) -----------------------------------------------
@pytest.mark.parametrize("k", [0, 1])
def test_the_lane_rebuilt_from_the_masks_has_no_redundant_well(sc, k):
    reads, filts = _fed_lane(k, 37)
    tb = _upload(sc, reads, filts)
    ld = _lane(sc, tb, INDEX, MAX_TILES, WAYS["one call"], EDGES)
    try:
        before = _finish(ld, k)[0]
        lane, trow, masks = ld.keep(15, masks=True)
    finally:
        ld.close()
        tb.free()
    assert before[3] > 350 and lane[2] == before[3] and lane[1] == before[0] - before[3]
    kept = [filts[s] & masks[INDEX[s]] for s in range(4)]
    assert all(((filts[s] & 1) >= masks[INDEX[s]]).all() for s in range(4))              # only PF wells are kept
    tb = _upload(sc, reads, kept)
    ld = _lane(sc, tb, INDEX, MAX_TILES, WAYS["a tile per call"], EDGES)
    try:
        after, after_tiles = _finish(ld, k)
        assert after[0] == lane[1] and after[3] == 0 and after[1] == 0                   # PF = Kept, nothing redundant, no class
        assert (after_tiles[:, 0] == trow[:, 1]).all()
        again = ld.keep(15, masks=True)                                # and keeping again keeps everything
        assert again[0][:4].tolist() == [lane[1], lane[1], 0, 0] and again[0][6] == 0
        assert all((again[2][INDEX[s]] == kept[s] & 1).all() for s in range(4))
    finally:
        ld.close()
        tb.free()


# ---- 3: a family that crosses a run and a tile ------------------------------------------------------
def test_families_that_cross_a_run_and_a_tile(sc):
    """2 tiles of 90 x 100 wells - a run of kLaneRun and a bit -, 37 cycles, equal reads: 300 originals in the first run
    of tile 0, each copied, with qualities of its own, into the second, partial run of tile 0, into the first run of
    tile 1 and into its second: families of four wells whose best lies in any of the four places."""
    n, cycles = 90 * 100, 37
    assert RUN < n < 2 * RUN
    rng = np.random.default_rng(9002)
    reads, filts = _random_tiles(rng, 2, n, cycles, pf=0.95)
    src = rng.choice(RUN, 300, replace=False)
    places = [(0, RUN, n), (1, 0, RUN), (1, RUN, n)]                   # (tile, first well, one past the last)
    for t, lo, hi in places:
        dst = lo + rng.choice(hi - lo, 300, replace=False)
        reads[t][dst] = _requalify(reads[0][src], rng.integers(0, 64, (300, cycles)).astype(np.uint8) << 2)
        filts[0][src] = filts[t][dst] = 1
    tiles = _host_tiles(reads, filts, [0, 1])
    fin_lane, fin_tiles, labels = lane_dups(tiles, n, 2)
    want = lane_keep(tiles, n, 2, labels, EDGES, 15)
    kept_copies = np.flatnonzero(np.concatenate([want[2][0], want[2][1]]) & (labels.reshape(-1) != np.arange(2 * n)))
    assert want[0][6] >= 300 and want[0][7] > 150
    for t, lo, hi in places:                                           # a best well in each of the three other places
        assert int(((kept_copies >= t * n + lo) & (kept_copies < t * n + hi)).sum()) >= 30, (t, lo)
    assert want[0][6] - want[0][7] >= 30                               # and roots that stay
    check_keep_identities(want[0], want[1], EDGES, 15, fin_lane, fin_tiles, sum_singles=want[3])
    tb = _upload(sc, reads, filts)
    ld = _lane(sc, tb, [0, 1], 2, [[0, 1]], EDGES)
    try:
        _finish(ld, 0)
        _same(ld.keep(15, masks=True), want)
    finally:
        ld.close()
        tb.free()


# ---- 4: contention ---------------------------------------------------------------------------------
def _ninth_fails(n):
    filt = np.ones(n, dtype=np.uint8)
    filt[::9] = 2                                                      # (only bit 0 counts: every ninth well fails)
    return filt, int((filt & 1).sum())


@pytest.mark.parametrize("k", [0, 1])
def test_a_tile_of_equal_reads_with_one_quality_keeps_its_root(sc, k):
    cycles, q, n = 37, 37, 8193                                        # a run and a well
    reads = [np.tile(np.array([q << 2 | c % 4 for c in range(cycles)], dtype=np.uint8), (n, 1))]
    filt, pf = _ninth_fails(n)
    tb = _upload(sc, reads, [filt])
    ld = _lane(sc, tb, [0], 1, [[0]], EDGES)
    try:
        _finish(ld, k)
        lane, trow, masks = ld.keep(15, masks=True)
        score = 32 * cycles                                            # 37 lies in the bin from 32
        assert lane.tolist() == [pf, 1, pf - 1, 0, score, (pf - 1) * score, 1, 0, score, 1, 0, 0, 0, 0, 0, 0, 0]
        assert trow.tolist() == [lane[:6].tolist()]
        assert np.flatnonzero(masks[0]).tolist() == [1] and masks[0][1] == 1               # well 0 fails the filter: the root is well 1
    finally:
        ld.close()
        tb.free()


def test_a_tile_of_equal_reads_with_random_qualities_keeps_one_well(sc):
    cycles, n = 83, 8193
    rng = np.random.default_rng(83)
    reads = [(np.arange(cycles) % 4 | rng.integers(1, 64, (n, cycles)) << 2).astype(np.uint8)]
    filt, pf = _ninth_fails(n)
    tiles = _host_tiles(reads, [filt], [0])
    fin_lane, fin_tiles, labels = lane_dups(tiles, n, 1)
    want = lane_keep(tiles, n, 1, labels, EDGES, 15)
    score = scores_of(tiles, n, 1, EDGES, 15)
    best = int(np.flatnonzero(want[2][0])[0])
    assert want[0][:4].tolist() == [pf, 1, pf - 1, 1] and want[0][6:8].tolist() == [1, 1] and best > 1
    assert score[best] == score[(filt & 1) != 0].max() and (score[:best][(filt[:best] & 1) != 0] < score[best]).all()
    tb = _upload(sc, reads, [filt])
    ld = _lane(sc, tb, [0], 1, [[0]], EDGES)
    try:
        _finish(ld, 0)
        got = ld.keep(15, masks=True)
        _same(got, want)
        assert np.flatnonzero(got[2][0]).tolist() == [best]            # exactly one well, the reference's
        _same(ld.keep(15, masks=True), want)
    finally:
        ld.close()
        tb.free()


# ---- 5: edges -------------------------------------------------------------------------------------
@pytest.mark.parametrize("edges", [[0], [0, 1, 62, 63], [0, 7, 7, 33]])
def test_keep_at_the_edges(sc, edges):
    """Two tiles of 1500 wells whose qualities are the edges of all three cases, the values beside them, 0 (with a base
    and as a no-call) and 63; copies at 0..1 cycles with qualities of their own from the same set; min_q at, below and
    above an edge."""
    cycles, n, k = 37, 1500, 1
    values = np.array([0, 1, 2, 6, 7, 8, 32, 33, 34, 61, 62, 63], dtype=np.uint8)
    rng = np.random.default_rng(63)
    draw = lambda shape: (values[rng.integers(0, values.size, shape)] << 2 | rng.integers(0, 4, shape)).astype(np.uint8)
    reads = [draw((n, cycles)) for _ in range(2)]                      # (byte 0: quality 0 and base 0, a no-call)
    for i in range(400):
        copy = _requalify(reads[0][i], draw(cycles))
        for c in rng.choice(cycles, i % 2, replace=False).tolist():
            copy[c] = _other_base(copy[c])
        reads[i % 2][700 + i] = copy
    filts = [(rng.random(n) < 0.9).astype(np.uint8) for _ in range(2)]
    tiles = _host_tiles(reads, filts, [1, 0])
    fin_lane, fin_tiles, labels = lane_near_dups(tiles, n, 2, k)
    tb = _upload(sc, reads, filts)
    ld = _lane(sc, tb, [1, 0], 2, [[0, 1]], edges, qual_calls=[[1], [0]])
    try:
        got_lane, got_tiles = _finish(ld, k)
        qhist = ld.qualities(0)[2]
        for min_q in (0, 7, 8, 33, 63):
            want = lane_keep(tiles, n, 2, labels, edges, min_q)
            assert want[0][6] > 250
            weighs = quality_weight(edges, min_q).any()
            assert (want[0][7] > 100) == bool(weighs) and (want[0][4] > 0) == bool(weighs)
            got = ld.keep(min_q, masks=True)
            _same(got, want, (edges, min_q))
            check_keep_identities(got[0], got[1], edges, min_q, got_lane, got_tiles, qhist=qhist, sum_singles=want[3],
                                  masks=got[2], labels=labels)
    finally:
        ld.close()
        tb.free()


# ---- 6: the interface's largest read: the 16-bit score at its bound --------------------------------
def test_1024_cycles_and_the_largest_score(sc):
    """3 tiles of 701 wells, 1024 cycles (103 words: rows that are no whole 16-byte pieces), equal reads and K = 1.  A
    family's copies are called at quality 63 throughout, 62 throughout, or at random: with the edges' last at 63 and
    min_q 0 the first scores 63 x 1024 = 64 512, the largest a score can be."""
    cycles, n = 1024, 701
    rng = np.random.default_rng(1024)
    reads, filts = _random_tiles(rng, 3, n, cycles, pf=0.95)
    reads[0][2][reads[0][2] == 0] = 1                                 # (copy 2 is called at 63 throughout: no no-call in it)
    for i in range(180):
        fresh = np.full(cycles, (63, 62)[i % 2] << 2, dtype=np.uint8) if i % 3 else rng.integers(4, 256, cycles).astype(np.uint8)
        copy = _requalify(reads[0][i], fresh)
        if i % 5 == 0:
            copy[(0, 1023, 511)[i % 3]] = _other_base(copy[(0, 1023, 511)[i % 3]])
        reads[1 + i % 2][300 + i] = copy
    for f in filts:
        f[:180] = 1
        f[300:480] = 1
    index = [0, 2, 1]                                                  # the originals have the smallest ids
    edges = [0, 20, 62, 63]
    tiles = _host_tiles(reads, filts, index)
    top = scores_of(tiles, n, 3, edges, 0).max()
    assert top == 63 * 1024 == 64512                                   # the largest a score can be
    tb = _upload(sc, reads, filts)
    try:
        for k in (0, 1):
            fin_lane, fin_tiles, labels = _labels(tiles, n, 3, k)
            ld = _lane(sc, tb, index, 3, [[0, 1], [2]], edges, qual_calls=[[2], [1, 0]])
            try:
                got_lane, got_tiles = _finish(ld, k)
                for min_q in (0, 63):
                    want = lane_keep(tiles, n, 3, labels, edges, min_q)
                    assert want[0][6] >= (140 if k == 0 else 175) and want[0][7] > 40 and want[0][16] > 40        # gains of 500 and more
                    got = ld.keep(min_q, masks=True)
                    _same(got, want, (k, min_q))
                    check_keep_identities(got[0], got[1], edges, min_q, got_lane, got_tiles, qhist=ld.qualities(0)[2],
                                          sum_singles=want[3])
            finally:
                ld.close()
    finally:
        tb.free()


# ---- 7: call discipline -----------------------------------------------------------------------------
def _raw(sc, ld, min_q, scratch, scratch_bytes, missing=None, keep=None):
    """wd_lane_keep itself -> (rc, lane row, tile rows); missing: the output passed as null; keep: the mask table"""
    out = [np.full(LANE_COLS, -1, dtype=np.int64), np.full((ld.max_tiles, TILE_COLS), -1, dtype=np.int64)]
    ptr = [None if i == missing else a.ctypes.data_as(ctypes.c_void_p) for i, a in enumerate(out)]
    rc = sc._lib.wd_lane_keep(ld._h, min_q, ctypes.c_void_p(scratch), scratch_bytes, *ptr, keep)
    return (rc,) + tuple(out)


def _untouched(res):
    return all((a == -1).all() for a in res[1:])


def test_call_discipline(sc):
    k, cycles = 1, 37
    reads, filts = _fed_lane(k, cycles)
    tiles = _host_tiles(reads, filts, INDEX)
    want = lane_keep(tiles, N, MAX_TILES, lane_near_dups(tiles, N, MAX_TILES, k)[2], EDGES, 15)
    want_eq = lane_keep(tiles, N, MAX_TILES, lane_dups(tiles, N, MAX_TILES)[2], EDGES, 15)
    need = sc.lane_keep_scratch_bytes(MAX_TILES, N)
    d_scratch = sc.malloc(need)
    sc.memset(d_scratch, 0x5A, need)                                   # dirty
    d_mask = sc.malloc(MAX_TILES * N)
    sc.memset(d_mask, 0x77, MAX_TILES * N)
    host = np.full(max(need, N), 0x33, dtype=np.uint8)
    table = lambda ptrs: (ctypes.c_void_p * MAX_TILES)(*ptrs)
    dev_masks = table([d_mask + t * N for t in range(MAX_TILES)])      # a mask for every index, added or not
    mask_of = lambda t: sc.d2h(d_mask + t * N, N, np.uint8)
    tb = _upload(sc, reads, filts)
    umi_tb = TileBatch(sc, len(reads), 8, N)                           # UMI reads: the first eight cycles, again
    for i, r in enumerate(reads):
        umi_tb.upload_tile(i, [np.ascontiguousarray(r[:, c]) for c in range(8)], filts[i])
    ld = LaneDups(sc, N, MAX_TILES, cycles)
    try:
        for slots in WAYS["1 + 3"]:
            ld.add_tables([INDEX[s] for s in slots], _tables(tb, slots))
        _finish(ld, k)
        res = _raw(sc, ld, 15, d_scratch, need)                        # no quality part
        assert res[0] == _lib.ERR_ARG and _untouched(res) and b"wd_lane_qual_begin" in sc._lib.wd_last_error(sc._ctx)
        with pytest.raises(ValueError):
            ld.keep(15)
        ld.restart()
        ld.qual_begin(EDGES)
        ld.umi_begin(8)
        for slots in WAYS["1 + 3"]:
            ld.add_tables([INDEX[s] for s in slots], _tables(tb, slots))
        ld.umi_add(umi_tb, INDEX)
        ld.qual_add(_tables(tb, [0, 1]), [INDEX[0], INDEX[1]])
        res = _raw(sc, ld, 15, d_scratch, need, keep=dev_masks)        # before any finish
        assert res[0] == _lib.ERR_ARG and _untouched(res) and b"finish" in sc._lib.wd_last_error(sc._ctx)
        with pytest.raises(ValueError):
            ld.keep(15)
        with pytest.raises(RuntimeError):                              # a near finish refused over budget is no finish
            ld.finish(hamming=k, pair_budget=3)
        res = _raw(sc, ld, 15, d_scratch, need, keep=dev_masks)
        assert res[0] == _lib.ERR_ARG and _untouched(res) and b"finish" in sc._lib.wd_last_error(sc._ctx)
        # a tile with reads but no qualities: slots 2 and 3 have none
        _finish(ld, k)
        res = _raw(sc, ld, 15, d_scratch, need, keep=dev_masks)
        assert res[0] == _lib.ERR_ARG and _untouched(res)
        assert b"tile index %d was added without qualities" % min(INDEX[2:]) in sc._lib.wd_last_error(sc._ctx)
        with pytest.raises(ValueError):
            ld.keep(15)
        # and the reverse: qualities for an index that was never added
        ld.restart()
        ld.add_tables([INDEX[0]], _tables(tb, [0]))
        ld.umi_add(umi_tb, INDEX)
        ld.qual_add(_tables(tb, [0, 1]), [INDEX[0], INDEX[1]])
        _finish(ld, 0)
        res = _raw(sc, ld, 15, d_scratch, need, keep=dev_masks)
        assert res[0] == _lib.ERR_ARG and _untouched(res)
        assert b"tile index %d got qualities but was never added" % INDEX[1] in sc._lib.wd_last_error(sc._ctx)
        assert (mask_of(0) == 0x77).all() and (mask_of(INDEX[0]) == 0x77).all()            # no mask was touched by any of these
        # the lane again, complete
        ld.restart()
        for slots in WAYS["descending indices"]:
            ld.add_tables([INDEX[s] for s in slots], _tables(tb, slots))
        ld.umi_add(umi_tb, INDEX)
        for slots in WAYS["a tile per call"]:
            ld.qual_add(_tables(tb, slots), [INDEX[s] for s in slots])
        _finish(ld, k)
        host_masks = table([None] * 3 + [host.ctypes.data] + [None] * 2)
        for bad in ((-1, d_scratch, need), (64, d_scratch, need), (15, 0, need), (15, d_scratch, need - 256), (15, d_scratch, 0),
                    (15, host.ctypes.data, need)):
            res = _raw(sc, ld, *bad, keep=dev_masks)
            assert res[0] == _lib.ERR_ARG and _untouched(res), bad
        res = _raw(sc, ld, 15, d_scratch, need, keep=host_masks)       # a mask pointer in host memory
        assert res[0] == _lib.ERR_ARG and _untouched(res) and (host == 0x33).all()
        assert b"mask of tile index 3 must be in device memory" in sc._lib.wd_last_error(sc._ctx)
        for missing in range(2):
            res = _raw(sc, ld, 15, d_scratch, need, missing=missing, keep=dev_masks)
            assert res[0] == _lib.ERR_ARG and _untouched(res)
        for q in (-1, 64):
            with pytest.raises(ValueError):
                ld.keep(q)
        assert all((mask_of(t) == 0x77).all() for t in range(MAX_TILES))
        first = _raw(sc, ld, 15, d_scratch, need, keep=dev_masks)      # the caller's scratch, dirty; a mask for every index
        assert first[0] == _lib.OK
        _same(first[1:], want)
        for t in range(MAX_TILES):                                     # a tile never added: zeros
            assert (mask_of(t) == (want[2][t] if t in want[2] else 0)).all(), t
        some = table([d_mask + t * N if t in (0, 5) else None for t in range(MAX_TILES)])    # masks for some tiles only
        sc.memset(d_mask, 0x77, MAX_TILES * N)
        res = _raw(sc, ld, 15, d_scratch, need, keep=some)
        assert res[0] == _lib.OK
        _same(res[1:], want)
        for t in range(MAX_TILES):
            assert (mask_of(t) == (want[2][t] if t in (0, 5) else 0x77)).all(), t
        res = _raw(sc, ld, 15, d_scratch, need)                        # and for none
        assert res[0] == _lib.OK
        _same(res[1:], want)
        _same(ld.keep(15, masks=True), want)                           # twice the same (identity 7)
        gc = ld.gc(0)
        _same(ld.keep(15, masks=True), want)                           # after the GC pass,
        umi = ld.umi(1, 64)
        _same(ld.keep(15, masks=True), want)                           # the UMI pass
        ld.qualities(1)
        ld.saturation(20)
        _same(ld.keep(15, masks=True), want)                           # and two more,
        assert all((a == b).all() for a, b in zip(gc, ld.gc(0))) and all((a == b).all() for a, b in zip(umi, ld.umi(1, 64)))      # which found the lane as they left it
        # another lane in the same workspaces, by equality
        ld.restart()
        with pytest.raises(ValueError):
            ld.keep(15)
        for slots in WAYS["one call"]:
            ld.qual_add(_tables(tb, slots), [INDEX[s] for s in slots])
            ld.add_tables([INDEX[s] for s in slots], _tables(tb, slots))
        ld.umi_add(umi_tb, INDEX)
        _finish(ld, 0)
        _same(ld.keep(15, masks=True), want_eq)
        ld.close()
        with pytest.raises(ValueError):
            ld.keep(15)
    finally:
        ld.close()
        umi_tb.free()
        tb.free()
        sc.free(d_scratch)
        sc.free(d_mask)


def test_a_lane_without_tiles_or_wells(sc):
    ld = LaneDups(sc, N, 3, 37)
    try:
        ld.qual_begin(EDGES)
        ld.finish()
        lane, trow, masks = ld.keep(15, masks=True)
        assert not lane.any() and not trow.any() and masks == {} and trow.shape == (3, TILE_COLS)
    finally:
        ld.close()
    ld = LaneDups(sc, 0, 3, 37)
    try:
        ld.qual_begin(EDGES)
        ld.finish()
        lane, trow = ld.keep(0)
        assert not lane.any() and not trow.any()
    finally:
        ld.close()


# ---- 8: the CLI -------------------------------------------------------------------------------------
def _main(argv):
    out = io.StringIO()
    with redirect_stdout(out):
        assert cwd.main(argv) == 0
    return out.getvalue()


def test_cli_lane_keep_block_and_filter_files(tmp_path):
    """The run directory of test_gpu_lanequality.py's CLI test: 2 lanes x 4 tiles; in each lane tile 1103's files are
    tile 1101's but for the last cycle, which is tile 1102's - copies one cycle apart whose last base is called at
    another quality.  The new block closes each lane's output and equals write_lane_keep of the reference; the filter
    files written are the reference's masks; and the run directory with them in place of its own has no redundant well
    left."""
    rows, cols, levels, k, L = 24, 50, 3, 1, 20                        # (smaller than there: four runs of the CLI)
    n = rows * cols
    x, y = synth.honeycomb_pixels(rows, cols)
    spec = synth.SynthSpec(seed=35, n_clusters=n, row=cols, plant_per_64k=8000, nocall_per_64k=500, plant_far=True)
    run_dir = str(tmp_path / "run")
    names = ["1101", "1102", "1103", "1104"]
    synth.write_run_dir(spec, run_dir, [1, 2], names, list(range(L)), slocs=synth.slocs_bytes(x, y))
    source = lambda t, c: "1101" if t == "1103" and c < L - 1 else "1102" if t == "1103" else t
    for lane in (1, 2):
        ldir = os.path.join(run_dir, "Data", "Intensities", "BaseCalls", "L%03d" % lane)
        shutil.copy(os.path.join(ldir, "s_%d_1101.filter" % lane), os.path.join(ldir, "s_%d_1103.filter" % lane))
        for c in range(L):
            cdir = os.path.join(ldir, "C%d.1" % (c + 1))
            shutil.copy(os.path.join(cdir, "s_%d_%s.bcl.gz" % (lane, source("1103", c))),
                        os.path.join(cdir, "s_%d_1103.bcl.gz" % lane))
    base = ["-s", "hiseq_x", "-r", run_dir, "-t", "1101,1102,1103,1104", "-i", "1,2", "-l", str(levels),
            "--cycles", "0-%d" % L, "-q", "--all-wells", "--lane-dups"]
    argv = base + ["--lane-dups-hamming", str(k)]
    edges = cwd.DEFAULT_QUALITY_BINS
    blocks, wants, filters = {}, {}, {}
    for lane in (1, 2):
        filters[lane] = [synth.filter_bytes(spec, lane, int(t if t != "1103" else "1101")) for t in names]
        tiles = [(i, [synth.plane_bytes(spec, lane, int(source(t, c)), c) for c in range(L)], filters[lane][i])
                 for i, t in enumerate(names)]
        for kk, min_q in ((k, 15), (0, 30)):
            labels = _labels(tiles, n, 4, kk)[2]
            wants[(lane, kk)] = res = lane_keep(tiles, n, 4, labels, edges, min_q)
            counts = report.LaneKeepCounts.from_rows(res[0], res[1], names, kk, min_q, edges, L)
            assert counts.families > 200 and counts.moved > (200 if kk else 40)
            for summary in (False, True):
                text = io.StringIO()
                report.write_lane_keep(str(lane), counts, verbose=not summary, out=text)
                blocks[(summary, lane, kk)] = text.getvalue()
    plain = _main(argv)
    out_dir = str(tmp_path / "dedup")
    run = _main(argv + ["--lane-dups-keep", "--lane-dups-keep-out", out_dir, "--tile-batch", "3"])
    b1, b2 = blocks[(False, 1, k)], blocks[(False, 2, k)]
    assert run.count(b1) == 1 and run.endswith(b2)
    assert run.replace(b1, "", 1)[:-len(b2)] == plain                  # minus the new blocks: the output without the flag
    assert run.index("LaneNearDupsSummary: 1") < run.index(b1) < run.index("LaneDupsSummary: 2")
    assert b1.count("LaneKeep: 1\tTile: ") == 4 and "LaneKeepSummary: 1\tTiles: 4\tHamming: 1\tMinQ: 15\t" in b1
    # one file per scanned tile, named as the tile's own, holding the reference's mask under the input's other bits
    for lane in (1, 2):
        written = sorted(os.listdir(os.path.join(out_dir, "L%03d" % lane)))
        assert written == ["s_%d_%s.filter" % (lane, t) for t in names]
        for i, t in enumerate(names):
            got = bcl.Tile(os.path.join(out_dir, "L%03d" % lane), t).read_filter()
            assert (got & 1 == wants[(lane, k)][2][i]).all() and (got & 0xFE == filters[lane][i] & 0xFE).all()
    assert sorted(os.listdir(out_dir)) == ["L001", "L002"]
    # -S, after every other block of the lane, beside --lane-dups-quality with bins given once, under equality
    full = _main(base + ["-S", "--lane-dups-keep", "--lane-dups-keep-min-q", "30", "--lane-dups-quality", "--lane-dups-gc"])
    b1, b2 = blocks[(True, 1, 0)], blocks[(True, 2, 0)]
    assert full.count(b1) == 1 and full.endswith(b2) and "LaneKeep: 1\tTile" not in b1 and "\tMinQ: 30\t" in b1
    assert full.index("LaneGCSummary: 1") < full.index(b1) < full.index("LaneDupsSummary: 2")
    assert full.index("LaneQualitiesSummary: 1") < full.index(b1) and "LaneQualitiesSummary: 2" in full
    # a copy of the run directory with the written files in place of its own, run with --lane-dups alone
    dedup_run = str(tmp_path / "run2")
    shutil.copytree(run_dir, dedup_run)
    for lane in (1, 2):
        for t in names:
            shutil.copy(os.path.join(out_dir, "L%03d" % lane, "s_%d_%s.filter" % (lane, t)),
                        os.path.join(dedup_run, "Data", "Intensities", "BaseCalls", "L%03d" % lane))
    again = _main([dedup_run if a == run_dir else a for a in argv] + ["-S"])
    for lane in (1, 2):
        kept = int(wants[(lane, k)][0][1])
        m = re.search(r"LaneNearDupsSummary: %d\tTiles: 4\tHamming: 1\tPF wells: (\d+)\t.*?\tRedundant: (\d+) " % lane, again)
        assert m and (int(m.group(1)), int(m.group(2))) == (kept, 0), (lane, m and m.groups(), kept)
        m = re.search(r"LaneDupsSummary: %d\tTiles: 4\tPF wells: (\d+)\t.*?\tRedundant: (\d+) " % lane, again)
        assert m and (int(m.group(1)), int(m.group(2))) == (kept, 0)
