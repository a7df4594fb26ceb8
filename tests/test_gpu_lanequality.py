"""A lane's reported base quality against its duplicate copies on the GPU (LaneDups.qual_begin / qual_add / qualities,
include/welldup_lanequality.h) against the host reference of tests/lanequality_ref.py on the labels of
tests/lanenear_ref.py / lanedups_ref.py - lane row, tile rows, QHist, Obs and Mis equal, nothing approximate - however
the tiles are fed and whatever hash_bits, and against the identities the header states."""
import ctypes
import io
import os
import re
import shutil
from contextlib import redirect_stdout

import numpy as np
import pytest

from lanedups_ref import lane_dups
from lanemismatch_ref import lane_mismatches
from lanenear_ref import lane_near_dups
from lanequality_ref import check_quality_identities, lane_qualities
from well_duplicates_amd import _lib
from well_duplicates_amd import count_well_duplicates as cwd
from well_duplicates_amd import report, synth
from well_duplicates_amd.scanner import LaneDups, Scanner, TileBatch

pytestmark = pytest.mark.gpu

ROWS, COLS = 44, 60
N = ROWS * COLS
TILES = [(1, 1101), (1, 1102), (1, 1103), (2, 1101), (2, 1103)]      # (1, 1102) is dead
INDEX = [5, 0, 3, 6, 1]                                               # slot -> tile index in a lane of MAX_TILES
MAX_TILES = 7                                                         # (indices 2 and 4 are never added)
WAYS = {"one call": [[0, 1, 2, 3, 4]], "a tile per call": [[0], [1], [2], [3], [4]], "2 + 3": [[0, 1], [2, 3, 4]],
        "descending indices": [[3], [0], [2], [4], [1]]}
QUAL_WAYS = {"one call": "2 + 3", "a tile per call": "one call", "2 + 3": "descending indices",
             "descending indices": "a tile per call"}                 # the qualities come batched otherwise than the reads
EDGES = [0, 2, 8, 14, 20, 26, 32, 38]                                 # the synthetic planes hold 0 and 2..40: every bin occurs
NAMES = ("lane row", "tile rows", "qhist", "obs", "mis")

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
    if k == 0:
        return ld.finish()[:2]
    got = ld.finish(hamming=k, pair_budget=1 << 27 if hash_bits == 1 else 0)      # (two buckets hold every read)
    return got[3], got[4]


def _same(got, want):
    for g, w, name in zip(got, want, NAMES):
        assert g.shape == w.shape and (g == w).all(), (name, g[g != w], w[g != w], np.argwhere(g != w)[:8])


def _other_base(b):
    """the byte with another base and the same quality, never 0 (a no-call becomes a base of quality 0)"""
    b = int(b)
    return (b & 0xFC) | ((b + 1) & 3) if b & 0xFC else 1 + (b & 3) % 3


def _requalify(read, fresh):
    """the read with the quality bits of `fresh`; a no-call stays one, and no base becomes a no-call"""
    new = (read & 3) | (fresh & 0xFC)
    return np.where(read == 0, 0, np.where(new == 0, read, new)).astype(np.uint8)


def _plant(reads, rng, src_tile, dst_tile, count, mismatches, requalify=True):
    """copies of `count` reads of src_tile on dst_tile, copy i with 1 + i % mismatches cycles changed (0: none);
    requalify: a copy's bases are called with qualities of their own, 2..40 (a no-call stays one)"""
    n, cycles = reads[0].shape
    a, b = rng.choice(n, count, replace=False), rng.choice(n, count, replace=False)
    copy = reads[src_tile][a].copy()
    if requalify:
        copy = _requalify(copy, rng.integers(2, 41, copy.shape).astype(np.uint8) << 2)
    reads[dst_tile][b] = copy
    for i, w in enumerate(b.tolist()):
        if mismatches:
            for c in rng.choice(cycles, min(cycles, 1 + i % mismatches), replace=False).tolist():
                reads[dst_tile][w, c] = _other_base(reads[dst_tile][w, c])


def _small_lane(k, cycles):
    """The lane of test_gpu_lanemismatch.py at `cycles` cycles: five synthetic tiles (39 quality levels and no-calls;
    copies planted inside every tile, one tile dead) and near copies at 1 .. k + 1 mismatches planted within tiles and
    across tiles (chains: a copy of a copy), the copies with qualities of their own."""
    spec = synth.SynthSpec(seed=91, n_clusters=N, row=COLS, plant_per_64k=8000, nocall_per_64k=400, dead_tiles=(1102,),
                           plant_far=True, filter_noise=True)
    assert spec.qual_levels == 39
    reads = [np.stack([synth.plane_bytes(spec, ln, t, c) for c in range(cycles)], axis=1) for ln, t in TILES]
    filts = [synth.filter_bytes(spec, ln, t) for ln, t in TILES]
    rng = np.random.default_rng(17 + k)
    for src, dst, count in ((0, 2, 300), (2, 3, 200), (0, 4, 150), (3, 4, 100), (0, 1, 50), (0, 0, 120), (3, 3, 120)):
        _plant(reads, rng, src, dst, count, k + 1)
    _plant(reads, rng, 2, 4, 80, 0)                                    # and equal reads across tiles
    return reads, filts


def _pf(filts):
    return int(sum(int((f & 1).sum()) for f in filts))


# ---- 1: the lane of test_gpu_lanemismatch.py ------------------------------------------------------
@pytest.mark.parametrize("cycles", [37, 83])         # a partial last word in 16-byte pieces; nine words
@pytest.mark.parametrize("k", [1, 2, 3])
def test_lane_qualities_match_reference_however_the_tiles_are_fed(sc, k, cycles):
    reads, filts = _small_lane(k, cycles)
    tiles = _host_tiles(reads, filts, INDEX)
    labels = lane_near_dups(tiles, N, MAX_TILES, k)[2]
    depths = (0, k, 7)
    want = {d: lane_qualities(tiles, N, MAX_TILES, labels, d, EDGES) for d in depths}
    mism = {d: lane_mismatches(tiles, N, MAX_TILES, labels, d) for d in depths}
    # the ground is covered: all eight bins among roots and members, mismatches in most cells, a pair beyond max_d
    lane, obs, mis = want[k][0], want[k][3], want[k][4]
    assert (obs.sum(axis=0) > 0).all() and (obs.sum(axis=1) > 0).all() and (mis > 0).sum() > 32
    assert want[0][0][1] < lane[1] < lane[0] and lane[3] > 200 and (want[k][2][[0] + list(range(2, 41))] > 0).all()
    for d in depths:
        check_quality_identities(*want[d], d, cycles, 8, mismatch=mism[d], pf_wells=_pf(filts),
                                 shallower=want[0] if d == k else want[k] if d == 7 else None)
    tb = _upload(sc, reads, filts)
    try:
        for bits in (0, 4, 1):
            for way, calls in WAYS.items():
                ld = _lane(sc, tb, INDEX, MAX_TILES, calls, EDGES, qual_calls=WAYS[QUAL_WAYS[way]], hash_bits=bits,
                           qual_first=way == "2 + 3")
                try:
                    _finish(ld, k, bits)
                    for d in depths:
                        got = ld.qualities(d)
                        _same(got, want[d])
                        check_quality_identities(*got, d, cycles, 8, mismatch=ld.mismatches(d), pf_wells=_pf(filts))
                finally:
                    ld.close()
    finally:
        tb.free()


# ---- 1b: pairs across runs and tiles -----------------------------------------------------------------
def test_pairs_that_cross_a_run_or_a_tile(sc):
    """The lane of test_gpu_lanemismatch.py's test of this name, the copies with qualities of their own: 2 tiles of
    90 x 100 wells - a run of kLaneRun and a bit -, 20 cycles, random reads, K = 2, max_d = 2.  300 originals in the
    first run of tile 0, each copied once at 0, 1 or 2 mismatches: 100 copies into the second, partial run of tile 0,
    100 into the first run of tile 1 and 100 into its second.  So a root sits in the first run of tile 0 and its member
    in one of the other three places - at least one pair in each, held to below on the reference's labels -: every
    pair crosses a run or a tile, and k_lq_tally takes a second run."""
    n, cycles, k = 90 * 100, 20, 2
    assert RUN < n < 2 * RUN
    rng = np.random.default_rng(9001)
    reads = [rng.integers(1, 256, (n, cycles)).astype(np.uint8) for _ in range(2)]
    for r in reads:
        r[rng.random(r.shape) < 0.005] = 0
    filts = [(rng.random(n) < 0.95).astype(np.uint8) for _ in range(2)]
    src = rng.choice(RUN, 300, replace=False)
    places = [(0, RUN, n), (1, 0, RUN), (1, RUN, n)]                   # (tile, first well, one past the last)
    for p, (t, lo, hi) in enumerate(places):
        dst = lo + rng.choice(hi - lo, 100, replace=False)
        for i, (a, b) in enumerate(zip(src[100 * p:100 * p + 100].tolist(), dst.tolist())):
            reads[t][b] = _requalify(reads[0][a], rng.integers(2, 41, cycles).astype(np.uint8) << 2)
            for c in rng.choice(cycles, i % 3, replace=False).tolist():
                reads[t][b, c] = _other_base(reads[t][b, c])
            filts[0][a] = filts[t][b] = 1
    tiles = _host_tiles(reads, filts, [0, 1])
    labels = lane_near_dups(tiles, n, 2, k)[2]
    want = lane_qualities(tiles, n, 2, labels, k, EDGES)
    mism = lane_mismatches(tiles, n, 2, labels, k)
    flat = labels.reshape(-1)
    member = np.flatnonzero((flat != 0xFFFFFFFF) & (flat != np.arange(flat.size)))
    assert member.size >= 300 and (flat[member] < RUN).all()           # every root in the first run of tile 0
    for t, lo, hi in places:                                           # and members in each of the other three places
        assert int(((member >= t * n + lo) & (member < t * n + hi)).sum()) >= 100, (t, lo)
    assert want[0][1] >= 300 and want[0][3] >= 250 and (want[3] > 0).sum() > 32 and (mism[0][4:7] >= 90).all()
    check_quality_identities(*want, k, cycles, 8, mismatch=mism, pf_wells=_pf(filts))
    tb = _upload(sc, reads, filts)
    ld = _lane(sc, tb, [0, 1], 2, [[0, 1]], EDGES)
    try:
        _finish(ld, k)
        got = ld.qualities(k)
        _same(got, want)
        check_quality_identities(*got, k, cycles, 8, mismatch=ld.mismatches(k), pf_wells=_pf(filts))
    finally:
        ld.close()
        tb.free()


# ---- 2: every cell at every awkward position ------------------------------------------------------
@pytest.mark.parametrize("cycles", [37, 83])
def test_every_cell_at_every_awkward_position(sc, cycles):
    """A lane per position: wells 0..63 are random reads, every base of bin 3 but at the position, where read
    8 a + b has bin a; well 64 + 8 a + b is its copy with another base there, every base of bin 5 but at the position,
    where it has bin b.  Mis is all ones, Obs the same plus 64 (L - 1) in cell (3, 5)."""
    edges = [0, 8, 16, 24, 32, 40, 48, 56]
    byte = lambda bin_, base: np.uint8((8 * bin_ + 1) << 2 | base)
    rng = np.random.default_rng(64)
    for at in (0, 9, 10, 19, 29, 30, cycles - 1):
        bases = rng.integers(0, 4, (64, cycles))
        reads = np.zeros((128 + 5, cycles), dtype=np.uint8)
        reads[:64] = byte(3, bases)
        reads[64:128] = byte(5, bases)
        for a in range(8):
            for b in range(8):
                reads[8 * a + b, at] = byte(a, bases[8 * a + b, at])
                reads[64 + 8 * a + b, at] = byte(b, (bases[8 * a + b, at] + 1) & 3)
        reads[128:] = byte(7, rng.integers(0, 4, (5, cycles)))         # and wells that are not PF
        filt = np.ones(len(reads), dtype=np.uint8)
        filt[128:] = 0
        want_mis = np.ones((8, 8), dtype=np.int64)
        want_obs = want_mis.copy()
        want_obs[3, 5] += 64 * (cycles - 1)
        tiles = _host_tiles([reads], [filt], [1])
        labels = lane_near_dups(tiles, len(reads), 2, 1)[2]
        ref = lane_qualities(tiles, len(reads), 2, labels, 1, edges)
        assert ref[0].tolist() == [64, 64, 64 * cycles, 64] and (ref[3] == want_obs).all() and (ref[4] == want_mis).all()
        tb = _upload(sc, [reads], [filt])
        ld = _lane(sc, tb, [1], 2, [[0]], edges)
        try:
            _finish(ld, 1)
            for d in (1, 7):
                got = ld.qualities(d)
                _same(got, ref)
                assert got[1].tolist() == [[0] * 4, [64, 64, 64 * cycles, 64]]
            lane, trow, qhist, obs, mis = ld.qualities(0)
            assert lane.tolist() == [64, 0, 0, 0] and not obs.any() and not mis.any() and (qhist == ref[2]).all()
        finally:
            ld.close()
            tb.free()


# ---- 3: edges -------------------------------------------------------------------------------------
@pytest.mark.parametrize("edges", [[0, 2, 10, 20, 25, 30, 35, 40], [0], [0, 1, 62, 63], [0, 7, 7, 33]])
def test_qualities_at_the_edges(sc, edges):
    """Two tiles whose qualities are the edges of the CLI's default bins, the values below them, 0 (with a base and as
    a no-call) and 63; copies at 0..2 cycles with qualities of their own from the same set."""
    cycles, n, k = 41, 1500, 2
    values = np.array(sorted({0, 63} | {e for e in cwd.DEFAULT_QUALITY_BINS} | {e - 1 for e in cwd.DEFAULT_QUALITY_BINS if e}),
                      dtype=np.uint8)
    rng = np.random.default_rng(63)
    draw = lambda shape: (values[rng.integers(0, values.size, shape)] << 2 | rng.integers(0, 4, shape)).astype(np.uint8)
    reads = [draw((n, cycles)) for _ in range(2)]                      # (byte 0: quality 0 and base 0, a no-call)
    for i in range(400):
        copy = _requalify(reads[0][i], draw(cycles))
        for c in rng.choice(cycles, i % 3, replace=False).tolist():
            copy[c] = _other_base(copy[c])
        reads[i % 2][700 + i] = copy
    filts = [(rng.random(n) < 0.9).astype(np.uint8) for _ in range(2)]
    tiles = _host_tiles(reads, filts, [1, 0])
    labels = lane_near_dups(tiles, n, 2, k)[2]
    want = lane_qualities(tiles, n, 2, labels, k, edges)
    seen = np.bincount(np.concatenate([(r[(f & 1).astype(bool)] >> 2).reshape(-1) for r, f in zip(reads, filts)]), minlength=64)
    assert (want[2] == seen).all() and set(np.flatnonzero(seen).tolist()) == set(values.tolist())
    assert want[0][1] > 250 and want[0][3] > 150
    check_quality_identities(*want, k, cycles, len(edges), mismatch=lane_mismatches(tiles, n, 2, labels, k), pf_wells=_pf(filts))
    tb = _upload(sc, reads, filts)
    ld = _lane(sc, tb, [1, 0], 2, [[0, 1]], edges, qual_calls=[[1], [0]])
    try:
        _finish(ld, k)
        got = ld.qualities(k)
        _same(got, want)
        assert (got[2] == seen).all()
        check_quality_identities(*got, k, cycles, len(edges), mismatch=ld.mismatches(k), pf_wells=_pf(filts))
    finally:
        ld.close()
        tb.free()


# ---- 4: the interface's largest read --------------------------------------------------------------
def test_1024_cycles(sc):
    """3 tiles of 601 wells, 1024 cycles (103 words: rows that are no whole 16-byte pieces), K = 2: copies with one or
    two cycles changed, at 0, at 1023 and in between, and copies of copies."""
    cycles, n, k = 1024, 601, 2
    rng = np.random.default_rng(1024)
    reads = [rng.integers(1, 256, (n, cycles)).astype(np.uint8) for _ in range(3)]
    for r in reads:
        r[rng.random(r.shape) < 0.005] = 0
    cuts = [[0], [cycles - 1], [9, 10], [1019, 1020], [511], []]
    for i in range(180):
        copy = _requalify(reads[0][i], rng.integers(4, 256, cycles).astype(np.uint8))
        for c in cuts[i % len(cuts)]:
            copy[c] = _other_base(copy[c])
        reads[1][300 + i] = copy
        if i % 2:                                                      # a chain: a copy of tile 1's copy, two further on
            reads[2][300 + i] = copy
            for c in (5, 700):
                reads[2][300 + i, c] = _other_base(reads[2][300 + i, c])
    filts = [(rng.random(n) < 0.95).astype(np.uint8) for _ in range(3)]
    for f in filts:
        f[:180] = 1
        f[300:480] = 1
    index = [0, 2, 1]                                                  # the originals have the smallest ids
    edges = [0, 5, 13, 21, 29, 37, 45, 53]
    tiles = _host_tiles(reads, filts, index)
    labels = lane_near_dups(tiles, n, 3, k)[2]
    want = {d: lane_qualities(tiles, n, 3, labels, d, edges) for d in (0, 2, 7)}
    assert want[7][0][0] >= 270 and want[2][0][1] < want[7][0][1] and (want[2][3] > 0).all()
    tb = _upload(sc, reads, filts)
    ld = _lane(sc, tb, index, 3, [[0, 1], [2]], edges, qual_calls=[[2], [1, 0]])
    try:
        _finish(ld, k)
        for d in (0, 2, 7):
            got = ld.qualities(d)
            _same(got, want[d])
            check_quality_identities(*got, d, cycles, 8, mismatch=ld.mismatches(d), pf_wells=_pf(filts))
    finally:
        ld.close()
        tb.free()


# ---- 5: contention ----------------------------------------------------------------------------------
def _ninth_fails():
    filt = np.ones(N, dtype=np.uint8)
    filt[::9] = 2                                                      # (only bit 0 counts: every ninth well fails)
    return filt, int((filt & 1).sum())


def test_a_tile_of_equal_reads_with_one_quality_is_one_cell(sc):
    cycles, q = 40, 37
    reads = [np.tile(np.array([q << 2 | c % 4 for c in range(cycles)], dtype=np.uint8), (N, 1))]
    filt, pf = _ninth_fails()
    edges = [0, 2, 10, 20, 25, 30, 35, 40]                             # 37 lies in bin 6
    tb = _upload(sc, reads, [filt])
    try:
        for k in (0, 1):
            ld = _lane(sc, tb, [0], 1, [[0]], edges)
            try:
                _finish(ld, k)
                lane, trow, qhist, obs, mis = ld.qualities(3)
                assert lane.tolist() == [pf - 1, pf - 1, (pf - 1) * cycles, 0] and trow.tolist() == [lane.tolist()]
                assert obs[6, 6] == (pf - 1) * cycles == obs.sum() and not mis.any()
                assert qhist[q] == pf * cycles == qhist.sum()
            finally:
                ld.close()
    finally:
        tb.free()


def test_a_tile_of_equal_reads_with_random_qualities(sc):
    cycles = 40
    rng = np.random.default_rng(40)
    reads = [(np.arange(cycles) % 4 | rng.integers(1, 64, (N, cycles)) << 2).astype(np.uint8)]
    filt, pf = _ninth_fails()
    edges = [0, 8, 16, 24, 32, 40, 48, 56]
    tiles = _host_tiles(reads, [filt], [0])
    want = lane_qualities(tiles, N, 1, lane_dups(tiles, N, 1)[2], 0, edges)
    assert want[0].tolist() == [pf - 1, pf - 1, (pf - 1) * cycles, 0] and (want[3] > 0).all()
    tb = _upload(sc, reads, [filt])
    ld = _lane(sc, tb, [0], 1, [[0]], edges)
    try:
        _finish(ld, 0)
        _same(ld.qualities(0), want)
        _same(ld.qualities(7), want)
    finally:
        ld.close()
        tb.free()


def test_2000_copies_changed_alike_fill_one_entry(sc):
    cycles, at = 40, 23
    rng = np.random.default_rng(2000)
    reads = [(rng.integers(0, 4, (N, cycles)) | 30 << 2).astype(np.uint8)]             # every base at quality 30
    reads[0][0, at] = 30 << 2 | 2                                      # the original has G there, every copy T at quality 7
    reads[0][1:2001] = reads[0][0]
    reads[0][1:2001, at] = 7 << 2 | 3
    filt = np.ones(N, dtype=np.uint8)
    edges = [0, 20]
    tb = _upload(sc, reads, [filt])
    ld = _lane(sc, tb, [0], 1, [[0]], edges)
    try:
        assert _finish(ld, 1)[0][3] == 2000
        lane, trow, qhist, obs, mis = ld.qualities(1)
        assert lane.tolist() == [2000, 2000, 2000 * cycles, 2000] and trow.tolist() == [lane.tolist()]
        assert obs[:2, :2].tolist() == [[0, 0], [2000, 2000 * (cycles - 1)]] and obs.sum() == 2000 * cycles
        assert mis[:2, :2].tolist() == [[0, 0], [2000, 0]] and mis.sum() == 2000
        assert qhist[7] == 2000 and qhist[30] == N * cycles - 2000 and qhist.sum() == N * cycles
    finally:
        ld.close()
        tb.free()


# ---- 6: call discipline -----------------------------------------------------------------------------
def _raw(sc, ld, max_d, scratch, scratch_bytes, missing=None):
    """wd_lane_qualities itself -> (rc, lane row, tile rows, qhist, obs, mis); missing: the output passed as null"""
    out = [np.full(4, -1, dtype=np.int64), np.full((ld.max_tiles, 4), -1, dtype=np.int64), np.full(64, -1, dtype=np.int64),
           np.full((8, 8), -1, dtype=np.int64), np.full((8, 8), -1, dtype=np.int64)]
    ptr = [None if i == missing else a.ctypes.data_as(ctypes.c_void_p) for i, a in enumerate(out)]
    rc = sc._lib.wd_lane_qualities(ld._h, max_d, ctypes.c_void_p(scratch), scratch_bytes, *ptr)
    return (rc,) + tuple(out)


def _untouched(res):
    return all((a == -1).all() for a in res[1:])


def _begin(sc, ld, edges, ws, ws_bytes):
    e = (ctypes.c_int * max(1, len(edges)))(*edges)
    return sc._lib.wd_lane_qual_begin(ld._h, len(edges), e, ctypes.c_void_p(ws), ws_bytes)


def test_call_discipline(sc):
    k, cycles = 2, 37
    reads, filts = _small_lane(k, cycles)
    tiles = _host_tiles(reads, filts, INDEX)
    labels = lane_near_dups(tiles, N, MAX_TILES, k)[2]
    want = lane_qualities(tiles, N, MAX_TILES, labels, k, EDGES)
    eq_labels = lane_dups(tiles, N, MAX_TILES)[2]
    want_eq = lane_qualities(tiles, N, MAX_TILES, eq_labels, 7, EDGES)
    check_quality_identities(*want_eq, 7, cycles, 8, mismatch=lane_mismatches(tiles, N, MAX_TILES, eq_labels, 7),
                             pf_wells=_pf(filts), equality=True)
    assert want_eq[0][0] > 100
    need = sc.lane_qual_scratch_bytes(MAX_TILES)
    d_scratch = sc.malloc(need)
    ws_bytes = sc.lane_qual_workspace_bytes(N, MAX_TILES, cycles)
    host = np.zeros(max(need, ws_bytes), dtype=np.uint8)
    d_ws = sc.malloc(ws_bytes)
    tb = _upload(sc, reads, filts)
    idx = TileBatch(sc, len(reads), 8, N)                              # index reads: the first eight cycles, again
    for i, r in enumerate(reads):
        idx.upload_tile(i, [np.ascontiguousarray(r[:, c]) for c in range(8)], filts[i])
    x, y = synth.honeycomb_pixels(ROWS, COLS)
    ld = LaneDups(sc, N, MAX_TILES, cycles)
    try:
        # begin: bad edges, a bad workspace
        for bad in ([], [1, 5], [0, 5, 4], [0, 64], [0, -1], list(range(9))):
            assert _begin(sc, ld, bad, d_ws, ws_bytes) == _lib.ERR_ARG, bad
            with pytest.raises(ValueError):
                ld.qual_begin(bad)
        assert sc._lib.wd_lane_qual_begin(ld._h, 2, None, ctypes.c_void_p(d_ws), ws_bytes) == _lib.ERR_ARG
        for ws, nbytes in ((0, ws_bytes), (d_ws, ws_bytes - 256), (d_ws, 0), (host.ctypes.data, ws_bytes)):
            assert _begin(sc, ld, EDGES, ws, nbytes) == _lib.ERR_ARG
        assert ld.qual_edges is None
        res = _raw(sc, ld, k, d_scratch, need)                         # no quality part
        assert res[0] == _lib.ERR_ARG and _untouched(res)
        assert sc._lib.wd_lane_qual_add(ld._h, 1, (ctypes.c_int * 1)(0), *_tables(tb, [0])) == _lib.ERR_ARG      # add before begin
        # a begin after an add
        ld.add_tables([INDEX[0]], _tables(tb, [0]))
        assert _begin(sc, ld, EDGES, d_ws, ws_bytes) == _lib.ERR_ARG and b"before the first" in sc._lib.wd_last_error(sc._ctx)
        with pytest.raises(ValueError):
            ld.qual_begin(EDGES)
        ld.restart()
        ld.qual_begin(EDGES)
        with pytest.raises(ValueError):                                # a second begin
            ld.qual_begin(EDGES)
        assert _begin(sc, ld, EDGES, d_ws, ws_bytes) == _lib.ERR_ARG
        ld.index_begin(8)
        ld.index_add(idx, INDEX)
        for slots in WAYS["2 + 3"]:
            ld.add_tables([INDEX[s] for s in slots], _tables(tb, slots))
        # qual_add: a bad index, a repeated one, well_stride 4; none of them changes anything
        ld.qual_add(_tables(tb, [0, 1]), [INDEX[0], INDEX[1]])
        for bad in ([INDEX[0]], [MAX_TILES], [-1], [2, 2]):
            with pytest.raises(ValueError):
                ld.qual_add(_tables(tb, [2] * len(bad)), bad)
        with pytest.raises(ValueError):
            ld.qual_add(_tables(tb, [2]), [INDEX[2]], well_stride=4)
        res = _raw(sc, ld, k, d_scratch, need)                         # before any finish
        assert res[0] == _lib.ERR_ARG and _untouched(res)
        with pytest.raises(ValueError):
            ld.qualities(k)
        with pytest.raises(RuntimeError):                              # a near finish refused over budget is no finish
            ld.finish(hamming=k, pair_budget=3)
        res = _raw(sc, ld, k, d_scratch, need)
        assert res[0] == _lib.ERR_ARG and _untouched(res) and b"finish" in sc._lib.wd_last_error(sc._ctx)
        with pytest.raises(ValueError):                                # (and after a refusal nothing more is added)
            ld.qual_add(_tables(tb, [2]), [INDEX[2]])
        # a tile with reads but no qualities: tiles 2, 3, 4 have none
        _finish(ld, k)
        res = _raw(sc, ld, k, d_scratch, need)
        assert res[0] == _lib.ERR_ARG and _untouched(res)
        assert b"tile index %d was added without qualities" % min(INDEX[2:]) in sc._lib.wd_last_error(sc._ctx)
        with pytest.raises(ValueError):
            ld.qualities(k)
        # the lane again, complete
        ld.restart()
        for slots in WAYS["2 + 3"]:
            ld.add_tables([INDEX[s] for s in slots], _tables(tb, slots))
        ld.index_add(idx, INDEX)
        for slots in WAYS["a tile per call"]:
            ld.qual_add(_tables(tb, slots), [INDEX[s] for s in slots])
        _finish(ld, k)
        for bad in ((-1, d_scratch, need), (8, d_scratch, need), (k, 0, need), (k, d_scratch, need - 256), (k, d_scratch, 0),
                    (k, host.ctypes.data, need)):
            res = _raw(sc, ld, *bad)
            assert res[0] == _lib.ERR_ARG and _untouched(res), bad
        for missing in range(5):
            res = _raw(sc, ld, k, d_scratch, need, missing=missing)
            assert res[0] == _lib.ERR_ARG and _untouched(res)
        for d in (-1, 8):
            with pytest.raises(ValueError):
                ld.qualities(d)
        first = _raw(sc, ld, k, d_scratch, need)                       # the caller's scratch, dirty from nothing
        assert first[0] == _lib.OK
        _same(first[1:], want)
        _same(ld.qualities(k), want)                                   # twice the same
        before = ld.index_finish(min_pf=1)
        _same(ld.qualities(k), want)                                   # and after the index finish,
        mism = ld.mismatches(k)
        _same(ld.qualities(k), want)                                   # the mismatch pass
        ld.distances(x, y, 2500)
        _same(ld.qualities(k), want)                                   # and the distance pass
        again = ld.index_finish(min_pf=1)                              # which found their tables as they left them
        assert all((a == b).all() for a, b in zip(before, again)) and all((a == b).all() for a, b in zip(mism, ld.mismatches(k)))
        # another lane in the same workspaces, by equality: Mis = 0
        ld.restart()
        with pytest.raises(ValueError):
            ld.qualities(k)
        for slots in WAYS["descending indices"]:
            ld.qual_add(_tables(tb, slots), [INDEX[s] for s in slots])
            ld.add_tables([INDEX[s] for s in slots], _tables(tb, slots))
        ld.index_add(idx, INDEX)
        _finish(ld, 0)
        got = ld.qualities(7)
        _same(got, want_eq)                                            # (QHist too: restart cleared it)
        check_quality_identities(*got, 7, cycles, 8, mismatch=ld.mismatches(7), pf_wells=_pf(filts), equality=True)
        ld.close()
        assert ld.d_qual == 0
        with pytest.raises(ValueError):
            ld.qualities(k)
        with pytest.raises(ValueError):
            ld.qual_begin(EDGES)
    finally:
        ld.close()
        idx.free()
        tb.free()
        sc.free(d_scratch)
        sc.free(d_ws)


# ---- 7: the CLI -------------------------------------------------------------------------------------
def _main(argv):
    out = io.StringIO()
    with redirect_stdout(out):
        assert cwd.main(argv) == 0
    return out.getvalue()


def test_cli_lane_quality_block(tmp_path):
    """The run directory of test_gpu_lanemismatch.py's CLI test: 2 lanes x 4 tiles; in each lane tile 1103's files are
    tile 1101's but for the last cycle, which is tile 1102's.  The new block closes each lane's output, equals
    write_lane_qualities of the reference, is the same for --tile-batch 1 and the default, and is all the flag adds."""
    rows, cols, levels, k, L = 36, 70, 3, 1, 40
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
    edges, few = cwd.DEFAULT_QUALITY_BINS, [0, 12, 30]
    blocks = {}
    for lane in (1, 2):
        tiles = [(i, [synth.plane_bytes(spec, lane, int(source(t, c)), c) for c in range(L)],
                  synth.filter_bytes(spec, lane, int(t if t != "1103" else "1101"))) for i, t in enumerate(names)]
        labels = {k: lane_near_dups(tiles, n, 4, k)[2], 0: lane_dups(tiles, n, 4)[2]}
        for summary in (False, True):
            for kk, d, e in ((k, k, edges), (k, 0, few), (0, 0, edges)):
                res = lane_qualities(tiles, n, 4, labels[kk], d, e)
                counts = report.LaneQualityCounts.from_rows(*res, names, kk, d, e)
                assert counts.pairs > (1000 if kk else 200) and (d == 0 or counts.mismatches > 1000)
                text = io.StringIO()
                report.write_lane_qualities(str(lane), counts, verbose=not summary, out=text)
                blocks[(summary, lane, kk, d)] = text.getvalue()
    plain = _main(argv)
    runs = [_main(argv + ["--lane-dups-quality", "--tile-batch", "1"]), _main(argv + ["--lane-dups-quality"])]
    assert runs[0] == runs[1]
    b1, b2 = blocks[(False, 1, k, k)], blocks[(False, 2, k, k)]
    assert runs[0].count(b1) == 1 and runs[0].endswith(b2)
    assert runs[0].replace(b1, "", 1)[:-len(b2)] == plain              # minus the new blocks: the output without the flag
    assert runs[0].index("LaneNearDupsSummary: 1") < runs[0].index(b1) < runs[0].index("LaneDupsSummary: 2")
    assert "LaneQualities: 1\tObs root bin 0-1:" in b1 and "truncated from above" in b1 and b1.count("\tBin: ") == 8
    # -S, after every other block of the lane, with bins of its own; the depth follows the mismatches'
    full = _main(argv + ["-S", "--lane-dups-quality", "--lane-dups-quality-bins", "0,12,30", "--lane-dups-index", "0-6",
                         "--lane-dups-mismatches", "--lane-dups-mismatches-max-d", "0", "--lane-dups-distance"])
    b1, b2 = blocks[(True, 1, k, 0)], blocks[(True, 2, k, 0)]
    assert full.count(b1) == 1 and full.endswith(b2) and b1.count("\tBin: ") == 3 and "Obs root bin" not in b1
    assert full.index("LaneDistancesSummary: 1") < full.index(b1) < full.index("LaneDupsSummary: 2")
    assert full.index("LaneMismatchesSummary: 1") < full.index(b1) and full.index("LaneIndexDupsSummary: 1") < full.index(b1)
    # without --lane-dups-hamming: the block is printed and says that every copy is identical
    eq = _main(base + ["-S", "--lane-dups-quality"])
    b1, b2 = blocks[(True, 1, 0, 0)], blocks[(True, 2, 0, 0)]
    assert eq.count(b1) == 1 and eq.endswith(b2) and "every copy is identical" in b1 and "\tMismatches: 0\t" in b1
    assert eq.replace(b1, "", 1)[:-len(b2)] == _main(base + ["-S"])
