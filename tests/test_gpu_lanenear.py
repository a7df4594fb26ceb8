"""Near-duplicate read clusters of a lane on the GPU (LaneDups.finish(hamming=K), include/welldup_lanenear.h)
against the host reference of tests/lanenear_ref.py - equality rows, cluster rows and both label arrays equal,
nothing approximate - however the tiles are fed and whatever hash_bits, and against the identities the header
states: K = 0 is the equality finish, K - 1 refines K, the per-tile clusters refine the lane's."""
import ctypes
import io
import os
import shutil
from contextlib import redirect_stdout

import numpy as np
import pytest

from lanedups_ref import check_identities, lane_dups
from lanenear_ref import (HAND, NEAR_PAIRS, check_near_identities, coarser, hand_made_lane, lane_near_dups, lay_end_to_end,
                          near_row)
from tiledups_ref import INVALID
from tilenear_ref import distinct_reads, long_boundary_check, long_boundary_reads
from well_duplicates_amd import _lib
from well_duplicates_amd import count_well_duplicates as cwd
from well_duplicates_amd import report, synth, workload
from well_duplicates_amd.scanner import LaneDups, Scanner, TileBatch

pytestmark = pytest.mark.gpu

ROWS, COLS, L = 44, 60, 40
N = ROWS * COLS
TILES = [(1, 1101), (1, 1102), (1, 1103), (2, 1101), (2, 1103)]      # (1, 1102) is dead
INDEX = [5, 0, 3, 6, 1]                                               # slot -> tile index in a lane of MAX_TILES
MAX_TILES = 7                                                         # (indices 2 and 4 are never added)
WAYS = {"one call": [[0, 1, 2, 3, 4]], "a tile per call": [[0], [1], [2], [3], [4]], "2 + 3": [[0, 1], [2, 3, 4]],
        "descending indices": [[3], [0], [2], [4], [1]]}


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


def _host_tiles(tb, index, slots=None):
    slots = range(tb.n_tiles) if slots is None else slots
    return [(index[s], [tb.download_plane(s, c) for c in range(tb.L)], tb.download_filter(s)) for s in slots]


def _reference(tb, index, max_tiles, k, method="all_pairs", slots=None):
    """(equality reference, near reference) from the bytes resident on the GPU."""
    tiles = _host_tiles(tb, index, slots)
    return lane_dups(tiles, tb.N, max_tiles), lane_near_dups(tiles, tb.N, max_tiles, k, method=method)


def _tables(tb, slots):
    ptrs = tb.plane_ptrs()
    return Scanner._tables([ptrs[s] for s in slots], [tb.filter_ptr(s) for s in slots], tb.L)


def _lane(sc, tb, index, max_tiles, calls, hash_bits=0):
    ld = LaneDups(sc, tb.N, max_tiles, tb.L, hash_bits=hash_bits)
    try:
        for slots in calls:
            ld.add_tables([index[s] for s in slots], _tables(tb, slots))
    except Exception:
        ld.close()
        raise
    return ld


def _feed(sc, tb, index, max_tiles, calls, k, hash_bits=0, labels=True, pair_budget=0):
    """calls: a list of lists of batch slots, one wd_lane_dups_add each -> LaneDups.finish(hamming=k)"""
    ld = _lane(sc, tb, index, max_tiles, calls, hash_bits)
    if hash_bits == 1 and not pair_budget:      # (two buckets hold every read of the lane: over the default on 10 000 reads)
        pair_budget = 1 << 27
    try:
        return ld.finish(labels=labels, hamming=k, pair_budget=pair_budget)
    finally:
        ld.close()


def _same(got, want_eq, want_near):
    lane, trow, labels, near_lane, near_tiles, near_labels = got
    assert (lane == want_eq[0]).all(), (lane, want_eq[0])
    assert (trow == want_eq[1]).all(), (trow, want_eq[1])
    assert (near_lane == want_near[0]).all(), (near_lane, want_near[0])
    assert (near_tiles == want_near[1]).all(), (near_tiles, want_near[1])
    if labels is not None:
        assert (labels == want_eq[2]).all()
        assert (near_labels == want_near[2]).all()
    check_identities(lane, trow)
    check_near_identities(near_lane, near_tiles)


def _other_base(b):
    """the byte with another base and the same quality bits, never 0"""
    return (b & 0xFC) | (((b & 3) + 1) & 3) | 4


def _plant(reads, rng, src_tile, dst_tile, count, mismatches):
    """copies of `count` reads of src_tile on dst_tile, copy i with 1 + i % mismatches cycles changed (0: none)"""
    n, cycles = reads[0].shape
    a, b = rng.choice(n, count, replace=False), rng.choice(n, count, replace=False)
    reads[dst_tile][b] = reads[src_tile][a]
    for i, w in enumerate(b.tolist()):
        if mismatches:
            for c in rng.choice(cycles, min(cycles, 1 + i % mismatches), replace=False).tolist():
                reads[dst_tile][w, c] = _other_base(reads[dst_tile][w, c])


def _small_lane(k):
    """Five synthetic tiles (copies planted inside every tile, one tile dead) and near copies at 1 .. k + 1
    mismatches planted within tiles and across tiles by hand (chains: a copy of a copy)."""
    spec = synth.SynthSpec(seed=91, n_clusters=N, row=COLS, plant_per_64k=8000, nocall_per_64k=400, dead_tiles=(1102,),
                           plant_far=True, filter_noise=True)
    reads = [np.stack([synth.plane_bytes(spec, ln, t, c) for c in range(L)], axis=1) for ln, t in TILES]
    filts = [synth.filter_bytes(spec, ln, t) for ln, t in TILES]
    rng = np.random.default_rng(17 + k)
    for src, dst, count in ((0, 2, 300), (2, 3, 200), (0, 4, 150), (3, 4, 100), (0, 1, 50), (0, 0, 120), (3, 3, 120)):
        _plant(reads, rng, src, dst, count, k + 1)
    _plant(reads, rng, 2, 4, 80, 0)                                    # and equal reads across tiles
    return reads, filts


@pytest.mark.parametrize("k", [1, 2, 3])
def test_lane_clusters_match_reference_however_the_tiles_are_fed(sc, k):
    reads, filts = _small_lane(k)
    tb = _upload(sc, reads, filts)
    try:
        want_eq, want = _reference(tb, INDEX, MAX_TILES, k)
        near_lane, near_tiles, near_labels = want
        assert near_lane[NEAR_PAIRS] > 200 and near_lane[4] > want_eq[0][4] + 100       # pairs found; clusters across tiles
        assert near_lane[3] > want_eq[0][3] + 200 and near_tiles[:, 3].sum() > want_eq[1][:, 3].sum() + 50
        assert (near_tiles[INDEX[1]] == 0).all() and (near_labels[INDEX[1]] == INVALID).all()      # the dead tile
        assert (near_tiles[[2, 4]] == 0).all() and (near_labels[[2, 4]] == INVALID).all()          # never added
        assert coarser(want_eq[2], near_labels)
        if k > 1:                                                      # the copies at k mismatches are not found at k - 1
            finer = lane_near_dups(_host_tiles(tb, INDEX), N, MAX_TILES, k - 1)
            assert coarser(finer[2], near_labels) and finer[0][NEAR_PAIRS] < near_lane[NEAR_PAIRS] - 100
        for bits in (0, 4, 1):
            for name, calls in WAYS.items():
                if bits and name not in ("one call", "descending indices"):
                    continue
                _same(_feed(sc, tb, INDEX, MAX_TILES, calls, k, hash_bits=bits), want_eq, want)
        got = _feed(sc, tb, INDEX, MAX_TILES, WAYS["2 + 3"], k, labels=False)
        assert got[2] is None and got[5] is None
        _same(got, want_eq, want)
        # K = 0: the rows and labels of the equality finish, NearPairs 0
        got0 = _feed(sc, tb, INDEX, MAX_TILES, WAYS["2 + 3"], 0)
        assert len(got0) == 3
        ld = _lane(sc, tb, INDEX, MAX_TILES, WAYS["one call"])
        try:
            raw = _raw_finish(sc, ld, 0, 0, 0, 0)
        finally:
            ld.close()
        _same(raw, want_eq, (near_row(want_eq[0], 0), want_eq[1], want_eq[2]))
        _same(got0 + (near_row(got0[0], 0), got0[1], got0[2]), want_eq, (near_row(want_eq[0], 0), want_eq[1], want_eq[2]))
    finally:
        tb.free()


def _raw_finish(sc, ld, k, scratch, scratch_bytes, budget, expect=_lib.OK):
    """wd_lane_near_dups_finish itself, with labels -> the six results, or the return code if it is not `expect`'s OK"""
    lane = np.zeros(_lib.LANEDUPS_LANE_COLS, dtype=np.int64)
    trow = np.zeros((ld.max_tiles, _lib.LANEDUPS_TILE_COLS), dtype=np.int64)
    near_lane = np.zeros(_lib.LANENEAR_LANE_COLS, dtype=np.int64)
    near_tiles = np.zeros((ld.max_tiles, _lib.LANEDUPS_TILE_COLS), dtype=np.int64)
    lt, nlt = ld._label_table("d_labels"), ld._label_table("d_near_labels")
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = sc._lib.wd_lane_near_dups_finish(ld._h, k, ctypes.c_void_p(scratch), scratch_bytes, budget, vp(lane), vp(trow), lt,
                                          vp(near_lane), vp(near_tiles), nlt)
    assert rc == expect, (rc, sc._lib.wd_last_error(sc._ctx))
    if rc != _lib.OK:
        return rc
    fetch = lambda p: sc.d2h(p, 4 * ld.N * ld.max_tiles, np.uint32).reshape(ld.max_tiles, ld.N)
    return lane, trow, fetch(ld.d_labels), near_lane, near_tiles, fetch(ld.d_near_labels)


def _upload_hand(sc):
    tiles = hand_made_lane()
    tb = TileBatch(sc, len(tiles), 6, 4)
    for i, (_, planes, filt) in enumerate(tiles):
        tb.upload_tile(i, planes, filt)
    return tb, [t[0] for t in tiles]


@pytest.mark.parametrize("k", [1, 2])
def test_hand_built_lane(sc, k):
    """The chain over three tiles, the N pair, the bridge that fails the filter, the read that joins at K = 2 only:
    the hand-worked rows and labels of lanenear_ref.HAND."""
    tb, index = _upload_hand(sc)
    try:
        want_eq = (np.array(HAND[0]["lane"][:NEAR_PAIRS] + HAND[0]["lane"][NEAR_PAIRS + 1:]), np.array(HAND[0]["tiles"]),
                   np.array(HAND[0]["labels"], dtype=np.uint32))
        want = (np.array(HAND[k]["lane"]), np.array(HAND[k]["tiles"]), np.array(HAND[k]["labels"], dtype=np.uint32))
        for bits in (0, 4, 1):
            for calls in ([[0, 1, 2, 3]], [[3], [2], [1], [0]], [[1, 3], [0, 2]]):
                _same(_feed(sc, tb, index, 5, calls, k, hash_bits=bits), want_eq, want)
    finally:
        tb.free()


def test_equality_outputs_are_those_of_a_plain_finish(sc):
    reads, filts = _small_lane(2)
    tb = _upload(sc, reads, filts)
    try:
        plain = _lane(sc, tb, INDEX, MAX_TILES, WAYS["2 + 3"])
        try:
            want = plain.finish(labels=True)
        finally:
            plain.close()
        for k in (1, 2, 3):
            got = _feed(sc, tb, INDEX, MAX_TILES, WAYS["a tile per call"], k)
            assert all((a == b).all() for a, b in zip(got[:3], want))
    finally:
        tb.free()


@pytest.mark.parametrize("k", [1, 2, 3])
def test_tile_clusters_refine_the_lane_clusters(sc, k):
    """Two wells of one tile that share a wd_tile_near_dups label share a lane cluster label; a lane of one tile at
    index 0 has the labels, Clusters, InClusters, NearPairs and size bins of wd_tile_near_dups."""
    reads, filts = _small_lane(k)
    x, y = synth.honeycomb_pixels(ROWS, COLS)
    sc.targets_from_coords(x, y, None, levels=3)
    tb = _upload(sc, reads, filts)
    try:
        tn_rows, tn_labels = tb.tile_near_dups(k, labels=True)
        got = _feed(sc, tb, INDEX, MAX_TILES, WAYS["2 + 3"], k)
        for s in range(tb.n_tiles):
            assert coarser(tn_labels[s], got[5][INDEX[s]])
            assert got[4][INDEX[s], 2] >= tn_rows[s, 2] and got[4][INDEX[s], 0] == tn_rows[s, 0]
        for s in (0, 2):
            one = _feed(sc, tb, [0] * tb.n_tiles, 1, [[s]], k, hash_bits=4 if s else 0)
            near_lane, near_tiles, near_labels = one[3:]
            assert (near_labels[0] == tn_labels[s]).all()
            assert near_lane[0] == tn_rows[s, 0] and (near_lane[1:3] == tn_rows[s, 1:3]).all()
            assert near_lane[NEAR_PAIRS] == tn_rows[s, 4] and (near_lane[NEAR_PAIRS + 1:] == tn_rows[s, -8:]).all()
            assert near_lane[4] == 0 and near_lane[5] == near_lane[1]
            check_near_identities(near_lane, near_tiles)
    finally:
        tb.free()


# ---- shapes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("cycles", [0, 9, 10, 11, 21, 151])
def test_lane_near_shapes(sc, k, cycles):
    """cycles 0 stands for K + 1, the fewest: segments of one cycle.  Rows of one word, of exactly one, of one and
    a cycle, of three and of sixteen (16-byte pieces), so that segment boundaries fall on and inside words; tiles
    of 1001 wells; then the same tiles less their first well, every plane on an odd address."""
    cycles = cycles or k + 1
    n = 1001
    rng = np.random.default_rng(100 * k + cycles)
    reads = [rng.integers(1, 256, (n, cycles)).astype(np.uint8) for _ in range(3)]
    for r in reads:
        r[rng.random(r.shape) < 0.02] = 0
    for src, dst in ((0, 1), (1, 2), (0, 2), (2, 2)):
        _plant(reads, rng, src, dst, 150, k + 1)
    if cycles > 4:                                                     # near twins that differ in the last cycle, and in the first
        reads[1][:40] = reads[0][:40]
        reads[1][:40, -1] = _other_base(reads[0][:40, -1])
        reads[2][40:80] = reads[0][40:80]
        reads[2][40:80, 0] = _other_base(reads[0][40:80, 0])
    filts = [(rng.random(n) < 0.9).astype(np.uint8) for _ in range(3)]
    tb = _upload(sc, reads, filts)
    try:
        want_eq, want = _reference(tb, [2, 0, 1], 3, k)
        assert want[0][NEAR_PAIRS] > (3 if cycles <= 4 else 100)
        for bits in (0, 1):
            _same(_feed(sc, tb, [2, 0, 1], 3, [[0, 1], [2]], k, hash_bits=bits), want_eq, want)
        tiles = [(i, [tb.download_plane(s, c)[1:] for c in range(cycles)], tb.download_filter(s)[1:])
                 for i, s in enumerate(range(3))]
        want1 = lane_dups(tiles, n - 1, 3), lane_near_dups(tiles, n - 1, 3, k)
        ld = LaneDups(sc, n - 1, 3, cycles)
        try:
            flat = [p + 1 for tile in tb.plane_ptrs() for p in tile]
            ld.add_tables([0, 1, 2], Scanner._tables([flat[i * cycles:(i + 1) * cycles] for i in range(3)],
                                                     [f + 1 for f in tb.filter_ptrs()], cycles))
            _same(ld.finish(labels=True, hamming=k), *want1)
        finally:
            ld.close()
    finally:
        tb.free()


@pytest.mark.parametrize("k", [1, 2, 3])
def test_fewer_cycles_than_segments_is_refused(sc, k):
    n = 64
    rng = np.random.default_rng(k)
    reads = [rng.integers(1, 256, (n, k)).astype(np.uint8)]
    tb = _upload(sc, reads, [np.ones(n, dtype=np.uint8)])
    ld = _lane(sc, tb, [0], 1, [[0]])
    try:
        with pytest.raises(ValueError) as e:
            ld.finish(labels=True, hamming=k)
        assert str(e.value).startswith(_lib.strerror(_lib.ERR_ARG)) and "cycles" in str(e.value)
        got = ld.finish(labels=True)                                   # nothing changed: the classes are still to be had
        want = lane_dups(_host_tiles(tb, [0]), n, 1)
        assert all((a == b).all() for a, b in zip(got, want))
    finally:
        ld.close()
        tb.free()


# ---- degenerate lanes ---------------------------------------------------------------------------
def test_every_read_equal_is_one_cluster(sc):
    spec = synth.SynthSpec(seed=3, n_clusters=N, row=COLS)
    filts = [synth.filter_bytes(spec, 1, 1101 + i) for i in range(3)]
    reads = [np.tile(np.array([0x42 + (c % 4) for c in range(L)], dtype=np.uint8), (N, 1)) for _ in range(3)]
    tb = _upload(sc, reads, filts)
    try:
        pf = [(f & 1).astype(bool) for f in filts]
        total = int(sum(p.sum() for p in pf))
        first = int(np.flatnonzero(pf[0])[0])
        for k, bits in ((1, 0), (3, 1)):
            got = _feed(sc, tb, [0, 1, 2], 3, [[0, 1, 2]], k, hash_bits=bits)
            assert got[3].tolist() == [total, 1, total, total - 1, 1, 3, 0, 0, 0, 0, 0, 0, 0, 0, 1]
            assert got[0].tolist() == got[3].tolist()[:NEAR_PAIRS] + got[3].tolist()[NEAR_PAIRS + 1:]
            assert (got[4] == got[1]).all() and (got[5] == got[2]).all()
            for i in range(3):
                assert (got[5][i][pf[i]] == first).all() and (got[5][i][~pf[i]] == INVALID).all()
    finally:
        tb.free()


def test_a_lane_with_no_pf_well_and_a_lane_of_one_tile_in_seven(sc):
    reads, filts = _small_lane(1)
    tb = _upload(sc, reads, [np.zeros(N, dtype=np.uint8) for _ in filts])
    try:
        got = _feed(sc, tb, INDEX, MAX_TILES, WAYS["2 + 3"], 2)
        assert not got[0].any() and not got[1].any() and not got[3].any() and not got[4].any()
        assert (got[2] == INVALID).all() and (got[5] == INVALID).all()
    finally:
        tb.free()
    tb = _upload(sc, reads, filts)
    try:
        want_eq, want = _reference(tb, INDEX, MAX_TILES, 2, slots=[3])
        assert want[0][NEAR_PAIRS] > 50 and want[0][4] == 0
        _same(_feed(sc, tb, INDEX, MAX_TILES, [[3]], 2), want_eq, want)
        empty = LaneDups(sc, N, MAX_TILES, L)                          # and one that nothing was added to
        try:
            got = empty.finish(labels=True, hamming=1)
            assert not got[3].any() and not got[4].any() and (got[5] == INVALID).all()
        finally:
            empty.close()
    finally:
        tb.free()


# ---- the heavy bucket and the refusal -----------------------------------------------------------
def test_heavy_bucket_refusal_and_retry(sc):
    """Three tiles of 200 distinct reads that share their first ten cycles of twenty: at K = 1 segment 0 has one
    bucket of all of them (more than 32: the long path), some within one mismatch of each other."""
    n, cycles, k = 200, 20, 1
    rng = np.random.default_rng(5)
    head = rng.integers(1, 256, cycles // 2).astype(np.uint8)
    reads = []
    for t in range(3):
        r = rng.integers(1, 256, (n, cycles)).astype(np.uint8)
        r[:, :cycles // 2] = head
        reads.append(r)
    for src, dst in ((0, 1), (1, 2), (0, 2), (1, 1)):
        _plant(reads, rng, src, dst, 30, 2)
    for r in reads:                                                    # (a plant may have changed a cycle of the head)
        r[:, :cycles // 2] = head
    filts = [np.ones(n, dtype=np.uint8) for _ in range(3)]
    filts[1][::17] = 0
    tb = _upload(sc, reads, filts)
    try:
        index = [4, 0, 2]
        want_eq, want = _reference(tb, index, 5, k)
        codes, pf = lay_end_to_end(_host_tiles(tb, index), n, 5)
        r = distinct_reads(codes, pf)[1].size
        bound = r * (r - 1) // 2
        assert r > 500 and want[0][NEAR_PAIRS] > 40
        ld = _lane(sc, tb, index, 5, [[0, 1], [2]])
        try:
            for budget in (1000, bound - 1):
                with pytest.raises(RuntimeError) as e:
                    ld.finish(labels=True, hamming=k, pair_budget=budget)
                msg = str(e.value)
                assert msg.startswith(_lib.strerror(_lib.ERR_UNSUPPORTED))
                assert "segment 0 (cycles 0..9)" in msg and "%d candidate pairs" % bound in msg
                assert "pair budget of %d" % budget in msg
                assert all((a == b).all() for a, b in zip(ld.refused, want_eq))      # delivered, and valid
            with pytest.raises(ValueError):                            # the table is resolved: nothing can be added
                ld.add_tables([1], _tables(tb, [0]))
            _same(ld.finish(labels=True, hamming=k, pair_budget=bound), want_eq, want)
            for again in (lambda: ld.finish(labels=True, hamming=k), lambda: ld.finish()):
                with pytest.raises(ValueError) as e:                   # after a success any finish is refused
                    again()
                assert str(e.value).startswith(_lib.strerror(_lib.ERR_ARG))
        finally:
            ld.close()
        ld = _lane(sc, tb, index, 5, [[2], [1], [0]], hash_bits=4)
        try:
            with pytest.raises(RuntimeError):
                ld.finish(hamming=2, pair_budget=10)
            _same(ld.finish(labels=True, hamming=k), want_eq, want)    # another k, the default budget
        finally:
            ld.close()
        ld = _lane(sc, tb, index, 5, [[0, 1, 2]])
        try:
            with pytest.raises(RuntimeError):
                ld.finish(labels=True, hamming=k, pair_budget=1000)
            got = ld.finish(labels=True)                               # or the plain finish
            assert all((a == b).all() for a, b in zip(got, want_eq))
        finally:
            ld.close()
    finally:
        tb.free()


def test_lane_clusters_at_the_long_slot_boundary(sc):
    """The reads of test_gpu_tilenear's boundary test dealt alternately onto two tiles of a lane of three indices,
    a tile per add call: slots of 31 and 32 distinct reads (the chain walk) and of 33 and 34 (the rank path), every
    one of them on both tiles.  All six outputs of the all-pairs reference; NearPairs and the size bins of
    tile_near_dups on the undealt reads."""
    reads, groups = long_boundary_reads()
    n, index = reads.shape[0] // 2, [2, 0]                             # (index 1 is never added)
    assert all(0 < int((g % 2).sum()) < g.size for g in groups)
    x, y = synth.honeycomb_pixels(16, 16)
    sc.targets_from_coords(x, y, None, levels=3)
    whole = _upload(sc, [reads], [np.ones(2 * n, dtype=np.uint8)])
    tb = _upload(sc, [reads[0::2], reads[1::2]], [np.ones(n, dtype=np.uint8)] * 2)
    try:
        want_eq, want = _reference(tb, index, 3, 1)
        well = np.arange(2 * n)
        long_boundary_check(want[2][np.array(index)[well % 2], well // 2], groups)
        got = _feed(sc, tb, index, 3, [[0], [1]], 1)
        _same(got, want_eq, want)
        tn_rows, _ = whole.tile_near_dups(1)
        assert got[3][NEAR_PAIRS] == tn_rows[0, 4] and (got[3][NEAR_PAIRS + 1:] == tn_rows[0, -8:]).all()
    finally:
        whole.free()
        tb.free()


# ---- scale --------------------------------------------------------------------------------------
def _patch_planes(sc, tb, src_slot, src, dst_slot, dst, cut):
    """reads of wells src of one resident tile copied to wells dst of another, copy i with cycles cut[i] changed"""
    for c in range(tb.L):
        a = tb.download_plane(src_slot, c)
        b = a if dst_slot == src_slot else tb.download_plane(dst_slot, c)
        b[dst] = a[src]
        for i, cs in enumerate(cut):
            if c in cs:
                b[dst[i]] = _other_base(b[dst[i]])
        sc.h2d(tb.plane_ptr(dst_slot, c), b)
    for slot, wells in ((src_slot, src), (dst_slot, dst)):
        f = tb.download_filter(slot)
        f[wells] |= 1
        sc.h2d(tb.filter_ptr(slot), f)


def test_lane_near_k2_on_four_tiles_of_200000_wells(sc):
    """4 x (400 x 500) wells, 24 cycles (segments of eight: buckets of several reads each), K = 2, 2 000 near
    copies planted on the next tile, against the pair-deletion reference."""
    rows_, cols_, cycles = 400, 500, 24
    n = rows_ * cols_
    spec = synth.SynthSpec(seed=12, n_clusters=n, row=cols_, plant_per_64k=1311, nocall_per_64k=328)
    tb = TileBatch(sc, 4, cycles, n)
    tb.fill_synthetic(spec, [(1, 1101 + i) for i in range(4)], list(range(cycles)))
    try:
        rng = np.random.default_rng(13)
        for s in range(4):
            src = rng.choice(n, 500, replace=False)
            dst = (src + n // 2 + rng.integers(0, 1000, 500)) % n
            cut = [rng.choice(cycles, 1 + i % 2, replace=False).tolist() for i in range(500)]
            _patch_planes(sc, tb, s, src, (s + 1) % 4, dst, cut)
        want_eq, want = _reference(tb, [3, 1, 0, 2], 4, 2, method="deletion")
        assert want[0][NEAR_PAIRS] >= 1900 and want[0][4] >= 1900
        _same(_feed(sc, tb, [3, 1, 0, 2], 4, [[0, 1], [2, 3]], 2), want_eq, want)
    finally:
        tb.free()


SAMPLE = 2000       # planted pairs whose labels are compared one by one on the full tiles (fixed by the seed below)


def test_lane_near_full_hiseq4000_tiles(sc):
    """Three tiles of 4 309 253 wells, 50 cycles, 2 % planted inside the tiles; 3 000 near copies (one mismatch) of
    reads of each tile planted on the NEXT tile, K = 1.  Checked by the identities, CrossTileClusters and NearPairs
    at least the planted count, the equality outputs against a plain finish, and - exactly - on SAMPLE of the 9 000
    planted pairs (drawn with seed 21), each of which must share a label."""
    n, cycles, per_tile = workload.HISEQ4000_ROWS * workload.HISEQ4000_COLS, 50, 3000
    assert n == 4309253
    spec = synth.SynthSpec(seed=6, n_clusters=n, row=workload.HISEQ4000_COLS, plant_per_64k=1311, nocall_per_64k=328)
    tb = TileBatch(sc, 3, cycles, n)
    tb.fill_synthetic(spec, [(1, 1101), (1, 1102), (1, 1103)], list(range(cycles)))
    try:
        rng = np.random.default_rng(8)
        planted = []
        for s in range(3):
            # (sources and targets apart: a target is never a later source, so no planted pair is overwritten)
            src = rng.choice(n // 2, per_tile, replace=False)
            dst = n // 2 + rng.choice(n // 2, per_tile, replace=False)
            cut = [[int(rng.integers(0, cycles))] for _ in range(per_tile)]
            _patch_planes(sc, tb, s, src, (s + 1) % 3, dst, cut)
            planted += [(s * n + a, ((s + 1) % 3) * n + b) for a, b in zip(src.tolist(), dst.tolist())]
        plain = _lane(sc, tb, [0, 1, 2], 3, [[0, 1, 2]])
        try:
            want_eq = plain.finish(labels=True)
        finally:
            plain.close()
        got = _feed(sc, tb, [0, 1, 2], 3, [[0, 1], [2]], 1)
        lane, trow, labels, near_lane, near_tiles, near_labels = got
        assert all((a == b).all() for a, b in zip(got[:3], want_eq))
        check_identities(lane, trow)
        check_near_identities(near_lane, near_tiles)
        assert coarser(labels, near_labels)
        total = 3 * per_tile
        assert near_lane[4] >= total and near_lane[NEAR_PAIRS] >= total and near_lane[3] > lane[3]
        flat, eq_flat = near_labels.reshape(-1), labels.reshape(-1)
        pick = np.random.default_rng(21).choice(total, SAMPLE, replace=False)
        for i in pick.tolist():
            a, b = planted[i]
            assert flat[a] == flat[b] != INVALID, (i, a, b)
            assert flat[a] <= min(a, b) and eq_flat[a] != eq_flat[b]
    finally:
        tb.free()


# ---- bad arguments ------------------------------------------------------------------------------
def test_bad_arguments_leave_the_lane_as_it_was(sc):
    reads, filts = _small_lane(1)
    tb = _upload(sc, reads, filts)
    ld = _lane(sc, tb, INDEX, MAX_TILES, WAYS["2 + 3"])
    need = sc.lane_near_scratch_bytes(N, MAX_TILES, L, 2)
    d_scratch = sc.malloc(need)
    host = np.zeros(need, dtype=np.uint8)
    try:
        want_eq = lane_dups(_host_tiles(tb, INDEX), N, MAX_TILES)
        bad = [(-1, d_scratch, need, 0), (4, d_scratch, need, 0), (2, d_scratch, need, -1), (2, 0, need, 0),
               (2, d_scratch, need - 256, 0), (2, d_scratch, 0, 0), (2, host.ctypes.data, need, 0)]
        for k, ptr, nbytes, budget in bad:
            assert _raw_finish(sc, ld, k, ptr, nbytes, budget, expect=_lib.ERR_ARG) == _lib.ERR_ARG
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        rows = [np.zeros(64, dtype=np.int64) for _ in range(4)]
        for missing in range(4):                                       # a null row
            args = [None if i == missing else vp(r) for i, r in enumerate(rows)]
            assert sc._lib.wd_lane_near_dups_finish(ld._h, 1, ctypes.c_void_p(d_scratch), need, 0, args[0], args[1], None,
                                                    args[2], args[3], None) == _lib.ERR_ARG
        lt = (ctypes.c_void_p * MAX_TILES)(*[host.ctypes.data] * MAX_TILES)      # labels in host memory
        big = [np.zeros(MAX_TILES * 8, dtype=np.int64) for _ in range(4)]
        for which in (0, 1):
            assert sc._lib.wd_lane_near_dups_finish(ld._h, 1, ctypes.c_void_p(d_scratch), need, 0, vp(big[0]), vp(big[1]),
                                                    lt if which == 0 else None, vp(big[2]), vp(big[3]),
                                                    lt if which == 1 else None) == _lib.ERR_ARG
        with pytest.raises(ValueError):
            ld.finish(hamming=4)
        with pytest.raises(ValueError):
            ld.finish(hamming=0, pair_budget=5)
        # none of these changed anything: a plain finish gives the reference
        got = ld.finish(labels=True)
        assert all((a == b).all() for a, b in zip(got, want_eq))
        assert _raw_finish(sc, ld, 1, d_scratch, need, 0, expect=_lib.ERR_ARG) == _lib.ERR_ARG      # after a finish
    finally:
        sc.free(d_scratch)
        ld.close()
        tb.free()


# ---- the CLI ------------------------------------------------------------------------------------
def _main(argv):
    out = io.StringIO()
    with redirect_stdout(out):
        assert cwd.main(argv) == 0
    return out.getvalue()


def test_cli_lane_near_block_and_tsv(tmp_path):
    """2 lanes x 4 tiles; in each lane tile 1103's files are tile 1101's but for the last cycle, which is tile
    1102's: near copies across tiles.  The near block is the same for --tile-batch 1, 2 and the default, equals the
    reference, and is all the flag adds to the output."""
    rows, cols, levels, k = 36, 70, 3, 1
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
    argv = ["-s", "hiseq_x", "-r", run_dir, "-t", "1101,1102,1103,1104", "-i", "1,2", "-l", str(levels),
            "--cycles", "0-%d" % L, "-q", "--all-wells"]
    blocks, want_tsv = {}, ["lane\ttile\twell\tclass_tile\tclass_well\tcluster_tile\tcluster_well"]
    for summary in (False, True):
        for lane in (1, 2):
            tiles = [(i, [synth.plane_bytes(spec, lane, int(source(t, c)), c) for c in range(L)],
                      synth.filter_bytes(spec, lane, int(t if t != "1103" else "1101"))) for i, t in enumerate(names)]
            eq_lane, eq_tiles, eq_labels = lane_dups(tiles, n, 4)
            near_lane, near_tiles, near_labels = lane_near_dups(tiles, n, 4, k)
            equal = report.LaneDupCounts.from_rows(eq_lane, eq_tiles, names)
            counts = report.LaneNearCounts.from_rows(near_lane, near_tiles, names)
            # (three wells in four of 1101 have a near twin on 1103, the fourth an equal one)
            assert counts.cross_tile_classes > equal.cross_tile_classes + 1000 and counts.near_pairs > 1000
            text = io.StringIO()
            report.write_lane_near_dups(str(lane), k, counts, verbose=not summary, out=text, equal=equal)
            blocks[(summary, lane)] = text.getvalue()
            if not summary:
                want_tsv += ["%d\t%s\t%d\t%s\t%d\t%s\t%d" % (lane, names[a], b, names[c], d, names[e], f)
                             for a, b, c, d, e, f in zip(*(v.tolist() for v in cwd.lane_cluster_members(eq_labels, near_labels)))]
    for summary in (False, True):
        flags = ["-S"] if summary else []
        near = ["--lane-dups", "--lane-dups-hamming", str(k)]
        plain = _main(argv + flags + ["--lane-dups"])
        tsv = str(tmp_path / "lane.tsv")
        runs = [_main(argv + flags + near + ["--tile-batch", "1"]),
                _main(argv + flags + near + ["--tile-batch", "2", "--lane-dups-out", tsv, "--lane-dups-pair-budget", "100000000"]),
                _main(argv + flags + near)]
        assert runs[0] == runs[1] == runs[2]
        assert open(tsv).read().splitlines() == want_tsv
        b1, b2 = blocks[(summary, 1)], blocks[(summary, 2)]
        assert runs[0].count(b1) == 1 and runs[0].endswith(b2)
        assert runs[0].replace(b1, "", 1)[:-len(b2)] == plain          # minus the new blocks: the output without the flag
        assert runs[0].index("LaneDupsSummary: 1") < runs[0].index(b1) < runs[0].index("LaneDupsSummary: 2")
    assert "Lane duplication at Hamming <= 1 (Redundant/PF wells): " in b2 and "\tby equality: " in b2
    with pytest.raises(RuntimeError) as e:                             # a refused lane ends the run with the library's message
        _main(argv + near + ["--lane-dups-pair-budget", "3"])
    assert "candidate pairs exceed the pair budget of 3" in str(e.value)
