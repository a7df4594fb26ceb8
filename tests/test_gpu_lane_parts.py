"""The feeding side of a lane's accumulator (LaneDups) and its three side parts - the qualities, the index keys, the UMI
keys - driven from one table: every refusal the four adds and the three begins share, against the literal message; the
check that a part was fed the lane's tiles, through each of the five passes that make it; the keys of the two key parts
on the same planes against laneindex_ref.key_of; restart() and close() with all three parts present.

The strings of EXPECT and EXPECT_MISMATCH are recordings: what the library printed before the four adds, the two key
begins and the five tile checks were given one body each.  They are whole strings on purpose - nothing here composes a
message from a part's name - so that they hold the messages byte for byte."""
import ctypes
from collections import namedtuple

import numpy as np
import pytest

from laneindex_ref import key_of
from well_duplicates_amd.scanner import LaneDups, Scanner, TileBatch

pytestmark = pytest.mark.gpu

N, T, L, K = 37, 3, 6, 4               # wells of a tile, tiles of the lane, cycles of a read, cycles of a key
EDGES = [0, 20, 30]

# name: begin with the usual argument, add, the pass that reads the part, and for the raw begin the entry, its size
# function and how the argument is handed over; keyed: an index or UMI part
Part = namedtuple("Part", "begin add reads entry ws_bytes cargs arg keyed")
PARTS = {
    "dups": Part(None, lambda ld, tables, idx, stride=1: ld.add_tables(idx, tables, well_stride=stride),
                 lambda ld: None, None, None, None, None, False),
    "qual": Part(lambda ld: ld.qual_begin(EDGES), lambda ld, *a: ld.qual_add(*a), lambda ld: ld.qualities(2),
                 "wd_lane_qual_begin", lambda sc, arg: sc.lane_qual_workspace_bytes(N, T, L),
                 lambda arg: (len(arg), (ctypes.c_int * len(arg))(*arg)), EDGES, False),
    "index": Part(lambda ld: ld.index_begin(K), lambda ld, *a: ld.index_add(*a), lambda ld: ld.index_finish(),
                  "wd_lane_index_begin", lambda sc, arg: sc.lane_index_workspace_bytes(N, T, arg), lambda arg: (arg,), K, True),
    "umi": Part(lambda ld: ld.umi_begin(K), lambda ld, *a: ld.umi_add(*a), lambda ld: ld.umi(),
                "wd_lane_umi_begin", lambda sc, arg: sc.lane_umi_workspace_bytes(N, T, arg), lambda arg: (arg,), K, True),
}

EXPECT = {
    "dups": {
        "workspace one byte short": "invalid argument: workspace smaller than wd_lane_dups_workspace",
        "well_stride 4": "invalid argument: lane duplicates read a plane per cycle (well_stride 1)",
        "more tiles than max_tiles": "invalid argument: lane duplicates: more tiles than the lane has room for",
        "tile index -1": "invalid argument: lane duplicates: tile index -1 out of range",
        "tile index max_tiles": "invalid argument: lane duplicates: tile index 3 out of range",
        "twice within a call": "invalid argument: lane duplicates: tile index 1 used twice",
        "twice across calls": "invalid argument: lane duplicates: tile index 0 used twice",
        "add after finish": "invalid argument: lane duplicates: add after finish",
    },
    "qual": {
        "add before begin": "invalid argument: lane qualities: add before wd_lane_qual_begin",
        "workspace one byte short": "invalid argument: workspace smaller than wd_lane_qual_workspace",
        "begin twice": "invalid argument: lane qualities: begin is called once",
        "well_stride 4": "invalid argument: lane qualities read a plane per cycle (well_stride 1)",
        "more tiles than max_tiles": "invalid argument: lane qualities: more tiles than the lane has room for",
        "tile index -1": "invalid argument: lane qualities: tile index -1 out of range",
        "tile index max_tiles": "invalid argument: lane qualities: tile index 3 out of range",
        "twice within a call": "invalid argument: lane qualities: tile index 1 used twice",
        "twice across calls": "invalid argument: lane qualities: tile index 0 used twice",
        "add after finish": "invalid argument: lane qualities: add after finish",
        "begin after finish": "invalid argument: lane qualities: begin after finish",
    },
    "index": {
        "add before begin": "invalid argument: lane index: add before wd_lane_index_begin",
        "0 cycles": "invalid argument: lane index: 1..20 index cycles, not 0",
        "21 cycles": "invalid argument: lane index: 1..20 index cycles, not 21",
        "workspace one byte short": "invalid argument: workspace smaller than wd_lane_index_workspace",
        "begin twice": "invalid argument: lane index: begin is called once",
        "well_stride 4": "invalid argument: lane index reads a plane per cycle (well_stride 1)",
        "more tiles than max_tiles": "invalid argument: lane index: more tiles than the lane has room for",
        "tile index -1": "invalid argument: lane index: tile index -1 out of range",
        "tile index max_tiles": "invalid argument: lane index: tile index 3 out of range",
        "twice within a call": "invalid argument: lane index: tile index 1 used twice",
        "null plane pointer": "invalid argument: null plane pointer",
        "twice across calls": "invalid argument: lane index: tile index 0 used twice",
        "add after finish": "invalid argument: lane index: add after finish",
        "begin after finish": "invalid argument: lane index: begin after finish",
    },
    "umi": {
        "add before begin": "invalid argument: lane umi: add before wd_lane_umi_begin",
        "0 cycles": "invalid argument: lane umi: 1..20 UMI cycles, not 0",
        "21 cycles": "invalid argument: lane umi: 1..20 UMI cycles, not 21",
        "workspace one byte short": "invalid argument: workspace smaller than wd_lane_umi_workspace",
        "begin twice": "invalid argument: lane umi: begin is called once",
        "well_stride 4": "invalid argument: lane umi reads a plane per cycle (well_stride 1)",
        "more tiles than max_tiles": "invalid argument: lane umi: more tiles than the lane has room for",
        "tile index -1": "invalid argument: lane umi: tile index -1 out of range",
        "tile index max_tiles": "invalid argument: lane umi: tile index 3 out of range",
        "twice within a call": "invalid argument: lane umi: tile index 1 used twice",
        "null plane pointer": "invalid argument: null plane pointer",
        "twice across calls": "invalid argument: lane umi: tile index 0 used twice",
        "add after finish": "invalid argument: lane umi: add after finish",
        "begin after finish": "invalid argument: lane umi: begin after finish",
    },
}
EXPECT_MISMATCH = {
    "added without": {
        "index_finish": "invalid argument: lane index: tile index 1 was added without index planes",
        "hops": "invalid argument: lane index: tile index 1 was added without index planes",
        "umi": "invalid argument: lane umi: tile index 1 was added without UMI planes",
        "qualities": "invalid argument: lane qualities: tile index 1 was added without qualities",
        "keep": "invalid argument: lane keep: tile index 1 was added without qualities",
    },
    "never added": {
        "index_finish": "invalid argument: lane index: tile index 1 got index planes but was never added",
        "hops": "invalid argument: lane index: tile index 1 got index planes but was never added",
        "umi": "invalid argument: lane umi: tile index 1 got UMI planes but was never added",
        "qualities": "invalid argument: lane qualities: tile index 1 got qualities but was never added",
        "keep": "invalid argument: lane keep: tile index 1 got qualities but was never added",
    },
}


@pytest.fixture(scope="module")
def sc():
    s = Scanner(0)
    yield s
    s.close()


def _plane_bytes(rng, codes):
    """codes 0..4 -> plane bytes: the base under a random quality that is not 0, byte 0 for N"""
    q = rng.integers(1, 64, codes.shape).astype(np.uint8)
    return np.where(codes == 4, 0, codes | (q << 2)).astype(np.uint8)


def _batch(sc, rng, cycles, n=N, tiles=T):
    tb = TileBatch(sc, tiles, cycles, n)
    for i in range(tiles):
        codes = rng.integers(0, 5, (cycles, n)).astype(np.uint8)
        tb.upload_tile(i, list(_plane_bytes(rng, codes)), (rng.random(n) < 0.8).astype(np.uint8))
    return tb


@pytest.fixture(scope="module")
def batches(sc):
    """(the reads of T tiles, the planes of their K key cycles)"""
    rng = np.random.default_rng(58)
    reads, keys = _batch(sc, rng, L), _batch(sc, rng, K)
    yield reads, keys
    reads.free()
    keys.free()


def _tables(tb, slots, null_at=None):
    ptrs = tb.plane_ptrs()
    pt, ft = Scanner._tables([ptrs[s] for s in slots], [tb.filter_ptr(s) for s in slots], tb.L)
    if null_at is not None:
        pt[null_at] = None
    return pt, ft


def _raw_begin(ld, part, arg, short=0):
    """The part's begin entry itself, on a workspace of the test's: sized for `arg` where a size exists for it, `short`
    bytes smaller.  -> raises what the return code means."""
    sc = ld.sc
    nbytes = part.ws_bytes(sc, arg if not part.keyed or 1 <= arg <= 20 else part.arg)
    d_ws = sc.malloc(max(1, nbytes))
    try:
        sc._ck(getattr(sc._lib, part.entry)(ld._h, *part.cargs(arg), ctypes.c_void_p(d_ws), nbytes - short))
    finally:
        sc.free(d_ws)


def refusals(sc, name, batches):
    """Every refusal of part `name`, in one lane -> {refusal: the message}.  None of them launches anything; after each
    the part stands as before, which the adds and the begin that follow show by succeeding."""
    part, reads = PARTS[name], batches[0]
    tb = batches[1] if part.keyed else reads
    out = {}

    def refused(key, call):
        with pytest.raises(ValueError) as e:
            call()
        out[key] = str(e.value)

    ld = LaneDups(sc, N, T, L)
    try:
        if part.begin:
            refused("add before begin", lambda: part.add(ld, _tables(tb, [0]), [0]))
            if part.keyed:
                refused("0 cycles", lambda: _raw_begin(ld, part, 0))
                refused("21 cycles", lambda: _raw_begin(ld, part, 21))
            refused("workspace one byte short", lambda: _raw_begin(ld, part, part.arg, short=1))
            part.begin(ld)
            refused("begin twice", lambda: _raw_begin(ld, part, part.arg))
        refused("well_stride 4", lambda: part.add(ld, _tables(tb, [0, 1]), [0, 1], 4))
        refused("more tiles than max_tiles", lambda: part.add(ld, _tables(tb, [0, 1, 2, 0]), [0, 1, 2, 0]))
        refused("tile index -1", lambda: part.add(ld, _tables(tb, [0, 1]), [1, -1]))
        refused("tile index max_tiles", lambda: part.add(ld, _tables(tb, [0, 1]), [1, T]))
        refused("twice within a call", lambda: part.add(ld, _tables(tb, [0, 1]), [1, 1]))
        if part.keyed:
            refused("null plane pointer", lambda: part.add(ld, _tables(tb, [0, 1], null_at=K + 1), [0, 1]))
        part.add(ld, _tables(tb, [0, 1]), [0, 1])                      # no refusal above has marked tile 0 or 1
        refused("twice across calls", lambda: part.add(ld, _tables(tb, [2, 0]), [2, 0]))
        part.add(ld, _tables(tb, [2]), [2])                            # nor has that one marked tile 2
        if part.begin:
            ld.add(reads, [0, 1, 2])
        ld.finish()
        refused("add after finish", lambda: part.add(ld, _tables(tb, [0]), [0]))
        if part.begin:
            refused("begin after finish", lambda: _raw_begin(ld, part, part.arg))
        part.reads(ld)                                                 # the part's tiles are still the lane's
    finally:
        ld.close()
    if name == "dups":                                                 # the accumulator's own begin
        nbytes, h = sc.lane_dups_workspace_bytes(N, T, L), ctypes.c_void_p()
        d_ws = sc.malloc(nbytes)
        try:
            refused("workspace one byte short", lambda: sc._ck(sc._lib.wd_lane_dups_begin(
                sc._ctx, N, T, L, ctypes.c_void_p(d_ws), nbytes - 1, 0, ctypes.byref(h))))
        finally:
            sc.free(d_ws)
    return out


def mismatches(sc, batches):
    """A lane of which tile 1 was added without the parts' planes, and one of which tile 1 got them but was never
    added -> {case: {pass: the message}} through the five passes that hold a part's tiles against the lane's."""
    reads, keys = batches
    out = {}
    for case, lane_tiles, part_tiles in (("added without", [0, 1], [0]), ("never added", [0], [0, 1])):
        ld = LaneDups(sc, N, T, L)
        try:
            for name in ("qual", "index", "umi"):
                PARTS[name].begin(ld)
                PARTS[name].add(ld, _tables(keys if PARTS[name].keyed else reads, part_tiles), part_tiles)
            ld.add_tables(lane_tiles, _tables(reads, lane_tiles))
            ld.finish()
            out[case] = {}
            for caller, call in (("index_finish", ld.index_finish), ("hops", lambda: ld.hops(2, 0, [])), ("umi", ld.umi),
                                 ("qualities", lambda: ld.qualities(2)), ("keep", ld.keep)):
                with pytest.raises(ValueError) as e:
                    call()
                out[case][caller] = str(e.value)
        finally:
            ld.close()
    return out


@pytest.mark.parametrize("name", list(PARTS))
def test_every_shared_refusal_prints_its_recorded_message_and_changes_nothing(sc, batches, name):
    got = refusals(sc, name, batches)
    assert sorted(got) == sorted(EXPECT[name])
    for key in got:
        assert got[key] == EXPECT[name][key], (name, key)


def test_a_part_fed_other_tiles_than_the_lane_is_refused_by_each_of_the_five_passes(sc, batches):
    assert mismatches(sc, batches) == EXPECT_MISMATCH


# ---- the two key parts pack the same planes into the same keys ------------------------------------------
def _key_lane(sc, n, cycles, offset):
    """T tiles of `cycles` planes, every plane `offset` bytes off a 256-byte boundary, fed to an index part and a UMI part
    of one lane through pointer tables, tiles (2, 0) and then (1) -> (index_keys, umi_keys, the keys key_of gives)"""
    rng = np.random.default_rng(1000 * n + 10 * cycles + offset)
    codes = rng.integers(0, 5, (T, cycles, n)).astype(np.uint8)
    data = _plane_bytes(rng, codes)
    stride = (n + 255) // 256 * 256
    d_planes = sc.malloc(T * cycles * stride + 1)
    ld = LaneDups(sc, n, T, L)
    try:
        at = lambda t, c: d_planes + offset + (t * cycles + c) * stride      # (+ n <= T * cycles * stride + offset)
        for t in range(T):
            for c in range(cycles):
                sc.h2d(at(t, c), np.ascontiguousarray(data[t, c]))
        ld.index_begin(cycles)
        ld.umi_begin(cycles)
        for tiles in ([2, 0], [1]):
            pt = (ctypes.c_void_p * (len(tiles) * cycles))(*[at(t, c) for t in tiles for c in range(cycles)])
            ld.index_add((pt, None), tiles)
            ld.umi_add((pt, None), tiles)
        want = np.array([key_of("".join("ACGTN"[b] for b in codes[t, :, w])) for t in range(T) for w in range(n)], dtype=np.uint64)
        return ld.index_keys(), ld.umi_keys(), want
    finally:
        ld.close()
        sc.free(d_planes)


@pytest.mark.parametrize("n,cycles,offset", [(n, c, 0) for n in (5, 4, 1024 + 3) for c in (1, 10, 11, 20)] +
                         [(5, 20, 1), (1024 + 3, 11, 1)])
def test_the_index_part_and_the_umi_part_pack_the_same_planes_into_the_same_keys(sc, n, cycles, offset):
    """n = 5: the tail of the kernel that packs four wells a lane, 4: no tail, 1027: more than one workgroup and a tail;
    one and two key words, each partly and wholly filled; offset 1: no plane is 4-byte aligned, so the kernel that packs
    a well a lane runs."""
    index, umi, want = _key_lane(sc, n, cycles, offset)
    assert index.shape == umi.shape == want.shape
    assert (index == want).all(), np.flatnonzero(index != want)[:8]
    assert (umi == want).all(), np.flatnonzero(umi != want)[:8]


# ---- restart() and close() with all three parts -----------------------------------------------------------
def _lane_results(ld, reads, keys, order):
    for name in ("qual", "index", "umi"):
        for tiles in order:
            PARTS[name].add(ld, _tables(keys if PARTS[name].keyed else reads, tiles), tiles)
    for tiles in order:
        ld.add_tables(tiles, _tables(reads, tiles))
    fin = ld.finish()[:2]
    return [fin, ld.index_finish(), ld.umi(), ld.qualities(2), ld.keep(), ld.index_keys(), ld.umi_keys()]


def _flat(results):
    return [np.asarray(a) for r in results for a in (r if isinstance(r, tuple) else (r,))]


def test_restart_with_all_three_parts_gives_what_a_fresh_accumulator_gives(sc, batches):
    reads, keys = batches
    rng = np.random.default_rng(59)
    reads2, keys2 = _batch(sc, rng, L), _batch(sc, rng, K)
    fresh = LaneDups(sc, N, T, L)
    ld = LaneDups(sc, N, T, L)
    try:
        for a in (fresh, ld):
            for name in ("qual", "index", "umi"):
                PARTS[name].begin(a)
        _lane_results(ld, reads, keys, ([0, 1, 2],))
        ld.restart()
        got = _flat(_lane_results(ld, reads2, keys2, ([1], [2, 0])))
        want = _flat(_lane_results(fresh, reads2, keys2, ([1], [2, 0])))
        assert len(got) == len(want) > 10
        for g, w in zip(got, want):
            assert g.shape == w.shape and (g == w).all()
        assert (ld.I, ld.U, ld.qual_edges) == (K, K, EDGES)
    finally:
        for a in (fresh, ld):
            a.close()
        reads2.free()
        keys2.free()


def test_a_begin_that_fails_leaves_nothing_allocated(sc, batches):
    """Each part's begin refused by the library after the workspace was allocated (the lane is finished; for the
    qualities also: a tile was added): the workspace is given back and the accumulator has no such part; close() then
    leaves the scanner with the allocations it had."""
    before = set(sc._owned)
    ld = LaneDups(sc, N, T, L)
    try:
        ld.add(batches[0], [0, 1, 2])
        held = set(sc._owned)
        with pytest.raises(ValueError):
            ld.qual_begin(EDGES)
        ld.finish()
        for name in ("qual", "index", "umi"):
            with pytest.raises(ValueError):
                PARTS[name].begin(ld)
        assert set(sc._owned) == held
        assert (ld.d_qual, ld.qual_bytes, ld.qual_edges) == (0, 0, None)
        assert (ld.d_index, ld.index_bytes, ld.I) == (0, 0, 0) and (ld.d_umi, ld.umi_bytes, ld.U) == (0, 0, 0)
    finally:
        ld.close()
    assert set(sc._owned) == before
