"""How far apart a lane's duplicate copies lie on the GPU (LaneDups.distances, include/welldup_lanedistance.h) against
the host reference of tests/lanedistance_ref.py on the labels of tests/lanedups_ref.py / lanenear_ref.py - lane row,
tile rows and TilePairs equal, nothing approximate - however the tiles are fed and whatever hash_bits, and against
the identities the header states."""
import ctypes
import io
import os
import shutil
from contextlib import redirect_stdout

import numpy as np
import pytest

from lanedistance_ref import EDGES, LANE_COLS, MAX_COORD, MAX_RADIUS, check_distance_identities, dist_bin, lane_distances
from lanedups_ref import lane_dups
from lanenear_ref import lane_near_dups
from test_gpu_lanemismatch import (COLS, INDEX, MAX_TILES, N, ROWS, WAYS, _finish, _host_tiles, _lane, _plant, _small_lane,
                                   _tables, _upload)
from well_duplicates_amd import _lib, cluster_indexes
from well_duplicates_amd import count_well_duplicates as cwd
from well_duplicates_amd import report, synth
from well_duplicates_amd.scanner import Scanner, TileBatch

pytestmark = pytest.mark.gpu

RADII = (0, 32, 33, 2500, MAX_RADIUS)
CYCLES = 37


@pytest.fixture(scope="module")
def sc():
    s = Scanner(0)
    yield s
    s.close()


@pytest.fixture(scope="module")
def small():
    """test_gpu_lanemismatch.py's small lane (five tiles of 44 x 60 wells in a lane of seven indices, one tile dead,
    copies planted within and across tiles) with the coordinates of that honeycomb, and the reference's answer under
    equality labels (k = 0) and under the clusters at K = 2, computed once.  That lane's equal reads across tiles are
    few (its copies differ at a cycle or more), so some more are planted, within tiles anywhere and across tiles."""
    reads, filts = _small_lane(2, CYCLES)
    rng = np.random.default_rng(44)
    for src, dst, count in ((0, 3, 150), (1, 2, 120), (0, 4, 100), (2, 2, 150), (4, 4, 100)):
        _plant(reads, rng, src, dst, count, 0)         # and equal copies, so that equality has its hundreds across tiles too
    tiles = _host_tiles(reads, filts, INDEX)
    x, y = synth.honeycomb_pixels(ROWS, COLS)
    eq_lane, eq_tiles, eq_labels = lane_dups(tiles, N, MAX_TILES)
    near_lane, near_tiles, near_labels = lane_near_dups(tiles, N, MAX_TILES, 2)
    finish = {0: (eq_lane, eq_tiles), 2: (np.concatenate([near_lane[:6], near_lane[7:]]), near_tiles)}
    labels = {0: eq_labels, 2: near_labels}
    want = {(k, r): lane_distances(labels[k], N, MAX_TILES, x, y, r) for k in (0, 2) for r in RADII}
    return dict(reads=reads, filts=filts, tiles=tiles, x=x, y=y, finish=finish, labels=labels, want=want)


def _same(got, want):
    for g, w, name in zip(got, want, ("lane row", "tile rows", "tile pairs")):
        assert g.shape == w.shape and (g == w).all(), (name, g[g != w], w[g != w], np.argwhere(g != w)[:8])


# ---- 1: the small lane of test_gpu_lanemismatch.py --------------------------------------------------
@pytest.mark.parametrize("k", [0, 2])
def test_lane_distances_match_reference_however_the_tiles_are_fed(sc, small, k):
    x, y, want = small["x"], small["y"], small["want"]
    # the ground is covered: same-tile and cross-tile pairs in the hundreds, three bins and more, roots elsewhere
    lane, trow, pairs = want[(k, 2500)]
    assert lane[1] >= 100 and lane[0] - lane[1] >= 100, lane
    assert (lane[3:] > 0).sum() >= 3 and np.triu(pairs, 1).sum() == lane[0] - lane[1] > 0
    assert want[(k, 0)][0][2] == 0 < want[(k, 32)][0][2] <= want[(k, 33)][0][2] <= lane[2] <= want[(k, MAX_RADIUS)][0][2] == lane[1]
    local_at = lambda r: lane_distances(small["labels"][k], N, MAX_TILES, x, y, r)[0][2]
    for r in RADII:
        check_distance_identities(*want[(k, r)], r, *small["finish"][k], local_at=local_at if r == 2500 else None)
    tb = _upload(sc, small["reads"], small["filts"])
    try:
        for bits in (0, 1):
            for calls in WAYS.values():
                ld = _lane(sc, tb, INDEX, MAX_TILES, calls, hash_bits=bits)
                try:
                    rows = _finish(ld, k, bits)
                    for r in RADII:
                        got = ld.distances(x, y, r)
                        _same(got, want[(k, r)])
                        check_distance_identities(*got, r, *rows)
                finally:
                    ld.close()
    finally:
        tb.free()


# ---- 2: the bins' edges and 64-bit arithmetic -------------------------------------------------------
def _two_squares_at_most(q):
    """-> (q', dx, dy): the largest q' <= q that is a sum of two squares, and such squares."""
    while True:
        dx = int(np.sqrt(q))
        while dx * dx > q:
            dx -= 1
        for a in range(dx, -1, -1):
            b = int(round(np.sqrt(q - a * a)))
            if a * a + b * b == q:
                return q, a, b
        q -= 1


def test_both_sides_of_every_edge_and_the_longest_distance(sc):
    """One tile of 300 wells on the line y = 0 but for the copies: for every edge 2^(10 + 2j), j = 0..9, a pair with
    q on the edge (dx = 32 x 2^j) and a pair just below it.  q = 2^(10 + 2j) - 1 itself cannot be planted: it is
    3 (mod 4), and no sum of two squares is; the pair below the edge takes the largest sum of two squares under the
    edge, which the search finds within a few units of it (1021 = 30^2 + 11^2 under 1024).  One more pair spans
    (0, 0) .. (2^24 - 1, 2^24 - 1): q = 2 (2^24 - 1)^2, where a 32-bit product is wrong.  The radii: every edge and
    every edge +- 1."""
    n, cycles = 300, 12
    x, y = np.arange(n, dtype=np.int64) * 50000, np.zeros(n, dtype=np.int64)      # roots and bystanders 50 000 apart
    assert x.max() + 20000 <= MAX_COORD
    rng = np.random.default_rng(300)
    reads = rng.integers(1, 256, (n, cycles)).astype(np.uint8)
    filt = np.ones(n, dtype=np.uint8)
    filt[250:] = 0
    planted, well = [], 0
    for j, edge in enumerate(EDGES):
        below, dx, dy = _two_squares_at_most(edge * edge - 1)
        assert edge * edge - 8 <= below < edge * edge and dist_bin([below, edge * edge]).tolist() == [j, j + 1]
        for q, ax, ay in ((below, dx, dy), (edge * edge, edge, 0)):
            x[well + 1], y[well + 1] = x[well] + ax, y[well] + ay
            reads[well + 1] = reads[well]
            planted.append(q)
            well += 2
    x[well], y[well], x[well + 1], y[well + 1] = 0, 0, MAX_COORD, MAX_COORD
    reads[well + 1] = reads[well]
    planted.append(2 * MAX_COORD * MAX_COORD)
    assert planted[-1] > 1 << 48
    tiles = _host_tiles([reads], [filt], [1])
    eq_lane, eq_tiles, labels = lane_dups(tiles, n, 2)
    radii = sorted({r for e in EDGES for r in (e - 1, e, e + 1)})
    want = {r: lane_distances(labels, n, 2, x, y, r) for r in radii + [MAX_RADIUS]}
    lane = want[MAX_RADIUS][0]
    assert lane[0] == lane[1] == 21 and lane[3:].tolist() == [1] + [2] * 9 + [2]      # every bin, both sides of every edge
    for j, e in enumerate(EDGES):                                      # the pair on the edge is not closer than the edge
        assert want[e - 1][0][2] == 2 * j == want[e][0][2] - 1 and want[e + 1][0][2] == 2 * j + 2
    tb = _upload(sc, [reads], [filt])
    ld = _lane(sc, tb, [1], 2, [[0]])
    try:
        rows = _finish(ld, 0)
        for r in radii + [MAX_RADIUS]:
            got = ld.distances(x, y, r)
            _same(got, want[r])
            check_distance_identities(*got, r, *rows, classes_of_two=True)
        lane_only = ld.distances(x, y, 2500, matrix=False)
        assert lane_only[2] is None
        _same(lane_only[:2], lane_distances(labels, n, 2, x, y, 2500)[:2])
    finally:
        ld.close()
        tb.free()


# ---- 3: contention ----------------------------------------------------------------------------------
BIG_ROWS, BIG_COLS = 90, 100                                           # 9000 wells: a run of 8192 and a bit


def _three_tiles(reads):
    filts = [np.ones(BIG_ROWS * BIG_COLS, dtype=np.uint8)] * 3
    return filts, _host_tiles(reads, filts, [0, 1, 2])


def test_a_lane_of_equal_reads_is_one_root(sc):
    n, cycles = BIG_ROWS * BIG_COLS, 20
    x, y = synth.honeycomb_pixels(BIG_ROWS, BIG_COLS)
    reads = [np.tile(np.array([0x42 + (c % 4) for c in range(cycles)], dtype=np.uint8), (n, 1))] * 3
    filts, tiles = _three_tiles(reads)
    labels = lane_dups(tiles, n, 3)[2]
    want = lane_distances(labels, n, 3, x, y, 2500)
    assert want[0][:2].tolist() == [3 * n - 1, n - 1] and want[2].tolist() == [[n - 1, n, n], [0] * 3, [0] * 3]
    assert (want[0][3:] > 0).sum() >= 5                                # every well of tile 0 against well 0: near and far
    tb = _upload(sc, reads, filts)
    try:
        ld = _lane(sc, tb, [0, 1, 2], 3, [[0, 1, 2]])
        try:
            rows = _finish(ld, 0)
            got = ld.distances(x, y, 2500)
            _same(got, want)
            check_distance_identities(*got, 2500, *rows)
        finally:
            ld.close()
    finally:
        tb.free()


def test_copies_beside_their_originals_are_one_bin(sc):
    n, cycles = BIG_ROWS * BIG_COLS, 20
    x, y = synth.honeycomb_pixels(BIG_ROWS, BIG_COLS)
    rng = np.random.default_rng(9000)
    reads = [rng.integers(1, 256, (n, cycles)).astype(np.uint8) for _ in range(3)]
    for r in reads:
        r[1::2] = r[0::2]                                              # every well of odd index: its left neighbour's read
    filts, tiles = _three_tiles(reads)
    labels = lane_dups(tiles, n, 3)[2]
    want = lane_distances(labels, n, 3, x, y, 32)
    half = n // 2
    assert want[0].tolist() == [3 * half, 3 * half, 3 * half, 3 * half] + [0] * 10
    assert want[1].tolist() == [[half] * 3] * 3 and want[2].tolist() == np.diag([half] * 3).tolist()
    tb = _upload(sc, reads, filts)
    try:
        ld = _lane(sc, tb, [0, 1, 2], 3, [[0], [1, 2]])
        try:
            rows = _finish(ld, 0)
            got = ld.distances(x, y, 32)
            _same(got, want)
            check_distance_identities(*got, 32, *rows, classes_of_two=True)
        finally:
            ld.close()
    finally:
        tb.free()


# ---- 4: call discipline -----------------------------------------------------------------------------
def _raw(sc, ld, x, y, radius, scratch, scratch_bytes, missing=(), matrix=True):
    """wd_lane_distances itself -> (rc, lane row, tile rows, tile pairs); x, y: int32 arrays or None; missing: the
    outputs passed as null (0: lane row, 1: tile rows); matrix=False: tile_pairs is null"""
    out = [np.full(LANE_COLS, -1, dtype=np.int64), np.full((ld.max_tiles, 3), -1, dtype=np.int64),
           np.full((ld.max_tiles, ld.max_tiles), -1, dtype=np.int64)]
    ptr = [None if i in missing or (i == 2 and not matrix) else a.ctypes.data_as(ctypes.c_void_p) for i, a in enumerate(out)]
    px, py = (None if v is None else v.ctypes.data_as(ctypes.c_void_p) for v in (x, y))
    rc = sc._lib.wd_lane_distances(ld._h, px, py, radius, ctypes.c_void_p(scratch), scratch_bytes, *ptr)
    return (rc,) + tuple(out)


def _untouched(res):
    return all((a == -1).all() for a in res[1:])


def test_call_discipline(sc, small):
    k, r = 2, 2500
    x64, y64, want = small["x"], small["y"], small["want"]
    x, y = x64.astype(np.int32), y64.astype(np.int32)
    need, need_lane = sc.lane_distance_scratch_bytes(N, MAX_TILES, True), sc.lane_distance_scratch_bytes(N, MAX_TILES, False)
    assert need_lane < need
    d_scratch = sc.malloc(need)
    host = np.zeros(need, dtype=np.uint8)
    reads, filts = small["reads"], small["filts"]
    tb = _upload(sc, reads, filts)
    idx = TileBatch(sc, len(reads), 8, N)                              # index reads: the first eight cycles, again
    for i, rd in enumerate(reads):
        idx.upload_tile(i, [np.ascontiguousarray(rd[:, c]) for c in range(8)], filts[i])
    ld = _lane(sc, tb, INDEX, MAX_TILES, WAYS["2 + 3"])
    try:
        ld.index_begin(8)
        ld.index_add(idx, INDEX)
        res = _raw(sc, ld, x, y, r, d_scratch, need)                   # before any finish
        assert res[0] == _lib.ERR_ARG and _untouched(res)
        with pytest.raises(ValueError):
            ld.distances(x64, y64, r)
        with pytest.raises(RuntimeError):                              # a near finish refused over budget is no finish
            ld.finish(hamming=k, pair_budget=3)
        res = _raw(sc, ld, x, y, r, d_scratch, need)
        assert res[0] == _lib.ERR_ARG and _untouched(res) and b"finish" in sc._lib.wd_last_error(sc._ctx)
        rows = _finish(ld, k)

        def good():                                                    # after every refusal: the reference's result
            first = _raw(sc, ld, x, y, r, d_scratch, need)
            assert first[0] == _lib.OK
            _same(first[1:], want[(k, r)])

        good()
        far = x.copy()
        far[1234] = MAX_COORD + 1
        low = y.copy()
        low[77] = -1
        for bad in (dict(radius=-1), dict(radius=MAX_RADIUS + 1), dict(x=None), dict(y=None), dict(missing=(0,)),
                    dict(missing=(1,)), dict(scratch=0), dict(scratch_bytes=need - 256), dict(scratch_bytes=0),
                    dict(scratch_bytes=need_lane), dict(scratch=host.ctypes.data), dict(x=far), dict(y=low)):
            args = dict(x=x, y=y, radius=r, scratch=d_scratch, scratch_bytes=need)
            args.update(bad)
            res = _raw(sc, ld, **args)
            assert res[0] == _lib.ERR_ARG and _untouched(res), bad
            if "x" in bad and bad["x"] is not None:
                assert b"well 1234 " in sc._lib.wd_last_error(sc._ctx)
            if "y" in bad and bad["y"] is not None:
                assert b"well 77 " in sc._lib.wd_last_error(sc._ctx)
            good()
        for rad in (-1, MAX_RADIUS + 1):
            with pytest.raises(ValueError):
                ld.distances(x64, y64, rad)
        with pytest.raises(ValueError):
            ld.distances(far.astype(np.int64) + (1 << 32), y64, r)     # (what int32 would fold back into range)
        with pytest.raises(ValueError):
            ld.distances(x64[:-1], y64[:-1], r)
        # tile_pairs = NULL: the smaller scratch is enough, and the rows are the same
        res = _raw(sc, ld, x, y, r, d_scratch, need_lane, matrix=False)
        assert res[0] == _lib.OK and (res[3] == -1).all()
        _same(res[1:3], want[(k, r)][:2])
        _same(ld.distances(x64, y64, r), want[(k, r)])                 # twice the same
        _same(ld.distances(x64, y64, r), want[(k, r)])
        mm_before = ld.mismatches(k)
        _same(ld.distances(x64, y64, r), want[(k, r)])                 # after the mismatch pass
        index_before = ld.index_finish(min_pf=1)
        for rad in RADII:
            got = ld.distances(x64, y64, rad)                          # and after the index finish, at every radius
            _same(got, want[(k, rad)])
            check_distance_identities(*got, rad, *rows)
        mm_after, index_after = ld.mismatches(k), ld.index_finish(min_pf=1)      # which give what they gave before
        assert all((a == b).all() for a, b in zip(mm_before, mm_after))
        assert all((a == b).all() for a, b in zip(index_before, index_after))
        # another lane in the same workspace, by equality
        ld.restart()
        with pytest.raises(ValueError):
            ld.distances(x64, y64, r)
        for slots in WAYS["descending indices"]:
            ld.add_tables([INDEX[s] for s in slots], _tables(tb, slots))
        ld.index_add(idx, INDEX)
        rows = _finish(ld, 0)
        got = ld.distances(x64, y64, r)
        _same(got, want[(0, r)])
        check_distance_identities(*got, r, *rows)
        ld.close()
        with pytest.raises(ValueError):
            ld.distances(x64, y64, r)
    finally:
        ld.close()
        idx.free()
        tb.free()
        sc.free(d_scratch)


# ---- 5: the CLI -------------------------------------------------------------------------------------
def _main(argv):
    out = io.StringIO()
    with redirect_stdout(out):
        assert cwd.main(argv) == 0
    return out.getvalue()


def test_cli_lane_distance_block(tmp_path):
    """The run directory of test_gpu_lanemismatch.py's CLI test, one lane of it and 24 cycles: tile 1103's files are
    tile 1101's but for the last cycle, which is tile 1102's.  The new block closes the lane's output, equals
    write_lane_distances of the reference's counts, is the same for --tile-batch 1 and the default, is all the flag
    adds, and is there - on the clusters, at another radius - with --lane-dups-hamming 2."""
    rows, cols, levels, L, lane = 36, 70, 3, 24, 1
    n = rows * cols
    x, y = synth.honeycomb_pixels(rows, cols)
    spec = synth.SynthSpec(seed=35, n_clusters=n, row=cols, plant_per_64k=8000, nocall_per_64k=500, plant_far=True)
    run_dir = str(tmp_path / "run")
    names = ["1101", "1102", "1103", "1104"]
    synth.write_run_dir(spec, run_dir, [lane], names, list(range(L)), slocs=synth.slocs_bytes(x, y))
    rx, ry = cluster_indexes.read_slocs(os.path.join(run_dir, "Data", "Intensities", "s.locs"))
    assert (rx == x).all() and (ry == y).all()
    area = float(x.max() - x.min()) * float(y.max() - y.min())
    source = lambda t, c: "1101" if t == "1103" and c < L - 1 else "1102" if t == "1103" else t
    ldir = os.path.join(run_dir, "Data", "Intensities", "BaseCalls", "L%03d" % lane)
    shutil.copy(os.path.join(ldir, "s_%d_1101.filter" % lane), os.path.join(ldir, "s_%d_1103.filter" % lane))
    for c in range(L):
        cdir = os.path.join(ldir, "C%d.1" % (c + 1))
        shutil.copy(os.path.join(cdir, "s_%d_%s.bcl.gz" % (lane, source("1103", c))),
                    os.path.join(cdir, "s_%d_1103.bcl.gz" % lane))
    argv = ["-s", "hiseq_x", "-r", run_dir, "-t", "1101,1102,1103,1104", "-i", str(lane), "-l", str(levels),
            "--cycles", "0-%d" % L, "-q", "--all-wells", "--lane-dups"]
    cases = {"equality": ([], 0, 2500, False), "hamming": (["--lane-dups-hamming", "2", "-S"], 2, 40, True)}
    tiles = [(i, [synth.plane_bytes(spec, lane, int(source(t, c)), c) for c in range(L)],
              synth.filter_bytes(spec, lane, int(t if t != "1103" else "1101"))) for i, t in enumerate(names)]
    eq = lane_dups(tiles, n, 4)
    near = lane_near_dups(tiles, n, 4, 2)
    blocks = {}
    for case, (_, k, radius, summary) in cases.items():
        final = report.LaneNearCounts.from_rows(near[0], near[1], names) if k else report.LaneDupCounts.from_rows(eq[0], eq[1], names)
        res = lane_distances(near[2] if k else eq[2], n, 4, x, y, radius)
        counts = report.LaneDistanceCounts.from_rows(*res, names, radius, final, area)
        assert counts.same_tile > 100 and counts.cross_tile > 100 and 0 < counts.local <= counts.same_tile
        assert radius != 40 or counts.local < counts.same_tile
        assert counts.library_size_without_local() > final.library_size() > 0
        text = io.StringIO()
        report.write_lane_distances(str(lane), counts, verbose=not summary, out=text)
        blocks[case] = text.getvalue()
    new = ["--lane-dups-distance"]
    plain = _main(argv)
    runs = [_main(argv + new + ["--tile-batch", "1"]), _main(argv + new)]
    block = blocks["equality"]
    assert runs[0] == runs[1] == plain + block                         # the new block is all the flag adds
    assert "LaneDistances: 1\tTile: 1103\t" in block and "(R = 2500;" in block
    assert "Estimated library size (distinct/X = 1 - exp(-PF/X)): " in plain          # (the existing line stays)
    clusters = _main(argv + cases["hamming"][0] + new + ["--lane-dups-distance-radius", "40"])
    block = blocks["hamming"]
    assert clusters.endswith(block) and clusters.count(block) == 1 and block != blocks["equality"]
    assert "LaneNearDupsSummary: 1" in clusters[:-len(block)] and "LaneDistances: 1\tTile:" not in block
    assert "Estimated library size without local copies (R = 40;" in block
