"""A lane's distinct reads against its depth on the GPU (LaneDups.saturation, include/welldup_lanesaturation.h) against
the host reference of tests/lanesaturation_ref.py on the labels of tests/lanedups_ref.py / lanenear_ref.py - head row,
NewReads and NewDistinct equal, nothing approximate - however the tiles are fed and whatever hash_bits, and against
the identities the header states."""
import ctypes
import io
import os
import shutil
from contextlib import redirect_stdout

import numpy as np
import pytest

from lanedistance_ref import lane_distances
from lanedups_ref import lane_dups
from lanenear_ref import lane_near_dups
from lanesaturation_ref import MAX_RADIUS, MAX_STEPS, check_saturation_identities, lane_saturation, step_of
from test_gpu_lanemismatch import (COLS, INDEX, MAX_TILES, N, ROWS, WAYS, _finish, _host_tiles, _lane, _plant, _small_lane,
                                   _upload)
from tiledups_ref import INVALID
from well_duplicates_amd import _lib, cluster_indexes
from well_duplicates_amd import count_well_duplicates as cwd
from well_duplicates_amd import report, synth
from well_duplicates_amd.scanner import Scanner

pytestmark = pytest.mark.gpu

STEPS = (1, 7, 20, 64)
FINER = (14, 32)                                                       # for the coarsening 14 -> 7 and 64 -> 32
SEEDS = (0, 12345)
RADII = (None, 0, 32, 300, 2500, MAX_RADIUS)                           # None: without coordinates
CYCLES = 37
MAX_COORD = _lib.LANEDISTANCE_MAX_COORD


@pytest.fixture(scope="module")
def sc():
    s = Scanner(0)
    yield s
    s.close()


def _coords(x, y, radius):
    return dict(x=None, y=None, radius=0) if radius is None else dict(x=x, y=y, radius=radius)


@pytest.fixture(scope="module")
def small():
    """test_gpu_lanemismatch.py's small lane (five tiles of 44 x 60 wells in a lane of seven indices, one tile dead)
    with test_gpu_lanedistance.py's extra equal copies and the coordinates of that honeycomb, and the reference's
    answer under equality labels (k = 0) and under the clusters at K = 2, computed once."""
    reads, filts = _small_lane(2, CYCLES)
    rng = np.random.default_rng(44)
    for src, dst, count in ((0, 3, 150), (1, 2, 120), (0, 4, 100), (2, 2, 150), (4, 4, 100)):
        _plant(reads, rng, src, dst, count, 0)
    tiles = _host_tiles(reads, filts, INDEX)
    x, y = synth.honeycomb_pixels(ROWS, COLS)
    eq_lane, eq_tiles, eq_labels = lane_dups(tiles, N, MAX_TILES)
    near_lane, near_tiles, near_labels = lane_near_dups(tiles, N, MAX_TILES, 2)
    finish = {0: (eq_lane, eq_tiles), 2: (np.concatenate([near_lane[:6], near_lane[7:]]), near_tiles)}
    labels = {0: eq_labels, 2: near_labels}
    want = {(k, s, seed, r): lane_saturation(labels[k], N, MAX_TILES, s, seed, **_coords(x, y, r))
            for k in (0, 2) for s in STEPS + FINER for seed in SEEDS for r in RADII}
    dist = {(k, r): lane_distances(labels[k], N, MAX_TILES, x, y, r)[0] for k in (0, 2) for r in RADII if r is not None}
    return dict(reads=reads, filts=filts, tiles=tiles, x=x, y=y, finish=finish, labels=labels, want=want, dist=dist)


def _same(got, want):
    for g, w, name in zip(got, want, ("head row", "new reads", "new distinct")):
        assert g.dtype == np.int64 and g.shape == w.shape and (g == w).all(), (name, g, w)


# ---- 1: the small lane of test_gpu_lanemismatch.py --------------------------------------------------
@pytest.mark.parametrize("k", [0, 2])
def test_lane_saturation_matches_reference_however_the_tiles_are_fed(sc, small, k):
    x, y, want, dist = small["x"], small["y"], small["want"], small["dist"]
    finish_lane = small["finish"][k][0]
    # the ground is covered: hundreds of same-tile and of cross-tile pairs, some but not all of the former dropped at
    # 32 and at 300 (a tile of 44 x 60 wells is less than 2500 units across: at 2500 every same-tile pair is dropped,
    # as at 2^25), every step of 20 with reads and with new molecules, and dropping moves a molecule to a later step
    pairs, same = int(dist[(k, 2500)][0]), int(dist[(k, 2500)][1])
    assert same >= 100 and pairs - same >= 100
    assert 0 < want[(k, 20, 0, 32)][0][1] < want[(k, 20, 0, 300)][0][1] < same
    assert want[(k, 20, 0, 2500)][0][1] == same == want[(k, 20, 0, MAX_RADIUS)][0][1]
    assert want[(k, 20, 0, 0)][0][1] == 0 == want[(k, 20, 0, None)][0][1]
    for seed in SEEDS:
        assert (want[(k, 20, seed, 2500)][1] > 0).all() and (want[(k, 20, seed, 2500)][2] > 0).all()
        assert (want[(k, 64, seed, MAX_RADIUS)][2] != want[(k, 64, seed, 0)][2]).any()
    assert (want[(k, 20, 0, 0)][1] != want[(k, 20, 12345, 0)][1]).any()
    for (kk, s, seed, r), res in want.items():
        if kk == k:
            check_saturation_identities(*res, finish_lane=finish_lane, local=0 if r is None else int(dist[(k, r)][2]),
                                        finer=want.get((k, 2 * s, seed, r)), other_seed=want[(k, s, 12345 - seed, r)])
    tb = _upload(sc, small["reads"], small["filts"])
    try:
        for bits in (0, 1):
            for calls in WAYS.values():
                ld = _lane(sc, tb, INDEX, MAX_TILES, calls, hash_bits=bits)
                try:
                    rows = _finish(ld, k, bits)
                    assert (rows[0] == finish_lane).all()
                    first = ld.saturation(20, 0, x, y, 2500)            # before the distance pass
                    _same(first, want[(k, 20, 0, 2500)])
                    got = {}
                    for r in RADII:
                        local = 0 if r is None else int(ld.distances(x, y, r)[0][2])
                        for s in STEPS + FINER:
                            for seed in SEEDS:
                                res = got[(s, seed, r)] = ld.saturation(s, seed, **_coords(x, y, r))
                                _same(res, want[(k, s, seed, r)])
                                assert res[0][1] == local               # Dropped = Local of the distance pass
                    for (s, seed, r), res in got.items():
                        check_saturation_identities(*res, finish_lane=rows[0], finer=got.get((2 * s, seed, r)),
                                                    other_seed=got[(s, 12345 - seed, r)])
                    assert (7, 0, 2500) in got and (14, 0, 2500) in got and (32, 0, 32) in got and (64, 0, 32) in got
                    _same(ld.saturation(20, 0, x, y, 2500), first)      # after it, and twice in a row
                    _same(ld.saturation(20, 0, x, y, 2500), first)
                finally:
                    ld.close()
    finally:
        tb.free()


# ---- 2: one molecule --------------------------------------------------------------------------------
BIG_ROWS, BIG_COLS = 90, 100                                           # 9000 wells: a run of 8192 and a bit


def test_a_lane_of_equal_reads_is_one_molecule(sc):
    n, cycles = BIG_ROWS * BIG_COLS, 20
    x, y = synth.honeycomb_pixels(BIG_ROWS, BIG_COLS)
    reads = [np.tile(np.array([0x42 + (c % 4) for c in range(cycles)], dtype=np.uint8), (n, 1))] * 3
    rng = np.random.default_rng(27000)
    filts = [(rng.random(n) >= 0.1).astype(np.uint8) for _ in range(3)]
    tiles = _host_tiles(reads, filts, [0, 1, 2])
    eq_lane, _, labels = lane_dups(tiles, n, 3)
    pf = np.flatnonzero(np.concatenate(filts))
    root = int(pf[0])
    assert 0.85 * 3 * n < pf.size < 0.95 * 3 * n and eq_lane[3] == pf.size - 1 and root < n
    tb = _upload(sc, reads, filts)
    try:
        ld = _lane(sc, tb, [0, 1, 2], 3, [[0, 1, 2]])
        try:
            rows = _finish(ld, 0)
            for s, seed in ((1, 0), (20, 0), (64, 0), (64, 77)):
                step = step_of(np.arange(3 * n), seed, s)
                got = ld.saturation(s, seed, x, y, 0)
                _same(got, lane_saturation(labels, n, 3, s, seed, x, y, 0))
                check_saturation_identities(*got, finish_lane=rows[0], local=0)
                one = np.zeros(s, dtype=np.int64)
                one[step[pf].min()] = 1                                 # a single 1, at the smallest step of any PF well
                assert (got[2] == one).all() and got[0].tolist() == [pf.size, 0]
                assert (got[1] == np.bincount(step[pf], minlength=s)).all()
                _same(ld.saturation(s, seed), got)                      # and without coordinates
                # every member on the root's tile is dropped and none elsewhere; the 1 sits at the rest's minimum
                got = ld.saturation(s, seed, x, y, MAX_RADIUS)
                _same(got, lane_saturation(labels, n, 3, s, seed, x, y, MAX_RADIUS))
                rest = np.concatenate([[root], pf[pf >= n]])
                assert got[0].tolist() == [pf.size, pf.size - rest.size] and pf.size - rest.size == int((pf < n).sum()) - 1
                one[:] = 0
                one[step[rest].min()] = 1
                assert (got[2] == one).all() and (got[1] == np.bincount(step[rest], minlength=s)).all()
                assert got[0][1] == ld.distances(x, y, MAX_RADIUS)[0][2]
        finally:
            ld.close()
    finally:
        tb.free()


# ---- 3: copies beside their originals ---------------------------------------------------------------
def test_copies_beside_their_originals_are_all_dropped(sc):
    n, cycles = 300, 12
    x, y = np.arange(n, dtype=np.int64) * 10, np.full(n, 1000, dtype=np.int64)      # 10 units apart
    rng = np.random.default_rng(300)
    reads = rng.integers(1, 256, (n, cycles)).astype(np.uint8)
    reads[1::2] = reads[0::2]                                          # every odd well: its left neighbour's read
    filt = (rng.random(n) >= 0.15).astype(np.uint8)
    tiles = _host_tiles([reads], [filt], [1])
    eq_lane, _, labels = lane_dups(tiles, n, 2)
    both = int((filt[0::2] & filt[1::2]).sum())
    pf = int(filt.sum())
    assert eq_lane[3] == both and 80 < both < 140 and pf - 2 * both > 20      # pairs, and singletons of either parity
    tb = _upload(sc, [reads], [filt])
    ld = _lane(sc, tb, [1], 2, [[0]])
    try:
        rows = _finish(ld, 0)
        for s in (1, 20, 64):
            got = ld.saturation(s, 3, x, y, 32)
            _same(got, lane_saturation(labels, n, 2, s, 3, x, y, 32))
            assert got[0].tolist() == [pf, both] and (got[1] == got[2]).all() and got[1].sum() == pf - both
            check_saturation_identities(*got, finish_lane=rows[0], local=int(ld.distances(x, y, 32)[0][2]))
            for kw in (dict(x=x, y=y, radius=0), dict(x=x, y=y, radius=10), dict()):         # strictly closer than R: none at 10
                got = ld.saturation(s, 3, **kw)
                _same(got, lane_saturation(labels, n, 2, s, 3, **kw))
                assert got[0].tolist() == [pf, 0] and got[1].sum() == pf and got[2].sum() == pf - both      # roots + singletons
                check_saturation_identities(*got, finish_lane=rows[0], local=0)
    finally:
        ld.close()
        tb.free()


# ---- 4: call discipline -----------------------------------------------------------------------------
def _raw(sc, ld, steps, seed, x, y, radius, scratch, scratch_bytes, missing=()):
    """wd_lane_saturation itself -> (rc, head row, new reads, new distinct); x, y: int32 arrays or None; missing: the
    outputs passed as null (0: head row, 1: new reads, 2: new distinct)"""
    out = [np.full(2, -1, dtype=np.int64), np.full(MAX_STEPS, -1, dtype=np.int64), np.full(MAX_STEPS, -1, dtype=np.int64)]
    ptr = [None if i in missing else a.ctypes.data_as(ctypes.c_void_p) for i, a in enumerate(out)]
    px, py = (None if v is None else v.ctypes.data_as(ctypes.c_void_p) for v in (x, y))
    rc = sc._lib.wd_lane_saturation(ld._h, steps, seed, px, py, radius, ctypes.c_void_p(scratch), scratch_bytes, *ptr)
    return (rc,) + tuple(out)


def _untouched(res):
    return all((a == -1).all() for a in res[1:])


def test_call_discipline(sc, small):
    k, s, seed, r = 2, 20, 12345, 2500
    x64, y64, want = small["x"], small["y"], small["want"]
    x, y = x64.astype(np.int32), y64.astype(np.int32)
    need, need_plain = sc.lane_saturation_scratch_bytes(N, MAX_TILES, True), sc.lane_saturation_scratch_bytes(N, MAX_TILES, False)
    assert need_plain < need
    d_scratch = sc.malloc(need)
    host = np.zeros(need, dtype=np.uint8)
    tb = _upload(sc, small["reads"], small["filts"])
    ld = _lane(sc, tb, INDEX, MAX_TILES, WAYS["2 + 3"])
    try:
        res = _raw(sc, ld, s, seed, x, y, r, d_scratch, need)          # before any finish
        assert res[0] == _lib.ERR_ARG and _untouched(res)
        with pytest.raises(ValueError):
            ld.saturation(s, seed, x64, y64, r)
        with pytest.raises(RuntimeError):                              # a near finish refused over budget is no finish
            ld.finish(hamming=k, pair_budget=3)
        res = _raw(sc, ld, s, seed, x, y, r, d_scratch, need)
        assert res[0] == _lib.ERR_ARG and _untouched(res) and b"finish" in sc._lib.wd_last_error(sc._ctx)
        rows = _finish(ld, k)

        def good():                                                    # after every refusal: the reference's result
            first = _raw(sc, ld, s, seed, x, y, r, d_scratch, need)
            assert first[0] == _lib.OK and (first[2][s:] == -1).all() and (first[3][s:] == -1).all()
            _same((first[1], first[2][:s], first[3][:s]), want[(k, s, seed, r)])

        good()
        far = x.copy()
        far[1234] = MAX_COORD + 1
        low = y.copy()
        low[77] = -1
        for bad in (dict(steps=0), dict(steps=-1), dict(steps=MAX_STEPS + 1), dict(radius=-1), dict(radius=MAX_RADIUS + 1),
                    dict(x=None), dict(y=None), dict(x=None, y=None), dict(missing=(0,)), dict(missing=(1,)),
                    dict(missing=(2,)), dict(scratch=0), dict(scratch_bytes=need - 256), dict(scratch_bytes=0),
                    dict(scratch_bytes=need_plain), dict(scratch=host.ctypes.data), dict(x=far), dict(y=low),
                    dict(x=far, radius=0)):
            args = dict(steps=s, seed=seed, x=x, y=y, radius=r, scratch=d_scratch, scratch_bytes=need)
            args.update(bad)
            res = _raw(sc, ld, **args)
            assert res[0] == _lib.ERR_ARG and _untouched(res), bad
            if bad.get("x") is not None:
                assert b"well 1234 " in sc._lib.wd_last_error(sc._ctx)
            if bad.get("y") is not None:
                assert b"well 77 " in sc._lib.wd_last_error(sc._ctx)
            good()
        for kw in (dict(steps=0), dict(steps=MAX_STEPS + 1), dict(radius=-1), dict(radius=MAX_RADIUS + 1), dict(seed=-1),
                   dict(seed=1 << 32), dict(x=None), dict(y=None), dict(x=None, y=None), dict(x=x64[:-1], y=y64[:-1]),
                   dict(x=far.astype(np.int64) + (1 << 32))):          # (what int32 would fold back into range)
            args = dict(steps=s, seed=seed, x=x64, y=y64, radius=r)
            args.update(kw)
            with pytest.raises(ValueError):
                ld.saturation(**args)
            good()
        # without coordinates the smaller scratch is enough, and with them radius 0 gives the same
        res = _raw(sc, ld, s, seed, None, None, 0, d_scratch, need_plain)
        assert res[0] == _lib.OK
        _same((res[1], res[2][:s], res[3][:s]), want[(k, s, seed, None)])
        _same(ld.saturation(s, seed, x64, y64, 0), want[(k, s, seed, None)])
        mm_before = ld.mismatches(k)
        _same(ld.saturation(s, seed, x64, y64, r), want[(k, s, seed, r)])      # after the mismatch pass
        mm_after = ld.mismatches(k)
        assert all((a == b).all() for a, b in zip(mm_before, mm_after))
        check_saturation_identities(*ld.saturation(s, seed, x64, y64, r), finish_lane=rows[0])
        # another lane in the same workspace, by equality
        ld.restart()
        with pytest.raises(ValueError):
            ld.saturation(s, seed, x64, y64, r)
        ld.add(tb, INDEX)
        rows = _finish(ld, 0)
        got = ld.saturation(s, seed, x64, y64, r)
        _same(got, want[(0, s, seed, r)])
        check_saturation_identities(*got, finish_lane=rows[0])
        ld.close()
        with pytest.raises(ValueError):
            ld.saturation(s, seed, x64, y64, r)
    finally:
        ld.close()
        tb.free()
        sc.free(d_scratch)


# ---- 5: the CLI -------------------------------------------------------------------------------------
def _main(argv):
    out = io.StringIO()
    with redirect_stdout(out):
        assert cwd.main(argv) == 0
    return out.getvalue()


def test_cli_lane_saturation_block(tmp_path):
    """The run directory of test_gpu_lanedistance.py's CLI test: tile 1103's files are tile 1101's but for the last
    cycle, which is tile 1102's.  The new block closes the lane's output, equals write_lane_saturation of the
    reference's counts and is all the flag adds; with --lane-dups-distance it takes that block's radius and drops
    that block's Local; with --lane-dups-hamming it is on the clusters."""
    rows, cols, levels, L, lane = 36, 70, 3, 24, 1
    n = rows * cols
    x, y = synth.honeycomb_pixels(rows, cols)
    spec = synth.SynthSpec(seed=35, n_clusters=n, row=cols, plant_per_64k=8000, nocall_per_64k=500, plant_far=True)
    run_dir = str(tmp_path / "run")
    names = ["1101", "1102", "1103", "1104"]
    synth.write_run_dir(spec, run_dir, [lane], names, list(range(L)), slocs=synth.slocs_bytes(x, y))
    rx, ry = cluster_indexes.read_slocs(os.path.join(run_dir, "Data", "Intensities", "s.locs"))
    assert (rx == x).all() and (ry == y).all()
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
    eq = lane_dups(tiles, n, 4)
    near = lane_near_dups(tiles, n, 4, 2)

    def block(k, steps, seed, radius, summary):
        final = report.LaneNearCounts.from_rows(near[0], near[1], names) if k else report.LaneDupCounts.from_rows(eq[0], eq[1], names)
        res = lane_saturation(near[2] if k else eq[2], n, 4, steps, seed, **_coords(x, y, radius or None))
        counts = report.LaneSaturationCounts.from_rows(*res, seed, radius, final, k)
        text = io.StringIO()
        report.write_lane_saturation(str(lane), counts, verbose=not summary, out=text)
        return text.getvalue(), counts

    new = ["--lane-dups-saturation"]
    plain = _main(argv)
    want, counts = block(0, 20, 0, 0, False)
    assert counts.redundant > 200 and counts.dropped == 0 and min(counts.new_distinct) > 0
    assert _main(argv + new) == plain + want                           # the new block is all the flag adds
    assert want.count("LaneSaturation: 1\tStep: ") == 20 and "Local copies dropped: none" in want
    # with the distance block: its radius, and its Local is what is dropped
    dist = ["--lane-dups-distance", "--lane-dups-distance-radius", "40"]
    with_dist = _main(argv + dist)
    want, counts = block(0, 20, 0, 40, False)
    got = _main(argv + dist + new)
    assert got == with_dist + want and "closer than R = 40 to" in want
    assert 0 < counts.dropped and ("\tR: 40\t" in with_dist) and ("\tLocal: %i (" % counts.dropped) in with_dist
    # on the clusters, with steps, seed and a radius of its own, the summary alone
    near_args = ["--lane-dups-hamming", "2", "-S"]
    want, counts = block(2, 7, 99, 2500, True)
    got = _main(argv + near_args + dist + new + ["--lane-dups-saturation-steps", "7", "--lane-dups-saturation-seed", "99",
                                                 "--lane-dups-saturation-radius", "2500"])
    assert got == _main(argv + near_args + dist) + want
    assert "Steps: 7\tSeed: 99\tHamming: 2\t" in want and "LaneSaturation: 1\tStep:" not in want and "R = 2500" in want
    assert counts.dropped > 0 and "LaneNearDupsSummary: 1" in got
