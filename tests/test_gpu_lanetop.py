"""A lane's most frequent reads and their spread on the GPU (LaneDups.top, include/welldup_lanetop.h) against the host
reference of tests/lanetop_ref.py on the labels of tests/lanedups_ref.py / lanenear_ref.py - head row, levels, roots,
sizes, exact counts, tile counts and reads equal, nothing approximate - however the tiles are fed, whatever hash_bits
and whatever the candidate capacity, and against the identities the header states."""
import ctypes
import io
import os
import shutil
from contextlib import redirect_stdout

import numpy as np
import pytest

from lanedups_ref import lane_dups
from lanenear_ref import lane_near_dups
from lanetop_ref import EDGES, LEVELS, MAX_PASSES, MAX_TOP, check_top_identities, lane_top, level_of
from test_gpu_lanemismatch import (BYTE, INDEX, MAX_TILES, N, WAYS, _finish, _host_tiles, _lane, _other_base, _small_lane,
                                   _upload)
from well_duplicates_amd import _lib, report, synth
from well_duplicates_amd import count_well_duplicates as cwd
from well_duplicates_amd.scanner import Scanner

pytestmark = pytest.mark.gpu

CYCLES = 37
N_TOPS = (1, 5, 18, 100, 1024)
# the sizes the issue names, and a size on either side of every edge of the first pass's log-linear bins up to 512
# (csrc/lane_top.inc: a bin per size below 8, then 8, 12, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512), and 4, 5, 6
# so that no level is empty
SIZES = (2, 3, 8, 9, 10, 11, 49, 50, 51, 63, 64, 65, 99, 100, 101, 499, 500, 501)
EDGE_SIZES = (4, 5, 6, 7, 12, 15, 16, 23, 24, 31, 32, 47, 48, 95, 96, 127, 128, 191, 192, 255, 256, 383, 384, 511, 512)
PAIRS = 320
NEAR_SIZES = (6, 20, 30)


@pytest.fixture(scope="module")
def sc():
    s = Scanner(0)
    yield s
    s.close()


def _fresh_read(rng, cycles):
    r = np.array([BYTE[c] for c in rng.integers(0, 4, cycles)], dtype=np.uint8)
    r[rng.random(cycles) < 0.03] = 0                                   # a no-call here and there
    return r


def _plant_families(reads, filts, rng):
    """Families of exactly the sizes above on PF wells nobody else is given: every third inside one tile, the others
    dealt round the tiles; PAIRS families of size 2; and, for K = 2, families whose copies carry 0, 1 or 2 mismatches
    against the family's read.  -> the sizes planted with equal copies"""
    cycles = reads[0].shape[1]
    pools = [rng.permutation(np.flatnonzero(f & 1)).tolist() for f in filts]
    live = [s for s, p in enumerate(pools) if p]

    def take(count, one_tile):
        if one_tile:
            s = max(live, key=lambda t: len(pools[t]))
            assert len(pools[s]) >= count
            return [(s, pools[s].pop()) for _ in range(count)]
        out, i = [], 0
        while len(out) < count:
            s = live[i % len(live)]
            i += 1
            if pools[s]:
                out.append((s, pools[s].pop()))
            else:
                assert any(pools[t] for t in live), "the lane has too few PF wells for the families"
        return out

    planted = []
    for i, size in enumerate(SIZES + EDGE_SIZES + (2,) * PAIRS):
        read = _fresh_read(rng, cycles)
        for s, w in take(size, one_tile=i % 3 == 0 and size <= 130):
            reads[s][w] = read
        planted.append(size)
    for size in NEAR_SIZES:
        read = _fresh_read(rng, cycles)
        for j, (s, w) in enumerate(take(size, one_tile=False)):
            reads[s][w] = read
            for c in rng.choice(cycles, j % 3, replace=False).tolist():
                reads[s][w, c] = _other_base(read[c])
    return planted


@pytest.fixture(scope="module")
def small():
    """test_gpu_lanemismatch.py's small lane (five tiles of 44 x 60 wells in a lane of seven indices, one tile dead, 37
    cycles) with the families above, and the reference's answer under the classes (k = 0) and the clusters at K = 2."""
    reads, filts = _small_lane(2, CYCLES)
    planted = _plant_families(reads, filts, np.random.default_rng(2048))
    tiles = _host_tiles(reads, filts, INDEX)
    eq_lane, _, eq_labels = lane_dups(tiles, N, MAX_TILES)
    near_lane, _, near_labels = lane_near_dups(tiles, N, MAX_TILES, 2)
    finish = {0: eq_lane, 2: np.concatenate([near_lane[:6], near_lane[7:]])}
    labels = {0: eq_labels, 2: near_labels}
    want = {(k, t): lane_top(labels[k], tiles, N, MAX_TILES, t) for k in (0, 2) for t in N_TOPS}
    return dict(reads=reads, filts=filts, tiles=tiles, finish=finish, want=want, planted=planted,
                live=sum(1 for f in filts if (f & 1).any()))


def _same(got, want):
    names = ("head row", "levels", "root", "size", "exact", "tile_count")
    for g, w, name in zip(got, want, names):
        assert g.dtype == w.dtype and g.shape == w.shape and (g == w).all(), (name, g, w)
    assert got[6] == want[6]


# ---- 1: the small lane of test_gpu_lanemismatch.py --------------------------------------------------
@pytest.mark.parametrize("k", [0, 2])
def test_lane_top_matches_reference_however_the_tiles_are_fed(sc, small, k):
    want, finish_lane, live = small["want"], small["finish"][k], small["live"]
    # the ground is covered, on the reference's answer: every planted size is a group's size, the cut at 100 splits a
    # tie, every level up to 500 is non-empty, a listed group lies on one tile and another on every tile with a PF
    # well, under K = 2 some group holds wells that differ from its root, and 1024 is more than the lane's groups
    # (test_fewer_groups_than_asked covers a list that ends before n_top on a lane of three)
    full = want[(k, 1024)]
    all_sizes = full[3].tolist()
    assert set(small["planted"]) <= set(all_sizes) and full[0][2] == min(full[0][1], 1024)
    groups = full[1][0]
    assert (groups[:level_of([500])[0] + 1] > 0).all(), groups
    hundred = want[(k, 100)]
    assert hundred[0][1] > 100 and all_sizes[99] == all_sizes[100] == hundred[3][99]
    touched = (hundred[5] > 0).sum(axis=1)
    assert live >= 4 and (touched == 1).any() and (touched == live).any()
    assert groups[1] >= 300
    if k:
        assert (full[4] < full[3]).any()
    for t in N_TOPS:
        check_top_identities(*want[(k, t)], n=N, n_top=t, finish_lane=finish_lane, equality=k == 0,
                             longer=full if t < 1024 else None, cycles=CYCLES)
    tb = _upload(sc, small["reads"], small["filts"])
    try:
        for bits in (0, 1):
            for calls in WAYS.values():
                ld = _lane(sc, tb, INDEX, MAX_TILES, calls, hash_bits=bits)
                try:
                    rows = _finish(ld, k, bits)
                    assert (rows[0] == finish_lane).all()
                    first = ld.top(100, 100)                            # before every other pass
                    _same(first, want[(k, 100)])
                    assert sc.get_option("lane_top_passes") > 1         # the cut lies inside a tie: the ids were refined
                    for t in N_TOPS:
                        for cap in (t, 2 * t, 0):                       # full refinement incl. the ids; a little room; the default
                            got = ld.top(t, cap)
                            _same(got, want[(k, t)])
                            passes = sc.get_option("lane_top_passes")
                            assert 1 <= passes <= MAX_PASSES == sc.get_option("lane_top_max_passes")
                            assert passes == 1 or cap                   # the default buffer holds every group of this lane
                        check_top_identities(*got, n=N, n_top=t, finish_lane=rows[0], equality=k == 0, cycles=CYCLES)
                    ld.mismatches(k)
                    ld.distances(*synth.honeycomb_pixels(44, 60), 300)
                    ld.saturation(20, 0)
                    _same(ld.top(100, 100), first)                      # after them, and twice in a row
                    _same(ld.top(100, 100), first)
                finally:
                    ld.close()
    finally:
        tb.free()


def test_fewer_groups_than_asked(sc):
    """three groups in a tile of 300 wells: the list ends at three whatever n_top, the rest is zeroed"""
    n, cycles = 300, 20
    rng = np.random.default_rng(3)
    reads = rng.integers(1, 256, (n, cycles)).astype(np.uint8)
    reads[[10, 200, 250]] = reads[5]
    reads[[7, 100]] = reads[150]
    reads[299] = reads[298]
    filt = np.ones(n, dtype=np.uint8)
    tiles = _host_tiles([reads], [filt], [1])
    eq_lane, _, labels = lane_dups(tiles, n, 2)
    tb = _upload(sc, [reads], [filt])
    ld = _lane(sc, tb, [1], 2, [[0]])
    try:
        rows = _finish(ld, 0)
        for t, cap in ((1, 1), (2, 2), (3, 3), (4, 4), (1024, 0), (1024, 1024)):
            want = lane_top(labels, tiles, n, 2, t)
            got = ld.top(t, cap)
            _same(got, want)
            check_top_identities(*got, n=n, n_top=t, finish_lane=rows[0], equality=True, cycles=cycles)
        assert got[2].tolist() == [n + 5, n + 7, n + 298] and got[3].tolist() == [4, 3, 2] and got[0].tolist() == [n, 3, 3, 9]
        res = _raw(sc, ld, 1024, 0, 0, 0, cycles=cycles, max_tiles=2, alloc=True)
        assert res[0] == _lib.OK and all((a[3:] == 0).all() for a in res[3:])     # entries past Listed are zeroed
    finally:
        ld.close()
        tb.free()


# ---- 2, 3: one molecule, two molecules --------------------------------------------------------------
BIG_ROWS, BIG_COLS = 90, 100                                           # 9000 wells: a run of 8192 and a bit


@pytest.mark.parametrize("split", [0, 6700])
def test_a_lane_of_one_or_two_molecules(sc, split):
    n, cycles = BIG_ROWS * BIG_COLS, 20
    a = np.array([0x42 + (c % 4) for c in range(cycles)], dtype=np.uint8)
    b = np.full(cycles, 0x42, dtype=np.uint8)                          # poly-G
    lane = np.tile(a, (3 * n, 1))
    lane[:split] = b
    reads = [lane[i * n:(i + 1) * n] for i in range(3)]
    rng = np.random.default_rng(27000)
    filts = [(rng.random(n) >= 0.1).astype(np.uint8) for _ in range(3)]
    tiles = _host_tiles(reads, filts, [0, 1, 2])
    eq_lane, _, labels = lane_dups(tiles, n, 3)
    pf = np.flatnonzero(np.concatenate(filts))
    tb = _upload(sc, reads, filts)
    try:
        ld = _lane(sc, tb, [0, 1, 2], 3, [[0, 1, 2]])
        try:
            rows = _finish(ld, 0)
            for t, cap in ((1, 1), (7, 7), (1024, 0)):
                got = ld.top(t, cap)
                _same(got, lane_top(labels, tiles, n, 3, t))
                check_top_identities(*got, n=n, n_top=t, finish_lane=rows[0], equality=True, cycles=cycles)
            head, levels, root, size, exact, tile_count, text = got
            per_tile = np.array([int(f.sum()) for f in filts])
            if not split:                                               # one group of size PF in the last level
                assert head.tolist() == [pf.size, 1, 1, pf.size] and root.tolist() == [pf[0]] and size.tolist() == [pf.size]
                assert levels[0].tolist() == [0] * 15 + [1] and levels[1][15] == pf.size > 10000
                assert (tile_count[0] == per_tile).all() and exact.tolist() == [pf.size] and text == ["GTAC" * 5]
            else:                                                       # the larger first, though its root comes later
                small_size = int((pf < split).sum())
                assert 5000 <= small_size < 10000 <= pf.size - small_size
                assert size.tolist() == [pf.size - small_size, small_size] and root.tolist() == [pf[pf >= split][0], pf[0]]
                assert levels[0].tolist() == [0] * 14 + [1, 1] and text == ["GTAC" * 5, "G" * 20]
                assert tile_count[1].tolist() == [small_size, 0, 0] and (tile_count.sum(axis=0) == per_tile).all()
        finally:
            ld.close()
    finally:
        tb.free()


# ---- 4: only pairs ----------------------------------------------------------------------------------
def test_only_pairs_takes_the_smallest_roots_within_the_stated_passes(sc):
    n, cycles = BIG_ROWS * BIG_COLS, 30
    rng = np.random.default_rng(9000)
    reads = [rng.integers(1, 256, (n, cycles)).astype(np.uint8) for _ in range(2)]
    for r in reads:
        r[1::2] = r[0::2]                                               # every odd well: its left neighbour's read
    filts = [np.ones(n, dtype=np.uint8) for _ in range(2)]
    tiles = _host_tiles(reads, filts, [2, 0])
    eq_lane, _, labels = lane_dups(tiles, n, 3)
    assert eq_lane[1] == n and eq_lane[6] == n                         # n classes, all of size 2
    tb = _upload(sc, reads, filts)
    try:
        ld = _lane(sc, tb, [2, 0], 3, [[0, 1]])
        try:
            rows = _finish(ld, 0)
            got = ld.top(7, 7)
            _same(got, lane_top(labels, tiles, n, 3, 7))
            assert got[2].tolist() == [0, 2, 4, 6, 8, 10, 12] and got[3].tolist() == [2] * 7
            passes = sc.get_option("lane_top_passes")
            assert 1 < passes <= sc.get_option("lane_top_max_passes") == MAX_PASSES      # the ids had to be refined
            check_top_identities(*got, n=n, n_top=7, finish_lane=rows[0], equality=True, cycles=cycles)
            _same(ld.top(7, 0), got)                                    # all 9000 roots fit the default buffer: one pass
            assert sc.get_option("lane_top_passes") == 1
            got = ld.top(1024, 1024)
            _same(got, lane_top(labels, tiles, n, 3, 1024))
            assert got[2].tolist() == list(range(0, 2048, 2))
        finally:
            ld.close()
    finally:
        tb.free()


# ---- 5: no group at all -----------------------------------------------------------------------------
def test_a_lane_without_a_group_lists_nothing(sc):
    n, cycles = 700, 30
    rng = np.random.default_rng(5)
    reads = [rng.integers(1, 256, (n, cycles)).astype(np.uint8) for _ in range(2)]
    filts = [(rng.random(n) >= 0.2).astype(np.uint8) for _ in range(2)]
    tiles = _host_tiles(reads, filts, [0, 1])
    eq_lane, _, labels = lane_dups(tiles, n, 2)
    assert eq_lane[1] == 0
    tb = _upload(sc, reads, filts)
    ld = _lane(sc, tb, [0, 1], 2, [[0, 1]])
    try:
        rows = _finish(ld, 0)
        for t, cap in ((1, 1), (100, 0)):
            got = ld.top(t, cap)
            _same(got, lane_top(labels, tiles, n, 2, t))
            pf = int(sum(f.sum() for f in filts))
            assert got[0].tolist() == [pf, 0, 0, 0] and got[1][0][0] == pf and len(got[2]) == 0 and got[6] == []
            check_top_identities(*got, n=n, n_top=t, finish_lane=rows[0], equality=True)
        res = _raw(sc, ld, 100, 0, 0, 0, cycles=cycles, max_tiles=2, alloc=True)
        assert res[0] == _lib.OK and all((a[:100] == 0).all() and (a[100:] == _ones(a)).all() for a in res[3:])
    finally:
        ld.close()
        tb.free()


# ---- 6: whole-word rows and rows of 16 words --------------------------------------------------------
@pytest.mark.parametrize("cycles", [10, 151])
def test_rows_of_one_and_of_sixteen_words_decode_to_the_reads(sc, cycles):
    n = 500
    rng = np.random.default_rng(cycles)
    reads = np.array([BYTE[c] for c in rng.integers(0, 5, n * cycles)], dtype=np.uint8).reshape(n, cycles)
    for src, copies in ((3, (40, 41, 300, 499)), (77, (78, 400)), (250, (0,))):
        reads[list(copies)] = reads[src]
    filt = np.ones(n, dtype=np.uint8)
    tiles = _host_tiles([reads], [filt], [0])
    eq_lane, _, labels = lane_dups(tiles, n, 1)
    tb = _upload(sc, [reads], [filt])
    ld = _lane(sc, tb, [0], 1, [[0]])
    try:
        rows = _finish(ld, 0)
        got = ld.top(10, 10)
        _same(got, lane_top(labels, tiles, n, 1, 10))
        assert got[3].tolist()[:3] == [5, 3, 2] and got[2].tolist()[:3] == [3, 77, 0]
        assert got[6][0] == "".join("ACGTN"[4 if b == 0 else b & 3] for b in reads[3].tolist()) and "N" in "".join(got[6])
        check_top_identities(*got, n=n, n_top=10, finish_lane=rows[0], equality=True, cycles=cycles)
    finally:
        ld.close()
        tb.free()


# ---- 7: call discipline -----------------------------------------------------------------------------
def _raw(sc, ld, n_top, cap, scratch, scratch_bytes, missing=(), cycles=CYCLES, max_tiles=MAX_TILES, alloc=False):
    """wd_lane_top itself -> (rc, head row, levels, root, size, exact, tile_count, reads), the outputs sized for 1024
    groups and filled with ones beforehand; missing: the outputs passed as null; alloc: with a scratch of its own"""
    out = [np.full(4, -1, dtype=np.int64), np.full((2, LEVELS), -1, dtype=np.int64)] + \
        [np.full(MAX_TOP, 0xFFFFFFFF, dtype=np.uint32) for _ in range(3)] + \
        [np.full((MAX_TOP, max_tiles), 0xFFFFFFFF, dtype=np.uint32), np.full((MAX_TOP, cycles), 0xFF, dtype=np.uint8)]
    ptr = [None if i in missing else a.ctypes.data_as(ctypes.c_void_p) for i, a in enumerate(out)]
    if alloc:
        scratch_bytes = sc.lane_top_scratch_bytes(ld.N, max_tiles, cycles, n_top, cap)
        scratch = sc.malloc(scratch_bytes)
    try:
        rc = sc._lib.wd_lane_top(ld._h, n_top, cap, ctypes.c_void_p(scratch), scratch_bytes, *ptr)
    finally:
        if alloc:
            sc.free(scratch)
    return (rc,) + tuple(out)


def _ones(a):
    return ~a.dtype.type(0)


def _untouched(res):
    return all((a == _ones(a)).all() for a in res[1:])


def test_call_discipline(sc, small):
    k, t, cap = 2, 18, 36
    want = small["want"]
    need = sc.lane_top_scratch_bytes(N, MAX_TILES, CYCLES, t, cap)
    assert need < sc.lane_top_scratch_bytes(N, MAX_TILES, CYCLES, t, 0)
    d_scratch = sc.malloc(need)
    host = np.zeros(need, dtype=np.uint8)
    tb = _upload(sc, small["reads"], small["filts"])
    ld = _lane(sc, tb, INDEX, MAX_TILES, WAYS["2 + 3"])
    try:
        res = _raw(sc, ld, t, cap, d_scratch, need)                    # before any finish
        assert res[0] == _lib.ERR_ARG and _untouched(res)
        with pytest.raises(ValueError):
            ld.top(t, cap)
        with pytest.raises(RuntimeError):                              # a near finish refused over budget is no finish
            ld.finish(hamming=k, pair_budget=3)
        res = _raw(sc, ld, t, cap, d_scratch, need)
        assert res[0] == _lib.ERR_ARG and _untouched(res) and b"finish" in sc._lib.wd_last_error(sc._ctx)
        _finish(ld, k)

        def good():                                                    # after every refusal: the reference's result
            res = _raw(sc, ld, t, cap, d_scratch, need)
            assert res[0] == _lib.OK and all((a[t:] == _ones(a)).all() for a in res[3:])
            w = want[(k, t)]
            _same((res[1], res[2], res[3][:t], res[4][:t], res[5][:t], res[6][:t],
                   [r.tobytes().decode() for r in res[7][:t]]), w)

        good()
        for bad in (dict(n_top=0), dict(n_top=-1), dict(n_top=MAX_TOP + 1), dict(cap=-1), dict(cap=t - 1), dict(cap=1),
                    dict(scratch=0), dict(scratch_bytes=need - 1), dict(scratch_bytes=0), dict(scratch=host.ctypes.data)) + \
                tuple(dict(missing=(i,)) for i in range(7)):
            args = dict(n_top=t, cap=cap, scratch=d_scratch, scratch_bytes=need)
            args.update(bad)
            res = _raw(sc, ld, **args)
            assert res[0] == _lib.ERR_ARG and _untouched(res), bad
            good()
        for kw in (dict(n_top=0), dict(n_top=MAX_TOP + 1), dict(cand_capacity=-1), dict(cand_capacity=t - 1)):
            args = dict(n_top=t, cand_capacity=cap)
            args.update(kw)
            with pytest.raises(ValueError):
                ld.top(**args)
            good()
        # another lane in the same workspace, by equality
        ld.restart()
        with pytest.raises(ValueError):
            ld.top(t, cap)
        ld.add(tb, INDEX)
        _finish(ld, 0)
        _same(ld.top(t, cap), want[(0, t)])
        ld.close()
        with pytest.raises(ValueError):
            ld.top(t, cap)
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


def test_cli_lane_top_block(tmp_path):
    """The run directory of test_gpu_lanesaturation.py's CLI test: tile 1103's files are tile 1101's but for the last
    cycle, which is tile 1102's.  The new block closes the lane's output, equals write_lane_top of the reference's
    counts and is all the flag adds, whatever --tile-batch; with --lane-dups-hamming it is on the clusters; the TSV is
    write_lane_top_tsv of the same counts."""
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
    eq = lane_dups(tiles, n, 4)
    near = lane_near_dups(tiles, n, 4, 2)

    def block(k, n_top, summary):
        final = report.LaneNearCounts.from_rows(near[0], near[1], names) if k else report.LaneDupCounts.from_rows(eq[0], eq[1], names)
        res = lane_top(near[2] if k else eq[2], tiles, n, 4, n_top)
        counts = report.LaneTopCounts.from_rows(*res, n_top, n, names, final, k)
        text, tsv = io.StringIO(), io.StringIO()
        report.write_lane_top(str(lane), counts, verbose=not summary, out=text)
        report.write_lane_top_tsv(str(lane), counts, tsv)
        return text.getvalue(), tsv.getvalue(), counts

    plain = _main(argv)
    want, tsv, counts = block(0, 50, False)
    assert counts.groups2 > 50 and len(counts.root) == 50 and want.count("LaneTop: 1\tRank: ") == 50
    assert any(sum(1 for v in row if v) > 1 for row in counts.tile_count)      # a listed class lies on several tiles
    for batch in ([], ["--tile-batch", "1"], ["--tile-batch", "2"]):
        assert _main(argv + batch) == plain
        out_file = str(tmp_path / "top.tsv")
        assert _main(argv + batch + ["--lane-dups-top", "50", "--lane-dups-top-out", out_file]) == plain + want
        assert open(out_file).read() == tsv                            # the new block is all the flag adds
    # on the clusters, after every other pass of the lane, the summary alone
    others = ["--lane-dups-hamming", "2", "-S", "--lane-dups-mismatches", "--lane-dups-distance", "--lane-dups-saturation"]
    want, tsv, counts = block(2, 7, True)
    got = _main(argv + others + ["--lane-dups-top", "7"])
    assert got == _main(argv + others) + want
    assert "Hamming: 2\t" in want and "Exact: " in want and "not a consensus" in want and want.count("\tRank: ") == 5
    assert any(e < s for e, s in zip(counts.exact, counts.size))
