"""Where a lane's duplicate copies differ on the GPU (LaneDups.mismatches, include/welldup_lanemismatch.h) against
the host reference of tests/lanemismatch_ref.py on the labels of tests/lanenear_ref.py / lanedups_ref.py - lane row,
tile rows and the substitution table equal, nothing approximate - however the tiles are fed and whatever hash_bits,
and against the identities the header states."""
import ctypes
import io
import os
import re
import shutil
from contextlib import redirect_stdout

import numpy as np
import pytest

from lanedups_ref import lane_dups
from lanemismatch_ref import LANE_COLS, check_mismatch_identities, lane_mismatches
from lanenear_ref import lane_near_dups
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
BYTE = {0: 0x40, 1: 0x81, 2: 0xC2, 3: 0x23, 4: 0x00}                  # a byte of every code A C G T N

with open(os.path.join(_lib.CSRC, "lane_mismatch.inc")) as _fh:
    WINDOW = int(re.search(r"constexpr int kLmWindow = (\d+);", _fh.read()).group(1))      # cycles counted in LDS
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


def _lane(sc, tb, index, max_tiles, calls, hash_bits=0):
    ld = LaneDups(sc, tb.N, max_tiles, tb.L, hash_bits=hash_bits)
    try:
        for slots in calls:
            ld.add_tables([index[s] for s in slots], _tables(tb, slots))
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
    for g, w, name in zip(got, want, ("lane row", "tile rows", "sub")):
        assert g.shape == w.shape and (g == w).all(), (name, g[g != w], w[g != w], np.argwhere(g != w)[:8])


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


def _small_lane(k, cycles):
    """The lane of test_gpu_lanenear.py at `cycles` cycles: five synthetic tiles (copies planted inside every tile,
    one tile dead) and near copies at 1 .. k + 1 mismatches planted within tiles and across tiles (chains: a copy
    of a copy)."""
    spec = synth.SynthSpec(seed=91, n_clusters=N, row=COLS, plant_per_64k=8000, nocall_per_64k=400, dead_tiles=(1102,),
                           plant_far=True, filter_noise=True)
    reads = [np.stack([synth.plane_bytes(spec, ln, t, c) for c in range(cycles)], axis=1) for ln, t in TILES]
    filts = [synth.filter_bytes(spec, ln, t) for ln, t in TILES]
    rng = np.random.default_rng(17 + k)
    for src, dst, count in ((0, 2, 300), (2, 3, 200), (0, 4, 150), (3, 4, 100), (0, 1, 50), (0, 0, 120), (3, 3, 120)):
        _plant(reads, rng, src, dst, count, k + 1)
    _plant(reads, rng, 2, 4, 80, 0)                                    # and equal reads across tiles
    return reads, filts


# ---- 1: the lane of test_gpu_lanenear.py ----------------------------------------------------------
@pytest.mark.parametrize("cycles", [37, 83])         # a partial last word in 16-byte pieces; nine words: past the eight-word piece
@pytest.mark.parametrize("k", [1, 2, 3])
def test_lane_mismatches_match_reference_however_the_tiles_are_fed(sc, k, cycles):
    reads, filts = _small_lane(k, cycles)
    tiles = _host_tiles(reads, filts, INDEX)
    near_lane, near_tiles, labels = lane_near_dups(tiles, N, MAX_TILES, k)
    depths = (0, k, 7)
    want = {d: lane_mismatches(tiles, N, MAX_TILES, labels, d) for d in depths}
    # the ground is covered: every distance up to K + 1, a pair beyond max_d, N in a counted mismatch, roots elsewhere
    lane = want[k][0]
    assert (lane[4:4 + k + 2] > 0).all(), lane
    assert want[0][0][1] < lane[1] < lane[0] and lane[3] > 0 and want[7][0][3] >= lane[3]
    flat = labels.reshape(-1)
    member = np.flatnonzero((flat != 0xFFFFFFFF) & (flat != np.arange(flat.size)))
    assert int((flat[member] // N != member // N).sum()) > 100
    for d in depths:
        check_mismatch_identities(*want[d], d, near_lane, near_tiles)
    assert (want[0][2] <= want[k][2]).all() and (want[k][2] <= want[7][2]).all()
    tb = _upload(sc, reads, filts)
    try:
        for bits in (0, 4, 1):
            for calls in WAYS.values():
                ld = _lane(sc, tb, INDEX, MAX_TILES, calls, hash_bits=bits)
                try:
                    rows = _finish(ld, k, bits)
                    for d in depths:
                        got = ld.mismatches(d)
                        _same(got, want[d])
                        check_mismatch_identities(*got, d, *rows)
                finally:
                    ld.close()
    finally:
        tb.free()


# ---- 1b: pairs across runs and tiles -----------------------------------------------------------------
def test_pairs_that_cross_a_run_or_a_tile(sc):
    """2 tiles of 90 x 100 wells - a run of kLaneRun and a bit -, 20 cycles, random reads, K = 2, max_d = 2.  300
    originals in the first run of tile 0, each copied once at 0, 1 or 2 mismatches: 100 copies into the second,
    partial run of tile 0, 100 into the first run of tile 1 and 100 into its second.  So a root sits in the first run
    of tile 0 and its member in one of the other three places - at least one pair in each, held to below on the
    reference's labels -: every pair crosses a run or a tile, and k_lm_tally takes a second run."""
    n, cycles, k = 90 * 100, 20, 2
    assert RUN < n < 2 * RUN
    rng = np.random.default_rng(9000)
    reads = [rng.integers(1, 256, (n, cycles)).astype(np.uint8) for _ in range(2)]
    for r in reads:
        r[rng.random(r.shape) < 0.005] = 0
    filts = [(rng.random(n) < 0.95).astype(np.uint8) for _ in range(2)]
    src = rng.choice(RUN, 300, replace=False)
    places = [(0, RUN, n), (1, 0, RUN), (1, RUN, n)]                   # (tile, first well, one past the last)
    for p, (t, lo, hi) in enumerate(places):
        dst = lo + rng.choice(hi - lo, 100, replace=False)
        for i, (a, b) in enumerate(zip(src[100 * p:100 * p + 100].tolist(), dst.tolist())):
            reads[t][b] = reads[0][a]
            for c in rng.choice(cycles, i % 3, replace=False).tolist():
                reads[t][b, c] = _other_base(reads[t][b, c])
            filts[0][a] = filts[t][b] = 1
    tiles = _host_tiles(reads, filts, [0, 1])
    near_lane, near_tiles, labels = lane_near_dups(tiles, n, 2, k)
    want = lane_mismatches(tiles, n, 2, labels, k)
    flat = labels.reshape(-1)
    member = np.flatnonzero((flat != 0xFFFFFFFF) & (flat != np.arange(flat.size)))
    assert member.size >= 300 and (flat[member] < RUN).all()           # every root in the first run of tile 0
    for t, lo, hi in places:                                           # and members in each of the other three places
        assert int(((member >= t * n + lo) & (member < t * n + hi)).sum()) >= 100, (t, lo)
    assert (want[0][4:7] >= 90).all() and want[0][0] == member.size
    check_mismatch_identities(*want, k, near_lane, near_tiles)
    tb = _upload(sc, reads, filts)
    ld = _lane(sc, tb, [0, 1], 2, [[0, 1]])
    try:
        rows = _finish(ld, k)
        got = ld.mismatches(k)
        _same(got, want)
        check_mismatch_identities(*got, k, *rows)
    finally:
        ld.close()
        tb.free()


# ---- 2: every ordered substitution at every awkward position --------------------------------------
@pytest.mark.parametrize("cycles", [37, 80])         # four words with a partial last one; eight full ones, one 16-byte piece pair
def test_every_ordered_substitution_at_every_awkward_position(sc, cycles):
    """Wells 0..4 hold the five reads of one code throughout (A.., C.., G.., T.., N..: every cycle apart, so they
    never link); then, for every position and every ordered pair (a, b), a copy of read a with that cycle changed
    to b: 7 x 20 pairs at distance 1, each of them alone in its entry of Sub."""
    positions = [0, 9, 10, 19, 29, 30, cycles - 1]
    rows = [[BYTE[a]] * cycles for a in range(5)]
    for c in positions:
        for a in range(5):
            for b in range(5):
                if a != b:
                    r = [BYTE[a]] * cycles
                    r[c] = BYTE[b]
                    rows.append(r)
    rows += [[BYTE[(w + c) % 4] for c in range(cycles)] for w in range(11)]       # and wells that are not PF
    reads = [np.array(rows, dtype=np.uint8)]
    filt = np.ones(len(rows), dtype=np.uint8)
    filt[-11:] = 0
    want_sub = np.zeros((cycles, 5, 5), dtype=np.int64)
    for c in positions:                                                # the expected entries: one each, nothing else
        for a in range(5):
            for b in range(5):
                want_sub[c, a, b] = int(a != b)
    pairs = 20 * len(positions)
    want_lane = [pairs, pairs, pairs, 8 * len(positions), 0, pairs] + [0] * 7
    tiles = _host_tiles(reads, [filt], [1])
    ref = lane_mismatches(tiles, len(rows), 2, lane_near_dups(tiles, len(rows), 2, 1)[2], 1)
    assert ref[0].tolist() == want_lane and (ref[2] == want_sub).all()
    tb = _upload(sc, reads, [filt])
    ld = _lane(sc, tb, [1], 2, [[0]])
    try:
        rows_ = _finish(ld, 1)
        for d in (1, 7):
            lane, trow, sub = ld.mismatches(d)
            assert lane.tolist() == want_lane and (sub == want_sub).all()
            assert trow.tolist() == [[0] * 4, want_lane[:4]]
            check_mismatch_identities(lane, trow, sub, d, *rows_)
        lane, trow, sub = ld.mismatches(0)
        assert lane.tolist() == [pairs, 0, 0, 0, 0, pairs] + [0] * 7 and not sub.any()
    finally:
        ld.close()
        tb.free()


# ---- 3: the interface's largest read --------------------------------------------------------------
def test_1024_cycles_on_both_sides_of_the_lds_window(sc):
    """3 tiles of 601 wells, 1024 cycles, K = 2.  Copies with one cycle changed at 0, at 1023 and on both sides of
    the last cycle the kernel counts in LDS (kLmWindow of csrc/lane_mismatch.inc), copies with two - one on each
    side, and both beyond -, and copies at three cycles that only a chain links."""
    cycles, n, k = 1024, 601, 2
    assert 10 < WINDOW < cycles - 10
    rng = np.random.default_rng(1024)
    reads = [rng.integers(1, 256, (n, cycles)).astype(np.uint8) for _ in range(3)]
    for r in reads:
        r[rng.random(r.shape) < 0.005] = 0
    cuts = [[0], [cycles - 1], [WINDOW - 1], [WINDOW], [WINDOW - 1, WINDOW], [WINDOW + 1, cycles - 1], [0, WINDOW - 2],
            [WINDOW - 10], [WINDOW + 9]]
    for i in range(180):                                               # tile 0's wells 0..179 copied to tiles 1 and 2
        cut = cuts[i % len(cuts)]
        reads[1][300 + i] = reads[0][i]
        for c in cut:
            reads[1][300 + i, c] = _other_base(reads[1][300 + i, c])
        if i % 2:                                                      # a chain: a copy of tile 1's copy, two further on
            reads[2][300 + i] = reads[1][300 + i]
            for c in (5, WINDOW + 5):
                reads[2][300 + i, c] = _other_base(reads[2][300 + i, c])
        else:                                                          # N there, or C where the read has N
            reads[2][300 + i] = reads[0][i]
            reads[2][300 + i, cut[0]] = 0 if reads[2][300 + i, cut[0]] else 0x41
    filts = [(rng.random(n) < 0.95).astype(np.uint8) for _ in range(3)]
    for f in filts:
        f[:180] = 1
        f[300:480] = 1
    index = [0, 2, 1]                                                  # the originals have the smallest ids
    tiles = _host_tiles(reads, filts, index)
    near_lane, near_tiles, labels = lane_near_dups(tiles, n, 3, k)
    want = {d: lane_mismatches(tiles, n, 3, labels, d) for d in (0, 1, 2, 7)}
    lane, sub = want[7][0], want[7][2]
    assert lane[0] >= 360 and lane[3] > 50 and (lane[5:8] > 0).all()
    assert sub[0].sum() > 0 and sub[cycles - 1].sum() > 0 and sub[WINDOW - 1].sum() > 0 and sub[WINDOW].sum() > 0
    assert want[2][0][1] < want[7][0][1]                               # a pair the chain carried beyond K
    tb = _upload(sc, reads, filts)
    ld = _lane(sc, tb, index, 3, [[0, 1], [2]])
    try:
        rows = _finish(ld, k)
        for d in (0, 1, 2, 7):
            got = ld.mismatches(d)
            _same(got, want[d])
            check_mismatch_identities(*got, d, *rows)
    finally:
        ld.close()
        tb.free()


# ---- 4: contention ----------------------------------------------------------------------------------
def test_a_tile_of_equal_reads_is_one_bin(sc):
    cycles = 40
    reads = [np.tile(np.array([0x42 + (c % 4) for c in range(cycles)], dtype=np.uint8), (N, 1))]
    filt = np.ones(N, dtype=np.uint8)
    filt[::9] = 2                                                      # (only bit 0 counts: every ninth well fails)
    pf = int((filt & 1).sum())
    assert pf == N - (N + 8) // 9 and 2000 < pf < N
    tb = _upload(sc, reads, [filt])
    try:
        for k in (0, 1):
            ld = _lane(sc, tb, [0], 1, [[0]])
            try:
                _finish(ld, k)
                lane, trow, sub = ld.mismatches(3)
                assert lane.tolist() == [pf - 1, pf - 1, 0, 0, pf - 1] + [0] * 8
                assert trow.tolist() == [[pf - 1, pf - 1, 0, 0]] and not sub.any()
            finally:
                ld.close()
    finally:
        tb.free()


def test_2000_copies_changed_alike_fill_one_entry(sc):
    cycles, at = 40, 23
    rng = np.random.default_rng(2000)
    reads = [rng.integers(1, 256, (N, cycles)).astype(np.uint8)]
    reads[0][0, at] = BYTE[2]                                          # the original has G there, every copy T
    reads[0][1:2001] = reads[0][0]
    reads[0][1:2001, at] = BYTE[3]
    filt = np.ones(N, dtype=np.uint8)
    want_sub = np.zeros((cycles, 5, 5), dtype=np.int64)
    want_sub[at, 2, 3] = 2000
    tb = _upload(sc, reads, [filt])
    ld = _lane(sc, tb, [0], 1, [[0]])
    try:
        rows = _finish(ld, 1)
        assert rows[0][3] == 2000
        lane, trow, sub = ld.mismatches(1)
        assert lane.tolist() == [2000, 2000, 2000, 0, 0, 2000] + [0] * 7
        assert trow.tolist() == [lane[:4].tolist()] and (sub == want_sub).all()
    finally:
        ld.close()
        tb.free()


# ---- 5: call discipline -----------------------------------------------------------------------------
def _raw(sc, ld, max_d, scratch, scratch_bytes, missing=None):
    """wd_lane_mismatches itself -> (rc, lane row, tile rows, sub); missing: the output pointer passed as null"""
    out = [np.full(LANE_COLS, -1, dtype=np.int64), np.full((ld.max_tiles, 4), -1, dtype=np.int64),
           np.full((ld.L, 5, 5), -1, dtype=np.int64)]
    ptr = [None if i == missing else a.ctypes.data_as(ctypes.c_void_p) for i, a in enumerate(out)]
    rc = sc._lib.wd_lane_mismatches(ld._h, max_d, ctypes.c_void_p(scratch), scratch_bytes, *ptr)
    return (rc,) + tuple(out)


def _untouched(res):
    return all((a == -1).all() for a in res[1:])


def test_call_discipline(sc):
    k, cycles = 2, 37
    reads, filts = _small_lane(k, cycles)
    tiles = _host_tiles(reads, filts, INDEX)
    near_lane, near_tiles, labels = lane_near_dups(tiles, N, MAX_TILES, k)
    want = lane_mismatches(tiles, N, MAX_TILES, labels, k)
    eq_lane, eq_tiles, eq_labels = lane_dups(tiles, N, MAX_TILES)
    want_eq = lane_mismatches(tiles, N, MAX_TILES, eq_labels, 7)
    check_mismatch_identities(*want_eq, 7, eq_lane, eq_tiles, equality=True)
    need = sc.lane_mismatch_scratch_bytes(MAX_TILES, cycles)
    d_scratch = sc.malloc(need)
    host = np.zeros(need, dtype=np.uint8)
    tb = _upload(sc, reads, filts)
    idx = TileBatch(sc, len(reads), 8, N)                              # index reads: the first eight cycles, again
    for i, r in enumerate(reads):
        idx.upload_tile(i, [np.ascontiguousarray(r[:, c]) for c in range(8)], filts[i])
    ld = _lane(sc, tb, INDEX, MAX_TILES, WAYS["2 + 3"])
    try:
        ld.index_begin(8)
        ld.index_add(idx, INDEX)
        res = _raw(sc, ld, k, d_scratch, need)                         # before any finish
        assert res[0] == _lib.ERR_ARG and _untouched(res)
        with pytest.raises(ValueError):
            ld.mismatches(k)
        with pytest.raises(RuntimeError):                              # a near finish refused over budget is no finish
            ld.finish(hamming=k, pair_budget=3)
        res = _raw(sc, ld, k, d_scratch, need)
        assert res[0] == _lib.ERR_ARG and _untouched(res) and b"finish" in sc._lib.wd_last_error(sc._ctx)
        rows = _finish(ld, k)
        for bad in ((-1, d_scratch, need), (8, d_scratch, need), (k, 0, need), (k, d_scratch, need - 256), (k, d_scratch, 0),
                    (k, host.ctypes.data, need)):
            res = _raw(sc, ld, *bad)
            assert res[0] == _lib.ERR_ARG and _untouched(res), bad
        for missing in range(3):
            res = _raw(sc, ld, k, d_scratch, need, missing=missing)
            assert res[0] == _lib.ERR_ARG and _untouched(res)
        for d in (-1, 8):
            with pytest.raises(ValueError):
                ld.mismatches(d)
        first = _raw(sc, ld, k, d_scratch, need)                       # the caller's scratch, dirty from nothing
        assert first[0] == _lib.OK
        _same(first[1:], want)
        _same(ld.mismatches(k), want)                                  # twice the same
        before = ld.index_finish(min_pf=1)
        _same(ld.mismatches(k), want)                                  # and after the index finish
        again = ld.index_finish(min_pf=1)                              # which found its tables as it left them
        assert all((a == b).all() for a, b in zip(before, again))
        check_mismatch_identities(*ld.mismatches(k), k, *rows)
        # another lane in the same workspace, by equality: only Dist[0]
        ld.restart()
        with pytest.raises(ValueError):
            ld.mismatches(k)
        for slots in WAYS["descending indices"]:
            ld.add_tables([INDEX[s] for s in slots], _tables(tb, slots))
        ld.index_add(idx, INDEX)
        rows = _finish(ld, 0)
        got = ld.mismatches(7)
        _same(got, want_eq)
        check_mismatch_identities(*got, 7, *rows, equality=True)
        assert got[0][4] == got[0][0] == eq_lane[3] > 0
        ld.close()
        with pytest.raises(ValueError):
            ld.mismatches(k)
    finally:
        ld.close()
        idx.free()
        tb.free()
        sc.free(d_scratch)


# ---- 6: the CLI -------------------------------------------------------------------------------------
def _main(argv):
    out = io.StringIO()
    with redirect_stdout(out):
        assert cwd.main(argv) == 0
    return out.getvalue()


def test_cli_lane_mismatch_block(tmp_path):
    """The run directory of test_gpu_lanenear.py's CLI test: 2 lanes x 4 tiles; in each lane tile 1103's files are
    tile 1101's but for the last cycle, which is tile 1102's.  The new block closes each lane's output, equals
    write_lane_mismatches of the reference, is the same for --tile-batch 1 and the default, and is all the flag adds."""
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
    argv = ["-s", "hiseq_x", "-r", run_dir, "-t", "1101,1102,1103,1104", "-i", "1,2", "-l", str(levels),
            "--cycles", "0-%d" % L, "-q", "--all-wells", "--lane-dups", "--lane-dups-hamming", str(k)]
    blocks = {}
    for lane in (1, 2):
        tiles = [(i, [synth.plane_bytes(spec, lane, int(source(t, c)), c) for c in range(L)],
                  synth.filter_bytes(spec, lane, int(t if t != "1103" else "1101"))) for i, t in enumerate(names)]
        labels = lane_near_dups(tiles, n, 4, k)[2]
        for summary in (False, True):
            for d in (k, 0):
                res = lane_mismatches(tiles, n, 4, labels, d)
                counts = report.LaneMismatchCounts.from_rows(*res, names, k, d, list(range(L)))
                assert counts.dist[1] > 1000 and (d == 0 or counts.sub[L - 1] != [[0] * 5] * 5)
                text = io.StringIO()
                report.write_lane_mismatches(str(lane), counts, verbose=not summary, out=text)
                blocks[(summary, lane, d)] = text.getvalue()
    for summary in (False, True):
        flags = ["-S"] if summary else []
        plain = _main(argv + flags)
        runs = [_main(argv + flags + ["--lane-dups-mismatches", "--tile-batch", "1"]),
                _main(argv + flags + ["--lane-dups-mismatches"])]
        assert runs[0] == runs[1]
        b1, b2 = blocks[(summary, 1, k)], blocks[(summary, 2, k)]
        assert runs[0].count(b1) == 1 and runs[0].endswith(b2)
        assert runs[0].replace(b1, "", 1)[:-len(b2)] == plain          # minus the new blocks: the output without the flag
        assert runs[0].index("LaneNearDupsSummary: 1") < runs[0].index(b1) < runs[0].index("LaneDupsSummary: 2")
        assert ("LaneMismatches: 1\tCycle: %d\t" % (L - 1) in b1) == (not summary)
    with_index = _main(argv + ["-S", "--lane-dups-mismatches", "--lane-dups-mismatches-max-d", "0", "--lane-dups-index", "0-6"])
    b1, b2 = blocks[(True, 1, 0)], blocks[(True, 2, 0)]
    assert with_index.count(b1) == 1 and with_index.endswith(b2)
    assert with_index.index("LaneIndexDupsSummary: 1") < with_index.index(b1) < with_index.index("LaneDupsSummary: 2")
