"""A lane's duplication against its reads' GC content on the GPU (LaneDups.gc, include/welldup_lanegc.h) against the
host reference of tests/lanegc_ref.py on the labels of tests/lanedups_ref.py / lanenear_ref.py - lane row, tile rows
and the histogram equal cell by cell, nothing approximate - however the tiles are fed and whatever hash_bits, and
against the identities the header states."""
import ctypes
import io
import os
import re
import shutil
from contextlib import redirect_stdout

import numpy as np
import pytest

from lanedups_ref import lane_dups
from lanegc_ref import COPY, HIST_COLS, LANE_COLS, ROOT, SINGLE, TILE_COLS, check_gc_identities, lane_gc, wells_of
from lanenear_ref import lane_near_dups
from test_gpu_lanemismatch import INDEX, MAX_TILES, N, RUN, WAYS, _finish, _host_tiles, _lane, _small_lane, _upload
from well_duplicates_amd import _lib
from well_duplicates_amd import count_well_duplicates as cwd
from well_duplicates_amd import report, synth
from well_duplicates_amd.scanner import Scanner

pytestmark = pytest.mark.gpu

BYTE = {"A": 0x40, "C": 0x81, "G": 0xC2, "T": 0x23, "N": 0x00}
with open(os.path.join(_lib.CSRC, "lane_gc.inc")) as _fh:
    WINDOW = int(re.search(r"constexpr int kLgcWindow = (\d+);", _fh.read()).group(1))    # values of g counted in LDS


@pytest.fixture(scope="module")
def sc():
    s = Scanner(0)
    yield s
    s.close()


def _same(got, want):
    for g, w, name in zip(got, want, ("lane row", "tile rows", "hist")):
        assert g.shape == w.shape and (g == w).all(), (name, g[g != w], w[g != w], np.argwhere(g != w)[:8])


def _labels(tiles, n, max_tiles, k):
    """-> (the finish's lane row in lane_dups' columns, its tile rows, labels) of the reference"""
    if k == 0:
        return lane_dups(tiles, n, max_tiles)
    near_lane, near_tiles, labels = lane_near_dups(tiles, n, max_tiles, k)
    return np.concatenate([near_lane[:6], near_lane[7:]]), near_tiles, labels


# ---- 1: the small lane ------------------------------------------------------------------------------
@pytest.mark.parametrize("cycles", [37, 83])         # four words with a partial last one; nine words
@pytest.mark.parametrize("k", [0, 2])
def test_lane_gc_matches_reference_however_the_tiles_are_fed(sc, k, cycles):
    reads, filts = _small_lane(k, cycles)
    tiles = _host_tiles(reads, filts, INDEX)
    fin_lane, fin_tiles, labels = _labels(tiles, N, MAX_TILES, k)
    depths = (0, 1, cycles)
    want = {m: lane_gc(tiles, N, MAX_TILES, labels, m) for m in depths}
    # the ground is covered: every population counted and skipped, over many g; under clusters copies whose g and
    # whose n are not their root's
    ids, g, nn, pop, size, L = wells_of(tiles, N, MAX_TILES, labels)
    flat = labels.reshape(-1).astype(np.int64)
    at = np.full(flat.size, -1, dtype=np.int64)
    at[ids] = np.arange(ids.size)
    copies = np.flatnonzero(pop == COPY)
    root_at = at[flat[ids[copies]]]
    other_g, other_n = int((g[copies] != g[root_at]).sum()), int((nn[copies] != nn[root_at]).sum())
    lane0, hist0 = want[0][0], want[0][2]
    spans = [int((hist0[:, p] > 0).sum()) for p in (SINGLE, ROOT, COPY)]
    print("k %d cycles %d: lane row at max_n 0 %s, distinct g per population %s, copies with another g %d, another n %d"
          % (k, cycles, lane0.tolist(), spans, other_g, other_n))
    if cycles == 37:
        assert (lane0[1:4] - lane0[4:7] >= 300).all() and (lane0[4:7] >= 70).all(), lane0
        assert min(spans) >= 18, spans
        if k == 2:
            assert other_g >= 100 and other_n >= 1, (other_g, other_n)
    else:
        assert (lane0[1:4] - lane0[4:7] > 0).all() and (lane0[4:7] > 0).all() and min(spans) > 0
        if k == 2:
            assert other_g > 0 and other_n > 0
    if k == 0:
        assert other_g == 0 and other_n == 0
    for m in depths:
        check_gc_identities(*want[m], m, fin_lane, fin_tiles, equality=k == 0, wider=want[cycles])
    tb = _upload(sc, reads, filts)
    try:
        for bits in (0, 1):
            for calls in WAYS.values():
                ld = _lane(sc, tb, INDEX, MAX_TILES, calls, hash_bits=bits)
                try:
                    rows = _finish(ld, k, bits)
                    for m in depths:
                        got = ld.gc(m)
                        _same(got, want[m])
                        check_gc_identities(*got, m, *rows, equality=k == 0)
                finally:
                    ld.close()
    finally:
        tb.free()


# ---- 2: row geometry ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cycles", [9, 10, 25, 51, 151])      # rows of 1 (partial), 1 (full), 3, 6 and 16 words
def test_rows_of_every_geometry(sc, cycles):
    """Two tiles of 8449 wells - odd, a run of kLaneRun and a bit, a last trip that ends inside the workgroup - at tile
    indices 1 and 2 of 3: with an odd number of words per row the tiles' first rows lie 4 and 8 bytes (1 word), 12 and
    8 bytes (3 words) past a 16-byte boundary.  Random reads, 0.5 % no-calls, 95 % PF, and 300 originals of the first
    run of the first tile copied once each: 100 into its second, partial run, 100 into the first run of the second
    tile and 100 into its second."""
    n = 8449
    assert RUN < n < 2 * RUN and n % 2 == 1 and (n - RUN) % 256 != 0
    words = (cycles + 9) // 10
    rng = np.random.default_rng(8449 + cycles)
    reads = [rng.integers(1, 256, (n, cycles)).astype(np.uint8) for _ in range(2)]
    for r in reads:
        r[rng.random(r.shape) < 0.005] = 0
    filts = [(rng.random(n) < 0.95).astype(np.uint8) for _ in range(2)]
    src = rng.choice(RUN, 300, replace=False)
    places = [(0, RUN, n), (1, 0, RUN), (1, RUN, n)]                   # (tile, first well, one past the last)
    for p, (t, lo, hi) in enumerate(places):
        dst = lo + rng.choice(hi - lo, 100, replace=False)
        for a, b in zip(src[100 * p:100 * p + 100].tolist(), dst.tolist()):
            reads[t][b] = reads[0][a]
            filts[0][a] = filts[t][b] = 1
    index = [1, 2]
    tiles = _host_tiles(reads, filts, index)
    fin_lane, fin_tiles, labels = lane_dups(tiles, n, 3)
    if words % 2:                                                      # the tiles' first rows off a 16-byte boundary
        assert (n * words * 4) % 16 != 0 and (2 * n * words * 4) % 16 != 0
    want = {m: lane_gc(tiles, n, 3, labels, m) for m in (0, 2, cycles)}
    assert want[0][0][3] >= 300 and want[0][0][2] >= 250 and (want[0][1][1:, 3] > 0).all()
    assert (want[0][0][4:7] > 0).all() or cycles < 25                  # (a read of nine cycles rarely has a no-call)
    assert not want[0][1][0].any()
    for m in (0, 2):
        check_gc_identities(*want[m], m, fin_lane, fin_tiles, equality=True, wider=want[cycles])
    tb = _upload(sc, reads, filts)
    ld = _lane(sc, tb, index, 3, [[0, 1]])
    try:
        rows = _finish(ld, 0)
        for m in (0, 2):
            got = ld.gc(m)
            _same(got, want[m])
            check_gc_identities(*got, m, *rows, equality=True)
    finally:
        ld.close()
        tb.free()


# ---- 3: extremes --------------------------------------------------------------------------------------
@pytest.mark.parametrize("cycles", [1024, 11])       # 103 words, g beyond the LDS window; two words
def test_reads_at_the_ends_of_the_histogram(sc, cycles):
    """One tile of 300 wells.  Planted: all G three times (g = L), all A, all T twice, all N twice, reads with exactly
    1, 5 and 6 no-calls and L - 1 (max_n and max_n + 1 for max_n = 0 and 5; all N is max_n = L), a read whose only C
    is the last cycle and one whose only G is cycle 0."""
    n = 300
    rng = np.random.default_rng(cycles)
    reads = [rng.integers(1, 256, (n, cycles)).astype(np.uint8)]
    r = reads[0]
    for w in (0, 7, 299):
        r[w] = BYTE["G"]
    r[1] = BYTE["A"]
    r[2] = r[150] = BYTE["T"]
    r[3] = r[298] = BYTE["N"]
    for w, count in ((10, 1), (11, 5), (12, 6), (13, cycles - 1)):
        r[w] = BYTE["A"]
        r[w, rng.choice(cycles, count, replace=False)] = 0
    r[20] = BYTE["A"]
    r[20, cycles - 1] = BYTE["C"]
    r[21] = BYTE["T"]
    r[21, 0] = BYTE["G"]
    filts = [np.ones(n, dtype=np.uint8)]
    filts[0][100:110] = 0
    tiles = _host_tiles(reads, filts, [0])
    fin_lane, fin_tiles, labels = lane_dups(tiles, n, 1)
    depths = (0, 5, cycles)
    want = {m: lane_gc(tiles, n, 1, labels, m) for m in depths}
    for m in depths:
        hist = want[m][2]
        assert hist[cycles, 1:].tolist() == [1, 2, 3]                  # the top bin: all G, a root and two copies
        assert hist[cycles, 0] == 0 or cycles == 11                    # (of 300 random reads of 11 cycles one may be all C and G)
        assert hist[1, 0] >= 2                                         # the lone C at the last cycle, the lone G at the first
        check_gc_identities(*want[m], m, fin_lane, fin_tiles, equality=True, wider=want[cycles])
    if cycles > WINDOW:
        assert want[0][2][WINDOW:].sum() == 6 and want[0][2][:WINDOW].sum() > 200
    # bin 0: all A single, all T a pair; then the reads of A with no-calls as max_n lets them in; all N at max_n = L
    extra = int(want[0][2][0, 0]) - 1                                  # (random reads of 11 cycles without C or G)
    assert extra == 0 or cycles == 11
    assert want[0][2][0].tolist() == [1 + extra, 1, 1, 2] and want[0][0][4:].tolist()[1:] == [1, 1, 2]
    assert want[5][2][0].tolist() == [3 + extra, 1, 1, 2] and want[cycles][2][0].tolist() == [5 + extra, 2, 2, 4]
    assert want[5][0][5:].tolist() == [1, 1, 2] and not want[cycles][0][4:].any()
    assert want[0][0][4] > want[5][0][4] >= 2
    tb = _upload(sc, reads, filts)
    ld = _lane(sc, tb, [0], 1, [[0]])
    try:
        rows = _finish(ld, 0)
        for m in depths:
            got = ld.gc(m)
            _same(got, want[m])
            check_gc_identities(*got, m, *rows, equality=True)
    finally:
        ld.close()
        tb.free()


# ---- 4: degenerate lanes ------------------------------------------------------------------------------
def test_a_lane_of_equal_reads_is_one_bin(sc):
    n, cycles = 9000, 40
    read = np.array([BYTE["ACGT"[c % 4]] for c in range(cycles)], dtype=np.uint8)
    read[:6] = BYTE["G"]                                               # g = 3 + 17 + 3 = 23: G at 0..5, then C, G of ACGT
    g = int(np.isin(read, [BYTE["C"], BYTE["G"]]).sum())
    reads = [np.tile(read, (n, 1)) for _ in range(3)]
    filts = [np.ones(n, dtype=np.uint8) for _ in range(3)]
    for f in filts:
        f[::9] = 2                                                     # (only bit 0 counts: every ninth well fails)
    pf = 3 * int((filts[0] & 1).sum())
    tiles = _host_tiles(reads, filts, [0, 1, 2])
    fin_lane, fin_tiles, labels = lane_dups(tiles, n, 3)
    want = lane_gc(tiles, n, 3, labels, 0)
    hist = np.zeros((cycles + 1, HIST_COLS), dtype=np.int64)
    hist[g] = [0, 1, pf - 1, pf]
    assert 0 < g < cycles and want[0].tolist() == [pf, 0, 1, pf - 1, 0, 0, 0, 0] and (want[2] == hist).all()
    assert (want[1][:, 2] == g * want[1][:, 1]).all() and (want[1][:, 4] == g * want[1][:, 3]).all()      # every tile's mean = g
    check_gc_identities(*want, 0, fin_lane, fin_tiles, equality=True)
    tb = _upload(sc, reads, filts)
    try:
        for k in (0, 1):
            ld = _lane(sc, tb, [0, 1, 2], 3, [[0, 1, 2]])
            try:
                rows = _finish(ld, k)
                for m in (0, cycles):
                    got = ld.gc(m)
                    _same(got, want)
                    check_gc_identities(*got, m, *rows, equality=True)
            finally:
                ld.close()
    finally:
        tb.free()


def test_a_lane_without_a_group(sc):
    n, cycles = 2000, 30
    rng = np.random.default_rng(30)
    reads = [rng.integers(1, 256, (n, cycles)).astype(np.uint8) for _ in range(2)]
    reads[1][rng.random(reads[1].shape) < 0.01] = 0
    filts = [(rng.random(n) < 0.9).astype(np.uint8) for _ in range(2)]
    tiles = _host_tiles(reads, filts, [1, 0])
    fin_lane, fin_tiles, labels = lane_dups(tiles, n, 2)
    want = lane_gc(tiles, n, 2, labels, 0)
    assert fin_lane[1] == 0 and want[0][2] == want[0][3] == 0 and not want[2][:, 1:].any() and want[0][4] > 100
    assert want[0][0] == want[0][1] > 3000 and want[2][:, 0].sum() == want[0][1] - want[0][4]
    tb = _upload(sc, reads, filts)
    ld = _lane(sc, tb, [1, 0], 2, [[0], [1]])
    try:
        rows = _finish(ld, 0)
        got = ld.gc(0)
        _same(got, want)
        check_gc_identities(*got, 0, *rows, equality=True)
    finally:
        ld.close()
        tb.free()


# ---- 5: call discipline -----------------------------------------------------------------------------
def _raw(sc, ld, max_n, scratch, scratch_bytes, missing=None):
    """wd_lane_gc itself -> (rc, lane row, tile rows, hist); missing: the output pointer passed as null"""
    out = [np.full(LANE_COLS, -1, dtype=np.int64), np.full((ld.max_tiles, TILE_COLS), -1, dtype=np.int64),
           np.full((ld.L + 1, HIST_COLS), -1, dtype=np.int64)]
    ptr = [None if i == missing else a.ctypes.data_as(ctypes.c_void_p) for i, a in enumerate(out)]
    rc = sc._lib.wd_lane_gc(ld._h, max_n, ctypes.c_void_p(scratch), scratch_bytes, *ptr)
    return (rc,) + tuple(out)


def _untouched(res):
    return all((a == -1).all() for a in res[1:])


def test_call_discipline(sc):
    k, cycles, m = 2, 37, 1
    reads, filts = _small_lane(k, cycles)
    tiles = _host_tiles(reads, filts, INDEX)
    want = lane_gc(tiles, N, MAX_TILES, lane_near_dups(tiles, N, MAX_TILES, k)[2], m)
    eq_lane, eq_tiles, eq_labels = lane_dups(tiles, N, MAX_TILES)
    want_eq = lane_gc(tiles, N, MAX_TILES, eq_labels, m)
    need = sc.lane_gc_scratch_bytes(MAX_TILES, cycles)
    d_scratch = sc.malloc(need)
    host = np.zeros(need, dtype=np.uint8)
    tb = _upload(sc, reads, filts)
    x, y = synth.honeycomb_pixels(44, 60)
    ld = _lane(sc, tb, INDEX, MAX_TILES, WAYS["2 + 3"])
    try:
        res = _raw(sc, ld, m, d_scratch, need)                         # before any finish
        assert res[0] == _lib.ERR_ARG and _untouched(res)
        assert b"lane gc comes after a successful finish of the lane" in sc._lib.wd_last_error(sc._ctx)
        with pytest.raises(ValueError):
            ld.gc(m)
        with pytest.raises(RuntimeError):                              # a near finish refused over budget is no finish
            ld.finish(hamming=k, pair_budget=3)
        res = _raw(sc, ld, m, d_scratch, need)
        assert res[0] == _lib.ERR_ARG and _untouched(res) and b"finish" in sc._lib.wd_last_error(sc._ctx)
        rows = _finish(ld, k)
        for bad in ((-1, d_scratch, need), (cycles + 1, d_scratch, need), (m, 0, need), (m, d_scratch, need - 1),
                    (m, d_scratch, 0), (m, host.ctypes.data, need)):
            res = _raw(sc, ld, *bad)
            assert res[0] == _lib.ERR_ARG and _untouched(res), bad
        for missing in range(3):
            res = _raw(sc, ld, m, d_scratch, need, missing=missing)
            assert res[0] == _lib.ERR_ARG and _untouched(res)
        for bad in (-1, cycles + 1):
            with pytest.raises(ValueError):
                ld.gc(bad)
        first = _raw(sc, ld, m, d_scratch, need)                       # the caller's scratch, dirty from nothing
        assert first[0] == _lib.OK
        _same(first[1:], want)
        _same(_raw(sc, ld, m, d_scratch, need)[1:], want)              # twice in a row, on the scratch the first call left
        _same(ld.gc(m), want)
        before = ld.mismatches(k), ld.top(20), ld.distances(x, y, 100)
        _same(ld.gc(m), want)                                          # after mismatches, top and distances
        again = ld.mismatches(k), ld.top(20), ld.distances(x, y, 100)  # which find the accumulator as they left it
        for a, b in zip(before, again):
            assert all(np.array_equal(u, v) for u, v in zip(a, b))
        check_gc_identities(*ld.gc(m), m, *rows)
        # another lane in the same workspace, by equality; and one without a tile: zeros
        ld.restart()
        with pytest.raises(ValueError):
            ld.gc(m)
        for slots in WAYS["descending indices"]:
            ld.add_tables([INDEX[s] for s in slots], _tables_of(tb, slots))
        rows = _finish(ld, 0)
        got = ld.gc(m)
        _same(got, want_eq)
        check_gc_identities(*got, m, *rows, equality=True)
        ld.restart()
        _finish(ld, 0)
        res = _raw(sc, ld, 0, d_scratch, need)
        assert res[0] == _lib.OK and not any(a.any() for a in res[1:])
        ld.close()
        with pytest.raises(ValueError):
            ld.gc(m)
    finally:
        ld.close()
        tb.free()
        sc.free(d_scratch)


def _tables_of(tb, slots):
    ptrs = tb.plane_ptrs()
    return Scanner._tables([ptrs[s] for s in slots], [tb.filter_ptr(s) for s in slots], tb.L)


# ---- 6: the CLI -------------------------------------------------------------------------------------
def _main(argv):
    out = io.StringIO()
    with redirect_stdout(out):
        assert cwd.main(argv) == 0
    return out.getvalue()


def test_cli_lane_gc_block(tmp_path):
    """The run directory of test_gpu_lanetop.py's CLI test: tile 1103's files are tile 1101's but for the last cycle,
    which is tile 1102's.  The new block closes the lane's output, equals write_lane_gc of the reference's counts and
    is all the flag adds, also under another --tile-batch; with --lane-dups-hamming it is on the clusters; the TSV is
    write_lane_gc_tsv of the same counts."""
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
    labels = {0: lane_dups(tiles, n, 4)[2], 2: lane_near_dups(tiles, n, 4, 2)[2]}

    def block(k, max_n, bins, summary):
        counts = report.LaneGCCounts.from_rows(*lane_gc(tiles, n, 4, labels[k], max_n), names, max_n, bins, k)
        text, tsv = io.StringIO(), io.StringIO()
        report.write_lane_gc(str(lane), counts, verbose=not summary, out=text)
        report.write_lane_gc_tsv(str(lane), counts, tsv)
        return text.getvalue(), tsv.getvalue(), counts

    plain = _main(argv)
    want, tsv, counts = block(0, 0, 20, False)
    assert counts.copies > 500 and counts.roots > 500 and counts.skipped > 0 and want.count("LaneGC: 1\tBin: ") == 20
    assert want.count("LaneGCTile: 1\t") == 4 and "LaneGCSummary: 1\tMaxN: 0\tCycles: 24\tBins: 20\t" in want
    out_file = str(tmp_path / "gc.tsv")
    got = _main(argv + ["--tile-batch", "1", "--lane-dups-gc", "--lane-dups-gc-out", out_file])
    assert got == plain + want                                         # the new block is all the flag adds
    assert "".join(line for line in got.splitlines(True) if not line.startswith("LaneGC")).rstrip("\n") == plain.rstrip("\n")
    assert open(out_file).read() == tsv
    # on the clusters, after every other pass of the lane, the summary alone, other bins and max_n
    others = ["--lane-dups-hamming", "2", "-S", "--lane-dups-mismatches", "--lane-dups-distance", "--lane-dups-top", "5"]
    want, tsv, counts = block(2, 3, 7, True)
    out_file = str(tmp_path / "gc2.tsv")
    got = _main(argv + others + ["--lane-dups-gc", "--lane-dups-gc-bins", "7", "--lane-dups-gc-max-n", "3",
                                 "--lane-dups-gc-out", out_file])
    assert got == _main(argv + others) + want and open(out_file).read() == tsv
    assert want.count("\tHamming: 2\t") == 8 and "LaneGCTile" not in want and "\tMaxN: 3\tCycles: 24\tBins: 7\t" in want
