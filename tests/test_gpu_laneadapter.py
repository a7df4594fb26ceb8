"""A lane's duplication by insert length on the GPU (LaneDups.adapter, include/welldup_laneadapter.h) against the host
reference of tests/laneadapter_ref.py on the labels of tests/lanedups_ref.py / lanenear_ref.py - lane row, tile rows
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

from laneadapter_cases import ADAPTER, INDEX, MAX_TILES, N, PARAMS, bytes_of, check_coverage, small_lane
from laneadapter_ref import HIST_COLS, LANE_COLS, TILE_COLS, check_adapter_identities, codes_of, lane_adapter
from lanedups_ref import lane_dups
from lanenear_ref import lane_near_dups
from test_gpu_lanemismatch import RUN, WAYS, _finish, _host_tiles, _lane, _upload
from well_duplicates_amd import _lib
from well_duplicates_amd import count_well_duplicates as cwd
from well_duplicates_amd import report, synth
from well_duplicates_amd.scanner import Scanner

pytestmark = pytest.mark.gpu

with open(os.path.join(_lib.CSRC, "lane_adapter.inc")) as _fh:
    _SRC = _fh.read()
WINDOW = int(re.search(r"constexpr int kLadWindow = (\d+);", _SRC).group(1))      # values of a counted in LDS
TRUSEQ = ADAPTER[:13]


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
# the three (m, E, O) of the cases, and around the first of them a stricter and a looser one for the monotony
STRICT, LOOSE = (13, 0, 13), (13, 3, 3)


@pytest.mark.parametrize("cycles", [37, 83])         # four words with a partial last one; nine words
@pytest.mark.parametrize("k", [0, 2])
def test_lane_adapter_matches_reference_however_the_tiles_are_fed(sc, k, cycles):
    reads, filts = small_lane(cycles)
    tiles = _host_tiles(reads, filts, INDEX)
    fin_lane, fin_tiles, labels = _labels(tiles, N, MAX_TILES, k)
    check_coverage(tiles, labels, k, cycles)
    every = PARAMS + [STRICT, LOOSE]
    want = {p: lane_adapter(tiles, N, MAX_TILES, labels, ADAPTER[:p[0]], p[1], p[2]) for p in every}
    print("k %d cycles %d: lane rows %s" % (k, cycles, {p: want[p][0].tolist() for p in every}))
    looser = {STRICT: PARAMS[0], PARAMS[0]: LOOSE}
    for p in every:
        check_adapter_identities(*want[p], *p, fin_lane, fin_tiles, equality=k == 0,
                                 looser=want[looser[p]] if p in looser else None)
    tb = _upload(sc, reads, filts)
    try:
        for bits in (0, 1):
            for calls in WAYS.values():
                ld = _lane(sc, tb, INDEX, MAX_TILES, calls, hash_bits=bits)
                try:
                    rows = _finish(ld, k, bits)
                    got = {}
                    for p in every:
                        got[p] = ld.adapter(ADAPTER[:p[0]], p[1], p[2])
                        _same(got[p], want[p])
                    for p in every:
                        check_adapter_identities(*got[p], *p, *rows, equality=k == 0,
                                                 looser=got[looser[p]] if p in looser else None)
                finally:
                    ld.close()
    finally:
        tb.free()


# ---- 2: row geometry ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cycles", [9, 10, 25, 51, 151, 171])   # rows of 1 (partial), 1 (full), 3, 6, 16 and 18 words
def test_rows_of_every_geometry(sc, cycles):
    """Two tiles of 8449 wells - odd, a run of kLaneRun and a bit, a last trip that ends inside the workgroup - at tile
    indices 1 and 2 of 3: with an odd number of words per row the tiles' first rows lie 4 and 8 bytes (1 word), 12 and
    8 bytes (3 words) past a 16-byte boundary; rows of 18 words are walked in sub-trips of fewer wells than a trip.
    Random reads, 0.5 % no-calls, 95 % PF; the adapter planted in the first and the last well of each run, in the last
    well of the first trip and the first of the second, in 300 wells anywhere, and 300 originals of the first run of
    the first tile copied once each into the other three runs."""
    n = 8449
    assert RUN < n < 2 * RUN and n % 2 == 1 and (n - RUN) % 256 != 0
    words = (cycles + 9) // 10
    m, e, o = 13, 1, 8
    rng = np.random.default_rng(8449 + cycles)
    codes = [rng.integers(0, 4, (n, cycles)).astype(np.uint8) for _ in range(2)]
    for c in codes:
        c[rng.random(c.shape) < 0.005] = 4
    filts = [(rng.random(n) < 0.95).astype(np.uint8) for _ in range(2)]
    ends = [0, 255, 256, RUN - 1, RUN, n - 1]
    for t in range(2):
        for i, w in enumerate(ends + rng.choice(n, 150, replace=False).tolist()):
            p = (7 * i + t) % (cycles - o + 1)
            codes[t][w, p:p + m] = TRUSEQ[:min(m, cycles - p)]
            filts[t][w] = 1
    src = rng.choice(RUN, 300, replace=False)
    places = [(0, RUN, n), (1, 0, RUN), (1, RUN, n)]                   # (tile, first well, one past the last)
    for p, (t, lo, hi) in enumerate(places):
        dst = lo + rng.choice(hi - lo, 100, replace=False)
        for a, b in zip(src[100 * p:100 * p + 100].tolist(), dst.tolist()):
            if b not in ends:
                codes[t][b] = codes[0][a]
                filts[0][a] = filts[t][b] = 1
    reads = [bytes_of(c, rng) for c in codes]
    index = [1, 2]
    tiles = _host_tiles(reads, filts, index)
    fin_lane, fin_tiles, labels = lane_dups(tiles, n, 3)
    if words % 2:                                                      # the tiles' first rows off a 16-byte boundary
        assert (n * words * 4) % 16 != 0 and (2 * n * words * 4) % 16 != 0
    if words > 16:
        assert "kLadStage = kTdBlock * 17;" in _SRC                    # a trip of these rows does not fit the block
    want = lane_adapter(tiles, n, 3, labels, TRUSEQ, e, o)
    assert want[0][3] >= 250 and want[0][2] >= 250 and (want[1][1:, 1] >= 100).all() and not want[1][0].any()
    assert int((want[2][:cycles - o + 1, :3].sum(axis=1) > 0).sum()) >= min(cycles - o + 1, 40)
    check_adapter_identities(*want, m, e, o, fin_lane, fin_tiles, equality=True)
    tb = _upload(sc, reads, filts)
    ld = _lane(sc, tb, index, 3, [[0, 1]])
    try:
        rows = _finish(ld, 0)
        got = ld.adapter(TRUSEQ, e, o)
        _same(got, want)
        check_adapter_identities(*got, m, e, o, *rows, equality=True)
    finally:
        ld.close()
        tb.free()


def test_1024_cycles_on_both_sides_of_the_lds_window(sc):
    """One tile of 600 wells at 1024 cycles (103 words: sub-trips of 42 wells): the adapter at positions below and at
    or beyond the LDS window, up to the last, with pairs among them."""
    n, cycles = 600, 1024
    m, e, o = 13, 1, 8
    rng = np.random.default_rng(1024)
    codes = rng.integers(0, 4, (n, cycles)).astype(np.uint8)
    at = {}
    for i, p in enumerate([0, 1, WINDOW - 1, WINDOW, WINDOW + 1, 511, 512, 1000, cycles - m, cycles - o] + rng.choice(cycles - o, 90).tolist()):
        codes[3 * i, :] = 3                                            # (all T before the plant: nothing matches earlier)
        codes[3 * i, p:p + m] = TRUSEQ[:min(m, cycles - p)]
        codes[3 * i, p + m:] = rng.integers(0, 4, max(0, cycles - p - m))
        at[3 * i] = p
        if i % 2:
            codes[3 * i + 1] = codes[3 * i]
    filts = [np.ones(n, dtype=np.uint8)]
    filts[0][500:510] = 0
    reads = [bytes_of(codes, rng)]
    tiles = _host_tiles(reads, filts, [0])
    fin_lane, fin_tiles, labels = lane_dups(tiles, n, 1)
    want = lane_adapter(tiles, n, 1, labels, TRUSEQ, e, o)
    assert want[2][WINDOW:cycles].sum() >= 30 and want[2][:WINDOW].sum() >= 10 and want[2][cycles - o, :3].sum() >= 1
    assert want[0][2] >= 40 and want[0][9] >= 1
    check_adapter_identities(*want, m, e, o, fin_lane, fin_tiles, equality=True)
    tb = _upload(sc, reads, filts)
    ld = _lane(sc, tb, [0], 1, [[0]])
    try:
        rows = _finish(ld, 0)
        got = ld.adapter(TRUSEQ, e, o)
        _same(got, want)
        check_adapter_identities(*got, m, e, o, *rows, equality=True)
    finally:
        ld.close()
        tb.free()


# ---- 3: degenerate lanes ------------------------------------------------------------------------------
def test_a_lane_of_equal_reads_with_the_adapter_is_one_row(sc):
    n, cycles, at = 9000, 40, 17
    m, e, o = 13, 1, 8
    read = np.array([c % 4 for c in range(cycles)], dtype=np.uint8)
    read[at:at + m] = TRUSEQ
    rng = np.random.default_rng(40)
    reads = [bytes_of(np.tile(read, (n, 1)), rng) for _ in range(3)]
    filts = [np.ones(n, dtype=np.uint8) for _ in range(3)]
    for f in filts:
        f[::9] = 2                                                     # (only bit 0 counts: every ninth well fails)
    pf = 3 * int((filts[0] & 1).sum())
    tiles = _host_tiles(reads, filts, [0, 1, 2])
    fin_lane, fin_tiles, labels = lane_dups(tiles, n, 3)
    want = lane_adapter(tiles, n, 3, labels, TRUSEQ, e, o)
    hist = np.zeros((cycles + 1, HIST_COLS), dtype=np.int64)
    hist[at] = [0, 1, pf - 1, pf]
    assert want[0].tolist() == [pf, 0, 1, pf - 1, 0, 1, pf - 1, pf, 0, 0] and (want[2] == hist).all()
    assert (want[1][:, 4] == at * want[1][:, 1]).all() and (want[1][:, 0] == want[1][:, 1]).all()
    check_adapter_identities(*want, m, e, o, fin_lane, fin_tiles, equality=True)
    tb = _upload(sc, reads, filts)
    try:
        for k in (0, 1):
            ld = _lane(sc, tb, [0, 1, 2], 3, [[0, 1, 2]])
            try:
                rows = _finish(ld, k)
                got = ld.adapter(TRUSEQ, e, o)
                _same(got, want)
                check_adapter_identities(*got, m, e, o, *rows, equality=True)
                none = ld.adapter(codes_of("TTTTTTTTTTTT"), 0, 12)     # and without it: row L alone
                assert none[0].tolist() == [pf, 0, 1, pf - 1, 0, 0, 0, 0, 0, 0] and none[2][cycles].tolist() == [0, 1, pf - 1, pf]
                assert not none[2][:cycles].any() and not none[1][:, [1, 3, 4]].any()
            finally:
                ld.close()
    finally:
        tb.free()


# ---- 4: call discipline -----------------------------------------------------------------------------
def _raw(sc, ld, codes, m, e, o, scratch, scratch_bytes, missing=None):
    """wd_lane_adapter itself -> (rc, lane row, tile rows, hist); missing: the output pointer passed as null"""
    out = [np.full(LANE_COLS, -1, dtype=np.int64), np.full((ld.max_tiles, TILE_COLS), -1, dtype=np.int64),
           np.full((ld.L + 1, HIST_COLS), -1, dtype=np.int64)]
    ptr = [None if i == missing else a.ctypes.data_as(ctypes.c_void_p) for i, a in enumerate(out)]
    codes = None if codes is None else np.ascontiguousarray(codes, dtype=np.uint8)
    rc = sc._lib.wd_lane_adapter(ld._h, None if codes is None else codes.ctypes.data_as(ctypes.c_void_p), m, e, o,
                                 ctypes.c_void_p(scratch), scratch_bytes, *ptr)
    return (rc,) + tuple(out)


def _untouched(res):
    return all((a == -1).all() for a in res[1:])


def test_call_discipline(sc):
    k, cycles = 2, 37
    m, e, o = PARAMS[0]
    reads, filts = small_lane(cycles)
    tiles = _host_tiles(reads, filts, INDEX)
    want = lane_adapter(tiles, N, MAX_TILES, lane_near_dups(tiles, N, MAX_TILES, k)[2], TRUSEQ, e, o)
    eq_lane, eq_tiles, eq_labels = lane_dups(tiles, N, MAX_TILES)
    want_eq = lane_adapter(tiles, N, MAX_TILES, eq_labels, TRUSEQ, e, o)
    need = sc.lane_adapter_scratch_bytes(MAX_TILES, cycles)
    d_scratch = sc.malloc(need)
    host = np.zeros(need, dtype=np.uint8)
    tb = _upload(sc, reads, filts)
    x, y = synth.honeycomb_pixels(44, 60)
    ld = _lane(sc, tb, INDEX, MAX_TILES, WAYS["2 + 3"])
    try:
        res = _raw(sc, ld, TRUSEQ, m, e, o, d_scratch, need)           # before any finish
        assert res[0] == _lib.ERR_ARG and _untouched(res)
        assert b"lane adapter comes after a successful finish of the lane" in sc._lib.wd_last_error(sc._ctx)
        with pytest.raises(ValueError):
            ld.adapter(TRUSEQ, e, o)
        with pytest.raises(RuntimeError):                              # a near finish refused over budget is no finish
            ld.finish(hamming=k, pair_budget=3)
        res = _raw(sc, ld, TRUSEQ, m, e, o, d_scratch, need)
        assert res[0] == _lib.ERR_ARG and _untouched(res) and b"finish" in sc._lib.wd_last_error(sc._ctx)
        rows = _finish(ld, k)
        bad_code = TRUSEQ.copy()
        bad_code[12] = 4
        long_one = np.zeros(38, dtype=np.uint8)
        for bad in ((TRUSEQ, 7, e, 7, d_scratch, need), (long_one, 33, e, o, d_scratch, need), (TRUSEQ, m, -1, o, d_scratch, need),
                    (TRUSEQ, m, 4, o, d_scratch, need), (TRUSEQ, m, e, 2, d_scratch, need), (TRUSEQ, m, e, m + 1, d_scratch, need),
                    (long_one, 32, e, 32, d_scratch, need - 1), (long_one, 38 - 6, e, 38, d_scratch, need),
                    (bad_code, m, e, o, d_scratch, need), (None, m, e, o, d_scratch, need), (TRUSEQ, m, e, o, 0, need),
                    (TRUSEQ, m, e, o, d_scratch, need - 1), (TRUSEQ, m, e, o, d_scratch, 0), (TRUSEQ, m, e, o, host.ctypes.data, need)):
            res = _raw(sc, ld, *bad)
            assert res[0] == _lib.ERR_ARG and _untouched(res), bad
        for missing in range(3):
            res = _raw(sc, ld, TRUSEQ, m, e, o, d_scratch, need, missing=missing)
            assert res[0] == _lib.ERR_ARG and _untouched(res)
        for bad in ((TRUSEQ[:7], e, 7), (TRUSEQ, 4, o), (TRUSEQ, e, 2), (TRUSEQ, e, 14), (bad_code, e, o), (long_one[:32], e, 32 + 6)):
            with pytest.raises(ValueError):
                ld.adapter(*bad)
        first = _raw(sc, ld, TRUSEQ, m, e, o, d_scratch, need)         # the caller's scratch, dirty from nothing
        assert first[0] == _lib.OK
        _same(first[1:], want)
        _same(_raw(sc, ld, TRUSEQ, m, e, o, d_scratch, need)[1:], want)        # twice in a row, on the scratch the first call left
        _same(ld.adapter(TRUSEQ, e, o), want)
        before = ld.mismatches(k), ld.top(20), ld.distances(x, y, 100), ld.gc(0)
        _same(ld.adapter(TRUSEQ, e, o), want)                          # after mismatches, top, distances and gc
        again = ld.mismatches(k), ld.top(20), ld.distances(x, y, 100), ld.gc(0)      # which find the accumulator as they left it
        for a, b in zip(before, again):
            assert all(np.array_equal(u, v) for u, v in zip(a, b))
        check_adapter_identities(*ld.adapter(TRUSEQ, e, o), m, e, o, *rows)
        # another lane in the same workspace, by equality; and one without a tile: zeros
        ld.restart()
        with pytest.raises(ValueError):
            ld.adapter(TRUSEQ, e, o)
        for slots in WAYS["descending indices"]:
            ld.add_tables([INDEX[s] for s in slots], _tables_of(tb, slots))
        rows = _finish(ld, 0)
        got = ld.adapter(TRUSEQ, e, o)
        _same(got, want_eq)
        check_adapter_identities(*got, m, e, o, *rows, equality=True)
        ld.restart()
        _finish(ld, 0)
        res = _raw(sc, ld, TRUSEQ, m, e, o, d_scratch, need)
        assert res[0] == _lib.OK and not any(a.any() for a in res[1:])
        ld.close()
        with pytest.raises(ValueError):
            ld.adapter(TRUSEQ, e, o)
    finally:
        ld.close()
        tb.free()
        sc.free(d_scratch)


def _tables_of(tb, slots):
    ptrs = tb.plane_ptrs()
    return Scanner._tables([ptrs[s] for s in slots], [tb.filter_ptr(s) for s in slots], tb.L)


# ---- 5: the CLI -------------------------------------------------------------------------------------
def _main(argv):
    out = io.StringIO()
    with redirect_stdout(out):
        assert cwd.main(argv) == 0
    return out.getvalue()


def test_cli_lane_adapter_block(tmp_path):
    """The run directory of test_gpu_lanegc.py's CLI test: tile 1103's files are tile 1101's but for the last cycle,
    which is tile 1102's.  The adapter is cut from the lane's largest family, so that reads carry it.  The new block
    follows the GC block and closes the lane's output, equals write_lane_adapter of the reference's counts and is all
    the flag adds, also under another --tile-batch; with --lane-dups-hamming it is on the clusters, there on scanned
    cycles that start later and offset the inserts; the TSV is write_lane_adapter_tsv of the same counts."""
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
            "-q", "--all-wells", "--lane-dups"]
    whole = ["--cycles", "0-%d" % L]

    def tiles_of(c0):
        return [(i, [synth.plane_bytes(spec, lane, int(source(t, c)), c) for c in range(c0, L)],
                 synth.filter_bytes(spec, lane, int(t if t != "1103" else "1101"))) for i, t in enumerate(names)]

    tiles = tiles_of(0)
    labels = {0: lane_dups(tiles, n, 4)[2]}
    # the adapter: cycles 6 .. 15 of the first well of the largest class, none of them a no-call
    flat = labels[0].reshape(-1)
    sizes = np.bincount(flat[flat != 0xFFFFFFFF].astype(np.int64))
    root = next(int(g) for g in np.argsort(-sizes, kind="stable")
                if all(tiles[g // n][1][c][g % n] for c in range(6, 16)))
    seq = "".join("ACGT"[tiles[root // n][1][c][root % n] & 3] for c in range(6, 16))

    def block(tiles, labels, k, name, e, o, bins, dimer, summary, first_cycle=0):
        codes = codes_of(name)
        counts = report.LaneAdapterCounts.from_rows(*lane_adapter(tiles, n, 4, labels, codes, e, o), names, name, len(codes),
                                                    e, o, bins, dimer, k, first_cycle)
        text, tsv = io.StringIO(), io.StringIO()
        report.write_lane_adapter(str(lane), counts, verbose=not summary, out=text)
        report.write_lane_adapter_tsv(str(lane), counts, tsv)
        return text.getvalue(), tsv.getvalue(), counts

    plain = _main(argv + whole + ["--lane-dups-gc"])
    want, tsv, counts = block(tiles, labels[0], 0, seq, 1, 8, 10, 10, False)
    assert counts.with_adapter >= sizes[root] >= 3 and counts.ad_copies >= 2 and counts.hist[6][3] >= sizes[root]
    assert want.count("LaneAdapter: 1\tBin: ") == 11 and want.count("LaneAdapterTile: 1\t") == 4
    assert "LaneAdapterSummary: 1\tAdapter: %s\tLength: 10\tMismatches: 1\tMinOverlap: 8\tCycles: 24\tBins: 10\t" % seq in want
    out_file = str(tmp_path / "adapter.tsv")
    got = _main(argv + whole + ["--tile-batch", "1", "--lane-dups-gc", "--lane-dups-adapter", seq.lower(),
                                "--lane-dups-adapter-out", out_file])
    assert got == plain + want                                         # the new block, after the GC block, is all the flag adds
    assert "".join(line for line in got.splitlines(True) if not line.startswith("LaneAdapter")).rstrip("\n") == plain.rstrip("\n")
    assert open(out_file).read() == tsv
    # on the clusters, after every other pass of the lane, the summary alone, with the other options, and on scanned
    # cycles that start at cycle 4: the positions are numbered from it, and the block says so
    late = tiles_of(4)
    part = ["--cycles", "4-%d" % L, "--lane-dups-hamming", "2", "-S", "--lane-dups-mismatches", "--lane-dups-distance",
            "--lane-dups-top", "5"]
    want, tsv, counts = block(late, lane_near_dups(late, n, 4, 2)[2], 2, seq, 3, 3, 4, 2, True, first_cycle=4)
    assert counts.inexact > 100 and counts.partial > 100 and counts.hist[2][3] >= 2
    out_file = str(tmp_path / "adapter2.tsv")
    opts = ["--lane-dups-adapter-mismatches", "3", "--lane-dups-adapter-min-overlap", "3", "--lane-dups-adapter-bins", "4",
            "--lane-dups-adapter-dimer", "2"]
    got = _main(argv + part + ["--lane-dups-adapter", seq, "--lane-dups-adapter-out", out_file] + opts)
    assert got.endswith(want) and got.count("LaneAdapter") == want.count("LaneAdapter") and open(out_file).read() == tsv
    assert want.count("\tHamming: 2\t") == 6 and "LaneAdapterTile" not in want and "\tDimers (a <= 2): " in want
    assert "\tCycles: 20\tOffset: 4\tBins: 4\t" in want and "\tBin: 0\tInsert: 4-8\t" in want
    # cycles that skip one are refused before anything is scanned
    with pytest.raises(ValueError, match="one ascending run of consecutive cycles"):
        cwd.main(argv + ["--cycles", "0-10,12-%d" % L, "--lane-dups-adapter", seq])
