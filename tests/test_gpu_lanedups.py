"""Read classes across the tiles of a lane on the GPU (the LaneDups accumulator, include/welldup_lanedups.h)
against the host reference of tests/lanedups_ref.py - lane row, tile rows and labels equal, nothing approximate -
however the tiles are fed, and against the per-tile classes (wd_tile_dups), which the lane's classes refine."""
import io
import os
import shutil
import time
from contextlib import redirect_stdout

import numpy as np
import pytest

from lanedups_ref import check_identities, lane_dups, members_of
from tiledups_ref import INVALID
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


def _reference(tb, index, max_tiles, slots=None):
    """The host reference from the bytes resident on the GPU."""
    slots = range(tb.n_tiles) if slots is None else slots
    tiles = [(index[s], [tb.download_plane(s, c) for c in range(tb.L)], tb.download_filter(s)) for s in slots]
    return lane_dups(tiles, tb.N, max_tiles)


def _feed(sc, tb, index, max_tiles, calls, hash_bits=0, labels=True):
    """calls: a list of lists of batch slots, one wd_lane_dups_add each -> LaneDups.finish()"""
    ld = LaneDups(sc, tb.N, max_tiles, tb.L, hash_bits=hash_bits)
    try:
        for slots in calls:
            ld.add_tables([index[s] for s in slots], _tables(tb, slots))
        return ld.finish(labels=labels)
    finally:
        ld.close()


def _tables(tb, slots):
    ptrs = tb.plane_ptrs()
    return Scanner._tables([ptrs[s] for s in slots], [tb.filter_ptr(s) for s in slots], tb.L)


def _same(got, want):
    lane, trow, labels = got
    assert (lane == want[0]).all(), (lane, want[0])
    assert (trow == want[1]).all(), (trow, want[1])
    if labels is not None:
        assert (labels == want[2]).all()


def _small_lane():
    """Five synthetic tiles (copies planted inside every tile, one tile dead) and reads copied across tiles by hand."""
    spec = synth.SynthSpec(seed=91, n_clusters=N, row=COLS, plant_per_64k=8000, nocall_per_64k=400, dead_tiles=(1102,),
                           plant_far=True, filter_noise=True)
    reads = [np.stack([synth.plane_bytes(spec, ln, t, c) for c in range(L)], axis=1) for ln, t in TILES]
    filts = [synth.filter_bytes(spec, ln, t) for ln, t in TILES]
    rng = np.random.default_rng(17)
    for src, dst, count in ((0, 2, 300), (2, 3, 200), (0, 4, 150), (3, 4, 100), (0, 1, 50)):
        a, b = rng.choice(N, count, replace=False), rng.choice(N, count, replace=False)
        reads[dst][b] = reads[src][a]                                  # (chains: a copy of a copy, copies of planted wells)
    return reads, filts


WAYS = {"one call": [[0, 1, 2, 3, 4]], "a tile per call": [[0], [1], [2], [3], [4]], "2 + 3": [[0, 1], [2, 3, 4]],
        "descending indices": [[3], [0], [2], [4], [1]], "one call, descending": [[3, 0, 2, 4, 1]]}


def test_lane_dups_match_reference_however_the_tiles_are_fed(sc):
    reads, filts = _small_lane()
    tb = _upload(sc, reads, filts)
    try:
        want = _reference(tb, INDEX, MAX_TILES)
        lane, trow, labels = want
        check_identities(lane, trow)
        assert lane[4] > 200 and trow[:, 3].sum() > 100                # classes across tiles, redundancy inside tiles
        assert lane[0] - lane[2] > 1000 and lane[6 + 1:].sum() > 20    # wells in no class; classes of three and more
        assert (trow[INDEX[1]] == 0).all() and (labels[INDEX[1]] == INVALID).all()      # the dead tile
        assert (trow[[2, 4]] == 0).all() and (labels[[2, 4]] == INVALID).all()          # never added
        for bits in (0, 4, 1):
            for name, calls in WAYS.items():
                if bits and name not in ("one call", "descending indices"):
                    continue
                _same(_feed(sc, tb, INDEX, MAX_TILES, calls, hash_bits=bits), want)
            got = _feed(sc, tb, INDEX, MAX_TILES, WAYS["2 + 3"], hash_bits=bits, labels=False)
            assert got[2] is None
            _same(got, want)
    finally:
        tb.free()


def test_planes_need_not_stay(sc):
    """One batch of one slot: tile A is uploaded and added, the same buffers are overwritten with tile B."""
    reads, filts = _small_lane()
    tb = TileBatch(sc, 1, L, N)
    ld = LaneDups(sc, N, 2, L)
    try:
        for i, slot in enumerate((0, 2)):
            tb.upload_tile(0, [np.ascontiguousarray(reads[slot][:, c]) for c in range(L)], filts[slot])
            ld.add(tb, [i])
        got = ld.finish(labels=True)
        tiles = [(i, [np.ascontiguousarray(reads[s][:, c]) for c in range(L)], filts[s]) for i, s in enumerate((0, 2))]
        want = lane_dups(tiles, N, 2)
        assert want[0][4] > 100
        _same(got, want)
    finally:
        ld.close()
        tb.free()


def test_lane_dups_hand_built_cases_across_tiles(sc):
    rng = np.random.default_rng(78)
    reads = [rng.integers(1, 256, (N, L)).astype(np.uint8) for _ in range(3)]      # [well, cycle], no byte 0 yet
    filts = [np.ones(N, dtype=np.uint8) for _ in range(3)]
    gid = lambda t, w: t * N + w
    # equal bases, every quality bit different, on two tiles
    reads[1][1900] = (reads[0][50] & 3) | ((reads[0][50] & 0xFC) ^ 0xFC)
    reads[0][50] |= 0x04                                                           # (neither byte is 0)
    reads[1][1900] |= 0x08
    # byte 0 against byte 0x40: N is not A
    reads[2][1800] = reads[0][60]
    reads[0][60, 11] = 0
    reads[2][1800, 11] = 0x40
    # N == N
    reads[0][70, 5] = 0
    reads[2][2000] = reads[0][70]
    # a twin that fails the filter (and one whose filter byte is 2: only bit 0 counts)
    reads[1][2100] = reads[0][80]
    filts[1][2100] = 0
    reads[2][2200] = reads[0][90]
    filts[2][2200] = 2
    filts[0][80] = 0x81                                                            # ... and any odd byte passes
    # a class of 12 over three tiles, several on one tile
    big = [(0, 300), (0, 301), (0, 2500), (0, 1234), (0, 7), (1, 0), (1, 2639), (1, 640), (1, 641), (2, 333), (2, 1500),
           (2, 2638)]
    for t, w in big[1:]:
        reads[t][w] = reads[0][300]
    # a class confined to one tile
    reads[2][100] = reads[2][2400]
    tb = _upload(sc, reads, filts)
    try:
        want = _reference(tb, [0, 1, 2], 3)
        lane, trow, lab = want
        flat = lab.reshape(-1)
        assert flat[gid(1, 1900)] == gid(0, 50) == flat[gid(0, 50)]
        assert flat[gid(0, 60)] == gid(0, 60) and flat[gid(2, 1800)] == gid(2, 1800)
        assert flat[gid(2, 2000)] == gid(0, 70)
        assert flat[gid(1, 2100)] == INVALID and flat[gid(0, 80)] == gid(0, 80)
        assert flat[gid(2, 2200)] == INVALID and flat[gid(0, 90)] == gid(0, 90)
        assert all(flat[gid(t, w)] == gid(0, 7) for t, w in big)
        assert flat[gid(2, 100)] == flat[gid(2, 2400)] == gid(2, 100)
        # PF, Classes, InClasses, Redundant, CrossTileClasses, TileSpans; sizes 2 (three) and >= 9 (one)
        assert lane.tolist() == [3 * N - 2, 4, 2 + 2 + 12 + 2, 14, 3, 2 + 2 + 3 + 1, 3, 0, 0, 0, 0, 0, 0, 1]
        assert trow.tolist() == [[N, 7, 5, 4, 4], [N - 1, 5, 4, 3, 5], [N - 1, 6, 5, 3, 5]]
        check_identities(lane, trow)
        for bits in (0, 4, 1):
            _same(_feed(sc, tb, [0, 1, 2], 3, [[0, 1, 2]], hash_bits=bits), want)
            _same(_feed(sc, tb, [0, 1, 2], 3, [[2], [1], [0]], hash_bits=bits), want)
    finally:
        tb.free()


@pytest.mark.parametrize("cycles", [1, 9, 10, 11, 151])
def test_lane_dups_shapes(sc, cycles):
    """Rows of one word, one word less a cycle, exactly one, one and a cycle, sixteen; tiles of 1001 wells (the last
    well goes through the tail of k_ld_pack), and planes that start on an odd address (all of them do)."""
    n = 1001
    rng = np.random.default_rng(cycles)
    reads = [rng.integers(0, 256, (n, cycles)).astype(np.uint8) for _ in range(3)]
    for r in reads:
        r[rng.random(r.shape) < 0.02] = 0
    for src, dst in ((0, 1), (1, 2), (0, 2), (2, 2)):
        a, b = rng.choice(n, 150, replace=False), rng.choice(n, 150, replace=False)
        reads[dst][b] = reads[src][a]
    if cycles > 1:                                                     # twins but for the last cycle
        reads[1][:40] = reads[0][:40]
        reads[1][:40, -1] = (reads[0][:40, -1] & 0xFC) | ((reads[0][:40, -1] + 1) & 3) | 4
    filts = [(rng.random(n) < 0.9).astype(np.uint8) for _ in range(3)]
    tb = _upload(sc, reads, filts)
    try:
        want = _reference(tb, [2, 0, 1], 3)
        check_identities(want[0], want[1])
        assert want[0][4] > (2 if cycles == 1 else 100)
        for bits in (0, 1):
            _same(_feed(sc, tb, [2, 0, 1], 3, [[0, 1], [2]], hash_bits=bits), want)
        # the same tiles less their first well: every plane starts one byte after a 256-byte boundary
        tiles = [(i, [tb.download_plane(s, c)[1:] for c in range(cycles)], tb.download_filter(s)[1:])
                 for i, s in enumerate(range(3))]
        want1 = lane_dups(tiles, n - 1, 3)
        ld = LaneDups(sc, n - 1, 3, cycles)
        try:
            flat = [p + 1 for tile in tb.plane_ptrs() for p in tile]
            ld.add_tables([0, 1, 2], Scanner._tables([flat[i * cycles:(i + 1) * cycles] for i in range(3)],
                                                     [f + 1 for f in tb.filter_ptrs()], cycles))
            _same(ld.finish(labels=True), want1)
        finally:
            ld.close()
    finally:
        tb.free()


def test_lane_dups_when_every_read_is_equal(sc, capsys):
    """Three tiles, one read: one slot takes every PF well of the lane.  It must finish; its time is printed."""
    spec = synth.SynthSpec(seed=3, n_clusters=N, row=COLS)
    filts = [synth.filter_bytes(spec, 1, 1101 + i) for i in range(3)]
    reads = [np.tile(np.array([0x42 + (c % 4) for c in range(L)], dtype=np.uint8), (N, 1)) for _ in range(3)]
    tb = _upload(sc, reads, filts)
    try:
        pf = [(f & 1).astype(bool) for f in filts]
        total = int(sum(p.sum() for p in pf))
        first = int(np.flatnonzero(pf[0])[0])
        for bits in (0, 1):
            t0 = time.perf_counter()
            lane, trow, labels = _feed(sc, tb, [0, 1, 2], 3, [[0, 1, 2]], hash_bits=bits)
            with capsys.disabled():
                print("\nevery read equal, 3 x %d wells, hash_bits %d: %.1f ms" % (N, bits, (time.perf_counter() - t0) * 1e3))
            assert lane.tolist() == [total, 1, total, total - 1, 1, 3, 0, 0, 0, 0, 0, 0, 0, 1]
            for i in range(3):
                k = int(pf[i].sum())
                assert trow[i].tolist() == [k, k, k, k - 1, k - (i == 0)]
                assert (labels[i][pf[i]] == first).all() and (labels[i][~pf[i]] == INVALID).all()
    finally:
        tb.free()


def test_lane_dups_refine_the_tile_classes(sc):
    """Per tile, InTile and TileRedundant are InClasses and Redundant of wd_tile_dups on that tile, and two wells of a
    tile share a lane label exactly when they share a tile label."""
    reads, filts = _small_lane()
    x, y = synth.honeycomb_pixels(ROWS, COLS)
    sc.targets_from_coords(x, y, None, levels=3)
    tb = _upload(sc, reads, filts)
    try:
        td_rows, td_labels = tb.tile_dups(labels=True)
        lane, trow, labels = _feed(sc, tb, INDEX, MAX_TILES, WAYS["2 + 3"])
        check_identities(lane, trow)
        assert td_rows[:, 3].sum() > 100
        for s in range(tb.n_tiles):
            ti = INDEX[s]
            assert trow[ti, 0] == td_rows[s, 0]
            assert trow[ti, 2] == td_rows[s, 2] and trow[ti, 3] == td_rows[s, 3]
            pf = td_labels[s] != INVALID
            assert ((labels[ti] != INVALID) == pf).all()
            pairs = np.stack([labels[ti][pf], td_labels[s][pf]], axis=1)
            if pairs.shape[0]:
                assert (np.unique(pairs, axis=0).shape[0] == np.unique(pairs[:, 0]).shape[0] ==
                        np.unique(pairs[:, 1]).shape[0])
    finally:
        tb.free()


def test_lane_dups_full_hiseq4000_tiles(sc):
    """Three tiles of 4 309 253 wells, 50 cycles.  The third has the first's planes, but for one plane whose upper
    half of the wells comes from the second: millions of classes across tiles, millions of wells in none."""
    n, LL = workload.HISEQ4000_ROWS * workload.HISEQ4000_COLS, 50
    assert n == 4309253
    spec = synth.SynthSpec(seed=6, n_clusters=n, row=workload.HISEQ4000_COLS, plant_per_64k=1311, nocall_per_64k=328)
    tb = TileBatch(sc, 3, LL, n)
    tb.fill_synthetic(spec, [(1, 1101), (1, 1102), (1, 1103)], list(range(LL)))
    try:
        for c in range(LL):
            plane = tb.download_plane(0, c)
            if c == 17:
                plane[n // 2:] = tb.download_plane(1, c)[n // 2:]
            sc.h2d(tb.plane_ptr(2, c), plane)
        want = _reference(tb, [0, 1, 2], 3)
        lane, trow, _ = want
        check_identities(lane, trow)
        assert lane[4] > 1_000_000 and lane[0] - lane[2] > 1_000_000
        assert trow[:, 3].sum() > 10_000                                # the planted copies inside the tiles
        _same(_feed(sc, tb, [0, 1, 2], 3, [[0, 1], [2]]), want)
    finally:
        tb.free()


def test_lane_dups_errors_leave_the_lane_as_it_was(sc):
    reads, filts = _small_lane()
    tb = _upload(sc, reads, filts)
    il = None
    ld = LaneDups(sc, N, MAX_TILES, L)
    try:
        want = _reference(tb, INDEX, MAX_TILES)
        ld.add_tables([INDEX[0], INDEX[1]], _tables(tb, [0, 1]))
        for bad in ([INDEX[1]], [INDEX[2], INDEX[0]], [INDEX[2], INDEX[2]], [INDEX[2], MAX_TILES], [-1, INDEX[3]]):
            with pytest.raises(ValueError) as e:                       # repeated, repeated in the call, out of range
                ld.add_tables(bad, _tables(tb, [2, 3][:len(bad)]))
            assert str(e.value).startswith(_lib.strerror(_lib.ERR_ARG))
        with pytest.raises(ValueError):                                # the interleaved layout
            ld.add_tables([INDEX[2]], _tables(tb, [2]), well_stride=4)
        assert sc.get_option("well_stride") == 1
        il = TileBatch(sc, 1, L, N, interleave=4)
        with pytest.raises(ValueError):
            ld.add(il, [INDEX[2]])
        with pytest.raises(ValueError):                                # a batch of another shape (checked in Python)
            ld.add(tb, [INDEX[2]])
        with pytest.raises(ValueError):                                # finish needs both rows
            sc._ck(sc._lib.wd_lane_dups_finish(ld._h, None, None, None))
        # none of these changed anything: the tiles they named can still be added, and the result is right
        ld.add_tables([INDEX[4], INDEX[2], INDEX[3]], _tables(tb, [4, 2, 3]))
        _same(ld.finish(labels=True), want)
        with pytest.raises(ValueError):                                # add after finish
            ld.add_tables([2], _tables(tb, [0]))
        with pytest.raises(ValueError):                                # finish twice
            ld.finish()
        ld.restart()                                                   # the same workspace, another lane
        ld.add_tables([INDEX[s] for s in range(5)], _tables(tb, range(5)))
        _same(ld.finish(), want)
        # a workspace too small
        import ctypes
        h = ctypes.c_void_p()
        rc = sc._lib.wd_lane_dups_begin(sc._ctx, N, MAX_TILES, L, ctypes.c_void_p(ld.d_ws), ld.ws_bytes - 256, 0,
                                        ctypes.byref(h))
        assert rc == _lib.ERR_ARG and not h.value
        assert sc.lane_dups_workspace_bytes(N, MAX_TILES, L) == ld.ws_bytes
        with pytest.raises(RuntimeError) as e:                         # 2^32 - 1 wells: labels are 32-bit
            LaneDups(sc, 4309253, 997, L)
        assert str(e.value).startswith(_lib.strerror(_lib.ERR_UNSUPPORTED))
    finally:
        ld.close()
        ld.close()                                                     # (a second close is a no-op)
        if il is not None:
            il.free()
        tb.free()


# ---- the CLI ------------------------------------------------------------------------------------
def _main(argv):
    out = io.StringIO()
    with redirect_stdout(out):
        assert cwd.main(argv) == 0
    return out.getvalue()


def test_cli_lane_dups_block_and_tsv(tmp_path):
    """2 lanes x 4 tiles; in each lane tile 1103's files are copies of tile 1101's.  The lane block is the same for
    --tile-batch 1, 2 and the default, equals the reference, and is all the flag adds to the output."""
    rows, cols, levels = 36, 70, 3
    n = rows * cols
    x, y = synth.honeycomb_pixels(rows, cols)
    spec = synth.SynthSpec(seed=35, n_clusters=n, row=cols, plant_per_64k=8000, nocall_per_64k=500, plant_far=True)
    run_dir = str(tmp_path / "run")
    names = ["1101", "1102", "1103", "1104"]
    synth.write_run_dir(spec, run_dir, [1, 2], names, list(range(L)), slocs=synth.slocs_bytes(x, y))
    for lane in (1, 2):
        ldir = os.path.join(run_dir, "Data", "Intensities", "BaseCalls", "L%03d" % lane)
        shutil.copy(os.path.join(ldir, "s_%d_1101.filter" % lane), os.path.join(ldir, "s_%d_1103.filter" % lane))
        for c in range(L):
            cdir = os.path.join(ldir, "C%d.1" % (c + 1))
            shutil.copy(os.path.join(cdir, "s_%d_1101.bcl.gz" % lane), os.path.join(cdir, "s_%d_1103.bcl.gz" % lane))
    argv = ["-s", "hiseq_x", "-r", run_dir, "-t", "1101,1102,1103,1104", "-i", "1,2", "-l", str(levels),
            "--cycles", "0-%d" % L, "-q", "--all-wells"]
    blocks, want_tsv = {}, ["lane\ttile\twell\tclass_tile\tclass_well"]
    for summary in (False, True):
        for lane in (1, 2):
            tiles = [(i, [synth.plane_bytes(spec, lane, int(t if t != "1103" else "1101"), c) for c in range(L)],
                      synth.filter_bytes(spec, lane, int(t if t != "1103" else "1101"))) for i, t in enumerate(names)]
            lane_row, tile_rows, labels = lane_dups(tiles, n, 4)
            counts = report.LaneDupCounts.from_rows(lane_row, tile_rows, names)
            # every PF well of 1101 has its twin on 1103; the copies planted inside the tiles are classes of their own
            assert counts.cross_tile_classes > 1000 and tile_rows[0, 1] == tile_rows[0, 0] and counts.within_tiles > 50
            text = io.StringIO()
            report.write_lane_dups(str(lane), counts, verbose=not summary, out=text)
            blocks[(summary, lane)] = text.getvalue()
            if not summary:
                want_tsv += ["%d\t%s\t%d\t%s\t%d" % (lane, names[a], b, names[c], d)
                             for a, b, c, d in zip(*(v.tolist() for v in members_of(labels, n)))]
    for summary in (False, True):
        flags = ["-S"] if summary else []
        plain = _main(argv + flags + ["--tile-dups"])
        tsv = str(tmp_path / "lane.tsv")
        runs = [_main(argv + flags + ["--tile-dups", "--lane-dups", "--tile-batch", "1"]),
                _main(argv + flags + ["--tile-dups", "--lane-dups", "--tile-batch", "2", "--lane-dups-out", tsv]),
                _main(argv + flags + ["--tile-dups", "--lane-dups"])]
        assert runs[0] == runs[1] == runs[2]
        assert open(tsv).read().splitlines() == want_tsv
        b1, b2 = blocks[(summary, 1)], blocks[(summary, 2)]
        assert runs[0].count(b1) == 1 and runs[0].endswith(b2)
        assert runs[0].replace(b1, "", 1)[:-len(b2)] == plain          # minus the new blocks: today's output
        assert runs[0].index(b1) < runs[0].index("TileDupsSummary: 2")  # lane 1's block closes lane 1's output
        bare = _main(argv + flags + ["--lane-dups"])
        assert bare.replace(b1, "", 1)[:-len(b2)] == _main(argv + flags)
    assert "Lane duplication (Redundant/PF wells): " in b2 and "Estimated library size" in b2
