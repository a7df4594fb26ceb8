"""Near-duplicate read clusters per tile on the GPU (wd_tile_near_dups, include/welldup_tilenear.h) against the
host reference of tests/tilenear_ref.py - rows and labels equal, integers, nothing approximate - and against
what they must agree with by definition: the classes of wd_tile_dups at K = 0, the clusters at K - 1, the
duplicate sets of wd_dup_sets at Hamming K on the same batch."""
import io
import os
import re
import subprocess
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

from tiledups_ref import INVALID, tile_dups
from tilenear_ref import HAND, hand_made_tile, long_boundary_check, long_boundary_reads, tile_near_dups
from well_duplicates_amd import _lib
from well_duplicates_amd import count_well_duplicates as cwd
from well_duplicates_amd import report, synth, workload
from well_duplicates_amd.scanner import MODE_HAMMING, Scanner, TileBatch

pytestmark = pytest.mark.gpu

ROWS, COLS = 44, 60
N = ROWS * COLS
LEVELS = 3
TILES = [(1, 1101), (1, 1102), (2, 1101)]


@pytest.fixture(scope="module")
def sc():
    s = Scanner(0)
    yield s
    s.close()


def _honeycomb(sc, rows=ROWS, cols=COLS, levels=LEVELS):
    x, y = synth.honeycomb_pixels(rows, cols)
    T, _ = sc.targets_from_coords(x, y, None, levels=levels)
    assert T == rows * cols
    return sc.get_targets()


def _reference(tb, csr, k, method="all_pairs", n=None, skip=0):
    """(rows, labels) of the host reference for every tile of a batch, from the bytes resident on the GPU
    (wells skip .. skip + n of every plane)."""
    _, lvl_off, nbr = csr
    n = tb.N if n is None else n
    rows, labels = [], []
    for i in range(tb.n_tiles):
        planes = [tb.download_plane(i, c)[skip:skip + n] for c in range(tb.L)]
        row, lab = tile_near_dups(planes, tb.download_filter(i)[skip:skip + n], lvl_off, nbr, k, method=method)
        rows.append(row)
        labels.append(lab)
    return np.array(rows), np.array(labels)


def _upload(sc, reads, filt):
    """[n, L] bytes -> a batch of one tile."""
    tb = TileBatch(sc, 1, reads.shape[1], reads.shape[0])
    tb.upload_tile(0, [np.ascontiguousarray(reads[:, c]) for c in range(reads.shape[1])], filt)
    return tb


def _other_base(b):
    return (int(b) & 0xFC | ((int(b) + 1) & 3)) or 0x41


def _plant_near(rng, reads, pairs, mismatches, keep_out=()):
    """Copies `pairs` reads onto wells chosen anywhere on the tile, each with 1..mismatches substituted cycles."""
    n, L = reads.shape
    free = np.setdiff1d(np.arange(n), np.asarray(keep_out, dtype=np.int64))
    src = rng.choice(free, pairs, replace=False)
    dst = rng.choice(np.setdiff1d(free, src), pairs, replace=False)
    reads[dst] = reads[src]
    for i, w in enumerate(dst.tolist()):
        for c in rng.choice(L, min(L, 1 + i % mismatches), replace=False).tolist():
            reads[w, c] = _other_base(reads[w, c])
    return src, dst


# ---- synthetic tiles ----------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
def test_near_dups_match_reference_on_small_tiles(sc, k):
    """Three tiles per call (one dead), L = K + 1, 25, 50, 151; the generator plants copies with one and two
    substituted cycles beside the exact ones."""
    csr = _honeycomb(sc)
    spec = synth.SynthSpec(seed=40 + k, n_clusters=N, row=COLS, plant_per_64k=8000, nocall_per_64k=400,
                           dead_tiles=(1102,), plant_far=True)
    for L in (k + 1, 25, 50, 151):
        tb = TileBatch(sc, len(TILES), L, N)
        tb.fill_synthetic(spec, TILES, list(range(L)))
        try:
            want_rows, want_labels = _reference(tb, csr, k)
            assert (want_rows[1] == 0).all()                                   # the dead tile: no PF well
            if L >= 25:
                assert want_rows[0, 4] > 0                                     # near pairs exist
                eq_rows, _ = tb.tile_dups()
                assert want_rows[0, 3] > eq_rows[0, 3]                         # ... and make more wells redundant
            rows, labels = tb.tile_near_dups(k, labels=True)
            assert (labels == want_labels).all(), (k, L)
            assert (rows == want_rows).all(), (k, L, rows, want_rows)
            rows2, none = tb.tile_near_dups(k)                                 # without labels
            assert none is None and (rows2 == want_rows).all()
        finally:
            tb.free()


@pytest.mark.parametrize("k,L", [(1, 25), (2, 50), (3, 151)])
def test_near_dups_unaligned_planes(sc, k, L):
    """Planes and filters that start one byte into their buffers: the fingerprint pass takes its scalar path."""
    csr = _honeycomb(sc)
    spec = synth.SynthSpec(seed=50 + k, n_clusters=N + 1, row=COLS, plant_per_64k=8000, nocall_per_64k=400)
    tb = TileBatch(sc, 2, L, N + 1)
    tb.fill_synthetic(spec, TILES[::2], list(range(L)))
    ws = sc.tile_near_dups_workspace_bytes(N, 2, k)
    d_ws = sc.malloc(ws + 2 * 4 * N)
    try:
        want_rows, want_labels = _reference(tb, csr, k, n=N, skip=1)
        assert want_rows[0, 4] > 0
        planes = [[tb.plane_ptr(i, c) + 1 for c in range(L)] for i in range(2)]
        filters = [tb.filter_ptr(i) + 1 for i in range(2)]
        rows = sc.tile_near_dups(planes, filters, N, k, d_ws, ws, labels=[d_ws + ws + 4 * N * i for i in range(2)])
        labels = sc.d2h(d_ws + ws, 2 * 4 * N, np.uint32).reshape(2, N)
        assert (rows == want_rows).all(), (rows, want_rows)
        assert (labels == want_labels).all()
    finally:
        sc.free(d_ws)
        tb.free()


def test_near_dups_hand_made_tile(sc):
    """The tile of tests/test_tilenear_host.py: a chain, N against N and against a base, a non-PF well between
    two clusters, quality bits, a class with a near copy far away - the hand-worked rows and labels."""
    planes, filt, (lvl_off, nbr) = hand_made_tile()
    sc.set_targets(np.arange(24, dtype=np.int32), lvl_off.astype(np.int32), nbr.astype(np.int32))
    tb = TileBatch(sc, 1, 6, 24)
    tb.upload_tile(0, planes, filt)
    try:
        for k in (1, 2):
            want = HAND[k]
            for bits in (0, 4, 1):
                rows, labels = tb.tile_near_dups(k, labels=True, hash_bits=bits)
                assert labels[0].tolist() == want["labels"], (k, bits)
                assert rows[0].tolist() == want["head"] + want["local"] + want["ring_wells"] + want["bins"], (k, bits)
        rows3, labels3 = tb.tile_near_dups(3, labels=True)
        want_row, want_lab = tile_near_dups(planes, filt, lvl_off, nbr, 3)
        assert (rows3[0] == want_row).all() and (labels3[0] == want_lab).all()
    finally:
        tb.free()


def _far_tile(seed, L=40):
    """Random reads; exact copies and near copies (one or two cycles) written far from their sources."""
    rng = np.random.default_rng(seed)
    reads = rng.integers(1, 256, (N, L)).astype(np.uint8)
    reads[rng.random((N, L)) < 0.005] = 0
    far = rng.permutation(N)[:120]
    reads[far[60:]] = reads[far[:60]]                                          # classes, far apart
    _plant_near(rng, reads, 150, 2)
    side = np.arange(100, N - 100, 97)                                         # ... and some side by side
    reads[side + 1] = reads[side]
    for w in side[::2].tolist():
        reads[w + 1, w % L] = _other_base(reads[w + 1, w % L])
    filt = np.where(rng.random(N) < 0.85, 1, 0).astype(np.uint8)
    return reads, filt


def test_near_dups_far_copies_and_identities(sc):
    """Near copies outside every ring: clusters and Local differ.  K = 0 is wd_tile_dups; the clusters at K
    coarsen those at K - 1; Local[l] >= InSets[l] and Redundant >= Redundant[levels] of the duplicate sets at
    Hamming K; hash_bits 4 and 1 change nothing."""
    csr = _honeycomb(sc)
    reads, filt = _far_tile(9)
    tb = _upload(sc, reads, filt)
    try:
        eq_rows, eq_labels = tb.tile_dups(labels=True)
        rows0, labels0 = tb.tile_near_dups(0, labels=True)
        assert (np.delete(rows0, 4, axis=1) == eq_rows).all() and (rows0[:, 4] == 0).all()
        assert (labels0 == eq_labels).all()
        prev_rows, prev = rows0, labels0
        for k in (1, 2, 3):
            want_rows, want_labels = _reference(tb, csr, k)
            rows, labels = tb.tile_near_dups(k, labels=True)
            assert (rows == want_rows).all(), (k, rows, want_rows)
            assert (labels == want_labels).all(), k
            r = rows[0]
            assert r[5 + LEVELS - 1] < r[2]                                    # wells whose cluster is all far away
            assert r[4] >= prev_rows[0, 4] and r[3] >= prev_rows[0, 3]
            if k <= 2:
                assert r[4] > prev_rows[0, 4] and r[3] > prev_rows[0, 3]       # (copies with one and with two cycles)
            pf = labels[0] != INVALID
            # equal label at K - 1 implies equal label at K: a cluster's label at K is one per label at K - 1
            pairs = np.unique(np.stack([prev[0][pf], labels[0][pf]]), axis=1)
            assert np.unique(pairs[0]).size == pairs.shape[1]
            _, sets, _ = tb.dup_sets(MODE_HAMMING, k)
            assert (r[5:5 + LEVELS] >= sets[0, 1 + LEVELS:1 + 2 * LEVELS]).all()
            assert r[0] == sets[0, 0] and r[3] >= sets[0, 3 * LEVELS]
            for bits in (4, 1):
                rows_b, labels_b = tb.tile_near_dups(k, labels=True, hash_bits=bits, pair_budget=1 << 40)
                assert (rows_b == want_rows).all() and (labels_b == want_labels).all(), (k, bits)
            prev_rows, prev = rows, labels
    finally:
        tb.free()


def test_near_dups_degenerate_tiles(sc):
    """All reads equal (one vertex), all reads N, no PF well at all."""
    csr = _honeycomb(sc)
    L = 30
    spec = synth.SynthSpec(seed=3, n_clusters=N, row=COLS)
    filt = synth.filter_bytes(spec, 1, 1101)
    pf = int((filt & 1).sum())
    tb = TileBatch(sc, 3, L, N)
    tb.upload_tile(0, [np.full(N, 0x42 + (c % 4), dtype=np.uint8) for c in range(L)], filt)
    tb.upload_tile(1, [np.zeros(N, dtype=np.uint8) for c in range(L)], filt)
    tb.upload_tile(2, [np.full(N, 0x42 + (c % 4), dtype=np.uint8) for c in range(L)], (filt & 0xFE))
    try:
        for k in (1, 3):
            want_rows, want_labels = _reference(tb, csr, k)
            for bits in (0, 1):
                rows, labels = tb.tile_near_dups(k, labels=True, hash_bits=bits)
                assert (rows == want_rows).all() and (labels == want_labels).all()
                for i in (0, 1):
                    assert rows[i, :5].tolist() == [pf, 1, pf, pf - 1, 0]
                    # (a PF well whose level-1 neighbours all fail the filter meets its cluster a ring further out)
                    assert rows[i, 5 + LEVELS - 1] == pf and rows[i, 5 + 2 * LEVELS:].tolist() == [0] * 7 + [1]
                assert (rows[2] == 0).all() and (labels[2] == INVALID).all()
    finally:
        tb.free()


# ---- the pair budget ------------------------------------------------------------------------------
def test_near_dups_heavy_bucket_and_refusal(sc):
    """3 000 distinct reads that share their whole first segment: one chain of about 4.5 M candidate pairs,
    under the default budget (2^24), exact.  With a budget of 1 000 the call is refused with a message that names
    tile and segment, and the next call on the same batch works as before."""
    csr = _honeycomb(sc, 50, 64)
    n, L, k = 50 * 64, 40, 1
    rng = np.random.default_rng(17)
    reads = rng.integers(1, 256, (n, L)).astype(np.uint8)
    heavy = np.sort(rng.choice(n, 3000, replace=False))
    reads[heavy, :L // 2] = reads[heavy[0], :L // 2]                           # segment 0 of K = 1 is cycles 0..19
    src = heavy[:300]
    dst = heavy[300:600]
    reads[dst] = reads[src]
    for i, w in enumerate(dst.tolist()):
        c = L // 2 + i % (L // 2)
        reads[w, c] = _other_base(reads[w, c])
    filt = np.ones(n, dtype=np.uint8)
    plain, plain_filt = rng.integers(1, 256, (n, L)).astype(np.uint8), np.ones(n, dtype=np.uint8)
    tb = TileBatch(sc, 2, L, n)
    tb.upload_tile(0, [np.ascontiguousarray(plain[:, c]) for c in range(L)], plain_filt)
    tb.upload_tile(1, [np.ascontiguousarray(reads[:, c]) for c in range(L)], filt)
    try:
        want_rows, want_labels = _reference(tb, csr, k)
        assert want_rows[1, 4] == 300 and want_rows[1, 1] == 300               # the planted pairs, and nothing else
        rows, labels = tb.tile_near_dups(k, labels=True)
        assert (rows == want_rows).all(), (rows, want_rows)
        assert (labels == want_labels).all()
        with pytest.raises(RuntimeError) as e:
            tb.tile_near_dups(k, labels=True, pair_budget=1000)
        msg = str(e.value)
        assert msg.startswith(_lib.strerror(_lib.ERR_UNSUPPORTED))
        assert "tile 1" in msg and "segment 0" in msg and "budget of 1000" in msg
        bound = int(re.search(r": (\d+) candidate pairs", msg).group(1))       # the chain, and what else shares its slot
        assert 3000 * 2999 // 2 <= bound <= 3200 * 3199 // 2
        again, again_labels = tb.tile_near_dups(k, labels=True)
        assert (again == want_rows).all() and (again_labels == want_labels).all()
        eq, _ = tb.tile_dups()                                                 # ... and so does everything else
        assert eq[1, 0] == n
    finally:
        tb.free()


def test_near_dups_at_the_long_slot_boundary(sc):
    """K = 1, 20 cycles, one tile of 16 x 16 PF wells: slots of 31 and 32 distinct reads (the chain walk, at most 31
    steps) and of 33 and 34 (the rank path), each with planted pairs at one mismatch - rows and labels of the
    all-pairs reference."""
    csr = _honeycomb(sc, 16, 16)
    reads, groups = long_boundary_reads()
    tb = _upload(sc, reads, np.ones(reads.shape[0], dtype=np.uint8))
    try:
        want_rows, want_labels = _reference(tb, csr, 1)
        long_boundary_check(want_labels[0], groups)
        rows, labels = tb.tile_near_dups(1, labels=True)
        assert (labels == want_labels).all()
        assert (rows == want_rows).all(), (rows, want_rows)
    finally:
        tb.free()


def test_near_dups_refuses_bad_arguments(sc):
    _honeycomb(sc)
    spec = synth.SynthSpec(seed=4, n_clusters=N, row=COLS)
    tb = TileBatch(sc, 1, 3, N)
    tb.fill_synthetic(spec, [(1, 1101)], [0, 1, 2])
    try:
        rows, _ = tb.tile_near_dups(2)                                         # L == K + 1 is served
        assert rows[0, 0] > 0
        with pytest.raises(ValueError):
            tb.tile_near_dups(3)                                               # L < K + 1
        with pytest.raises(ValueError):
            tb.tile_near_dups(4)
        with pytest.raises(ValueError):
            tb.tile_near_dups(1, pair_budget=-1)
        ws = sc.tile_near_dups_workspace_bytes(N, 1, 2)
        with pytest.raises(ValueError):                                        # a workspace too small
            sc.tile_near_dups(None, tb.filter_ptrs(), N, 2, tb.d_tnear, ws - 256, tables=tb.tables, L=3)
        sc.set_option("well_stride", 4)
        try:
            with pytest.raises(RuntimeError) as e:
                sc.tile_near_dups(None, tb.filter_ptrs(), N, 2, tb.d_tnear, ws, tables=tb.tables, L=3)
            assert str(e.value).startswith(_lib.strerror(_lib.ERR_UNSUPPORTED))
        finally:
            sc.set_option("well_stride", 1)
        again, _ = tb.tile_near_dups(2)
        assert (again == rows).all()
    finally:
        tb.free()


# ---- large tiles ----------------------------------------------------------------------------------
def _plant_far_on_device(sc, tb, rng, pairs, mismatches):
    """Near copies written far from their sources into tile 0 of a resident batch (the planes fetched to the
    host, patched and sent back)."""
    n, L = tb.N, tb.L
    src = rng.choice(n, pairs, replace=False)
    dst = (src + n // 2 + rng.integers(0, 1000, pairs)) % n
    cut = [rng.choice(L, 1 + i % mismatches, replace=False).tolist() for i in range(pairs)]
    for c in range(L):
        plane = tb.download_plane(0, c)
        plane[dst] = plane[src]
        for i, cs in enumerate(cut):
            if c in cs:
                plane[dst[i]] = _other_base(plane[dst[i]])
        sc.h2d(tb.plane_ptr(0, c), plane)
    f = tb.download_filter(0)
    f[dst] |= 1
    f[src] |= 1
    sc.h2d(tb.filter_ptr(0), f)


def test_near_dups_full_hiseq4000_tile(sc):
    """One full tile (4 309 253 wells, 50 cycles, 2 % planted, 3 000 near copies half a tile from their
    sources), K = 1, against the deletion-neighbourhood reference."""
    n, L = workload.HISEQ4000_ROWS * workload.HISEQ4000_COLS, 50
    csr = _honeycomb(sc, workload.HISEQ4000_ROWS, workload.HISEQ4000_COLS)
    assert n == 4309253
    spec = synth.SynthSpec(seed=6, n_clusters=n, row=workload.HISEQ4000_COLS, plant_per_64k=1311, nocall_per_64k=328)
    tb = TileBatch(sc, 1, L, n)
    tb.fill_synthetic(spec, [(1, 1101)], list(range(L)))
    try:
        _plant_far_on_device(sc, tb, np.random.default_rng(8), 3000, 1)
        rows, labels = tb.tile_near_dups(1, labels=True)
        eq_rows, _ = tb.tile_dups()
        want_rows, want_labels = _reference(tb, csr, 1, method="deletion")
        assert (rows == want_rows).all(), (rows, want_rows)
        assert (labels == want_labels).all()
        assert want_rows[0, 4] >= 2900 and want_rows[0, 3] >= eq_rows[0, 3] + 2900
        assert want_rows[0, 5 + LEVELS - 1] < want_rows[0, 2] - 2900           # the far copies are not local
    finally:
        tb.free()


def test_near_dups_k2_on_200000_wells(sc):
    """400 x 500 wells, 24 cycles (segments of eight: buckets of several reads each), K = 2, against the
    pair-deletion reference."""
    rows_, cols_, L = 400, 500, 24
    n = rows_ * cols_
    csr = _honeycomb(sc, rows_, cols_)
    spec = synth.SynthSpec(seed=12, n_clusters=n, row=cols_, plant_per_64k=1311, nocall_per_64k=328)
    tb = TileBatch(sc, 1, L, n)
    tb.fill_synthetic(spec, [(1, 1101)], list(range(L)))
    try:
        _plant_far_on_device(sc, tb, np.random.default_rng(13), 2000, 2)
        rows, labels = tb.tile_near_dups(2, labels=True)
        want_rows, want_labels = _reference(tb, csr, 2, method="deletion")
        assert (rows == want_rows).all(), (rows, want_rows)
        assert (labels == want_labels).all()
        assert want_rows[0, 4] >= 1900
    finally:
        tb.free()


# ---- the CLI ------------------------------------------------------------------------------------
CLI_L = 40


def _cli_run(tmp_path, levels=3):
    rows, cols = 36, 70
    n = rows * cols
    x, y = synth.honeycomb_pixels(rows, cols)
    spec = synth.SynthSpec(seed=33, n_clusters=n, row=cols, plant_per_64k=8000, nocall_per_64k=500, plant_far=True)
    run_dir = str(tmp_path / "run")
    synth.write_run_dir(spec, run_dir, [1], ["1101", "1102"], list(range(CLI_L)), slocs=synth.slocs_bytes(x, y))
    argv = ["-s", "hiseq_x", "-r", run_dir, "-t", "1101,1102", "-i", "1", "-l", str(levels),
            "--cycles", "0-%d" % CLI_L, "-q", "--all-wells"]
    return spec, x, y, argv


def _main(argv):
    out = io.StringIO()
    with redirect_stdout(out):
        assert cwd.main(argv) == 0
    return out.getvalue()


def test_cli_near_block_and_tsv(sc, tmp_path):
    levels, k = 3, 1
    spec, x, y, argv = _cli_run(tmp_path, levels)
    sc.targets_from_coords(x, y, None, levels=levels)
    _, lvl_off, nbr = sc.get_targets()
    want, equal, want_tsv = {}, report.TileDupCounts.zeros(levels), ["lane\ttile\twell\tclass\tcluster"]
    for tile in ("1101", "1102"):
        planes = [synth.plane_bytes(spec, 1, int(tile), c) for c in range(CLI_L)]
        filt = synth.filter_bytes(spec, 1, int(tile))
        row, lab = tile_near_dups(planes, filt, lvl_off, nbr, k)
        eq_row, eq_lab = tile_dups(planes, filt, lvl_off, nbr)
        want[tile] = report.TileNearCounts.from_block(row, levels, wells=spec.n_clusters)
        equal = equal + report.TileDupCounts.from_block(eq_row, levels, wells=spec.n_clusters)
        wells, clusters = cwd.set_members(lab)
        want_tsv += ["1\t%s\t%d\t%d\t%d" % (tile, w, c, s)
                     for w, c, s in zip(wells.tolist(), eq_lab[wells].tolist(), clusters.tolist())]
    assert want["1101"].near_pairs > 0
    for summary in ([], ["-S"]):
        block = io.StringIO()
        report.write_tile_near_dups("1", k, want, verbose=not summary, out=block, levels=levels, equal=equal)
        for before in ([], ["--dup-sets"]):
            tsv = str(tmp_path / "classes.tsv")
            plain = _main(argv + summary + before + ["--tile-dups", "--tile-dups-out", tsv])
            plain_tsv = open(tsv).read()
            with_near = _main(argv + summary + before + ["--tile-dups", "--tile-dups-out", tsv,
                                                         "--tile-dups-hamming", str(k)])
            assert with_near == plain + block.getvalue()                       # every byte before the new block stays
            assert open(tsv).read().splitlines() == want_tsv
            assert plain_tsv.splitlines()[0] == "lane\ttile\twell\tclass"
    assert "Tile duplication at Hamming <= 1 (Redundant/PF wells): " in with_near and "\tby equality: " in with_near
    # a budget no tile of this run can meet: the run ends with the library's message
    with pytest.raises(RuntimeError) as e:
        _main(argv + ["--tile-dups", "--tile-dups-hamming", "1", "--tile-dups-pair-budget", "1"])
    assert "pair budget of 1" in str(e.value) and "segment" in str(e.value)


def test_cli_near_two_ranks(tmp_path):
    """torchrun, two ranks on GPU 0 (gloo): the clusters' rows go through the one merge behind the classes'."""
    import socket
    _, _, _, argv = _cli_run(tmp_path)
    argv = argv + ["--dup-sets", "--tile-dups", "--tile-dups-hamming", "2"]
    single = _main(argv)
    assert "TileDupsSummary: 1\tTiles: 2" in single and "TileNearDupsSummary: 1\tTiles: 2\tHamming: 2" in single
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    report_file = str(tmp_path / "report.txt")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                          "--master-addr", "127.0.0.1", "--master-port", str(port),
                          "-m", "well_duplicates_amd.count_well_duplicates"] + argv +
                         ["--device", "0", "--dist-backend", "gloo", "-o", report_file],
                         cwd=repo, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert res.returncode == 0, res.stderr.decode()[-2000:]
    assert open(report_file).read() == single
