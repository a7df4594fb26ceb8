"""Read classes per tile on the GPU (wd_tile_dups, include/welldup_tiledups.h) against the host reference
of tests/tiledups_ref.py - rows and labels equal, nothing approximate - and against the duplicate sets at
equality (wd_dup_sets), which reach the same wells by another route: Local[l] == InSets[l], and a local set
lies inside a class."""
import io
import os
import subprocess
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

from tiledups_ref import INVALID, tile_dups
from well_duplicates_amd import _lib
from well_duplicates_amd import count_well_duplicates as cwd
from well_duplicates_amd import report, synth, workload
from well_duplicates_amd.scanner import Scanner, TileBatch

pytestmark = pytest.mark.gpu

ROWS, COLS, L = 44, 60, 40
TILES = [(1, 1101), (1, 1102), (2, 1101)]


@pytest.fixture(scope="module")
def sc():
    s = Scanner(0)
    yield s
    s.close()


def _small(sc, levels, far):
    n = ROWS * COLS
    x, y = synth.honeycomb_pixels(ROWS, COLS)
    T, _ = sc.targets_from_coords(x, y, None, levels=levels)
    assert T == n
    spec = synth.SynthSpec(seed=21 + levels, n_clusters=n, row=COLS, plant_per_64k=8000, nocall_per_64k=400,
                           dead_tiles=(1102,), plant_far=far)
    return spec, sc.get_targets()


def _reference(tb, csr):
    """(rows, labels) of the host reference for every tile of a batch, from the bytes resident on the GPU."""
    _, lvl_off, nbr = csr
    rows, labels = [], []
    for i in range(tb.n_tiles):
        planes = [tb.download_plane(i, c) for c in range(tb.L)]
        row, lab = tile_dups(planes, tb.download_filter(i), lvl_off, nbr)
        rows.append(row)
        labels.append(lab)
    return np.array(rows), np.array(labels)


def _check_identities(tb, rows, labels, levels):
    """Against the duplicate sets at equality on the same batch, every tile."""
    _, sets, set_labels = tb.dup_sets(0, 0, labels=True)
    for i in range(tb.n_tiles):
        in_sets = sets[i, 1 + levels:1 + 2 * levels]
        assert (rows[i, 4:4 + levels] == in_sets).all(), (i, rows[i], sets[i])
        assert rows[i, 0] == sets[i, 0]                                        # PF wells
        assert rows[i, 3] >= sets[i, 3 * levels]                               # Redundant >= Redundant[levels]
        pf = labels[i] != INVALID
        assert ((set_labels[i] != INVALID) == pf).all()
        # a well and the smallest well of its local set are classmates
        assert (labels[i][pf] == labels[i][set_labels[i][pf].astype(np.int64)]).all()


@pytest.mark.parametrize("levels,far", [(3, False), (3, True), (5, True)])
def test_tile_dups_match_reference_on_small_tiles(sc, levels, far):
    """Three tiles (one dead); with hash_bits 4 and 1 unequal reads share a fingerprint and nothing changes."""
    spec, csr = _small(sc, levels, far)
    tb = TileBatch(sc, len(TILES), L, spec.n_clusters)
    tb.fill_synthetic(spec, TILES, list(range(L)))
    try:
        want_rows, want_labels = _reference(tb, csr)
        assert want_rows[0, 1] == {(3, False): 118, (3, True): 101, (5, True): 100}[(levels, far)]
        assert want_rows[0, 4 + 2 * levels + 1:].sum() > 0                     # classes of more than two wells
        assert (want_rows[1] == 0).all()                                       # the dead tile: no PF well
        if far:
            assert want_rows[0, 4 + levels - 1] < want_rows[0, 2]              # non-local classmates exist
        else:
            assert want_rows[0, 4 + levels - 1] == want_rows[0, 2]
        if (levels, far) == (3, True):
            assert (want_rows[0, 2], want_rows[0, 4 + levels - 1]) == (205, 137)
        for bits in (0, 4, 1):
            rows, labels = tb.tile_dups(labels=True, hash_bits=bits)
            assert (labels == want_labels).all(), (levels, far, bits)
            assert (rows == want_rows).all(), (levels, far, bits, rows, want_rows)
            rows2, none = tb.tile_dups(hash_bits=bits)                         # without labels
            assert none is None and (rows2 == want_rows).all()
        _check_identities(tb, want_rows, want_labels, levels)
    finally:
        tb.free()


def test_tile_dups_hand_built_tile(sc):
    levels = 3
    spec, csr = _small(sc, levels, False)
    n = spec.n_clusters
    rng = np.random.default_rng(77)
    reads = rng.integers(1, 256, (n, L)).astype(np.uint8)                      # [well, cycle], no byte 0 yet
    filt = np.ones(n, dtype=np.uint8)
    far_a, far_b = 7, 7 + n // 2                                               # a read copied half a tile away
    reads[far_b] = reads[far_a]
    named = [far_b, 1900, 1800, 2000, 2100, 2200]                              # (the wells the cases below use)
    scattered = np.sort(rng.choice(np.setdiff1d(np.arange(100, n - 100), named), 12, replace=False))
    reads[scattered] = reads[scattered[0]]                                     # a class of 12 all over the tile
    q_a, q_b = 50, 1900                                                        # equal bases, every quality value different
    reads[q_b] = (reads[q_a] & 3) | ((reads[q_a] & 0xFC) ^ 0xFC)
    reads[q_a] |= 0x04                                                         # (neither byte is 0)
    reads[q_b] |= 0x08
    z_a, z_b = 60, 1800                                                        # byte 0 against a byte with low bits 0
    reads[z_b] = reads[z_a]
    reads[z_a, 11] = 0
    reads[z_b, 11] = 0x40
    n_a, n_b = 70, 2000                                                        # N == N
    reads[n_a, 5] = 0
    reads[n_b] = reads[n_a]
    t_a, t_b = 80, 2100                                                        # the twin fails the filter
    reads[t_b] = reads[t_a]
    filt[t_b] = 0
    f_a, f_b = 90, 2200                                                        # filter byte 2: only bit 0 counts
    reads[f_b] = reads[f_a]
    filt[f_b] = 2
    filt[far_a] = 0x81                                                         # ... and any odd byte passes
    tb = TileBatch(sc, 1, L, n)
    tb.upload_tile(0, [np.ascontiguousarray(reads[:, c]) for c in range(L)], filt)
    try:
        want_rows, want_labels = _reference(tb, csr)
        lab = want_labels[0]
        assert lab[far_b] == far_a and lab[far_a] == far_a
        assert (lab[scattered] == scattered[0]).all()
        assert lab[q_b] == q_a and lab[n_b] == n_a
        assert lab[z_a] == z_a and lab[z_b] == z_b
        assert lab[t_a] == t_a and lab[t_b] == INVALID and lab[f_a] == f_a and lab[f_b] == INVALID
        assert want_rows[0, :4].tolist() == [n - 2, 4, 2 + 12 + 2 + 2, 14]
        assert want_rows[0, 4 + 2 * levels:].tolist() == [3, 0, 0, 0, 0, 0, 0, 1]
        assert want_rows[0, 4 + levels - 1] < want_rows[0, 2]
        for bits in (0, 4, 1):
            rows, labels = tb.tile_dups(labels=True, hash_bits=bits)
            assert (labels == want_labels).all(), bits
            assert (rows == want_rows).all(), (bits, rows, want_rows)
        _check_identities(tb, want_rows, want_labels, levels)
    finally:
        tb.free()


def test_tile_dups_when_every_read_is_equal(sc):
    """One slot takes every well: one class of all PF wells, labelled with the first of them."""
    levels = 3
    spec, csr = _small(sc, levels, False)
    n = spec.n_clusters
    tb = TileBatch(sc, 1, L, n)
    filt = synth.filter_bytes(spec, 1, 1101)
    tb.upload_tile(0, [np.full(n, 0x42 + (c % 4), dtype=np.uint8) for c in range(L)], filt)
    try:
        pf = (filt & 1).astype(bool)
        first = int(np.flatnonzero(pf)[0])
        want_rows, want_labels = _reference(tb, csr)
        for bits in (0, 1):
            rows, labels = tb.tile_dups(labels=True, hash_bits=bits)
            assert (rows == want_rows).all() and (labels == want_labels).all()
            r = rows[0]
            assert r[:4].tolist() == [pf.sum(), 1, pf.sum(), pf.sum() - 1]
            assert (r[4:4 + levels] == pf.sum()).all()                          # Local[l] == InClasses for every l
            assert r[4 + 2 * levels:].tolist() == [0] * 7 + [1]
            assert (labels[0][pf] == first).all() and (labels[0][~pf] == INVALID).all()
        _check_identities(tb, want_rows, want_labels, levels)
    finally:
        tb.free()


def test_tile_dups_deterministic_across_batches(sc):
    """The same batch twice, and eight tiles in one batch or one by one: identical rows and labels."""
    spec, _ = _small(sc, 3, True)
    tiles = [(1, 1101 + i) for i in range(8)]
    big = TileBatch(sc, 8, L, spec.n_clusters)
    big.fill_synthetic(spec, tiles, list(range(L)))
    try:
        r1, l1 = big.tile_dups(labels=True)
        r2, l2 = big.tile_dups(labels=True)
        assert (r1 == r2).all() and (l1 == l2).all()
        assert (r1[1] == 0).all() and (np.delete(r1[:, 1], 1) > 0).all()       # (1102 is the dead tile)
        for i, t in enumerate(tiles):
            one = TileBatch(sc, 1, L, spec.n_clusters)
            one.fill_synthetic(spec, [t], list(range(L)))
            try:
                r, lab = one.tile_dups(labels=True)
            finally:
                one.free()
            assert (r[0] == r1[i]).all() and (lab[0] == l1[i]).all()
    finally:
        big.free()


def test_tile_dups_full_hiseq4000_tile(sc):
    """One full tile (4 309 253 wells, 3 levels, 150 bp, 2 % planted): rows and labels equal the host
    reference, the identities hold against the duplicate sets at equality."""
    levels, n, LL = 3, workload.HISEQ4000_ROWS * workload.HISEQ4000_COLS, 150
    x, y = synth.honeycomb_pixels(workload.HISEQ4000_ROWS, workload.HISEQ4000_COLS)
    T, _ = sc.targets_from_coords(x, y, None, levels=levels)
    assert T == n == 4309253
    csr = sc.get_targets()
    spec = synth.SynthSpec(seed=5, n_clusters=n, row=workload.HISEQ4000_COLS, plant_per_64k=1311, nocall_per_64k=328)
    tb = TileBatch(sc, 1, LL, n)
    tb.fill_synthetic(spec, [(1, 1101)], list(range(LL)))
    try:
        rows, labels = tb.tile_dups(labels=True)
        want_rows, want_labels = _reference(tb, csr)
        assert (rows == want_rows).all(), (rows, want_rows)
        assert (labels == want_labels).all()
        assert want_rows[0, 3] > 0.005 * want_rows[0, 0]                        # ~2 % planted: many classes
        _check_identities(tb, rows, labels, levels)
    finally:
        tb.free()


def test_tile_dups_refuses_what_it_cannot_do(sc):
    """The interleaved layout -> WD_ERR_UNSUPPORTED, sampled targets -> WD_ERR_ARG; the context works on."""
    levels = 3
    spec, csr = _small(sc, levels, True)
    n = spec.n_clusters
    tb = TileBatch(sc, 1, L, n)
    tb.fill_synthetic(spec, [(1, 1101)], list(range(L)))
    try:
        good, _ = tb.tile_dups()
        ws = sc.tile_dups_workspace_bytes(n, 1)
        sc.set_option("well_stride", 4)
        try:
            with pytest.raises(RuntimeError) as e:
                sc.tile_dups(None, tb.filter_ptrs(), n, tb.d_tdups, ws, tables=tb.tables, L=L)
            assert str(e.value).startswith(_lib.strerror(_lib.ERR_UNSUPPORTED))
        finally:
            sc.set_option("well_stride", 1)
        with pytest.raises(ValueError):                                        # a workspace too small: WD_ERR_ARG
            sc.tile_dups(None, tb.filter_ptrs(), n, tb.d_tdups, ws - 256, tables=tb.tables, L=L)
        centre, lvl_off, nbr = csr
        keep = np.arange(0, n, 7)
        sub_off = np.zeros((keep.size, levels + 1), dtype=np.int32)
        sub_nbr = []
        for j, t in enumerate(keep.tolist()):
            sub_off[j, 0] = len(sub_nbr)
            for l in range(levels):
                sub_nbr += nbr[lvl_off[t, l]:lvl_off[t, l + 1]].tolist()
                sub_off[j, l + 1] = len(sub_nbr)
        sc.set_targets(centre[keep], sub_off, np.array(sub_nbr, dtype=np.int32))
        with pytest.raises(ValueError):                                        # T != N: WD_ERR_ARG
            tb.tile_dups()
        blocks, _ = tb.count(0, 0)                                             # the context still scans
        assert blocks[0, 0] > 0
        x, y = synth.honeycomb_pixels(ROWS, COLS)
        sc.targets_from_coords(x, y, None, levels=levels)
        again, _ = tb.tile_dups()
        assert (again == good).all()
    finally:
        tb.free()


# ---- the CLI ------------------------------------------------------------------------------------
def _cli_run(tmp_path, levels=3):
    rows, cols = 36, 70
    n = rows * cols
    x, y = synth.honeycomb_pixels(rows, cols)
    spec = synth.SynthSpec(seed=33, n_clusters=n, row=cols, plant_per_64k=8000, nocall_per_64k=500, plant_far=True)
    run_dir = str(tmp_path / "run")
    synth.write_run_dir(spec, run_dir, [1], ["1101", "1102"], list(range(L)), slocs=synth.slocs_bytes(x, y))
    argv = ["-s", "hiseq_x", "-r", run_dir, "-t", "1101,1102", "-i", "1", "-l", str(levels),
            "--cycles", "0-%d" % L, "-q", "--all-wells"]
    return spec, x, y, argv


def _main(argv):
    out = io.StringIO()
    with redirect_stdout(out):
        assert cwd.main(argv) == 0
    return out.getvalue()


def test_cli_tile_dups_block_and_tsv(sc, tmp_path):
    levels = 3
    spec, x, y, argv = _cli_run(tmp_path, levels)
    sc.targets_from_coords(x, y, None, levels=levels)
    _, lvl_off, nbr = sc.get_targets()
    want, want_tsv = {}, ["lane\ttile\twell\tclass"]
    for tile in ("1101", "1102"):
        planes = [synth.plane_bytes(spec, 1, int(tile), c) for c in range(L)]
        row, lab = tile_dups(planes, synth.filter_bytes(spec, 1, int(tile)), lvl_off, nbr)
        want[tile] = report.TileDupCounts.from_block(row, levels, wells=spec.n_clusters)
        wells, classes = cwd.set_members(lab)
        want_tsv += ["1\t%s\t%d\t%d" % (tile, w, s) for w, s in zip(wells.tolist(), classes.tolist())]
    assert want["1101"].classes > 0 and want["1101"].local[-1] < want["1101"].in_classes
    for summary in ([], ["-S"]):
        block = io.StringIO()
        report.write_tile_dups("1", want, verbose=not summary, out=block, levels=levels)
        for before in ([], ["--dup-sets"]):
            plain = _main(argv + summary + before)
            tsv = str(tmp_path / "classes.tsv")
            with_classes = _main(argv + summary + before + ["--tile-dups", "--tile-dups-out", tsv])
            assert with_classes == plain + block.getvalue()
            assert open(tsv).read().splitlines() == want_tsv
        # a scan by another metric: the classes stay by equality
        assert _main(argv + summary + ["-e", "0", "--tile-dups"]).endswith(block.getvalue())
    assert "Tile duplication (Redundant/PF wells): " in with_classes
    assert "Local share at level 3 (Local/InClasses): " in with_classes
    assert "Exact duplication (Redundant/PF wells): " in with_classes


def test_cli_tile_dups_two_ranks(tmp_path):
    """torchrun, two ranks on GPU 0 (gloo): the widened rows go through the one merge; the report equals the
    single-process run's."""
    import socket
    _, _, _, argv = _cli_run(tmp_path)
    argv = argv + ["--dup-sets", "--tile-dups"]
    single = _main(argv)
    assert "DupSetsSummary: 1\tTiles: 2" in single and "TileDupsSummary: 1\tTiles: 2" in single
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
