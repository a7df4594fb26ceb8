"""The dense chain's Levenshtein <= 2 on scripted indels (tests/lev2_scripts.py): one deletion plus one insertion
with the first mismatch p and the last mismatch t on every pair of boundary cycles - the 8 + 2 split of sig_codes,
the end of the signature word, of the screen word, the row's chunks and groups, the ballot words of lev2_gather, the
read's last chunk and cycle - from both wells of a pair, beside pairs that pass the screen and must be refused behind
it (k_dense_mark's strike, k_dense_verify), pairs that are equal reads to the screen, and a tile whose shared prefix
floods the survivor queues.  Every combination of one-ended / two-ended compare, packed rows / planes (row_lev2 /
lev2_gather), LDS windows / gather, default queue / a queue of 3 (the overflow loop of k_dense_verify, with
lev2_window in it for L <= 10) against the oracle: per-target counts, tallies, and the hit log with the distances;
and tiles 0 and 1 alone on the planes under a queue of 64, which they cannot overflow, so that lev2_gather decides.
tests/test_lev2_scripts_host.py checks the inputs themselves; tests/test_dense_forms.py the closed forms on the CPU."""
import numpy as np
import pytest

import lev2_scripts as ls
from helpers import blocks_to_reference
from oracle import oracle
from well_duplicates_amd.scanner import INVALID_TARGET, Scanner, TileBatch

pytestmark = pytest.mark.gpu

OPTIONS = ("dense_kernel", "dense_pack", "dense_windows", "dense_queue_cap", "dense_sym", "line_walk")


@pytest.fixture(scope="module")
def sc():
    s = Scanner(0)
    s.defaults = [(name, s.get_option(name)) for name in OPTIONS]      # the library's own, read back
    yield s
    s.close()


def restore(sc):
    sc.hitlog_enable(0)
    for name, v in sc.defaults:
        sc.set_option(name, v)


_want = {}


def want(L):
    """Per tile (per-target counts with -1 for invalid centres, tally block), the hits of all tiles as sorted
    (tile, target, slot, dist), and the scripted pairs' share of them - from the oracle, once per L."""
    if L not in _want:
        case = ls.generate(L)
        centre, lvl_off, nbr = case.csr
        slots = np.arange(nbr.shape[0])
        tgt = np.searchsorted(lvl_off[:, 0], slots, side="right") - 1
        tiles, hits = [], []
        for i, (valid, dups, lens, dist) in enumerate(ls.expected(L)):
            tiles.append((np.where(valid[:, None] == 1, dups, -1), oracle.tally_tile(valid, dups, lens)))
            ok = (valid[tgt] == 1) & (dist <= 2)
            hits += [(i, int(t), int(p), int(dist[p])) for t, p in zip(tgt[ok], slots[ok])]
        # what the hit log must say of the scripted pairs: (record, whether it is there) for both wells of each
        # (target t's centre is well t)
        scripted = []
        for p in case.pairs:
            d = int(ls.expected(L)[p.tile][3][ls.slot_of(case, p.w, p.v)])
            scripted += [((p.tile, x, ls.slot_of(case, x, y), d), d <= 2, p) for x, y in ((p.w, p.v), (p.v, p.w))]
        assert sum(there for _, there, _ in scripted) > 0
        _want[L] = (tiles, sorted(hits), scripted)
    return _want[L]


def compare(case, blocks, pt, what, n_tiles=None):
    """the first n_tiles tiles (all of them by default) of a batch against the oracle"""
    tiles = want(case.L)[0][:n_tiles]
    levels = case.csr[1].shape[1] - 1
    assert blocks.shape[0] == pt.shape[0] == len(tiles)
    for i, (counts, tally) in enumerate(tiles):
        got = pt[i].astype(np.int64)
        got[got == INVALID_TARGET] = -1
        bad = np.flatnonzero((got != counts).any(axis=1))
        assert bad.size == 0, (what, i, [(int(w), got[w].tolist(), counts[w].tolist(), scripts_at(case, i, int(w))) for w in bad[:8]])
        assert (blocks_to_reference(blocks[i], levels) == tally).all(), (what, i)


def scripts_at(case, tile, well):
    """the scripted pairs a well takes part in: the (L, p, t, kind) cell of a failure"""
    return [repr(p) for p in case.pairs if p.tile == tile and well in (p.w, p.v)]


def upload(sc, case, n_tiles=None):
    tiles = case.tiles[:n_tiles]
    tb = TileBatch(sc, len(tiles), case.L, case.csr[0].shape[0])
    for i, t in enumerate(tiles):
        tb.upload_tile(i, t.planes, t.filt)
    return tb


@pytest.mark.parametrize("L", ls.LENGTHS)
def test_dense_chain_on_scripted_indels(sc, L):
    case = ls.generate(L)
    _, want_hits, scripted = want(L)
    cap = len(want_hits) + 64
    tb = upload(sc, case)
    # tiles 0 and 1 alone: one overflowing queue (tile 2 has many) turns the whole batch to packed rows, and
    # lev2_gather would see no pair; these two cannot overflow a queue of 64 (test_lev2_scripts_host.py)
    assert ls.GATHER_TILES == (0, 1)
    tbg = upload(sc, case, 2)
    gather_hits = [h for h in want_hits if h[0] < 2]
    try:
        sc.set_option("dense_kernel", 1)
        for sym in (1, 0):
            sc.set_option("dense_sym", sym)
            sc.set_targets(*case.csr)
            for windows in (1, 0):
                what = (L, "tiles 0 and 1", "sym", sym, "pack", 0, "windows", windows, "queue_cap", ls.QUEUE_MAX)
                sc.set_option("dense_pack", 0)
                sc.set_option("dense_windows", windows)
                sc.set_option("dense_queue_cap", ls.QUEUE_MAX)
                sc.hitlog_enable(cap)
                blocks, pt = tbg.count(2, 2, per_target=True)
                hits, total = sc.hitlog_fetch(cap)
                compare(case, blocks, pt, what, 2)
                assert sc.last_kernel().startswith("dense chain") and sc.get_option("dense_sym_on") == sym, what
                got = sorted((int(h["tile"]), int(h["target"]), int(h["slot"]), int(h["dist"])) for h in hits)
                assert total == len(gather_hits) and got == gather_hits, (what, total, len(gather_hits))
            for pack in (-1, 0, 1):
                for windows in (1, 0):
                    for qcap in (0, 3):
                        what = (L, "sym", sym, "pack", pack, "windows", windows, "queue_cap", qcap)
                        sc.set_option("dense_pack", pack)
                        sc.set_option("dense_windows", windows)
                        sc.set_option("dense_queue_cap", qcap)
                        sc.hitlog_enable(cap if qcap == 0 else 0)
                        blocks, pt = tb.count(2, 2, per_target=True)
                        compare(case, blocks, pt, what)
                        assert sc.last_kernel().startswith("dense chain"), (what, sc.last_kernel())
                        assert sc.get_option("dense_sym_on") == sym, what
                        groups = sc.get_option("dense_window_groups")
                        assert (groups > 0) if windows else (groups == 0), (what, groups)
                        if qcap == 0:
                            hits, total = sc.hitlog_fetch(cap)
                            got = sorted((int(h["tile"]), int(h["target"]), int(h["slot"]), int(h["dist"])) for h in hits)
                            assert total == len(want_hits) and got == want_hits, (what, total, len(want_hits))
                            # ... in particular a scripted pair within 2 is recorded at both of its wells, with the
                            # distance the textbook DP gives
                            seen = set(got)
                            for record, there, p in scripted:
                                assert (record in seen) == there, (what, p, record)
    finally:
        restore(sc)
        tb.free()
        tbg.free()


def test_scripted_indels_through_an_unaligned_pointer_table(sc):
    """The same tiles (L = 43) behind a table of plane pointers at odd addresses, n + 7 bytes apart: k_dense_sig builds
    the signature and screen words well by well, the pack kernel takes its byte path.  Same blocks and counts."""
    L = 43
    case = ls.generate(L)
    n = case.csr[0].shape[0]
    tb = upload(sc, case)
    slab = sc.malloc(len(case.tiles) * L * (n + 7) + 64)
    try:
        ptrs = [[slab + 3 + (i * L + c) * (n + 7) for c in range(L)] for i in range(len(case.tiles))]
        for i, t in enumerate(case.tiles):
            for c in range(L):
                sc.h2d(ptrs[i][c], t.planes[c])
        sc.set_targets(*case.csr)
        sc.set_option("dense_kernel", 1)
        for pack in (-1, 0, 1):
            sc.set_option("dense_pack", pack)
            blocks, pt = sc.count_tiles(ptrs, tb.filter_ptrs(), n, 2, 2, per_target=True)
            assert sc.last_kernel().startswith("dense chain"), sc.last_kernel()
            compare(case, blocks, pt, ("pointer table", "pack", pack))
            b2, p2 = tb.count(2, 2, per_target=True)                        # the strided layout
            assert (b2 == blocks).all() and (p2 == pt).all()
    finally:
        restore(sc)
        sc.free(slab)
        tb.free()


def test_scripted_indels_outside_the_dense_chain(sc):
    """The same tiles (L = 43) with the dense chain switched off, target by target and pair by pair in the order of
    the neighbour wells: whatever kernels the dispatcher picks use lev2_stream.inc on their own and must agree too."""
    L = 43
    case = ls.generate(L)
    tb = upload(sc, case)
    try:
        sc.set_targets(*case.csr)
        sc.set_option("dense_kernel", 0)
        for walk in (0, 1):
            sc.set_option("line_walk", walk)
            blocks, pt = tb.count(2, 2, per_target=True)
            assert not sc.last_kernel().startswith("dense chain"), sc.last_kernel()
            compare(case, blocks, pt, ("dense_kernel 0", "line_walk", walk, sc.last_kernel()))
    finally:
        restore(sc)
        tb.free()
