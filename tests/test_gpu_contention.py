"""The class table and the union-find of the near-duplicate passes under contention on the GPU: the reads of
tests/contention_inputs.py - families of hundreds of equal and near reads on a dozen roots, chains of 100 reads whose
every union meets a fresh root - through TileBatch.tile_dups / tile_near_dups and LaneDups (tiles added in several
orders, split over calls), against the host references of tests/tiledups_ref.py, tilenear_ref.py, lanedups_ref.py
and lanenear_ref.py: rows and labels equal, nothing approximate.  The other GPU tests plant pairs and short chains,
which make few unions or none on a common root; tests/test_near_emu.py and tests/test_readclasses_emu.py run the
same kinds of reads through the kernels' sources on the CPU, where the order of the lanes can be chosen."""
import numpy as np
import pytest

from contention_inputs import chain, families, filters, line_rings, split
from lanedups_ref import check_identities, lane_dups
from lanenear_ref import NEAR_PAIRS, check_near_identities, lane_near_dups
from tiledups_ref import INVALID, tile_dups
from tilenear_ref import tile_near_dups
from well_duplicates_amd.scanner import LaneDups, Scanner, TileBatch

pytestmark = pytest.mark.gpu

N_TILES = 3
INDEX = [0, 2, 3]                                  # slot -> tile index, ascending: ids descend along a descending chain
MAX_TILES = 5                                      # (indices 1 and 4 are never added)
WAYS = {"one call": [[0, 1, 2]], "a tile per call, descending": [[2], [1], [0]], "2 + 1": [[1, 2], [0]]}
KINDS = ("families", "chain_permuted", "chain_descending")
SHAPES = [(n, L) for n in (300, 4099) for L in (13, 31)]      # a full workgroup and a partial one; 16 and a bit


@pytest.fixture(scope="module")
def sc():
    s = Scanner(0)
    yield s
    s.close()


def _space(kind, seed, n, L):
    """-> (reads [n, L], filter [n]) of one id space"""
    if kind == "families":
        return families(seed, n, L)[0], filters(seed + 1, n)
    reads, wells = chain(seed, n, L, 100, descending=kind == "chain_descending")
    return reads, filters(seed + 1, n, keep=wells)


def _planes(reads):
    return [np.ascontiguousarray(reads[:, c]) for c in range(reads.shape[1])]


def _upload(sc, reads, filts):
    tb = TileBatch(sc, len(reads), reads[0].shape[1], reads[0].shape[0])
    for i, (r, f) in enumerate(zip(reads, filts)):
        tb.upload_tile(i, _planes(r), f)
    return tb


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("n,L", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_tile_classes_and_clusters_under_contention(sc, kind, n, L, k):
    """Every tile an id space of its own; hash_bits 0, 4 and 1 (two slots per segment for all vertices of a tile)."""
    centre, lvl_off, nbr = line_rings(n)
    sc.set_targets(centre, lvl_off, nbr)
    spaces = [_space(kind, 100 * k + 10 * t + L, n, L) for t in range(N_TILES)]
    reads, filts = [s[0] for s in spaces], [s[1] for s in spaces]
    want_eq = [tile_dups(_planes(r), f, lvl_off, nbr) for r, f in zip(reads, filts)]
    want = [tile_near_dups(_planes(r), f, lvl_off, nbr, k) for r, f in zip(reads, filts)]
    for t in range(N_TILES):                       # the inputs do what they are for
        pf = want[t][1] != INVALID
        classes = np.unique(want_eq[t][1][pf]).size
        unions = classes - np.unique(want[t][1][pf]).size
        assert unions >= (50 if kind == "families" else 99) and want[t][0][4] >= unions
    tb = _upload(sc, reads, filts)
    try:
        for bits in (0, 4, 1):
            rows, labels = tb.tile_dups(labels=True, hash_bits=bits)
            for t in range(N_TILES):
                assert (labels[t] == want_eq[t][1]).all(), (bits, t)
                assert (rows[t] == want_eq[t][0]).all(), (bits, t, rows[t], want_eq[t][0])
            rows, labels = tb.tile_near_dups(k, labels=True, hash_bits=bits, pair_budget=1 << 40 if bits else 0)
            for t in range(N_TILES):
                assert (labels[t] == want[t][1]).all(), (bits, t)
                assert (rows[t] == want[t][0]).all(), (bits, t, rows[t], want[t][0])
    finally:
        tb.free()


def _feed(sc, tb, calls, k, hash_bits):
    """calls: a list of lists of batch slots, one wd_lane_dups_add each -> LaneDups.finish(hamming=k)"""
    ld = LaneDups(sc, tb.N, MAX_TILES, tb.L, hash_bits=hash_bits)
    try:
        ptrs = tb.plane_ptrs()
        for slots in calls:
            ld.add_tables([INDEX[s] for s in slots],
                          Scanner._tables([ptrs[s] for s in slots], [tb.filter_ptr(s) for s in slots], tb.L))
        # (a masked fingerprint holds every read of the lane in 2 or 16 buckets - or fewer: the low bits of the fold of a
        # segment that lies high in its 30-bit word hardly differ - which is over the default budget on 12 000 reads)
        return ld.finish(labels=True, hamming=k, pair_budget=1 << 27 if hash_bits else 0)
    finally:
        ld.close()


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("n,L", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_lane_classes_and_clusters_under_contention(sc, kind, n, L, k):
    """The three tiles end to end are one id space: families and chains run across the tiles, and a descending chain
    descends in global ids whatever the order the tiles are added in."""
    reads, filt = _space(kind, 200 * k + L, N_TILES * n, L)
    reads, filts = split(reads, filt, N_TILES)
    tiles = [(INDEX[s], _planes(reads[s]), filts[s]) for s in range(N_TILES)]
    want_eq = lane_dups(tiles, n, MAX_TILES)
    want = lane_near_dups(tiles, n, MAX_TILES, k)
    assert want[0][NEAR_PAIRS] >= (50 if kind == "families" else 99)                        # the inputs do what they are for
    assert want[0][4] >= 1                                                                  # clusters across tiles
    assert (want[2][[1, 4]] == INVALID).all()
    tb = _upload(sc, reads, filts)
    try:
        for bits in (0, 4, 1):
            for name, calls in WAYS.items():
                lane, trow, labels, near_lane, near_tiles, near_labels = _feed(sc, tb, calls, k, bits)
                assert (labels == want_eq[2]).all(), (bits, name)
                assert (lane == want_eq[0]).all() and (trow == want_eq[1]).all(), (bits, name, lane, want_eq[0])
                assert (near_labels == want[2]).all(), (bits, name)
                assert (near_lane == want[0]).all() and (near_tiles == want[1]).all(), (bits, name, near_lane, want[0])
                check_identities(lane, trow)
                check_near_identities(near_lane, near_tiles)
    finally:
        tb.free()
