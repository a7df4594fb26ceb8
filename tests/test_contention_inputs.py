"""What tests/contention_inputs.py promises of its reads, checked on the host with the references the GPU tests use:
the families give hundreds of unions on a dozen roots and classes of many wells, the chains are chains - one cycle
from step to step, one cluster at K = 1 - and descend where they are said to; the probe edge has the groups it says, at
representatives that share an entry."""
import numpy as np
import pytest

from contention_inputs import CENTRES, LANE_RUN, LI_PROBE, chain, families, filters, li_home, line_rings, probe_edge_index, split
from laneindex_ref import index_keys
from tiledups_ref import INVALID, codes_of
from tilenear_ref import distinct_reads, edges_all_pairs, tile_near_dups


def _planes(reads):
    return [np.ascontiguousarray(reads[:, c]) for c in range(reads.shape[1])]


@pytest.mark.parametrize("L", [13, 31])
def test_families_put_hundreds_of_unions_on_a_dozen_roots(L):
    n = 300
    reads, which = families(3, n, L)
    filt = filters(4, n)
    _, lvl_off, nbr = line_rings(n)
    assert 250 < int((filt & 1).sum()) < n and (filt >> 1).any()
    codes = codes_of(_planes(reads), n)
    class_lab, reps = distinct_reads(codes, (filt & 1).astype(bool))
    pf = class_lab != INVALID
    assert reps.size < pf.sum() - 40                                   # classes: many claims meet a slot that is taken
    assert np.bincount(class_lab[pf].astype(np.int64)).max() >= 8     # ... the centres' own reads, many wells each
    assert (codes == 4).any()
    for k in (1, 2, 3):
        edges = edges_all_pairs(codes, reps, k)
        row, labels = tile_near_dups(_planes(reads), filt, lvl_off, nbr, k)
        clusters = np.unique(labels[pf]).size
        assert reps.size - clusters >= (50 if k == 1 else 100)         # unions that merge two trees, at the least, in 300 wells
        assert edges.shape[0] >= reps.size - clusters and row[4] == edges.shape[0]
        if k == 3:
            # every read is within 3 of its centre: a family with its centre's read present is one cluster
            assert clusters <= 2 * CENTRES
            roots, size = np.unique(labels[pf], return_counts=True)
            assert (size >= 10).sum() >= CENTRES - 2
    # wells of one cluster at K = 3 mostly share a family (two centres are never 6 cycles apart by chance at L >= 13)
    assert np.unique(which).size == CENTRES


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("L", [13, 31])
def test_chains_are_chains(L, descending):
    n, length = 300, 100
    reads, wells = chain(5, n, L, length, descending)
    assert wells.size == length and np.unique(wells).size == length
    if descending:
        assert (np.diff(wells) < 0).all()
    else:
        assert (np.diff(wells) < 0).any() and (np.diff(wells) > 0).any()
    codes = codes_of(_planes(reads), n).T                              # [n, L]
    step = (codes[wells[1:]] != codes[wells[:-1]]).sum(axis=1)
    assert (step == 1).all()
    assert np.unique(codes[wells], axis=0).shape[0] == length          # no read of the chain comes twice
    filt = filters(6, n, keep=wells)
    assert (filt[wells] & 1).all()
    _, lvl_off, nbr = line_rings(n)
    row, labels = tile_near_dups(_planes(reads), filt, lvl_off, nbr, 1)
    assert (labels[wells] == wells.min()).all()                        # one cluster, whose label is its smallest well
    assert row[4] >= length - 1


def test_split_and_rings():
    reads, _ = families(1, 3 * 50, 13)
    filt = filters(2, 3 * 50)
    tiles, filts = split(reads, filt, 3)
    assert len(tiles) == 3 and all(t.shape == (50, 13) for t in tiles) and (np.concatenate(tiles) == reads).all()
    assert (np.concatenate(filts) == filt).all()
    centre, lvl_off, nbr = line_rings(5)
    assert centre.tolist() == [0, 1, 2, 3, 4] and lvl_off.shape == (5, 3)
    assert nbr[lvl_off[2, 0]:lvl_off[2, 1]].tolist() == [1, 3] and nbr[lvl_off[2, 1]:lvl_off[2, 2]].tolist() == [0, 4]
    assert nbr[lvl_off[0, 0]:lvl_off[0, 2]].tolist() == [1, 2]


@pytest.mark.parametrize("I", [8, 20])
@pytest.mark.parametrize("extra", [0, 1, 4])
def test_probe_edge_groups_share_an_entry(I, extra):
    n, groups = 9000, LI_PROBE + extra
    tiles, filts, reps, slot = probe_edge_index(300 + extra, n, I, groups)
    assert len(tiles) == 2 and all(t.shape == (n, I) for t in tiles) and all(f.shape == (n,) for f in filts)
    assert reps.size == groups and (np.diff(reps) > 0).all() and reps[-1] < LANE_RUN
    assert (li_home(reps) == slot).all() and 0 <= slot < 512
    keys, _ = index_keys([(t, [np.ascontiguousarray(x[:, c]) for c in range(I)]) for t, x in enumerate(tiles)], n, 2)
    pf = (np.concatenate(filts) & 1).astype(bool)
    assert not pf[:reps[0]].any() and pf[reps].all() and 0.85 * 2 * n < pf.sum() < 2 * n - reps[0]
    ukeys, first = np.unique(keys[pf], return_index=True)
    # exactly these groups, each with its representative where it was put, and wells enough behind each on both tiles
    assert ukeys.size == groups and sorted(np.flatnonzero(pf)[first].tolist()) == reps.tolist()
    for t in range(2):
        here = keys[t * n:(t + 1) * n][pf[t * n:(t + 1) * n]]
        assert np.unique(here).size == groups and np.unique(here, return_counts=True)[1].min() >= 100
    assert I <= 10 or (np.unique(keys >> np.uint64(32)).size > 1 and np.unique(keys & np.uint64(0xFFFFFFFF)).size > 1)
    assert (np.concatenate(filts) >> 1).any()                          # (only bit 0 counts)
