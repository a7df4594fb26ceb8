"""The injected graphs of tests/dupsets_graphs.py without a GPU: the host union-find against scipy's connected
components on every family, the vectorised edge builder against edges_from_reads with the oracle's distances, the
self-naming well by the header's definition, and every family's non-degeneracy at the GPU tests' own size."""
import numpy as np
import pytest

import dupsets_graphs as dg
from dupsets_ref import INVALID, dup_sets, edges_from_reads, read_strings
from oracle import oracle

SMALL_N = 1003              # not a multiple of 8: the last three wells have no filler of their own and name the last one
GPU_N = 70000


@pytest.fixture(scope="module", params=dg.CASES)
def small_case(request):
    return dg.make_case(request.param, SMALL_N, levels=8 if not request.param.startswith("corners") else 4)


def test_reference_against_scipy_on_every_family(small_case):
    sparse = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    case, n, levels = small_case, small_case.n, small_case.levels
    for mode in (0, 1):
        rows, labels = case.reference(mode)
        for tile, row, lab in zip(case.tiles, rows, labels):
            a, b, lev = dg.edges_from_colours(tile, case.csr, mode)
            loops = a == b
            for l in range(levels):
                m = (lev <= l) & ~loops
                g = sparse.coo_matrix((np.ones(m.sum()), (a[m], b[m])), shape=(n, n))
                _, comp = csgraph.connected_components(g, directed=False)
                sizes = np.bincount(comp[tile.pf], minlength=comp.max() + 1)
                assert row[1 + l] == (sizes >= 2).sum()
                assert row[1 + levels + l] == sizes[sizes >= 2].sum()
            smallest = np.full(comp.max() + 1, n, dtype=np.int64)         # outermost level: labels are component minima
            np.minimum.at(smallest, comp, np.arange(n))
            assert (lab[tile.pf] == smallest[comp][tile.pf]).all() and (lab[~tile.pf] == INVALID).all()
            dg.check_row(row, levels)


@pytest.mark.parametrize("mode,k", dg.METRICS)
def test_vectorised_edges_equal_edges_from_reads(small_case, mode, k):
    case = small_case
    dist = oracle.hamming if mode == 1 else oracle.levenshtein
    for tile in case.tiles[:2]:
        want = edges_from_reads(read_strings(tile.planes(), case.n), tile.pf, case.csr[1], case.csr[2], mode, k, dist)
        got = dg.edges_from_colours(tile, case.csr, mode)
        assert sorted(zip(*(x.tolist() for x in got))) == sorted(zip(*(x.tolist() for x in want)))
        assert got[0].shape[0] > 0


def test_colours_are_far_apart_and_mutations_near():
    tile = dg.tile_random(64, 1, knock=0.0, mutate=0.5, stretch=8)
    seqs = read_strings(tile.planes(), 64)
    assert len(set(seqs)) > 4 and all(len(s) == dg.L and "N" not in s for s in seqs)
    for i in range(64):
        for j in range(i):
            d = (oracle.hamming(seqs[i], seqs[j]), oracle.levenshtein(seqs[i], seqs[j]))
            if tile.colour[i] == tile.colour[j]:
                assert d[0] == d[1] == int(tile.mut[i] != tile.mut[j])
            else:
                assert min(d) > 3


def test_self_naming_well_is_in_no_set():
    """include/welldup_sets.h: a set is a component of at least two wells."""
    row, labels = dup_sets(6, np.ones(6, bool), [2, 4, 4], [2, 4, 5], [0, 0, 1], 2)
    pf, sets, in_sets, red, bins = dg.split_row(row, 2)
    assert sets.tolist() == [0, 1] and in_sets.tolist() == [0, 2] and red.tolist() == [0, 1]
    assert bins.sum() == sets[-1] and labels.tolist() == [0, 1, 2, 3, 4, 4]
    case = dg.make_case("corners", SMALL_N, levels=4)
    a, b, lev = dg.edges_from_colours(case.tiles[0], case.csr, 1)
    assert ((a == dg.CORNER_SELF) & (b == dg.CORNER_SELF)).sum() == 1             # the edge builder still reports it
    rows, labels = case.reference(1)
    assert labels[0][dg.CORNER_SELF] == dg.CORNER_SELF
    assert (rows[0][-8:].sum() == rows[0][4]) and rows[0][1 + 4] == 7             # InSets[0]: the self-namers not counted


def test_csr_declarations():
    a, b, lev = dg.gnm(SMALL_N, 8, 2, 9)
    one, sym = dg.to_csr(SMALL_N, 8, a, b, lev, False), dg.to_csr(SMALL_N, 8, a, b, lev, True)
    assert not dg.is_symmetric(one) and dg.is_symmetric(sym)
    for csr in (one, sym):
        assert (np.diff(csr[1], axis=1) >= 1).all() and (csr[0] == np.arange(SMALL_N)).all()
    t, l = dg.slots_of(one)
    named = set(zip(t.tolist(), one[2].tolist(), l.tolist()))
    assert set(zip(a.tolist(), b.tolist(), lev.tolist())) <= named
    fill = dg.is_filler(SMALL_N)
    assert all(fill[w] for (u, w, _) in named - set(zip(a.tolist(), b.tolist(), lev.tolist())))
    # both declarations of a graph are one graph: the same sets
    tile = dg.tile_random(SMALL_N, 3)
    r1 = dup_sets(SMALL_N, tile.pf, *dg.edges_from_colours(tile, one, 1), 8)
    r2 = dup_sets(SMALL_N, tile.pf, *dg.edges_from_colours(tile, sym, 1), 8)
    assert (r1[0] == r2[0]).all() and (r1[1] == r2[1]).all()


@pytest.mark.parametrize("name", dg.CASES)
def test_families_are_not_degenerate_at_the_gpu_size(name):
    dg.check_nondegenerate(dg.make_case(name, GPU_N))


def test_ladder_of_sixteen_levels():
    case = dg.make_case("ladder-one", GPU_N, levels=16)
    dg.check_nondegenerate(case)
    assert dg.split_row(case.reference(1)[0][0], 16)[1][-1] == 1
