"""Duplicate sets on the GPU (wd_dup_sets) over injected graphs (tests/dupsets_graphs.py): paths, stars, ladders,
late merges of large components, every size bin, multigraph corners and random graphs, as targets over 70 000
wells whose reads and filters make named pairs duplicates at will.  What a honeycomb with planted duplicates
never produces - long parent paths, thousands of hooks on one root, components merging at a late level, tiles
interleaved in the hit log - against the host union-find over edges built from the reads, and the scan's own
counters against the oracle.  Everything is equal or it is wrong: no tolerance anywhere."""
import numpy as np
import pytest

import dupsets_graphs as dg
from helpers import blocks_to_reference
from oracle import oracle
from well_duplicates_amd.scanner import Scanner, TileBatch

pytestmark = pytest.mark.gpu

N = 70000           # just over the 65 536 targets at which dense_kernel = -1 takes the dense chain; not a multiple of 64
L = dg.L
DENSE = (1, 0, -1)


@pytest.fixture(scope="module")
def sc():
    s = Scanner(0)
    yield s
    s.set_option("dense_kernel", -1)
    s.close()


_cases = {}


def _case(name, levels=8):
    """One reference per case and module (the host union-find over 70 000 wells takes a few tenths of a second)."""
    key = (name, levels)
    if key not in _cases:
        case = dg.make_case(name, N, levels)
        case.planes = [t.planes() for t in case.tiles]
        case.blocks = {}
        _cases[key] = case
    return _cases[key]


def _want_blocks(case, mode, k):
    """The scan's own counter rows from the oracle (they count the pairs with fillers too)."""
    if (mode, k) not in case.blocks:
        rows = []
        for tile, planes in zip(case.tiles, case.planes):
            valid, dups, lens, _ = oracle.count_tile(planes, tile.filter(), *case.csr, mode, k)
            rows.append(oracle.tally_tile(valid, dups, lens))
        case.blocks[(mode, k)] = np.array(rows)
    return case.blocks[(mode, k)]


def _batch(sc, case, tiles=None):
    tiles = range(len(case.tiles)) if tiles is None else tiles
    sc.set_targets(*case.csr)
    tb = TileBatch(sc, len(tiles), L, N)
    for slot, i in enumerate(tiles):
        tb.upload_tile(slot, case.planes[i], case.tiles[i].filter())
    return tb


def _check_device_rows(tb, blocks, rows, levels):
    for row in rows:
        dg.check_row(row, levels)
    assert tb.edges == blocks[:, 1 + levels:1 + 2 * levels].sum()


def _parity(sc, case, metrics=dg.METRICS, dense=DENSE):
    levels = case.levels
    k_max = int((case.csr[1][:, -1] - case.csr[1][:, 0]).max())
    tb = _batch(sc, case)
    try:
        for mode, k in metrics:
            want_rows, want_labels = case.reference(mode)
            want_blocks = _want_blocks(case, mode, k)
            for d in dense:
                sc.set_option("dense_kernel", d)
                blocks, rows, labels = tb.dup_sets(mode, k, labels=True)
                what = (case.name, mode, k, d, sc.last_kernel())
                assert (labels == want_labels).all(), (what, np.flatnonzero((labels != want_labels).any(axis=0))[:10])
                assert (rows == want_rows).all(), (what, rows, want_rows)
                ref_blocks = np.array([blocks_to_reference(b, levels) for b in blocks])
                assert (ref_blocks == want_blocks).all(), what
                _check_device_rows(tb, blocks, rows, levels)
                if d != 0 and k <= 2 and levels <= 8:
                    assert sc.last_kernel().startswith("dense chain"), what
                    assert sc.get_option("dense_sym_on") == (1 if case.symmetric else 0), what
                else:
                    # the queue kernel, or - a target of more slots than its four passes hold - the general one
                    assert sc.last_kernel().startswith("k_scan_q" if k_max <= 4 * 127 else "k_scan<"), what
                b2, r2, l2 = tb.dup_sets(mode, k, labels=True)                    # the same call again
                assert (b2 == blocks).all() and (r2 == rows).all() and (l2 == labels).all(), what
    finally:
        sc.set_option("dense_kernel", -1)
        tb.free()


@pytest.mark.parametrize("name", dg.CASES)
def test_sets_match_reference_on_injected_graph(sc, name):
    """Every family and declaration: four metrics; the dense chain (forced and by itself) and, with it off, the
    queue kernel (the general kernel where a hub has more slots than that one takes) as the edge source, each
    kernel asserted by name; each call twice."""
    case = _case(name)
    dg.check_nondegenerate(case)
    _parity(sc, case)


def test_sets_ladder_of_sixteen_levels(sc):
    """Beyond the dense chain's eight levels: the queue kernel alone, the per-level counters up to 16."""
    case = _case("ladder-one", 16)
    assert dg.split_row(case.reference(1)[0][0], 16)[1].tolist() == [-(-61250 // (2 << l)) for l in range(16)]
    _parity(sc, case, dense=(-1, 0))


def test_sets_self_naming_well_is_in_no_set(sc):
    """include/welldup_sets.h: a set has at least two wells.  The scan still counts the well's record."""
    case = _case("corners")
    tb = _batch(sc, case, tiles=[0])
    try:
        for d in DENSE:
            sc.set_option("dense_kernel", d)
            blocks, rows, labels = tb.dup_sets(1, 2, labels=True)
            pf, sets, in_sets, red, bins = dg.split_row(rows[0], case.levels)
            assert labels[0][dg.CORNER_SELF] == dg.CORNER_SELF and labels[0][dg.CORNER_SELF_IN_SET + 1] == dg.CORNER_SELF_IN_SET
            assert bins.sum() == sets[-1] == 4 and in_sets.tolist() == [7, 7] + [9] * (case.levels - 2)
            assert tb.edges == blocks[0][1 + case.levels:1 + 2 * case.levels].sum()  # the records are all there
            assert (blocks_to_reference(blocks[0], case.levels) == _want_blocks(case, 1, 2)[0]).all()
    finally:
        sc.set_option("dense_kernel", -1)
        tb.free()


@pytest.mark.parametrize("name", ["star-last", "star-sym-last"])
def test_sets_star_regrowth_under_contention(sc, name):
    """A first capacity of 16 edges on the star (every hook on one word): the sizing retry gives what the
    automatic capacity gives."""
    case = _case(name)
    tb = _batch(sc, case)
    try:
        for mode, k in ((0, 0), (2, 2)):
            out = []
            for cap in (0, 16):
                blocks, rows, labels = tb.dup_sets(mode, k, labels=True, edge_cap=cap)
                out.append((blocks, rows, labels, np.array(tb.edges)))
            assert out[1][3] > 60000
            for a, b in zip(out[0], out[1]):
                assert (a == b).all()
            assert (out[0][1] == case.reference(mode)[0]).all() and (out[0][2] == case.reference(mode)[1]).all()
    finally:
        tb.free()


@pytest.mark.parametrize("name", ["merge-one", "gnm2-sym-s4"])
def test_sets_batch_equals_tiles_one_by_one(sc, name):
    """Three tiles in one hit log, or each tile alone: the same rows and labels."""
    case = _case(name)
    tb = _batch(sc, case)
    try:
        got = {m: tb.dup_sets(*m, labels=True) for m in ((0, 0), (1, 2))}
    finally:
        tb.free()
    for i in range(len(case.tiles)):
        one = _batch(sc, case, tiles=[i])
        try:
            for (mode, k), (blocks, rows, labels) in got.items():
                b, r, lab = one.dup_sets(mode, k, labels=True)
                assert (b[0] == blocks[i]).all() and (r[0] == rows[i]).all() and (lab[0] == labels[i]).all(), (name, i, mode)
                assert (r[0] == case.reference(mode)[0][i]).all()
        finally:
            one.free()
