"""The scripted indel inputs of tests/lev2_scripts.py against the oracle (Levenshtein, k = 2, with distances), before
anything runs on a GPU: these are conditions on the INPUT, which the generator alone has to meet - the shifts that must
be there are there at every pair of boundary cycles and from both directions, enough pairs pass the screen and must
be refused behind it, enough are equal reads to the screen, the background holds no duplicates of its own, and no
scripted well fails the filter.  The counts the summary of the change quotes are printed."""
import numpy as np
import pytest

import lev2_scripts as ls
from oracle import oracle


def _text(codes):
    return "".join("ACGTN"[int(c)] for c in codes)


@pytest.mark.parametrize("L", ls.LENGTHS)
def test_scripts_meet_their_conditions(L):
    case = ls.generate(L)
    exp = ls.expected(L)
    centre, lvl_off, nbr = case.csr
    n = centre.shape[0]
    assert len(case.tiles) == 3 and n == 2400 and lvl_off.shape[1] - 1 == 3
    wells = [(p.tile, x) for p in case.pairs for x in (p.w, p.v)]
    assert len(set(wells)) == len(wells)                                     # scripted wells are distinct
    lower = sum(p.v < p.w for p in case.pairs)
    assert min(lower, len(case.pairs) - lower) >= len(case.pairs) // 2 - 2   # alternately below and above w

    # tiles 0 and 1 cannot overflow a survivor queue of 64 (the screen restated: test_properties checks the same
    # restatement against the distance), so with "dense_pack" 0 lev2_gather decides their survivors; tile 2 can
    for ti in ls.GATHER_TILES:
        assert ls.queue_bound(case, ti) <= ls.QUEUE_MAX, (L, ti, ls.queue_bound(case, ti))
    assert ls.queue_bound(case, 2) > ls.QUEUE_MAX

    exact2 = {}                      # (p, t, direction) -> pairs at distance exactly 2 with >= 3 mismatching cycles
    n_exact2 = n_behind = n_tail = 0
    for pr in case.pairs:
        tile = case.tiles[pr.tile]
        valid, dups, lens, dist = exp[pr.tile]
        assert tile.filt[pr.w] & 1 and tile.filt[pr.v] & 1 and valid[pr.w] and valid[pr.v]
        a, b = tile.codes[pr.w], tile.codes[pr.v]
        d = int(dist[ls.slot_of(case, pr.w, pr.v)])
        assert d == int(dist[ls.slot_of(case, pr.v, pr.w)]) >= 0             # the pair is in both wells' rings
        mism = np.flatnonzero(a != b)
        n_exact2 += d == 2
        if d == 2 and mism.size >= 3 and pr.direction is not None and mism[0] == pr.p and mism[-1] == pr.t \
                and pr.tile in ls.GATHER_TILES:
            exact2[(pr.p, pr.t, pr.direction)] = exact2.get((pr.p, pr.t, pr.direction), 0) + 1
        if L > ls.SCREEN:
            fa, fb = _text(a[:ls.SCREEN]).replace("N", "A"), _text(b[:ls.SCREEN]).replace("N", "A")
            n_behind += d >= 3 and oracle.levenshtein(fa, fb) <= 2
            n_tail += mism.size > 0 and mism[0] >= ls.SCREEN
    B = ls.boundary_set(L)
    for p in B:
        for t in B:
            if t - p >= 4:
                for direction in ("up", "down"):
                    assert exact2.get((p, t, direction), 0) >= 1, (L, p, t, direction)
    if L > ls.SCREEN:
        assert n_behind >= 30 and n_tail >= 30, (L, n_behind, n_tail)
    print("L %d: %d scripted pairs, %d at distance exactly 2, %d pass the screen at distance >= 3, "
          "%d with the first mismatch at cycle 16 or later" % (L, len(case.pairs), n_exact2, n_behind, n_tail))

    # the background: nothing within distance 2 but the scripts and what tile 2's shared prefix produces
    slots = np.arange(nbr.shape[0])
    slot_c = np.searchsorted(lvl_off[:, 0], slots, side="right") - 1
    for ti, tile in enumerate(case.tiles):
        owner = np.full(n, -1)
        for j, pr in enumerate(case.pairs):
            if pr.tile == ti:
                owner[pr.w] = owner[pr.v] = j
        dist = exp[ti][3]
        near = (dist >= 0) & (dist <= 2) & ~((owner[slot_c] >= 0) & (owner[slot_c] == owner[nbr]))
        assert ti == 2 or not near.any(), (L, ti, int(near.sum()))
        assert (tile.shared[slot_c[near]] & tile.shared[nbr[near]]).all(), (L, ti)
        assert 0.01 < 1 - (tile.filt & 1).mean() < 0.05                      # 3 % of the wells fail the filter
        if ti == 2:
            assert (tile.shared[slot_c] & tile.shared[nbr]).sum() > 2000     # the screen passes pairs in bulk there


def test_closed_form_of_the_generator_equals_the_oracle():
    """closed_form only steers the redraws; it must not steer them wrongly: every neighbour pair of one case."""
    case = ls.generate(17)
    centre, lvl_off, nbr = case.csr
    slot_c = np.searchsorted(lvl_off[:, 0], np.arange(nbr.shape[0]), side="right") - 1
    for tile, (valid, dups, lens, dist) in zip(case.tiles, ls.expected(17)):
        got = ls.closed_form(tile.codes[slot_c], tile.codes[nbr])
        ok = dist >= 0
        assert (got[ok] == np.minimum(dist[ok], 3)).all()
