"""The ring generator's edge cases (tests/genrings_cases.py) on the host: the project's vectorised generator
(cluster_indexes.generate) equals the plain reference at every one of them - its sha256 fixtures
(tests/test_synth_and_generator.py) only cover honeycombs -, and the cases tell the reference from each of its mutants:
a window one record shorter or longer on either side, `<` for `<=` and back at either bound of a ring, distances in
float32.  A case set that cannot has not tested what it is there for."""
import numpy as np
import pytest

import genrings_cases as gc
from well_duplicates_amd import cluster_indexes

# mutant -> (its knobs, the case that catches it)
MUTANTS = {
    "low_reach_minus_1": (dict(reach_lo=gc.WINDOW - 1), "window"),
    "low_reach_plus_1": (dict(reach_lo=gc.WINDOW + 1), "window"),
    "high_reach_minus_1": (dict(reach_hi=gc.WINDOW - 1), "window"),
    "high_reach_plus_1": (dict(reach_hi=gc.WINDOW + 1), "window"),
    "inner_bound_le": (dict(inner_le=True), "boundaries"),
    "outer_bound_lt": (dict(outer_lt=True), "boundaries"),
    "float32_distance": (dict(f32=True), "largest_radius"),
}


def _same(a, b):
    return all(u.shape == v.shape and (u == v).all() for u, v in zip(a, b))


@pytest.mark.parametrize("name", gc.NAMES)
def test_numpy_generator_equals_plain_reference(name):
    case = gc.case(name)
    centres = gc.centres_of(case)
    if case.error == "empty":
        with pytest.raises(RuntimeError):
            cluster_indexes.generate(case.x, case.y, centres, case.levels, case.max_dists)
        return
    got = cluster_indexes.generate(case.x, case.y, centres, case.levels, case.max_dists)
    assert [c for c, _ in got] == centres
    assert _same(gc.csr_of(centres, [[r.tolist() for r in rings] for _, rings in got], case.levels), case.want)
    assert all((np.diff(r) > 0).all() for _, rings in got for r in rings)


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_cases_tell_the_reference_from_its_mutants(mutant):
    knobs, name = MUTANTS[mutant]
    case = gc.case(name)
    try:
        changed = not _same(gc.brute_csr(case, **knobs), case.want)
    except RuntimeError:
        changed = True
    assert changed, (mutant, name)


def test_what_each_window_and_boundary_mutant_changes():
    """The mutants' own results at the cases that catch them: which record, which well."""
    w, c = gc.case("window"), gc.WINDOW + 2
    ring = lambda **k: gc.brute_rings(w.x, w.y, c, 1, w.max_dists, **k)[0]
    assert ring() == [2, c + 1, c + gc.WINDOW + 1]
    assert ring(reach_lo=gc.WINDOW - 1) == [c + 1, c + gc.WINDOW + 1]
    assert ring(reach_lo=gc.WINDOW + 1) == [1, 2, c + 1, c + gc.WINDOW + 1]
    assert ring(reach_hi=gc.WINDOW - 1) == [2, c + 1]
    assert ring(reach_hi=gc.WINDOW + 1) == [2, c + 1, c + gc.WINDOW + 1, c + gc.WINDOW + 2]
    # the clamped variants tell the same mutants apart wherever the bound in question lies inside the table
    for name in ("window_centre_0", "window_centre_%d" % gc.WINDOW, "window_centre_%d" % (gc.WINDOW + 1),
                 "window_centre_%d" % (2 * gc.WINDOW + 9), "window_n_%d" % (c + gc.WINDOW + 2),
                 "window_n_%d" % (c + gc.WINDOW + 1)):
        v = gc.case(name)
        (cv,), n = gc.centres_of(v), v.x.shape[0]
        for knob, reach, inside in (("reach_lo", gc.WINDOW - 1, cv - gc.WINDOW >= 0),
                                    ("reach_lo", gc.WINDOW + 1, cv - gc.WINDOW - 1 >= 0),
                                    ("reach_hi", gc.WINDOW - 1, cv + gc.WINDOW + 1 < n),
                                    ("reach_hi", gc.WINDOW + 1, cv + gc.WINDOW + 2 < n)):
            assert (not _same(gc.brute_csr(v, **{knob: reach}), v.want)) == inside, (name, knob, reach)
    # at a ring's bounds: a well at exactly md[r] belongs to ring r - 1 alone, one at distance 1 to none
    b = gc.case("boundaries")
    (cb,) = gc.centres_of(b)
    n_on = lambda radii: sum(len(gc.circle_points(m)) for m in radii)
    sizes = lambda **k: [len(r) for r in gc.brute_rings(b.x, b.y, cb, 32, b.max_dists, **k)]
    base, inner, outer = sizes(), sizes(inner_le=True), sizes(outer_lt=True)
    md = b.max_dists
    assert [i - s for i, s in zip(inner, base)] == [len(gc.circle_points(md[r])) + (r == 0) for r in range(32)]
    assert [s - o for o, s in zip(outer, base)] == [len(gc.circle_points(md[r + 1])) for r in range(32)]
    # (m, 1) lies past md[r]: in ring r, and beyond the last ring for the last radius
    assert sum(base) == n_on(md[1:]) + 32 + 1                      # .. the circles, (m, 1) for all but the last, and (1, 1)
