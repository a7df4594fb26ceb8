"""The ring generator's edge cases and a plain reference, shared by tests/test_genrings_host.py (the numpy generator),
tests/test_genrings_emu.py (csrc/gen_rings.inc on the CPU under shuffled schedules) and tests/test_gpu_generator.py
(wd_targets_from_coords on the device): one definition of the cases and of the truth.

brute_rings is get_indexes (prepare_cluster_indexes.py:38-78) written from its definition: scan the records from
max(0, c - 20000) on, bin each by its pixel distance to the centre - math.sqrt of Python ints, in double precision -
into ring r when md[r] < dist <= md[r + 1], and stop after the first record whose index exceeds c + 20000 (which is
therefore examined: c + 20001 is the last one).  Its knobs exist for the host test alone, which shows that the cases
tell a generator with the default knobs from one with any of them turned."""
import functools
import math
import os
import tempfile
from collections import namedtuple

import numpy as np

from well_duplicates_amd import cluster_indexes, synth

WINDOW = 20000                   # MAX_SEARCH_AREA
CAPACITY = 2048                  # kGenMaxMatches (csrc/gen_rings.inc): the device refuses a centre with more matches
FAR = 5000                       # the pixel of a well that is nobody's neighbour

# want: (centre, lvl_off [T, levels + 1], nbr) int32 from brute_rings, None where it raises.  error: None, "empty"
# (RuntimeError: a ring without wells, everywhere) or "capacity" (RuntimeError on the device alone: `want` stands for
# the host generator, which has no such limit).
Case = namedtuple("Case", "name x y centres levels max_dists want error")


def brute_rings(x, y, c, levels, max_dists, reach_lo=WINDOW, reach_hi=WINDOW, inner_le=False, outer_lt=False,
                f32=False):
    """The rings of centre c as `levels` ascending lists of record indices; RuntimeError if one is empty."""
    xs, ys = [int(v) for v in x], [int(v) for v in y]
    md = [int(m) for m in max_dists]
    n, cx, cy = len(xs), xs[c], ys[c]
    rings = [[] for _ in range(levels)]
    j = max(0, c - reach_lo)
    while j < n:
        dx, dy = xs[j] - cx, ys[j] - cy
        d2 = dx * dx + dy * dy
        dist = np.sqrt(np.float32(d2)) if f32 else math.sqrt(d2)
        for r in range(levels):
            inner = md[r] <= dist if inner_le else md[r] < dist
            outer = dist < md[r + 1] if outer_lt else dist <= md[r + 1]
            if inner and outer:
                rings[r].append(j)
        if j > c + reach_hi:
            break
        j += 1
    for r in range(levels):
        if not rings[r]:
            raise RuntimeError("Got no wells for cluster %d at (%d,%d) level %d" % (c, cx, cy, r))
    return rings


def centres_of(case):
    return list(range(len(case.x))) if case.centres is None else [int(c) for c in case.centres]


def csr_of(centres, rings_per_centre, levels):
    """[(rings of a centre)] -> (centre, lvl_off, nbr) int32, the layout of wd_get_targets."""
    off = np.zeros((len(centres), levels + 1), dtype=np.int32)
    nbr, p = [], 0
    for t, rings in enumerate(rings_per_centre):
        for r in range(levels):
            off[t, r] = p
            nbr.extend(rings[r])
            p += len(rings[r])
        off[t, levels] = p
    return np.array(centres, dtype=np.int32), off, np.array(nbr, dtype=np.int32)


def brute_csr(case, **knobs):
    cs = centres_of(case)
    return csr_of(cs, [brute_rings(case.x, case.y, c, case.levels, case.max_dists, **knobs) for c in cs], case.levels)


def _case(name, x, y, centres, levels, max_dists=None, error=None):
    md = list(max_dists) if max_dists is not None else cluster_indexes.max_dists_for(levels)
    x, y = np.asarray(x, dtype=np.int64), np.asarray(y, dtype=np.int64)
    centres = None if centres is None else np.asarray(centres, dtype=np.int32)
    case = Case(name, x, y, centres, levels, md, None, error)
    if error == "empty":
        try:
            brute_csr(case)
        except RuntimeError:
            return case
        raise AssertionError("%s: expected an empty ring" % name)
    return case._replace(want=brute_csr(case))


# ---- the window: every well far away but the centre at (1000, 1000) and the probes, `dx` pixels to its right
def _window(n, c, probes):
    x, y = np.full(n, FAR, np.int64), np.full(n, FAR, np.int64)
    x[c] = y[c] = 1000
    for off, dx in probes:
        if 0 <= c + off < n:
            assert off != 0
            x[c + off], y[c + off] = 1000 + dx, 1000
    return x, y


EDGE_OFFSETS = (-WINDOW - 1, -WINDOW, -1, 1, WINDOW, WINDOW + 1, WINDOW + 2)


def _window_cases():
    n, c = 2 * WINDOW + 10, WINDOW + 2
    x, y = _window(n, c, [(o, 10) for o in (-WINDOW - 1, -WINDOW, 1, WINDOW + 1, WINDOW + 2)])
    case = _case("window", x, y, [c], 1)
    assert case.want[2].tolist() == [2, WINDOW + 3, 2 * WINDOW + 3]
    yield case
    # the clamps: a centre at record 0, where the low bound first leaves 0 and just past it, at the last record
    for c2 in (0, WINDOW, WINDOW + 1, n - 1):
        x, y = _window(n, c2, [(o, 10) for o in EDGE_OFFSETS])
        yield _case("window_centre_%d" % c2, x, y, [c2], 1)
    # the table ends at the last record examined, and one before it
    for n2 in (c + WINDOW + 2, c + WINDOW + 1):
        x, y = _window(n2, c, [(o, 10) for o in EDGE_OFFSETS])
        case = _case("window_n_%d" % n2, x, y, [c], 1)
        assert case.want[2][-1] == n2 - 1
        yield case
    # a ring whose only well is the last record examined, and the first one that is not
    x, y = _window(n, c, [(1, 10), (WINDOW + 1, 30)])
    yield _case("window_last_ring_kept", x, y, [c], 2)
    x, y = _window(n, c, [(1, 10), (WINDOW + 2, 30)])
    yield _case("window_last_ring_empty", x, y, [c], 2, error="empty")


# ---- ring boundaries
def circle_points(m):
    """Every integer point at distance exactly m from the origin."""
    pts = [(m, 0), (-m, 0), (0, m), (0, -m)]
    for a in range(1, m):
        b = math.isqrt(m * m - a * a)
        if b > 0 and a * a + b * b == m * m:
            pts += [(a, b), (-a, b), (a, -b), (-a, -b)]
    return pts


def _boundary_points(radii):
    pts = [(1, 0), (1, 1), (0, 0)]
    for m in radii:
        pts += circle_points(m) + [(m, 1)]
    return pts


def _scatter(pts, seed, cx=2000, cy=2000):
    """The points around a centre at (cx, cy), in a seeded order, the centre among them: (x, y, centre's record)."""
    order = np.random.default_rng(seed).permutation(len(pts) + 1)
    x, y = np.zeros(len(pts) + 1, np.int64), np.zeros(len(pts) + 1, np.int64)
    for rec, k in enumerate(order):
        dx, dy = pts[k - 1] if k else (0, 0)
        x[rec], y[rec] = cx + dx, cy + dy
    return x, y, int(np.flatnonzero(order == 0)[0])


def _boundary_cases():
    md = cluster_indexes.max_dists_for(32)
    assert sum(len(circle_points(m)) > 4 for m in md) >= 12         # radii with integer points off the axes
    x, y, c = _scatter(_boundary_points(md), 3)
    yield _case("boundaries", x, y, [c], 32)
    # the ABI's largest radius: 30000^2 = 9e8 fits an int; 9e8 + 1 is beyond float32's 24 bits
    pts = [(18000, 24000), (18000, 24001), (30000, 0), (30000, 1), (0, 1), (0, 0)]
    x, y, c = _scatter(pts, 4, 100, 100)
    case = _case("largest_radius", x, y, [c], 2, [0, 1, 30000])
    assert case.want[1].tolist() == [[0, 1, 3]]
    yield case


# ---- capacity: rings [1, 22, 42], wells alternating between the rings by index, the centre in the middle
def _capacity(inside, far_every=0):
    x, y, k = [], [], 0
    while k < inside:
        if far_every and len(x) % far_every == 0:
            x.append(FAR), y.append(FAR)
            continue
        if len(x) == inside // 2:
            x.append(1000), y.append(1000)                          # the centre
            continue
        ring = len(x) % 2
        x.append(1000 + (30 if ring else 10) + k % 7), y.append(1000 - k % 5)
        k += 1
    return x, y, inside // 2


def _capacity_cases():
    for name, inside, far_every, error in (("capacity_2048", CAPACITY, 0, None),
                                           ("capacity_2049", CAPACITY + 1, 0, "capacity"),
                                           ("capacity_2048_and_far", CAPACITY, 5, None)):
        x, y, c = _capacity(inside, far_every)
        case = _case(name, x, y, [c], 2, [1, 22, 42], error=error)
        assert x[c] == 1000 and y[c] == 1000
        _, off, nbr = case.want
        assert off[0, 2] == inside and min(off[0, 1], inside - off[0, 1]) > 800
        assert (nbr[:off[0, 1]] % 2 == 0).all() and (nbr[off[0, 1]:] % 2 == 1).all()
        yield case


# ---- order: three rings of about 500 wells each, a well's ring its index % 3
def _order_table(n_in=1500, c=750):
    x = [1000 + (10, 30, 50)[j % 3] + j % 9 for j in range(n_in + 1)]
    y = [1000 + j % 11 for j in range(n_in + 1)]
    x[c] = y[c] = 1000
    return x, y, c


def _order_cases():
    x, y, c = _order_table()
    case = _case("order", x, y, [c], 3)
    _, off, nbr = case.want
    for r in range(3):
        ring = nbr[off[0, r]:off[0, r + 1]]
        assert ring.shape[0] >= 499 and (ring % 3 == r).all() and (np.diff(ring) > 0).all()
    yield case


# ---- several centres in one call, not in ascending order: lvl_off is a prefix sum over centres
def _several_cases():
    n, cw = 2 * WINDOW + 10, WINDOW + 2
    x, y = _window(n, cw, [(-WINDOW - 1, 10), (-WINDOW, 10), (1, 10), (2, 30), (3, 50), (WINDOW + 1, 10),
                           (WINDOW + 2, 10)])
    bx, by, bc = _scatter(_boundary_points(cluster_indexes.max_dists_for(3)), 5, 9000, 1000)
    x[5000:5000 + len(bx)], y[5000:5000 + len(bx)] = bx, by
    ox, oy, oc = _order_table()
    x[30000:30000 + len(ox)], y[30000:30000 + len(ox)] = ox, np.asarray(oy) + 8000
    centres = [30000 + oc, 5000 + bc, cw]
    case = _case("several_centres", x, y, centres, 3)
    assert (np.diff(case.want[1].ravel()) >= 0).all() and case.want[1][1, 0] > 1000
    yield case


def _small_cases():
    yield _case("two_wells", [1000, 1010], [1000, 1000], None, 1)
    yield _case("one_well", [1000], [1000], None, 1, error="empty")


# ---- a jittered honeycomb, every well a centre, through an s.locs file
JITTER_SEED = 1


def _jitter_cases():
    x, y = synth.honeycomb_pixels(24, 40)
    rng = np.random.default_rng(JITTER_SEED)
    x, y = x + rng.integers(-2, 3, x.shape[0]), y + rng.integers(-2, 3, y.shape[0])
    fd, path = tempfile.mkstemp(suffix=".locs")
    try:
        with os.fdopen(fd, "wb") as fh:
            fh.write(synth.slocs_bytes(x, y))
        x2, y2 = cluster_indexes.read_slocs(path)
    finally:
        os.unlink(path)
    assert (x2 == x).all() and (y2 == y).all()
    yield _case("jittered_honeycomb", x2, y2, None, 3)      # (an empty ring under this seed raises here)


# the cases by name, for a test to parametrise over without building them while tests are collected
NAMES = ("window", "window_centre_0", "window_centre_20000", "window_centre_20001", "window_centre_40009",
         "window_n_40004", "window_n_40003", "window_last_ring_kept", "window_last_ring_empty", "boundaries",
         "largest_radius", "capacity_2048", "capacity_2049", "capacity_2048_and_far", "order", "several_centres",
         "two_wells", "one_well", "jittered_honeycomb")


@functools.lru_cache(maxsize=None)
def cases():
    """Every case, built once and shared: the arrays are read-only."""
    out = []
    for family in (_window_cases, _boundary_cases, _capacity_cases, _order_cases, _several_cases, _small_cases,
                   _jitter_cases):
        out.extend(family())
    assert tuple(c.name for c in out) == NAMES
    for c in out:                                                   # nobody may change what the tests share
        for a in (c.x, c.y, c.centres) + (c.want or ()):
            if a is not None:
                a.setflags(write=False)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)
