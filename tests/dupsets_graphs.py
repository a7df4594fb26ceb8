"""Graphs injected into the duplicate sets (wd_dup_sets) as targets, reads and filters.  Test plumbing, no GPU.

wd_dup_sets takes any CSR with T == N and centre[t] == t, so a graph becomes a tile:
  * a naming (a, b, l) puts well b into ring l of well a;
  * reads are COLOURS: colour c is the letter "ACGT"[c] at every cycle, and a well may differ from its colour's
    read at cycle 0 only (mut != 0).  Two wells of one colour are 0 or 1 substitutions apart, wells of two
    colours at least L - 1 >= 4: a named pair of one colour is a duplicate under Hamming <= 2 and
    Levenshtein <= 2 / <= 3 (and under equality when the cycle-0 letters agree), a pair of two colours under none;
  * no ring may be empty (the scan refuses it), so a ring without a naming names a FILLER: every 8th well
    (w % 8 == 7) fails the filter in every tile and is named by the wells of its block of 8.  Half the fillers
    carry the read of the wells that name them (the scan logs the pair, the sets must drop it), half another.
Two declarations of a graph: one-ended (a names b only; the order inside a ring is whatever the builder gave) and
symmetric (b names a back in the same ring, fillers name back, every ring strictly ascending: what the dense
chain's one-ended compare asks for)."""
from __future__ import annotations

import numpy as np

from dupsets_ref import SIZE_BINS

BLOCK = 8                       # wells per filler block; the filler is the block's last well
L = 12                          # cycles of the injected reads
METRICS = ((0, 0), (1, 2), (2, 2), (2, 3))          # equality, Hamming <= 2, Levenshtein <= 2, <= 3


def is_filler(n):
    return np.arange(n) % BLOCK == BLOCK - 1


def real_wells(n):
    """The wells a graph may use as vertices, ascending."""
    return np.flatnonzero(~is_filler(n))


def filler_of(w, n):
    """The filler a well names in a ring that carries no naming (n >= BLOCK)."""
    last = (n // BLOCK) * BLOCK - 1
    return np.minimum(np.asarray(w, dtype=np.int64) | (BLOCK - 1), last)


# ---- targets ----------------------------------------------------------------------------------
def to_csr(n, levels, a, b, lev, symmetric):
    """Namings (a[i] names b[i] in ring lev[i]) -> (centre, lvl_off, nbr) with every well a target and no ring
    empty.  symmetric: the namings are closed under (a, b) -> (b, a) and every ring is sorted and unique."""
    assert n >= 2 * BLOCK
    a = np.asarray(a, dtype=np.int64)
    b = np.asarray(b, dtype=np.int64)
    lev = np.asarray(lev, dtype=np.int64)
    fill = np.flatnonzero(is_filler(n))
    # the fillers name each other round a cycle, at every level
    fa = np.repeat(fill, levels)
    fb = np.repeat(np.roll(fill, -1), levels)
    fl = np.tile(np.arange(levels), fill.shape[0])
    # a real well's ring without a naming names the block's filler
    has = np.zeros((n, levels), dtype=bool)
    has[a, lev] = True
    if symmetric:
        has[b, lev] = True
    has[fill] = True
    ew, el = np.nonzero(~has)
    a = np.concatenate([a, fa, ew])
    b = np.concatenate([b, fb, filler_of(ew, n)])
    lev = np.concatenate([lev, fl, el])
    if symmetric:
        a, b = np.concatenate([a, b]), np.concatenate([b, a])
        lev = np.concatenate([lev, lev])
        key = np.unique((a * levels + lev) * n + b)
        a, lev, b = key // n // levels, key // n % levels, key % n
    else:
        order = np.argsort(a * levels + lev, kind="stable")
        a, b, lev = a[order], b[order], lev[order]
    counts = np.bincount(a * levels + lev, minlength=n * levels).reshape(n, levels)
    assert counts.min() >= 1
    ends = np.cumsum(counts.reshape(-1)).reshape(n, levels)
    lvl_off = np.zeros((n, levels + 1), dtype=np.int32)
    lvl_off[:, 1:] = ends
    lvl_off[1:, 0] = ends[:-1, -1]
    return np.arange(n, dtype=np.int32), lvl_off, b.astype(np.int32)


def is_symmetric(csr):
    """What k_dense_symcheck asks of the targets, on the host."""
    centre, lvl_off, nbr = csr
    n, levels = lvl_off.shape[0], lvl_off.shape[1] - 1
    if (lvl_off[1:, 0] != lvl_off[:-1, -1]).any():       # rows that share slots: not what a generator writes
        return False
    t, lev = slots_of(csr)
    if (nbr == t).any():
        return False
    key = (t * levels + lev) * n + nbr
    if (np.diff(key) <= 0).any():                       # rows in order, every ring strictly ascending
        return False
    back = (nbr.astype(np.int64) * levels + lev) * n + t
    return bool(np.isin(back, key).all())


def slots_of(csr):
    """(target, ring) of every slot of nbr, for a CSR whose rows lie one after the other."""
    centre, lvl_off, nbr = csr
    n, levels = lvl_off.shape[0], lvl_off.shape[1] - 1
    counts = np.diff(lvl_off.astype(np.int64), axis=1).reshape(-1)
    assert lvl_off[0, 0] == 0 and (lvl_off[1:, 0] == lvl_off[:-1, -1]).all() and lvl_off[-1, -1] == nbr.shape[0]
    rows = np.repeat(np.arange(n * levels), counts)
    return rows // levels, rows % levels


# ---- reads and filters ------------------------------------------------------------------------
class Tile:
    """colour[n] in 0..3, mut[n] in 0..3 (added to the colour at cycle 0), pf[n] bool."""

    def __init__(self, colour, mut, pf):
        n = colour.shape[0]
        self.colour = np.asarray(colour, dtype=np.uint8)
        self.mut = np.asarray(mut, dtype=np.uint8)
        self.pf = np.asarray(pf, dtype=bool) & ~is_filler(n)

    def planes(self):
        """L planes of n bytes: a called base is (quality << 2) | code, never 0 (0 is a no-call)."""
        n = self.colour.shape[0]
        qual = (1 + np.arange(n) % 59).astype(np.uint8) << 2
        first = qual | ((self.colour + self.mut) & 3)
        rest = qual | self.colour
        return [first if c == 0 else rest for c in range(L)]

    def filter(self):
        return self.pf.astype(np.uint8)


def fillers_coloured(colour):
    """Fillers in both flavours: an even block's filler carries the read of the well before it, an odd block's
    the next colour."""
    n = colour.shape[0]
    out = colour.copy()
    f = np.flatnonzero(is_filler(n))
    out[f] = (colour[f - 1] + (f // BLOCK) % 2) & 3
    return out


def tile_full(n):
    """One colour, nothing mutated, every well but the fillers passes: the graph as declared, under every metric."""
    return Tile(fillers_coloured(np.zeros(n, dtype=np.uint8)), np.zeros(n, dtype=np.uint8), np.ones(n, dtype=bool))


def tile_random(n, seed, knock=0.3, mutate=0.1, stretch=997):
    """About 30 % of the wells knocked out, colours in stretches of 997 wells, one well in ten mutated."""
    rng = np.random.default_rng(seed)
    colour = ((np.arange(n) // stretch) * 3 % 4).astype(np.uint8)
    mut = np.where(rng.random(n) < mutate, rng.integers(1, 4, n), 0).astype(np.uint8)
    return Tile(fillers_coloured(colour), mut, rng.random(n) >= knock)


def tile_dead(n):
    return Tile(np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=bool))


def edges_from_colours(tile, csr, mode):
    """edges_from_reads for colour-coded reads, vectorised: every slot (t, s) of ring l with both wells PF, of
    one colour and (equality only) with the same letter at cycle 0.  lvl_off rows may share slots."""
    centre, lvl_off, nbr = csr
    levels = lvl_off.shape[1] - 1
    ea, eb, el = [], [], []
    w = nbr.astype(np.int64)
    for l in range(levels):
        lo, hi = lvl_off[:, l].astype(np.int64), lvl_off[:, l + 1].astype(np.int64)
        t = np.repeat(np.arange(lvl_off.shape[0]), hi - lo)
        s = np.arange((hi - lo).sum()) - np.repeat(np.cumsum(hi - lo) - (hi - lo), hi - lo) + np.repeat(lo, hi - lo)
        v = w[s]
        ok = tile.pf[t] & tile.pf[v] & (tile.colour[t] == tile.colour[v])
        if mode == 0:
            ok &= tile.mut[t] == tile.mut[v]
        ea.append(t[ok])
        eb.append(v[ok])
        el.append(np.full(int(ok.sum()), l, dtype=np.int64))
    ea, eb, el = np.concatenate(ea), np.concatenate(eb), np.concatenate(el)
    order = np.lexsort((el, ea))                       # target by target, ring by ring, slots in order (stable)
    return ea[order], eb[order], el[order]


# ---- families: namings over the real wells ------------------------------------------------------
def path(n, levels, backwards=False):
    """The real wells in a row, the level cycling along it; backwards: every well names its predecessor."""
    r = real_wells(n)
    lev = np.arange(r.shape[0] - 1) % levels
    return (r[1:], r[:-1], lev) if backwards else (r[:-1], r[1:], lev)


def star(n, levels, hub_last, every=1):
    """Every real well (every `every`-th) names the hub once (the hub is the last real well, or the first)."""
    r = real_wells(n)
    hub, rest = (r[-1], r[:-1]) if hub_last else (r[0], r[1:])
    rest = rest[::every]
    return rest, np.full(rest.shape[0], hub), np.arange(rest.shape[0]) % levels      # (every ring of the hub is used)


def ladder(n, levels, seed=7):
    """Level l joins neighbouring blocks of 2^l real wells by one edge between a random well of each."""
    r = real_wells(n)
    m = r.shape[0] - r.shape[0] % 2                      # an even number of vertices: everyone is paired at level 0
    rng = np.random.default_rng(seed)
    a, b, lev = [], [], []
    for l in range(levels):
        s = 1 << l
        left = np.arange(0, m - s, 2 * s)                # first well of a block that has a right neighbour
        if left.shape[0] == 0:
            break
        right_len = np.minimum(s, m - (left + s))
        a.append(r[left + rng.integers(0, s, left.shape[0])])
        b.append(r[left + s + rng.integers(0, 1 << 30, left.shape[0]) % right_len])
        lev.append(np.full(left.shape[0], l))
    return np.concatenate(a), np.concatenate(b), np.concatenate(lev)


def late_merge(n, levels, seed=11):
    """Two components at level 0 - a random recursive tree on the lower half of the real wells, a path on the upper
    half - joined by one edge at the outermost level.  -> (namings, first well of the upper component)."""
    r = real_wells(n)
    h = r.shape[0] // 2
    rng = np.random.default_rng(seed)
    kid = np.arange(1, h)
    mum = (rng.random(h - 1) * kid).astype(np.int64)     # a random earlier well
    a = np.concatenate([r[mum], r[h:-1], [r[h // 2]]])
    b = np.concatenate([r[kid], r[h + 1:], [r[-1]]])
    lev = np.concatenate([np.zeros(h - 1 + r.shape[0] - h - 1, dtype=np.int64), [levels - 1]])
    return (a, b, lev), int(r[h])


def size_bins(n, levels):
    """Runs of 1, 2, .. 11 consecutive real wells, repeated: a path in even repetitions, a clique in odd ones.
    -> (namings, repetitions)."""
    r = real_wells(n)
    sizes = np.arange(1, SIZE_BINS + 4)
    reps = r.shape[0] // int(sizes.sum())
    a, b, lev = [], [], []
    pos = 0
    for rep in range(reps):
        for s in sizes.tolist():
            w = r[pos:pos + s]
            pos += s
            if rep % 2 == 0:
                i, j = np.arange(s - 1), np.arange(1, s)
            else:
                i, j = np.triu_indices(s, 1)
            a.append(w[i])
            b.append(w[j])
            lev.append((i + j + rep) % levels)
    return (np.concatenate(a), np.concatenate(b), np.concatenate(lev)), reps


def size_bins_expected(reps):
    """Sets of exactly 2 .. 8 wells, then those of 9, 10 and 11 together."""
    return [reps] * (SIZE_BINS - 1) + [3 * reps]


def gnm(n, levels, degree, seed):
    """G(n, m) on the real wells with m = degree * n / 2 random pairs (repeats allowed), random levels; the lower
    well names the higher one."""
    r = real_wells(n)
    rng = np.random.default_rng(seed)
    m = int(degree * r.shape[0] / 2)
    u = rng.integers(0, r.shape[0], m)
    v = rng.integers(0, r.shape[0], m)
    keep = u != v
    u, v = np.minimum(u, v)[keep], np.maximum(u, v)[keep]
    shuffle = rng.permutation(u.shape[0])                # rings in any order
    return r[u][shuffle], r[v][shuffle], rng.integers(0, levels, u.shape[0])[shuffle]


# the multigraph corners: a few dozen wells of a larger tile, every other real well in no set
CORNER_SELF = 30                # names itself in ring 1, and nothing else of its colour
CORNER_SELF_IN_SET = 33         # names itself in ring 0 and joins 34 at level 2 only
CORNER_BRIDGE = 41              # fails the filter: 40 - 41 - 42 must stay apart
CORNER_SHARED = (50, 51)        # two targets with one lvl_off row, both naming 52 in ring 0


def corners(n, levels):
    """-> (csr, tile): one-ended by nature (a names b at level 2 while b names a at level 0)."""
    assert levels >= 3
    nam = [(10, 11, 0), (10, 11, 2),                     # the same pair in rings 0 and 2 of one well
           (20, 21, 2), (21, 20, 0),                     # level 2 from one end, level 0 from the other
           (CORNER_SELF, CORNER_SELF, 1),
           (CORNER_SELF_IN_SET, CORNER_SELF_IN_SET, 0), (CORNER_SELF_IN_SET, 34, 2),
           (40, CORNER_BRIDGE, 0), (CORNER_BRIDGE, 42, 0),
           (CORNER_SHARED[0], 52, 0)]
    a, b, lev = (np.array(x) for x in zip(*nam))
    centre, lvl_off, nbr = to_csr(n, levels, a, b, lev, symmetric=False)
    lvl_off[CORNER_SHARED[1]] = lvl_off[CORNER_SHARED[0]]
    tile = tile_full(n)
    tile.pf[CORNER_BRIDGE] = False
    return (centre, lvl_off, nbr), tile


# ---- what every sets row must satisfy -----------------------------------------------------------
def split_row(row, levels):
    """-> (PF, Sets[levels], InSets[levels], Redundant[levels], bins[8])"""
    row = np.asarray(row)
    assert row.shape[0] == 1 + 3 * levels + SIZE_BINS
    return (int(row[0]), row[1:1 + levels], row[1 + levels:1 + 2 * levels], row[1 + 2 * levels:1 + 3 * levels],
            row[1 + 3 * levels:])


def check_row(row, levels):
    pf, sets, in_sets, red, bins = split_row(row, levels)
    assert bins.sum() == sets[-1], (bins, sets)
    assert (red == in_sets - sets).all(), row
    assert (np.diff(in_sets) >= 0).all() and (np.diff(red) >= 0).all(), row
    assert (sets >= 0).all() and (2 * sets <= in_sets).all() and in_sets[-1] <= pf, row
    # Sets[l] itself is not monotone (sets merge); what it may not do is grow by more than the wells that join
    assert (np.diff(sets) <= np.diff(in_sets) // 2).all(), row


# ---- the cases of the tests: (family, declaration) -> targets and a batch of tiles ------------------
class Case:
    def __init__(self, name, levels, csr, tiles, symmetric, **extra):
        self.name, self.levels, self.csr, self.tiles, self.symmetric, self.extra = name, levels, csr, tiles, symmetric, extra
        self.n = csr[0].shape[0]
        self._ref = {}

    def reference(self, mode):
        """(sets rows, labels) of the host union-find for every tile; Hamming and Levenshtein share their edges."""
        from dupsets_ref import dup_sets
        key = 0 if mode == 0 else 1
        if key not in self._ref:
            out = [dup_sets(self.n, t.pf, *edges_from_colours(t, self.csr, key), self.levels) for t in self.tiles]
            self._ref[key] = (np.array([o[0] for o in out]), np.array([o[1] for o in out]))
        return self._ref[key]


def standard_tiles(n, seed):
    """All PF but the fillers; about 30 % knocked out, colours in stretches; dead."""
    return [tile_full(n), tile_random(n, seed), tile_dead(n)]


CASES = ("path-one", "path-back", "path-sym", "star-last", "star-first", "star-sym-last", "star-sym-first", "ladder-one", "ladder-sym", "merge-one",
         "merge-sym", "bins-one", "bins-sym", "corners", "gnm1-one-s1", "gnm1-sym-s2", "gnm2-one-s3", "gnm2-sym-s4",
         "gnm2-one-s5")


def make_case(name, n, levels=8):
    fam, _, rest = name.partition("-")
    decl = rest.split("-")[0]
    sym = decl == "sym"
    extra = {}
    tiles = standard_tiles(n, len(name) + sum(map(ord, name)))
    if fam == "path":
        nam = path(n, levels, backwards=decl == "back")
        knocked = tile_full(n)
        knocked.pf[real_wells(n)[real_wells(n).shape[0] // 3]] = False     # one well out: two sets
        tiles = tiles[:2] + [knocked, tiles[2]]
    elif fam == "star":
        # (declared from both ends and with the hub first, one lane of the dense chain's one-ended compare walks the
        # hub's whole row: 8.3 s for this test's 48 calls at 61 249 slots on an MI355X, so a quarter of them there)
        nam = star(n, levels, hub_last=name.endswith("last"), every=4 if name == "star-sym-first" else 1)
        hub = int(nam[1][0])
        extra["members"] = np.sort(np.append(nam[0], hub))
        keep_hub = tile_random(n, 5, stretch=n)             # one colour, 30 % knocked out, the hub kept
        keep_hub.pf[hub] = True
        no_hub = tile_full(n)
        no_hub.pf[hub] = False                              # no set at all
        tiles = [tiles[0], keep_hub, no_hub, tiles[2]]
        extra["hub"] = hub
    elif fam == "ladder":
        nam = ladder(n, levels)
    elif fam == "merge":
        nam, extra["upper"] = late_merge(n, levels)
    elif fam == "bins":
        nam, extra["reps"] = size_bins(n, levels)
    elif fam == "corners":
        csr, tile = corners(n, levels)
        return Case(name, levels, csr, [tile, tiles[1], tiles[2]], False)
    elif fam.startswith("gnm"):
        nam = gnm(n, levels, int(fam[3:]), int(rest.split("-s")[1]))
    else:
        raise ValueError(name)
    return Case(name, levels, to_csr(n, levels, *nam, symmetric=sym), tiles, sym, **extra)


def check_nondegenerate(case):
    """Each family does what it is there for - asked of the reference, before any device is."""
    n, levels = case.n, case.levels
    fam = case.name.partition("-")[0]
    assert is_symmetric(case.csr) == case.symmetric
    real = int((~is_filler(n)).sum())
    for mode in (0, 1):
        rows, labels = case.reference(mode)
        for row in rows:
            check_row(row, levels)
        pf, sets, in_sets, red, bins = split_row(rows[0], levels)
        first = int(real_wells(n)[0])
        assert pf == real - (fam == "corners") and rows[-1][0] == 0 and rows[-1][1:].sum() == 0            # full tile, dead tile
        if fam == "path":
            assert sets[-1] == 1 and in_sets[-1] == real and bins.tolist() == [0] * 7 + [1]
            assert (labels[0][case.tiles[0].pf] == first).all()
            assert sets[0] == (real - 1 + levels - 1) // levels                       # level 0: every levels-th edge
            assert split_row(rows[2], levels)[1][-1] == 2                             # one well knocked out
            assert split_row(rows[1], levels)[1][-1] > 100
        elif fam == "star":
            mem = case.extra["members"]
            assert sets.tolist() == [1] * levels and in_sets[-1] == mem.shape[0] and red[-1] == mem.shape[0] - 1
            assert (np.diff(in_sets) > 0).all() and mem.shape[0] >= real // 4          # every ring of the hub hooks
            assert (labels[0][mem] == mem[0]).all() and (labels[0] == mem[0]).sum() == mem.shape[0]
            r1 = split_row(rows[1], levels)
            assert r1[1][-1] == 1 and 0.6 * mem.shape[0] < r1[2][-1] < 0.8 * mem.shape[0]
            assert rows[2][1:].sum() == 0 and rows[2][0] == real - 1                  # the hub fails the filter
        elif fam == "ladder":
            m = real - real % 2
            assert sets.tolist() == [-(-m // (2 << l)) for l in range(levels)]
            assert (in_sets == m).all() and (red == m - sets).all()
        elif fam == "merge":
            upper = case.extra["upper"]
            assert sets.tolist() == [2] * (levels - 1) + [1] and (in_sets == real).all()
            assert red.tolist() == [real - 2] * (levels - 1) + [real - 1]
            assert labels[0][upper] == first and (labels[0][case.tiles[0].pf] == first).all()
        elif fam == "bins":
            assert bins.tolist() == size_bins_expected(case.extra["reps"]) and case.extra["reps"] >= 2
            assert sets[-1] == 10 * case.extra["reps"]
        elif fam == "corners":
            lab = labels[0]
            assert lab[11] == 10 and lab[21] == 20 and lab[34] == CORNER_SELF_IN_SET
            assert lab[CORNER_SELF] == CORNER_SELF and lab[40] == 40 and lab[42] == 42
            assert lab[CORNER_BRIDGE] == 0xFFFFFFFF and lab[51] == 50 and lab[52] == 50
            # {10, 11} and {20, 21} and {50, 51, 52} from level 0, {33, 34} at level 2; the self-namers add nothing
            assert sets.tolist() == [3, 3] + [4] * (levels - 2) and in_sets.tolist() == [7, 7] + [9] * (levels - 2)
            assert bins.tolist() == [3, 1, 0, 0, 0, 0, 0, 0]
        elif fam == "gnm1":
            assert (bins > 0).all() and bins[-1] > 20                                 # about the threshold: every bin fills
        elif fam == "gnm2":
            sizes = np.bincount(labels[0][case.tiles[0].pf].astype(np.int64))
            assert sizes.max() > 0.5 * real and (bins[:3] > 0).all()                  # a giant component and debris
            assert (np.diff(sets) < 0).any() and (np.diff(sets[:2]) > 0).all()        # sets appear, then merge
        if fam != "corners":
            assert split_row(rows[1], levels)[1].max() > 0                            # the knocked-out tile has sets too
    r0 = case.reference(0)[0]
    assert (r0[1] != case.reference(1)[0][1]).any() or fam == "corners"               # mutations matter to equality alone
