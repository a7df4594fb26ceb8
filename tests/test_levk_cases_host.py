"""What the cases of tests/levk_cases.py hold, asserted from the CPU oracle's distances alone - so that a generator that
drifted (a script whose edits cancel, an inserted letter that repeats its neighbour) cannot hide a kernel's failure behind
a case set that no longer has a pair at the threshold.  No GPU, no kernel: the oracle, numpy, and a textbook DP restricted
to a band (levk_cases.restricted_distance), which with the whole band must be the oracle's distance.

Per (instantiation, threshold the kernel is given), over all of its cases with k < L:
  >= 8 pairs at distance exactly k, >= 8 at exactly k + 1;
  >= 8 pairs below k whose alignment needs an indel (the edit distance is smaller than the Hamming distance) - for k >= 3:
       an indel in equal-length reads comes with its opposite, so such a pair lies at 2 or more, never below k = 2;
  >= 8 pairs above k + 1 - where k + 2 <= L: no pair of reads of L cycles lies above L, so k = L - 1 has none;
  >= 4 band-edge pairs: distance <= k, but the DP restricted to |j - i| <= H - 1, H = k / 2, says > k - the pair needs the
       outermost diagonal of the band the launcher hands the kernel;
  >= 4 pairs with Hamming distance > k and edit distance <= k.
The cases with k >= L (the hit log wants true distances: every pair is a duplicate) are held to their distances by the
emulator and the GPU test; they have no threshold to stand at and are left out of the counts here."""
import collections
import re
import os

import numpy as np

import levk_cases as lc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOORS = dict(at_k=8, at_k1=8, below_indel=8, above=8, band_edge=4, hamming_far=4)


def _source(name):
    return open(os.path.join(REPO, "well_duplicates_amd", "csrc", name)).read()


def test_the_launchers_figures_are_the_librarys():
    """B1, the H-rounding and kLevB2 are read off the launchers, not only restated (levk_cases.py restates them)."""
    m = re.search(r"constexpr int lev_first\(int H\) \{ return H == 1 \? (\d+) : H == 2 \? (\d+) : H == 3 \? (\d+) : H == 4 \? (\d+) : H <= 6 \? (\d+) : (\d+); \}",
                  _source("wd_shared.h"))
    assert dict(zip(lc.SEQ_H, (int(v) for v in m.groups()))) == lc.LEV_FIRST
    scan = _source("welldup_scan.hip")
    assert int(re.search(r"constexpr int kLevB2 = (\d+);", scan).group(1)) == lc.LEV_B2
    chain = re.findall(r"if \(h <= (\d+)\) launch_lev<(\d+)>", scan) + re.findall(r"else launch_lev<(\d+)>\(ctx, a, grid, strided\);", scan)
    assert chain == [("1", "1"), ("2", "2"), ("3", "3"), ("4", "4"), ("6", "6"), "8"], chain
    assert [lc.seq_h(h) for h in range(1, 9)] == [1, 2, 3, 4, 6, 6, 8, 8]
    assert "const bool lev_generic = lev && kk / 2 > 8;" in scan
    queue = _source("welldup_queue.hip")
    assert "first_even = lev_first(H) - (H <= 2 ? 2 : 0), first_odd = lev_first(H) + 1 - (H == 1 ? 2 : 0);" in queue
    assert "WD_LAUNCH_Q(true, 8, 1, 4, lds);" in queue
    assert [lc.queue_first("plane", k) for k in range(2, 8)] == [5, 6, 8, 11, 13, 14] and lc.queue_first("il", 3) == 8
    assert lc.qc.K_PASS * lc.qc.K_MAX_PASSES == 508


def test_no_case_is_dropped_and_every_instantiation_is_named():
    cases = lc.cases()
    assert [c.name for c in cases] == lc.planned_names()
    kernels = {c.kernel for c in cases}
    queue = {"k_scan_q<%s, %d, %d, 1>" % (S, B1, H) for S in ("false", "true") for B1, H in ((5, 1), (6, 1), (8, 2), (11, 2), (13, 3), (14, 3))}
    queue.add("k_scan_q<true, 8, 1, 4>")
    seq = {"k_scan<LevState<%d>, %s, %d, 8>" % (H, S, lc.LEV_FIRST[H]) for H in lc.SEQ_H for S in ("false", "true")}
    generic = {"k_scan_lev_generic<false>", "k_scan_lev_generic<true>"}
    assert (len(queue), len(seq), len(generic)) == (13, 12, 2) and kernels == queue | seq | generic
    # both thresholds of every band, the rounded ones included; k_scan with and without the early exit
    for S in ("false", "true"):
        for k in range(2, 18):
            name = "k_scan<LevState<%d>, %s, %d, 8>" % (lc.seq_h(k // 2), S, lc.LEV_FIRST[lc.seq_h(k // 2)])
            assert {c.early for c in cases if c.group == (name, k)} == {0, 1}, (name, k)
    assert {c.kk for c in cases if c.kernel == "k_scan_q<true, 8, 1, 4>"} == {2, 3}
    assert {(c.L, c.kk) for c in cases if c.kind == "generic"} == {(40, 18), (40, 19), (40, 39), (64, 18), (64, 19), (64, 63), (20, 20)}
    assert any(c.kernel.startswith("k_scan<LevState<8>") and c.L == 16 and c.k == 16 and c.hit_cap > 0 for c in cases)
    assert any(c.kind == "seq" and c.queue_kernel == 1 and c.early == 1 and int(np.diff(c.lvl_off[:, [0, -1]]).max()) == 509 for c in cases)
    # the shapes: slot counts, levels, tiles, the hit log on for every instantiation
    for kernel in kernels:
        mine = [c for c in cases if c.kernel == kernel]
        slots = {int(v) for c in mine for v in np.diff(c.lvl_off[:, [0, -1]], axis=1).reshape(-1)}
        assert {1, 64, 127, 128} <= slots or kernel.startswith("k_scan_lev_generic"), (kernel, sorted(slots))
        assert any(c.hit_cap > 0 for c in mine) and all(c.per_target for c in mine), kernel
        assert {len(c.tiles) for c in mine} == {1, 2} and max(c.levels for c in mine) == 8 and min(c.levels for c in mine) == 1, kernel
        assert all(257 <= c.n <= 4099 for c in mine)
    assert lc.not_launchable() == []          # (every L of the list at or below its k is left out by _lengths: none is planned and then dropped)


def test_the_case_set_holds_its_conditions():
    counts = collections.defaultdict(lambda: collections.Counter())
    possible = collections.defaultdict(lambda: dict(below_indel=False, above=False))
    for c in lc.cases():
        cen, nb, dist = lc.pairs_of(c)
        assert (lc.restricted_distance(cen, nb, c.L) == dist).all(), c.name      # the helper with the whole band is the oracle
        if c.kk >= c.L:
            assert (dist <= c.kk).all() and len(set(dist.tolist())) >= 8, c.name     # every pair a duplicate, at many distances
            continue
        k, H = c.kk, c.kk // 2
        ham = (cen != nb).sum(axis=1)
        narrow = lc.restricted_distance(cen, nb, H - 1)
        assert (ham >= dist).all() and (narrow >= dist).all()
        n = counts[c.group]
        n["at_k"] += int((dist == k).sum())
        n["at_k1"] += int((dist == k + 1).sum())
        n["below_indel"] += int(((dist < k) & (ham > dist)).sum())
        n["above"] += int((dist > k + 1).sum())
        n["band_edge"] += int(((dist <= k) & (narrow > k)).sum())
        n["hamming_far"] += int(((ham > k) & (dist <= k)).sum())
        n["nocall_shared"] += int(((cen == 0) & (nb == 0)).any(axis=1).sum())
        n["nocall_one_side"] += int(((cen == 0) != (nb == 0)).any(axis=1).sum())
        possible[c.group]["below_indel"] |= k >= 3
        possible[c.group]["above"] |= k + 2 <= c.L
    assert len(counts) == 14 + 32 + 8
    for group, n in sorted(counts.items()):
        print("%-36s k %2d: at k %4d, at k + 1 %4d, below k with an indel %4d, above k + 1 %4d, band-edge %4d, Hamming-far %4d, "
              "no-call shared %4d / on one side %4d" % (group + tuple(n[key] for key in ("at_k", "at_k1", "below_indel", "above", "band_edge",
                                                                                          "hamming_far", "nocall_shared", "nocall_one_side"))))
    for group, n in counts.items():
        for key, floor in FLOORS.items():
            if possible[group].get(key, True):
                assert n[key] >= floor, (group, key, n[key])
            else:
                assert n[key] == 0, (group, key, n[key])                      # (what cannot be is not there either)
        assert n["nocall_shared"] >= 8 and n["nocall_one_side"] >= 8, (group, n)


def test_the_restricted_dp_is_the_textbooks():
    """The helper against the plain double loop on a few hundred random pairs, at bands 0, 1, 3 and the whole table."""
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 3, size=(200, 9)), rng.integers(0, 3, size=(200, 9))

    def plain(x, y, band):
        L, big = len(x), 1 << 20
        d = [[big] * (L + 1) for _ in range(L + 1)]
        for i in range(L + 1):
            for j in range(L + 1):
                if abs(j - i) > band:
                    continue
                if i == 0 or j == 0:
                    d[i][j] = i + j
                else:
                    d[i][j] = min(d[i - 1][j - 1] + (x[i - 1] != y[j - 1]), d[i - 1][j] + 1, d[i][j - 1] + 1, big)
        return d[L][L]

    for band in (0, 1, 3, 9):
        got = lc.restricted_distance(a, b, band)
        assert got.tolist() == [plain(x, y, band) for x, y in zip(a.tolist(), b.tolist())], band
    assert (lc.restricted_distance(a, b, 0) == (a != b).sum(axis=1)).all()
