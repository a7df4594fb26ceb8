"""The scripted-survival builder (tests/survival_ref.py) on the host: every input the GPU parity tests of
tests/test_gpu_survival.py use is built here, run through the model of the kernels' work distribution and through
the CPU oracle.  These are conditions on the INPUTS: each one must drive the queues' decisions it was written for.
If a constant of the kernels changes, the mirrored constant in survival_ref.py has to follow, and this module then
names the regime that went empty."""
import numpy as np
import pytest

import survival_ref as sr
from oracle import oracle


def oracle_tile(c, i, mode, k, _cache={}):
    key = (c.name, i, mode, k)
    if key not in _cache:
        s = c.tiles[i]
        _cache[key] = oracle.count_tile(s.planes, s.filt, *c.geom.csr(), mode, k, want_dist=True)
    return _cache[key]


def test_mirrored_constants_match_the_sources():
    """The constants survival_ref.py mirrors, read back from the kernels' sources."""
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "well_duplicates_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in
            ("wd_shared.h", "scan_queue.inc", "scan_lines.inc", "device_common.inc", "welldup_queue.hip", "welldup_scan.hip")}

    def const(f, name):
        m = re.search(r"constexpr int %s = ([^;]+);" % name, text[f])
        assert m, (f, name)
        return m.group(1).strip()

    assert const("wd_shared.h", "kPass") == str(sr.K_PASS)
    assert const("wd_shared.h", "kMaxPasses") == str(sr.K_MAX_PASSES)
    assert const("wd_shared.h", "kWaves") == "kBlock / kWave" and const("wd_shared.h", "kBlock") == "256" \
        and const("wd_shared.h", "kWave") == "64" and sr.K_WAVES == 4
    assert const("scan_queue.inc", "kFinishAllMax") == str(sr.K_FINISH_ALL_MAX)
    assert const("scan_queue.inc", "kFinishInPlace") == str(sr.K_FINISH_IN_PLACE)
    assert const("scan_queue.inc", "kQCap") == "WD_QCAP" and "#define WD_QCAP %d\n" % sr.K_QCAP in text["scan_queue.inc"]
    assert const("scan_lines.inc", "kLwTargets") == str(sr.K_LW_TARGETS)
    assert const("scan_lines.inc", "kLwPairs") == str(sr.K_LW_PAIRS)
    assert const("scan_lines.inc", "kLwStep") == "2 * kWave" and sr.K_LW_STEP == 128
    assert const("scan_lines.inc", "kLwQCap") == str(sr.K_LW_QCAP)
    assert const("scan_lines.inc", "kLwInPlace") == str(sr.K_LW_IN_PLACE)
    assert "int finish_from(int k) { return 8 + 4 * max(k, 0); }" in text["device_common.inc"]
    first = "a.k <= 0 ? 2 : (a.k == 1 ? 3 : (a.k == 2 ? 5 : (a.k == 3 ? 6 : 8)))"
    assert first in text["welldup_queue.hip"] and first.replace("a.k", "kk") in text["welldup_scan.hip"]
    assert [sr.auto_first(k) for k in range(5)] == [2, 3, 5, 6, 8]
    # the invariants of the queues' sizes are compile-time checks
    assert "static_assert(kQCap >= kPass && kQCap >= kFinishAllMax" in text["scan_queue.inc"]
    assert "static_assert(kLwQCap >= kLwStep && kLwQCap >= kFinishAllMax" in text["scan_lines.inc"]


@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_builder_keeps_its_conventions(name):
    c = sr.case(name)
    g = c.geom
    wells = np.concatenate([g.centre, g.nbr])
    assert np.unique(wells).shape[0] == wells.shape[0] == g.n                 # all wells disjoint
    assert (np.diff(g.nbr) > 0).all()                                          # pair order by well = (target, slot) order
    assert c.line_pairs // g.K + 2 <= sr.K_LW_TARGETS                          # blocks stay under build_line_tables' other cut
    for s in c.tiles:
        b = np.stack(s.planes, axis=1)
        assert ((b == 0) == (s.codes == 0)).all() and (b[b != 0] >> 2 != 0).all()   # N = 0, quality bits else
        assert (s.codes[g.centre] == 0).any()
        assert not s.valid[c.bad].any() and s.valid.sum() == g.T - len(c.bad)
        assert ((s.filt[g.nbr] & 1) == 0).any()                                # neighbours that fail the filter
        assert len(np.unique(s.filt >> 1)) > 16                                # the other bits are noise
        # the script's convention: death d >= k + 1 is the cycle of the (k + 1)-th mismatch, else a duplicate
        di = s.death_index(c.k)
        want = np.where(s.death >= c.k + 1, s.death - 1, s.L)
        assert (di == want).all()
        n_mm = s.mismatches().sum(axis=2)
        dup = s.death <= c.k
        assert (n_mm[dup] <= c.k).all() and (n_mm[(s.death > 0) & dup] == s.death[(s.death > 0) & dup]).all()
        assert (n_mm[~dup] == c.k + 1).all()
    assert (c.tiles[0].death != c.tiles[1].death).any()                        # two tiles, two scripts


@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_every_case_enters_its_regimes(name):
    """Row by row: whatever the code's structure lets an input of this shape reach is reached (>= 1), by both tiles;
    whatever it cannot reach is not (the model agrees with the structure)."""
    c = sr.case(name)
    for lp in ((c.line_pairs, 512) if c.kernel == "lines" else (None,)):
        possible = sr.possible_rows(c.B1, c.k, c.L, c.layout, c.units_per_wave(lp), c.thr)
        for i in range(2):
            R = c.regimes(i, lp)
            if c.kind == "striped":
                # any 128 consecutive pairs hold 42 or 43 survivors: both sides of kLwInPlace, nothing else
                alive = (np.where(c.tiles[i].valid[:, None], c.tiles[i].death_index(c.k), -1) >= c.B1).reshape(-1)
                run = np.convolve(alive[:(c.geom.T - 70) * c.geom.K], np.ones(128, dtype=np.int64), "valid")
                assert set(np.unique(run)) == {sr.K_LW_IN_PLACE - 1, sr.K_LW_IN_PLACE}
                assert R["queued_top"] >= 1 and R["inplace_at"] >= 1, (name, lp, i, R)
                continue
            for row in sr.REGIME_ROWS:
                if row in possible:
                    assert R[row] >= 1, "%s (line_pairs %s, tile %d): regime %s is empty: %r" % (name, lp, i, row, R)
                else:
                    assert R[row] == 0, "%s (line_pairs %s, tile %d): regime %s cannot be entered: %r" % (name, lp, i, row, R)


@pytest.mark.parametrize("layout", ["plane", "il"])
@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("kernel", ["queue", "lines"])
def test_every_regime_is_entered_for_every_threshold_and_layout(kernel, k, layout):
    """Over the cases of one kernel, threshold and layout every row of the table is >= 1: what one read length
    cannot reach (a ragged last chunk where L - B1 is a multiple of 4, a short last round where the rounds end at L)
    another one does."""
    total = {r: 0 for r in sr.REGIME_ROWS}
    for name, spec in sr.CASES.items():
        if spec[0] == kernel and spec[5] == k and spec[6] == layout and len(spec) == 7:
            for i in range(2):
                for r, v in sr.case(name).regimes(i).items():
                    total[r] += v
    empty = [r for r in sr.REGIME_ROWS if total[r] == 0]
    assert not empty, (kernel, k, layout, empty)


@pytest.mark.parametrize("name", sorted(sr.CASES))
def test_model_duplicates_equal_the_oracle(name):
    """The model's set of duplicate pairs is the oracle's Hamming result, pair for pair."""
    c = sr.case(name)
    g = c.geom
    for i, s in enumerate(c.tiles):
        valid, dups, lens, dist = oracle_tile(c, i, 1, c.k)
        assert (valid.astype(bool) == s.valid).all()
        want = (dist.reshape(g.T, g.K) <= c.k) & s.valid[:, None]
        got = s.model_duplicates(c.k)
        assert (got == want).all() and got.sum() > 0
        per_level = np.stack([got[:, a:b].sum(axis=1) for a, b in zip(g.lvl_off[0, :-1], g.lvl_off[0, 1:])], axis=1)
        assert (per_level[s.valid] == dups[s.valid]).all()


def test_edit_scripts_are_close_in_edit_distance_and_far_in_hamming():
    c = sr.case("q_k2_plane_L37")
    s = sr.add_edit_scripts(np.random.default_rng(5), c.tiles[0])
    g = c.geom
    lev = oracle.count_tile(s.planes, s.filt, *g.csr(), 2, 2, want_dist=True)[3]
    ham = oracle.count_tile(s.planes, s.filt, *g.csr(), 1, 2, want_dist=True)[3]
    p = np.arange(0, g.T * g.K, 7)
    assert (lev[p] <= 2).all()
    assert (ham[p] > 2).mean() > 0.8 and (ham[p] > 10).any()
    assert (lev[p[0::2]] <= 2).all() and (lev[p[1::2]] == 2).any()             # shifts, and an insertion with a deletion
