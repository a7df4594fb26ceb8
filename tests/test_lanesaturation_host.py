"""A lane's distinct reads against its depth without a GPU: the numpy reference of tests/lanesaturation_ref.py against
the identities include/welldup_lanesaturation.h states and against fixed step values, the header against the binding,
the scratch arithmetic, the CLI's flag checks, the fit check, the report's text and what the curve says of a finite
library."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from lanedistance_ref import lane_distances
from lanesaturation_ref import (HEAD_COLS, MAX_RADIUS, MAX_STEPS, check_saturation_identities, coarsen, dropped_wells,
                                lane_saturation, step_of)
from tiledups_ref import INVALID
from well_duplicates_amd import _lib, report
from well_duplicates_amd import count_well_duplicates as cwd

HEADER = os.path.join(_lib.INCLUDE, "welldup_lanesaturation.h")


# ---- the reference ------------------------------------------------------------------------------
def test_fixed_step_values():
    assert step_of(np.arange(8), 0, 64).tolist() == [0, 20, 12, 33, 9, 51, 23, 6]
    assert step_of([(1 << 32) - 2], 7, 64).tolist() == [46]
    for s in (1, 2, 7, 20, 64):                                        # every step in range, and the halving the header names
        a, b = step_of(np.arange(5000), 12345, s), step_of(np.arange(5000), 12345, min(2 * s, 64))
        assert a.min() >= 0 and a.max() == s - 1
        assert 2 * s > 64 or (b // 2 == a).all()
    assert (step_of(np.arange(100), 0, 1) == 0).all()


def _random_lane(rng, n, max_tiles, added, share=0.35):
    """labels uint32 [max_tiles, n]: PF wells of the added tiles, `share` of them members of an earlier PF well"""
    labels = np.full(max_tiles * n, INVALID, dtype=np.uint32)
    for t in added:
        ids = np.arange(t * n, (t + 1) * n)
        pf = ids[rng.random(n) < 0.9]
        labels[pf] = pf
    pf = np.flatnonzero(labels != INVALID)
    for g in pf[rng.random(pf.size) < share].tolist():
        earlier = pf[:np.searchsorted(pf, g)]
        roots = earlier[labels[earlier] == earlier]
        if roots.size:                                                 # half of them on the well's own tile where there is one
            own = roots[roots // n == g // n]
            labels[g] = rng.choice(own if own.size and rng.random() < 0.5 else roots)
    flat = labels
    member = np.flatnonzero((flat != INVALID) & (flat != np.arange(flat.size)))
    assert (flat[flat[member]] == flat[member]).all()
    return labels.reshape(max_tiles, n)


def test_reference_identities_on_a_random_lane():
    rng = np.random.default_rng(64)
    n, max_tiles, added = 400, 4, [0, 1, 3]
    labels = _random_lane(rng, n, max_tiles, added)
    x, y = rng.integers(0, 3000, n), rng.integers(0, 3000, n)
    flat = labels.reshape(-1)
    pf = int((flat != INVALID).sum())
    redundant = int(((flat != INVALID) & (flat != np.arange(flat.size))).sum())
    finish_lane = [pf, 0, 0, redundant]
    assert redundant > 200
    for radius, coords in ((0, False), (0, True), (32, True), (700, True), (MAX_RADIUS, True)):
        cx, cy = (x, y) if coords else (None, None)
        dist = lane_distances(labels, n, max_tiles, x, y, radius)[0]
        res = {(s, seed): lane_saturation(labels, n, max_tiles, s, seed, cx, cy, radius)
               for s in (1, 10, 20, 40, 32, 64) for seed in (0, 99)}
        for (s, seed), got in res.items():
            check_saturation_identities(*got, finish_lane=finish_lane, local=int(dist[2]),
                                        finer=res.get((2 * s, seed)), other_seed=res[(s, 99 - seed)])
        assert (coarsen(coarsen(res[(40, 0)][1])) == res[(10, 0)][1]).all()
        assert (coarsen(coarsen(res[(40, 0)][2])) == res[(10, 0)][2]).all()
        one = res[(1, 0)]
        assert one[1].tolist() == [pf - int(dist[2])] and one[2].tolist() == [pf - redundant]
        assert (res[(20, 0)][1] != res[(20, 99)][1]).any()              # (another seed is another draw)
    assert 0 < lane_distances(labels, n, max_tiles, x, y, 700)[0][2] < lane_distances(labels, n, max_tiles, x, y, MAX_RADIUS)[0][2]
    assert not dropped_wells(labels, n, max_tiles, x, y, 0).any() and not dropped_wells(labels, n, max_tiles).any()
    # a lane without a class
    single = np.where(flat != INVALID, np.arange(flat.size), INVALID).astype(np.uint32)
    got = lane_saturation(single, n, max_tiles, 20, 5, x, y, 2500)
    check_saturation_identities(*got, finish_lane=[pf, 0, 0, 0], local=0, no_class=True)
    # dropping matters: a class whose earliest-step member is dropped is found at a later step
    assert (lane_saturation(labels, n, max_tiles, 20, 0, x, y, MAX_RADIUS)[2] !=
            lane_saturation(labels, n, max_tiles, 20, 0)[2]).any()


def test_a_hand_worked_lane():
    """One tile index of two, six wells: well 0 the root of 2 and 5, well 3 single, well 1 not PF, well 4 a member
    of 3.  Steps by the fixed values at S = 64, seed 0: ids 6..11 are [23, 6, ...]: worked out from step_of itself
    for the ids used, then held against the definitions by hand."""
    n, max_tiles = 6, 2
    labels = np.full(12, INVALID, dtype=np.uint32)
    base = 6                                                           # tile index 1
    labels[base + 0], labels[base + 2], labels[base + 5] = base, base, base
    labels[base + 3], labels[base + 4] = base + 3, base + 3
    st = step_of(np.arange(12), 0, 64)
    head, r, d = lane_saturation(labels, n, max_tiles, 64, 0)
    assert head.tolist() == [5, 0] and r.sum() == 5 and d.sum() == 2
    want_d = np.zeros(64, dtype=np.int64)
    want_d[min(st[6], st[8], st[11])] += 1
    want_d[min(st[9], st[10])] += 1
    assert (d == want_d).all() and (r == np.bincount(st[[6, 8, 9, 10, 11]], minlength=64)).all()
    x, y = np.array([0, 0, 10, 0, 5000, 20]), np.zeros(6, dtype=np.int64)
    head, r, d = lane_saturation(labels, n, max_tiles, 64, 0, x, y, 25)       # wells 2 and 5 are closer than 25 to well 0
    assert head.tolist() == [5, 2] and r.sum() == 3
    want_d[:] = 0
    want_d[st[6]] += 1
    want_d[min(st[9], st[10])] += 1
    assert (d == want_d).all()
    head, r, d = lane_saturation(labels, n, max_tiles, 64, 0, x, y, 20)       # strictly less: well 5 at 20 stays
    assert head.tolist() == [5, 1]


# ---- C ABI --------------------------------------------------------------------------------------
def test_lanesaturation_header_and_binding_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert '#include "welldup_lanedistance.h"' in text
    syms = sorted(set(re.findall(r"\b(wd_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.LANESATURATION_PROTOTYPES) == ["wd_lane_saturation", "wd_lane_saturation_scratch"]
    assert int(re.search(r"#define WD_LANESATURATION_MAX_STEPS\s+(\d+)", text).group(1)) == _lib.LANESATURATION_MAX_STEPS == MAX_STEPS
    assert int(re.search(r"#define WD_LANESATURATION_HEAD_COLS\s+(\d+)", text).group(1)) == _lib.LANESATURATION_HEAD_COLS == HEAD_COLS
    assert _lib.LANESATURATION_MAX_RADIUS == MAX_RADIUS == report.LANE_SATURATION_MAX_RADIUS
    assert report.LANE_SATURATION_MAX_STEPS == MAX_STEPS
    taken = set()
    for table in (_lib.PROTOTYPES, _lib.SETS_PROTOTYPES, _lib.TILEDUPS_PROTOTYPES, _lib.TILENEAR_PROTOTYPES,
                  _lib.LANEDUPS_PROTOTYPES, _lib.LANENEAR_PROTOTYPES, _lib.LANEINDEX_PROTOTYPES, _lib.LANEMISMATCH_PROTOTYPES,
                  _lib.LANEDISTANCE_PROTOTYPES, _lib.LANEQUALITY_PROTOTYPES):
        taken |= set(table)
    assert not set(_lib.LANESATURATION_PROTOTYPES) & taken
    source = open(os.path.join(_lib.CSRC, "lane_saturation.inc")).read()
    for kernel in ("k_ls_min", "k_ls_tally"):
        assert kernel in source and _lib.unit_of_kernel(kernel) == "tiledups"
    assert "asm" not in source                                         # plain C++ and vector atomics only
    deps = {os.path.basename(f) for f in _lib._deps(os.path.join(_lib.CSRC, "welldup_tiledups.hip"))}
    assert {"lane_saturation.inc", "welldup_lanesaturation.h", "lane_distance.inc", "welldup_lanedistance.h"} <= deps
    quality = open(os.path.join(_lib.CSRC, "lane_quality.inc")).read()      # the unit's last line is pinned to that file:
    assert quality.rstrip().splitlines()[-2:] == ['#include "lane_saturation.inc"', "#endif"]      # it comes after all of it
    assert "k_ls_min and k_ls_tally (lane_saturation.inc)" in open(os.path.join(_lib.CSRC, "lane_mismatch.inc")).read()
    _lib.build()
    lib = _lib.load()
    for s in syms:                                                     # exported, and bound as the table says
        assert getattr(lib, s).argtypes == _lib.LANESATURATION_PROTOTYPES[s][1]
    ids = _lib.build_ids()
    assert ids["tiledups"] == _lib.source_unit_ids()["tiledups"] and ids["all"] == _lib.source_build_id()


def _formula(n, tiles, coords):
    """The arithmetic include/welldup_lanesaturation.h states."""
    up = lambda v: (v + 255) // 256 * 256
    return up(4 * tiles * n) + (up(8 * n) if coords else 0) + 65536 + 1024 + up(4 * tiles)


def _scratch(lib, n, tiles, coords):
    b = ctypes.c_size_t()
    rc = lib.wd_lane_saturation_scratch(n, tiles, coords, ctypes.byref(b))
    return rc, b.value


def test_scratch_size_needs_no_gpu_and_matches_the_header():
    _lib.build()
    lib = _lib.load()
    text = open(HEADER).read()
    for piece in ("4 * max_tiles * N", "+ 8 * N", "+ 65536", "+ 1024", "+ 4 * max_tiles", "rounded up to 256 bytes",
                  "1 965 267 712 bytes"):
        assert piece in text, piece
    for n in (0, 1, 31, 32, 33, 2640, 9000, 4309650):
        for tiles in (0, 1, 3, 7, 64, 65, 112, 4096):
            for coords in (0, 1):
                assert _scratch(lib, n, tiles, coords) == (0, _formula(n, tiles, coords)), (n, tiles, coords)
    assert _scratch(lib, 4309650, 112, 1) == (0, 1965267712)           # the header's HiSeq 4000 lane
    assert _scratch(lib, 10, 65535, 0)[0] == 0 and _scratch(lib, 10, 65536, 0)[0] == _lib.ERR_UNSUPPORTED
    assert _scratch(lib, -1, 3, 0)[0] == _lib.ERR_ARG and _scratch(lib, 10, -1, 1)[0] == _lib.ERR_ARG
    assert lib.wd_lane_saturation_scratch(10, 3, 1, None) == _lib.ERR_ARG
    row = (ctypes.c_int64 * 64)()                                      # a null handle is refused before anything is looked at
    xy = (ctypes.c_int32 * 8)()
    assert lib.wd_lane_saturation(None, 20, 0, xy, xy, 5, None, 0, row, row, row) == _lib.ERR_ARG


# ---- CLI ----------------------------------------------------------------------------------------
def test_cli_flag_checks(tmp_path, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["-s", "hiseq_4000", "-r", str(tmp_path), "--all-wells"]
    sat = ["--lane-dups", "--lane-dups-saturation"]
    args = cwd.parse_args(base + sat)
    assert args.lane_dups_saturation and args.lane_dups_saturation_steps is None and args.lane_dups_saturation_seed is None
    assert args.lane_dups_saturation_radius is None
    assert not cwd.parse_args(base + ["--lane-dups"]).lane_dups_saturation
    args = cwd.parse_args(base + sat + ["--lane-dups-saturation-steps", "64", "--lane-dups-saturation-seed",
                                        str((1 << 32) - 1), "--lane-dups-saturation-radius", str(1 << 25)])
    assert (args.lane_dups_saturation_steps, args.lane_dups_saturation_seed, args.lane_dups_saturation_radius) == \
        (64, (1 << 32) - 1, 1 << 25)
    args = cwd.parse_args(base + sat + ["--lane-dups-hamming", "2", "--lane-dups-distance", "--lane-dups-saturation-steps", "1",
                                        "--lane-dups-saturation-seed", "0", "--lane-dups-saturation-radius", "0"])
    assert (args.lane_dups_saturation_steps, args.lane_dups_saturation_seed, args.lane_dups_saturation_radius) == (1, 0, 0)
    needs = "--lane-dups-saturation-%s needs --lane-dups-saturation"
    for extra, message in ((["--lane-dups-saturation"], "--lane-dups-saturation needs --lane-dups"),
                           (["--tile-dups", "--lane-dups-saturation"], "--lane-dups-saturation needs --lane-dups"),
                           (["--lane-dups", "--lane-dups-saturation-steps", "20"], needs % "steps"),
                           (["--lane-dups", "--lane-dups-saturation-seed", "0"], needs % "seed"),
                           (["--lane-dups", "--lane-dups-distance", "--lane-dups-saturation-radius", "0"], needs % "radius"),
                           (sat + ["--lane-dups-saturation-steps", "0"], "--lane-dups-saturation-steps takes 1..64, not 0"),
                           (sat + ["--lane-dups-saturation-steps", "65"], "--lane-dups-saturation-steps takes 1..64, not 65"),
                           (sat + ["--lane-dups-saturation-seed", "-1"], "--lane-dups-saturation-seed takes 0..4294967295, not -1"),
                           (sat + ["--lane-dups-saturation-seed", str(1 << 32)],
                            "--lane-dups-saturation-seed takes 0..4294967295, not 4294967296"),
                           (sat + ["--lane-dups-saturation-radius", "-1"],
                            "--lane-dups-saturation-radius takes 0..33554432, not -1"),
                           (sat + ["--lane-dups-saturation-radius", str((1 << 25) + 1)],
                            "--lane-dups-saturation-radius takes 0..33554432, not 33554433")):
        with pytest.raises(SystemExit):
            cwd.parse_args(base + extra)
        assert message in " ".join(capsys.readouterr().err.split())
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cwd.parse_args(base + sat)
    assert "--lane-dups runs in a single process only" in " ".join(capsys.readouterr().err.split())


def test_cli_help_and_docstring_name_the_new_options(capsys):
    with pytest.raises(SystemExit):
        cwd.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for piece in ("--lane-dups-saturation ", "--lane-dups-saturation-steps S", "--lane-dups-saturation-seed SEED",
                  "--lane-dups-saturation-radius R", "(1..64, default 20)", "saturation curve"):
        assert piece in text, piece
    assert "--lane-dups-saturation" in cwd.__doc__ and "report.write_lane_saturation" in cwd.__doc__


def test_the_saturation_scratch_counts_when_a_lane_is_fitted():
    cwd.check_lane_dups_fits(1000, 2000, 2, 3, 4, scratch=500, distance=100, quality=300, saturation=100)
    with pytest.raises(MemoryError) as e:
        cwd.check_lane_dups_fits(1000, 2000, 2, 3, 4, scratch=500, distance=100, quality=300, saturation=101)
    msg = str(e.value)
    assert ("2001 bytes, 500 of them for --lane-dups-hamming, 100 of them for --lane-dups-distance, 300 of them for "
            "--lane-dups-quality, 101 of them for --lane-dups-saturation)") in msg and "2000 bytes" in msg
    with pytest.raises(MemoryError) as e:
        cwd.check_lane_dups_fits(1000, 1050, 2, 3, 4, saturation=51)
    assert "(1051 bytes, 51 of them for --lane-dups-saturation)" in str(e.value)
    with pytest.raises(MemoryError) as e:                              # without the flag the message is what it was
        cwd.check_lane_dups_fits(1000, 1400, 2, 3, 4, scratch=401)
    assert "(1401 bytes, 401 of them for --lane-dups-hamming)" in str(e.value)


# ---- the report ---------------------------------------------------------------------------------
def _text(counts, verbose=True):
    out = io.StringIO()
    report.write_lane_saturation("3", counts, verbose=verbose, out=out)
    return out.getvalue()


def test_fixed_counts_as_a_report():
    c = report.LaneSaturationCounts(pf=1000, dropped=10, redundant=100, new_reads=[495, 495], new_distinct=[470, 430],
                                    steps=2, seed=3, radius=2500, k=0)
    size = lambda n, d: "%.0f" % report.library_size(n, d)
    lines = _text(c).split("\n")
    assert lines[0] == "" and lines[-1] == "" and len(lines) == 9
    assert lines[1] == ("LaneSaturation: 3\tStep: 1/2\tShare: 0.50000\tReads: 495\tDistinct: 470\tDuplication: 0.05051\t"
                        "Library size: %s\tNewReads: 495\tNewDistinct: 470\tYield: 0.94949" % size(495, 470))
    assert lines[2] == ("LaneSaturation: 3\tStep: 2/2\tShare: 1.00000\tReads: 990\tDistinct: 900\tDuplication: 0.09091\t"
                        "Library size: %s\tNewReads: 495\tNewDistinct: 430\tYield: 0.86869" % size(990, 900))
    assert lines[3] == ("LaneSaturationSummary: 3\tSteps: 2\tSeed: 3\tHamming: 0\tPF wells: 1000\tDropped: 10\tReads: 990\t"
                        "Distinct: 900\tDuplication: 0.09091\tLibrary size: %s" % size(990, 900))
    assert lines[4] == ("New molecules per 1000 further reads (measured, no model: the last step's 495 reads brought 430): "
                        "868.7")
    ratio = report.library_size(990, 900) / report.library_size(495, 470)
    assert lines[5].startswith("Library size at full depth / at step 1/2: %.3f (near 1: " % ratio) and 1.0 < ratio < 1.2
    x = report.library_size(990, 900)
    proj = [x * (1 - np.exp(-f * 990 / x)) for f in (2, 4)]
    assert lines[6] == ("Projection (Lander-Waterman with the full-depth size, not a measurement): "
                        "2x reads: %.0f distinct, duplication %.5f\t4x reads: %.0f distinct, duplication %.5f" % (
                            proj[0], 1 - proj[0] / 1980, proj[1], 1 - proj[1] / 3960))
    assert 900 < proj[0] < proj[1] < x
    assert lines[7] == ("Local copies dropped: 10 closer than R = 2500 to the first well of their class on its tile "
                        "(0.01000 of PF wells)")
    short = _text(c, verbose=False).split("\n")
    assert short == [""] + lines[3:]                                   # the summary alone
    assert c.half_step() == 0 and report.LaneSaturationCounts(steps=20, new_reads=[1] * 20, new_distinct=[1] * 20).half_step() == 9
    assert report.LaneSaturationCounts(steps=7, new_reads=[1] * 7, new_distinct=[1] * 7).half_step() == 2


def test_zero_redundancy_and_an_empty_lane_as_a_report():
    c = report.LaneSaturationCounts(pf=10, dropped=0, redundant=0, new_reads=[4, 6], new_distinct=[4, 6], steps=2, seed=0,
                                    radius=0, k=2)
    text = _text(c)
    assert text.count("Library size: n/a") == 3 and "Hamming: 2" in text
    assert "Library size at full depth / at step 1/2: n/a (" in text
    assert "2x reads: n/a\t4x reads: n/a" in text and text.endswith("Local copies dropped: none (no radius)\n")
    assert "brought 6): 1000.0" in text
    empty = report.LaneSaturationCounts()
    text = _text(empty)
    assert "Reads: 0\tDistinct: 0\tDuplication: 0.00000\tLibrary size: n/a" in text and "brought 0): n/a" in text


def test_from_rows_holds_the_result_against_the_finish():
    final = report.LaneDupCounts(pf=1000, redundant=100)
    c = report.LaneSaturationCounts.from_rows([1000, 10], [495, 495], [470, 430], 3, 2500, final)
    assert c == report.LaneSaturationCounts(1000, 10, 100, [495, 495], [470, 430], 2, 3, 2500, 0)
    with pytest.raises(AssertionError):
        report.LaneSaturationCounts.from_rows([1000, 10], [495, 495], [470, 431], 3, 2500, final)
    with pytest.raises(AssertionError):
        report.LaneSaturationCounts.from_rows([1000, 10], [495, 494], [470, 430], 3, 2500, final)


# ---- what the curve says ------------------------------------------------------------------------
@pytest.mark.parametrize("trial", range(6))
def test_a_finite_library_is_found_from_half_the_reads_on(trial):
    """13 200 reads drawn uniformly from 6 000 molecules, ids in the order of the draw: every step of 20 brings reads
    and new molecules, and Lander-Waterman - whose assumption this is - gives the 6 000 within 15 % from the 10th
    step on (a simulation with this hash and 40 seeds: at worst 9.6 % from the 5th step on)."""
    molecules, reads, steps = 6000, 13200, 20
    rng = np.random.default_rng(trial)
    drawn = rng.integers(0, molecules, reads)
    _, first, inverse = np.unique(drawn, return_index=True, return_inverse=True)
    labels = first[inverse].astype(np.uint32)                          # the first well of the molecule
    head, r, d = lane_saturation(labels, reads, 1, steps, seed=trial)
    assert head.tolist() == [reads, 0] and (r > 0).all() and (d > 0).all()
    check_saturation_identities(head, r, d, finish_lane=[reads, 0, 0, reads - first.size])
    cr, cd = np.cumsum(r), np.cumsum(d)
    for j in range(9, steps):
        size = report.library_size(int(cr[j]), int(cd[j]))
        assert abs(size / molecules - 1.0) < 0.15, (j, size)
    counts = report.LaneSaturationCounts.from_rows(head, r, d, trial, 0, report.LaneDupCounts(pf=reads, redundant=reads - first.size))
    assert abs(counts.size_ratio() - 1.0) < 0.15                       # the model holds: the ratio is near 1
    assert (d / r)[-1] < (d / r)[0]                                    # and later reads bring less
