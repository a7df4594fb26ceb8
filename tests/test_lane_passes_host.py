"""The table of the passes after a lane's finish (well_duplicates_amd/lane_passes.py): its order, and the defaults of
every pass - command line -> parameters is a pure function, checked here against what the help texts promise."""
from types import SimpleNamespace

import numpy as np
import pytest

from well_duplicates_amd import _lib
from well_duplicates_amd import count_well_duplicates as cwd
from well_duplicates_amd import lane_passes

# the order the blocks are documented to print in (the module docstring of the CLI, the help of every pass: "after
# every other block of the lane", in the order the passes were added)
ORDER = ["--lane-dups-mismatches", "--lane-dups-distance", "--lane-dups-quality", "--lane-dups-saturation", "--lane-dups-top",
         "--lane-dups-hops", "--lane-dups-gc", "--lane-dups-consensus", "--lane-dups-umi", "--lane-dups-keep"]
X, Y = np.arange(6), np.arange(6) * 2
RUN = SimpleNamespace(xy=(X, Y), cycle_list=list(range(15)))
BINS = cwd.DEFAULT_QUALITY_BINS


def _resolve(extra):
    args = cwd.parse_args(["-s", "hiseq_x", "-r", "/nowhere", "--all-wells", "--lane-dups"] + extra)
    return {p.flag: params for p, params in lane_passes.resolve_passes(args, RUN)}


def test_the_table_is_in_the_documented_order():
    assert [p.flag for p in lane_passes.LANE_PASSES] == ORDER
    assert len({p.key for p in lane_passes.LANE_PASSES}) == len(ORDER)
    doc = cwd.__doc__
    at = [doc.index(" " + flag + " ") for flag in ORDER if flag != "--lane-dups-mismatches"]
    assert at == sorted(at)
    # the clauses of the memory message follow it too
    flags = [flag for p in lane_passes.LANE_PASSES for _, flag in p.fit]
    assert [f for i, f in enumerate(flags) if f not in flags[:i]] == ORDER + ["--lane-dups-keep-umi"]


HAM, MIS = ["--lane-dups-hamming", "3"], ["--lane-dups-hamming", "3", "--lane-dups-mismatches"]
CASES = [
    # a pass that is not asked for resolves to nothing
    ([], {}),
    (HAM, {}),
    # mismatches: max-d explicit, else K
    (MIS, {"--lane-dups-mismatches": {"d": 3}}),
    (MIS + ["--lane-dups-mismatches-max-d", "0"], {"--lane-dups-mismatches": {"d": 0}}),
    # quality max-d: explicit, else the mismatches max-d, else K, else 0 without --lane-dups-hamming
    (["--lane-dups-quality"], {"--lane-dups-quality": {"edges": BINS, "d": 0}}),
    (HAM + ["--lane-dups-quality"], {"--lane-dups-quality": {"edges": BINS, "d": 3}}),
    (MIS + ["--lane-dups-mismatches-max-d", "1", "--lane-dups-quality"],
     {"--lane-dups-mismatches": {"d": 1}, "--lane-dups-quality": {"edges": BINS, "d": 1}}),
    (MIS + ["--lane-dups-mismatches-max-d", "1", "--lane-dups-quality", "--lane-dups-quality-max-d", "0",
            "--lane-dups-quality-bins", "0,7,30"],
     {"--lane-dups-mismatches": {"d": 1}, "--lane-dups-quality": {"edges": [0, 7, 30], "d": 0}}),
    # consensus max-d: the same chain; max-family 256
    (["--lane-dups-consensus"], {"--lane-dups-consensus": {"d": 0, "max_family": 256}}),
    (HAM + ["--lane-dups-consensus"], {"--lane-dups-consensus": {"d": 3, "max_family": 256}}),
    (MIS + ["--lane-dups-mismatches-max-d", "2", "--lane-dups-consensus", "--lane-dups-consensus-max-family", "9"],
     {"--lane-dups-mismatches": {"d": 2}, "--lane-dups-consensus": {"d": 2, "max_family": 9}}),
    (MIS + ["--lane-dups-mismatches-max-d", "2", "--lane-dups-consensus", "--lane-dups-consensus-max-d", "0"],
     {"--lane-dups-mismatches": {"d": 2}, "--lane-dups-consensus": {"d": 0, "max_family": 256}}),
    # distance: the coordinates and the radius, 2500 by default
    (["--lane-dups-distance"], {"--lane-dups-distance": {"x": X, "y": Y, "radius": 2500}}),
    # saturation: steps 20, seed 0; radius explicit, else the distance radius only when --lane-dups-distance is given,
    # else 0; no coordinates at radius 0
    (["--lane-dups-saturation"], {"--lane-dups-saturation": {"steps": 20, "seed": 0, "x": None, "y": None, "radius": 0}}),
    (["--lane-dups-saturation", "--lane-dups-distance-radius", "77"],
     {"--lane-dups-saturation": {"steps": 20, "seed": 0, "x": None, "y": None, "radius": 0}}),
    (["--lane-dups-saturation", "--lane-dups-distance", "--lane-dups-distance-radius", "77"],
     {"--lane-dups-distance": {"x": X, "y": Y, "radius": 77},
      "--lane-dups-saturation": {"steps": 20, "seed": 0, "x": X, "y": Y, "radius": 77}}),
    (["--lane-dups-saturation", "--lane-dups-distance", "--lane-dups-saturation-radius", "0", "--lane-dups-saturation-steps", "1",
      "--lane-dups-saturation-seed", "9"],
     {"--lane-dups-distance": {"x": X, "y": Y, "radius": 2500},
      "--lane-dups-saturation": {"steps": 1, "seed": 9, "x": None, "y": None, "radius": 0}}),
    (["--lane-dups-saturation", "--lane-dups-saturation-radius", "5"],
     {"--lane-dups-saturation": {"steps": 20, "seed": 0, "x": X, "y": Y, "radius": 5}}),
    # top: N as given
    (["--lane-dups-top", "7"], {"--lane-dups-top": {"n": 7}}),
    # hops: E 1 and 10 pairs from the bare flag; 0 pairs is a valid request
    (["--lane-dups-index", "15-21", "--lane-dups-hops"], {"--lane-dups-hops": {"e": 1, "pairs": 10}}),
    (["--lane-dups-index", "15-21", "--lane-dups-hops", "0", "--lane-dups-hops-mismatches", "0"],
     {"--lane-dups-hops": {"e": 0, "pairs": 0}}),
    # gc: 20 bins, max-n 0
    (["--lane-dups-gc"], {"--lane-dups-gc": {"max_n": 0, "bins": 20}}),
    (["--lane-dups-gc", "--lane-dups-gc-bins", "5", "--lane-dups-gc-max-n", "15"], {"--lane-dups-gc": {"max_n": 15, "bins": 5}}),
    # umi: E 1, max-family 256, the molecules written down only under --lane-dups-keep-umi
    (["--lane-dups-umi", "15-17,20-22"],
     {"--lane-dups-umi": {"cycles": [15, 16, 20, 21], "e": 1, "max_family": 256, "molecules": False}}),
    (["--lane-dups-umi", "15-17", "--lane-dups-umi-mismatches", "0", "--lane-dups-umi-max-family", "2"],
     {"--lane-dups-umi": {"cycles": [15, 16], "e": 0, "max_family": 2, "molecules": False}}),
    (["--lane-dups-umi", "15-17", "--lane-dups-keep", "--lane-dups-keep-umi"],
     {"--lane-dups-umi": {"cycles": [15, 16], "e": 1, "max_family": 256, "molecules": True},
      "--lane-dups-keep": {"min_q": _lib.LANEKEEP_DEFAULT_MIN_Q, "edges": BINS, "out": None, "by_molecule": True}}),
    # keep: min-q LANEKEEP_DEFAULT_MIN_Q, the edges of --lane-dups-quality-bins (accepted with --lane-dups-keep alone)
    (["--lane-dups-keep"],
     {"--lane-dups-keep": {"min_q": _lib.LANEKEEP_DEFAULT_MIN_Q, "edges": BINS, "out": None, "by_molecule": False}}),
    (["--lane-dups-keep", "--lane-dups-keep-min-q", "0", "--lane-dups-quality-bins", "0,20", "--lane-dups-keep-out", "dir"],
     {"--lane-dups-keep": {"min_q": 0, "edges": [0, 20], "out": "dir", "by_molecule": False}}),
]


def _same(got, want):
    assert list(got) == list(want)
    for key in want:
        if isinstance(want[key], np.ndarray):
            assert got[key] is want[key], key       # (the coordinates are handed on, not copied)
        else:
            assert got[key] == want[key] and type(got[key]) is type(want[key]), (key, got[key], want[key])


@pytest.mark.parametrize("extra,want", CASES, ids=[" ".join(c[0])[:70] or "nothing" for c in CASES])
def test_defaults_of_the_passes(extra, want):
    got = _resolve(extra)
    assert [f for f in ORDER if f in got] == list(got) and set(got) == set(want)
    for flag in want:
        _same(got[flag], want[flag])


def test_gc_max_n_beyond_the_scanned_cycles_is_a_value_error_of_the_run():
    with pytest.raises(ValueError, match=r"--lane-dups-gc-max-n takes 0\.\.15, the scanned cycles, not 16"):
        _resolve(["--lane-dups-gc", "--lane-dups-gc-max-n", "16"])


def test_the_parts_of_the_accumulator_are_asked_for_by_the_passes():
    """The qualities beside the reads: by the quality pass and by the keep; the UMI side batch: by the UMI pass."""
    def parts(extra):
        args = cwd.parse_args(["-s", "hiseq_x", "-r", "/nowhere", "--all-wells", "--lane-dups"] + extra)
        return [p.parts(params) for p, params in lane_passes.resolve_passes(args, RUN)]
    assert parts(["--lane-dups-gc", "--lane-dups-top", "3"]) == [{}, {}]
    assert parts(["--lane-dups-quality"]) == [{"quality": BINS}]
    assert parts(["--lane-dups-keep", "--lane-dups-quality-bins", "0,9"]) == [{"quality": [0, 9]}]
    assert parts(["--lane-dups-umi", "3-5", "--lane-dups-gc"]) == [{}, {"sides": {"umi": [3, 4]}}]


def test_the_memory_check_counts_a_shared_region_once():
    """--lane-dups-keep alone counts the quality part and the quality scratch, under the quality pass's keyword."""
    sc = SimpleNamespace(lane_qual_workspace_bytes=lambda n, t, c: 1000 * n, lane_qual_scratch_bytes=lambda t: 10 * t,
                         lane_keep_scratch_bytes=lambda t, n: 7, lane_molecules_bytes=lambda t, n: 5)
    run = SimpleNamespace(xy=(X, Y), cycle_list=list(range(15)), n_wells=3, n_tiles=4)

    def parts(extra):
        args = cwd.parse_args(["-s", "hiseq_x", "-r", "/nowhere", "--all-wells", "--lane-dups"] + extra)
        got = {}
        for p, params in lane_passes.resolve_passes(args, run):
            got.update(p.bytes(sc, run, params))
        return got
    assert parts(["--lane-dups-keep"]) == {"quality": 3040, "keep": 7}
    assert parts(["--lane-dups-keep", "--lane-dups-quality"]) == {"quality": 3040, "keep": 7}
    with pytest.raises(MemoryError) as e:
        cwd.check_lane_dups_fits(100, 3000, 4, 3, 15, **parts(["--lane-dups-keep"]))
    assert "(3147 bytes, 3040 of them for --lane-dups-quality, 7 of them for --lane-dups-keep), and" in str(e.value)
    with pytest.raises(TypeError):
        cwd.check_lane_dups_fits(100, 3000, 4, 3, 15, keeps=1)
