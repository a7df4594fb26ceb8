"""A lane's duplication per index read without a GPU: the host reference the GPU tests compare against (its two
implementations against each other and against a hand-worked lane, the header's identities), the C ABI and its
workspace arithmetic, the CLI's flag checks, the report block, the TSV and the fit check."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from laneindex_ref import (GROUP_COLS, HAND_INDEX, HAND_KEYS, LANE_COLS, MAX_CYCLES, check_index_identities,
                           hand_made_index, index_keys, key_of, lane_index, lane_index_literal)
from lanedups_ref import lane_dups
from lanenear_ref import HAND, hand_made_lane, lane_near_dups
from tiledups_ref import INVALID
from well_duplicates_amd import _lib, report
from well_duplicates_amd import count_well_duplicates as cwd

HEADER = os.path.join(_lib.INCLUDE, "welldup_laneindex.h")


def _same(a, b):
    assert all((np.asarray(x) == np.asarray(y)).all() and np.asarray(x).shape == np.asarray(y).shape for x, y in zip(a, b)), (a, b)


# ---- the host reference -------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1])
def test_references_give_the_hand_worked_answer(k):
    tiles, index = hand_made_lane(), hand_made_index()
    labels = lane_near_dups(tiles, 4, 5, k)[2]
    assert labels.tolist() == HAND[k]["labels"]
    assert HAND_KEYS == {name: key_of(name) for name in HAND_KEYS}
    for min_pf, want in HAND_INDEX[k].items():
        for fn in (lane_index, lane_index_literal):
            for order in (index, index[::-1]):
                lane, other, rows, keys = fn(order, labels, 4, 5, min_pf)
                assert lane.tolist() == want["lane"] and other.tolist() == want["other"]
                assert rows.tolist() == want["rows"] and keys.tolist() == [HAND_KEYS[name] for name in want["keys"]]
                check_index_identities((lane, other, rows, keys), HAND[k]["lane"])
    # the keys: well 16 fails the filter but has a key all the same; tile index 3 got no planes
    keys, given = index_keys(index, 4, 5)
    assert given.tolist() == [True, True, True, False, True] and keys[16] == HAND_KEYS["AC"] and (keys[12:16] == 0).all()


def _random_lane(seed, n, L, I, n_tiles, max_tiles, libraries):
    """Random reads with copies planted anywhere on the lane, index reads from a few libraries of skewed shares, some
    with an error or an N, and copies that keep or change their library."""
    rng = np.random.default_rng(seed)
    index = sorted(rng.choice(max_tiles, n_tiles, replace=False).tolist())
    m = n_tiles * n
    reads = rng.integers(1, 256, (m, L)).astype(np.uint8)
    reads[rng.random(reads.shape) < 0.01] = 0
    lib_reads = rng.integers(1, 256, (libraries, I)).astype(np.uint8)
    share = rng.random(libraries) ** 2 + 0.02
    idx = lib_reads[rng.choice(libraries, m, p=share / share.sum())]
    idx = (idx & 3) | (rng.integers(1, 64, idx.shape).astype(np.uint8) << 2)           # other quality bits
    err = rng.random(m) < 0.05
    col = rng.integers(0, I, m)
    idx[err, col[err]] = (idx[err, col[err]] + 1) & 3 | 4
    idx[rng.random(idx.shape) < 0.005] = 0
    for keep in (True, False, True):
        src, dst = rng.choice(m, m // 10, replace=False), rng.choice(m, m // 10, replace=False)
        reads[dst] = reads[src]
        if keep:
            idx[dst] = idx[src]
    filt = (rng.random(m) < 0.85).astype(np.uint8) | (rng.integers(0, 2, m).astype(np.uint8) << 1)
    tiles = [(ti, [np.ascontiguousarray(reads[i * n:(i + 1) * n, c]) for c in range(L)], filt[i * n:(i + 1) * n])
             for i, ti in enumerate(index)]
    itiles = [(ti, [np.ascontiguousarray(idx[i * n:(i + 1) * n, c]) for c in range(I)]) for i, ti in enumerate(index)]
    return tiles, itiles


@pytest.mark.parametrize("I", [1, 6, 10, 11, 20])
def test_the_references_agree_on_random_lanes(I):
    n, max_tiles = 300, 6
    tiles, itiles = _random_lane(5 + I, n, 12, I, 4, max_tiles, libraries=7)
    eq_lane, _, eq_labels = lane_dups(tiles, n, max_tiles)
    near_lane, _, near_labels = lane_near_dups(tiles, n, max_tiles, 1)
    for lane_row, labels in ((eq_lane, eq_labels), (near_lane, near_labels)):
        for min_pf in (1, 2, 30, 10 ** 6):
            a = lane_index(itiles, labels, n, max_tiles, min_pf)
            _same(a, lane_index_literal(itiles, labels, n, max_tiles, min_pf))
            check_index_identities(a, lane_row)
            assert a[0].shape == (LANE_COLS,) and a[1].shape == (GROUP_COLS,) and a[2].shape == (a[0][1], GROUP_COLS)
        lane, other, rows, keys = lane_index(itiles, labels, n, max_tiles, 30)
        assert lane[3] > 10 and lane[0] > (4 if I == 1 else 20) and other[0] > 0 and rows[:, 3].sum() > 10
        assert 2 <= rows.shape[0] <= 8
    # a single index read: one row [PF, InClasses, InClasses, Redundant, 0]
    one = [(ti, [np.full(n, 0x42, dtype=np.uint8)] * I) for ti, _ in itiles]
    lane, other, rows, keys = lane_index(one, eq_labels, n, max_tiles)
    assert lane.tolist() == [1, 1, eq_lane[1], 0, 0] and not other.any()
    assert rows.tolist() == [[eq_lane[0], eq_lane[2], eq_lane[2], eq_lane[3], 0]] and keys.tolist() == [key_of("G" * I)]
    # index cycles that are among the scanned ones: no class is mixed
    inside = [(ti, planes[3:3 + min(I, 9)]) for ti, planes, _ in tiles]
    lane, other, rows, keys = lane_index(inside, eq_labels, n, max_tiles)
    assert lane[2] == eq_lane[1] and lane[3] == 0 and lane[4] == 0 and not rows[:, 4].any()
    # a tile whose index planes are missing is noticed
    with pytest.raises(AssertionError):
        lane_index(itiles[1:], eq_labels, n, max_tiles)
    assert (eq_labels[[t for t in range(max_tiles) if t not in [x[0] for x in tiles]]] == INVALID).all()


# ---- C ABI --------------------------------------------------------------------------------------
def test_laneindex_header_and_binding_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert '#include "welldup_lanenear.h"' in text
    syms = sorted(set(re.findall(r"\b(wd_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.LANEINDEX_PROTOTYPES) == ["wd_lane_index_add", "wd_lane_index_begin", "wd_lane_index_finish",
                                                         "wd_lane_index_workspace"]
    assert int(re.search(r"#define WD_LANEINDEX_MAX_CYCLES (\d+)", text).group(1)) == _lib.LANEINDEX_MAX_CYCLES == MAX_CYCLES
    assert int(re.search(r"#define WD_LANEINDEX_GROUP_COLS (\d+)", text).group(1)) == _lib.LANEINDEX_GROUP_COLS == GROUP_COLS
    assert int(re.search(r"#define WD_LANEINDEX_LANE_COLS (\d+)", text).group(1)) == _lib.LANEINDEX_LANE_COLS == LANE_COLS
    assert GROUP_COLS == report.LANE_INDEX_GROUP_COLS and LANE_COLS == report.LANE_INDEX_LANE_COLS
    for kernel in ("k_li_pack", "k_li_group", "k_li_glabel", "k_li_sub", "k_li_tally", "k_li_emit", "k_li_rows"):
        assert _lib.unit_of_kernel(kernel) == "tiledups"
        assert kernel in open(os.path.join(_lib.CSRC, "lane_index.inc")).read()
    deps = {os.path.basename(f) for f in _lib._deps(os.path.join(_lib.CSRC, "welldup_tiledups.hip"))}
    assert {"lane_index.inc", "welldup_laneindex.h", "lane_near.inc", "lane_dups.inc", "read_classes.inc"} <= deps
    # the sources are included in this order: the index part uses what the near finish leaves behind
    unit = open(os.path.join(_lib.CSRC, "welldup_tiledups.hip")).read()
    assert unit.index('#include "lane_near.inc"') < unit.index('#include "lane_index.inc"')
    _lib.build()
    lib = _lib.load()
    for s in syms:
        assert getattr(lib, s).argtypes == _lib.LANEINDEX_PROTOTYPES[s][1]
    ids = _lib.build_ids()
    assert ids["tiledups"] == _lib.source_unit_ids()["tiledups"] and ids["all"] == _lib.source_build_id()
    # csrc/lane_index.inc is one of the sources the library's id is taken over; the header comes in through the unit's
    assert "lane_index.inc" in [f for f in os.listdir(_lib.CSRC) if f.endswith((".hip", ".inc", ".h"))]
    assert os.path.join(_lib.INCLUDE, "welldup_laneindex.h") in _lib._deps(os.path.join(_lib.CSRC, "welldup_tiledups.hip"))


def _formula(N, tiles, I):
    """The arithmetic include/welldup_laneindex.h states."""
    up = lambda v: (v + 255) // 256 * 256
    W = tiles * N
    return 4096 + 4096 + 256 + up(8 * tiles * I) + up(4 * tiles) + up(8 * W) + up(4 * W) + up(20 * W)


def _workspace(lib, N, tiles, I):
    b = ctypes.c_size_t()
    rc = lib.wd_lane_index_workspace(N, tiles, I, ctypes.byref(b))
    return rc, b.value


def test_workspace_size_needs_no_gpu_and_matches_the_header():
    _lib.build()
    lib = _lib.load()
    text = open(HEADER).read()
    for piece in ("4096 + 4096 + 256", "+ 8 * max_tiles * I", "+ 4 * max_tiles", "+ 8 * W", "+ 4 * W", "+ 20 * W",
                  "W = max_tiles * N", "rounded up to 256 bytes", "32 bytes per well", "15.4 GB"):
        assert piece in text, piece
    for N, tiles in [(2640, 7), (1000, 3), (1001, 3), (4309253, 112), (7, 1), (0, 3), (5, 0)]:
        for I in (1, 8, 10, 11, 20):
            rc, got = _workspace(lib, N, tiles, I)
            assert (rc, got) == (0, _formula(N, tiles, I)), (N, tiles, I)
            assert got <= 32 * N * tiles + 8448 + 8 * tiles * I + 4 * tiles + 5 * 256      # 32 bytes a well, small parts
    # the HiSeq 4000 lane at 8 index cycles: 32 bytes for each of 112 x 4 309 253 wells, and 16 KB in front of them
    W = 112 * 4309253
    assert _workspace(lib, 4309253, 112, 8) == (0, 15444379136) and 15444379136 - 32 * W == 16384
    # errors as wd_lane_dups_workspace, and I outside 1..20
    assert _workspace(lib, 4309253, 997, 8)[0] == _lib.ERR_UNSUPPORTED
    assert _workspace(lib, 65537, 65535, 8)[0] == _lib.ERR_UNSUPPORTED
    assert _workspace(lib, 10, 65536, 8)[0] == _lib.ERR_UNSUPPORTED
    for bad in ((-1, 2, 8), (10, -1, 8), (10, 2, -1), (10, 2, 0), (10, 2, 21)):
        assert _workspace(lib, *bad)[0] == _lib.ERR_ARG, bad
    assert lib.wd_lane_index_workspace(10, 1, 8, None) == _lib.ERR_ARG
    # a null handle is refused before anything is looked at
    row = (ctypes.c_int64 * 8)()
    n = ctypes.c_int64()
    assert lib.wd_lane_index_begin(None, 8, None, 0) == _lib.ERR_ARG
    assert lib.wd_lane_index_add(None, 0, None, None) == _lib.ERR_ARG
    assert lib.wd_lane_index_finish(None, 1, 0, row, row, None, None, ctypes.byref(n)) == _lib.ERR_ARG


# ---- CLI ----------------------------------------------------------------------------------------
def test_cli_flag_checks(tmp_path, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["-s", "hiseq_4000", "-r", str(tmp_path), "--all-wells"]
    args = cwd.parse_args(base + ["--lane-dups", "--lane-dups-index", "151-159,159-167"])
    assert args.lane_dups_index == "151-159,159-167" and args.lane_dups_index_min_share == 0.001
    args = cwd.parse_args(base + ["--lane-dups", "--lane-dups-index", "30-50", "--lane-dups-index-min-share", "1"])
    assert args.lane_dups_index_min_share == 1.0
    assert cwd.parse_args(base + ["--lane-dups"]).lane_dups_index is None
    for extra, message in ((["--lane-dups-index", "151-159"], "--lane-dups-index needs --lane-dups"),
                           (["--tile-dups", "--lane-dups-index", "151-159"], "--lane-dups-index needs --lane-dups"),
                           (["--lane-dups", "--lane-dups-index", "100-121"], "--lane-dups-index takes 1..20 cycles, not 21"),
                           (["--lane-dups", "--lane-dups-index", "0-11,20-30"], "--lane-dups-index takes 1..20 cycles, not 21"),
                           (["--lane-dups", "--lane-dups-index", "8-8"], "--lane-dups-index takes ranges of cycles"),
                           (["--lane-dups", "--lane-dups-index", "eight"], "--lane-dups-index takes ranges of cycles"),
                           (["--lane-dups", "--lane-dups-index", "0-8", "--lane-dups-index-min-share", "0"],
                            "--lane-dups-index-min-share takes a share in (0, 1], not 0"),
                           (["--lane-dups", "--lane-dups-index", "0-8", "--lane-dups-index-min-share", "1.01"],
                            "--lane-dups-index-min-share takes a share in (0, 1], not 1.01")):
        with pytest.raises(SystemExit):
            cwd.parse_args(base + extra)
        assert message in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cwd.parse_args(base + ["--lane-dups", "--lane-dups-index", "0-8"])
    err = " ".join(capsys.readouterr().err.split())
    assert "--lane-dups runs in a single process only" in err and "WORLD_SIZE" in err


def test_cli_help_names_the_new_options(capsys):
    with pytest.raises(SystemExit):
        cwd.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--lane-dups-index RANGES" in text and "--lane-dups-index-min-share F" in text and "index column" in text


def test_listing_from_the_share():
    assert cwd.index_listing(0.001, 482636336) == (482637, 1001)
    assert cwd.index_listing(0.001, 0) == (1, 1001) and cwd.index_listing(1.0, 77) == (77, 2)
    assert cwd.index_listing(0.3, 10) == (3, 4) and cwd.index_listing(0.01, 1234) == (13, 101)
    for f in (0.001, 0.01, 0.3, 0.07, 1.0):                            # the cap is never met: n groups of min_pf wells
        for pf in (1, 10, 999, 12345):                                # hold n * min_pf <= PF wells
            min_pf, cap = cwd.index_listing(f, pf)
            assert pf // min_pf < cap


def test_the_index_workspace_counts_when_a_lane_is_fitted():
    cwd.check_lane_dups_fits(1000, 1800, 2, 3, 4, scratch=500, index=300)
    with pytest.raises(MemoryError) as e:
        cwd.check_lane_dups_fits(1000, 1800, 2, 3, 4, scratch=500, index=301)
    msg = str(e.value)
    assert "1801 bytes, 500 of them for --lane-dups-hamming, 301 of them for --lane-dups-index" in msg and "1800 bytes" in msg
    with pytest.raises(MemoryError) as e:
        cwd.check_lane_dups_fits(1000, 1200, 2, 3, 4, index=201)
    assert "(1201 bytes, 201 of them for --lane-dups-index)" in str(e.value)
    cwd.check_lane_dups_fits(1000, 1000, 2, 3, 4)


# ---- report -------------------------------------------------------------------------------------
def test_index_bases():
    assert report.index_bases(key_of("ACGTN"), [5]) == "ACGTN"
    assert report.index_bases(key_of("ACGTNACGTNAC"), [8, 4]) == "ACGTNACG+TNAC"
    assert report.index_bases(key_of("T" * 20), [10, 10]) == "TTTTTTTTTT+TTTTTTTTTT"
    assert report.index_bases(key_of("GATTACAGATTACAGATTAC"), [1, 12, 7]) == "G+ATTACAGATTAC+AGATTAC"
    assert report.index_bases(0, [3]) == "AAA"


def test_lane_index_counts_and_text():
    # groups given out of order: by PF descending, equal PF by key (the first cycle is the lowest digit)
    rows = [[300, 0, 0, 0, 0], [500, 40, 30, 20, 10], [300, 12, 12, 6, 0]]
    keys = [key_of("AACG"), key_of("GGTT"), key_of("CAAA")]
    assert key_of("CAAA") < key_of("AACG")
    c = report.LaneIndexCounts.from_rows([9, 3, 70, 5, 12], [100, 8, 0, 0, 2], rows, keys, [3, 1], 1200, 42)
    assert [name for name, _ in c.rows] == ["GGT+T", "CAA+A", "AAC+G"]
    assert (c.groups, c.listed, c.group_spans, c.mixed_classes, c.mixed_wells, c.pf, c.classes) == (9, 3, 70, 5, 12, 1200, 42)
    assert c.within_libraries == 26 and c.across_libraries == 28
    out = io.StringIO()
    report.write_lane_index_dups("3", c, out=out)
    assert out.getvalue() == (
        "\n"
        "LaneIndexDups: 3\tIndex: GGT+T\tPF wells: 500 (0.41667)\tInGroup: 30\tGroupRedundant: 20 (0.04000)\t"
        "Library size: " + "%.0f" % report.library_size(500, 480) + "\tMixed: 10 (0.02000)\n"
        "LaneIndexDups: 3\tIndex: CAA+A\tPF wells: 300 (0.25000)\tInGroup: 12\tGroupRedundant: 6 (0.02000)\t"
        "Library size: " + "%.0f" % report.library_size(300, 294) + "\tMixed: 0 (0.00000)\n"
        "LaneIndexDups: 3\tIndex: AAC+G\tPF wells: 300 (0.25000)\tInGroup: 0\tGroupRedundant: 0 (0.00000)\t"
        "Library size: n/a\tMixed: 0 (0.00000)\n"
        "LaneIndexDups: 3\tIndex: Other\tPF wells: 100 (0.08333)\tInGroup: 0\tGroupRedundant: 0 (0.00000)\t"
        "Library size: n/a\tMixed: 2 (0.02000)\n"
        "LaneIndexDupsSummary: 3\tGroups: 9\tListed: 3\tRedundant within libraries: 26 (0.48148 of Redundant)\t"
        "across libraries: 28 (0.51852 of Redundant)\tMixedClasses: 5\n")
    out = io.StringIO()
    report.write_lane_index_dups("1", report.LaneIndexCounts.from_rows([0] * 5, [0] * 5, [], [], [8], 0, 0), hamming=2,
                                 out=out)
    assert out.getvalue() == (
        "\n"
        "LaneIndexDups: 1\tHamming: 2\tIndex: Other\tPF wells: 0 (0.00000)\tInGroup: 0\tGroupRedundant: 0 (0.00000)\t"
        "Library size: n/a\tMixed: 0 (0.00000)\n"
        "LaneIndexDupsSummary: 1\tHamming: 2\tGroups: 0\tListed: 0\tRedundant within libraries: 0 (0.00000 of Redundant)\t"
        "across libraries: 0 (0.00000 of Redundant)\tMixedClusters: 0\n")
    with pytest.raises(AssertionError):
        report.LaneIndexCounts.from_rows([9, 2, 70, 5, 12], [0] * 5, rows, keys, [4], 1200, 42)      # Listed is 3


def test_the_hand_worked_lane_as_a_report():
    labels = np.array(HAND[1]["labels"], dtype=np.uint32)
    got = lane_index(hand_made_index(), labels, 4, 5, 4)
    c = report.LaneIndexCounts.from_rows(*got, [1, 1], HAND[1]["lane"][0], HAND[1]["lane"][1])
    assert [(name, r) for name, r in c.rows] == [("A+C", [7, 6, 4, 3, 2]), ("G+T", [5, 4, 0, 0, 4])]
    assert c.other == [3, 2, 0, 0, 2] and c.within_libraries == 3 and c.across_libraries == 4
    assert c.within_libraries + c.across_libraries == HAND[1]["lane"][3]      # Redundant of the clusters


# ---- TSV ----------------------------------------------------------------------------------------
def test_lane_members_tsv_with_the_index_column(tmp_path):
    names = ["1101", "1102", "1103", None, "1105"]
    classes = np.array(HAND[0]["labels"], dtype=np.uint32)
    clusters = np.array(HAND[1]["labels"], dtype=np.uint32)
    keys = index_keys(hand_made_index(), 4, 5)[0]
    path = str(tmp_path / "lane.tsv")
    m = cwd.lane_members(classes)
    cwd.write_lane_members(path, {"2": (names,) + m}, index=([2], {"2": keys[m[0] * 4 + m[1]]}))
    assert open(path).read().splitlines() == [
        "lane\ttile\twell\tclass_tile\tclass_well\tindex", "2\t1101\t0\t1101\t0\tAC", "2\t1101\t2\t1101\t2\tAC",
        "2\t1105\t1\t1101\t2\tGT", "2\t1105\t2\t1101\t0\tAC"]
    m = cwd.lane_cluster_members(classes, clusters)
    cwd.write_lane_members(path, {"2": (names,) + m}, index=([1, 1], {"2": keys[m[0] * 4 + m[1]]}))
    lines = open(path).read().splitlines()
    assert lines[0] == "lane\ttile\twell\tclass_tile\tclass_well\tcluster_tile\tcluster_well\tindex"
    assert lines[1:4] == ["2\t1101\t0\t1101\t0\t1101\t0\tA+C", "2\t1101\t1\t1101\t1\t1101\t1\tA+C",
                          "2\t1101\t2\t1101\t2\t1101\t2\tA+C"]
    assert lines[-2:] == ["2\t1105\t1\t1101\t2\t1101\t2\tG+T", "2\t1105\t2\t1101\t0\t1101\t0\tA+C"] and len(lines) == 13
    assert [ln.split("\t")[-1] for ln in lines[4:-2]] == ["G+T", "A+C", "G+T", "N+N", "A+C", "G+T", "N+N"]
    # without the flag the file is what it was
    cwd.write_lane_members(path, {"2": (names,) + cwd.lane_members(classes)})
    assert open(path).read().splitlines()[0] == "lane\ttile\twell\tclass_tile\tclass_well"
