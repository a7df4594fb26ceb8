"""Read classes across the tiles of a lane without a GPU: the host reference the GPU tests compare against (its
two methods against each other and against a hand-worked lane), the identities of include/welldup_lanedups.h,
the C ABI and its workspace arithmetic, the CLI's flag checks, the report block and the TSV."""
import ctypes
import io
import math
import os
import re

import numpy as np
import pytest

from lanedups_ref import (LANE_COLS, TILE_COLS, check_identities, groups_by_dict, groups_by_unique, lane_dups,
                          lane_dups_literal, members_of, _lane_rows)
from tiledups_ref import INVALID, class_labels, codes_of
from well_duplicates_amd import _lib, report
from well_duplicates_amd import count_well_duplicates as cwd

HEADER = os.path.join(_lib.INCLUDE, "welldup_lanedups.h")
A, C, G, T = 0x40, 0x81, 0xC2, 0x23          # quality bits on top of the base's two low bits


# ---- the host reference -------------------------------------------------------------------------
def hand_made_lane():
    """Tile indices 0, 1 and 3 of a lane with room for four tiles, seven wells each, three cycles:
         index 0 (ids 0..6)    ACG  ACG  TTT  NNT  GGG* CCC  AAT          * fails the filter
         index 1 (ids 7..13)   TTT  ACG  NNT  AAT  CCC* GGG  GCA
         index 3 (ids 21..27)  ACG  ACG  GGG  CAT  TTT  TTT  CAT
    ACG = {0, 1, 8, 21, 22}, TTT = {2, 7, 25, 26}, NNT = {3, 9}, AAT = {6, 10} (bytes 0x04 0x08: A, not N),
    GGG = {12, 23} (well 4 of index 0 is not PF), CAT = {24, 27} on one tile; CCC (5) and GCA (13) are alone."""
    N0 = 0
    t0 = [(A, C, G), (A | 0x3C, C, G | 0x10), (T, T, T), (N0, N0, T), (G, G, G), (C, C, C), (A, A, T)]
    t1 = [(T | 0x40, T, T), (A, C | 0x04, G), (N0, N0, T | 0x80), (0x04, 0x08, T), (C, C, C), (G, G, G), (G, C, A)]
    t3 = [(A, C, G), (A, C, G), (G, G | 0x20, G), (C, A, T), (T, T, T), (T, T, T), (C, A, T)]
    f0 = [1, 1, 1, 3, 2, 1, 0x81]
    f1 = [1, 1, 1, 1, 0, 1, 1]
    f3 = [1] * 7
    mk = lambda reads: [np.array([r[c] for r in reads], dtype=np.uint8) for c in range(3)]
    return [(0, mk(t0), np.array(f0, dtype=np.uint8)), (1, mk(t1), np.array(f1, dtype=np.uint8)),
            (3, mk(t3), np.array(f3, dtype=np.uint8))]


HAND_LANE = [19, 6, 17, 11, 5, 13, 4, 0, 1, 1, 0, 0, 0, 0]
HAND_TILES = [[6, 5, 2, 1, 1], [6, 5, 0, 0, 4], [0, 0, 0, 0, 0], [7, 7, 6, 3, 6]]
HAND_LABELS = [[0, 0, 2, 3, INVALID, 5, 6], [2, 0, 3, 6, INVALID, 12, 13], [INVALID] * 7, [0, 0, 12, 24, 2, 2, 24]]


@pytest.mark.parametrize("fn", [lane_dups, lane_dups_literal])
@pytest.mark.parametrize("method", ["unique", "dict"])
def test_both_references_give_the_hand_worked_answer(fn, method):
    tiles = hand_made_lane()
    for order in (tiles, tiles[::-1]):
        lane, trow, labels = fn(order, 7, 4, method=method)
        assert lane.tolist() == HAND_LANE
        assert trow.tolist() == HAND_TILES
        assert labels.tolist() == HAND_LABELS
        check_identities(lane, trow)
    assert (lane[2] - lane[5], lane[5] - lane[1]) == (4, 7)           # redundant within tiles, across tiles


def _random_lane(seed, n, L, n_tiles, max_tiles):
    rng = np.random.default_rng(seed)
    index = sorted(rng.choice(max_tiles, n_tiles, replace=False).tolist())
    reads = rng.integers(1, 256, (n_tiles * n, L)).astype(np.uint8)
    reads[rng.random(reads.shape) < 0.01] = 0
    m = n_tiles * n
    src = rng.choice(m, m // 5, replace=False)
    dst = rng.choice(m, m // 5, replace=False)                         # copies anywhere on the lane, chains included
    reads[dst] = reads[src]
    flip = rng.choice(m, m // 20, replace=False)                       # quality bits never matter
    reads[flip] = np.where(reads[flip] == 0, 0, reads[flip] ^ 0x54)
    filt = (rng.random(m) < 0.85).astype(np.uint8) | (rng.integers(0, 2, m).astype(np.uint8) << 1)
    return [(ti, [np.ascontiguousarray(reads[i * n:(i + 1) * n, c]) for c in range(L)], filt[i * n:(i + 1) * n])
            for i, ti in enumerate(index)]


@pytest.mark.parametrize("L", [1, 9, 25])
def test_the_two_methods_agree_on_random_lanes(L):
    n, max_tiles = 300, 6
    tiles = _random_lane(3 + L, n, L, 4, max_tiles)
    ids, rows = _lane_rows(tiles, n)
    ga, gb = groups_by_unique(ids, rows), groups_by_dict(ids, rows)
    assert ((ga[:, None] == ga[None, :]) == (gb[:, None] == gb[None, :])).all()
    results = [fn(tiles, n, max_tiles, method=m) for fn in (lane_dups, lane_dups_literal) for m in ("unique", "dict")]
    for lane, trow, labels in results[1:]:
        assert (lane == results[0][0]).all() and (trow == results[0][1]).all() and (labels == results[0][2]).all()
    lane, trow, labels = results[0]
    assert lane.shape == (LANE_COLS,) and trow.shape == (max_tiles, TILE_COLS)
    # (one cycle: five reads exist; each of the four bases is a class on every tile, N on the tiles that have one)
    assert (lane[1] == 5 and 16 < lane[5] <= 20 if L == 1 else lane[1] > 20 and lane[4] > 10) and lane[0] < 4 * n
    check_identities(lane, trow)
    never = sorted(set(range(max_tiles)) - {t[0] for t in tiles})
    assert (trow[never] == 0).all() and (labels[never] == INVALID).all()


def test_identities_against_the_tile_reference():
    """Per tile, InTile / TileRedundant are InClasses / Redundant of the per-tile classes, and two wells of one tile
    share a lane label exactly when they share a tile label."""
    n, max_tiles = 400, 5
    tiles = _random_lane(77, n, 12, 5, max_tiles)
    for ti in (1, 3):                                                  # and copies inside a tile
        planes = tiles[ti][1]
        for p in planes:
            p[200:260] = p[100:160]
    lane, trow, labels = lane_dups(tiles, n, max_tiles)
    check_identities(lane, trow)
    assert trow[:, 3].sum() > 100 and lane[5] - lane[1] > 100
    for ti, planes, filt in tiles:
        pf = (filt & 1).astype(bool)
        tl = class_labels(codes_of(planes, n), pf)
        size = np.bincount(tl[pf].astype(np.int64), minlength=n)
        in_classes = int((size[tl[pf].astype(np.int64)] >= 2).sum())
        assert trow[ti, 2] == in_classes and trow[ti, 3] == in_classes - int((size >= 2).sum())
        w = np.flatnonzero(pf)
        assert ((labels[ti][w][:, None] == labels[ti][w][None, :]) == (tl[w][:, None] == tl[w][None, :])).all()
        assert ((labels[ti] == INVALID) == ~pf).all()


# ---- C ABI --------------------------------------------------------------------------------------
def test_lanedups_header_and_binding_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert '#include "welldup_tiledups.h"' in text
    syms = sorted(set(re.findall(r"\b(wd_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.LANEDUPS_PROTOTYPES) == ["wd_lane_dups_add", "wd_lane_dups_begin", "wd_lane_dups_end",
                                                         "wd_lane_dups_finish", "wd_lane_dups_workspace"]
    assert not set(syms) & (set(_lib.PROTOTYPES) | set(_lib.SETS_PROTOTYPES) | set(_lib.TILEDUPS_PROTOTYPES) |
                            set(_lib.TILENEAR_PROTOTYPES))
    assert int(re.search(r"#define WD_LANEDUPS_TILE_COLS (\d+)", text).group(1)) == _lib.LANEDUPS_TILE_COLS == TILE_COLS
    assert "#define WD_LANEDUPS_LANE_COLS (6 + WD_DUPSET_SIZE_BINS)" in text
    assert _lib.LANEDUPS_LANE_COLS == LANE_COLS == report.LANE_ROW_COLS
    for kernel in ("k_ld_pack<true>", "k_ld_pack<false>", "k_ld_insert", "k_ld_resolve", "k_ld_classes",
                   "k_ld_span_count", "k_ld_span_sum"):
        assert _lib.unit_of_kernel(kernel) == "tiledups"
    assert _lib.UNITS[-1] == "tiledups"
    _lib.build()
    lib = _lib.load()
    for s in syms:
        assert getattr(lib, s).argtypes == _lib.LANEDUPS_PROTOTYPES[s][1]
    lib.wd_lane_dups_end(None)                                         # NULL is fine


def test_build_id_covers_the_new_sources():
    deps = {os.path.basename(f) for f in _lib._deps(os.path.join(_lib.CSRC, "welldup_tiledups.hip"))}
    assert {"lane_dups.inc", "welldup_lanedups.h", "tile_near.inc", "near_core.inc", "read_classes.inc", "welldup_tiledups.h"} <= deps
    for u in _lib.UNITS[:-1]:
        other = {os.path.basename(f) for f in _lib._deps(os.path.join(_lib.CSRC, "welldup_%s.hip" % u))}
        assert not {"lane_dups.inc", "welldup_lanedups.h"} & other
    _lib.build()
    assert _lib.build_ids()["all"] == _lib.source_build_id()
    assert _lib.build_ids()["tiledups"] == _lib.source_unit_ids()["tiledups"]
    # the id of the whole is taken over csrc/* and the five public headers, the new one among them
    import hashlib
    h = hashlib.sha256()
    files = sorted(os.path.join(_lib.CSRC, f) for f in os.listdir(_lib.CSRC) if f.endswith((".hip", ".inc", ".h")))
    assert os.path.join(_lib.CSRC, "lane_dups.inc") in files
    files += [os.path.join(_lib.INCLUDE, f) for f in ("welldup.h", "welldup_sets.h", "welldup_tiledups.h",
                                                      "welldup_tilenear.h", "welldup_lanedups.h")]
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        h.update(open(f, "rb").read())
    assert h.hexdigest()[:16] == _lib.source_build_id()


def _formula(N, tiles, L):
    """The arithmetic include/welldup_lanedups.h states."""
    up = lambda v: (v + 255) // 256 * 256
    W, R = tiles * N, (L + 9) // 10
    S = 64
    while S < 2 * W:
        S *= 2
    parts = [512 * 8 * tiles, 512 * 16, 8 * tiles * L, 8 * tiles, 8 * tiles, 4 * tiles, 8 * S, 4 * R * W, 8 * W, 4 * W, 4 * W]
    return sum(up(p) for p in parts)


def _workspace(lib, N, tiles, L):
    b = ctypes.c_size_t()
    rc = lib.wd_lane_dups_workspace(N, tiles, L, ctypes.byref(b))
    return rc, b.value


def test_workspace_size_needs_no_gpu_and_matches_the_header():
    _lib.build()
    lib = _lib.load()
    text = open(HEADER).read()
    for piece in ("512 * (8 * max_tiles + 16)", "8 * max_tiles * L", "4 * max_tiles", "8 * S", "4 * R * W",
                  "8 * W + 4 * W + 4 * W", "R = ceil(L / 10)", "power of two >= max(64, 2 W)"):
        assert piece in text, piece
    for N, tiles, L in [(2640, 5, 40), (1000, 3, 1), (1000, 3, 10), (1000, 3, 11), (4309253, 112, 51), (4309253, 112, 151),
                        (7, 1, 0), (0, 3, 5), (5, 0, 5)]:
        assert _workspace(lib, N, tiles, L) == (0, _formula(N, tiles, L)), (N, tiles, L)
    # the sizing of a HiSeq 4000 lane: 8.6 GB of table; ~28 GB at 51 cycles, ~47 GB at 151, under 64 GB
    W = 112 * 4309253
    assert 2 * W <= 1 << 30 < 4 * W
    at51, at151 = _workspace(lib, 4309253, 112, 51)[1], _workspace(lib, 4309253, 112, 151)[1]
    assert 27e9 < at51 < 29e9 and 46e9 < at151 < 48e9 and at151 < 64e9
    assert at151 - at51 == pytest.approx(4 * 10 * W + 8 * 112 * 100, abs=4096)
    # monotone in each argument
    base = _workspace(lib, 100000, 8, 50)[1]
    for bigger in ((100001, 8, 50), (100000, 9, 50), (100000, 8, 51), (200000, 8, 50), (100000, 16, 50)):
        assert _workspace(lib, *bigger)[1] > base, bigger
    assert _workspace(lib, 100000, 8, 60)[1] - base >= 4 * 800000
    last = 0
    for L in range(0, 160):
        now = _workspace(lib, 4321, 7, L)[1]
        assert now >= last
        last = now
    # labels are 32-bit: max_tiles * N >= 2^32 - 1 is refused
    assert _workspace(lib, 4309253, 996, 50)[0] == 0                   # 4 292 015 988 wells
    assert _workspace(lib, 4309253, 997, 50)[0] == _lib.ERR_UNSUPPORTED
    assert _workspace(lib, (1 << 32) - 2, 1, 10)[0] == 0
    assert _workspace(lib, (1 << 32) - 1, 1, 10)[0] == _lib.ERR_UNSUPPORTED
    assert _workspace(lib, 65537, 65535, 10)[0] == _lib.ERR_UNSUPPORTED
    assert _workspace(lib, 10, 2, 1025)[0] == _lib.ERR_UNSUPPORTED and _workspace(lib, 10, 2, 1024)[0] == 0
    for bad in ((-1, 2, 10), (10, -1, 10), (10, 2, -1)):
        assert _workspace(lib, *bad)[0] == _lib.ERR_ARG
    assert lib.wd_lane_dups_workspace(10, 1, 10, None) == _lib.ERR_ARG


# ---- CLI ----------------------------------------------------------------------------------------
def test_cli_flag_checks(tmp_path, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["-s", "hiseq_4000", "-r", str(tmp_path)]
    args = cwd.parse_args(base + ["--all-wells", "--lane-dups", "--lane-dups-out", "x.tsv"])
    assert args.lane_dups and args.lane_dups_out == "x.tsv" and not args.tile_dups
    args = cwd.parse_args(base + ["--all-wells"])
    assert not args.lane_dups and args.lane_dups_out is None
    for extra, message in ((["-f", "targets.list", "--lane-dups"], "--lane-dups needs --all-wells"),
                           (["--all-wells", "--lane-dups-out", "x.tsv"], "--lane-dups-out needs --lane-dups")):
        with pytest.raises(SystemExit):
            cwd.parse_args(base + extra)
        assert message in capsys.readouterr().err
    monkeypatch.setenv("WORLD_SIZE", "2")
    assert cwd.parse_args(base + ["--all-wells", "--tile-dups"]).tile_dups
    with pytest.raises(SystemExit):
        cwd.parse_args(base + ["--all-wells", "--lane-dups"])
    err = " ".join(capsys.readouterr().err.split())
    assert "--lane-dups runs in a single process only" in err and "WORLD_SIZE" in err


def test_cli_help_names_the_new_options(capsys):
    with pytest.raises(SystemExit):
        cwd.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--lane-dups " in text and "--lane-dups-out PATH" in text and "on whatever tiles they lie" in text


def test_a_lane_that_does_not_fit_is_refused_with_both_figures():
    cwd.check_lane_dups_fits(1000, 1000, 2, 3, 4)
    with pytest.raises(MemoryError) as e:
        cwd.check_lane_dups_fits(47_000_000_000, 31_500_000_000, 112, 4309253, 151)
    msg = str(e.value)
    assert "--lane-dups needs 47.00 GB" in msg and "31.50 GB" in msg and "112 tiles x 4309253 wells x 151 cycles" in msg
    assert "47000000000 bytes" in msg and "31500000000 bytes" in msg


# ---- report -------------------------------------------------------------------------------------
def _hand_counts():
    return report.LaneDupCounts.from_rows(HAND_LANE, HAND_TILES, ["1101", "1102", None, "1104"])


def test_lanedup_counts_decode():
    c = _hand_counts()
    assert (c.pf, c.classes, c.in_classes, c.redundant, c.cross_tile_classes, c.tile_spans) == (19, 6, 17, 11, 5, 13)
    assert c.sizes == [4, 0, 1, 1, 0, 0, 0, 0] and sorted(c.tiles) == ["1101", "1102", "1104"]
    assert c.tiles["1104"] == [7, 7, 6, 3, 6]
    assert (c.within_tiles, c.across_tiles) == (4, 7) and c.lane_duplication() == 11 / 19
    assert c.to_rows() == (HAND_LANE, [HAND_TILES[0], HAND_TILES[1], HAND_TILES[3]])
    back = report.LaneDupCounts.from_rows(np.array(HAND_LANE), np.array(HAND_TILES)[:2], ["a", "b"])
    assert sorted(back.tiles) == ["a", "b"]
    with pytest.raises(AssertionError):
        report.LaneDupCounts.from_rows(HAND_LANE[:-1], HAND_TILES, ["a", "b", "c", "d"])
    z = report.LaneDupCounts()
    assert z.lane_duplication() == 0.0 and z.library_size() is None


def test_write_lane_dups_text():
    out = io.StringIO()
    report.write_lane_dups("3", _hand_counts(), verbose=True, out=out)
    size = report.library_size(19, 8)
    assert out.getvalue() == (
        "\n"
        "LaneDups: 3\tTile: 1101\tPF wells: 6\tInLane: 5\tInTile: 2\tTileRedundant: 1\tLaneRedundant: 1\n"
        "LaneDups: 3\tTile: 1102\tPF wells: 6\tInLane: 5\tInTile: 0\tTileRedundant: 0\tLaneRedundant: 4\n"
        "LaneDups: 3\tTile: 1104\tPF wells: 7\tInLane: 7\tInTile: 6\tTileRedundant: 3\tLaneRedundant: 6\n"
        "LaneDupsSummary: 3\tTiles: 3\tPF wells: 19\tClasses: 6\tInClasses: 17 (0.89474)\tRedundant: 11 (0.57895)\t"
        "CrossTileClasses: 5\tTileSpans: 13\n"
        "ClassSizes: 2: 4\t3: 0\t4: 1\t5: 1\t6: 0\t7: 0\t8: 0\t>=9: 0\n"
        "Redundant within tiles: 4 (0.36364 of Redundant)\tacross tiles: 7 (0.63636 of Redundant)\n"
        "Lane duplication (Redundant/PF wells): 57.89%\n"
        "Estimated library size (distinct/X = 1 - exp(-PF/X)): " + "%.0f" % size + "\n")
    assert 8 < size < 10
    out = io.StringIO()
    report.write_lane_dups("1", report.LaneDupCounts.from_rows([500] + [0] * 13, [[500, 0, 0, 0, 0]], ["1101"]),
                           verbose=False, out=out)
    assert out.getvalue() == (
        "\n"
        "LaneDupsSummary: 1\tTiles: 1\tPF wells: 500\tClasses: 0\tInClasses: 0 (0.00000)\tRedundant: 0 (0.00000)\t"
        "CrossTileClasses: 0\tTileSpans: 0\n"
        "ClassSizes: 2: 0\t3: 0\t4: 0\t5: 0\t6: 0\t7: 0\t8: 0\t>=9: 0\n"
        "Redundant within tiles: 0 (0.00000 of Redundant)\tacross tiles: 0 (0.00000 of Redundant)\n"
        "Lane duplication (Redundant/PF wells): 0.00%\n"
        "Estimated library size (distinct/X = 1 - exp(-PF/X)): n/a\n")
    out = io.StringIO()
    report.write_lane_dups("1", report.LaneDupCounts(), verbose=True, out=out)          # no tile, no PF well
    assert "LaneDupsSummary: 1\tTiles: 0\tPF wells: 0\t" in out.getvalue() and out.getvalue().endswith(": n/a\n")


def test_library_size_solves_its_equation():
    last = 0.0
    for n, redundant in [(19, 11), (1000, 500), (1000, 100), (1000, 1), (482_636_336, 48_000_000), (482_636_336, 1_000_000),
                         (482_636_336, 1000), (482_636_336, 1)]:
        c = n - redundant
        x = report.library_size(n, c)
        assert x > c
        assert abs(-x * math.expm1(-n / x) - c) <= 1e-9 * c, (n, redundant, x)
    for redundant in (900, 500, 100, 10, 1):                            # the fewer copies, the larger the library
        x = report.library_size(1000, 1000 - redundant)
        assert x > last
        last = x
    assert report.library_size(1000, 1000) is None and report.library_size(0, 0) is None
    assert report.library_size(1000, 999) == pytest.approx(1000 * 1000 / 2, rel=2e-3)   # n - n^2 / 2X = c


# ---- TSV ----------------------------------------------------------------------------------------
def test_lane_members_tsv(tmp_path):
    labels = np.array(HAND_LABELS, dtype=np.uint32)
    got = cwd.lane_members(labels)
    want = members_of(labels, 7)
    assert all((a == b).all() for a, b in zip(got, want))
    assert got[0].tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 3, 3, 3, 3, 3, 3, 3]
    path = str(tmp_path / "lane.tsv")
    names = ["1101", "1102", "1103", "1104"]
    cwd.write_lane_members(path, {"2": (names,) + got, "1": (names,) + tuple(a[:2] for a in got)})
    assert open(path).read().splitlines() == [
        "lane\ttile\twell\tclass_tile\tclass_well", "1\t1101\t0\t1101\t0", "1\t1101\t1\t1101\t0",
        "2\t1101\t0\t1101\t0", "2\t1101\t1\t1101\t0", "2\t1101\t2\t1101\t2", "2\t1101\t3\t1101\t3", "2\t1101\t6\t1101\t6",
        "2\t1102\t0\t1101\t2", "2\t1102\t1\t1101\t0", "2\t1102\t2\t1101\t3", "2\t1102\t3\t1101\t6", "2\t1102\t5\t1102\t5",
        "2\t1104\t0\t1101\t0", "2\t1104\t1\t1101\t0", "2\t1104\t2\t1102\t5", "2\t1104\t3\t1104\t3", "2\t1104\t4\t1101\t2",
        "2\t1104\t5\t1101\t2", "2\t1104\t6\t1104\t3"]
