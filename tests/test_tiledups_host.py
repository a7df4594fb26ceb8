"""Read classes per tile without a GPU: the report block, the CLI's flag checks, the C ABI of
include/welldup_tiledups.h and the host reference the GPU tests compare against."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from tiledups_ref import INVALID, class_labels, codes_of, tile_dups
from well_duplicates_amd import _lib, report
from well_duplicates_amd import count_well_duplicates as cwd

HEADER = os.path.join(_lib.INCLUDE, "welldup_tiledups.h")


# ---- report -----------------------------------------------------------------------------------
def _two_tiles():
    # rows as wd_tile_dups writes them, two levels; tiles of 2001 wells
    a = report.TileDupCounts.from_block([1000, 20, 45, 25, 10, 30, 270, 810, 17, 2, 0, 0, 0, 0, 0, 1], 2, wells=2001)
    b = report.TileDupCounts.from_block([500, 1, 2, 1, 2, 2, 12, 36, 1, 0, 0, 0, 0, 0, 0, 0], 2, wells=2001)
    return {"1102": b, "1101": a}


def test_tiledup_counts_decode_and_add():
    row = [1000, 20, 45, 25, 10, 30, 270, 810, 17, 2, 0, 0, 0, 0, 0, 1]
    c = report.TileDupCounts.from_block(np.array(row), 2, wells=2001)
    assert (c.pf, c.classes, c.in_classes, c.redundant) == (1000, 20, 45, 25)
    assert c.local == [10, 30] and c.ring_wells == [270, 810] and c.sizes == [17, 2, 0, 0, 0, 0, 0, 1]
    assert c.even_den == 45 * 2000 and c.to_block() == row
    assert report.TileDupCounts.from_block(row, 2).even_den == 0
    s = c + _two_tiles()["1102"]
    assert (s.pf, s.classes, s.in_classes, s.redundant) == (1500, 21, 47, 26)
    assert s.local == [12, 32] and s.ring_wells == [282, 846] and s.sizes == [18, 2, 0, 0, 0, 0, 0, 1]
    assert s.even_den == 47 * 2000
    assert s.tile_duplication() == 26 / 1500 and s.local_share() == 32 / 47
    z = report.TileDupCounts.zeros(3)
    assert z.levels == 3 and z.tile_duplication() == 0.0 and z.local_share() == 0.0
    with pytest.raises(ValueError):
        c + z
    with pytest.raises(AssertionError):
        report.TileDupCounts.from_block(row, 3)


def test_write_tile_dups_text():
    out = io.StringIO()
    report.write_tile_dups("3", _two_tiles(), verbose=True, out=out)
    assert out.getvalue() == (
        "\n"
        "TileDups: 3\tTile: 1101\tPF wells: 1000\tClasses: 20\tInClasses: 45\tRedundant: 25\n"
        "Level: 1\tLocal: 10\tRingWells: 270\n"
        "Level: 2\tLocal: 30\tRingWells: 810\n"
        "TileDups: 3\tTile: 1102\tPF wells: 500\tClasses: 1\tInClasses: 2\tRedundant: 1\n"
        "Level: 1\tLocal: 2\tRingWells: 12\n"
        "Level: 2\tLocal: 2\tRingWells: 36\n"
        "TileDupsSummary: 3\tTiles: 2\tPF wells: 1500\tClasses: 21\tInClasses: 47 (0.03133)\tRedundant: 26 (0.01733)\n"
        "Level: 1\tLocal: 12 (0.25532 of InClasses)\tEvenly spread: 0.00300\n"
        "Level: 2\tLocal: 32 (0.68085 of InClasses)\tEvenly spread: 0.00900\n"
        "ClassSizes: 2: 18\t3: 2\t4: 0\t5: 0\t6: 0\t7: 0\t8: 0\t>=9: 1\n"
        "Tile duplication (Redundant/PF wells): 1.73%\n"
        "Local share at level 2 (Local/InClasses): 68.09%\n")


def test_write_tile_dups_summary_only_no_pf_wells_no_classes():
    out = io.StringIO()
    report.write_tile_dups("1", _two_tiles(), verbose=False, out=out)       # -S: no per-tile lines
    assert "TileDups: " not in out.getvalue()
    assert out.getvalue().startswith("\nTileDupsSummary: 1\tTiles: 2\tPF wells: 1500\tClasses: 21\t")
    out = io.StringIO()
    report.write_tile_dups("2", {"1101": report.TileDupCounts.zeros(3)}, verbose=False, out=out)
    assert out.getvalue() == (
        "\n"
        "TileDupsSummary: 2\tTiles: 1\tPF wells: 0\tClasses: 0\tInClasses: 0 (0.00000)\tRedundant: 0 (0.00000)\n"
        "Level: 1\tLocal: 0 (0.00000 of InClasses)\tEvenly spread: 0.00000\n"
        "Level: 2\tLocal: 0 (0.00000 of InClasses)\tEvenly spread: 0.00000\n"
        "Level: 3\tLocal: 0 (0.00000 of InClasses)\tEvenly spread: 0.00000\n"
        "ClassSizes: 2: 0\t3: 0\t4: 0\t5: 0\t6: 0\t7: 0\t8: 0\t>=9: 0\n"
        "Tile duplication (Redundant/PF wells): 0.00%\n"
        "Local share at level 3 (Local/InClasses): 0.00%\n")
    # PF wells but no class: still no division by zero
    out = io.StringIO()
    no_class = report.TileDupCounts.from_block([800] + [0] * (3 + 2 + 8), 1, wells=1000)
    report.write_tile_dups("2", {"1101": no_class}, verbose=True, out=out)
    assert out.getvalue() == (
        "\n"
        "TileDups: 2\tTile: 1101\tPF wells: 800\tClasses: 0\tInClasses: 0\tRedundant: 0\n"
        "Level: 1\tLocal: 0\tRingWells: 0\n"
        "TileDupsSummary: 2\tTiles: 1\tPF wells: 800\tClasses: 0\tInClasses: 0 (0.00000)\tRedundant: 0 (0.00000)\n"
        "Level: 1\tLocal: 0 (0.00000 of InClasses)\tEvenly spread: 0.00000\n"
        "ClassSizes: 2: 0\t3: 0\t4: 0\t5: 0\t6: 0\t7: 0\t8: 0\t>=9: 0\n"
        "Tile duplication (Redundant/PF wells): 0.00%\n"
        "Local share at level 1 (Local/InClasses): 0.00%\n")


# ---- CLI ----------------------------------------------------------------------------------------
def test_cli_refuses_tile_dups_without_all_wells(tmp_path, capsys):
    base = ["-s", "hiseq_4000", "-r", str(tmp_path)]
    with pytest.raises(SystemExit):
        cwd.parse_args(base + ["-f", "targets.list", "--tile-dups"])
    assert "--tile-dups needs --all-wells" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cwd.parse_args(base + ["--all-wells", "--tile-dups-out", str(tmp_path / "classes.tsv")])
    assert "--tile-dups-out needs --tile-dups" in capsys.readouterr().err
    args = cwd.parse_args(base + ["--all-wells", "--tile-dups", "--tile-dups-out", "x.tsv"])
    assert args.tile_dups and args.tile_dups_out == "x.tsv" and not args.dup_sets
    args = cwd.parse_args(base + ["--all-wells"])
    assert not args.tile_dups and args.tile_dups_out is None


def test_cli_refuses_tile_dups_out_with_ranks(tmp_path, monkeypatch, capsys):
    monkeypatch.setenv("WORLD_SIZE", "2")
    base = ["-s", "hiseq_4000", "-r", str(tmp_path), "--all-wells", "--tile-dups"]
    assert cwd.parse_args(base).tile_dups
    with pytest.raises(SystemExit):
        cwd.parse_args(base + ["--tile-dups-out", "x.tsv"])
    assert "--tile-dups-out is written by a single process only" in capsys.readouterr().err


def test_cli_help_says_classes_are_by_equality(capsys):
    with pytest.raises(SystemExit):
        cwd.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--tile-dups" in text and "always by equality" in text and "near-duplicate classes" in text


def test_class_members_tsv(tmp_path):
    labels = np.array([0, 1, 2, 2, INVALID, 0], dtype=np.uint32)
    wells, classes = cwd.set_members(labels)
    path = str(tmp_path / "classes.tsv")
    cwd.write_set_members(path, {("1", "1101"): (wells, classes)}, column="class")
    assert open(path).read().splitlines() == ["lane\ttile\twell\tclass", "1\t1101\t0\t0", "1\t1101\t2\t2",
                                              "1\t1101\t3\t2", "1\t1101\t5\t0"]


# ---- C ABI --------------------------------------------------------------------------------------
def test_tiledups_header_and_binding_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert '#include "welldup_sets.h"' in text                   # (WD_DUPSET_SIZE_BINS)
    syms = sorted(set(re.findall(r"\b(wd_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.TILEDUPS_PROTOTYPES) == ["wd_tile_dups", "wd_tile_dups_workspace"]
    assert not set(syms) & (set(_lib.PROTOTYPES) | set(_lib.SETS_PROTOTYPES))
    assert _lib.UNITS[-1] == "tiledups"
    assert _lib.unit_of_kernel("k_td_insert") == "tiledups" and _lib.unit_of_kernel("k_td_fingerprint<true>") == "tiledups"
    assert _lib.unit_of_kernel("k_sets_union") == "sets"
    _lib.build()
    lib = _lib.load()
    for s in syms:
        assert getattr(lib, s) is not None


def test_build_id_names_the_tiledups_unit():
    _lib.build()
    ids = _lib.build_ids()
    units = _lib.source_unit_ids()
    assert list(units) == list(_lib.UNITS)
    assert ids["tiledups"] == units["tiledups"] != "unknown"
    assert ids["all"] == _lib.source_build_id()
    # only core and the new unit see the new unit's private header
    deps = {u: {os.path.basename(f) for f in _lib._deps(os.path.join(_lib.CSRC, "welldup_%s.hip" % u))} for u in _lib.UNITS}
    assert [u for u in _lib.UNITS if "wd_tiledups.h" in deps[u]] == ["core", "tiledups"]
    assert [u for u in _lib.UNITS if "welldup_tiledups.h" in deps[u]] == ["tiledups"]


def test_workspace_size_needs_no_gpu():
    _lib.build()
    lib = _lib.load()
    b = ctypes.c_size_t()
    assert lib.wd_tile_dups_workspace(1000, 3, ctypes.byref(b)) == 0
    # per tile: 2048 slots of 8 bytes, 20 bytes per well; counters and pointer tables on top
    floor = 3 * (2048 * 8 + 20 * 1000)
    assert floor < b.value < floor + 3 * 64 * 1024 + 64 * 1024
    big = ctypes.c_size_t()
    assert lib.wd_tile_dups_workspace(4309253, 1, ctypes.byref(big)) == 0
    assert big.value > (1 << 24) * 8 + 20 * 4309253                 # 2 N = 8.6 M -> 2^24 slots
    assert lib.wd_tile_dups_workspace(-1, 3, ctypes.byref(b)) == _lib.ERR_ARG
    assert lib.wd_tile_dups_workspace(10, 1, None) == _lib.ERR_ARG


# ---- the host reference -------------------------------------------------------------------------
A, C, G, T = 0x40, 0x81, 0xC2, 0x23          # quality bits on top of the base's two low bits


def _grid_rings(rows, cols):
    """Level 1: the wells left, right, above and below; level 2: the diagonal ones."""
    lvl_off, nbr = [], []
    for r in range(rows):
        for c in range(cols):
            row = [len(nbr)]
            for ring in ([(0, -1), (0, 1), (-1, 0), (1, 0)], [(-1, -1), (-1, 1), (1, -1), (1, 1)]):
                for dr, dc in ring:
                    if 0 <= r + dr < rows and 0 <= c + dc < cols:
                        nbr.append((r + dr) * cols + c + dc)
                row.append(len(nbr))
            lvl_off.append(row)
    return lvl_off, nbr


def test_reference_on_a_hand_made_tile():
    """3 x 4 wells, three cycles:
         0  1  2  3        X = {0, 5, 11} read ACG (0 and 5 diagonal: level 2; 11 far from both)
         4  5  6  7        Y = {2, 3}     read NNT (side by side: level 1)
         8  9 10 11        Z = {1, 8}     read TTT (far apart, but 1 is put into ring 1 of 8: one-sided)
    well 6 reads AAT (a non-zero byte with low bits 0 is A, not N: not Y), well 7 reads ACG but its filter byte
    is 2, well 9 fails the filter, wells 4 and 10 are alone."""
    reads = {0: (A, C, G), 5: (A | 0x3C, C, G | 0x10), 11: (A, C | 0x04, G),
             2: (0, 0, T), 3: (0, 0, T | 0x80), 6: (0x04, 0x08, T),
             1: (T, T, T), 8: (T | 0x40, T, T), 7: (A, C, G), 9: (A, C, G),
             4: (G, G, G), 10: (C, 0, C)}
    planes = [np.array([reads[w][c] for w in range(12)], dtype=np.uint8) for c in range(3)]
    filt = np.array([1, 1, 1, 3, 1, 1, 1, 2, 0x81, 0, 1, 1], dtype=np.uint8)
    lvl_off, nbr = _grid_rings(3, 4)
    # well 8 = (2, 0): put well 1 into its ring 1 (nothing puts 8 into a ring of 1)
    at = lvl_off[8][1]
    nbr.insert(at, 1)
    lvl_off[8][1] += 1
    lvl_off[8][2] += 1
    for w in range(9, 12):
        lvl_off[w] = [v + 1 for v in lvl_off[w]]
    assert codes_of(planes, 12)[:, 2].tolist() == [4, 4, 3] and codes_of(planes, 12)[:, 6].tolist() == [0, 0, 3]
    row, labels = tile_dups(planes, filt, np.array(lvl_off), np.array(nbr))
    assert labels.tolist() == [0, 1, 2, 2, 4, 0, 6, INVALID, 1, INVALID, 10, 0]
    assert row[:4].tolist() == [10, 3, 7, 4]                       # PF, Classes, InClasses, Redundant
    assert row[4:6].tolist() == [4, 6]                             # Local: 2, 3, 1, 8 at level 1; 0, 5 join at level 2
    # rings of the wells in classes (0, 1, 2, 3, 5, 8, 11): 2+3+3+2+4+3+2 side wells, 1+2+2+1+4+1+1 diagonal
    assert row[6:8].tolist() == [19, 31]
    assert row[8:].tolist() == [2, 1, 0, 0, 0, 0, 0, 0]


def test_reference_confirms_groups_on_the_rows():
    """class_labels never trusts its hash: rows that differ in one cycle are told apart, a class of ten
    lands in the last bin."""
    rng = np.random.default_rng(5)
    n, L = 300, 25
    planes = [rng.integers(1, 256, n).astype(np.uint8) for _ in range(L)]
    big = rng.choice(n, 10, replace=False)
    for p in planes:
        p[big] = p[big[0]]
    near = [w for w in range(n) if w not in big][:2]
    for c, p in enumerate(planes):
        p[near[1]] = p[near[0]] ^ (1 if c == 7 else 0)              # differs in cycle 7 only
    pf = np.ones(n, dtype=bool)
    labels = class_labels(codes_of(planes, n), pf)
    assert (labels[big] == big.min()).all() and (labels == big.min()).sum() == 10
    assert labels[near[0]] == near[0] and labels[near[1]] == near[1]
    lvl_off = np.zeros((n, 2), dtype=np.int64)                      # no rings at all
    row, _ = tile_dups(planes, pf.astype(np.uint8), lvl_off, np.zeros(0, dtype=np.int64))
    assert row[:4].tolist() == [n, 1, 10, 9] and row[4:6].tolist() == [0, 0]
    assert row[6:].tolist() == [0] * 7 + [1]
