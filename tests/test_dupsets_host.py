"""Duplicate sets without a GPU: the report block, the CLI's flag checks, the C ABI of
include/welldup_sets.h and the host union-find the GPU tests compare against."""
import io
import os
import re

import numpy as np
import pytest

from dupsets_ref import INVALID, dup_sets, levels_of_slots
from well_duplicates_amd import _lib, report
from well_duplicates_amd import count_well_duplicates as cwd

SETS_HEADER = os.path.join(_lib.INCLUDE, "welldup_sets.h")


# ---- report -----------------------------------------------------------------------------------
def _two_tiles():
    a = report.DupSetCounts(1000, [3, 5], [7, 12], [4, 7], [2, 1, 1, 0, 0, 0, 0, 1])
    b = report.DupSetCounts(500, [1, 1], [2, 2], [1, 1], [1, 0, 0, 0, 0, 0, 0, 0])
    return {"1102": b, "1101": a}


def test_dupset_counts_decode_and_add():
    row = [1000, 3, 5, 7, 12, 4, 7, 2, 1, 1, 0, 0, 0, 0, 1]
    c = report.DupSetCounts.from_block(np.array(row), 2)
    assert c == _two_tiles()["1101"]
    s = c + _two_tiles()["1102"]
    assert (s.pf, s.sets, s.in_sets, s.redundant) == (1500, [4, 6], [9, 14], [5, 8])
    assert s.sizes == [3, 1, 1, 0, 0, 0, 0, 1]
    assert s.exact_duplication() == 8 / 1500
    assert report.DupSetCounts.zeros(3).exact_duplication() == 0.0
    with pytest.raises(ValueError):
        c + report.DupSetCounts.zeros(3)


def test_write_dup_sets_text():
    out = io.StringIO()
    report.write_dup_sets("3", _two_tiles(), verbose=True, out=out)
    assert out.getvalue() == (
        "\n"
        "DupSets: 3\tTile: 1101\tPF wells: 1000\n"
        "Level: 1\tSets: 3\tInSets: 7\tRedundant: 4\n"
        "Level: 2\tSets: 5\tInSets: 12\tRedundant: 7\n"
        "DupSets: 3\tTile: 1102\tPF wells: 500\n"
        "Level: 1\tSets: 1\tInSets: 2\tRedundant: 1\n"
        "Level: 2\tSets: 1\tInSets: 2\tRedundant: 1\n"
        "DupSetsSummary: 3\tTiles: 2\tPF wells: 1500\n"
        "Level: 1\tSets: 4\tInSets: 9 (0.00600)\tRedundant: 5 (0.00333)\n"
        "Level: 2\tSets: 6\tInSets: 14 (0.00933)\tRedundant: 8 (0.00533)\n"
        "SetSizes (level 2): 2: 3\t3: 1\t4: 1\t5: 0\t6: 0\t7: 0\t8: 0\t9+: 1\n"
        "Exact duplication (Redundant/PF wells): 0.53%\n")


def test_write_dup_sets_summary_only_and_no_pf_wells():
    out = io.StringIO()
    report.write_dup_sets("1", _two_tiles(), verbose=False, out=out)        # -S: no per-tile lines
    assert "DupSets: " not in out.getvalue()
    assert out.getvalue().startswith("\nDupSetsSummary: 1\tTiles: 2\tPF wells: 1500\n")
    out = io.StringIO()
    report.write_dup_sets("2", {"1101": report.DupSetCounts.zeros(3)}, verbose=False, out=out)
    assert out.getvalue() == (
        "\n"
        "DupSetsSummary: 2\tTiles: 1\tPF wells: 0\n"
        "Level: 1\tSets: 0\tInSets: 0 (0.00000)\tRedundant: 0 (0.00000)\n"
        "Level: 2\tSets: 0\tInSets: 0 (0.00000)\tRedundant: 0 (0.00000)\n"
        "Level: 3\tSets: 0\tInSets: 0 (0.00000)\tRedundant: 0 (0.00000)\n"
        "SetSizes (level 3): 2: 0\t3: 0\t4: 0\t5: 0\t6: 0\t7: 0\t8: 0\t9+: 0\n"
        "Exact duplication (Redundant/PF wells): 0.00%\n")


# ---- CLI ----------------------------------------------------------------------------------------
def test_cli_refuses_dup_sets_without_all_wells(tmp_path, capsys):
    base = ["-s", "hiseq_4000", "-r", str(tmp_path)]
    with pytest.raises(SystemExit):
        cwd.parse_args(base + ["-f", "targets.list", "--dup-sets"])
    assert "--dup-sets needs --all-wells" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cwd.parse_args(base + ["--all-wells", "--dup-sets-out", str(tmp_path / "sets.tsv")])
    assert "--dup-sets-out needs --dup-sets" in capsys.readouterr().err
    args = cwd.parse_args(base + ["--all-wells", "--dup-sets", "--dup-sets-out", "x.tsv"])
    assert args.dup_sets and args.dup_sets_out == "x.tsv"
    assert not cwd.parse_args(base + ["--all-wells"]).dup_sets


def test_cli_refuses_dup_sets_out_with_ranks(tmp_path, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    base = ["-s", "hiseq_4000", "-r", str(tmp_path), "--all-wells", "--dup-sets"]
    assert cwd.parse_args(base).dup_sets
    with pytest.raises(SystemExit):
        cwd.parse_args(base + ["--dup-sets-out", "x.tsv"])


def test_set_members_and_tsv(tmp_path):
    labels = np.array([0, 0, 2, INVALID, 2, 5, 0], dtype=np.uint32)
    wells, sets = cwd.set_members(labels)
    assert wells.tolist() == [0, 1, 2, 4, 6] and sets.tolist() == [0, 0, 2, 2, 0]
    path = str(tmp_path / "sets.tsv")
    cwd.write_set_members(path, {("2", "1101"): (np.array([3, 4]), np.array([3, 3])),
                                 ("1", "1102"): (wells, sets)})
    lines = open(path).read().splitlines()
    assert lines[0] == "lane\ttile\twell\tset"
    assert lines[1:] == ["1\t1102\t0\t0", "1\t1102\t1\t0", "1\t1102\t2\t2", "1\t1102\t4\t2", "1\t1102\t6\t0",
                         "2\t1101\t3\t3", "2\t1101\t4\t3"]


# ---- C ABI --------------------------------------------------------------------------------------
def test_sets_header_and_binding_agree():
    text = re.sub(r"/\*.*?\*/", "", open(SETS_HEADER).read(), flags=re.S)
    assert '#include "welldup.h"' in text
    syms = sorted(set(re.findall(r"\b(wd_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.SETS_PROTOTYPES)
    assert int(re.search(r"#define WD_DUPSET_SIZE_BINS (\d+)", text).group(1)) == _lib.DUPSET_SIZE_BINS
    assert "sets" in _lib.UNITS and _lib.unit_of_kernel("k_sets_union") == "sets"
    _lib.build()
    lib = _lib.load()
    for s in syms:
        assert getattr(lib, s) is not None
    # the workspace size needs no GPU: two uint32 per well and tile, and a little more
    import ctypes
    b = ctypes.c_size_t()
    assert lib.wd_dup_sets_workspace(1000, 3, ctypes.byref(b)) == 0
    assert 8 * 1000 * 3 < b.value < 8 * 1000 * 3 + 3 * 64 * 1024
    assert lib.wd_dup_sets_workspace(-1, 3, ctypes.byref(b)) == _lib.ERR_ARG


# ---- the host reference -------------------------------------------------------------------------
def test_reference_chain_and_triangle():
    n = 10
    pf = np.ones(n, dtype=bool)
    # chain 9-7-5-3 (single linkage: one set), triangle 0-1-2 (three edges, two merges)
    a = [9, 7, 5, 0, 1, 2]
    b = [7, 5, 3, 1, 2, 0]
    lev = [0, 1, 2, 0, 0, 0]
    row, labels = dup_sets(n, pf, a, b, lev, 3)
    assert row[0] == 10
    sets, in_sets, red, bins = row[1:4], row[4:7], row[7:10], row[10:]
    assert in_sets.tolist() == [5, 6, 7]            # {0,1,2,9,7}, + 5, + 3
    assert red.tolist() == [3, 4, 5]
    assert sets.tolist() == [2, 2, 2]
    assert bins.tolist() == [0, 1, 1, 0, 0, 0, 0, 0]  # a set of 3 and one of 4
    assert labels.tolist() == [0, 0, 0, 3, 4, 3, 6, 3, 8, 3]


def test_reference_drops_edges_to_non_pf_wells():
    pf = np.array([1, 1, 0, 1], dtype=bool)
    row, labels = dup_sets(4, pf, [0, 1, 3], [2, 2, 2], [0, 0, 0], 1)
    assert row.tolist() == [3, 0, 0, 0] + [0] * 8
    assert labels.tolist() == [0, 1, INVALID, 3]


def test_reference_pair_found_at_two_levels():
    """The same pair from both ends: level 2 from one end, level 1 from the other -> level 1."""
    row, labels = dup_sets(6, np.ones(6, bool), [4, 1], [1, 4], [1, 0], 3)
    assert row[1:4].tolist() == [1, 1, 1] and row[4:7].tolist() == [2, 2, 2] and row[7:10].tolist() == [1, 1, 1]
    assert labels.tolist() == [0, 1, 2, 3, 1, 5]


def test_reference_levels_of_slots_with_an_empty_ring():
    lvl_off = np.array([[0, 2, 2, 5], [5, 6, 8, 9]])
    assert levels_of_slots(lvl_off, [0, 0, 0, 1, 1, 1], [0, 1, 2, 5, 6, 8]).tolist() == [0, 0, 2, 0, 1, 2]


def test_reference_against_scipy_components():
    sparse = pytest.importorskip("scipy.sparse")
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    rng = np.random.default_rng(3)
    n = 400
    pf = rng.random(n) < 0.8
    a = rng.integers(0, n, 300)
    b = rng.integers(0, n, 300)
    lev = rng.integers(0, 3, 300)
    row, labels = dup_sets(n, pf, a, b, lev, 3)
    keep = pf[a] & pf[b]
    for l in range(3):
        m = keep & (lev <= l)
        g = sparse.coo_matrix((np.ones(m.sum()), (a[m], b[m])), shape=(n, n))
        _, comp = csgraph.connected_components(g, directed=False)
        sizes = np.bincount(comp[pf], minlength=comp.max() + 1)
        assert row[1 + l] == (sizes >= 2).sum()
        assert row[4 + l] == sizes[sizes >= 2].sum()
