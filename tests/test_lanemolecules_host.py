"""The best well of each UMI molecule without a GPU: the header against the binding, the size of the molecule region
and its error codes, the parser's refusals, the fit check, the reference on the hand-made lane of
tests/test_lanekeep_host.py with UMIs that split one family, join another and halve a third, and the report block by
molecule spelled out - with `By:` absent where the flag is."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

from lanedups_ref import lane_dups
from lanekeep_ref import check_keep_identities, lane_keep
from lanemolecules_ref import check_molecule_arrays, check_molecule_identities, lane_keep_molecules, lane_molecules
from laneumi_ref import check_umi_identities, lane_umi
from test_lanekeep_host import BLOCK as FAMILY_BLOCK
from test_lanekeep_host import CODE, EDGES, hand_made_lane
from tiledups_ref import INVALID
from well_duplicates_amd import _lib, report
from well_duplicates_amd import count_well_duplicates as cwd

HEADER = os.path.join(_lib.INCLUDE, "welldup_lanemolecules.h")


# ---- C ABI --------------------------------------------------------------------------------------
def test_lanemolecules_header_and_binding_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(wd_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.LANEMOLECULES_PROTOTYPES) == ["wd_lane_keep_molecules", "wd_lane_molecules_bytes",
                                                             "wd_lane_molecules_part", "wd_lane_umi_molecules"]
    taken = set()
    for name in dir(_lib):
        if name.endswith("PROTOTYPES") and name != "LANEMOLECULES_PROTOTYPES":
            taken |= set(getattr(_lib, name))
    assert not set(_lib.LANEMOLECULES_PROTOTYPES) & taken
    umi = open(os.path.join(_lib.CSRC, "lane_umi.inc")).read()
    keep = open(os.path.join(_lib.CSRC, "lane_keep.inc")).read()
    for kernel in ("k_lu_pairs_mol", "k_lu_group_mol"):
        assert kernel in umi and _lib.unit_of_kernel(kernel) == "tiledups"
    # one device body behind each pair of kernels, one host body behind each pair of entries; the keep kernels as they stand
    assert umi.count("template <bool kEmit>") == 2 and "lu_pairs<false>" in umi and "lu_pairs<true>" in umi
    assert "lu_group<false>" in umi and "lu_group<true>" in umi and umi.count("tn_unite(") == 1
    assert umi.count("int lu_run(") == 1 and umi.count("lu_run(ld") == 2
    assert keep.count("int lk_run(") == 1 and keep.count("lk_run(ld") == 2 and keep.count("hipLaunchKernelGGL(k_lk_score") == 1
    assert "written in a call exactly once" in umi and "asm" not in umi
    deps = {os.path.basename(f) for f in _lib._deps(os.path.join(_lib.CSRC, "welldup_tiledups.hip"))}
    assert "welldup_lanemolecules.h" in deps
    assert "lane_molecules_emu.cpp" in open(os.path.join(_lib.REPO, "tools", "wave_emu.h")).read()
    _lib.build()
    lib = _lib.load()
    for s in syms:                                                     # exported, and bound as the table says
        assert getattr(lib, s).argtypes == _lib.LANEMOLECULES_PROTOTYPES[s][1]


def _bytes(lib, tiles, wells):
    b = ctypes.c_size_t()
    return lib.wd_lane_molecules_bytes(tiles, wells, ctypes.byref(b)), b.value


def test_region_size_needs_no_gpu_and_matches_the_header():
    _lib.build()
    lib = _lib.load()
    up = lambda v: (v + 255) // 256 * 256
    for tiles, wells in ((1, 1), (3, 8193), (112, 4309253), (0, 100), (5, 0), (65535, 65535)):
        rc, got = _bytes(lib, tiles, wells)
        assert rc == _lib.OK and got == 2 * up(4 * tiles * wells), (tiles, wells)
    assert _bytes(lib, 112, 4309253)[1] - 8 * 112 * 4309253 < 512      # 8 bytes per well of the lane
    # the argument errors and the limits of wd_lane_umi_scratch
    assert _bytes(lib, -1, 10)[0] == _lib.ERR_ARG and _bytes(lib, 1, -1)[0] == _lib.ERR_ARG
    assert lib.wd_lane_molecules_bytes(1, 1, None) == _lib.ERR_ARG
    assert _bytes(lib, 65536, 1)[0] == _lib.ERR_UNSUPPORTED and _bytes(lib, 2, 1 << 31)[0] == _lib.ERR_UNSUPPORTED
    for tiles, wells in ((65535, 65537), (1, (1 << 32) - 2), (1, (1 << 32) - 1), (2, (1 << 31) - 1)):
        s = ctypes.c_size_t()
        assert _bytes(lib, tiles, wells)[0] == lib.wd_lane_umi_scratch(tiles, wells, ctypes.byref(s)), (tiles, wells)


# ---- CLI ----------------------------------------------------------------------------------------
def test_cli_flag_checks(tmp_path, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["-s", "hiseq_4000", "-r", str(tmp_path), "--all-wells"]
    on = ["--lane-dups", "--lane-dups-keep", "--lane-dups-umi", "0-9"]
    assert cwd.parse_args(base + on + ["--lane-dups-keep-umi"]).lane_dups_keep_umi
    assert not cwd.parse_args(base + on).lane_dups_keep_umi
    for extra, message in ((["--lane-dups", "--lane-dups-umi", "0-9", "--lane-dups-keep-umi"],
                            "--lane-dups-keep-umi needs --lane-dups-keep"),
                           (["--lane-dups", "--lane-dups-keep", "--lane-dups-keep-umi"], "--lane-dups-keep-umi needs --lane-dups-umi"),
                           (["--lane-dups", "--lane-dups-keep-umi"], "--lane-dups-keep-umi needs --lane-dups-keep"),
                           (["--lane-dups-keep-umi"], "--lane-dups-keep-umi needs --lane-dups-keep")):
        with pytest.raises(SystemExit):
            cwd.parse_args(base + extra)
        assert message in " ".join(capsys.readouterr().err.split()), extra


def test_cli_help_and_documents_name_the_new_option(capsys):
    with pytest.raises(SystemExit):
        cwd.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--lane-dups-keep-umi" in text and "one well per UMI molecule" in text and "is not offered: the molecules" not in text
    assert "--lane-dups-keep-umi" in cwd.__doc__
    for name in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        doc = " ".join(open(os.path.join(_lib.REPO, name)).read().split())
        assert "--lane-dups-keep-umi" in doc, name
        assert "instead of per family is not offered" not in doc, name
    design = open(os.path.join(_lib.REPO, "DESIGN.md")).read()
    assert "5.31" in design and "wd_lane_umi_molecules" in design


def test_the_molecule_region_counts_when_a_lane_is_fitted():
    cwd.check_lane_dups_fits(1000, 2000, 2, 3, 4, quality=300, umi=100, umi_scratch=100, keep=200, molecules=300)
    with pytest.raises(MemoryError) as e:
        cwd.check_lane_dups_fits(1000, 2000, 2, 3, 4, quality=300, umi=100, umi_scratch=100, keep=200, molecules=301)
    msg = str(e.value)
    assert ("2001 bytes, 300 of them for --lane-dups-quality, 200 of them for --lane-dups-umi, 200 of them for "
            "--lane-dups-keep, 301 of them for --lane-dups-keep-umi)") in msg and "2000 bytes" in msg
    with pytest.raises(MemoryError) as e:                              # without the flag the message is what it was
        cwd.check_lane_dups_fits(1000, 1400, 2, 3, 4, keep=401)
    assert str(e.value) == ("--lane-dups needs 0.00 GB of device memory for a lane of 2 tiles x 3 wells x 4 cycles "
                            "(1401 bytes, 401 of them for --lane-dups-keep), and 0.00 GB (1400 bytes) are free")


# ---- the reference on the hand-made lane ------------------------------------------------------------
# The wells of tests/test_lanekeep_host.py (tile indices 0 and 2 of three, six wells each; family A = 0, 3, 13, 16,
# B = 2, 14, C = 4, 15) with two UMI cycles.  At E = 0: A halves into {0, 3} and {13, 16}, B stays one molecule, C
# splits into two of one well.  At E = 1 A's halves stay apart (two cycles differ) and C joins (one does).
UMIS = {0: ["AA", "CA", "GG", "AA", "AC", "TT"], 2: ["TT", "CC", "GG", "AA", "CC", "NA"]}


def umi_tiles():
    byte = lambda u, c: 0 if u[c] == "N" else CODE[u[c]] | 30 << 2
    return [(ti, [np.array([byte(u, c) for u in UMIS[ti]], dtype=np.uint8) for c in range(2)]) for ti in (2, 0)]


def test_reference_on_the_hand_made_lane():
    """An anchor for tests/lanemolecules_ref.py, checked by hand: it runs the reference alone, no product code, so it
    passes with or without the feature.  What the GPU tests hold the kernels against is this reference."""
    tiles = hand_made_lane()
    fin_lane, _, labels = lane_dups(tiles, 6, 3)
    flat = labels.reshape(-1)
    assert flat[[0, 3, 13, 16]].tolist() == [0] * 4 and flat[[2, 14]].tolist() == [2, 2] and flat[[4, 15]].tolist() == [4, 4]
    mol, molmem = lane_molecules(umi_tiles(), 6, 3, labels, 0, 256)
    I = INVALID
    assert mol.reshape(-1).tolist() == [0, 1, 2, 0, 4, I, I, I, I, I, I, I, 12, 13, 2, 15, 13, 17]
    assert molmem.reshape(-1).tolist() == [1, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0]
    check_molecule_arrays(mol, molmem, labels)
    at1 = lane_molecules(umi_tiles(), 6, 3, labels, 1, 256)
    assert at1[0].reshape(-1)[[4, 15]].tolist() == [4, 4] and at1[1].reshape(-1)[4] == 1 and at1[0].reshape(-1)[13] == 13
    # max_family 3 leaves family A Large: one molecule, as the finish left it
    capped = lane_molecules(umi_tiles(), 6, 3, labels, 0, 3)
    assert capped[0].reshape(-1)[[0, 3, 13, 16]].tolist() == [0] * 4 and capped[1].reshape(-1)[0] == 3
    check_molecule_arrays(*capped, labels)
    # E >= U: the families
    whole = lane_molecules(umi_tiles(), 6, 3, labels, 2, 256)
    assert (whole[0] == labels).all()
    family = lane_keep(tiles, 6, 3, labels, EDGES, 15)
    for e, mf, arrays in ((0, 256, (mol, molmem)), (1, 256, at1), (0, 3, capped), (2, 256, whole)):
        U = lane_umi(tiles, umi_tiles(), 6, 3, labels, e, mf)
        check_umi_identities(*U, e, U=2, finish_lane=fin_lane)
        K = lane_keep_molecules(tiles, 6, 3, arrays[0], EDGES, 15)
        check_keep_identities(K[0], K[1], EDGES, 15, sum_singles=K[3])
        check_molecule_identities(U[0], K[0], fin_lane, family_keep_lane=family[0], masks=K[2], family_masks=family[2])
        if e == 2:
            assert (K[0] == family[0]).all() and all((K[2][t] == family[2][t]).all() for t in K[2])
    K = lane_keep_molecules(tiles, 6, 3, mol, EDGES, 15)
    # {0, 3}: 3 scores 80 against 0; {13, 16} and {2, 14} tie: the first well stays; 4 and 15 are alone now
    assert K[2][0].tolist() == [0, 1, 1, 1, 1, 0] and K[2][2].tolist() == [1, 1, 0, 1, 0, 1]
    assert family[2][0].tolist() == [0, 1, 1, 0, 1, 0] and family[2][2].tolist() == [1, 1, 0, 0, 0, 1]


# ---- the report -----------------------------------------------------------------------------------
def _counts(by):
    tiles = hand_made_lane()
    labels = lane_dups(tiles, 6, 3)[2]
    mol = lane_molecules(umi_tiles(), 6, 3, labels, 0, 256)[0]
    lane, trow, _, _ = lane_keep(tiles, 6, 3, mol if by == "molecule" else labels, EDGES, 15)
    return report.LaneKeepCounts.from_rows(lane, trow, ["1101", None, "1103"], 0, 15, EDGES, 4, by=by)


def _text(counts, verbose=True):
    out = io.StringIO()
    report.write_lane_keep("3", counts, verbose=verbose, out=out)
    return out.getvalue()


BLOCK = [
    "",
    # tile 1101: 400 / (4 x 4) and 0 / (1 x 4); tile 1103: 230 / 16 and 190 / 8
    "LaneKeep: 3\tTile: 1101\tPF: 5\tKept: 4\tDropped: 1 (0.20000)\tMovedIn: 1\tMeanScore kept: 25.000\tdropped: 0.000",
    "LaneKeep: 3\tTile: 1103\tPF: 6\tKept: 4\tDropped: 2 (0.33333)\tMovedIn: 0\tMeanScore kept: 14.375\tdropped: 23.750",
    "LaneKeepSummary: 3\tTiles: 2\tHamming: 0\tMinQ: 15\tCycles: 4\tWeights: 0,0,20,30\tPF: 11\tKept: 8 (0.72727)\t"
    "Dropped: 3 (0.27273)\tMolecules: 3\tMoved: 1 (0.33333 of Molecules)\tBy: molecule",
    # 630 / (8 x 4), 190 / (3 x 4), 190 / (3 x 4)
    "Mean score per base\tkept wells: 19.688\tfirst wells of molecules: 15.833\tdropped wells: 15.833",
    "MoleculesByGain: 0: 2\t1-9: 0\t10-19: 0\t20-49: 0\t50-99: 1\t100-199: 0\t200-499: 0\t500+: 0",
    "",
]


def test_write_lane_keep_by_molecule_every_line():
    assert _text(_counts("molecule")).split("\n") == BLOCK
    short = _text(_counts("molecule"), verbose=False).split("\n")
    assert short == [line for line in BLOCK if not line.startswith("LaneKeep: ")]


def test_by_is_absent_without_the_flag():
    """Without --lane-dups-keep-umi the block is byte for byte what it was; "By: family" is said only when asked for."""
    plain = _text(_counts(None))
    assert plain.split("\n") == FAMILY_BLOCK and "By:" not in plain
    said = _text(_counts("family")).split("\n")
    assert said[3] == FAMILY_BLOCK[3] + "\tBy: family" and said[:3] + said[4:] == FAMILY_BLOCK[:3] + FAMILY_BLOCK[4:]
    with pytest.raises(AssertionError):
        report.LaneKeepCounts.from_rows([0] * 17, [[0] * 6], ["1101"], 0, 15, [0], 0, by="umi")
