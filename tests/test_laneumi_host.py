"""The host side of --lane-dups-umi without a GPU: tests/laneumi_ref.py on hand-written families whose answer is written
out here, the identities of include/welldup_laneumi.h on it, the CLI's argument checks, the memory check's new terms
and report.write_lane_umi / write_lane_umi_tsv on a fixed row."""
import io

import numpy as np
import pytest

from laneumi_ref import (BIN_NAMES, LANE_COLS, bin_of, check_umi_identities, lane_umi, molecules_of, umi_keys)
from well_duplicates_amd import _lib
from well_duplicates_amd import count_well_duplicates as cwd
from well_duplicates_amd import report

BYTE = {"A": 0x40, "C": 0x81, "G": 0xC2, "T": 0x23, "N": 0x00}
INVALID = 0xFFFFFFFF
N, MAX_TILES = 6, 3            # tile indices 0 and 2 are added, 1 never


def _hand_made():
    """global id -> (label, UMI).  A pair with equal UMIs (0, 1); a pair with different ones (2, 3); a chain a - b - c
    with d(a, c) = 2 over two tiles (4, 5, 12); an N against a base (13, 14); a single well (17); 15 and 16 not PF."""
    wells = {0: (0, "ACGT"), 1: (0, "ACGT"), 2: (2, "ACGT"), 3: (2, "TTTT"), 4: (4, "AAAA"), 5: (4, "AAAC"),
             12: (4, "AACC"), 13: (13, "ANGT"), 14: (13, "ACGT"), 15: (INVALID, "GGGG"), 16: (INVALID, "ACGT"), 17: (17, "ACGT")}
    labels = np.full((MAX_TILES, N), INVALID, dtype=np.uint32)
    umi = {0: [["A"] * 4 for _ in range(N)], 2: [["A"] * 4 for _ in range(N)]}
    for g, (lab, u) in wells.items():
        labels[g // N, g % N] = lab
        umi[g // N][g % N] = list(u)
    umi_tiles = [(ti, [np.array([BYTE[rows[w][c]] for w in range(N)], dtype=np.uint8) for c in range(4)]) for ti, rows in umi.items()]
    tiles = [(ti, [], None) for ti in umi]
    return tiles, umi_tiles, labels


def test_hand_written_families():
    tiles, umi_tiles, labels = _hand_made()
    # E = 1: the chain is one molecule, the N differs from the base it stands for at one cycle and joins it
    lane, trow = lane_umi(tiles, umi_tiles, N, MAX_TILES, labels, 1, 256)
    assert lane.tolist() == [9, 4, 2, 4, 5, 8, 1, 2, 1, 0, 0] + [3, 1, 0, 0, 0, 0, 0, 0] + [2, 2, 1, 0, 0, 0, 0, 0]
    assert trow.tolist() == [[6, 2, 2], [0, 0, 0], [3, 2, 0]]
    check_umi_identities(lane, trow, 1, U=4)
    # E = 0: equality alone - the chain is three molecules, N is a fifth symbol
    lane0, trow0 = lane_umi(tiles, umi_tiles, N, MAX_TILES, labels, 0, 256)
    assert lane0.tolist() == [9, 1, 7, 4, 8, 8, 3, 7, 1, 0, 0] + [1, 2, 1, 0, 0, 0, 0, 0] + [7, 1, 0, 0, 0, 0, 0, 0]
    assert trow0.tolist() == [[6, 1, 4], [0, 0, 0], [3, 0, 3]]
    check_umi_identities(lane0, trow0, 0, U=4)
    check_umi_identities(lane, trow, 1, U=4, lower_e=(lane0, trow0), at_e0=(lane0, trow0))
    # max_family 2: the chain of three is Large and not looked into
    lane2, trow2 = lane_umi(tiles, umi_tiles, N, MAX_TILES, labels, 1, 2)
    assert lane2.tolist() == [6, 2, 2, 3, 4, 5, 1, 2, 1, 1, 3] + [2, 1, 0, 0, 0, 0, 0, 0] + [2, 2, 0, 0, 0, 0, 0, 0]
    assert trow2.tolist() == [[4, 1, 2], [0, 0, 0], [2, 1, 0]]
    check_umi_identities(lane2, trow2, 1, U=4)
    # E >= U: every family is one molecule
    lane3, trow3 = lane_umi(tiles, [(ti, p[:3]) for ti, p in umi_tiles], N, MAX_TILES, labels, 3, 256)
    assert lane3[4] == lane3[3] == 4 and lane3[2] == 0
    check_umi_identities(lane3, trow3, 3, U=3)
    # the keys as the library packs them: ten 3-bit codes a word, N = 4
    keys = umi_keys(umi_tiles, N, MAX_TILES)
    assert keys[13] == 0 | 4 << 3 | 2 << 6 | 3 << 9 and keys[3] == 3 | 3 << 3 | 3 << 6 | 3 << 9 and keys[6] == 0


def test_molecules_do_not_depend_on_the_order_and_bins():
    rng = np.random.default_rng(5)
    chain = np.zeros((40, 12), dtype=np.uint8)
    for i in range(1, 40):
        chain[i] = chain[i - 1]
        chain[i, i % 12] = (chain[i, i % 12] + 1) % 4
    for e in range(4):
        want = sorted(len(m) for m in molecules_of(chain, e))
        for _ in range(3):
            perm = rng.permutation(40)
            assert sorted(len(m) for m in molecules_of(chain[perm], e)) == want
    assert len(molecules_of(chain, 1)) == 1 and len(molecules_of(chain, 0)) == 40
    assert [bin_of(v) for v in (1, 2, 3, 4, 5, 8, 9, 16, 17, 64, 65, 1024)] == [0, 1, 2, 3, 4, 4, 5, 5, 6, 6, 7, 7]
    assert len(BIN_NAMES) == _lib.LANEUMI_BINS and LANE_COLS == _lib.LANEUMI_LANE_COLS == report.LANE_UMI_LANE_COLS
    assert BIN_NAMES == _lib.LANEUMI_BIN_NAMES == report.LANE_UMI_BIN_NAMES


def test_the_header_and_the_binding_agree():
    import os
    import re
    text = open(os.path.join(_lib.INCLUDE, "welldup_laneumi.h")).read()
    consts = dict(re.findall(r"#define (WD_LANEUMI_[A-Z_]+) (\d+)", text))
    assert {k: int(v) for k, v in consts.items()} == {
        "WD_LANEUMI_MAX_CYCLES": _lib.LANEUMI_MAX_CYCLES, "WD_LANEUMI_MAX_E": _lib.LANEUMI_MAX_E,
        "WD_LANEUMI_MAX_FAMILY": _lib.LANEUMI_MAX_FAMILY, "WD_LANEUMI_LANE_COLS": _lib.LANEUMI_LANE_COLS,
        "WD_LANEUMI_TILE_COLS": _lib.LANEUMI_TILE_COLS, "WD_LANEUMI_BINS": _lib.LANEUMI_BINS}
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(wd_lane_umi[a-z_]*)\s*\(", code))) == sorted(_lib.LANEUMI_PROTOTYPES)


# ---- CLI ----------------------------------------------------------------------------------------
def test_cli_flag_checks(tmp_path, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    base = ["-s", "hiseq_4000", "-r", str(tmp_path), "--all-wells"]
    args = cwd.parse_args(base + ["--lane-dups", "--lane-dups-umi", "0-9"])
    assert args.lane_dups_umi == "0-9"
    assert (args.lane_dups_umi_mismatches, args.lane_dups_umi_max_family, args.lane_dups_umi_out) == (None,) * 3
    assert cwd.parse_args(base + ["--lane-dups"]).lane_dups_umi is None
    args = cwd.parse_args(base + ["--lane-dups", "--lane-dups-hamming", "2", "--lane-dups-index", "151-159", "--lane-dups-umi",
                                  "0-8,159-171", "--lane-dups-umi-mismatches", "3", "--lane-dups-umi-max-family", "1024",
                                  "--lane-dups-umi-out", "u.tsv"])
    assert (args.lane_dups_umi_mismatches, args.lane_dups_umi_max_family, args.lane_dups_umi_out) == (3, 1024, "u.tsv")
    args = cwd.parse_args(base + ["--lane-dups", "--lane-dups-umi", "3-4", "--lane-dups-umi-mismatches", "0",
                                  "--lane-dups-umi-max-family", "2"])
    assert (args.lane_dups_umi_mismatches, args.lane_dups_umi_max_family) == (0, 2)
    on = ["--lane-dups", "--lane-dups-umi", "0-9"]
    for extra, message in ((["--lane-dups-umi", "0-9"], "--lane-dups-umi needs --lane-dups"),
                           (["--tile-dups", "--lane-dups-umi", "0-9"], "--lane-dups-umi needs --lane-dups"),
                           (["--lane-dups", "--lane-dups-umi-mismatches", "1"], "--lane-dups-umi-mismatches needs --lane-dups-umi"),
                           (["--lane-dups", "--lane-dups-umi-max-family", "10"], "--lane-dups-umi-max-family needs --lane-dups-umi"),
                           (["--lane-dups", "--lane-dups-umi-out", "x.tsv"], "--lane-dups-umi-out needs --lane-dups-umi"),
                           (["--lane-dups", "--lane-dups-umi", "0-21"], "--lane-dups-umi takes 1..20 cycles, not 21"),
                           (["--lane-dups", "--lane-dups-umi", "0-10,20-31"], "--lane-dups-umi takes 1..20 cycles, not 21"),
                           (["--lane-dups", "--lane-dups-umi", "5-5"], "--lane-dups-umi takes ranges of cycles"),
                           (["--lane-dups", "--lane-dups-umi", "nine"], "--lane-dups-umi takes ranges of cycles"),
                           (on + ["--lane-dups-umi-mismatches", "4"], "--lane-dups-umi-mismatches takes 0..3, not 4"),
                           (on + ["--lane-dups-umi-mismatches", "-1"], "--lane-dups-umi-mismatches takes 0..3, not -1"),
                           (on + ["--lane-dups-umi-max-family", "1"], "--lane-dups-umi-max-family takes 2..1024, not 1"),
                           (on + ["--lane-dups-umi-max-family", "1025"], "--lane-dups-umi-max-family takes 2..1024, not 1025")):
        with pytest.raises(SystemExit):
            cwd.parse_args(base + extra)
        assert message in " ".join(capsys.readouterr().err.split()), extra
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        cwd.parse_args(base + on)
    assert "--lane-dups runs in a single process only" in " ".join(capsys.readouterr().err.split())


def test_cli_help_and_docstring_name_the_new_options(capsys):
    with pytest.raises(SystemExit):
        cwd.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for piece in ("--lane-dups-umi RANGES", "--lane-dups-umi-mismatches E", "--lane-dups-umi-max-family M",
                  "--lane-dups-umi-out FILE", "2..1024, default 256", "0..3, default 1", "16 bytes of device memory per well"):
        assert piece in text, piece
    for flag in ("--lane-dups-umi,", "--lane-dups-umi-mismatches", "--lane-dups-umi-max-family", "--lane-dups-umi-out",
                 "report.write_lane_umi"):
        assert flag in cwd.__doc__, flag


def test_the_umi_terms_count_when_a_lane_is_fitted():
    cwd.check_lane_dups_fits(1000, 2000, 2, 3, 4, scratch=500, umi=200, umi_scratch=300)
    with pytest.raises(MemoryError) as e:
        cwd.check_lane_dups_fits(1000, 2000, 2, 3, 4, scratch=500, consensus=100, umi=200, umi_scratch=201)
    assert ("(2001 bytes, 500 of them for --lane-dups-hamming, 100 of them for --lane-dups-consensus, 401 of them for "
            "--lane-dups-umi), and 0.00 GB (2000 bytes) are free") in str(e.value)
    with pytest.raises(MemoryError) as e:
        cwd.check_lane_dups_fits(1000, 1400, 2, 3, 4, scratch=401)
    assert "(1401 bytes, 401 of them for --lane-dups-hamming)" in str(e.value)


# ---- the report ---------------------------------------------------------------------------------
LANE_ROW = [900, 300, 350, 400, 600, 640, 150, 380, 12, 2, 700] + [250, 120, 20, 6, 4, 0, 0, 0] + [350, 220, 20, 0, 10, 0, 0, 0]
TILE_ROWS = [[500, 170, 200], [0, 0, 0], [400, 130, 150]]

BLOCK = """
LaneUmi: 3\tTile: 1101\tWells: 500\tUmiRedundant: 170\tLone: 200
LaneUmi: 3\tTile: 1103\tWells: 400\tUmiRedundant: 130\tLone: 150
LaneUmiSummary: 3\tTiles: 2\tHamming: 1\tUmiCycles: 9\tMismatches: 1\tMaxFamily: 256\tFamilies: 400\tWells: 900 (0.09000 of PF)\t\
Molecules: 600\tDistinctUmis: 640\tUmiRedundant: 300\tLone: 350\tSplitFamilies: 150 (0.37500 of Families)\tSplitWells: 380\t\
WithN: 12\tLarge left out: 2 (700 wells)
Lane duplication (Redundant/PF wells): 11.98%\twith the UMI: 9.98% (998 redundant wells, 1198 before)
Estimated library size (distinct/X = 1 - exp(-PF/X)): 38332\twith the UMI: 46708
Copies that are molecules of their own: 200 of 500 (0.40000)
UMI reads merged as read errors: 40 (4.938e-03 per UMI base)
MoleculesPerFamily: 1: 250\t2: 120\t3: 20\t4: 6\t5-8: 4\t9-16: 0\t17-64: 0\t65+: 0
MoleculeSizes: 1: 350\t2: 220\t3: 20\t4: 0\t5-8: 10\t9-16: 0\t17-64: 0\t65+: 0
"""


def _counts():
    # (the finish: 10 000 PF wells; 402 groups of two or more with 900 + 700 wells: 1198 redundant)
    return report.LaneUmiCounts.from_rows(LANE_ROW, TILE_ROWS, ["1101", None, "1103"], 1, 1, 256, 9, 10000, 1198)


def test_write_lane_umi_on_a_fixed_row():
    c = _counts()
    check_umi_identities(np.array(LANE_ROW), np.array(TILE_ROWS), 1, U=9, finish_lane=[10000, 402, 1600, 1198])
    assert c.to_rows() == (LANE_ROW, [TILE_ROWS[0], TILE_ROWS[2]])
    assert c.redundant_with_umi == 300 + 700 - 2 and c.own_molecules == 200
    assert c.merged_rate() == pytest.approx(40 / 8100)
    for verbose in (True, False):
        text = io.StringIO()
        report.write_lane_umi("3", c, verbose=verbose, out=text)
        want = BLOCK if verbose else "\n" + "".join(line + "\n" for line in BLOCK.strip("\n").split("\n") if "\tTile: " not in line)
        assert text.getvalue() == want
    # the library sizes are the estimator's, of the lane's reads and the distinct ones either way
    assert "%.0f" % report.library_size(10000, 10000 - 1198) == "38332"
    assert "%.0f" % report.library_size(10000, 10000 - 998) == "46708"
    empty = io.StringIO()
    report.write_lane_umi("1", report.LaneUmiCounts(umi_cycles=8), out=empty)
    assert "n/a per UMI base" in empty.getvalue() and "with the UMI: n/a" in empty.getvalue()


def test_the_tsv_parses_back_to_the_rows():
    c = _counts()
    text = io.StringIO()
    report.write_lane_umi_tsv("3", c, text)
    report.write_lane_umi_tsv("4", c, text, header=False)
    lines = text.getvalue().strip("\n").split("\n")
    assert lines[0] == "lane\ttable\tkey\twells\tumi_redundant\tlone" and len(lines) == 1 + 2 * (8 + 8 + 2)
    rows = [ln.split("\t") for ln in lines[1:]]
    for lane in ("3", "4"):
        mine = [r for r in rows if r[0] == lane]
        assert [int(r[3]) for r in mine if r[1] == "per_family"] == LANE_ROW[11:19]
        assert [int(r[3]) for r in mine if r[1] == "size"] == LANE_ROW[19:]
        assert [r[2] for r in mine if r[1] == "size"] == list(BIN_NAMES)
        assert {r[2]: [int(v) for v in r[3:]] for r in mine if r[1] == "tile"} == {"1101": TILE_ROWS[0], "1103": TILE_ROWS[2]}
