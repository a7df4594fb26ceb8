"""A lane's duplication by insert length without a GPU: the header against the binding, the scratch formula and its
error codes, the reference against a char-by-char search, the identities on the small lane of the GPU tests, the
bit vectors the kernel matches by against allowed(p), the parser's names and refusals, the fit check, and the report
block and the TSV on the reference's counts."""
import ctypes
import io
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from laneadapter_cases import ADAPTER, INDEX, MAX_TILES, N, PARAMS, check_coverage, scripted, small_lane
from laneadapter_ref import (HIST_COLS, LANE_COLS, MAX_E, MAX_LEN, MIN_LEN, MIN_OVERLAP, NAMES, TILE_COLS, allowed,
                             check_adapter_identities, codes_of, first_match_literal, first_matches, ge_vectors,
                             lane_adapter)
from lanedups_ref import lane_dups
from lanenear_ref import lane_near_dups
from well_duplicates_amd import _lib, lane_passes, report
from well_duplicates_amd import count_well_duplicates as cwd

HEADER = os.path.join(_lib.INCLUDE, "welldup_laneadapter.h")


def _host_tiles(reads, filts, index):
    return [(index[s], [np.ascontiguousarray(r[:, c]) for c in range(r.shape[1])], f)
            for s, (r, f) in enumerate(zip(reads, filts))]


# ---- C ABI --------------------------------------------------------------------------------------
def test_laneadapter_header_and_binding_agree():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    syms = sorted(set(re.findall(r"\b(wd_[a-z0-9_]+)\s*\(", text)))
    assert syms == sorted(_lib.LANEADAPTER_PROTOTYPES) == ["wd_lane_adapter", "wd_lane_adapter_scratch"]
    define = lambda name: int(re.search(r"#define WD_LANEADAPTER_%s\s+(.+)" % name, text).group(1).strip())
    assert define("HIST_COLS") == _lib.LANEADAPTER_HIST_COLS == HIST_COLS == report.LANE_ADAPTER_HIST_COLS
    assert define("LANE_COLS") == _lib.LANEADAPTER_LANE_COLS == LANE_COLS == report.LANE_ADAPTER_LANE_COLS
    assert define("TILE_COLS") == _lib.LANEADAPTER_TILE_COLS == TILE_COLS == report.LANE_ADAPTER_TILE_COLS
    assert define("MIN_LEN") == _lib.LANEADAPTER_MIN_LEN == MIN_LEN and define("MAX_LEN") == _lib.LANEADAPTER_MAX_LEN == MAX_LEN
    assert define("MAX_E") == _lib.LANEADAPTER_MAX_E == MAX_E and define("MIN_OVERLAP") == _lib.LANEADAPTER_MIN_OVERLAP == MIN_OVERLAP
    taken = set()
    for name in dir(_lib):
        if name.endswith("PROTOTYPES") and name != "LANEADAPTER_PROTOTYPES":
            taken |= set(getattr(_lib, name))
    assert not set(_lib.LANEADAPTER_PROTOTYPES) & taken
    source = open(os.path.join(_lib.CSRC, "lane_adapter.inc")).read()
    assert "k_lad_tally" in source and _lib.unit_of_kernel("k_lad_tally") == "tiledups"
    assert "asm" not in source                                         # plain C++ and vector atomics only
    assert "lgc_piece(" in source and "lgc_piece(const" not in source  # the piece loads are lane_gc.inc's, used, not copied
    assert "static_assert(kLadStage * 4 + kLadWindow * kLadCols * 4 + kLadTileCnt * 4 <=" in source      # the LDS budget
    assert "WD_LAD_NAIVE" in source and "k_ld_pack" in source          # the code-by-code form; whose layout the rows have
    deps = {os.path.basename(f) for f in _lib._deps(os.path.join(_lib.CSRC, "welldup_tiledups.hip"))}
    assert {"lane_adapter.inc", "welldup_laneadapter.h"} <= deps
    unit = open(os.path.join(_lib.CSRC, "welldup_tiledups.hip")).read()
    assert unit.index('#include "lane_gc.inc"') < unit.index('#include "lane_adapter.inc"')
    _lib.build()
    lib = _lib.load()
    for s in syms:                                                     # exported, and bound as the table says
        assert getattr(lib, s).argtypes == _lib.LANEADAPTER_PROTOTYPES[s][1]


def _scratch(lib, tiles, cycles):
    b = ctypes.c_size_t()
    rc = lib.wd_lane_adapter_scratch(tiles, cycles, ctypes.byref(b))
    return rc, b.value


def test_scratch_size_needs_no_gpu_and_matches_the_header():
    _lib.build()
    lib = _lib.load()
    text = open(HEADER).read()
    for piece in ("5632 * max_tiles", "+ 2048 * (L + 1)", "+ 4 * max_tiles", "+ 1024", "rounded up to 256 bytes", "943 616 bytes"):
        assert piece in text, piece
    up = lambda v: (v + 255) // 256 * 256
    for tiles in (0, 1, 7, 64, 65, 112, 4096, 65535):
        for cycles in (0, 1, 10, 37, 151, 1024):
            assert _scratch(lib, tiles, cycles) == (0, 5632 * tiles + 2048 * (cycles + 1) + up(4 * tiles) + 1024)
    assert _scratch(lib, 112, 151) == (0, 943616)                      # the header's HiSeq 4000 lane
    assert _scratch(lib, 65536, 10)[0] == _lib.ERR_UNSUPPORTED and _scratch(lib, 3, 1025)[0] == _lib.ERR_UNSUPPORTED
    assert _scratch(lib, -1, 10)[0] == _lib.ERR_ARG and _scratch(lib, 3, -1)[0] == _lib.ERR_ARG
    assert lib.wd_lane_adapter_scratch(3, 10, None) == _lib.ERR_ARG
    row = (ctypes.c_int64 * 64)()                                      # a null handle is refused before anything is looked at
    assert lib.wd_lane_adapter(None, None, 13, 1, 8, None, 0, row, row, row) == _lib.ERR_ARG


# ---- the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("params", PARAMS + [(13, 3, 3), (19, 2, 8)], ids=str)
def test_reference_against_a_char_by_char_search(params):
    m, e, o = params
    L = 41
    rng = np.random.default_rng(m * 100 + e * 10 + o)
    reads = [r for r, _ in scripted(L, rng, [params])]
    random = rng.integers(0, 5, (2000, L)).astype(np.uint8)
    random[rng.random(random.shape) < 0.7] = 0                         # (mostly A: a run of A matches an adapter's A)
    reads = np.concatenate([np.array(reads, dtype=np.uint8), random, rng.integers(0, 4, (500, L)).astype(np.uint8)])
    a, mism = first_matches(reads.T, ADAPTER[:m], e, o)
    lit = [first_match_literal(r, ADAPTER[:m], e, o) for r in reads]
    assert a.tolist() == [v[0] for v in lit] and mism.tolist() == [v[1] for v in lit]
    assert set(range(L - o + 1)) <= set(a.tolist()) and (a == L).sum() > 100 and a.max() == L
    assert (mism <= e).all() and (e == 0 or (mism == e).any()) and not mism[a == L].any()
    if o < m:
        assert ((a < L) & (L - a < m)).any()


def test_the_bit_vectors_against_allowed():
    for L in (9, 10, 37, 64, 65, 151, 1024):
        for m in (8, 13, 19, 32):
            for e in range(4):
                for o in {3, 8, m}:
                    if o > L:
                        continue
                    ge = ge_vectors(L, m, e, o)
                    for p in range(L + 40):
                        ok = allowed(L, m, e, o, p) if p < L else -1
                        assert [(g >> p) & 1 for g in ge] == [int(x <= ok) for x in range(4)], (L, m, e, o, p)
                    assert ge[0] == (1 << (L - o + 1)) - 1 and all(a & b == a for b, a in zip(ge, ge[1:]))
    # allowed(p) itself: E at full overlap, floor(E o / m) below, nothing below O
    assert [allowed(20, 13, 3, 8, p) for p in (0, 7, 8, 9, 12, 13)] == [3, 3, 2, 2, 1, -1]
    assert [allowed(20, 13, 1, 3, p) for p in (7, 8, 17, 18)] == [1, 0, 0, -1]


@pytest.mark.parametrize("k", [0, 2])
def test_identities_on_the_small_lane(k):
    cycles = 37
    reads, filts = small_lane(cycles)
    tiles = _host_tiles(reads, filts, INDEX)
    if k == 0:
        fin_lane, fin_tiles, labels = lane_dups(tiles, N, MAX_TILES)
    else:
        near_lane, fin_tiles, labels = lane_near_dups(tiles, N, MAX_TILES, k)
        fin_lane = np.concatenate([near_lane[:6], near_lane[7:]])
    check_coverage(tiles, labels, k, cycles)
    want = {p: lane_adapter(tiles, N, MAX_TILES, labels, ADAPTER[:p[0]], p[1], p[2])
            for p in PARAMS + [(13, 0, 13), (13, 3, 3)]}
    for p, looser in (((13, 0, 13), (13, 1, 8)), ((13, 1, 8), (13, 3, 3)), ((13, 3, 3), None), ((8, 0, 3), None),
                      ((32, 3, 32), None)):
        check_adapter_identities(*want[p], *p, fin_lane, fin_tiles, equality=k == 0,
                                 looser=want[looser] if looser else None)
    assert want[(13, 0, 13)][0][4:7].sum() < want[(13, 1, 8)][0][4:7].sum() < want[(13, 3, 3)][0][4:7].sum()
    with pytest.raises(AssertionError):                                # the monotony check can fail: the other way round
        check_adapter_identities(*want[(13, 3, 3)], 13, 3, 3, looser=want[(13, 0, 13)])


# ---- CLI ----------------------------------------------------------------------------------------
BASE = ["-s", "hiseq_4000", "-r", "/nowhere", "--all-wells"]


def test_cli_names_and_refusals(capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert lane_passes.ADAPTER_NAMES == NAMES
    for text, name, seq in (("truseq", "truseq", "AGATCGGAAGAGC"), ("NexTera", "nextera", "CTGTCTCTTATACACATCT"),
                            ("smallrna", "smallrna", "TGGAATTCTCGG"), ("acgtacgt", "ACGTACGT", "ACGTACGT"),
                            ("A" * 32, "A" * 32, "A" * 32)):
        assert lane_passes.parse_adapter(text) == (name, codes_of(seq).tolist())
    args = cwd.parse_args(BASE + ["--lane-dups", "--lane-dups-adapter", "truseq"])
    assert args.lane_dups_adapter == "truseq" and cwd.parse_args(BASE + ["--lane-dups"]).lane_dups_adapter is None
    assert (args.lane_dups_adapter_mismatches, args.lane_dups_adapter_min_overlap, args.lane_dups_adapter_bins,
            args.lane_dups_adapter_dimer, args.lane_dups_adapter_out) == (None,) * 5
    ad = ["--lane-dups", "--lane-dups-adapter", "truseq"]
    names = "truseq (AGATCGGAAGAGC), nextera (CTGTCTCTTATACACATCT), smallrna (TGGAATTCTCGG), or 8..32 letters of ACGT"
    for extra, message in (
            (["--lane-dups-adapter", "truseq"], "--lane-dups-adapter needs --lane-dups"),
            (["--lane-dups", "--lane-dups-adapter-mismatches", "1"], "--lane-dups-adapter-mismatches needs --lane-dups-adapter"),
            (["--lane-dups", "--lane-dups-adapter-min-overlap", "8"], "--lane-dups-adapter-min-overlap needs --lane-dups-adapter"),
            (["--lane-dups", "--lane-dups-adapter-bins", "5"], "--lane-dups-adapter-bins needs --lane-dups-adapter"),
            (["--lane-dups", "--lane-dups-adapter-dimer", "5"], "--lane-dups-adapter-dimer needs --lane-dups-adapter"),
            (["--lane-dups", "--lane-dups-adapter-out", "x"], "--lane-dups-adapter-out needs --lane-dups-adapter"),
            (ad + ["--lane-dups-adapter-mismatches", "4"], "--lane-dups-adapter-mismatches takes 0..3, not 4"),
            (ad + ["--lane-dups-adapter-mismatches", "-1"], "--lane-dups-adapter-mismatches takes 0..3, not -1"),
            (ad + ["--lane-dups-adapter-min-overlap", "2"], "--lane-dups-adapter-min-overlap takes 3..the adapter's length, not 2"),
            (ad + ["--lane-dups-adapter-min-overlap", "14"], "--lane-dups-adapter-min-overlap takes 3..13, the adapter's length, not 14"),
            (ad + ["--lane-dups-adapter-bins", "1"], "--lane-dups-adapter-bins takes 2..100, not 1"),
            (ad + ["--lane-dups-adapter-bins", "101"], "--lane-dups-adapter-bins takes 2..100, not 101"),
            (ad + ["--lane-dups-adapter-dimer", "-1"], "--lane-dups-adapter-dimer takes an insert length of 0 or more, not -1"),
            (["--lane-dups", "--lane-dups-adapter", "illumina"], "--lane-dups-adapter takes " + names + ", not 'illumina'"),
            (["--lane-dups", "--lane-dups-adapter", "ACGTACG"], "--lane-dups-adapter takes " + names + ", not 'ACGTACG'"),
            (["--lane-dups", "--lane-dups-adapter", "ACGTNACGT"], "--lane-dups-adapter takes " + names),
            (["--lane-dups", "--lane-dups-adapter", "A" * 33], "--lane-dups-adapter takes " + names)):
        with pytest.raises(SystemExit):
            cwd.parse_args(BASE + extra)
        assert message in " ".join(capsys.readouterr().err.split()), message
    assert cwd.parse_args(BASE + ad + ["--lane-dups-adapter-min-overlap", "13"]).lane_dups_adapter_min_overlap == 13


def _resolve(extra, cycle_list):
    args = cwd.parse_args(BASE + ["--lane-dups"] + extra)
    run = SimpleNamespace(xy=(None, None), cycle_list=cycle_list)
    return {p.flag: params for p, params in lane_passes.resolve_passes(args, run)}


def test_defaults_and_the_refusals_of_the_run():
    truseq = codes_of(NAMES["truseq"]).tolist()
    assert _resolve([], list(range(30))) == {}
    assert _resolve(["--lane-dups-adapter", "truseq"], list(range(5, 35))) == {"--lane-dups-adapter": {
        "name": "truseq", "codes": truseq, "e": 1, "overlap": 8, "bins": 10, "dimer": 10}}
    got = _resolve(["--lane-dups-adapter", "ggaattctcg", "--lane-dups-adapter-mismatches", "0", "--lane-dups-adapter-min-overlap", "3",
                    "--lane-dups-adapter-bins", "4", "--lane-dups-adapter-dimer", "0"], list(range(30)))
    assert got == {"--lane-dups-adapter": {"name": "GGAATTCTCG", "codes": codes_of("GGAATTCTCG").tolist(), "e": 0, "overlap": 3,
                                           "bins": 4, "dimer": 0}}
    # the adapter's block comes after the GC block and before the consensus block
    both = _resolve(["--lane-dups-consensus", "--lane-dups-adapter", "nextera", "--lane-dups-gc"], list(range(30)))
    assert list(both) == ["--lane-dups-gc", "--lane-dups-adapter", "--lane-dups-consensus"]
    flags = [p.flag for p in lane_passes.ALL_PASSES]
    assert flags.index("--lane-dups-adapter") == flags.index("--lane-dups-gc") + 1 and len(set(flags)) == len(flags) == 11
    assert [p for p in lane_passes.ALL_PASSES if p.flag != "--lane-dups-adapter"] == list(lane_passes.LANE_PASSES)
    with pytest.raises(ValueError, match=r"--lane-dups-adapter takes scanned cycles that are one ascending run of consecutive "
                                         r"cycles \(a position in a read that skips cycles is not an insert length\)"):
        _resolve(["--lane-dups-adapter", "truseq"], list(range(10)) + list(range(12, 30)))
    with pytest.raises(ValueError, match="one ascending run"):
        _resolve(["--lane-dups-adapter", "truseq"], [3, 2, 1, 0, 4, 5, 6, 7, 8, 9])
    with pytest.raises(ValueError, match=r"--lane-dups-adapter-min-overlap takes 3\.\.7, the scanned cycles, not 8"):
        _resolve(["--lane-dups-adapter", "truseq"], list(range(7)))
    assert _resolve(["--lane-dups-adapter", "truseq", "--lane-dups-adapter-min-overlap", "7"], list(range(7)))


def test_cli_help_and_docstring_name_the_new_options(capsys):
    with pytest.raises(SystemExit):
        cwd.parse_args(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    for piece in ("--lane-dups-adapter NAME|SEQ", "--lane-dups-adapter-mismatches E", "--lane-dups-adapter-min-overlap O",
                  "--lane-dups-adapter-bins B", "--lane-dups-adapter-dimer D", "--lane-dups-adapter-out FILE", "truseq (AGATCGGAAGAGC)",
                  "floor(E * o / m)"):
        assert piece in text, piece
    for flag in ("--lane-dups-adapter,", "--lane-dups-adapter-mismatches", "--lane-dups-adapter-min-overlap", "--lane-dups-adapter-bins",
                 "--lane-dups-adapter-dimer", "--lane-dups-adapter-out", "report.write_lane_adapter"):
        assert flag in cwd.__doc__, flag


def test_the_adapter_scratch_counts_when_a_lane_is_fitted():
    cwd.check_lane_dups_fits(1000, 2000, 2, 3, 4, scratch=500, gc=300, adapter=200)
    with pytest.raises(MemoryError) as e:
        cwd.check_lane_dups_fits(1000, 2000, 2, 3, 4, scratch=500, gc=300, adapter=201, consensus=1)
    assert ("2002 bytes, 500 of them for --lane-dups-hamming, 300 of them for --lane-dups-gc, 201 of them for "
            "--lane-dups-adapter, 1 of them for --lane-dups-consensus)") in str(e.value)
    with pytest.raises(MemoryError) as e:                              # without the flag the message is what it was
        cwd.check_lane_dups_fits(1000, 1400, 2, 3, 4, scratch=401)
    assert str(e.value) == ("--lane-dups needs 0.00 GB of device memory for a lane of 2 tiles x 3 wells x 4 cycles "
                            "(1401 bytes, 401 of them for --lane-dups-hamming), and 0.00 GB (1400 bytes) are free")
    sc = SimpleNamespace(lane_adapter_scratch_bytes=lambda t, c: 1000 * t + c)
    run = SimpleNamespace(xy=(None, None), cycle_list=list(range(30)), n_wells=5, n_tiles=4)
    args = cwd.parse_args(BASE + ["--lane-dups", "--lane-dups-adapter", "truseq"])
    (p, params), = lane_passes.resolve_passes(args, run)
    assert p.bytes(sc, run, params) == {"adapter": 4030} and p.parts(params) == {}


# ---- the report ---------------------------------------------------------------------------------------
def _counts(bins=10, dimer=10, k=0, first_cycle=0, params=PARAMS[0]):
    cycles = 37
    reads, filts = small_lane(cycles)
    tiles = _host_tiles(reads, filts, INDEX)
    labels = lane_dups(tiles, N, MAX_TILES)[2]
    m, e, o = params
    rows = lane_adapter(tiles, N, MAX_TILES, labels, ADAPTER[:m], e, o)
    names = [None] * MAX_TILES
    for s, ti in enumerate(INDEX):
        names[ti] = "11%02d" % s
    return rows, report.LaneAdapterCounts.from_rows(*rows, names, "truseq", m, e, o, bins, dimer, k, first_cycle)


def _block(counts, verbose=True):
    out = io.StringIO()
    report.write_lane_adapter("3", counts, verbose=verbose, out=out)
    return out.getvalue()


def _fields(line):
    return dict(f.split(": ", 1) for f in line.split("\t")[1:])


@pytest.mark.parametrize("bins", [2, 7, 10, 37, 100])
def test_write_lane_adapter_totals_and_bins(bins):
    (lane, trow, hist), counts = _counts(bins=bins, dimer=4)
    text = _block(counts)
    lines = text.split("\n")
    assert lines[0] == "" and lines[-1] == "" and len(lines) == 1 + bins + 1 + 5 + 1 + 1
    rows = [_fields(ln) for ln in lines[1:bins + 2]]
    assert [r["Bin"] for r in rows] == [str(b) for b in range(bins)] + ["none"]
    # the bins partition 0 .. L - 1, in order, of equal width but for the rounding; "none" has no range
    spans = [tuple(int(v) for v in r["Insert"].split("-")) for r in rows[:-1] if r["Insert"] != "-"]
    assert [p for lo, hi in spans for p in range(lo, hi + 1)] == list(range(37)) and rows[-1]["Insert"] == "-"
    assert max(hi - lo for lo, hi in spans) - min(hi - lo for lo, hi in spans) <= 1
    assert all(r["Insert"] == "-" for r in rows[:-1]) is False and sum(r["Insert"] == "-" for r in rows[:-1]) == max(0, bins - 37)
    # the block's totals are the lane row's
    first = lambda r, key: int(r[key].split(" ")[0])
    assert sum(first(r, "Distinct") for r in rows) == lane[1] + lane[2]
    assert sum(first(r, "Reads") for r in rows) == lane[0] and sum(first(r, "Redundant") for r in rows) == lane[3]
    assert sum(first(r, "Copies") for r in rows) == lane[3]
    assert sum(first(r, "Reads") for r in rows[:-1]) == lane[4] + lane[7] and first(rows[-1], "Copies") == lane[3] - lane[6]
    tiles = [_fields(ln) for ln in lines[bins + 2:bins + 7]]
    assert [t["Tile"] for t in tiles] == ["1100", "1101", "1102", "1103", "1104"]
    assert sum(first(t, "PF") for t in tiles) == lane[0] and sum(first(t, "Adapter") for t in tiles) == lane[4:7].sum()
    assert sum(first(t, "CopiesAdapter") for t in tiles) == lane[6] and tiles[1]["MeanInsert"] == "n/a"
    s = _fields(lines[-2])
    assert lines[-2].startswith("LaneAdapterSummary: 3\tAdapter: truseq\tLength: 13\tMismatches: 1\tMinOverlap: 8\tCycles: 37\tBins: %d\t" % bins)
    with_ad, dimers = int(lane[4:7].sum()), int(hist[:5, :3].sum())
    assert s["PF"] == str(lane[0]) and s["WithAdapter"] == "%d (%.5f)" % (with_ad, with_ad / lane[0])
    assert s["Dimers (a <= 4)"] == "%d (%.5f)" % (dimers, dimers / lane[0]) and 0 < dimers < with_ad
    assert s["Inexact"] == "%d (%.5f)" % (lane[8], lane[8] / with_ad) and s["Partial"] == "%d (%.5f)" % (lane[9], lane[9] / with_ad)
    dup = lambda h: (h[:, 3].sum() - h[:, 1].sum()) / (h[:, 0].sum() + h[:, 3].sum())
    assert s["Duplication"] == "%.5f" % dup(hist) and s["Duplication of dimers"] == "%.5f" % dup(hist[:5])
    assert s["of other reads with adapter"] == "%.5f" % dup(hist[5:37]) and s["of reads without"] == "%.5f" % dup(hist[37:])
    pos = np.arange(37)
    assert s["MeanInsert distinct"] == "%.2f" % ((pos * hist[:37, :2].sum(axis=1)).sum() / hist[:37, :2].sum())
    assert s["MeanInsert redundant"] == "%.2f" % ((pos * hist[:37, 2]).sum() / hist[:37, 2].sum())
    assert _block(counts, verbose=False) == "\n".join(ln for ln in lines if not ln.startswith("LaneAdapterTile")) and "Offset" not in text


def test_write_lane_adapter_offset_hamming_and_an_empty_lane():
    _, counts = _counts(bins=5, k=2, first_cycle=20)
    text = _block(counts, verbose=False)
    assert text.count("\tHamming: 2\t") == 7 and "\tCycles: 37\tOffset: 20\tBins: 5\t" in text
    assert "\tBin: 0\tInsert: 20-27\t" in text and "\tBin: 4\tInsert: 50-56\t" in text
    _, plain = _counts(bins=5)
    shift = lambda key, t: float(_fields(t.split("\n")[-2])[key])
    assert shift("MeanInsert distinct", text) == pytest.approx(shift("MeanInsert distinct", _block(plain)) + 20, abs=0.011)
    empty = report.LaneAdapterCounts.from_rows([0] * 10, [[0] * 5], [[0] * 4] * 11, ["1101"], "ACGTACGT", 8, 0, 3)
    text = _block(empty)
    assert text.count("Distinct: 0 (0.00000)\tReads: 0\tRedundant: 0\tDuplication: 0.00000\tRelative: n/a\tMeanFamily: n/a") == 11
    assert "WithAdapter: 0 (0.00000)" in text and "MeanInsert distinct: n/a\tMeanInsert redundant: n/a" in text


def test_write_lane_adapter_tsv():
    (lane, trow, hist), counts = _counts(first_cycle=3)
    out = io.StringIO()
    report.write_lane_adapter_tsv("3", counts, out)
    lines = out.getvalue().split("\n")
    assert lines[0] == "lane\tinsert\tsingle\troots\tcopies\tfamily_wells\tcumulative" and lines[-1] == "" and len(lines) == 40
    seen = 0
    for a, line in enumerate(lines[1:-1]):
        seen += int(hist[a, :3].sum())
        want = ["3", "none" if a == 37 else str(a + 3)] + [str(v) for v in hist[a]] + ["-" if a == 37 else "%.5f" % (seen / lane[0])]
        assert line.split("\t") == want
    assert lines[37].endswith("%.5f" % (lane[4:7].sum() / lane[0]))   # the curve ends at the share of reads with adapter
    out = io.StringIO()
    report.write_lane_adapter_tsv("4", counts, out, header=False)
    assert out.getvalue().startswith("4\t3\t") and len(out.getvalue().split("\n")) == 39
