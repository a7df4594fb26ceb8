"""k_lad_tally's source (csrc/lane_adapter.inc) run on the CPU under shuffled schedules: tools/lane_adapter_emu.cpp
compiles the kernel as it stands, twice - the bit-parallel search and the code-by-code one of -DWD_LAD_NAIVE -, plays
the 256 lanes of a workgroup with fibers (tools/wave_emu.h) and holds both forms to the definitions of
include/welldup_laneadapter.h computed directly, char by char: the search alone on scripted rows for every L, m, E and
O of its list, the host's table against allowed(p), and the kernel - the staging of the rows in LDS with its sub-trips,
the search, the wave-grouped histogram, its overflow into memory beyond the LDS window and its flush - under the eleven
schedules.  The program is built with the address and undefined-behaviour sanitizers, and its rows, its table and its
staging block are heap blocks of exactly their size.  Two builds broken on purpose must fail: a shift that does not
carry across the 64-bit position words ends in MISMATCH, a staging block one row short in a sanitizer report.  No GPU
is involved (the GPU tests compare the kernel itself with tests/laneadapter_ref.py: tests/test_gpu_laneadapter.py)."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
         "-I" + os.path.join(REPO, "include")]
SRC = os.path.join(REPO, "tools", "lane_adapter_emu.cpp")
NAMES = ("case", "N", "L", "words", "mis", "m", "E", "O", "mode", "schedules", "families", "with", "inexact", "partial",
         "beyond", "distinct", "sub", "points")
LINE = re.compile(r"case (\d+) ok: N (\d+) L (\d+) words (\d+) mis (\d+) m (\d+) E (\d+) O (\d+) mode (\d+) "
                  r"schedules (\d+) families (\d+) with (\d+) inexact (\d+) partial (\d+) beyond (\d+) distinct (\d+) "
                  r"sub (\d+) points (\d+)")
LS, MS = (9, 10, 37, 63, 64, 65, 83, 151, 1024), (8, 13, 19, 32)


def _build(tmp_path, name, *defines):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++"] + FLAGS + list(defines) + [SRC, "-o", exe])
    return exe


def test_both_forms_give_the_definitions_result_under_every_schedule(tmp_path):
    out = subprocess.run([_build(tmp_path, "lane_adapter_emu")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "MISMATCH" not in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
    lines = out.stdout.strip().split("\n")
    # the search alone: every L with every m, E and O (O = 8 = m once; O <= L), thousands of scripted rows
    combos, rows = (int(v) for v in re.fullmatch(r"search ok: combos (\d+) rows (\d+)", lines[0]).groups())
    assert combos == sum(1 for L in LS for m in MS for e in range(4) for o in {3, 8, m} if o <= L) and rows > 100000
    cases = [dict(zip(NAMES, (int(v) for v in row))) for row in LINE.findall(out.stdout)]
    assert len(cases) == len(lines) - 1 == 18
    assert all(c["schedules"] == 11 and c["points"] > 0 for c in cases)
    scripted = [c for c in cases if c["mode"] == 0]
    # the ground: every L, m and E, the three kinds of O, rows whose base lies 0 to 3 words past a 16-byte boundary,
    # tiles whose wells are 1, 2 and 3 past a multiple of four and of a run and a bit, the three kinds of lane
    assert {c["L"] for c in scripted} == set(LS) and {c["L"] for c in cases if c["mode"]} >= {63, 151, 1024}
    assert {c["m"] for c in scripted} == set(MS) and {c["E"] for c in scripted} == {0, 1, 2, 3}
    assert {3, 8} <= {c["O"] for c in scripted} and any(c["O"] == c["m"] > 8 for c in scripted)
    assert {c["mis"] for c in cases} == {0, 1, 2, 3} and {c["mode"] for c in cases} == {0, 1, 2}
    assert {c["N"] % 4 for c in cases} >= {1, 2, 3} and max(c["N"] for c in cases) > 8192
    # rows of more than 16 words go through sub-trips of fewer wells than a trip; a beyond the LDS window goes to memory
    assert all((c["sub"] < 256) == (c["words"] > 16) for c in cases) and any(c["words"] == 103 for c in cases)
    assert all((c["beyond"] > 0) == (c["L"] == 1024) for c in cases)
    # the scripted reads hit every a in 0 .. L - O (and "no adapter"); with E = 0 nothing is inexact, with O = m
    # nothing partial, and elsewhere both occur
    assert all(c["distinct"] == c["L"] - c["O"] + 2 for c in scripted)
    assert all(c["inexact"] == 0 for c in cases if c["E"] == 0) and all(c["partial"] == 0 for c in cases if c["O"] == c["m"])
    assert all(c["inexact"] > 0 for c in scripted if c["E"] > 0 and c["L"] >= 37)
    assert all(c["partial"] > 0 for c in scripted if c["O"] < c["m"])
    assert all(c["families"] >= 5 + 15 for c in scripted)
    # a lane of equal reads that carry the adapter: one family, one row of the histogram
    eq = [c for c in cases if c["mode"] == 1]
    assert len(eq) == 3 and all(c["families"] == 1 and c["distinct"] == 1 and c["with"] > 1000 for c in eq)
    assert all(c["families"] > 600 for c in cases if c["mode"] == 2)


def test_a_shift_that_drops_its_carry_is_noticed(tmp_path):
    out = subprocess.run([_build(tmp_path, "lane_adapter_emu_carry", "-DWD_LAD_DROP_CARRY")], capture_output=True,
                         text=True, timeout=900)
    assert out.returncode == 1 and "MISMATCH search" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])


def test_a_staging_block_one_row_short_is_noticed(tmp_path):
    out = subprocess.run([_build(tmp_path, "lane_adapter_emu_short", "-DLANE_ADAPTER_EMU_SHORT_LDS")],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode != 0 and "heap-buffer-overflow" in out.stderr, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
