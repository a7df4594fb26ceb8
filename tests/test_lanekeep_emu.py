"""The kernels of csrc/lane_keep.inc run on the CPU under shuffled schedules: tools/lane_keep_emu.cpp compiles k_lk_score
and k_lk_mark as they stand (with lgc_piece of csrc/lane_gc.inc), plays the 256 lanes of a workgroup with fibers
(tools/wave_emu.h), launches the two as wd_lane_keep launches them and lets the schedule hand over to another lane at
every atomic - never, always, with probability 1/3 under eight seeds, lanes in reverse, workgroups permuted.  Which
lane's atomicMin reaches a family's word first depends on the schedule: under each one every score, every family's
word, every mask byte and every counter must be what the header's definitions give, computed directly, so the same
under every schedule.  The program is built with the address and undefined-behaviour sanitizers.  A second build whose
minimum is broken on purpose (-DWAVE_EMU_TORN_MIN: a scheduling point between its load and its store, so that a lane
writes over a smaller key another lane stored in between) must end in MISMATCH: the test can fail.  No GPU is involved;
the emulation is sequentially consistent and says nothing about caches or time (the GPU tests compare the kernels
themselves with tests/lanekeep_ref.py: tests/test_gpu_lanekeep.py)."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
         "-I" + os.path.join(REPO, "include")]
SRC = os.path.join(REPO, "tools", "lane_keep_emu.cpp")
NAMES = ("case", "N", "L", "words", "mis", "min_q", "mode", "schedules", "families", "moved", "planted", "mins", "bound",
         "points")
LINE = re.compile(r"case (\d+) ok: N (\d+) L (\d+) words (\d+) mis (\d+) min_q (\d+) mode (\d+) schedules (\d+) "
                  r"families (\d+) moved (\d+) planted (\d+) mins (\d+) bound (\d+) points (\d+)")
RUN = 8192                                                             # kLaneRun


def test_every_schedule_gives_the_definitions_result(tmp_path):
    exe = str(tmp_path / "lane_keep_emu")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "MISMATCH" not in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
    cases = [dict(zip(NAMES, (int(v) for v in row))) for row in LINE.findall(out.stdout)]
    assert len(cases) == len(out.stdout.strip().split("\n")) == 18
    # never, reverse, always and eight seeds at 1/3 per case
    assert all(c["schedules"] == 11 and c["points"] > 0 for c in cases)
    fam = [c for c in cases if c["mode"] == 0]
    # the ground: rows of 1, 3, 4, 6, 16 and 103 words at every offset of the base from a 16-byte boundary; tiles whose
    # wells are 1, 2 and 3 past a multiple of four, of less than a run and of a run and a bit; every min_q
    assert {c["words"] for c in fam} == {1, 3, 4, 6, 16, 103} == {c["words"] for c in cases if c["mode"]}
    assert {c["mis"] for c in cases} == {0, 1, 2, 3}
    assert {c["N"] % 4 for c in cases} >= {1, 2, 3} and {c["N"] for c in cases} >= {RUN + 1, 9000}
    assert {c["N"] for c in fam if c["words"] >= 16} >= {701, RUN + 1}
    assert {c["min_q"] for c in fam} == {0, 15, 64} and {c["min_q"] for c in cases if c["mode"] == 1} == {0, 15}
    # the six block families, the five hand-made ones and sparse ones besides; with weights, families whose best is not
    # their root, and with every weight zero none
    assert all(c["planted"] == c["families"] >= 11 + 20 for c in fam)
    assert all(c["moved"] >= 3 for c in fam if c["min_q"] < 64) and all(c["moved"] == 0 for c in fam if c["min_q"] == 64)
    # a lane of equal reads is one family: with one quality its root stays, with random ones it does not; and the
    # atomics of k_lk_score on it stay at or below one per wave and trip (the emulator fails above the bound) - in fact far below
    eq = [c for c in cases if c["mode"] in (1, 2)]
    assert len(eq) == 6 and all(c["families"] == 1 for c in eq)
    assert all(c["moved"] == 0 for c in eq if c["mode"] == 1) and all(c["moved"] == 1 for c in eq if c["mode"] == 2)
    assert all(0 < c["mins"] <= c["bound"] for c in eq)
    assert all(c["mins"] <= 16 for c in eq if c["mode"] == 1)         # one per wave, while the first are under way


def test_a_torn_minimum_is_noticed(tmp_path):
    exe = str(tmp_path / "lane_keep_emu_torn")
    subprocess.check_call(["g++"] + FLAGS + ["-DWAVE_EMU_TORN_MIN", SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 1 and "MISMATCH" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
