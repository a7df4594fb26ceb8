"""The kernels of csrc/lane_umi.inc run on the CPU under shuffled schedules: tools/lane_umi_emu.cpp compiles k_lu_pairs
and k_lu_group as they stand, behind k_lc_reserve and k_lc_scatter of csrc/lane_consensus.inc, plays the 256 lanes of a
workgroup with fibers (tools/wave_emu.h), launches the four as wd_lane_umi launches them and lets the schedule hand over
to another lane at every atomic - never, always, with probability 1/3 under eight seeds, lanes in reverse, workgroups
permuted.  Where a copy lands in its family's range, and which member becomes the root of a component of the union-find
in LDS, depend on the schedule: under each one the counters must be what the header's definitions give, computed by a
union by brute force, so the same under every schedule.  The program is built with the address and undefined-behaviour
sanitizers.  A second build whose compare-and-swap is broken on purpose (-DWAVE_EMU_TORN_CAS: a scheduling point
between its load and its store, so that two lanes hook the same root) must end in MISMATCH: the test can fail.  No GPU
is involved; the emulation is sequentially consistent and says nothing about caches or time (the GPU tests compare the
kernels themselves with tests/laneumi_ref.py: tests/test_gpu_laneumi.py)."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
         "-I" + os.path.join(REPO, "include")]
SRC = os.path.join(REPO, "tools", "lane_umi_emu.cpp")
NAMES = ("case", "U", "E", "N", "max_family", "schedules", "wells", "redundant", "lone", "families", "molecules", "distinct",
         "split", "with_n", "large", "largest", "chains", "second_word", "big_molecules", "points", "lost")
LINE = re.compile(r"case (\d+) ok: U (\d+) E (\d+) N (\d+) max_family (\d+) schedules (\d+) wells (\d+) redundant (\d+) "
                  r"lone (\d+) families (\d+) molecules (\d+) distinct (\d+) split (\d+) with_n (\d+) large (\d+) "
                  r"largest (\d+) chains (\d+) second_word (\d+) big_molecules (\d+) points (\d+) lost (\d+)")


def test_every_schedule_gives_the_definitions_counts(tmp_path):
    exe = str(tmp_path / "lane_umi_emu")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "MISMATCH" not in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
    cases = [dict(zip(NAMES, (int(v) for v in row))) for row in LINE.findall(out.stdout)]
    assert len(cases) == len(out.stdout.strip().split("\n")) == 12
    # never, reverse, always and eight seeds at 1/3 per case
    assert all(c["schedules"] == 11 and c["points"] > 0 for c in cases)
    # the ground: every UMI length and every E, both with a tile of less than a run and one of a run and a bit; the cap
    # at 2 (nothing gathered but the pairs), below 128, above it and at 1024; a family at the cap in every case and one
    # above it (large >= 1)
    assert {c["U"] for c in cases} == {1, 8, 10, 11, 20} and {c["E"] for c in cases} == {0, 1, 2, 3}
    assert {c["U"] for c in cases if c["N"] == 9000} == {1, 8, 10, 11, 20} and {c["N"] for c in cases} == {1000, 9000}
    assert {c["max_family"] for c in cases} == {2, 70, 130, 1024}
    assert all(c["largest"] == c["max_family"] and c["large"] >= 1 and c["chains"] == 6 for c in cases)
    assert all(c["families"] >= 50 and c["wells"] >= 2 * c["families"] for c in cases)
    assert all(c["wells"] >= 2 + 3 + 63 + 64 + 65 + 128 + c["max_family"] + 200 for c in cases if c["max_family"] >= 130)
    # split families, lone wells and wells with N; molecules merged by a read error wherever E allows one
    assert all(c["with_n"] > 0 and c["redundant"] > 0 for c in cases)
    assert all(c["split"] > 0 and c["lone"] > 0 for c in cases if c["E"] < c["U"])
    assert all(c["molecules"] == c["distinct"] for c in cases if c["E"] == 0)
    assert all(c["families"] < c["molecules"] < c["distinct"] for c in cases if 1 <= c["E"] < c["U"])
    assert all(c["families"] == c["molecules"] and c["lone"] == 0 and c["split"] == 0 for c in cases if c["E"] >= c["U"])
    # molecules of 65 or more wells: a chain that only the closure joins, beyond one chunk of the wave
    assert all(c["big_molecules"] >= 1 for c in cases if c["max_family"] >= 70)
    assert all(c["big_molecules"] >= 2 for c in cases if c["max_family"] >= 130 and c["E"] >= 1)
    # an edge whose keys differ in the second word alone
    assert all(c["second_word"] > 0 for c in cases if c["U"] > 10 and c["E"] >= 1)
    assert all(c["second_word"] == 0 for c in cases if c["U"] <= 10)
    # the union-find in LDS lost compare-and-swaps under the shuffled schedules - two lanes at one root - and the
    # result stood
    assert sum(c["lost"] for c in cases) > 100


def test_a_torn_compare_and_swap_is_noticed(tmp_path):
    exe = str(tmp_path / "lane_umi_emu_torn")
    subprocess.check_call(["g++"] + FLAGS + ["-DWAVE_EMU_TORN_CAS", SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 1 and "MISMATCH" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
