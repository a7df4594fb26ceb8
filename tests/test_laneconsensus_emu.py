"""The three kernels of csrc/lane_consensus.inc run on the CPU under shuffled schedules: tools/lane_consensus_emu.cpp
compiles k_lc_reserve, k_lc_scatter and k_lc_vote as they stand, plays the 256 lanes of a workgroup with fibers
(tools/wave_emu.h), launches the three with the grids the host call gives them and lets the schedule hand over to
another lane at every atomic - never, always, with probability 1/3 under eight seeds, lanes in reverse, workgroups
permuted.  Where a copy lands in its family's range depends on the schedule: under each one every range must be a
permutation of the family's copies, and the counters and the call matrix must be what the header's definitions give,
so the same under every schedule.  A second build whose atomic add is broken on purpose (-DWAVE_EMU_TORN_ADD: a
scheduling point between its load and its store) must end in MISMATCH: the test can fail.  No GPU is involved; the
emulation is sequentially consistent and says nothing about caches or time (the GPU tests compare the kernels
themselves with tests/laneconsensus_ref.py: tests/test_gpu_laneconsensus.py)."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
         "-I" + os.path.join(REPO, "include")]
SRC = os.path.join(REPO, "tools", "lane_consensus_emu.cpp")
NAMES = ("case", "L", "words", "N", "max_d", "max_family", "schedules", "families", "wells", "profiled", "mismatches",
         "with_n", "undecided", "first_off", "pairs", "large", "dist8", "beyond", "points")
LINE = re.compile(r"case (\d+) ok: L (\d+) words (\d+) N (\d+) max_d (\d+) max_family (\d+) schedules (\d+) families (\d+) "
                  r"wells (\d+) profiled (\d+) mismatches (\d+) with_n (\d+) undecided (\d+) first_off (\d+) pairs (\d+) "
                  r"large (\d+) dist8 (\d+) beyond (\d+) points (\d+)")


def test_every_schedule_gives_the_definitions_counts(tmp_path):
    exe = str(tmp_path / "lane_consensus_emu")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "MISMATCH" not in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
    cases = [dict(zip(NAMES, (int(v) for v in row))) for row in LINE.findall(out.stdout)]
    assert len(cases) == len(out.stdout.strip().split("\n")) == 12
    # never, reverse, always and eight seeds at 1/3 per case
    assert all(c["schedules"] == 11 and c["points"] > 0 for c in cases)
    # the ground: every row length with a tile of less than a run and one of a run and a bit; every max_d; families at
    # the cap and one above it (large >= 1 in every case: the family of max_family + 1 wells), the cap at 4096 once
    assert {(c["words"], c["N"]) for c in cases} == {(w, n) for w in (1, 3, 4, 6, 16, 103) for n in (700, 9000)}
    assert {c["max_d"] for c in cases} == set(range(8))
    assert {c["max_family"] for c in cases} == {64, 70, 4096}
    assert all(c["large"] >= 1 and c["pairs"] >= 4 and c["families"] >= 100 for c in cases)
    assert all(c["wells"] >= 3 * c["families"] + 63 + 64 + c["max_family"] for c in cases)
    assert all(c["wells"] >= 4096 + 65 + 64 + 63 for c in cases if c["max_family"] == 4096)
    # wells that disagree with the vote, wells beyond d = 7, cycles without a majority, first wells that are off
    assert all(c["undecided"] >= 10 and c["first_off"] >= 10 and c["dist8"] >= 5 and c["profiled"] < c["wells"] for c in cases)
    assert all(c["mismatches"] > 0 and c["with_n"] > 0 for c in cases if c["max_d"] >= 1)
    assert all(c["mismatches"] == 0 for c in cases if c["max_d"] == 0)
    # errors beyond the LDS window, where calls is added to in memory at once
    window = int(re.search(r"constexpr int kLmWindow = (\d+);",
                           open(os.path.join(REPO, "well_duplicates_amd", "csrc", "lane_mismatch.inc")).read()).group(1))
    assert window < 1024 and sum(c["beyond"] for c in cases if c["L"] == 1024) > 100
    assert all(c["beyond"] == 0 for c in cases if c["L"] <= window)


def test_a_torn_add_is_noticed(tmp_path):
    exe = str(tmp_path / "lane_consensus_emu_torn")
    subprocess.check_call(["g++"] + FLAGS + ["-DWAVE_EMU_TORN_ADD", SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 1 and "MISMATCH" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
