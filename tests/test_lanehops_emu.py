"""k_lh_tally's source (csrc/lane_hops.inc) run on the CPU: tools/lane_hops_emu.cpp compiles the kernel as it stands and
plays the 256 lanes of a workgroup with fibers that meet at every __syncthreads, __ballot and __shfl, so the two
wave-grouped adds, the binary search of the listing, the LDS table of matrix cells, its overflow into memory and its
flush are checked against the header's definitions here, without a GPU (the GPU tests compare the kernel itself with
tests/lanehops_ref.py: tests/test_gpu_lanehops.py).  Every trial runs under the eleven schedules of tools/emu_reads.h - a
lane may hand over at every atomic -, so the claims of the LDS table (a plain atomicCAS) meet on free entries; those
that lose are counted, and a second build with that claim torn on purpose (-DWAVE_EMU_TORN_CAS=3) must end in MISMATCH."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = ["g++", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
         "-I" + os.path.join(REPO, "include"), os.path.join(REPO, "tools", "lane_hops_emu.cpp")]


def test_emulated_kernel_gives_the_definitions_counts(tmp_path):
    exe = str(tmp_path / "lane_hops_emu")
    subprocess.check_call(BUILD + ["-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "MISMATCH" not in out.stdout, (out.stdout, out.stderr)
    ok = re.findall(r"trial (\d+) ok: I (\d+) split (\d+) E (\d+) N (\d+) M (\d+) mode (\d+) pairs (\d+) cells (\d+) slots (\d+)",
                    out.stdout)
    t = [tuple(int(v) for v in row) for row in ok]
    trials = [dict(zip(("trial", "I", "split", "E", "N", "M", "mode", "pairs", "cells", "slots"), row)) for row in t]
    assert len(trials) == 12 and all(r["pairs"] > 0 for r in trials)
    slots = int(re.search(r"constexpr int kLhSlots = (\d+);",
                          open(os.path.join(REPO, "well_duplicates_amd", "csrc", "lane_hops.inc")).read()).group(1))
    assert {r["slots"] for r in trials} == {slots}
    # the ground: runs that end inside a trip and tiles of more than a run; part 2 empty, beginning inside the first
    # word, at the word boundary and inside the second; every E and M asked for
    assert {r["N"] for r in trials} == {700, 9000}
    assert {(r["I"], r["split"]) for r in trials} == {(8, 8), (16, 8), (16, 16), (20, 10), (20, 13)}
    assert {r["E"] for r in trials} == {0, 1, 3} and {r["M"] for r in trials} == {0, 3, 1024}
    # a pool, one key (one cell), every key unlisted (one cell: Other x Other), more cells in a run than the table holds
    assert {r["mode"] for r in trials} == {0, 1, 2, 3}
    assert all(r["cells"] == 1 for r in trials if r["mode"] in (1, 2))
    assert any(r["cells"] > 4 * slots for r in trials if r["mode"] == 3)
    assert any(r["N"] == 9000 and r["mode"] == 1 for r in trials)
    # the eleven schedules: the one that never hands over loses nothing; the pooled trials and those with many cells
    # lose claims of the LDS table, summed over the schedules at 1/3
    sched = re.findall(r"trial (\d+) ok: .* mode (\d+) .* schedules (\d+) points (\d+) never_lost (\d+) lost_lds (\d+)$", out.stdout, re.M)
    sched = [dict(zip(("trial", "mode", "schedules", "points", "never_lost", "lost_lds"), (int(v) for v in row))) for row in sched]
    assert [r["trial"] for r in sched] == list(range(12)) and [r["mode"] for r in sched] == [r["mode"] for r in trials]
    assert all(r["schedules"] == 11 and r["never_lost"] == 0 and r["points"] > 0 for r in sched)
    assert all(r["lost_lds"] >= 1 for r in sched if r["mode"] in (0, 3))
    assert sum(r["mode"] == 0 for r in sched) >= 5 and sum(r["mode"] == 3 for r in sched) == 2


def test_a_torn_claim_of_the_lds_table_is_noticed(tmp_path):
    exe = str(tmp_path / "lane_hops_emu_torn")
    subprocess.check_call(BUILD + ["-DWAVE_EMU_TORN_CAS=3", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 1 and "MISMATCH" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
