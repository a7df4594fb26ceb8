"""k_lgc_tally's source (csrc/lane_gc.inc) run on the CPU: tools/lane_gc_emu.cpp compiles the kernel as it stands and
plays the 256 lanes of a workgroup with fibers that meet at every __syncthreads, __ballot and __shfl, so the
contiguous 16-byte loading with its head and tail, the wells' sums in LDS with their double buffer, the wave-grouped
histogram, its overflow into memory beyond the LDS window and its flush are checked against the header's definitions
here, without a GPU (the GPU tests compare the kernel itself with tests/lanegc_ref.py: tests/test_gpu_lanegc.py)."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emulated_kernel_gives_the_definitions_counts(tmp_path):
    exe = str(tmp_path / "lane_gc_emu")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
                           "-I" + os.path.join(REPO, "include"), os.path.join(REPO, "tools", "lane_gc_emu.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "MISMATCH" not in out.stdout, (out.stdout, out.stderr)
    names = ("trial", "L", "words", "N", "max_n", "mode", "mis", "counted", "skipped", "beyond")
    ok = re.findall(r"trial (\d+) ok: L (\d+) words (\d+) N (\d+) max_n (\d+) mode (\d+) mis (\d+) counted (\d+) "
                    r"skipped (\d+) beyond (\d+)", out.stdout)
    trials = [dict(zip(names, (int(v) for v in row))) for row in ok]
    assert len(trials) == 18 and all(r["counted"] > 0 for r in trials)
    # the ground: runs that end inside a trip and tiles of more than a run; every row length with both; a rows' base
    # at every offset from a 16-byte boundary; the three kinds of lane; max_n of 0, 1 and L with every row length
    assert {r["N"] for r in trials} == {700, 9000}
    assert {(r["words"], r["N"]) for r in trials} == {(w, n) for w in (1, 3, 4, 6, 16, 103) for n in (700, 9000)}
    assert {r["mis"] for r in trials} == {0, 1, 2, 3} and {r["mode"] for r in trials} == {0, 1, 2}
    for words in (1, 3, 4, 6, 16, 103):
        mine = [r for r in trials if r["words"] == words]
        assert sorted(min(r["max_n"], 2) for r in mine) == [0, 1, 2] and {r["mode"] for r in mine} == {0, 1, 2}
        assert len({r["mis"] for r in mine}) == 3
    assert any(r["skipped"] > 0 for r in trials) and all(r["skipped"] == 0 for r in trials if r["max_n"] == r["L"])
    # g beyond the LDS window, where the histogram is added to in memory at once
    window = int(re.search(r"constexpr int kLgcWindow = (\d+);",
                           open(os.path.join(REPO, "well_duplicates_amd", "csrc", "lane_gc.inc")).read()).group(1))
    assert window < 1024 and sum(r["beyond"] for r in trials if r["L"] == 1024) > 500
    assert all(r["beyond"] == 0 for r in trials if r["L"] < window)
