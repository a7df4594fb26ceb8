"""k_lm_tally's source (csrc/lane_mismatch.inc) run on the CPU: tools/lane_mismatch_emu.cpp compiles the kernel as
it stands and plays the 256 lanes of a workgroup with fibers that meet at every __syncthreads, __ballot and __shfl, so
the wave-grouped adds, the LDS histogram, its flush and the cycles beyond its window are checked against the header's
definitions here, without a GPU (the GPU tests compare the kernel itself with tests/lanemismatch_ref.py:
tests/test_gpu_lanemismatch.py)."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emulated_kernel_gives_the_definitions_counts(tmp_path):
    exe = str(tmp_path / "lane_mismatch_emu")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
                           "-I" + os.path.join(REPO, "include"), os.path.join(REPO, "tools", "lane_mismatch_emu.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "MISMATCH" not in out.stdout, (out.stdout, out.stderr)
    ok = re.findall(r"trial (\d+) ok: L (\d+) N (\d+) max_d (\d+) mode (\d+) pairs (\d+)", out.stdout)
    assert len(ok) == 12 and all(int(t[5]) > 0 for t in ok)
    window = int(re.search(r"constexpr int kLmWindow = (\d+);",
                           open(os.path.join(REPO, "well_duplicates_amd", "csrc", "lane_mismatch.inc")).read()).group(1))
    # the ground: every max_d, runs that end inside a tile and tiles of more than a run, reads on both sides of the
    # window, and each of the three kinds of lane on both
    assert {int(t[3]) for t in ok} == set(range(8)) and {int(t[2]) for t in ok} == {700, 9000}
    for mode in (0, 1, 2):
        sizes = {int(t[1]) for t in ok if int(t[4]) == mode}
        assert min(sizes) < window < max(sizes) or mode == 2, (mode, sizes)
