"""k_lq_tally's source (csrc/lane_quality.inc, with lm_compare and lm_fold of csrc/lane_mismatch.inc) run on the CPU:
tools/lane_quality_emu.cpp compiles the kernel as it stands on tools/wave_emu.h, so the grouping by ballots, the
counting of a word's observations cell by cell, the cell carried across words, the mask of the last word and the flush
of the LDS histogram are checked against the header's definitions here, without a GPU (the GPU tests compare the
kernel itself with tests/lanequality_ref.py: tests/test_gpu_lanequality.py)."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emulated_kernel_gives_the_definitions_counts(tmp_path):
    exe = str(tmp_path / "lane_quality_emu")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
                           "-I" + os.path.join(REPO, "include"), os.path.join(REPO, "tools", "lane_quality_emu.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "MISMATCH" not in out.stdout, (out.stdout, out.stderr)
    ok = re.findall(r"trial (\d+) ok: L (\d+) N (\d+) max_d (\d+) mode (\d+) pairs (\d+) profiled (\d+) cells (\d+) most (\d+)",
                    out.stdout)
    ok = [tuple(int(v) for v in t) for t in ok]
    assert len(ok) == 14 and all(t[5] > 0 and t[6] > 0 for t in ok)
    # the ground: every kind of lane at L = 37, 83 and 1024, tiles of less than a run and of more, every max_d
    for mode in (0, 1, 2, 3):
        assert {37, 1024} <= {t[1] for t in ok if t[4] == mode} and (mode == 3 or 83 in {t[1] for t in ok if t[4] == mode})
    assert {t[2] for t in ok} == {700, 9000} and {t[3] for t in ok} == set(range(8))
    for t in ok:
        if t[4] == 1:                                      # equal reads, one quality: every observation in one cell
            assert t[7] == 1 and t[8] == t[6] * t[1] and t[6] == t[5]
        if t[4] == 2:                                      # equal reads, random qualities: every pair profiled, many cells
            assert t[6] == t[5] and t[7] >= 32
        if t[4] == 3:                                      # one pair whose cycles visit the cells in turn
            assert t[5] == 1 and t[7] == min(t[1], 64) and t[8] == -(-t[1] // 64)
    assert any(t[4] == 3 and t[1] == 64 and t[7] == 64 and t[8] == 1 for t in ok)      # every cell, one observation each
