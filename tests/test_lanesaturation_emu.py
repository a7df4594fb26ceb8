"""k_ls_min's and k_ls_tally's source (csrc/lane_saturation.inc) run on the CPU: tools/lane_saturation_emu.cpp compiles
the kernels as they stand on the shims of tools/wave_emu.h, which play the 256 lanes of a workgroup with fibers that
meet at every __syncthreads and __ballot, so the step function, the dropped test, the pre-read before the atomic
minimum, the LDS histogram and its flush are checked against the header's definitions here, without a GPU (the GPU
tests compare the kernels themselves with tests/lanesaturation_ref.py: tests/test_gpu_lanesaturation.py)."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emulated_kernels_give_the_definitions_counts(tmp_path):
    exe = str(tmp_path / "lane_saturation_emu")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
                           "-I" + os.path.join(REPO, "include"), os.path.join(REPO, "tools", "lane_saturation_emu.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "MISMATCH" not in out.stdout and "runtime error" not in out.stderr, (out.stdout, out.stderr)
    ok = re.findall(r"trial (\d+) ok: N (\d+) mode (\d+) steps (\d+) radius (-?\d+) pf (\d+) dropped (\d+) reads (\d+) "
                    r"distinct (\d+)", out.stdout)
    assert len(ok) == 72 and len(out.stdout.strip().split("\n")) == 72
    trials = [dict(zip(("n", "mode", "steps", "radius", "pf", "dropped", "reads", "distinct"), (int(v) for v in t[1:])))
              for t in ok]
    # the ground: a run that ends inside a tile and a tile of more than one run, the three kinds of lane, 1, 20 and
    # 64 steps, the three radii and the form without coordinates (radius -1) - every combination
    assert {(t["n"], t["mode"], t["steps"], t["radius"]) for t in trials} == {
        (n, m, s, r) for n in (700, 9000) for m in (0, 1, 2) for s in (1, 20, 64) for r in (0, 2500, 1 << 25, -1)}
    for t in trials:
        assert t["reads"] == t["pf"] - t["dropped"] and 0 < t["distinct"] <= t["reads"]
        if t["radius"] <= 0:
            assert t["dropped"] == 0
        if t["mode"] == 0:                                             # sparse pairs within and across tiles
            assert t["distinct"] < t["reads"] and (t["radius"] != 1 << 25 or t["dropped"] > 0)
        if t["mode"] == 1:                                             # equal reads: one molecule
            assert t["distinct"] == 1 and (t["radius"] != 1 << 25 or 0.3 * t["pf"] < t["dropped"] < 0.7 * t["pf"])
        if t["mode"] == 2 and t["radius"] > 0:                         # every copy beside its original: all dropped
            assert t["distinct"] == t["reads"] and t["dropped"] > 0.45 * t["pf"]
    text = open(os.path.join(REPO, "tools", "lane_saturation_emu.cpp")).read()
    assert '#include "wave_emu.h"' in text and "ucontext_t" not in text and "swapcontext" not in text
    assert "atomicMin" in open(os.path.join(REPO, "tools", "wave_emu.h")).read()
