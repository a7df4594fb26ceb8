"""k_lg_tally's source (csrc/lane_distance.inc) run on the CPU: tools/lane_distance_emu.cpp compiles the kernel as it
stands on the shims of tools/wave_emu.h, which play the 256 lanes of a workgroup with fibers that meet at every
__syncthreads, __ballot and __shfl, so the wave-grouped adds, the bin taken from the highest bit, the LDS histogram of
root tiles and its flush are checked against the header's definitions here, without a GPU (the GPU tests compare the
kernel itself with tests/lanedistance_ref.py: tests/test_gpu_lanedistance.py)."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emulated_kernel_gives_the_definitions_counts(tmp_path):
    exe = str(tmp_path / "lane_distance_emu")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
                           "-I" + os.path.join(REPO, "include"), os.path.join(REPO, "tools", "lane_distance_emu.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "MISMATCH" not in out.stdout and "runtime error" not in out.stderr, (out.stdout, out.stderr)
    ok = re.findall(r"trial (\d+) ok: N (\d+) mode (\d+) radius (\d+) matrix (\d+) pairs (\d+) same (\d+) local (\d+) dist ([\d ]+)",
                    out.stdout)
    assert len(ok) == 24 and all(int(t[5]) > 0 for t in ok)
    trials = [dict(n=int(t[1]), mode=int(t[2]), radius=int(t[3]), matrix=int(t[4]), pairs=int(t[5]), same=int(t[6]),
                   local=int(t[7]), dist=[int(v) for v in t[8].split()]) for t in ok]
    # the ground: a run that ends inside a tile and a tile of more than one run, the three kinds of lane, the four
    # radii, with the matrix and without - every kind of lane at every size and radius, and both ways
    assert {(t["n"], t["mode"], t["radius"]) for t in trials} == {(n, m, r) for n in (700, 9000) for m in (0, 1, 2)
                                                                  for r in (0, 32, 2500, 1 << 25)}
    for mode in (0, 1, 2):
        assert {t["matrix"] for t in trials if t["mode"] == mode} == {0, 1}
    for t in trials:
        assert sum(t["dist"]) == t["same"] and len(t["dist"]) == 11
        assert t["local"] == (0 if t["radius"] == 0 else t["same"] if t["radius"] == 1 << 25 else t["local"])
        if t["radius"] == 32:
            assert t["local"] == t["dist"][0]
        if t["mode"] == 1:                                             # equal reads: every PF well but one is a pair
            assert t["pairs"] > 1.7 * t["n"] and t["same"] < t["pairs"] and t["dist"][10] > 0
        if t["mode"] == 2:                                             # every copy beside its original
            assert t["dist"] == [t["same"]] + [0] * 10 and t["same"] == t["pairs"] > 0.9 * t["n"]
    # both emulators stand on one set of shims
    for name in ("lane_distance_emu.cpp", "lane_mismatch_emu.cpp"):
        text = open(os.path.join(REPO, "tools", name)).read()
        assert '#include "wave_emu.h"' in text and "ucontext_t" not in text and "swapcontext" not in text
