"""k_lt_hist's, k_lt_collect's and k_lt_spread's source (csrc/lane_top.inc) run on the CPU: tools/lane_top_emu.cpp
compiles the kernels as they stand on the shims of tools/wave_emu.h, which play the 256 lanes of a workgroup with
fibers that meet at every __syncthreads, __ballot and __shfl, so the first pass's bins and levels, a linear pass over a
range of keys, the compaction behind one atomic per wave and the LDS table's spread and exact counts are checked
against the header's definitions here, without a GPU (the GPU tests compare the kernels themselves with
tests/lanetop_ref.py: tests/test_gpu_lanetop.py)."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emulated_kernels_give_the_definitions_counts(tmp_path):
    exe = str(tmp_path / "lane_top_emu")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
                           "-I" + os.path.join(REPO, "include"), os.path.join(REPO, "tools", "lane_top_emu.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "MISMATCH" not in out.stdout and "runtime error" not in out.stderr, (out.stdout, out.stderr)
    ok = re.findall(r"trial (\d+) ok: N (\d+) mode (\d+) words (\d+) pf (\d+) groups (\d+) candidates (\d+) listed (\d+)",
                    out.stdout)
    assert len(ok) == 18 and len(out.stdout.strip().split("\n")) == 18
    trials = [dict(zip(("n", "mode", "words", "pf", "groups", "candidates", "listed"), (int(v) for v in t[1:]))) for t in ok]
    # the ground: a run that ends inside a tile and a tile of more than one run, the three kinds of lane, rows of one
    # to four words, a list of five and a full one
    assert {(t["n"], t["mode"]) for t in trials} == {(n, m) for n in (700, 9000) for m in (0, 1, 2)}
    assert {t["words"] for t in trials} == {1, 2, 3, 4}
    for t in trials:
        assert 0 < t["candidates"] <= t["groups"] and 0 < t["listed"] <= min(t["groups"], 1024)
        if t["mode"] == 0:                                             # scattered groups of 2 .. 600 wells
            assert 10 <= t["groups"] <= 24
        if t["mode"] == 1:                                             # equal reads: one group holds the lane
            assert t["groups"] == 1
        if t["mode"] == 2:                                             # pairs only
            assert t["groups"] == t["pf"] // 2
    assert any(t["listed"] == 1024 for t in trials) and any(t["listed"] == 5 for t in trials)
    text = open(os.path.join(REPO, "tools", "lane_top_emu.cpp")).read()
    assert '#include "wave_emu.h"' in text and "ucontext_t" not in text and "swapcontext" not in text
    assert "mbcnt" in open(os.path.join(REPO, "tools", "wave_emu.h")).read()
