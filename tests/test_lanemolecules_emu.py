"""The emitting kernels of csrc/lane_umi.inc and the keep kernels on what they write, run on the CPU under shuffled
schedules: tools/lane_molecules_emu.cpp compiles k_lu_pairs_mol and k_lu_group_mol as they stand, behind k_lc_reserve and
k_lc_scatter of csrc/lane_consensus.inc, then k_lk_score and k_lk_mark of csrc/lane_keep.inc with mol and molmem in the
places of label and members, plays the 256 lanes of a workgroup with fibers (tools/wave_emu.h), launches them as
wd_lane_umi_molecules and wd_lane_keep_molecules do and lets the schedule hand over to another lane at every atomic.
Every buffer is a heap block of exactly its size, mol and molmem hold a pattern before each run and every store to them
is counted: under each schedule every word is written exactly once and is what include/welldup_lanemolecules.h defines,
by a union by brute force; so are the UMI rows, the mask bytes and the keep rows.  The program is built with the address
and undefined-behaviour sanitizers.  A second build whose compare-and-swap is broken on purpose (-DWAVE_EMU_TORN_CAS)
must end in MISMATCH: the test can fail.  No GPU is involved; the emulation is sequentially consistent and says nothing
about caches or time (the GPU tests compare the kernels themselves with tests/lanemolecules_ref.py:
tests/test_gpu_lanemolecules.py)."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
         "-I" + os.path.join(REPO, "include")]
SRC = os.path.join(REPO, "tools", "lane_molecules_emu.cpp")
NAMES = ("case", "U", "E", "N", "max_family", "schedules", "wells", "molecules", "redundant", "large", "largest", "big", "chains",
         "chains_200", "joined_pairs", "split_pairs", "kept_molecules", "moved", "dropped", "dropped_by_family", "ties", "points", "lost")
LINE = re.compile(r"case (\d+) ok: " + " ".join(r"%s (\d+)" % n for n in NAMES[1:]))


def test_every_schedule_gives_the_definitions_molecules_and_masks(tmp_path):
    exe = str(tmp_path / "lane_molecules_emu")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "MISMATCH" not in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
    cases = [dict(zip(NAMES, (int(v) for v in row))) for row in LINE.findall(out.stdout)]
    assert len(cases) == len(out.stdout.strip().split("\n")) == 8
    assert all(c["schedules"] == 11 and c["points"] > 0 for c in cases)
    # the ground: every UMI length, every E and one at or above U; N % 4 = 1, 2, 3 and a run and a bit; the cap at 2
    # (nothing gathered but the pairs), at 70 and at 1024; a family at the cap and one above it in every case
    assert {c["U"] for c in cases} == {1, 8, 10, 11, 20} and {c["E"] for c in cases} == {0, 1, 2, 3}
    assert any(c["E"] >= c["U"] for c in cases)
    assert {c["N"] % 4 for c in cases} == {1, 2, 3} and any(c["N"] > 8192 for c in cases) and any(c["N"] < 8192 for c in cases)
    assert {c["max_family"] for c in cases} == {2, 70, 1024}
    assert all(c["largest"] == c["max_family"] and c["large"] >= 1 for c in cases)
    # the chains that are gathered (a Large family's UMIs are never looked at): none at the cap of 2; of 3, 3, 64, 65 and
    # 65 wells at 70; at 1024 thirteen - the chains of 3, 64, 65 and 200 each with ids ascending, descending and permuted
    assert {c["max_family"]: c["chains"] for c in cases} == {2: 0, 70: 5, 1024: 13}
    assert all(c["chains_200"] == (7 if c["max_family"] == 1024 else 0) for c in cases)
    # pairs that are one molecule and pairs that are two; families of more than 64 wells wherever the cap lets them in
    assert all(c["joined_pairs"] > 0 for c in cases)
    assert all(c["split_pairs"] > 0 for c in cases if c["E"] < c["U"])
    assert all(c["big"] >= 7 for c in cases if c["max_family"] >= 70) and all(c["big"] >= 13 for c in cases if c["max_family"] == 1024)
    # molecules of two or more wells, some whose best well is not their first, wells of equal scores in one molecule
    assert all(c["kept_molecules"] > 0 and c["moved"] > 0 and c["ties"] > 0 for c in cases)
    # by molecule never drops more than by family, fewer wherever a family splits, and the same at E >= U
    assert all(c["dropped"] <= c["dropped_by_family"] for c in cases)
    assert all(c["dropped"] < c["dropped_by_family"] for c in cases if c["E"] < c["U"])
    assert all(c["dropped"] == c["dropped_by_family"] for c in cases if c["E"] >= c["U"])
    # the union-find in LDS lost compare-and-swaps under the shuffled schedules, and the result stood
    assert sum(c["lost"] for c in cases) > 100


def test_a_torn_compare_and_swap_is_noticed(tmp_path):
    exe = str(tmp_path / "lane_molecules_emu_torn")
    subprocess.check_call(["g++"] + FLAGS + ["-DWAVE_EMU_TORN_CAS", SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 1 and "MISMATCH" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
