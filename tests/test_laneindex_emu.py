"""The seven kernels of csrc/lane_index.inc run on the CPU under shuffled schedules: tools/lane_index_emu.cpp compiles
them as they stand, launches them as wd_lane_index_add, li_tally and wd_lane_index_finish do, plays the 256 lanes of a
workgroup with fibers (tools/wave_emu.h) and lets the schedule hand over to another lane at every atomic - never,
always, with probability 1/3 under eight seeds, lanes in reverse, workgroups permuted.  Each schedule must give the
definitions of include/welldup_laneindex.h computed directly, and the same glabel as every other.  The GPU tests
(tests/test_gpu_laneindex.py) see the few orders the hardware happens to produce; here the claims lost in the lane's
table (claim_or_join under k_li_group's and k_li_sub's closures) and in k_li_tally's table in LDS (a plain atomicCAS)
are counted, and a case whose schedules lose none has not tested what it is there for.  Two more builds with a
compare-and-swap broken on purpose - the table's claim, and the LDS claim alone - must end in MISMATCH: the test can
fail.  No GPU is involved; the emulation is sequentially consistent and says nothing about caches or time."""
import os
import re
import subprocess

import numpy as np

from contention_inputs import LANE_RUN, LI_PROBE, LI_SLOTS, li_home

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
         "-I" + os.path.join(REPO, "include")]
SRC = os.path.join(REPO, "tools", "lane_index_emu.cpp")
NAMES = ("case", "family", "I", "N", "unaligned", "k", "slot", "schedules", "pf", "groups", "spans", "mixed_classes",
         "mixed_wells", "field", "listed", "chunk", "points", "never_lost", "lost_table", "lost_lds")
LINE = re.compile(r"case (\d+) ok: family (\w+) " + " ".join(r"%s (-?\d+)" % name for name in NAMES[2:]))


def _constant(name, inc):
    text = open(os.path.join(REPO, "well_duplicates_amd", "csrc", inc)).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def test_every_schedule_gives_the_definitions_index(tmp_path):
    exe = str(tmp_path / "lane_index_emu")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "MISMATCH" not in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
    lines = out.stdout.strip().split("\n")
    cases = [dict(zip(NAMES, (v if i == 1 else int(v) for i, v in enumerate(row)))) for row in LINE.findall(out.stdout)]
    assert len(cases) == len(lines) - 1 >= 30
    # never, reverse, always and eight seeds at 1/3 per case; the schedule that never yields loses no compare-and-swap
    assert all(c["schedules"] == 11 and c["never_lost"] == 0 for c in cases)
    fam = lambda name: [c for c in cases if c["family"] == name]
    probe, run = _constant("kLiProbe", "lane_index.inc"), _constant("kLaneRun", "lane_pass.inc")
    assert (probe, run, _constant("kLiSlots", "lane_index.inc")) == (LI_PROBE, LANE_RUN, LI_SLOTS)
    # the pool: less than a run and a run and a bit; keys of one cycle, inside a word, of exactly one word, one cycle
    # more, two words; planes aligned (k_li_pack<true>) and not; classes inside a group and across groups
    pool = fam("pool")
    assert {(c["N"], c["I"]) for c in pool} == {(n, i) for n in (700, 9000) for i in (1, 8, 10, 11, 16, 20)}
    assert {c["unaligned"] for c in pool} == {0, 1}
    assert all(c["groups"] >= (5 if c["I"] == 1 else 12) and c["pf"] < 2 * c["N"] * 0.93 for c in pool)
    assert all(c["mixed_classes"] >= 10 and c["spans"] > c["mixed_classes"] * 2 and c["mixed_wells"] > 100 for c in pool)
    # the probe edge: as many groups as a probe path is long, one more, four more, at representatives with one home
    edge = fam("probe")
    assert sorted((c["k"], c["I"]) for c in edge) == [(probe, 8), (probe + 1, 8), (probe + 1, 20), (probe + 4, 8)]
    assert all(c["groups"] == c["k"] and 0 <= c["slot"] < LI_SLOTS and c["N"] > run for c in edge)
    # what those two are for: claims lost in the lane's table and in the LDS table, summed over the schedules at 1/3
    assert all(c["lost_table"] >= 1 and c["lost_lds"] >= 1 for c in pool + edge)
    # one key: a workgroup's 16-bit fields reach a whole run
    one = fam("one_class") + fam("pairs")
    assert {(c["family"], c["N"]) for c in one} == {(f, n) for f in ("one_class", "pairs") for n in (run, run + 1)}
    assert all(c["groups"] == 1 and c["pf"] == 2 * c["N"] and c["field"] == run and c["mixed_wells"] == 0 for c in one)
    assert all(c["spans"] == (1 if c["family"] == "one_class" else c["N"]) for c in one)
    # every key distinct: far more groups in a run than the LDS table holds, and a list longer than a chunk of rows
    (dist,) = fam("distinct")
    assert (dist["I"], dist["N"]) == (20, 9000) and dist["groups"] == dist["pf"] > 16 * LI_SLOTS
    assert dist["listed"] == dist["groups"] > dist["chunk"] > 0 and dist["mixed_wells"] == dist["spans"] > 1000
    # the edges: no PF well, less than a workgroup, every N % 4 with planes aligned and at odd addresses
    (none,) = fam("no_pf")
    assert none["pf"] == none["groups"] == none["listed"] == 0
    assert {c["N"] < 256 for c in fam("small")} == {True} and {c["unaligned"] for c in fam("small")} == {0, 1}
    assert {(c["N"] % 4, c["unaligned"]) for c in fam("tail")} == {(r, u) for r in (1, 2, 3) for u in (0, 1)}
    assert all(c["listed"] == c["groups"] for c in cases)              # (min_pf <= 1 lists every group)
    # the GPU tests' copy of li_home (tests/contention_inputs.py) against the kernel's own
    assert lines[0].startswith("homes: ")
    homes = [tuple(int(v) for v in pair.split("=")) for pair in lines[0].split()[1:]]
    assert len(homes) >= 16 and max(i for i, _ in homes) > 1 << 31
    assert li_home(np.array([i for i, _ in homes])).tolist() == [h for _, h in homes]


def test_a_torn_compare_and_swap_is_noticed(tmp_path):
    # plain: the claim of the lane's table alone (the __hip_atomic compare-and-swap of claim_or_join); =3: the LDS claim alone
    for define in ("-DWAVE_EMU_TORN_CAS", "-DWAVE_EMU_TORN_CAS=3"):
        exe = str(tmp_path / ("lane_index_emu_torn" + define[-1]))
        subprocess.check_call(["g++"] + FLAGS + [define, SRC, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
        assert out.returncode == 1 and "MISMATCH" in out.stdout, (define, out.returncode, out.stdout[-2000:], out.stderr[-2000:])
