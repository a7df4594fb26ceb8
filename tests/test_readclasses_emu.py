"""The lock-free class table (claim_or_join, csrc/read_classes.inc) run on the CPU under shuffled schedules:
tools/read_classes_emu.cpp compiles k_td_fingerprint / k_td_insert / k_td_resolve and k_ld_insert / k_ld_resolve /
k_ld_classes / k_ld_span_count as they stand, plays the 256 lanes of a workgroup with fibers (tools/wave_emu.h) and
lets the schedule hand over to another lane at every atomic - never, always, with probability 1/3 under eight seeds,
lanes in reverse, workgroups permuted.  Each schedule must give the definitions computed directly, and the same labels as every other.
The GPU tests see the few orders the hardware happens to produce; here the claims lost between a lane's load and its
compare-and-swap are counted, and a case whose schedules lose none has not tested what it is there for.  A second
build with a compare-and-swap broken on purpose (-DWAVE_EMU_TORN_CAS: a scheduling point between its load and its
store) must end in MISMATCH: the test can fail.  No GPU is involved; the emulation is sequentially consistent and says
nothing about caches or time."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
         "-I" + os.path.join(REPO, "include")]
SRC = os.path.join(REPO, "tools", "read_classes_emu.cpp")
LINE = re.compile(r"case (\d+) ok: path (\w+) kind (\w+) L (\d+) words (\d+) bits (\d+) order (\d) schedules (\d+) pf (\d+) "
                  r"classes (\d+) wrapped (\d+) points (\d+) never_lost (\d+) lost_table (\d+)")
NAMES = ("case", "path", "kind", "L", "words", "bits", "order", "schedules", "pf", "classes", "wrapped", "points",
         "never_lost", "lost_table")


def test_every_schedule_gives_the_definitions_classes(tmp_path):
    exe = str(tmp_path / "read_classes_emu")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "MISMATCH" not in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
    cases = [dict(zip(NAMES, (v if i in (1, 2) else int(v) for i, v in enumerate(row)))) for row in LINE.findall(out.stdout)]
    assert len(cases) == len(out.stdout.strip().split("\n")) >= 50
    # never, reverse, always and eight seeds at 1/3 per case; the schedule that never yields loses no compare-and-swap
    assert all(c["schedules"] == 11 and c["never_lost"] == 0 for c in cases)
    tile = [c for c in cases if c["path"] == "tile"]
    lane = [c for c in cases if c["path"] == "lane"]
    # the ground.  Planes of 1 .. 151 cycles: the ends of the 30-bit words and of compare_wells' 16-cycle blocks; rows
    # of 1, 2, 3 and 16 words; a mask of 2 bits (every tag collides: the reads decide) and none, with each of them
    fam_t = [c for c in tile if c["kind"] == "families"]
    fam_l = [c for c in lane if c["kind"] == "families"]
    assert {(c["L"], c["bits"]) for c in fam_t} == {(l, b) for l in (1, 10, 11, 16, 17, 151) for b in (2, 0)}
    assert {(c["words"], c["bits"], c["order"]) for c in fam_l} == {(w, b, o) for w in (1, 2, 3, 16) for b in (2, 0) for o in (0, 1)}
    for mine in (tile, lane):
        assert {c["kind"] for c in mine} == {"families", "chain_permuted", "chain_descending", "equal", "no_pf"}
        assert all(c["pf"] == 0 and c["classes"] == 0 for c in mine if c["kind"] == "no_pf")
        assert all(c["classes"] == (2 if mine is tile else 1) and c["pf"] > 500 for c in mine if c["kind"] == "equal")
    # what the families are for: every case loses claims, summed over its schedules at 1/3
    assert all(c["lost_table"] >= 1 for c in fam_t + fam_l)
    assert all(c["classes"] >= 300 for c in fam_t + fam_l if c["L"] >= 10)
    # a table of the host's size: probe paths that run past its end and go on at slot 0
    assert sum(c["wrapped"] for c in tile) > 0


def test_a_torn_compare_and_swap_is_noticed(tmp_path):
    exe = str(tmp_path / "read_classes_emu_torn")
    subprocess.check_call(["g++"] + FLAGS + ["-DWAVE_EMU_TORN_CAS", SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 1 and "MISMATCH" in out.stdout, (out.returncode, out.stdout[-2000:], out.stderr[-2000:])
