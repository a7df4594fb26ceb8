"""csrc/gen_rings.inc run on the CPU under shuffled schedules: tools/gen_rings_emu.cpp compiles k_gen_rings as it
stands, plays the 256 lanes of a workgroup with fibers (tools/wave_emu.h), launches the count pass, the host's prefix sum
and the fill pass as wd_targets_from_coords does, and lets the schedule hand over to another lane at every atomic -
never, always, with probability 1/3 under eight seeds, lanes in reverse, workgroups permuted.  The cases and their truth
are those of tests/genrings_cases.py, written into a small file each; every schedule must give the file's CSR or its
refusal.  The GPU sees the few slot orders the hardware happens to produce: here the order in which the lanes took
their LDS slots in the fill pass is counted, and the order and capacity cases must show slots out of index order -
otherwise the schedules did not test the ranking.  A second build whose atomic add is broken on purpose
(-DWAVE_EMU_TORN_ADD: two matches may take one slot) must end in MISMATCH at those cases: the test can fail.  The
emulator is a stand-alone program built with the address and undefined-behaviour sanitizers; no GPU is involved, and
the emulation is sequentially consistent and says nothing about caches or time."""
import os
import re
import subprocess

import numpy as np

import genrings_cases as gc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
         "-I" + os.path.join(REPO, "include")]
SRC = os.path.join(REPO, "tools", "gen_rings_emu.cpp")
NAMES = ("n", "T", "levels", "P", "status", "schedules", "never_descents", "descents", "orders", "unplaced", "points")
LINE = re.compile(r"case (\w+) ok: " + " ".join(r"%s (\d+)" % name for name in NAMES))
STATUS = {None: 0, "empty": 2, "capacity": 4}


def _constant(name):
    text = open(os.path.join(REPO, "well_duplicates_amd", "csrc", "gen_rings.inc")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def write_case(path, case):
    centre = np.array(gc.centres_of(case), dtype="<i4")
    parts = [np.array(case.max_dists, dtype="<i4"), case.x.astype("<i4"), case.y.astype("<i4"), centre]
    P = 0
    if case.want is not None:
        assert (case.want[0] == centre).all()
        parts += [case.want[1].astype("<i4").ravel(), case.want[2].astype("<i4")]
        P = case.want[2].shape[0]
    head = np.array([0x31435247, case.x.shape[0], centre.shape[0], case.centres is not None, case.levels,
                     STATUS[case.error], P], dtype="<i4")
    with open(path, "wb") as fh:
        for a in [head] + parts:
            fh.write(a.tobytes())


def _files(tmp_path):
    paths = []
    for case in gc.cases():
        paths.append(str(tmp_path / (case.name + ".grc")))
        write_case(paths[-1], case)
    return paths


def test_every_schedule_gives_the_reference_rings(tmp_path):
    assert (_constant("kGenWindow"), _constant("kGenMaxMatches")) == (gc.WINDOW, gc.CAPACITY)
    exe = str(tmp_path / "gen_rings_emu")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    out = subprocess.run([exe] + _files(tmp_path), capture_output=True, text=True, timeout=900)
    print(out.stdout)                                     # per case: the schedules run and the slots out of index order
    assert out.returncode == 0 and "MISMATCH" not in out.stdout, (out.stdout[-3000:], out.stderr[-3000:])
    rows = {row[0]: dict(zip(NAMES, (int(v) for v in row[1:]))) for row in LINE.findall(out.stdout)}
    assert list(rows) == [c.name for c in gc.cases()] and len(out.stdout.strip().split("\n")) == len(rows)
    for case in gc.cases():
        r = rows[case.name]
        assert (r["n"], r["T"], r["levels"]) == (case.x.shape[0], len(gc.centres_of(case)), case.levels)
        assert r["status"] == STATUS[case.error] and r["P"] == (0 if case.want is None else case.want[2].shape[0])
        # never, reverse, always and eight seeds at 1/3; every add of the fill pass was a match the reference knows
        assert r["schedules"] == 11 and r["unplaced"] == 0 and r["points"] > 0
    # what the ranking is for: slots out of index order under the shuffled schedules, and another order under every one
    for name in ("order", "capacity_2048", "capacity_2049", "capacity_2048_and_far", "several_centres"):
        assert rows[name]["descents"] >= 1000 and rows[name]["orders"] == 11, (name, rows[name])
    assert rows["jittered_honeycomb"]["descents"] >= 1000


def test_a_torn_slot_claim_is_noticed(tmp_path):
    exe = str(tmp_path / "gen_rings_emu_torn")
    subprocess.check_call(["g++"] + FLAGS + ["-DWAVE_EMU_TORN_ADD", SRC, "-o", exe])
    out = subprocess.run([exe] + _files(tmp_path), capture_output=True, text=True, timeout=900)
    print(out.stdout)
    assert out.returncode == 1, (out.returncode, out.stdout[-3000:], out.stderr[-3000:])
    failed = dict(re.findall(r"MISMATCH case (\w+) schedule \d+ \(\w+\): ([a-z_ ]+?) \d+:", out.stdout))
    # the count pass is whole in that build: the offsets are right, and a ring lacks the match whose slot was taken
    for name in ("order", "capacity_2048", "capacity_2048_and_far", "several_centres"):
        assert failed.get(name) == "nbr", (name, failed)
    assert failed.get("capacity_2049") == "status after the fill pass", failed       # (fewer slots taken than matches)
