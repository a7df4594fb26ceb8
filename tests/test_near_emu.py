"""The union-find on labels (tn_find / tn_unite, csrc/near_core.inc) and the kernels around it, run on the CPU under
shuffled schedules: tools/near_emu.cpp compiles the kernels of csrc/tile_near.inc and csrc/lane_near.inc as they stand,
plays the 256 lanes of a workgroup with fibers (tools/wave_emu.h) and lets the schedule hand over to another lane at
every atomic - never, always, with probability 1/3 under eight seeds, lanes in reverse, workgroups permuted.  Each
schedule must give the definitions computed directly, and the same labels as every other.  The GPU tests see the few
orders the hardware happens to produce; here the retry loop of tn_unite and the lost compare-and-swaps of the table are
counted, and a case whose schedules lose none has not tested what it is there for.  A second build with a
compare-and-swap broken on purpose (-DWAVE_EMU_TORN_CAS: a scheduling point between its load and its store) must end
in MISMATCH: the test can fail.  No GPU is involved; the emulation is sequentially consistent and says nothing about
caches or time."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
         "-I" + os.path.join(REPO, "include")]
SRC = os.path.join(REPO, "tools", "near_emu.cpp")
LINE = re.compile(r"case (\d+) ok: path (\w+) kind (\w+) K (\d+) L (\d+) bits (\d+) schedules (\d+) classes (\d+) "
                  r"unions (\d+) near_pairs (\d+) long_slots (\d+) s32 (\d) s33 (\d) points (\d+) never_lost (\d+) "
                  r"lost_table (\d+) lost_union (\d+)")
NAMES = ("case", "path", "kind", "K", "L", "bits", "schedules", "classes", "unions", "near_pairs", "long_slots", "s32",
         "s33", "points", "never_lost", "lost_table", "lost_union")


def test_every_schedule_gives_the_definitions_clusters(tmp_path):
    exe = str(tmp_path / "near_emu")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "MISMATCH" not in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
    cases = [dict(zip(NAMES, (v if i in (1, 2) else int(v) for i, v in enumerate(row)))) for row in LINE.findall(out.stdout)]
    assert len(cases) == len(out.stdout.strip().split("\n")) >= 50
    # never, reverse, always and eight seeds at 1/3 per case; the schedule that never yields loses no compare-and-swap
    assert all(c["schedules"] == 11 and c["never_lost"] == 0 for c in cases)
    for path in ("tile", "lane"):
        mine = [c for c in cases if c["path"] == path]
        assert {c["kind"] for c in mine} == {"families", "chain_permuted", "chain_descending", "slots", "equal", "no_pf"}
        fam = [c for c in mine if c["kind"] == "families"]
        # the ground: every K with L = K + 1, 13, 21, 30 and 31 (segment ends inside a word, on its boundary, one past
        # it); masks of 1 bit, 4 bits and full with every K, and the mask of 1 bit at three different L
        assert {(c["K"], c["L"]) for c in fam} == {(k, l) for k in (1, 2, 3) for l in (k + 1, 13, 21, 30, 31)}
        assert {(c["K"], c["bits"]) for c in fam} == {(k, b) for k in (1, 2, 3) for b in (1, 4, 0)}
        assert len({c["L"] for c in fam if c["bits"] == 1}) == 3
        # what the families are for: hundreds of unions, and in every case compare-and-swaps lost in the table and in
        # the union-find, summed over the schedules at 1/3
        assert all(c["lost_table"] >= 1 and c["lost_union"] >= 1 for c in fam)
        assert sum(c["unions"] >= 150 for c in fam) >= 12
        # the chains: 99 unions per id space, each on a fresh root; both kinds with every K
        for kind in ("chain_permuted", "chain_descending"):
            chains = [c for c in mine if c["kind"] == kind]
            assert {c["K"] for c in chains} == {1, 2, 3}
            assert all(c["L"] >= 13 and c["unions"] >= 99 * (2 if path == "tile" else 1) for c in chains)
        # slots of exactly 32 vertices (the last a lane walks alone) and 33 (the first a wave takes), and a long one
        slots = [c for c in mine if c["kind"] == "slots"]
        assert {c["K"] for c in slots} == {1, 2, 3}
        assert all(c["s32"] == 1 and c["s33"] == 1 and c["long_slots"] >= 1 and c["bits"] == 0 for c in slots)
        assert all(c["classes"] == (2 if path == "tile" else 1) and c["unions"] == 0 for c in mine if c["kind"] == "equal")
        assert all(c["classes"] == 0 and c["points"] > 0 for c in mine if c["kind"] == "no_pf")
        assert any(c["long_slots"] > 0 for c in fam)


def test_a_torn_compare_and_swap_is_noticed(tmp_path):
    # =2: torn in the union-find alone (tn_unite's hook); plain: in the table's claim as well
    for define in ("-DWAVE_EMU_TORN_CAS", "-DWAVE_EMU_TORN_CAS=2"):
        exe = str(tmp_path / ("near_emu_torn" + define[-1]))
        subprocess.check_call(["g++"] + FLAGS + [define, SRC, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
        assert out.returncode == 1 and "MISMATCH" in out.stdout, (define, out.returncode, out.stdout[-2000:], out.stderr[-2000:])
