"""The union-find of the duplicate sets (find_split / find_ro / unite and the seven k_sets_* kernels, csrc/dup_sets.inc)
run on the CPU under shuffled schedules: tools/dup_sets_emu.cpp compiles the kernels as they stand, plays the 256 lanes
of a workgroup with fibers (tools/wave_emu.h) and lets the schedule hand over to another lane at every atomic - the
relaxed loads and stores of the parent pointers among them -: never, always, with probability 1/3 under eight seeds,
lanes in reverse, workgroups permuted.  A case is a graph as a target table, filters and hit records; the kernels are
launched as wd_dup_sets launches them, in three ways: one pass over the batch with the records sorted by tile (a), the
same with the records shuffled (b: both paths of k_sets_union's hook counter), and tile by tile with tile0 = i (c: the
host's third path, which no GPU test reaches).  Every run must give the definitions computed directly - labels, PF,
Sets, InSets, Redundant, the size bins - and after every k_sets_union launch the roots must be exactly the PF wells less
the hooks counted so far: Redundant[l] is a count of successful compare-and-swaps, and the comment in the source that it
is the number of merges "whatever order the edges run in" is what this checks.  A case of a contended family whose
schedules lose no compare-and-swap has not tested what it is there for.  Further builds with a compare-and-swap broken
on purpose (-DWAVE_EMU_TORN_CAS: a scheduling point between its load and its store) must end in MISMATCH: the test can
fail.  No GPU is involved; the emulation is sequentially consistent and says nothing about caches or time."""
import os
import re
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-std=c++17",
         "-I" + os.path.join(REPO, "include")]
SRC = os.path.join(REPO, "tools", "dup_sets_emu.cpp")
LINE = re.compile(r"case (\d+) ok: family (\w+) levels (\d+) way (\w) schedules (\d+) records (\d+) wgs (\d+) ragged (\d) "
                  r"kept (\d+) merges (\d+) sets (\d+) flag (\d) lds_hooks (\d+) global_hooks (\d+) points (\d+) "
                  r"never_lost (\d+) lost (\d+)")
NAMES = ("case", "family", "levels", "way", "schedules", "records", "wgs", "ragged", "kept", "merges", "sets", "flag",
         "lds_hooks", "global_hooks", "points", "never_lost", "lost")
MAX_LEVELS = 32                                    # WD_MAX_LEVELS, include/welldup.h
GRAPHS = ("path_asc", "path_desc", "path_perm", "star_first", "star_last", "cliques", "gnm_low", "gnm_high")
TWO_LEVELS = ("ladder", "late_merge", "corners")   # an inner and an outer level: not with one level
BAD = ("bad_slot", "bad_tile", "bad_target", "bad_nbr")
CONTENDED = ("star_last", "path_desc", "gnm_high")


def test_every_schedule_and_way_gives_the_definitions_sets(tmp_path):
    exe = str(tmp_path / "dup_sets_emu")
    subprocess.check_call(["g++"] + FLAGS + [SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "MISMATCH" not in out.stdout, (out.stdout[-2000:], out.stderr[-2000:])
    rows = [dict(zip(NAMES, (v if i in (1, 3) else int(v) for i, v in enumerate(row)))) for row in LINE.findall(out.stdout)]
    assert len(rows) == len(out.stdout.strip().split("\n"))
    # never, reverse, always and eight seeds at 1/3 per case and way; the schedule that never yields loses no compare-and-swap
    assert all(r["schedules"] == 11 and r["never_lost"] == 0 for r in rows)
    # every family at 1, 3, 8 and the most levels there are (the bad records at 1 and 8), each in the three ways
    want = {(f, l) for f in GRAPHS for l in (1, 3, 8, MAX_LEVELS)} | {(f, l) for f in TWO_LEVELS for l in (3, 8, MAX_LEVELS)} | \
           {(f, l) for f in BAD for l in (1, 8)}
    assert {(r["family"], r["levels"], r["way"]) for r in rows} == {(f, l, w) for f, l in want for w in "abc"}
    assert len(rows) == 3 * len(want)
    for r in rows:
        # the records of a launch fill several workgroups and leave the last one ragged; unions happen and are counted
        assert r["wgs"] >= (3 if r["way"] == "c" else 6) and r["ragged"] == 1 and r["records"] > r["kept"] > 0, r
        assert r["merges"] > 0 and r["lds_hooks"] + r["global_hooks"] == 11 * r["merges"] and r["points"] > 0, r
        # records shuffled: workgroups of several tiles, both of k_sets_union's counters; tile by tile: the one in LDS alone
        if r["way"] == "b":
            assert r["lds_hooks"] > 0 and r["global_hooks"] > 0, r
        if r["way"] == "c":
            assert r["global_hooks"] == 0, r
        # records the targets cannot place raise the flag (the emulator: and change nothing else); no other case does
        assert r["flag"] == (1 if r["family"] in BAD else 0), r
        # what the contended families are for: compare-and-swaps lost, summed over the eight schedules at 1/3
        if r["family"] in CONTENDED:
            assert r["lost"] >= 1, r
    # the three ways of a case run the same graph
    for f, l in want:
        assert len({(r["records"], r["kept"], r["merges"], r["sets"]) for r in rows if (r["family"], r["levels"]) == (f, l)}) == 1
    # a star is one set per tile whose hub passes the filter (two of the three), a dense G(n, m) mostly one giant set
    assert all(r["sets"] == 2 for r in rows if r["family"].startswith("star"))
    assert all(r["merges"] > 3 * r["sets"] for r in rows if r["family"] == "gnm_high")


def test_a_torn_compare_and_swap_is_noticed_sets(tmp_path):
    # =2: torn in the compare-and-swaps tagged as a union-find's, which unite's hooks are; plain: in all of them
    for define in ("-DWAVE_EMU_TORN_CAS", "-DWAVE_EMU_TORN_CAS=2"):
        exe = str(tmp_path / ("dup_sets_emu_torn" + define[-1]))
        subprocess.check_call(["g++"] + FLAGS + [define, SRC, "-o", exe])
        out = subprocess.run([exe], capture_output=True, text=True, timeout=900)
        assert out.returncode == 1 and "MISMATCH" in out.stdout, (define, out.returncode, out.stdout[-2000:], out.stderr[-2000:])
