#!/usr/bin/env python3
"""Near-duplicate read clusters per tile (TileBatch.tile_near_dups, include/welldup_tilenear.h) beside what they
sit next to, on the same resident batch in the same process: every well of a full-size tile a centre, `--tiles`
tiles; wall clock per call (all are synchronous) of tile_near_dups for K = 1 and K = 2, of tile_dups, of the
equality scan (TileBatch.count) and of the duplicate sets (TileBatch.dup_sets), with NearPairs per K.
`--heavy` adds the case the pair budget is sized by: one small tile of `--heavy` distinct reads that share their
whole first segment (one chain of heavy * (heavy - 1) / 2 candidate pairs), and prints the pairs compared per
second.  For per-kernel times run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/tilenear_probe.py

in a run of its own (the k_tn_* rows of the stats are this stage, k_td_* the stage it shares with tile_dups)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from well_duplicates_amd import synth, workload                  # noqa: E402
from well_duplicates_amd.scanner import Scanner, TileBatch       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=workload.HISEQ4000_ROWS)
ap.add_argument("--cols", type=int, default=workload.HISEQ4000_COLS)
ap.add_argument("--levels", type=int, default=3)
ap.add_argument("--bases", type=int, default=150)
ap.add_argument("--tiles", type=int, default=16)
ap.add_argument("--plant", type=int, default=1311, help="planted wells per 65536 (1311 = 2 %%)")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--ks", default="1,2", help="distances to time")
ap.add_argument("--heavy", type=int, default=0, help="also time one chain of this many distinct reads (K = 1)")
a = ap.parse_args()

n = a.rows * a.cols
x, y = synth.honeycomb_pixels(a.rows, a.cols)
sc = Scanner(0)
T, P = sc.targets_from_coords(x, y, None, levels=a.levels)
spec = synth.SynthSpec(seed=5, n_clusters=n, row=a.cols, plant_per_64k=a.plant)
tb = TileBatch(sc, a.tiles, a.bases, n)
tb.fill_synthetic(spec, [(1, 1101 + i) for i in range(a.tiles)], list(range(a.bases)))
print("%d tiles of %d wells, %d levels (%.1f slots per well), %d bases, %.2f %% planted"
      % (a.tiles, n, a.levels, P / T, a.bases, 100.0 * a.plant / 65536))


def timed(fn, reps=a.reps):
    fn()                                             # warm-up: buffers, tables
    best, total = 1e30, 0.0
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        best, total = min(best, dt), total + dt
    return out, best * 1e3, total / reps * 1e3


def line(what, best, mean, tiles):
    print("  %-18s best %8.3f ms  mean %8.3f ms  (%.4f ms per tile)" % (what, best, mean, best / tiles))


lv = a.levels
(rows, _), t_best, t_mean = timed(lambda: tb.tile_dups())
pf = int(rows[:, 0].sum())
print("%d PF wells; by equality: %d classes, %d wells in them, tile duplication %.3f %%"
      % (pf, int(rows[:, 1].sum()), int(rows[:, 2].sum()), 100.0 * rows[:, 3].sum() / max(1, pf)))
line("tile_dups", t_best, t_mean, a.tiles)
for k in [int(v) for v in a.ks.split(",") if v]:
    (near, _), n_best, n_mean = timed(lambda: tb.tile_near_dups(k))
    assert (near[:, 0] == rows[:, 0]).all() and (near[:, 3] >= rows[:, 3]).all()
    line("tile_near_dups K=%d" % k, n_best, n_mean, a.tiles)
    print("    %d clusters, %d wells in them, %d near pairs, tile duplication %.3f %%, local share at level %d %.2f %%;"
          " %.2f x tile_dups" % (int(near[:, 1].sum()), int(near[:, 2].sum()), int(near[:, 4].sum()),
                                 100.0 * near[:, 3].sum() / max(1, pf), lv,
                                 100.0 * near[:, 5 + lv - 1].sum() / max(1, int(near[:, 2].sum())), n_best / t_best))
try:                                                 # the candidate pairs of tile 0's first segment: a budget of one pair
    tb.tile_near_dups(1, pair_budget=1)              # is refused with a message that names them
except RuntimeError as e:
    print("  with a pair budget of 1: %s" % e)
(blocks, _), c_best, c_mean = timed(lambda: tb.count(0, 0))
line("count", c_best, c_mean, a.tiles)
(b2, sets, _), s_best, s_mean = timed(lambda: tb.dup_sets(0, 0))
line("dup_sets", s_best, s_mean, a.tiles)
tb.free()

if a.heavy:
    rows_h, cols_h, L, m = 64, max(64, -(-a.heavy // 60)), 40, a.heavy
    nh = rows_h * cols_h
    xh, yh = synth.honeycomb_pixels(rows_h, cols_h)
    sc.targets_from_coords(xh, yh, None, levels=a.levels)
    rng = np.random.default_rng(1)
    reads = rng.integers(1, 256, (nh, L)).astype(np.uint8)
    heavy = rng.choice(nh, m, replace=False)
    reads[heavy, :L // 2] = reads[heavy[0], :L // 2]
    one = TileBatch(sc, 1, L, nh)
    one.upload_tile(0, [np.ascontiguousarray(reads[:, c]) for c in range(L)], np.ones(nh, dtype=np.uint8))
    pairs = m * (m - 1) // 2
    (near, _), h_best, h_mean = timed(lambda: one.tile_near_dups(1, pair_budget=2 * pairs), reps=3)
    (_, _), e_best, _ = timed(lambda: one.tile_dups(), reps=3)
    print("one chain of %d distinct reads (%d candidate pairs, %d wells, %d bases):" % (m, pairs, nh, L))
    line("tile_near_dups K=1", h_best, h_mean, 1)
    line("tile_dups", e_best, e_best, 1)
    print("    %.3g pairs per second (the chain's share of the call)" % (pairs / max(1e-9, (h_best - e_best) * 1e-3)))
    one.free()
sc.close()
