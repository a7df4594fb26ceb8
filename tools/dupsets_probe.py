#!/usr/bin/env python3
"""Duplicate sets against the plain scan on the same resident batch: every well of a full-size tile a
centre, `--tiles` tiles scanned by TileBatch.count and by TileBatch.dup_sets (include/welldup_sets.h), wall
clock per call (both are synchronous).  The difference is what the sets cost: the hit log the scan then
writes, and the k_sets_* kernels.  For per-kernel times run it under

    rocprofv3 --kernel-trace --stats -d <dir> -o run -- python tools/dupsets_probe.py

(the k_sets_* rows of the stats are the sets stage, k_dense_* the scan)."""
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
ap.add_argument("--modes", default="0:0,2:2", help="mode:k pairs (0 = equality, 1 = Hamming, 2 = Levenshtein)")
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


def timed(fn):
    fn()                                             # warm-up: buffers, tables, the hit log's size
    best, total = 1e30, 0.0
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        best, total = min(best, dt), total + dt
    return out, best * 1e3, total / a.reps * 1e3


for pair in a.modes.split(","):
    mode, k = (int(v) for v in pair.split(":"))
    (blocks, _), c_best, c_mean = timed(lambda: tb.count(mode, k))
    kernel = sc.last_kernel()
    (b2, rows, _), s_best, s_mean = timed(lambda: tb.dup_sets(mode, k))
    assert (b2 == blocks).all(), "dup_sets' out_tile differs from count's"
    lv = a.levels
    pf = int(rows[:, 0].sum())
    red = int(rows[:, 1 + 3 * lv - 1].sum())
    print("mode %d k %d (%s): %d edges, %d sets, exact duplication %.3f %%"
          % (mode, k, kernel, tb.edges, int(rows[:, lv].sum()), 100.0 * red / max(1, pf)))
    print("  count     best %8.3f ms  mean %8.3f ms  (%.4f ms per tile)" % (c_best, c_mean, c_best / a.tiles))
    print("  dup_sets  best %8.3f ms  mean %8.3f ms  (%.4f ms per tile)" % (s_best, s_mean, s_best / a.tiles))
    print("  sets cost best %8.3f ms  (%.4f ms per tile)" % (s_best - c_best, (s_best - c_best) / a.tiles))
tb.free()
sc.close()
