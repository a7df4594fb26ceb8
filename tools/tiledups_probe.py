#!/usr/bin/env python3
"""Read classes per tile (TileBatch.tile_dups, include/welldup_tiledups.h) beside what they sit next to, on
the same resident batch in the same process: every well of a full-size tile a centre, `--tiles` tiles;
wall clock per call (all are synchronous) of tile_dups, of the equality scan (TileBatch.count) and of the
duplicate sets (TileBatch.dup_sets minus the scan), and the rate of a kernel that only reads the planes
(Scanner.stream_read_gbs) - the fingerprint pass reads exactly those bytes once.  `--equal` adds one tile
whose reads are all equal (one slot of the table takes every well: the worst case).  For per-kernel
times run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/tiledups_probe.py

(the k_td_* rows of the stats are this stage, k_sets_* the sets stage, k_dense_* the scan)."""
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
ap.add_argument("--equal", action="store_true", help="also time one tile whose reads are all equal")
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


def line(what, best, mean, tiles):
    print("  %-12s best %8.3f ms  mean %8.3f ms  (%.4f ms per tile)" % (what, best, mean, best / tiles))


lv = a.levels
(rows, _), t_best, t_mean = timed(lambda: tb.tile_dups())
(blocks, _), c_best, c_mean = timed(lambda: tb.count(0, 0))
(b2, sets, _), s_best, s_mean = timed(lambda: tb.dup_sets(0, 0))
assert (b2 == blocks).all(), "dup_sets' out_tile differs from count's"
assert (rows[:, 4:4 + lv] == sets[:, 1 + lv:1 + 2 * lv]).all(), "Local differs from the sets' InSets at equality"
pf, in_classes = int(rows[:, 0].sum()), int(rows[:, 2].sum())
print("%d PF wells, %d classes, %d wells in them, tile duplication %.3f %%, local share at level %d %.2f %%"
      % (pf, int(rows[:, 1].sum()), in_classes, 100.0 * rows[:, 3].sum() / max(1, pf), lv,
         100.0 * rows[:, 4 + lv - 1].sum() / max(1, in_classes)))
line("tile_dups", t_best, t_mean, a.tiles)
line("count", c_best, c_mean, a.tiles)
line("dup_sets", s_best, s_mean, a.tiles)
print("  sets cost    best %8.3f ms  (%.4f ms per tile)" % (s_best - c_best, (s_best - c_best) / a.tiles))
plane_bytes = tb.plane_bytes
gbs = sc.stream_read_gbs(tb.d_planes, plane_bytes)
read_ms = plane_bytes / gbs / 1e6
print("  pure read of the planes: %.0f GB/s, %.3f ms (%.4f ms per tile); tile_dups / pure read = %.2f"
      % (gbs, read_ms, read_ms / a.tiles, t_best / read_ms))
tb.free()

if a.equal:
    one = TileBatch(sc, 1, a.bases, n)
    filt = np.ones(n, dtype=np.uint8)
    one.upload_tile(0, [np.full(n, 0x42 + (c % 4), dtype=np.uint8) for c in range(a.bases)], filt)
    (rows, _), e_best, e_mean = timed(lambda: one.tile_dups())
    assert rows[0, :4].tolist() == [n, 1, n, n - 1]
    print("every read equal, one tile:")
    line("tile_dups", e_best, e_mean, 1)
    one.free()
sc.close()
