#!/usr/bin/env python3
"""Read classes of a whole lane (scanner.LaneDups, include/welldup_lanedups.h) beside what they sit next to: a
lane of `--tiles` full-size tiles fed in batches of `--batch` through two TileBatches that take turns, as the
CLI streams a lane (the buffers of a batch are overwritten two batches later).  Wall clock per call (all are
synchronous), in the same process and on the same resident batches: LaneDups.add and, at the end,
LaneDups.finish; TileBatch.tile_dups; the equality scan (TileBatch.count); and the rate of a kernel that only
reads the planes (Scanner.stream_read_gbs) - k_ld_pack reads exactly those bytes once.  The tiles are those of
tools/tiledups_probe.py (seed 5, tiles 1101.., 2 % planted inside each tile), which share no read; with `--cross`
every odd tile repeats the tile before it but for the first cycle, so that a quarter of its wells have a
classmate there and the lane's table is joined as often as claimed.
`--equal` adds a lane of three tiles whose reads are all equal (one slot takes every well: the worst case).
`--hamming K` feeds a second accumulator the same batches and times LaneDups.finish(hamming=K) - the near-duplicate
clusters of the lane, include/welldup_lanenear.h - beside the equality finish, and TileBatch.tile_near_dups at the
same K beside tile_dups on every batch: the near finish less the equality finish is held against tile_near_dups
less tile_dups.  `--heavy M` adds a lane of four tiles with M distinct reads in all that share their first segment
(one bucket, M (M - 1) / 2 candidate pairs: the pair rate on packed rows).
`--index I [--libraries M]` times the lane's duplication per index read (include/welldup_laneindex.h): the lane is
streamed again into an accumulator with an index part of I cycles, once per case - M libraries of equal size, one
library (every counter on one row: the hottest case), and uniform random index reads (the most groups) - and
LaneDups.index_add per tile and LaneDups.index_finish are printed beside the equality add and finish on the same
batches.  With `--hops` LaneDups.hops (which libraries the lane's duplicate copies join, include/welldup_lanehops.h)
is timed per tile on each of the three, in the same process and on the same labels, beside index_finish, the equality
finish and LaneDups.mismatches(0): split I / 2 (a single index for I = 1), E = 1, the listing index_finish's first
1024 groups - on the lane of random index reads, where no group is large enough to be listed, 1024 keys that no well
carries, so that every pair searches the whole listing twice and lands in the one cell Other x Other.
`--hamming K --mismatches` times LaneDups.mismatches(K) (where the lane's duplicate copies differ,
include/welldup_lanemismatch.h) per tile of the lane beside the equality finish on the same batches, on three
inputs: the planted lane (after the near finish), the `--equal` lane (every well a pair of one root, every pair in
Dist[0]) and a lane of three tiles whose copies all differ from their original at one and the same cycle, by the
same substitution (one entry of Sub takes every add: the contended histogram entry).
`--distance [--radius R]` times LaneDups.distances (how far apart the lane's duplicate copies lie,
include/welldup_lanedistance.h) per tile of the lane beside the equality finish and LaneDups.mismatches on the same
batches and the same (equality) labels, on three inputs: the planted lane, the `--equal` lane (every pair on one root:
one bin and one root tile take every add of a wave) and a lane of three tiles whose wells of odd index all repeat
their left neighbour (everything in Dist[0] and Local).  The call includes the host's check, interleaving and upload
of the coordinates (8 bytes per well of a tile, once per call whatever the tiles): the kernel's own time is the
k_lg_tally row of the trace below, the rest of the call is that host part.
`--hamming K --quality` times the lane's reported base quality against its copies (include/welldup_lanequality.h):
LaneDups.qual_add per tile beside add on the same batches, and LaneDups.qualities(K) per tile beside mismatches(K) and
the equality finish, on three inputs: the planted lane (39 quality levels, the CLI's default bins), the `--equal` lane,
whose bases all carry one quality value (every well a profiled pair, every observation in one cell of Obs: the case the
counting inside a lane is there for), and the `--equal` lane with random qualities (every cell of Obs, no two
neighbouring cycles alike).
`--saturation [--steps S] [--radius R]` times LaneDups.saturation (the lane's distinct reads against its depth,
include/welldup_lanesaturation.h) per tile of the lane beside LaneDups.distances and the equality finish on the same
batches and labels, with the local copies within R dropped and without coordinates, on the three inputs of
`--distance`: the planted lane, the `--equal` lane (every pair's minimum goes to one word: what the read before the
atomic is for) and the lane whose odd wells repeat their left neighbour (with R every pair is dropped).  The call
includes the memset of its 4 bytes per well of the lane and the upload of the coordinates: the kernels' own times are
the k_ls_min and k_ls_tally rows of the trace below.
`--top N [--capacity C]` times LaneDups.top(N, C) (the lane's most frequent reads and their spread,
include/welldup_lanetop.h) per tile of the lane beside the equality finish and LaneDups.saturation (without coordinates)
on the same batches and labels, on three inputs: the planted lane, the `--equal` lane (one group holds every well: one
rank takes every add of k_lt_spread) and the lane whose odd wells repeat their left neighbour - classes of size 2 only,
the tie worst case; with `--capacity N` the selection there has to refine the root ids to the end, the longest it can
be.  The histogram passes taken are printed, and the bytes a pass streams (8 per well) over the time of a pass against
the pure read.
`--adapter [NAME]` times LaneDups.adapter (the lane's duplication by insert length, include/welldup_laneadapter.h; E 1, O
8) five times beside LaneDups.gc(0), the equality finish and a pure read of as many bytes as the pass reads - medians
and spreads of five -, on three inputs: the planted lane, the `--equal` lane, and a lane of three tiles whose every
read carries the adapter from a random cycle on (every search finds something).  Run it on the shipped library and,
with WELLDUP_LIB, on a `tools/build_variant.py ladnaive tiledups -DWD_LAD_NAIVE=1` build: the code-by-code search.
`--gc` times LaneDups.gc(0) (the lane's duplication against its reads' GC content, include/welldup_lanegc.h) per tile
of the lane beside the equality finish, LaneDups.mismatches(0) and LaneDups.top(100) on the same batches and labels,
and beside Scanner.stream_read_gbs over as many bytes as the pass reads - every packed row of the lane, label and
members: 4 ceil(cycles / 10) + 8 bytes per well -, on three inputs: the planted lane, the `--equal` lane (every well
of a wave on one bin of the histogram) and the lane whose odd wells repeat their left neighbour (pairs only: every
second well a root that adds its family's size).
`--hamming K --consensus [--max-family M]` times LaneDups.consensus(K, M) (the lane's errors against its families' vote,
include/welldup_laneconsensus.h) per tile of the lane beside LaneDups.mismatches(K) and the equality finish on the same
batches and labels, and beside Scanner.stream_read_gbs over 8 bytes per well - label and members, all that the
reservation and the scatter read of a lane without a voted family: their floor -, on three inputs: the planted lane
(after the near finish; its copies are mostly pairs, which do not vote), the `--equal` lane (one Large family: no list,
no vote) and a lane of three tiles whose wells repeat the first of every three (every well in a voted family of three:
the longest list there is).
`--umi U [--umi-e E] [--max-family M]` times LaneDups.umi_add per tile beside LaneDups.index_add of the same planes, and
LaneDups.umi(E, M) (the lane's duplicates split by molecular identifier, include/welldup_laneumi.h) per tile of the lane
beside LaneDups.consensus(0, M), the equality finish and Scanner.stream_read_gbs over 16 bytes per well - label, members
and the UMI keys: what the pass reads of a lane of pairs -, on three inputs: the planted lane (the UMI planes are U
further cycles of the same synthetic tiles: a planted copy carries its original's UMI), the `--equal` lane (one Large
family: counted, never looked into) and a lane of three tiles whose odd wells repeat their left neighbour, their UMI
too but for its last cycle (pairs only: k_lu_pairs does everything, a quarter of the pairs equal, the others one apart).
`--keep [--min-q Q]` times LaneDups.keep(Q) (the best well of each family as a keep mask, include/welldup_lanekeep.h) per
tile of the lane, with and without the masks, beside LaneDups.gc(0), LaneDups.qualities(0), the equality finish and
Scanner.stream_read_gbs over as many bytes as the pass reads - every quality row, label and members in k_lk_score, label,
members and the score in k_lk_mark: 4 ceil(cycles / 10) + 18 bytes per well -, on three inputs: the planted lane (a
planted copy carries its original's qualities: every family ties and its root stays, one atomic per family member),
the `--equal` lane with one quality and the `--equal` lane with random qualities (one family holds every well: the
case the grouping and the two skips of k_lk_score exist for).
`--umi U --keep --keep-umi` gives the three lanes of `--umi` a quality part too and times, on each, LaneDups.umi(E, M,
molecules=True) beside umi(E, M) - the same rows, and 8 bytes per well written (include/welldup_lanemolecules.h) - and
LaneDups.keep(Q, by_molecule=True) beside keep(Q): the same kernels on the molecules.
For per-kernel times run it under

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/lanedups_probe.py

(the k_ld_* rows of the stats are this stage, k_li_* the index part, k_lm_* the mismatch pass, k_lg_* the distance pass,
k_lq_* the quality part, k_ls_* the saturation pass, k_lt_* the top pass, k_lh_* the hops pass, k_lgc_* the GC pass, k_lad_* the adapter pass,
k_lc_* the consensus pass and the gather of the UMI pass, k_lu_* the UMI pass, k_lk_* the keep pass, k_td_* the per-tile classes, k_dense_* the scan)."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from well_duplicates_amd import synth, workload                  # noqa: E402
from well_duplicates_amd.scanner import LaneDups, Scanner, TileBatch       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=workload.HISEQ4000_ROWS)
ap.add_argument("--cols", type=int, default=workload.HISEQ4000_COLS)
ap.add_argument("--levels", type=int, default=3)
ap.add_argument("--cycles", type=int, default=150)
ap.add_argument("--tiles", type=int, default=32)
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--plant", type=int, default=1311, help="planted wells per 65536 inside a tile (1311 = 2 %%)")
ap.add_argument("--cross", action="store_true", help="every odd tile repeats the tile before it but for the first cycle")
ap.add_argument("--equal", action="store_true", help="also time a lane of three tiles whose reads are all equal")
ap.add_argument("--hamming", type=int, default=0, metavar="K", help="also time the near finish at Hamming distance <= K")
ap.add_argument("--heavy", type=int, default=0, metavar="M",
                help="also time a lane of M distinct reads that share their first segment (needs --hamming)")
ap.add_argument("--index", type=int, default=0, metavar="I", help="also time the index part with I index cycles (1..20)")
ap.add_argument("--libraries", type=int, default=96, metavar="M", help="libraries of the pooled lane (with --index)")
ap.add_argument("--hops", action="store_true",
                help="also time LaneDups.hops beside index_finish, the equality finish and mismatches(0) (needs --index)")
ap.add_argument("--mismatches", action="store_true",
                help="also time LaneDups.mismatches(K) beside the equality finish (needs --hamming; three inputs)")
ap.add_argument("--distance", action="store_true",
                help="also time LaneDups.distances beside the equality finish and mismatches (three inputs with --equal)")
ap.add_argument("--radius", type=int, default=2500, metavar="R", help="the radius of --distance and --saturation")
ap.add_argument("--saturation", action="store_true",
                help="also time LaneDups.saturation beside distances and the equality finish (three inputs with --equal)")
ap.add_argument("--steps", type=int, default=20, metavar="S", help="the steps of --saturation")
ap.add_argument("--top", type=int, default=0, metavar="N",
                help="also time LaneDups.top(N) beside the equality finish and saturation (three inputs with --equal)")
ap.add_argument("--capacity", type=int, default=0, metavar="C", help="the candidate capacity of --top (0: the default)")
ap.add_argument("--gc", action="store_true",
                help="also time LaneDups.gc(0) beside the equality finish, mismatches(0), top(100) and a pure read of as "
                     "many bytes (three inputs with --equal)")
ap.add_argument("--adapter", nargs="?", const="truseq", default=None, metavar="NAME",
                help="also time LaneDups.adapter (truseq, nextera, smallrna or 8..32 letters of ACGT; E 1, O 8) five times "
                     "beside gc(0), the equality finish and a pure read of as many bytes (three inputs with --equal)")
ap.add_argument("--consensus", action="store_true",
                help="also time LaneDups.consensus(K, M) beside mismatches(K), the equality finish and a pure read of "
                     "label and members (needs --hamming; three inputs with --equal)")
ap.add_argument("--max-family", type=int, default=256, metavar="M", help="the largest family of --consensus that votes")
ap.add_argument("--umi", type=int, default=0, metavar="U",
                help="also time LaneDups.umi_add beside index_add and LaneDups.umi(E, M) beside consensus(0, M), the "
                     "equality finish and a pure read of label, members and keys, with U UMI cycles (1..20; three inputs "
                     "with --equal)")
ap.add_argument("--umi-e", type=int, default=1, metavar="E", help="the differing cycles of --umi that are one molecule (0..3)")
ap.add_argument("--quality", action="store_true",
                help="also time LaneDups.qual_add beside add and LaneDups.qualities(K) beside mismatches(K) (needs "
                     "--hamming; three inputs with --equal)")
ap.add_argument("--keep", action="store_true",
                help="also time LaneDups.keep(Q) beside gc(0), qualities(0), the equality finish and a pure read of as many "
                     "bytes (three inputs with --equal)")
ap.add_argument("--keep-umi", action="store_true",
                help="with --umi U and --keep: also time LaneDups.umi(E, M, molecules=True) beside umi(E, M) and "
                     "LaneDups.keep(Q, by_molecule=True) beside keep(Q), on the three lanes of --umi")
ap.add_argument("--min-q", type=int, default=15, metavar="Q", help="the min_q of --keep (0..63)")
a = ap.parse_args()
if not 0 <= a.min_q <= 63:
    ap.error("--min-q takes 0..63")
if a.mismatches and not a.hamming:
    ap.error("--mismatches needs --hamming K")
if a.consensus and not a.hamming:
    ap.error("--consensus needs --hamming K")
if a.quality and not a.hamming:
    ap.error("--quality needs --hamming K")
if a.hops and not a.index:
    ap.error("--hops needs --index I")
if a.keep_umi and not (a.umi and a.keep):
    ap.error("--keep-umi needs --umi U and --keep")
if a.umi and not 1 <= a.umi <= 20:
    ap.error("--umi takes 1..20 cycles")
if not 0 <= a.umi_e <= 3:
    ap.error("--umi-e takes 0..3")
QUALITY_BINS = [0, 2, 10, 20, 25, 30, 35, 40]         # the CLI's default

n = a.rows * a.cols
x, y = synth.honeycomb_pixels(a.rows, a.cols)
sc = Scanner(0)
T, P = sc.targets_from_coords(x, y, None, levels=a.levels)
spec = synth.SynthSpec(seed=5, n_clusters=n, row=a.cols, plant_per_64k=a.plant)
ws = sc.lane_dups_workspace_bytes(n, a.tiles, a.cycles)
print("lane of %d tiles of %d wells, %d cycles, batches of %d; %.2f %% planted inside a tile%s; workspace %.2f GB"
      % (a.tiles, n, a.cycles, a.batch, 100.0 * a.plant / 65536,
         ", odd tiles repeat the tile before but for cycle 0" if a.cross else "", ws / 1e9))


def clock(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def fill(tb, tiles):
    """tools/tiledups_probe.py's tiles; with --cross every odd tile has the planes of the tile before it but for
    cycle 0, and a filter of its own: the wells whose first base happens to agree (a quarter) are copies"""
    for s, t in enumerate(tiles):
        own = 1101 + t
        base = own - 1 if (a.cross and t % 2) else own
        sc.synth_filter(tb.filter_ptr(s), spec, 1, own)
        for c in range(a.cycles):
            sc.synth_plane(tb.plane_ptr(s, c), spec, 1, own if c == 0 else base, c)
    sc.synchronize()


batches = [list(range(b0, min(a.tiles, b0 + a.batch))) for b0 in range(0, a.tiles, a.batch)]
tbs = [TileBatch(sc, a.batch, a.cycles, n), TileBatch(sc, a.batch, a.cycles, n)] if a.tiles else []
ld = LaneDups(sc, n, a.tiles, a.cycles)
ldn = LaneDups(sc, n, a.tiles, a.cycles) if a.hamming else None
if a.quality:
    print("quality part: workspace %.2f GB" % (sc.lane_qual_workspace_bytes(n, a.tiles, a.cycles) / 1e9))
    ldn.qual_begin(QUALITY_BINS)
t_add = t_td = t_cnt = t_read = t_tn = t_qadd = 0.0
read_gbs = []
td_pf = td_red = 0
for bi, tiles in enumerate(batches):
    tb = tbs[bi % 2]
    if len(tiles) != tb.n_tiles:                     # a short last batch
        tb = TileBatch(sc, len(tiles), a.cycles, n, reuse=tb)
        tbs[bi % 2] = tb
    fill(tb, tiles)
    if bi == 0:                                      # warm-up of every path, on a lane that is dropped
        warm = LaneDups(sc, n, len(tiles), a.cycles)
        warm.add(tb, list(range(len(tiles))))
        warm.finish()
        warm.close()
        tb.tile_dups()
        tb.count(0, 0)
        if a.hamming:
            warm = LaneDups(sc, n, len(tiles), a.cycles)
            if a.quality:
                warm.qual_begin(QUALITY_BINS)
                warm.qual_add(tb, list(range(len(tiles))))
            warm.add(tb, list(range(len(tiles))))
            warm.finish(hamming=a.hamming)
            warm.close()
            tb.tile_near_dups(a.hamming)
    _, dt = clock(lambda: ld.add(tb, tiles))
    t_add += dt
    if a.hamming:
        ldn.add(tb, tiles)
        if a.quality:
            _, dt = clock(lambda: ldn.qual_add(tb, tiles))
            t_qadd += dt
        _, dt = clock(lambda: tb.tile_near_dups(a.hamming))
        t_tn += dt
    (rows, _), dt = clock(lambda: tb.tile_dups())
    t_td += dt
    td_pf += int(rows[:, 0].sum())
    td_red += int(rows[:, 3].sum())
    _, dt = clock(lambda: tb.count(0, 0))
    t_cnt += dt
    gbs = sc.stream_read_gbs(tb.d_planes, tb.plane_bytes)
    read_gbs.append(gbs)
    t_read += tb.plane_bytes / gbs / 1e6
(lane, trow, _), t_fin = clock(lambda: ld.finish())


def time_distances(acc, tiles_n, t_finish, what):
    """LaneDups.distances and, on the same labels, LaneDups.mismatches(0), each after a first call that pays for
    loading the kernel; and the call without the matrix"""
    acc.distances(x, y, a.radius)
    dg, t_dg = clock(lambda: acc.distances(x, y, a.radius))
    _, t_dg0 = clock(lambda: acc.distances(x, y, a.radius, matrix=False))
    acc.mismatches(0)
    dm, t_dm = clock(lambda: acc.mismatches(0))
    row = dg[0]
    assert row[0] == dm[0][0] and row[3:].sum() == row[1] and (dg[1].sum(axis=0) == row[:3]).all(), "the rows do not add up"
    print("%s: distances, R = %d: %d pairs, %d on the root's tile, %d local; Dist %s; root tiles met per tile: %.1f"
          % (what, a.radius, row[0], row[1], row[2], " ".join(str(v) for v in row[3:]),
             float((dg[2] > 0).sum()) / max(1, tiles_n)))
    print("  %-22s %9.3f ms  (%.4f ms per tile; without the matrix %.4f; mismatches(0): %.4f; the equality finish: %.4f)"
          % ("lane distances", t_dg, t_dg / tiles_n, t_dg0 / tiles_n, t_dm / tiles_n, t_finish / tiles_n))
    return row


def time_saturation(acc, tiles_n, t_finish, what):
    """LaneDups.saturation with the local copies dropped and without coordinates, and on the same labels
    LaneDups.distances without the matrix, each after a first call that pays for loading the kernels"""
    acc.saturation(a.steps, 0, x, y, a.radius)
    sat, t_s = clock(lambda: acc.saturation(a.steps, 0, x, y, a.radius))
    plain, t_s0 = clock(lambda: acc.saturation(a.steps, 0))
    acc.distances(x, y, a.radius, matrix=False)
    dg, t_dg = clock(lambda: acc.distances(x, y, a.radius, matrix=False))
    head, reads, distinct = sat
    assert reads.sum() == head[0] - head[1] and head[1] == dg[0][2] and distinct.sum() == head[0] - dg[0][0] == plain[2].sum() \
        and plain[1].sum() == head[0], "the saturation rows do not add up"
    print("%s: saturation, %d steps, R = %d: %d PF wells, %d dropped, %d distinct; the last step: %d new of %d reads"
          % (what, a.steps, a.radius, head[0], head[1], distinct.sum(), distinct[-1], reads[-1]))
    print("  %-22s %9.3f ms  (%.4f ms per tile; without coordinates %.4f; distances without the matrix: %.4f; "
          "saturation / distances = %.2f; the equality finish: %.4f)"
          % ("lane saturation", t_s, t_s / tiles_n, t_s0 / tiles_n, t_dg / tiles_n, t_s / t_dg, t_finish / tiles_n))


def time_top(acc, tiles_n, t_finish, what):
    """LaneDups.top(N, C) and, on the same labels, LaneDups.saturation without coordinates, each after a first call
    that pays for loading the kernels; the time of a histogram pass is taken from the call with capacity N less the
    call with the default capacity, over the passes they differ by"""
    acc.top(a.top, a.capacity)
    top, t_t = clock(lambda: acc.top(a.top, a.capacity))
    passes = sc.get_option("lane_top_passes")
    full, t_full = clock(lambda: acc.top(a.top, a.top))
    full_passes = sc.get_option("lane_top_passes")
    one, t_one = clock(lambda: acc.top(a.top, 0))
    one_passes = sc.get_option("lane_top_passes")
    acc.saturation(a.steps, 0)
    sat, t_s = clock(lambda: acc.saturation(a.steps, 0))
    head, levels, root, size, exact, tile_count, reads = top
    assert levels[1].sum() == head[0] == sat[0][0] and levels[0].sum() == sat[2].sum() and (size == exact).all() \
        and (tile_count.sum(axis=1) == size).all() and all((f == t).all() for f, t in zip(full[:6], top[:6])) \
        and all((f == t).all() for f, t in zip(one[:6], top[:6])), "the top rows do not add up"
    print("%s: top %d, capacity %d: %d PF wells, %d groups, %d listed covering %d wells; sizes %s ...; levels %s"
          % (what, a.top, a.capacity, head[0], head[1], head[2], head[3], " ".join(str(v) for v in size[:5]),
             " ".join(str(v) for v in levels[0])))
    print("  %-22s %9.3f ms  (%.4f ms per tile, %d histogram passes of at most %d; capacity N: %.4f in %d passes; default: "
          "%.4f in %d; saturation without coordinates: %.4f; the equality finish: %.4f)"
          % ("lane top", t_t, t_t / tiles_n, passes, sc.get_option("lane_top_max_passes"), t_full / tiles_n, full_passes,
             t_one / tiles_n, one_passes, t_s / tiles_n, t_finish / tiles_n))
    if full_passes > one_passes:
        per_pass = (t_full - t_one) / (full_passes - one_passes)
        print("  a histogram pass: %.4f ms, %.1f us per tile: 8 bytes per well at %.0f GB/s (pure read: %.0f GB/s)"
              % (per_pass, 1e3 * per_pass / tiles_n, 8.0 * n * tiles_n / per_pass / 1e6, float(np.mean(read_gbs))))


def time_gc(acc, tiles_n, t_finish, what):
    """LaneDups.gc(0) and, on the same labels, LaneDups.mismatches(0) and LaneDups.top(100), each after a first call
    that pays for loading the kernels; and a pure read of as many bytes as the pass reads, from the accumulator's own
    workspace"""
    acc.gc(0)
    (grow, gtiles, ghist), t_g = clock(lambda: acc.gc(0))
    _, t_g2 = clock(lambda: acc.gc(a.cycles))
    acc.mismatches(0)
    mm, t_m = clock(lambda: acc.mismatches(0))
    acc.top(100)
    top, t_t = clock(lambda: acc.top(100))
    nbytes = tiles_n * n * (4 * ((a.cycles + 9) // 10) + 8)
    gbs = sc.stream_read_gbs(acc.d_ws, min(nbytes, acc.ws_bytes))
    t_read = nbytes / gbs / 1e6
    assert grow[0] == grow[1:4].sum() == top[0][0] and grow[3] == mm[0][0] and \
        ghist[:, 3].sum() + grow[7] == grow[2] + grow[3] and (ghist[:, :3].sum(axis=0) == grow[1:4] - grow[4:7]).all() and \
        gtiles[:, 0].sum() == grow[0], "the gc rows do not add up"
    g = np.arange(ghist.shape[0])
    print("%s: gc, max_n 0: %d PF wells, %d single, %d roots, %d copies, %d skipped; %d values of g taken, mean GC of the "
          "distinct molecules %.4f, of the copies %.4f"
          % (what, grow[0], grow[1], grow[2], grow[3], grow[4:7].sum(), int((ghist[:, :3].sum(axis=1) > 0).sum()),
             (g * (ghist[:, 0] + ghist[:, 1])).sum() / max(1, (ghist[:, 0] + ghist[:, 1]).sum()) / a.cycles,
             (g * ghist[:, 2]).sum() / max(1, ghist[:, 2].sum()) / a.cycles))
    print("  %-22s %9.3f ms  (%.4f ms per tile; max_n = L: %.4f; %.1f MB per tile at %.0f GB/s; a pure read of as many bytes: "
          "%.4f ms per tile at %.0f GB/s; gc / read = %.2f; mismatches(0): %.4f; top(100): %.4f; the equality finish: %.4f)"
          % ("lane gc", t_g, t_g / tiles_n, t_g2 / tiles_n, nbytes / tiles_n / 1e6, nbytes / t_g / 1e6, t_read / tiles_n, gbs,
             t_g / t_read, t_m / tiles_n, t_t / tiles_n, t_finish / tiles_n))


def time_adapter(acc, tiles_n, t_finish, what):
    """LaneDups.adapter(codes, 1, 8) five times and LaneDups.gc(0) five times on the same labels, each after a first
    call that pays for loading the kernels - the medians and the spread (max - min) of the five -, and a pure read of as
    many bytes as the pass reads, from the accumulator's own workspace"""
    from well_duplicates_amd.lane_passes import parse_adapter
    name, codes = parse_adapter(a.adapter)
    acc.adapter(codes, 1, 8)
    runs = [clock(lambda: acc.adapter(codes, 1, 8)) for _ in range(5)]
    acc.gc(0)
    t_gs = sorted(clock(lambda: acc.gc(0))[1] for _ in range(5))
    t_as = sorted(t for _, t in runs)
    t_a, t_g = t_as[2], t_gs[2]
    row, tiles, hist = runs[0][0]
    nbytes = tiles_n * n * (4 * ((a.cycles + 9) // 10) + 8)
    gbs = sc.stream_read_gbs(acc.d_ws, min(nbytes, acc.ws_bytes))
    t_read = nbytes / gbs / 1e6
    assert all((r[0] == row).all() and (r[1] == tiles).all() and (r[2] == hist).all() for r, _ in runs), "the runs differ"
    assert row[0] == row[1:4].sum() == tiles[:, 0].sum() and (hist[:, :3].sum(axis=0) == row[1:4]).all() and \
        (hist[:-1, :3].sum(axis=0) == row[4:7]).all() and hist[:, 3].sum() == row[2] + row[3] and \
        tiles[:, 4].sum() == (np.arange(a.cycles) * hist[:-1, :3].sum(axis=1)).sum(), "the adapter rows do not add up"
    print("%s: adapter %s, E 1, O 8: %d PF wells, %d single, %d roots, %d copies; with adapter %d, inexact %d, partial %d; "
          "%d values of a taken" % (what, name, row[0], row[1], row[2], row[3], row[4:7].sum(), row[8], row[9],
                                    int((hist[:-1, :3].sum(axis=1) > 0).sum())))
    print("  %-22s %9.3f ms  (median of five, spread %.3f; %.4f ms per tile; %.1f MB per tile at %.0f GB/s; a pure read of as "
          "many bytes: %.4f ms per tile at %.0f GB/s; adapter / read = %.2f; gc(0): %.4f ms per tile, median of five, spread "
          "%.3f ms; adapter / gc = %.2f; the equality finish: %.4f)"
          % ("lane adapter", t_a, t_as[-1] - t_as[0], t_a / tiles_n, nbytes / tiles_n / 1e6, nbytes / t_a / 1e6,
             t_read / tiles_n, gbs, t_a / t_read, t_g / tiles_n, t_gs[-1] - t_gs[0], t_a / t_g, t_finish / tiles_n))


def time_consensus(acc, tiles_n, t_finish, what):
    """LaneDups.consensus(K, M) and, on the same labels, LaneDups.mismatches(K), each after a first call that pays for
    loading the kernels; and a pure read of 8 bytes per well, from the accumulator's own workspace"""
    acc.consensus(a.hamming, a.max_family)
    (crow, ctiles, calls), t_c = clock(lambda: acc.consensus(a.hamming, a.max_family))
    _, t_c0 = clock(lambda: acc.consensus(0, a.max_family))
    acc.mismatches(a.hamming)
    mm, t_m = clock(lambda: acc.mismatches(a.hamming))
    nbytes = tiles_n * n * 8
    gbs = sc.stream_read_gbs(acc.d_ws, min(nbytes, acc.ws_bytes))
    t_read = nbytes / gbs / 1e6
    assert crow[11:].sum() == crow[1] and calls.sum() == crow[2] * a.cycles - crow[6] and \
        (ctiles.sum(axis=0) == crow[1:5]).all() and 2 * crow[8] + crow[1] + crow[10] == mm[0][0] + crow[8] + crow[0] + crow[9], \
        "the consensus rows do not add up"
    print("%s: consensus, max_d %d, max_family %d: %d families of %d wells, %d profiled, %d mismatches (%d with N), %d "
          "undecided, %d first wells off; %d pairs and %d large families of %d wells left out; Dist %s"
          % (what, a.hamming, a.max_family, crow[0], crow[1], crow[2], crow[3], crow[4], crow[5], crow[7], crow[8], crow[9],
             crow[10], " ".join(str(v) for v in crow[11:])))
    print("  %-22s %9.3f ms  (%.4f ms per tile; max_d 0: %.4f; a pure read of label and members, 8 bytes per well: %.4f ms "
          "per tile at %.0f GB/s; consensus / read = %.2f; mismatches(%d): %.4f; consensus / mismatches = %.2f; the "
          "equality finish: %.4f)"
          % ("lane consensus", t_c, t_c / tiles_n, t_c0 / tiles_n, t_read / tiles_n, gbs, t_c / t_read, a.hamming,
             t_m / tiles_n, t_c / t_m, t_finish / tiles_n))


def time_qualities(acc, tiles_n, t_finish, t_qual_add, t_plain_add, what):
    """LaneDups.qualities(K) and, on the same labels, LaneDups.mismatches(K), each after a first call that pays for
    loading the kernel"""
    acc.qualities(a.hamming)
    q, t_q = clock(lambda: acc.qualities(a.hamming))
    acc.mismatches(a.hamming)
    m, t_m = clock(lambda: acc.mismatches(a.hamming))
    row = q[0]
    assert (row[[0, 1, 3]] == m[0][:3]).all() and q[3].sum() == row[2] == row[1] * a.cycles and q[4].sum() == row[3], \
        "the quality rows do not add up"
    print("%s: qualities, max_d %d: %d pairs, %d profiled, %d observations in %d cells of Obs (the fullest holds %.4f), "
          "%d mismatches in %d cells of Mis; %d quality values seen"
          % (what, a.hamming, row[0], row[1], row[2], int((q[3] > 0).sum()), q[3].max() / max(1, row[2]), row[3],
             int((q[4] > 0).sum()), int((q[2] > 0).sum())))
    print("  %-22s %9.3f ms  (%.4f ms per tile; add: %.4f; qual_add / add = %.2f)"
          % ("lane qual_add", t_qual_add, t_qual_add / tiles_n, t_plain_add / tiles_n, t_qual_add / t_plain_add))
    print("  %-22s %9.3f ms  (%.4f ms per tile; mismatches(%d): %.4f; qualities / mismatches = %.2f; the equality finish: "
          "%.4f)" % ("lane qualities", t_q, t_q / tiles_n, a.hamming, t_m / tiles_n, t_q / t_m, t_finish / tiles_n))


if a.distance:
    time_distances(ld, max(1, a.tiles), t_fin, "the planted lane")
if a.saturation:
    time_saturation(ld, max(1, a.tiles), t_fin, "the planted lane")
if a.top:
    time_top(ld, max(1, a.tiles), t_fin, "the planted lane")
if a.gc:
    time_gc(ld, max(1, a.tiles), t_fin, "the planted lane")
if a.adapter:
    time_adapter(ld, max(1, a.tiles), t_fin, "the planted lane")
ld.close()
if a.hamming:
    near, t_near = clock(lambda: ldn.finish(hamming=a.hamming))
    if a.mismatches:
        ldn.mismatches(a.hamming)                    # (the first call of a kernel pays for loading it)
        mm, t_mm = clock(lambda: ldn.mismatches(a.hamming))
        assert mm[0][0] == near[3][3] and mm[0][4:].sum() == mm[0][0], "Pairs is not the near finish's Redundant"
    if a.quality:
        time_qualities(ldn, max(1, a.tiles), t_fin, t_qadd, t_add, "the planted lane")
    if a.consensus:
        time_consensus(ldn, max(1, a.tiles), t_fin, "the planted lane")
    ldn.close()
    assert (near[0] == lane).all() and (near[1] == trow).all(), "the near finish delivers other classes"
for tb in tbs:
    tb.free()

k = max(1, a.tiles)
wells = lane[0]
print("%d PF wells, %d classes (%d across tiles), %d wells in them; lane duplication %.3f %% (within tiles %d, across "
      "tiles %d); the tiles one by one: %.3f %%" % (wells, lane[1], lane[4], lane[2], 100.0 * lane[3] / max(1, wells),
                                                   lane[2] - lane[5], lane[5] - lane[1], 100.0 * td_red / max(1, td_pf)))
assert trow[:, 3].sum() == td_red and wells == td_pf, "TileRedundant differs from tile_dups' Redundant"
print("  %-22s %9.3f ms  (%.4f ms per tile, %.2f G wells/s)" % ("lane_dups add", t_add, t_add / k, a.tiles * n / t_add / 1e6))
print("  %-22s %9.3f ms  (%.4f ms per tile)" % ("lane_dups finish", t_fin, t_fin / k))
print("  %-22s %9.3f ms  (%.4f ms per tile)" % ("add + finish", t_add + t_fin, (t_add + t_fin) / k))
print("  %-22s %9.3f ms  (%.4f ms per tile)" % ("tile_dups", t_td, t_td / k))
print("  %-22s %9.3f ms  (%.4f ms per tile)" % ("count", t_cnt, t_cnt / k))
print("  %-22s %9.3f ms  (%.4f ms per tile, %.0f GB/s)" % ("pure read of the planes", t_read, t_read / k,
                                                            float(np.mean(read_gbs)) if read_gbs else 0.0))
print("  (add + finish) / tile_dups = %.2f; add / pure read = %.2f" % ((t_add + t_fin) / t_td, t_add / t_read))

if a.hamming:
    nl = near[3]
    print("Hamming <= %d: %d clusters (%d across tiles), %d wells in them, %d near pairs of distinct reads; lane duplication "
          "%.3f %% (by equality %.3f %%)" % (a.hamming, nl[1], nl[4], nl[2], nl[6], 100.0 * nl[3] / max(1, wells),
                                             100.0 * lane[3] / max(1, wells)))
    print("  %-22s %9.3f ms  (%.4f ms per tile)" % ("lane near finish", t_near, t_near / k))
    print("  %-22s %9.3f ms  (%.4f ms per tile)" % ("  less the finish", t_near - t_fin, (t_near - t_fin) / k))
    print("  %-22s %9.3f ms  (%.4f ms per tile)" % ("tile_near_dups", t_tn, t_tn / k))
    print("  %-22s %9.3f ms  (%.4f ms per tile)" % ("  less tile_dups", t_tn - t_td, (t_tn - t_td) / k))
    print("  (near finish - finish) / (tile_near_dups - tile_dups) = %.2f" % ((t_near - t_fin) / (t_tn - t_td)))

if a.mismatches:
    row = mm[0]
    print("mismatches, max_d %d: %d pairs, %d profiled, %d mismatches (%d with N); Dist %s"
          % (a.hamming, row[0], row[1], row[2], row[3], " ".join(str(v) for v in row[4:])))
    print("  %-22s %9.3f ms  (%.4f ms per tile; the equality finish: %.4f)" % ("lane mismatches", t_mm, t_mm / k, t_fin / k))

if a.heavy and a.hamming:
    m4 = (a.heavy + 3) // 4
    rng = np.random.default_rng(7)
    head = (a.cycles + a.hamming) // (a.hamming + 1)                    # covers the first segment
    four = TileBatch(sc, 4, a.cycles, m4)
    for s in range(4):
        reads = rng.integers(1, 256, (m4, a.cycles)).astype(np.uint8)
        reads[:, :head] = 0x41
        four.upload_tile(s, [np.ascontiguousarray(reads[:, c]) for c in range(a.cycles)], np.ones(m4, dtype=np.uint8))
    pairs = 4 * m4 * (4 * m4 - 1) // 2
    times = []
    for hamming in (0, a.hamming, 0, a.hamming):
        hv = LaneDups(sc, m4, 4, a.cycles)
        hv.add(four, [0, 1, 2, 3])
        got, dt = clock(lambda: hv.finish(hamming=hamming, pair_budget=pairs if hamming else 0))
        hv.close()
        times.append(dt)
    assert got[0][1] == 0, "the heavy lane's reads are not distinct"
    dt = times[3] - times[2]
    print("heavy: %d distinct reads on four tiles share cycles 0..%d: %d candidate pairs; finish %.3f ms, near finish "
          "%.3f ms: %.3g pairs per second" % (4 * m4, head - 1, pairs, times[2], times[3], pairs / (dt * 1e-3)))
    four.free()

if a.index:
    I = a.index
    iws = sc.lane_index_workspace_bytes(n, a.tiles, I)
    print("index part: %d index cycles, workspace %.2f GB" % (I, iws / 1e9))
    rng = np.random.default_rng(11)
    tb, itb = TileBatch(sc, a.batch, a.cycles, n), TileBatch(sc, a.batch, I, n)
    for name, m in (("%d libraries of equal size" % a.libraries, a.libraries), ("one library", 1), ("random index reads", 0)):
        lib = rng.integers(1, 256, (max(1, m), I)).astype(np.uint8)
        li = LaneDups(sc, n, a.tiles, a.cycles)
        li.index_begin(I)
        i_add = i_iadd = 0.0
        for tiles in batches:
            if len(tiles) != tb.n_tiles:
                tb, itb = TileBatch(sc, len(tiles), a.cycles, n, reuse=tb), TileBatch(sc, len(tiles), I, n, reuse=itb)
            fill(tb, tiles)
            for s_ in range(len(tiles)):
                reads = lib[rng.integers(0, m, n)] if m else rng.integers(1, 256, (n, I)).astype(np.uint8)
                for c in range(I):
                    sc.h2d(itb.plane_ptr(s_, c), np.ascontiguousarray(reads[:, c]))
            _, dt = clock(lambda: li.add(tb, tiles))
            i_add += dt
            _, dt = clock(lambda: li.index_add(itb, tiles))
            i_iadd += dt
        (ilane, _, _), i_fin = clock(lambda: li.finish())
        pf = int(ilane[0])
        (irow, other, rows, ikeys), i_ifin = clock(lambda: li.index_finish(max(1, -(-pf // 1000)), 1001))
        _, i_again = clock(lambda: li.index_finish(max(1, -(-pf // 1000)), 1001))
        if a.hops:
            listed = ikeys[:1024]
            if listed.size == 0:                     # keys that begin with N, which no generated index read does
                digits = min(I - 1, 5)
                listed = np.array([4 | sum(((i >> (2 * d)) & 3) << (3 * (d + 1)) for d in range(digits))
                                   for i in range(4 ** digits)], dtype=np.uint64)
            split = max(1, I // 2)
            li.hops(split, 1, listed)                # (the first call of a kernel pays for loading it)
            hp, t_hp = clock(lambda: li.hops(split, 1, listed))
            li.mismatches(0)
            hm, t_hm = clock(lambda: li.mismatches(0))
            assert hp[0][0] == hm[0][0] == ilane[3] and hp[0][4:].sum() == hp[0][0] == hp[2].sum(), "the hops rows do not add up"
            print("  %-22s %9.3f ms  (%.4f ms per tile; mismatches(0): %.4f; hops / mismatches = %.2f; index_finish: %.4f; "
                  "the equality finish: %.4f)" % ("lane hops", t_hp, t_hp / k, t_hm / k, t_hp / t_hm, i_ifin / k, i_fin / k))
            print("    split %d, E 1, %d listed: %d pairs, %d on the root's tile, one index read swapped %d, both %d; State %s; "
                  "%d cells of the matrix occupied" % (split, listed.size, hp[0][0], hp[0][1], hp[0][2], hp[0][3],
                                                       " ".join(str(v) for v in hp[0][4:]), int((hp[2] > 0).sum())))
        li.close()
        assert rows[:, 0].sum() + other[0] == pf and (ilane[:4] == lane[:4]).all(), "the index rows do not add up"
        print("%s: %d groups, %d listed, %d mixed classes of %d" % (name, irow[0], irow[1], irow[3], ilane[1]))
        print("  %-22s %9.3f ms  (%.4f ms per tile)" % ("lane_dups add", i_add, i_add / k))
        print("  %-22s %9.3f ms  (%.4f ms per tile; add x I / L = %.4f)" % ("index_add", i_iadd, i_iadd / k,
                                                                          i_add / k * I / a.cycles))
        print("  %-22s %9.3f ms  (%.4f ms per tile)" % ("lane_dups finish", i_fin, i_fin / k))
        print("  %-22s %9.3f ms  (%.4f ms per tile; again, the listing only: %.3f ms)" % ("index_finish", i_ifin, i_ifin / k,
                                                                                        i_again))
    tb.free()
    itb.free()

if a.equal:
    three = TileBatch(sc, 3, a.cycles, n)
    for s in range(3):
        three.upload_tile(s, [np.full(n, 0x42 + (c % 4), dtype=np.uint8) for c in range(a.cycles)], np.ones(n, dtype=np.uint8))
    eq = LaneDups(sc, n, 3, a.cycles)
    if a.quality:
        eq.qual_begin(QUALITY_BINS)
    _, e_add = clock(lambda: eq.add(three, [0, 1, 2]))
    if a.quality:
        _, e_qadd = clock(lambda: eq.qual_add(three, [0, 1, 2]))
    (lane, trow, _), e_fin = clock(lambda: eq.finish())
    assert lane[:6].tolist() == [3 * n, 1, 3 * n, 3 * n - 1, 1, 3]
    print("every read equal, three tiles: add %.3f ms, finish %.3f ms" % (e_add, e_fin))
    if a.mismatches:
        eq.mismatches(a.hamming)
        em, e_mm = clock(lambda: eq.mismatches(a.hamming))
        assert em[0].tolist() == [3 * n - 1, 3 * n - 1, 0, 0, 3 * n - 1] + [0] * 8
        print("  %-22s %9.3f ms  (%.4f ms per tile; the equality finish: %.4f)" % ("lane mismatches", e_mm, e_mm / 3, e_fin / 3))
    if a.distance:
        row = time_distances(eq, 3, e_fin, "every read equal, three tiles")
        assert row[:2].tolist() == [3 * n - 1, n - 1], "the equal lane's pairs are not all on well 0 of tile 0"
    if a.saturation:
        time_saturation(eq, 3, e_fin, "every read equal, three tiles")
    if a.top:
        time_top(eq, 3, e_fin, "every read equal, three tiles")
    if a.gc:
        time_gc(eq, 3, e_fin, "every read equal, three tiles")
    if a.adapter:
        time_adapter(eq, 3, e_fin, "every read equal, three tiles")
    if a.consensus:
        time_consensus(eq, 3, e_fin, "every read equal, three tiles")
    if a.quality:
        time_qualities(eq, 3, e_fin, e_qadd, e_add, "every read equal, one quality value, three tiles")
        # the same bases under random qualities 1..63: eight random planes take turns
        rng = np.random.default_rng(13)
        pool = [rng.integers(1, 64, n).astype(np.uint8) << 2 for _ in range(8)]
        for s in range(3):
            for c in range(a.cycles):
                sc.h2d(three.plane_ptr(s, c), pool[(3 * s + c) % 8] | np.uint8((0x42 + c % 4) & 3))
        sc.synchronize()
        rq = LaneDups(sc, n, 3, a.cycles)
        rq.qual_begin(QUALITY_BINS)
        _, r_add = clock(lambda: rq.add(three, [0, 1, 2]))
        _, r_qadd = clock(lambda: rq.qual_add(three, [0, 1, 2]))
        _, r_fin = clock(lambda: rq.finish())
        time_qualities(rq, 3, r_fin, r_qadd, r_add, "every read equal, random qualities, three tiles")
        rq.close()
    eq.close()
    three.free()

if a.consensus:
    # three tiles without planted copies whose wells 3 j + 1 and 3 j + 2 repeat well 3 j, cycle by cycle: triples only
    bare = synth.SynthSpec(seed=5, n_clusters=n, row=a.cols, plant_per_64k=0)
    three = TileBatch(sc, 3, a.cycles, n)
    for s in range(3):
        sc.h2d(three.filter_ptr(s), np.ones(n, dtype=np.uint8))
        for c in range(a.cycles):
            sc.synth_plane(three.plane_ptr(s, c), bare, 1, 1101 + s, c)
            sc.synchronize()
            plane = sc.d2h(three.plane_ptr(s, c), n, np.uint8).copy()
            first = plane[0::3]
            plane[1::3] = first[:plane[1::3].size]
            plane[2::3] = first[:plane[2::3].size]
            sc.h2d(three.plane_ptr(s, c), plane)
    sc.synchronize()
    tr = LaneDups(sc, n, 3, a.cycles)
    tr.add(three, [0, 1, 2])
    _, tr_fin = clock(lambda: tr.finish())
    time_consensus(tr, 3, tr_fin, "every well one of three equal wells, three tiles")
    assert tr.consensus(0, a.max_family)[0][0] >= 3 * (n // 3), "the wells are not triples"
    tr.close()
    three.free()
if a.mismatches:
    # tile 0: the planted tile 1101 with G at cycle `at` of every well; tiles 1 and 2: the same with T there
    at = a.cycles // 2
    three = TileBatch(sc, 3, a.cycles, n)
    for s in range(3):
        sc.h2d(three.filter_ptr(s), np.ones(n, dtype=np.uint8))
        for c in range(a.cycles):
            if c == at:
                sc.h2d(three.plane_ptr(s, c), np.full(n, 0x42 if s == 0 else 0x43, dtype=np.uint8))
            else:
                sc.synth_plane(three.plane_ptr(s, c), spec, 1, 1101, c)
    sc.synchronize()
    one = LaneDups(sc, n, 3, a.cycles)
    one.add(three, [0, 1, 2])
    (_, _, _, onear, _, _), o_near = clock(lambda: one.finish(hamming=1))
    one.mismatches(1)
    om, o_mm = clock(lambda: one.mismatches(1))
    assert om[0][5] >= 2 * n and om[2][at, 2, 3] >= 2 * n, "the copies are not one cycle from their originals"
    print("every copy G>T at cycle %d of its original, three tiles: %d pairs, %d of them at distance 1, Sub[%d][G][T] = %d; "
          "near finish %.3f ms" % (at, om[0][0], om[0][5], at, om[2][at, 2, 3], o_near))
    print("  %-22s %9.3f ms  (%.4f ms per tile)" % ("lane mismatches", o_mm, o_mm / 3))
    one.close()
    three.free()
if a.distance or a.saturation or a.top or a.gc:
    # three tiles without planted copies whose wells of odd index repeat the well to their left, cycle by cycle
    bare = synth.SynthSpec(seed=5, n_clusters=n, row=a.cols, plant_per_64k=0)
    three = TileBatch(sc, 3, a.cycles, n)
    for s in range(3):
        sc.h2d(three.filter_ptr(s), np.ones(n, dtype=np.uint8))
        for c in range(a.cycles):
            sc.synth_plane(three.plane_ptr(s, c), bare, 1, 1101 + s, c)
            sc.synchronize()
            plane = sc.d2h(three.plane_ptr(s, c), n, np.uint8).copy()
            plane[1::2] = plane[0::2][:plane[1::2].size]
            sc.h2d(three.plane_ptr(s, c), plane)
    sc.synchronize()
    nb = LaneDups(sc, n, 3, a.cycles)
    nb.add(three, [0, 1, 2])
    (nlane, _, _), n_fin = clock(lambda: nb.finish())
    if a.distance:
        row = time_distances(nb, 3, n_fin, "every odd well a copy of its left neighbour, three tiles")
        assert row[0] >= 3 * (n // 2) and row[3] >= 0.99 * row[1], "the copies do not sit beside their originals"
    if a.saturation:
        time_saturation(nb, 3, n_fin, "every odd well a copy of its left neighbour, three tiles")
    if a.top:
        time_top(nb, 3, n_fin, "every odd well a copy of its left neighbour, three tiles")
    if a.gc:
        time_gc(nb, 3, n_fin, "every odd well a copy of its left neighbour, three tiles")
    nb.close()
    three.free()
if a.adapter:
    # three tiles without planted copies whose every read carries the adapter from a random cycle on (as much as fits)
    from well_duplicates_amd.lane_passes import parse_adapter
    bare = synth.SynthSpec(seed=5, n_clusters=n, row=a.cols, plant_per_64k=0)
    codes = np.array(parse_adapter(a.adapter)[1], dtype=np.uint8)
    rng = np.random.default_rng(29)
    three = TileBatch(sc, 3, a.cycles, n)
    for s in range(3):
        sc.h2d(three.filter_ptr(s), np.ones(n, dtype=np.uint8))
        at = rng.integers(0, a.cycles - 8 + 1, n)
        for c in range(a.cycles):
            sc.synth_plane(three.plane_ptr(s, c), bare, 1, 1101 + s, c)
            sc.synchronize()
            plane = sc.d2h(three.plane_ptr(s, c), n, np.uint8).copy()
            j = c - at
            inside = (j >= 0) & (j < codes.size)
            plane[inside] = codes[j[inside]] | 0x80
            sc.h2d(three.plane_ptr(s, c), plane)
    sc.synchronize()
    ad = LaneDups(sc, n, 3, a.cycles)
    ad.add(three, [0, 1, 2])
    _, ad_fin = clock(lambda: ad.finish())
    time_adapter(ad, 3, ad_fin, "every read with the adapter at a random cycle, three tiles")
    got = ad.adapter(codes, 1, 8)[0]
    assert got[4:7].sum() == got[0] == 3 * n, "a read is without its adapter"
    ad.close()
    three.free()


def time_umi(acc, tiles_n, t_finish, t_umi_add, t_index_add, what):
    """LaneDups.umi(E, M) and, on the same labels, LaneDups.consensus(0, M), each after a first call that pays for loading
    the kernels; and a pure read of 16 bytes per well, from the accumulator's own workspace"""
    acc.umi(a.umi_e, a.max_family)
    (urow, utiles), t_u = clock(lambda: acc.umi(a.umi_e, a.max_family))
    (urow0, _), t_u0 = clock(lambda: acc.umi(0, a.max_family))
    acc.consensus(0, max(3, a.max_family))
    crow, t_c = clock(lambda: acc.consensus(0, max(3, a.max_family)))
    nbytes = tiles_n * n * 16
    gbs = sc.stream_read_gbs(acc.d_ws, min(nbytes, acc.ws_bytes))
    t_read = nbytes / gbs / 1e6
    assert urow[1] == urow[0] - urow[4] and urow[11:19].sum() == urow[3] and urow[19:].sum() == urow[4] and \
        urow[19] == urow[2] and (utiles.sum(axis=0) == urow[:3]).all() and urow0[4] == urow0[5] == urow[5] and \
        urow[3] >= crow[0][0] + crow[0][8], "the UMI rows do not add up"
    print("%s: umi, %d cycles, E %d, max_family %d: %d families of %d wells, %d molecules (%d at E 0), %d redundant, %d lone, "
          "%d families split, %d wells with N; %d large families of %d wells left out; MolPerFamily %s; MoleculeSize %s"
          % (what, a.umi, a.umi_e, a.max_family, urow[3], urow[0], urow[4], urow0[4], urow[1], urow[2], urow[6], urow[8], urow[9],
             urow[10], " ".join(str(v) for v in urow[11:19]), " ".join(str(v) for v in urow[19:])))
    print("  %-22s %9.3f ms  (%.4f ms per tile; index_add of the same planes: %.4f; umi_add / index_add = %.2f)"
          % ("lane umi_add", t_umi_add, t_umi_add / tiles_n, t_index_add / tiles_n, t_umi_add / t_index_add))
    print("  %-22s %9.3f ms  (%.4f ms per tile; E 0: %.4f; a pure read of label, members and keys, 16 bytes per well: %.4f ms "
          "per tile at %.0f GB/s; umi / read = %.2f; consensus(0): %.4f; umi / consensus = %.2f; the equality finish: %.4f)"
          % ("lane umi", t_u, t_u / tiles_n, t_u0 / tiles_n, t_read / tiles_n, gbs, t_u / t_read, t_c / tiles_n, t_u / t_c,
             t_finish / tiles_n))


def time_molecules(acc, tiles_n, what):
    """LaneDups.umi(E, M, molecules=True) beside umi(E, M) and LaneDups.keep(Q, by_molecule=True) beside keep(Q), each
    after a first call that pays for loading the kernels (and, for the molecules, for allocating their region)"""
    acc.umi(a.umi_e, a.max_family, molecules=True)
    (mrow, mtiles), t_m = clock(lambda: acc.umi(a.umi_e, a.max_family, molecules=True))
    (urow, utiles), t_u = clock(lambda: acc.umi(a.umi_e, a.max_family))
    acc.keep(a.min_q)
    (krow, _), t_k = clock(lambda: acc.keep(a.min_q))
    acc.keep(a.min_q, by_molecule=True)
    (brow, btiles), t_b = clock(lambda: acc.keep(a.min_q, by_molecule=True))
    assert (mrow == urow).all() and (mtiles == utiles).all(), "the rows of umi(molecules=True) are not those of umi()"
    assert brow[0] == brow[1] + brow[2] == krow[0] and brow[2] == urow[1] + urow[10] - urow[9] <= krow[2] and \
        brow[6] == urow[4] - urow[19] + urow[9] and brow[1] == krow[1] - krow[6] + urow[4] + urow[9] and \
        (btiles.sum(axis=0) == brow[:6]).all() and brow[9:].sum() == brow[6], "the rows by molecule do not add up"
    print("%s: keep by molecule, E %d, max_family %d, min_q %d: %d PF wells, %d kept (%d by family), %d dropped (%d), %d "
          "molecules of two or more wells (%d families), %d of them moved (%d)"
          % (what, a.umi_e, a.max_family, a.min_q, brow[0], brow[1], krow[1], brow[2], krow[2], brow[6], krow[6], brow[7], krow[7]))
    print("  %-22s %9.3f ms  (%.4f ms per tile; umi(E, M): %.4f; molecules / umi = %.2f; 8 bytes per well written: %.1f MB per tile)"
          % ("lane umi, molecules", t_m, t_m / tiles_n, t_u / tiles_n, t_m / t_u, 8 * n / 1e6))
    print("  %-22s %9.3f ms  (%.4f ms per tile; keep(Q): %.4f; by molecule / by family = %.2f)"
          % ("lane keep, by molecule", t_b, t_b / tiles_n, t_k / tiles_n, t_b / t_k))


if a.umi:
    print("umi part: %d UMI cycles, workspace %.2f GB, scratch %.2f GB"
          % (a.umi, sc.lane_umi_workspace_bytes(n, a.tiles, a.umi) / 1e9, sc.lane_umi_scratch_bytes(a.tiles, n) / 1e9))
    # the planted lane: the UMI planes are the cycles behind the read's, of the same synthetic tiles
    tb, utb = TileBatch(sc, a.batch, a.cycles, n), TileBatch(sc, a.batch, a.umi, n)
    lu = LaneDups(sc, n, a.tiles, a.cycles)
    lu.index_begin(a.umi)
    lu.umi_begin(a.umi)
    if a.keep_umi:
        lu.qual_begin(QUALITY_BINS)
    u_uadd = u_iadd = 0.0
    for bi, tiles in enumerate(batches):
        if len(tiles) != tb.n_tiles:
            tb, utb = TileBatch(sc, len(tiles), a.cycles, n, reuse=tb), TileBatch(sc, len(tiles), a.umi, n, reuse=utb)
        fill(tb, tiles)
        for s_, t in enumerate(tiles):
            for c in range(a.umi):
                sc.synth_plane(utb.plane_ptr(s_, c), spec, 1, 1101 + t, a.cycles + c)
        sc.synchronize()
        lu.add(tb, tiles)
        if a.keep_umi:
            lu.qual_add(tb, tiles)
        if bi == 0:                                  # (the first call of a kernel pays for loading it)
            warm = LaneDups(sc, n, len(tiles), a.cycles)
            warm.index_begin(a.umi)
            warm.umi_begin(a.umi)
            warm.index_add(utb, list(range(len(tiles))))
            warm.umi_add(utb, list(range(len(tiles))))
            warm.close()
        _, dt = clock(lambda: lu.index_add(utb, tiles))
        u_iadd += dt
        _, dt = clock(lambda: lu.umi_add(utb, tiles))
        u_uadd += dt
    _, u_fin = clock(lambda: lu.finish())
    assert (lu.umi_keys() == lu.index_keys()).all(), "the UMI keys differ from the index keys of the same planes"
    time_umi(lu, max(1, a.tiles), u_fin, u_uadd, u_iadd, "the planted lane")
    if a.keep_umi:
        time_molecules(lu, max(1, a.tiles), "the planted lane")
    lu.close()
    tb.free()
    utb.free()
    three, uthree = TileBatch(sc, 3, a.cycles, n), TileBatch(sc, 3, a.umi, n)
    if a.equal:
        for s in range(3):
            three.upload_tile(s, [np.full(n, 0x42 + (c % 4), dtype=np.uint8) for c in range(a.cycles)], np.ones(n, dtype=np.uint8))
            for c in range(a.umi):
                sc.synth_plane(uthree.plane_ptr(s, c), spec, 1, 1101 + s, a.cycles + c)
        sc.synchronize()
        eq = LaneDups(sc, n, 3, a.cycles)
        eq.index_begin(a.umi)
        eq.umi_begin(a.umi)
        if a.keep_umi:
            eq.qual_begin(QUALITY_BINS)
        eq.add(three, [0, 1, 2])
        if a.keep_umi:
            eq.qual_add(three, [0, 1, 2])
        _, e_iadd = clock(lambda: eq.index_add(uthree, [0, 1, 2]))
        _, e_uadd = clock(lambda: eq.umi_add(uthree, [0, 1, 2]))
        _, e_fin = clock(lambda: eq.finish())
        time_umi(eq, 3, e_fin, e_uadd, e_iadd, "every read equal, three tiles")
        if a.keep_umi:
            time_molecules(eq, 3, "every read equal, three tiles")
        assert eq.umi(a.umi_e, a.max_family)[0][9:11].tolist() == [1, 3 * n], "the equal lane is not one Large family"
        eq.close()
    # three tiles without planted copies whose wells of odd index repeat the well to their left, cycle by cycle, and its
    # UMI but for the last cycle
    bare = synth.SynthSpec(seed=5, n_clusters=n, row=a.cols, plant_per_64k=0)
    for s in range(3):
        sc.h2d(three.filter_ptr(s), np.ones(n, dtype=np.uint8))
        for c in range(a.cycles + a.umi):
            dst = three.plane_ptr(s, c) if c < a.cycles else uthree.plane_ptr(s, c - a.cycles)
            sc.synth_plane(dst, bare, 1, 1101 + s, c)
            sc.synchronize()
            if c < a.cycles + a.umi - 1:
                plane = sc.d2h(dst, n, np.uint8).copy()
                plane[1::2] = plane[0::2][:plane[1::2].size]
                sc.h2d(dst, plane)
    sc.synchronize()
    pr = LaneDups(sc, n, 3, a.cycles)
    pr.index_begin(a.umi)
    pr.umi_begin(a.umi)
    if a.keep_umi:
        pr.qual_begin(QUALITY_BINS)
    pr.add(three, [0, 1, 2])
    if a.keep_umi:
        pr.qual_add(three, [0, 1, 2])
    _, p_iadd = clock(lambda: pr.index_add(uthree, [0, 1, 2]))
    _, p_uadd = clock(lambda: pr.umi_add(uthree, [0, 1, 2]))
    _, p_fin = clock(lambda: pr.finish())
    time_umi(pr, 3, p_fin, p_uadd, p_iadd, "every odd well a copy of its left neighbour, three tiles")
    if a.keep_umi:
        time_molecules(pr, 3, "every odd well a copy of its left neighbour, three tiles")
    prow = pr.umi(0, a.max_family)[0]
    assert prow[3] >= 3 * (n // 2) - 3 and prow[11 + 2:19].sum() == 0, "the families are not pairs"
    pr.close()
    three.free()
    uthree.free()


def time_keep(acc, tiles_n, t_finish, what):
    """LaneDups.keep(Q) without and with the masks and, on the same labels, LaneDups.gc(0) and LaneDups.qualities(0), each
    after a first call that pays for loading the kernels; and a pure read of as many bytes as the pass reads, from the
    accumulator's own quality workspace"""
    acc.keep(a.min_q)
    (krow, ktiles), t_k = clock(lambda: acc.keep(a.min_q))
    (_, _, masks), t_km = clock(lambda: acc.keep(a.min_q, masks=True))
    acc.gc(0)
    (grow, _, _), t_g = clock(lambda: acc.gc(0))
    acc.qualities(0)
    q, t_q = clock(lambda: acc.qualities(0))
    nbytes = tiles_n * n * (4 * ((a.cycles + 9) // 10) + 18)
    gbs = sc.stream_read_gbs(acc.d_qual, min(nbytes, acc.qual_bytes))
    t_read = nbytes / gbs / 1e6
    weight = np.array([max(e for e in QUALITY_BINS if e <= v) for v in range(64)])
    weight[weight < a.min_q] = 0
    assert krow[0] == krow[1] + krow[2] == grow[0] and krow[2] == grow[3] and krow[6] == grow[2] and \
        (ktiles.sum(axis=0) == krow[:6]).all() and krow[9:].sum() == krow[6] and krow[7] == krow[6] - krow[9] == krow[3] and \
        krow[4] + krow[5] == (weight * q[2]).sum() and sum(int(m.sum()) for m in masks.values()) == krow[1], \
        "the keep rows do not add up"
    print("%s: keep, min_q %d: %d PF wells, %d kept, %d dropped, %d families, %d of them moved; mean score per base of the kept "
          "%.3f, of the families' first wells %.3f, of the dropped %.3f; families by gain %s"
          % (what, a.min_q, krow[0], krow[1], krow[2], krow[6], krow[7], krow[4] / max(1, krow[1] * a.cycles),
             krow[8] / max(1, krow[6] * a.cycles), krow[5] / max(1, krow[2] * a.cycles), " ".join(str(v) for v in krow[9:])))
    print("  %-22s %9.3f ms  (%.4f ms per tile; with the masks: %.4f; %.1f MB per tile at %.0f GB/s; a pure read of as many "
          "bytes: %.4f ms per tile at %.0f GB/s; keep / read = %.2f; gc(0): %.4f; keep / gc = %.2f; qualities(0): %.4f; the "
          "equality finish: %.4f)"
          % ("lane keep", t_k, t_k / tiles_n, t_km / tiles_n, nbytes / tiles_n / 1e6, nbytes / t_k / 1e6, t_read / tiles_n, gbs,
             t_k / t_read, t_g / tiles_n, t_k / t_g, t_q / tiles_n, t_finish / tiles_n))


if a.keep:
    print("keep pass: quality workspace %.2f GB, scratch %.2f GB"
          % (sc.lane_qual_workspace_bytes(n, a.tiles, a.cycles) / 1e9, sc.lane_keep_scratch_bytes(a.tiles, n) / 1e9))
    tb = TileBatch(sc, a.batch, a.cycles, n)
    lk = LaneDups(sc, n, a.tiles, a.cycles)
    lk.qual_begin(QUALITY_BINS)
    for tiles in batches:
        if len(tiles) != tb.n_tiles:
            tb = TileBatch(sc, len(tiles), a.cycles, n, reuse=tb)
        fill(tb, tiles)
        lk.add(tb, tiles)
        lk.qual_add(tb, tiles)
    _, k_fin = clock(lambda: lk.finish())
    time_keep(lk, max(1, a.tiles), k_fin, "the planted lane")
    lk.close()
    tb.free()
    if a.equal:
        three = TileBatch(sc, 3, a.cycles, n)
        rng = np.random.default_rng(13)
        for name, random_q in (("every read equal with one quality, three tiles", False),
                               ("every read equal with random qualities, three tiles", True)):
            for c in range(a.cycles):
                plane = (rng.integers(1, 64, n).astype(np.uint8) << 2 if random_q else np.uint8(37 << 2)) | np.uint8(c % 4)
                plane = np.ascontiguousarray(np.broadcast_to(plane, (n,)), dtype=np.uint8)
                for s in range(3):                   # (the other two tiles: the same qualities, shifted along the tile)
                    sc.h2d(three.plane_ptr(s, c), np.roll(plane, 1009 * s) if random_q and s else plane)
            for s in range(3):
                sc.h2d(three.filter_ptr(s), np.ones(n, dtype=np.uint8))
            sc.synchronize()
            eq = LaneDups(sc, n, 3, a.cycles)
            eq.qual_begin(QUALITY_BINS)
            eq.add(three, [0, 1, 2])
            eq.qual_add(three, [0, 1, 2])
            _, e_fin = clock(lambda: eq.finish())
            time_keep(eq, 3, e_fin, name)
            erow = eq.keep(a.min_q)[0]
            assert erow[1] == 1 and erow[6] == 1 and (erow[7] == 0 or random_q), "the equal lane is not one family with one well kept"
            eq.close()
        three.free()
sc.close()
