/*
 * welldup_lanedistance.h - how far apart a lane's duplicate copies lie (libwelldup.so, the `tiledups` translation unit).
 *
 * welldup_lanedups.h and welldup_lanenear.h group the reads of a lane wherever they lie and say how many wells that
 * makes redundant, "within tiles" and "across tiles"; welldup_tiledups.h says which share of a tile's classes lies
 * inside the rings of -l levels, about 100 units.  Nothing says whether a redundant well sits beside its original -
 * a copy made on the flowcell, which tells nothing about the library - or anywhere on the tile, as a PCR copy does.
 * wd_lane_distances reads the labels that the last finish left in the accumulator together with the wells'
 * coordinates and bins the distance of every redundant well from its root.
 * Definitions, for one lane, after a successful finish of either kind:
 *   coordinates   x[w], y[w], w = 0 .. N - 1: int32, the same for every tile of the lane (one s.locs per run), each
 *                 in 0 .. 2^24 - 1; the units are the caller's (the CLI passes the FASTQ-header units
 *                 int(v * 10 + 1000.5) of the s.locs positions);
 *   labels, pair, root
 *                 as welldup_lanemismatch.h: a pair is a PF well w with label(w) != global id(w), its root
 *                 r = label(w), the smallest global id of its class or cluster; one pair per redundant well;
 *   same-tile pair
 *                 the root lies on the member's tile: r / N == tile index(w); every other pair is a cross-tile pair;
 *   q(w)          of a same-tile pair: (x_w - x_r)^2 + (y_w - y_r)^2 in 64-bit integers (it can reach nearly 2^49);
 *   Dist          WD_LANEDISTANCE_DIST_BINS = 11 bins over the same-tile pairs, by integer tests on q only:
 *                   bin 0            q < 2^10: a distance under 32 units (on a honeycomb: the first ring);
 *                   bin b = 1 .. 9   2^(8 + 2b) <= q < 2^(10 + 2b): distances in [32 * 2^(b-1), 32 * 2^b);
 *                   bin 10           q >= 2^28: a distance of 16 384 or more.
 *                 It does not depend on the radius;
 *   Local         the same-tile pairs with q < radius^2 ("closer than R"), radius the caller's, 0 .. 2^25.  Strictly
 *                 less, so that Local at R = 32 * 2^j is exactly the sum of Dist[0..j];
 *   TilePairs     [max_tiles][max_tiles] int64, optional: TilePairs[a][b] = the pairs whose root lies on tile index
 *                 a and whose member lies on tile index b;
 *   lane row      WD_LANEDISTANCE_LANE_COLS int64 [Pairs, SameTile, Local, Dist[0..10]];
 *   tile row      WD_LANEDISTANCE_TILE_COLS int64 per tile index [Pairs, SameTile, Local], attributed to the tile of
 *                 the MEMBER w; zero for an index never added.
 * Identities: Pairs = Redundant of the last finish's lane row, and per tile Pairs = LaneRedundant of that finish's
 * tile row; the sum of Dist = SameTile; Local(32 * 2^j) = the sum of Dist[0..j] for j = 0 .. 9; Local(0) = 0,
 * Local(2^25) = SameTile, and Local is monotone in the radius; the tile rows sum to the lane row's first three
 * columns; column b of TilePairs sums to tile row b's Pairs, and its diagonal entry is that row's SameTile;
 * TilePairs[a][b] = 0 for a > b (the root is the smallest global id); per tile SameTile <= TileRedundant of the
 * finish, with equality when no class has more than two members; nothing depends on the order or batching of the
 * add calls, on hash_bits, on whether wd_lane_index_finish or wd_lane_mismatches ran before, or on how often the
 * call is made.
 * One limit: a member is paired with the ROOT of its class, not with the nearest classmate on its own tile.  A well
 * whose root lies on another tile while a second classmate sits beside it counts as cross-tile (a local copy of a
 * PCR copy: second order).  SameTile / (InClasses - TileSpans) of the finish says how much that is.
 */
#ifndef WELLDUP_LANEDISTANCE_H
#define WELLDUP_LANEDISTANCE_H

#include "welldup_lanemismatch.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WD_LANEDISTANCE_DIST_BINS 11
#define WD_LANEDISTANCE_LANE_COLS (3 + WD_LANEDISTANCE_DIST_BINS)
#define WD_LANEDISTANCE_TILE_COLS 3
#define WD_LANEDISTANCE_MAX_COORD ((1 << 24) - 1)
#define WD_LANEDISTANCE_MAX_RADIUS (1 << 25)
#define WD_LANEDISTANCE_MATRIX_MAX_TILES 4096

/* Device memory wd_lane_distances needs for tiles of N wells and an accumulator of max_tiles tiles; matrix != 0: with
 * TilePairs.  Host arithmetic only.  With every part rounded up to 256 bytes:
 *     8 * N                               the coordinates, (x, y) side by side: a well's position is one 8-byte load
 *   + 1536 * max_tiles                    per tile index 64 copies of 3 uint64: Pairs, SameTile, Local
 *   + 8192                                Dist, 64 copies of 16 uint64 (11 used)
 *   + 4 * max_tiles                       the tile indices that were added
 *   + 8 * max_tiles * max_tiles           TilePairs, one copy (only when matrix is set): a workgroup adds to its
 *                                         column once per root tile it met
 * (a HiSeq 4000 lane of 112 tiles of 4 309 650 wells, with the matrix: 34 758 400 bytes, 34.8 MB, of which the
 * coordinates are 34.5 MB).
 * A negative size or a null pointer: WD_ERR_ARG; max_tiles > 65535, or matrix with max_tiles > 4096 (the kernel
 * counts a column of TilePairs in 16 KB of LDS): WD_ERR_UNSUPPORTED. */
int wd_lane_distance_scratch(int64_t N, int max_tiles, int matrix, size_t *bytes);

/* After a successful finish of either kind and before wd_lane_dups_end, any number of times and with any radius,
 * before or after wd_lane_index_finish and wd_lane_mismatches.  x, y (N int32 each), lane_row
 * (WD_LANEDISTANCE_LANE_COLS int64), tile_rows (max_tiles x WD_LANEDISTANCE_TILE_COLS int64) and tile_pairs
 * (max_tiles x max_tiles int64, [root's tile][member's tile], or null: no matrix) are HOST memory.  scratch_dev:
 * DEVICE memory of at least wd_lane_distance_scratch(N, max_tiles, tile_pairs != NULL) bytes, the caller's; free to
 * reuse when the call returns.  The call checks the coordinates on the host, copies them into the scratch side by
 * side, reads the label array and writes nothing but its scratch.  Synchronous on the context's stream.
 * WD_ERR_ARG, changing nothing: a call before a successful finish (a near finish refused over budget is none), a
 * radius outside 0 .. 2^25, a null x, y, lane_row or tile_rows, a scratch region that is null, in host memory or
 * too small, a coordinate outside 0 .. 2^24 - 1 (wd_last_error names the well). */
int wd_lane_distances(wd_lane_dups *ld, const int32_t *x, const int32_t *y, int64_t radius, void *scratch_dev,
                      size_t scratch_bytes, int64_t *lane_row, int64_t *tile_rows, int64_t *tile_pairs);

#ifdef __cplusplus
}
#endif
#endif /* WELLDUP_LANEDISTANCE_H */
