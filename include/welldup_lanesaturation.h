/*
 * welldup_lanesaturation.h - a lane's distinct reads against its depth (libwelldup.so, the `tiledups` translation unit).
 *
 * welldup_lanedups.h and welldup_lanenear.h say how many wells of a lane are redundant at the depth the lane was
 * sequenced to: one point, from which a library size is solved.  Nothing says how the distinct reads grew on the way
 * there - what the last reads still brought, and whether the library size stays put when it is solved from half the
 * reads.  wd_lane_saturation reads the labels that the last finish left in the accumulator and counts, for nested
 * pseudo-random subsamples of the PF wells that grow to the whole lane, the wells and the distinct reads among them:
 * exact, since a label is there for every well.  The local copies welldup_lanedistance.h identifies can be left out.
 * Definitions, for one lane, after a successful finish of either kind; labels, pair, root, same-tile pair, the
 * coordinates and q as welldup_lanedistance.h:
 *   step of a well  for the well's global id g (uint32), S steps, 1 <= S <= WD_LANESATURATION_MAX_STEPS = 64, and
 *                 the caller's seed (uint32), everything mod 2^32 except the last line:
 *                   h = g + seed * 0x9E3779B9
 *                   h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16
 *                   step(g) = (uint64(h) * S) >> 32                    in 0 .. S - 1
 *                 The subsample at step j: every counted well with step <= j.  The subsamples are nested and the one
 *                 at S - 1 is the lane;
 *   dropped well  with coordinates and radius > 0: a same-tile pair with q < radius^2 - exactly what
 *                 wd_lane_distances counts as Local, by the same integer test, coordinates 0 .. 2^24 - 1, radius
 *                 0 .. 2^25.  Without coordinates, or with radius 0, no well is dropped.  A root is never dropped;
 *   counted well  a PF well that is not dropped;
 *   NewReads[j]   the counted wells with step = j;
 *   NewDistinct[j]
 *                 the wells with label = own global id (roots, and PF wells in no class) whose class step is j: the
 *                 smallest step of the counted wells of the class, the well's own step when it has no class;
 *   head row      WD_LANESATURATION_HEAD_COLS = 2 int64 [PF, Dropped].
 * Identities: the sum of NewReads = PF - Dropped; the sum of NewDistinct = PF - Redundant of the last finish's lane
 * row; Dropped = Local of wd_lane_distances at the same radius; every prefix sum of NewDistinct <= the same prefix
 * sum of NewReads; coarsening: the result for S steps is the result for 2 S steps with steps 2j and 2j + 1 added
 * (floor(step_2S / 2) = step_S, and the minimum commutes with that); with S = 1 the single step holds both totals; a
 * lane without a class has NewDistinct = NewReads; nothing depends on the order or batching of the add calls, on
 * hash_bits, on which other passes ran after the finish, or on how often the call is made; the totals do not depend
 * on the seed.
 */
#ifndef WELLDUP_LANESATURATION_H
#define WELLDUP_LANESATURATION_H

#include "welldup_lanedistance.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WD_LANESATURATION_MAX_STEPS 64
#define WD_LANESATURATION_HEAD_COLS 2

/* Device memory wd_lane_saturation needs for tiles of N wells and an accumulator of max_tiles tiles; with_coords != 0:
 * with the coordinates.  Host arithmetic only.  With every part rounded up to 256 bytes:
 *     4 * max_tiles * N                   per well a word: the smallest step among the counted members of the class
 *                                         the well is the root of
 *   + 8 * N                               the coordinates, (x, y) side by side (only when with_coords is set)
 *   + 65536                               NewReads and NewDistinct, 64 copies of 2 x 64 uint64
 *   + 1024                                PF and Dropped, 64 copies of 2 uint64
 *   + 4 * max_tiles                       the tile indices that were added
 * (a HiSeq 4000 lane of 112 tiles of 4 309 650 wells, with coordinates: 1 965 267 712 bytes, 1.97 GB, of which the
 * words are 1.93 GB).
 * A negative size or a null pointer: WD_ERR_ARG; max_tiles > 65535: WD_ERR_UNSUPPORTED. */
int wd_lane_saturation_scratch(int64_t N, int max_tiles, int with_coords, size_t *bytes);

/* After a successful finish of either kind and before wd_lane_dups_end, any number of times and with any steps, seed
 * and radius, before or after wd_lane_index_finish, wd_lane_mismatches, wd_lane_distances and wd_lane_qualities.
 * x, y (N int32 each, or both null: no coordinates, and radius must be 0), head_row (WD_LANESATURATION_HEAD_COLS
 * int64), new_reads and new_distinct (steps int64 each) are HOST memory.  scratch_dev: DEVICE memory of at least
 * wd_lane_saturation_scratch(N, max_tiles, x != NULL) bytes, the caller's; free to reuse when the call returns.  The
 * call checks the coordinates on the host, copies them into the scratch side by side, reads the label array and
 * writes nothing but its scratch.  Synchronous on the context's stream.
 * WD_ERR_ARG, changing nothing: a call before a successful finish (a near finish refused over budget is none), steps
 * outside 1 .. 64, a radius outside 0 .. 2^25, exactly one of x and y null, radius > 0 without coordinates, a null
 * head_row, new_reads or new_distinct, a scratch region that is null, in host memory or too small, a coordinate
 * outside 0 .. 2^24 - 1 (wd_last_error names the well). */
int wd_lane_saturation(wd_lane_dups *ld, int steps, uint32_t seed, const int32_t *x, const int32_t *y, int64_t radius,
                       void *scratch_dev, size_t scratch_bytes, int64_t *head_row, int64_t *new_reads,
                       int64_t *new_distinct);

#ifdef __cplusplus
}
#endif
#endif /* WELLDUP_LANESATURATION_H */
