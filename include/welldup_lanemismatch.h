/*
 * welldup_lanemismatch.h - where a lane's duplicate copies differ (libwelldup.so, the `tiledups` translation unit).
 *
 * welldup_lanenear.h links the reads of a lane at Hamming distance <= K and says how many wells that makes
 * redundant; it does not say how far the copies it linked lie from each other, nor at which cycles they differ.
 * The first tells whether K was large enough (the mass sits in the last bin) or so large that unrelated reads are
 * linked (chains far from their root); the second is a sequencing error profile: copies of one molecule should be
 * identical, so the cycles at which they differ are errors (or no-calls), read off the lane itself, without a
 * spike-in and without an alignment.  wd_lane_mismatches reads the packed rows and the labels that the last finish
 * left in the accumulator, together.
 * Definitions, for one lane, after a successful finish of either kind:
 *   read, PF wells, alphabet (A C G T N = codes 0..4, N == N, N differs from every base), global id
 *                 as welldup_lanedups.h;
 *   labels        whatever the last successful finish left in the accumulator: class labels after
 *                 wd_lane_dups_finish, cluster labels after wd_lane_near_dups_finish with k >= 1
 *                 (welldup_laneindex.h's rule);
 *   pair          every PF well w with label(w) != global id(w), paired with its root r = label(w): exactly
 *                 Redundant pairs, one per redundant well;
 *   d(w)          the number of scanned cycles at which the reads of r and w differ (single linkage lets a member
 *                 lie further than K from its root);
 *   Dist          WD_LANEMISMATCH_DIST_BINS bins: the pairs with d = 0, 1, .., 7 and d >= 8.  It does not depend
 *                 on max_d;
 *   profiled pair a pair with d <= max_d, max_d the caller's, 0 .. WD_LANEMISMATCH_MAX_D.  Only profiled pairs
 *                 enter the substitution counts: a chain member far from its root is probably another molecule;
 *   Sub           L x 5 x 5 int64: Sub[c][a][b] = the profiled pairs whose root has code a and whose member has
 *                 code b != a at scanned cycle c.  The diagonal is zero; agreeing cycles are not counted.  The
 *                 direction (root, member) is arbitrary but deterministic: the root is the smallest global id;
 *   lane row      WD_LANEMISMATCH_LANE_COLS int64 [Pairs, Profiled, Mismatches, WithN, Dist[0..8]].  Mismatches:
 *                 the sum of Sub; WithN: the part of it where a or b is N;
 *   tile row      WD_LANEMISMATCH_TILE_COLS int64 per tile index [Pairs, Profiled, Mismatches, WithN], attributed
 *                 to the tile of the MEMBER w; zero for an index never added.
 * Identities: Pairs = Redundant of the last finish's lane row, and per tile Pairs = LaneRedundant of that finish's
 * tile row; the sum of Dist = Pairs; Profiled = the sum of Dist[d] over d <= max_d; Mismatches = the sum of
 * d x Dist[d] over d <= max_d (exact because max_d <= 7 lies below the open bin); the tile rows sum to the lane
 * row's first four columns; under equality labels Dist[0] = Pairs and everything else is zero; Sub at max_d - 1 is
 * entrywise <= Sub at max_d; nothing depends on the order or batching of the add calls, on hash_bits, or on
 * whether wd_lane_index_finish ran before.
 */
#ifndef WELLDUP_LANEMISMATCH_H
#define WELLDUP_LANEMISMATCH_H

#include "welldup_laneindex.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WD_LANEMISMATCH_MAX_D 7
#define WD_LANEMISMATCH_DIST_BINS 9
#define WD_LANEMISMATCH_LANE_COLS (4 + WD_LANEMISMATCH_DIST_BINS)
#define WD_LANEMISMATCH_TILE_COLS 4

/* Device memory wd_lane_mismatches needs for an accumulator of max_tiles tiles and L cycles.  Host arithmetic only.
 * With every part rounded up to 256 bytes:
 *     2048 * max_tiles                    per tile index 64 copies of 4 uint64: Pairs, Profiled, Mismatches, WithN
 *   + 8192                                Dist, 64 copies of 16 uint64 (9 used)
 *   + 4 * max_tiles                       the tile indices that were added
 *   + 200 * L                             Sub, L x 25 uint64, one copy: a workgroup adds to it once per entry of
 *                                         its own histogram that is not zero
 * (a HiSeq 4000 lane of 112 tiles at 151 cycles: 268 KB).  It does not depend on the wells of a tile.
 * A negative size or a null pointer: WD_ERR_ARG; L > 1024 or max_tiles > 65535: WD_ERR_UNSUPPORTED. */
int wd_lane_mismatch_scratch(int max_tiles, int L, size_t *bytes);

/* After a successful finish of either kind and before wd_lane_dups_end, any number of times and with any max_d,
 * before or after wd_lane_index_finish.  lane_row (WD_LANEMISMATCH_LANE_COLS int64), tile_rows (max_tiles x
 * WD_LANEMISMATCH_TILE_COLS int64) and sub (L x 25 int64, [cycle][root's code][member's code]) are HOST memory.
 * scratch_dev: DEVICE memory of at least wd_lane_mismatch_scratch bytes, the caller's; free to reuse when the call
 * returns.  The call reads the packed rows and the label array and writes nothing but its scratch: the table and
 * the per-well slot word, which wd_lane_index_finish uses, stay as they are.  Synchronous on the context's stream.
 * WD_ERR_ARG, changing nothing: a call before a successful finish (a near finish refused over budget is none),
 * max_d outside 0 .. WD_LANEMISMATCH_MAX_D, a null output pointer, a scratch region that is null, in host memory or
 * too small. */
int wd_lane_mismatches(wd_lane_dups *ld, int max_d, void *scratch_dev, size_t scratch_bytes, int64_t *lane_row,
                       int64_t *tile_rows, int64_t *sub);

#ifdef __cplusplus
}
#endif
#endif /* WELLDUP_LANEMISMATCH_H */
