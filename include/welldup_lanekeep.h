/*
 * welldup_lanekeep.h - the best well of each of a lane's families, as a keep mask (libwelldup.so, the `tiledups`
 * translation unit).
 *
 * The passes after a finish measure a lane's duplication; this one acts on it.  Of every family - a read class, or a
 * cluster under a near finish - one well survives, the one with the highest sum of reported base qualities at or
 * above min_q (the choice of Picard's MarkDuplicates), and every other well of the family is dropped.  The result is
 * a byte per well, which the caller folds into the PF bit of the run directory's .filter files: a deduplicated lane
 * for every downstream converter, without a FASTQ and without an alignment.
 * Definitions, for one lane, after a successful finish of either kind, on an accumulator that has a quality part.
 * Read, PF, global id, label, members and the populations Single / Root / Copy are as in welldup_lanegc.h; bins, edges
 * and bin(q) as in welldup_lanequality.h.
 *   weight        of bin i: edges[i] if edges[i] >= min_q, else 0.  min_q is the caller's, 0 .. 63.  edges[0] == 0, so
 *                 bin 0 always weighs 0: no-calls and the unused codes of a row's last word add nothing.  On an
 *                 instrument whose quality levels are the edges a well's score is exactly Picard's sum, otherwise a
 *                 lower bound of it;
 *   score(w)      of a PF well: the sum over the scanned cycles of the weight of the bin of its quality at that cycle.
 *                 At most 63 x 1024 = 64 512: it fits 16 bits for every L the accumulator takes;
 *   family        a Root with its Copies, of any size.  Nothing is gathered: there is no limit on a family;
 *   best(f)       the member of the family with the largest score; ties go to the smallest global id.  A root has the
 *                 smallest id of its family, so best != root implies score(best) > score(root) strictly;
 *   kept(w)       w is PF, and either Single or the best of its family.  Every other PF well is dropped;
 *   gain(f)       score(best) - score(root), >= 0, counted once per family, at the root.  GainBins[8] counts the
 *                 families by gain: 0, 1-9, 10-19, 20-49, 50-99, 100-199, 200-499, >= 500;
 *   lane row      WD_LANEKEEP_LANE_COLS = 17 int64 [PF, Kept, Dropped, MovedIn, SumKept, SumDropped, Families, Moved,
 *                 SumRoots], then GainBins[8].  SumKept / SumDropped / SumRoots are scores summed over the kept wells
 *                 (Singles included), the dropped wells and the roots of families; Moved counts the families whose
 *                 best is not their root;
 *   tile row      WD_LANEKEEP_TILE_COLS = 6 int64 per tile index: the first six lane columns, counted by the well's own
 *                 tile.  MovedIn counts the kept wells that are Copies.  Zero for an index never added;
 *   keep mask     per tile, optionally, N bytes: 1 for a kept well, 0 for any other - dropped, not PF, or of a tile
 *                 never added.
 * Identities:
 *   1. PF = Kept + Dropped = PF of the last finish's lane row; Dropped = its Redundant; Kept - Families = the Singles;
 *   2. the tile rows sum to the first six lane columns; per tile PF is that finish's tile PF; per tile Dropped need not
 *      be the finish's LaneRedundant (the best of a family may lie on another tile than its root): only the sums agree;
 *   3. Moved = Families - GainBins[0] = the lane's MovedIn; the sum of GainBins = Families;
 *   4. SumKept + SumDropped = the sum over q of weight[bin(q)] x QHist[q], QHist that of wd_lane_qualities on the
 *      same accumulator;
 *   5. SumKept - SumSingles >= SumRoots, with equality iff Moved == 0; the difference is the sum of the gains;
 *   6. with min_q above every edge all weights are 0: best = root everywhere, the mask is label == id, every Sum is 0;
 *   7. Moved and the masks depend on neither the order or batching of the add and qual_add calls, nor hash_bits, nor
 *      which other passes ran before, nor how often the call is made;
 *   8. a lane rebuilt from the same planes with filter & mask as its filter has Redundant = 0 and PF = Kept, under the
 *      equality finish and under a near finish with the same K: wells of different clusters are more than K apart,
 *      and one well per cluster is left.
 */
#ifndef WELLDUP_LANEKEEP_H
#define WELLDUP_LANEKEEP_H

#include "welldup_lanequality.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WD_LANEKEEP_LANE_COLS 17
#define WD_LANEKEEP_TILE_COLS 6
#define WD_LANEKEEP_GAIN_BINS 8
#define WD_LANEKEEP_MAX_Q 63

/* Device memory wd_lane_keep needs for an accumulator of max_tiles tiles of wells_per_tile wells.  Host arithmetic
 * only.  With W = max_tiles * wells_per_tile and every part rounded up to 256 bytes:
 *     8 * W                               best: per well of the lane (0xFFFF - score) << 32 | id of the best of the
 *                                         family rooted there
 *   + 2 * W                               score: per well, 16 bits
 *   + 3072 * max_tiles                    per tile index 64 copies of 6 uint64: the tile row
 *   + 5632                                64 copies of 11 uint64: Families, Moved, SumRoots, GainBins
 *   + 4 * max_tiles                       the tile indices that were added
 *   + 8 * max_tiles                       the mask pointers, by tile index
 * (a HiSeq 4000 lane, 112 x 4 309 253 wells: 4.83 GB).  A negative size or a null pointer: WD_ERR_ARG; max_tiles >
 * 65535 or max_tiles * wells_per_tile >= 2^32 - 1: WD_ERR_UNSUPPORTED. */
int wd_lane_keep_scratch(int max_tiles, int64_t wells_per_tile, size_t *bytes);

/* After a successful finish of either kind and before wd_lane_dups_end, any number of times and with any min_q,
 * before or after every other pass.  lane_row (WD_LANEKEEP_LANE_COLS int64) and tile_rows (max_tiles x
 * WD_LANEKEEP_TILE_COLS int64) are HOST memory.  keep_dev: null, or max_tiles pointers in HOST memory, by tile index,
 * each null or N bytes of DEVICE memory that receive the tile's keep mask (zeros for an index never added).
 * scratch_dev: DEVICE memory of at least wd_lane_keep_scratch(max_tiles, N) bytes, the caller's; free to reuse when the
 * call returns.  The call reads the label array, the members and the quality rows and writes nothing but its scratch
 * and the masks.  Synchronous on the context's stream.  A lane without wells or tiles: WD_OK with zeros.
 * WD_ERR_ARG, changing nothing: no quality part, a call before a successful finish (a near finish refused over budget
 * is none), a tile index that was given to wd_lane_dups_add and not to wd_lane_qual_add or the reverse (wd_last_error
 * names one such tile), min_q outside 0 .. WD_LANEKEEP_MAX_Q, a null lane_row or tile_rows, a scratch region that is
 * null, in host memory or too small, a mask pointer in host memory. */
int wd_lane_keep(wd_lane_dups *ld, int min_q, void *scratch_dev, size_t scratch_bytes, int64_t *lane_row,
                 int64_t *tile_rows, uint8_t *const *keep_dev);

#ifdef __cplusplus
}
#endif
#endif /* WELLDUP_LANEKEEP_H */
