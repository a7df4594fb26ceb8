/*
 * welldup_laneconsensus.h - a lane's errors against its families' vote (libwelldup.so, the `tiledups` translation unit).
 *
 * wd_lane_mismatches compares every redundant well with the first well of its group, so an error in that first well is
 * counted once per copy and in the wrong direction: it cannot tell G>T from T>G.  A family of three or more wells
 * holds the answer: the base most of its members call at a cycle is the molecule's, and a member that disagrees made
 * the error.  wd_lane_consensus gathers the members of every family in device memory, takes the vote per cycle and
 * counts every well's calls against it - a DIRECTIONAL confusion matrix per cycle, exact over every family of the
 * lane, without an alignment.
 * Definitions, for one lane, after a successful finish of either kind (read, PF, the codes A C G T N = 0..4, the global
 * id, the labels and members as in welldup_lanegc.h):
 *   family        a root r (label(r) == id(r), members(r) >= 1) with its copies: n = members(r) + 1 wells;
 *   voted family  a family with 3 <= n <= max_family, max_family the caller's, 3 .. WD_LANECONSENSUS_MAX_FAMILY.  A
 *                 family of 2 cannot vote: it is counted in PairFamilies.  A family above max_family is a contaminant
 *                 (poly-G, an adapter dimer: what wd_lane_top names), not a molecule: it is counted in LargeFamilies /
 *                 LargeWells and never gathered;
 *   consensus     of a voted family at scanned cycle c: the code a (0..4, N votes like a base) that STRICTLY MORE THAN
 *                 HALF of its n wells hold.  If no code is, the cycle is undecided for the family and none of its
 *                 wells is compared there;
 *   d(w)          of a well of a voted family, the root included: the decided cycles at which its code is not the
 *                 consensus;
 *   Dist          9 bins, d = 0..7 and d >= 8, over every well of every voted family;
 *   profiled      a well of a voted family with d(w) <= max_d, max_d the caller's, 0..7;
 *   calls         int64 [L][5][5]: calls[c][a][b] = the profiled wells of the voted families for which c is decided,
 *                 whose consensus at c is a and whose own code is b.  The diagonal is the agreeing calls, so
 *                 P(b | a, c) is read directly; off the diagonal a is the molecule and b the error;
 *   lane row      WD_LANECONSENSUS_LANE_COLS = 20 int64 [Families, Wells, Profiled, Mismatches, WithN, Undecided,
 *                 UndecidedCalls, FirstWellOff, PairFamilies, LargeFamilies, LargeWells, Dist[0..8]]: Families and Wells
 *                 the voted families and their wells; Mismatches the off-diagonal sum of calls, WithN its part with a or
 *                 b = N; Undecided the (family, cycle) pairs without a majority, UndecidedCalls the same weighted by the
 *                 family's profiled wells; FirstWellOff the voted families whose root has d >= 1;
 *   tile row      WD_LANECONSENSUS_TILE_COLS = 4 int64 per tile index, by the well's own tile [Wells, Profiled,
 *                 Mismatches, WithN]; zero for an index never added.
 * Identities:
 *   1. PairFamilies + Families + LargeFamilies = Classes of the last finish's lane row (under a near finish: its
 *      clusters of two or more wells);
 *   2. 2 PairFamilies + Wells + LargeWells = Classes + Redundant of that row: the wells of all groups of two or more;
 *   3. the sum of Dist = Wells;
 *   4. Profiled = the sum of Dist[d] over d <= max_d;
 *   5. Mismatches = the sum of d x Dist[d] over d <= max_d;
 *   6. the sum of calls = Profiled x L - UndecidedCalls;
 *   7. the tile rows sum to the lane row's columns 1..4;
 *   8. within a voted family fewer than n / 2 wells sit off the diagonal at any cycle: for every c and a the
 *      off-diagonal sum of calls[c][a] is smaller than calls[c][a][a] whenever max_d lets every well in, and the
 *      diagonal of a decided cycle is never empty;
 *   9. under equality labels Dist[0] = Wells and calls is diagonal; Undecided, Mismatches and FirstWellOff are 0;
 *  10. Families, Wells and every cell of calls grow with max_family; calls at max_d - 1 is entrywise <= calls at max_d;
 *  11. nothing depends on the order or batching of the add calls, on hash_bits, on which other passes ran before, on
 *      how often the call is made, or on the order in which a family's members landed in the list.
 */
#ifndef WELLDUP_LANECONSENSUS_H
#define WELLDUP_LANECONSENSUS_H

#include "welldup_lanedups.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WD_LANECONSENSUS_MAX_D 7
#define WD_LANECONSENSUS_DIST_BINS 9
#define WD_LANECONSENSUS_MAX_FAMILY 4096
#define WD_LANECONSENSUS_LANE_COLS 20
#define WD_LANECONSENSUS_TILE_COLS 4

/* Device memory wd_lane_consensus needs for an accumulator of max_tiles tiles of wells_per_tile wells and reads of L
 * cycles.  Host arithmetic only.  With W = max_tiles * wells_per_tile and every part rounded up to 256 bytes:
 *     2048 * max_tiles                    per tile index 64 copies of 4 uint64: the tile row
 *   + 8192                                64 copies of 16 uint64: the lane's counters
 *   + 256                                 the cursor of the reservation: list words and families in one uint64
 *   + 4 * max_tiles                       the tile indices that were added
 *   + 200 * L                             calls, L x 25 uint64
 *   + 4 * W                               per well: where its family's range begins (written for the voted roots)
 *   + 4 * W                               the member list and the family table in one region: the list grows from its
 *                                         front - the n - 1 copies of each voted family, the root is known from the
 *                                         table -, the table of roots from its back, one word per family: together one
 *                                         word per voted well
 * which is 8 bytes per well of the lane plus the counters (a HiSeq 4000 lane of 112 tiles of 4.3 M wells at 151 cycles:
 * 3.85 GB, beside the accumulator's 47 GB).
 * A negative argument or a null pointer: WD_ERR_ARG; L > 1024, max_tiles > 65535 or W >= 2^32 - 1: WD_ERR_UNSUPPORTED. */
int wd_lane_consensus_scratch(int max_tiles, int64_t wells_per_tile, int L, size_t *bytes);

/* After a successful finish of either kind and before wd_lane_dups_end, any number of times and with any max_d and
 * max_family, before or after every other pass.  lane_row (WD_LANECONSENSUS_LANE_COLS int64), tile_rows (max_tiles x
 * WD_LANECONSENSUS_TILE_COLS int64) and calls (L x 5 x 5 int64) are HOST memory.  scratch_dev: DEVICE memory of at
 * least wd_lane_consensus_scratch(max_tiles, wells_per_tile, L) bytes, the caller's, whatever it holds; free to reuse
 * when the call returns.  The call reads the label array, the members and the packed rows and writes nothing but its
 * scratch.  Synchronous on the context's stream.  A lane without wells or tiles: WD_OK with zeros.
 * WD_ERR_ARG, changing nothing: a call before a successful finish (a near finish refused over budget is none), max_d
 * outside 0 .. 7, max_family outside 3 .. 4096, a null lane_row, tile_rows or calls, a scratch region that is null, in
 * host memory or too small. */
int wd_lane_consensus(wd_lane_dups *ld, int max_d, int max_family, void *scratch_dev, size_t scratch_bytes,
                      int64_t *lane_row, int64_t *tile_rows, int64_t *calls);

#ifdef __cplusplus
}
#endif
#endif /* WELLDUP_LANECONSENSUS_H */
