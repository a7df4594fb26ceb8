/*
 * welldup_lanetop.h - a lane's most frequent reads and their spread (libwelldup.so, the `tiledups` translation unit).
 *
 * welldup_lanedups.h and the headers after it say how much of a lane is duplicated, where, how far apart, at which
 * quality, and whether more sequencing pays.  None says WHICH reads the duplicates are: one adapter dimer at 4 % of
 * the lane, or a million small PCR families.  wd_lane_top reads what the last finish left in the accumulator - the
 * label of every well, the members counted at the roots, the packed rows - and delivers the duplication levels of the
 * whole lane and the n_top largest groups: root, size, how the group lies over the tiles, how many of its wells carry
 * exactly the root's read, and the read itself.  Exact, for every PF well of the lane.
 * Definitions, for one lane, after a successful finish of either kind; labels, roots and the global id
 * g = tile_index * N + well as welldup_lanedups.h / welldup_lanenear.h:
 *   group         a class (equality finish) or a cluster (near finish) of >= 2 PF wells; size = members at the root
 *                 + 1.  A PF well in no group is a group of size 1 for the levels only; it is never listed;
 *   levels        WD_LANETOP_LEVELS = 16 duplication levels by size, lower edges WD_LANETOP_EDGES
 *                 1 2 3 4 5 6 7 8 9 10 50 100 500 1000 5000 10000, the last open-ended.  Per level two int64:
 *                 Groups[i] (groups whose size falls in level i) and Wells[i] (the wells in them);
 *   order         groups of size >= 2 by size descending, ties by root global id ascending: a total order;
 *   list          the first min(n_top, Classes) groups in that order, 1 <= n_top <= WD_LANETOP_MAX = 1024.  Per listed
 *                 group: root (uint32 global id), size (uint32), exact (uint32: the wells of the group, root included,
 *                 whose read equals the root's, decided on the packed rows, all ceil(L / 10) words; size under an
 *                 equality finish), tile_count [max_tiles] (uint32: the group's wells per tile index, zero for an
 *                 index never added), read (L bytes from "ACGTN", the root's packed row decoded, not NUL-terminated);
 *   head row      WD_LANETOP_HEAD_COLS = 4 int64 [PF, Groups2, Listed, Covered]: Groups2 the groups of size >= 2,
 *                 Covered the sum of the listed sizes.
 * Identities: the sum of Wells = PF; Groups[0] = Wells[0] = PF - InClasses; the sum of Groups[1:] = Groups2 = Classes;
 * Groups[1 .. 7] are the finish's lane-row size bins 2 .. 8 and the sum of Groups[8:] is its ">= 9" bin;
 * Wells[i] = (i + 1) Groups[i] for i < 9; the sum of Wells[1:] = InClasses (lane row, bins, Classes and InClasses of
 * the finish that ran last: the near row after a near finish); per listed group the sum of tile_count = size,
 * 1 <= exact <= size and tile_count[tile of the root] >= 1; the list for n_top = a is the first a entries of the list
 * for any b > a; nothing depends on the order or batching of the add calls, on hash_bits, on cand_capacity, on which
 * other passes ran after the finish, or on how often the call is made.
 *
 * The selection is exact whatever the sizes are - fifty million classes of size 2, or one class that holds the lane:
 * histograms over the key (size, ~root) narrow the range that holds the n_top-th group until the roots at or above
 * it fit the candidate buffer, in at most WD_LANETOP_MAX_PASSES streaming passes over label and members (8 bytes a
 * well each); wd_get_option "lane_top_passes" reads how many the last call took, "lane_top_max_passes" the bound.
 */
#ifndef WELLDUP_LANETOP_H
#define WELLDUP_LANETOP_H

#include "welldup_lanesaturation.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WD_LANETOP_MAX 1024
#define WD_LANETOP_LEVELS 16
#define WD_LANETOP_HEAD_COLS 4
#define WD_LANETOP_EDGES {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 50, 100, 500, 1000, 5000, 10000}
#define WD_LANETOP_MAX_PASSES 8
#define WD_LANETOP_DEFAULT_CAPACITY 65536

/* Device memory wd_lane_top needs for an accumulator of max_tiles tiles and L cycles, a list of n_top groups and a
 * candidate buffer of cand_capacity roots (0: WD_LANETOP_DEFAULT_CAPACITY, raised to n_top); N takes no part in it.
 * Host arithmetic only.  With C the capacity in force and every part rounded up to 256 bytes:
 *     1 065 984                           the histograms, 64 copies of 2082 uint64: 2048 bins, the roots above the
 *                                         range, a spare word, and the 16 levels' Groups and Wells
 *   + 8 * C                               the candidates, {root, size}
 *   + 256                                 the candidates' count
 *   + 16384                               the listed roots' table, 2048 slots of {root, rank}
 *   + 4 * n_top                           the listed roots
 *   + 4 * n_top * max_tiles               tile_count
 *   + 4 * n_top                           exact
 *   + 4 * n_top * ceil(L / 10)            the listed roots' packed rows
 *   + 4 * max_tiles                       the tile indices that were added
 * (a HiSeq 4000 lane of 112 tiles and 151 cycles, n_top = 100 and the default capacity: 1 659 648 bytes, 1.7 MB,
 * whatever the 4 309 650 wells of a tile).
 * A negative size, n_top outside 1 .. 1024, a capacity that is negative or positive and below n_top, or a null
 * pointer: WD_ERR_ARG; max_tiles > 65535 or L > 1024: WD_ERR_UNSUPPORTED. */
int wd_lane_top_scratch(int64_t N, int max_tiles, int L, int n_top, int64_t cand_capacity, size_t *bytes);

/* After a successful finish of either kind and before wd_lane_dups_end, any number of times and with any n_top and
 * capacity, before or after wd_lane_index_finish, wd_lane_mismatches, wd_lane_distances, wd_lane_qualities and
 * wd_lane_saturation.  head_row (WD_LANETOP_HEAD_COLS int64), levels ([2][WD_LANETOP_LEVELS] int64: Groups, then
 * Wells), root, size, exact (n_top uint32 each), tile_count ([n_top][max_tiles] uint32) and reads ([n_top][L] bytes)
 * are HOST memory; entries past Listed are zeroed.  scratch_dev: DEVICE memory of at least
 * wd_lane_top_scratch(N, max_tiles, L, n_top, cand_capacity) bytes, the caller's; free to reuse when the call
 * returns.  The call reads label, members and the rows and writes nothing but its scratch.  Synchronous on the
 * context's stream.
 * cand_capacity: how many candidate roots the compaction buffer holds; with cand_capacity = n_top the selection runs
 * to the end (to a single key), with a large one it ends early.  The result does not depend on it.
 * WD_ERR_ARG, changing nothing: a call before a successful finish (a near finish refused over budget is none), n_top
 * outside 1 .. 1024, a capacity that is negative or positive and below n_top, a null output, a scratch region that is
 * null, in host memory or too small.  WD_ERR_STATE: the candidates are not as many as the histograms promised (it
 * cannot happen; the check costs one word). */
int wd_lane_top(wd_lane_dups *ld, int n_top, int64_t cand_capacity, void *scratch_dev, size_t scratch_bytes,
                int64_t *head_row, int64_t *levels, uint32_t *root, uint32_t *size, uint32_t *exact,
                uint32_t *tile_count, char *reads);

#ifdef __cplusplus
}
#endif
#endif /* WELLDUP_LANETOP_H */
