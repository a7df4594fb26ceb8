/*
 * welldup_lanenear.h - near-duplicate read clusters of a lane (libwelldup.so, the `tiledups` translation unit).
 *
 * welldup_lanedups.h groups the PF wells of a lane by equal reads; welldup_tilenear.h links the PF wells of ONE
 * tile by Hamming distance <= K.  Two copies of one molecule differ in a base or two more often than not, and
 * land on whatever tiles: the duplication of the library shows in the clusters of the LANE at Hamming <= K.
 * wd_lane_near_dups_finish stands in for wd_lane_dups_finish on an accumulator built by wd_lane_dups_begin /
 * wd_lane_dups_add, and delivers the classes exactly as that call would, and beside them the clusters.
 * Definitions, for one lane and the scanned cycles:
 *   read, PF wells, alphabet, global id   as welldup_lanedups.h (N == N, N differs from every base);
 *   edge          joins two PF wells of the lane, on whatever tiles, whose reads differ in at most K cycles
 *                 (K = 1 .. WD_LANENEAR_MAX_K);
 *   lane cluster  a connected component of at least two PF wells (single linkage; a non-PF well is no vertex and
 *                 bridges nothing);
 *   label         of a well: the smallest global id of its cluster; its own global id for a PF well in no
 *                 cluster; WD_INVALID_TARGET for a non-PF well and for every well of a tile index never added;
 *   near lane row WD_LANENEAR_LANE_COLS int64: [PF, Clusters, InClusters, Redundant, CrossTileClusters, TileSpans,
 *                 NearPairs, size bins 2..8 and >= 9].  NearPairs: the unordered pairs of DISTINCT READS of the
 *                 lane (one read per equality class, singletons included) at distance 1..K; it depends on neither
 *                 the order of execution, the order of the add calls, nor hash_bits.  The other columns as the
 *                 lane row of welldup_lanedups.h with "class" read as "cluster";
 *   near tile row WD_LANEDUPS_TILE_COLS int64 per tile index: [PF, InLane, InTile, TileRedundant, LaneRedundant] as
 *                 welldup_lanedups.h with "classmate" read as "well of the same cluster".
 * K = 0 gives the rows and labels of wd_lane_dups_finish with NearPairs 0; equal labels at K - 1 imply equal
 * labels at K; the identities of welldup_lanedups.h hold for the cluster rows; two wells of one tile that share a
 * wd_tile_near_dups label at K share a lane cluster label at K (not conversely: a read on another tile can bridge
 * them).  Levenshtein clusters are not offered (welldup_tilenear.h says why).
 */
#ifndef WELLDUP_LANENEAR_H
#define WELLDUP_LANENEAR_H

#include "welldup_lanedups.h"
#include "welldup_tilenear.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WD_LANENEAR_MAX_K 3
#define WD_LANENEAR_LANE_COLS (7 + WD_DUPSET_SIZE_BINS)

/* Extra device memory wd_lane_near_dups_finish needs at distance k for an accumulator of max_tiles tiles of N wells
 * and L cycles.  Host arithmetic only.  Chain link and rank of a read live in the accumulator's 8-byte
 * fingerprint / slot word per well and the segment buckets in its table, both dead once the classes are resolved;
 * the scratch holds what they cannot.  With W = max_tiles * N and every part rounded up to 256 bytes:
 *     k == 0:  0
 *     k >= 1:  64                          per segment {candidate pairs, members of long buckets}, 4 x 2 uint64
 *            + 512                         NearPairs, 64 copies of a uint64
 *            + 4 * W                       the members of the buckets of more than 32 reads
 * (a HiSeq 4000 lane, 112 x 4 309 253 wells: 1.93 GB).  Segment fingerprints take no memory: they are computed
 * from the packed rows.  Errors as wd_lane_dups_workspace; k outside 0 .. WD_LANENEAR_MAX_K: WD_ERR_ARG. */
int wd_lane_near_dups_scratch(int64_t N, int max_tiles, int L, int k, size_t *bytes);

/* Instead of wd_lane_dups_finish: lane_row, tile_rows and labels_dev get what that call delivers, and
 * near_lane_row (WD_LANENEAR_LANE_COLS int64), near_tile_rows (max_tiles x WD_LANEDUPS_TILE_COLS int64, both HOST
 * memory, not null) and near_labels_dev (as labels_dev: nullable; entries null or DEVICE pointers to N uint32) the
 * clusters at Hamming distance <= k.  k = 0 runs the equality finish and copies.  scratch_dev: DEVICE memory of
 * at least wd_lane_near_dups_scratch bytes (k = 0: may be null), the caller's; free to reuse when the call returns.
 * pair_budget: the most candidate pairs one segment of the lane may have - the sum of c (c - 1) / 2 over its
 * buckets, c the distinct reads in a bucket; 0 = the default, max(16 * max_tiles * N, 2^24).  The bounds of all
 * k + 1 segments are computed, in linear time, before any label is changed: a lane over budget returns
 * WD_ERR_UNSUPPORTED, wd_last_error names the segment, the count and the budget, the equality rows and labels have
 * been delivered and are valid, and the call may be repeated with another k or budget (the same equality results
 * are delivered again; wd_lane_dups_finish may be called instead; wd_lane_dups_add may not), or the lane ended.
 * After a success any finish is WD_ERR_ARG.  WD_ERR_ARG, changing nothing: k outside 0 .. WD_LANENEAR_MAX_K,
 * L < k + 1, a negative budget, a scratch region that is too small, null or in host memory, a null row, a label
 * pointer in host memory, a call after a successful finish. */
int wd_lane_near_dups_finish(wd_lane_dups *ld, int k, void *scratch_dev, size_t scratch_bytes, int64_t pair_budget,
                             int64_t *lane_row, int64_t *tile_rows, uint32_t *const *labels_dev,
                             int64_t *near_lane_row, int64_t *near_tile_rows, uint32_t *const *near_labels_dev);

#ifdef __cplusplus
}
#endif
#endif /* WELLDUP_LANENEAR_H */
