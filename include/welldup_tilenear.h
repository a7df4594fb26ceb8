/*
 * welldup_tilenear.h - near-duplicate read clusters of every tile (libwelldup.so, the `tiledups` translation unit).
 *
 * welldup_tiledups.h groups the wells of a tile by equal reads.  Two copies of one molecule often differ in a
 * base or two, so this groups them by Hamming distance instead, wherever on the tile they lie, exactly (every
 * pair is decided on the reads).  Definitions, for one tile and the scanned cycles:
 *   read, vertices  as welldup_tiledups.h: byte 0 is N, any other byte "ACGT"[byte & 3]; quality bits never
 *                matter, N == N, N differs from every base; the vertices are the wells that pass the filter;
 *   edge         two PF wells whose reads differ in at most k cycles;
 *   cluster      a connected component of at least two PF wells over the edges (single linkage, as the
 *                duplicate sets of welldup_sets.h: A~B and B~C put A, B and C together even when A and C differ
 *                in more than k cycles).  A non-PF well is no vertex and bridges nothing.  Clusters,
 *                InClusters (the wells in them), Redundant = InClusters - Clusters; size bins 2..8 and >= 9;
 *   NearPairs    unordered pairs of distinct reads (one per equality class, singletons included) at distance
 *                1..k: the edges the clustering had to find beyond what equality gives;
 *   label        of a well: the smallest well index of its cluster; its own index for a PF well in none;
 *                WD_INVALID_TARGET for a non-PF well;
 *   Local[l], RingWells[l]  as welldup_tiledups.h with "classmate" read as "well of the same cluster".
 * k = 0 gives the classes of wd_tile_dups and NearPairs = 0; the clusters at k coarsen those at k - 1.
 * Levenshtein clusters over a tile are not offered (an insertion or deletion shifts every later segment of
 * the read, and the method below rests on segments that stay in place).
 *
 * Method: the reads are cut into k + 1 segments; two reads within k mismatches agree on a whole segment, so
 * for each segment the distinct reads are bucketed by the segment's fingerprint and compared inside a bucket.
 * A segment of low diversity (amplicons, a shared adaptor) makes buckets whose pairs cannot be enumerated:
 * the number of candidate pairs of every (tile, segment) is computed first, in linear time, and a call that
 * would exceed pair_budget is refused before any pair is compared.
 */
#ifndef WELLDUP_TILENEAR_H
#define WELLDUP_TILENEAR_H

#include "welldup_tiledups.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WD_TILENEAR_MAX_K 3

/* device workspace wd_tile_near_dups needs for n_tiles tiles of N wells at distance k (0..3): that of
 * wd_tile_dups_workspace plus 4 (k + 1) bytes per well for k >= 1.  k outside 0..3: WD_ERR_ARG. */
int wd_tile_near_dups_workspace(int64_t N, int n_tiles, int k, size_t *bytes);

/* The near-duplicate clusters of n_tiles resident tiles.  Arguments, checks and error codes as wd_tile_dups;
 * in addition k outside 0..3, L < k + 1 or pair_budget < 0 is WD_ERR_ARG.
 *   k              largest Hamming distance of an edge; 0 runs wd_tile_dups
 *   workspace_dev  device memory of at least wd_tile_near_dups_workspace(N, n_tiles, k) bytes
 *   hash_bits      as wd_tile_dups, applied to the segment fingerprints as well; the result does not depend on
 *                  it (the candidate pairs, and so what pair_budget admits, do)
 *   pair_budget    most candidate pairs (the sum over a segment's buckets of c (c - 1) / 2, c = distinct reads
 *                  in the bucket) one tile may have in one segment; 0 = the default, max(16 N, 2^24).  A call
 *                  that exceeds it returns WD_ERR_UNSUPPORTED, wd_last_error names the tile, the segment, the
 *                  count and the budget; nothing is left behind and the next call works as usual
 *   out_rows       n_tiles HOST rows of 5 + 2*levels + WD_DUPSET_SIZE_BINS int64:
 *                  [PF wells, Clusters, InClusters, Redundant, NearPairs, Local[levels], RingWells[levels], size bins]
 *   labels_dev     nullable; else n_tiles DEVICE pointers to N uint32 labels each (definitions above)
 * Synchronous, on the context's stream; keeps nothing in the context. */
int wd_tile_near_dups(wd_ctx *ctx, int n_tiles, int L,
                      const uint8_t *const *planes, const uint8_t *const *filter, int64_t N, int k,
                      void *workspace_dev, size_t workspace_bytes, int hash_bits, int64_t pair_budget,
                      int64_t *out_rows, uint32_t *const *labels_dev);

#ifdef __cplusplus
}
#endif
#endif /* WELLDUP_TILENEAR_H */
