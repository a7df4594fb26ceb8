/*
 * welldup_sets.h - duplicate sets of every tile (libwelldup.so, the `sets` translation unit).
 *
 * With every well a centre (wd_targets_from_coords(..., centres = NULL, ...)) the scan sees every
 * duplicate pair of a tile, so the wells can be grouped into duplicate sets and the duplication of a
 * lane measured instead of estimated (the reference's headline figures are estimates from sampled
 * targets: count_well_duplicates.py:108-125).  Definitions, for one tile:
 *   vertices     wells that pass the filter (byte & 1, bcl_direct_reader.py:246);
 *   edge, level  PF wells a, b with b in ring l of a or a in ring l of b and dist(a, b) <= k (the scan's
 *                metric and k); a pair in several rings has the smallest of them as its level;
 *   Sets[l]      connected components of at least two wells in the graph of the edges of level <= l
 *                (single linkage); InSets[l] = wells in them; Redundant[l] = InSets[l] - Sets[l];
 *                A well that names itself in one of its rings (nbr[slot] == centre) is no pair: the scan counts
 *                and logs that record as it does any duplicate (Dups, edges_out), the sets ignore it.
 *   label        of a well: the smallest well index of its outermost-level set; a PF well in no set is
 *                labelled with its own index, a non-PF well with WD_INVALID_TARGET.
 */
#ifndef WELLDUP_SETS_H
#define WELLDUP_SETS_H

#include "welldup.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WD_DUPSET_SIZE_BINS 8          /* set sizes 2..8 and >= 9 */

/* device workspace wd_dup_sets needs for n_tiles tiles of N wells (two uint32 per well and tile, plus
 * counters) */
int wd_dup_sets_workspace(int64_t N, int n_tiles, size_t *bytes);

/* The scan of wd_count_tiles (same planes/filter/N/mode/k contract, same out_tile rows) plus the
 * duplicate sets of every tile.  Targets must be every well (T == N, centre[t] == t), else WD_ERR_ARG.
 * The filters must be in device memory (they are read again by the sets kernels).
 *   workspace_dev   device memory of at least wd_dup_sets_workspace(N, n_tiles) bytes
 *   out_sets   n_tiles HOST rows of 1 + 3*levels + WD_DUPSET_SIZE_BINS int64:
 *              [PF wells, Sets[0..levels), InSets[0..levels), Redundant[0..levels), size bins]
 *              (the size bins count the sets of the outermost level)
 *   labels_dev nullable; else n_tiles DEVICE pointers to N uint32 labels each (definitions above)
 *   edge_cap   0 = automatic; otherwise the first attempt's hit-log capacity (tests force regrowth)
 *   edges_out  nullable: hit records processed
 * The context's hit log is the edge buffer: a scan whose duplicates do not fit it is repeated once with
 * a log of the size it reported; if that does not fit in half the free device memory the tiles are
 * scanned one at a time, and a tile that alone does not fit fails the call with WD_ERR_NOMEM.
 * WD_ERR_STATE: the hit log disagrees with the scan's Dups counters.
 * Synchronous.  Leaves the hit log disabled. */
int wd_dup_sets(wd_ctx *ctx, int n_tiles, int L, int mode, int k,
                const uint8_t *const *planes, const uint8_t *const *filter, int64_t N,
                void *workspace_dev, size_t workspace_bytes, int64_t edge_cap,
                int64_t *out_tile, int64_t *out_sets, uint32_t *const *labels_dev, int64_t *edges_out);

#ifdef __cplusplus
}
#endif
#endif /* WELLDUP_SETS_H */
