/*
 * welldup_tiledups.h - read classes of every tile (libwelldup.so, the `tiledups` translation unit).
 *
 * The scan and the duplicate sets (welldup_sets.h) only see duplicates inside the rings.  This groups the
 * wells of a tile by their whole read, wherever on the tile they lie, and says how much of that
 * duplication is local.  Definitions, for one tile and the scanned cycles:
 *   read         of a well: byte 0 is N, any other byte is "ACGT"[byte & 3] (bcl_direct_reader.py:352-361);
 *                quality bits never matter, N == N;
 *   vertices     wells that pass the filter (byte & 1), as for the duplicate sets;
 *   class        a maximal group of at least two PF wells with equal reads.  Classes, InClasses (the wells
 *                in them), Redundant = InClasses - Classes; size bins 2..8 and >= 9;
 *   label        of a well: the smallest well index of its class; its own index for a PF well in no
 *                class; WD_INVALID_TARGET for a non-PF well;
 *   Local[l]     l = 1..levels, cumulative: wells in a class that have a classmate m with m in a ring <= l
 *                of the well or the well in a ring <= l of m (the rule welldup_sets.h uses for an edge);
 *   RingWells[l] over the wells in classes, the sum of the sizes of their rings <= l: what Local[l] would
 *                be for classmates spread evenly is RingWells[l] / (InClasses * (N - 1)) per classmate.
 * Classes are by equality only; the near-duplicate clusters of a whole tile (Hamming distance <= K) are
 * wd_tile_near_dups in welldup_tilenear.h.
 */
#ifndef WELLDUP_TILEDUPS_H
#define WELLDUP_TILEDUPS_H

#include "welldup_sets.h"

#ifdef __cplusplus
extern "C" {
#endif

/* device workspace wd_tile_dups needs for n_tiles tiles of N wells: per tile a hash table of the smallest
 * power of two >= 2 N slots of 8 bytes and 20 bytes per well, plus counters and pointer tables */
int wd_tile_dups_workspace(int64_t N, int n_tiles, size_t *bytes);

/* The read classes of n_tiles resident tiles.  planes / filter / N as for wd_count_tiles, but every pointer
 * must be a DEVICE pointer, a plane per cycle (option "well_stride" 4: WD_ERR_UNSUPPORTED).  The targets
 * must be every well (T == N, centre[t] == t), else WD_ERR_ARG: their rings give Local and RingWells.
 *   workspace_dev  device memory of at least wd_tile_dups_workspace(N, n_tiles) bytes
 *   hash_bits      0 = all; 1..32: only that many bits of a read's fingerprint are used, so that unequal
 *                  reads share a fingerprint (tests).  Equality is decided on the reads themselves: the
 *                  result does not depend on hash_bits.
 *   out_rows       n_tiles HOST rows of 4 + 2*levels + WD_DUPSET_SIZE_BINS int64:
 *                  [PF wells, Classes, InClasses, Redundant, Local[levels], RingWells[levels], size bins]
 *   labels_dev     nullable; else n_tiles DEVICE pointers to N uint32 labels each (definitions above)
 * Synchronous, on the context's stream; keeps nothing in the context. */
int wd_tile_dups(wd_ctx *ctx, int n_tiles, int L,
                 const uint8_t *const *planes, const uint8_t *const *filter, int64_t N,
                 void *workspace_dev, size_t workspace_bytes, int hash_bits,
                 int64_t *out_rows, uint32_t *const *labels_dev);

#ifdef __cplusplus
}
#endif
#endif /* WELLDUP_TILEDUPS_H */
