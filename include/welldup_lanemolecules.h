/*
 * welldup_lanemolecules.h - the best well of each UMI molecule, as a keep mask (libwelldup.so, the `tiledups`
 * translation unit).
 *
 * wd_lane_umi (welldup_laneumi.h) counts how many of a family's "copies" are molecules of their own; wd_lane_keep
 * (welldup_lanekeep.h) keeps one well per family, and so drops every well that the UMI pass has just shown to be a
 * distinct molecule.  Here the UMI pass writes its molecules down, and the keep pass runs on them: one well per
 * molecule survives.
 * Definitions, for one lane, after a successful finish of either kind, on an accumulator with a UMI part (and, for
 * the keep, a quality part).  Family, gathered, Large, molecule, first well, E and max_family are welldup_laneumi.h's;
 * score, best, kept and the rows are welldup_lanekeep.h's; kInvalid is 0xFFFFFFFF; g is a well's global id,
 * tile index * N + its number in the tile; W = max_tiles * N.
 *   mol, molmem   two arrays of W uint32 in the caller's molecule region, mol at its start and molmem
 *                 4 * W bytes, rounded up to 256, behind it.  For the well g:
 *                   not PF, or of a tile never added     mol[g] = kInvalid,  molmem[g] = 0;
 *                   Single (a family of one)             mol[g] = g,         molmem[g] = 0;
 *                   of a gathered family                 mol[g] = the first well of its molecule; molmem[g] = the
 *                                                        molecule's wells - 1 at that first well, 0 elsewhere;
 *                   of a Large family                    mol[g] = label[g],  molmem[g] = members[g] at the root, 0
 *                                                        elsewhere: the family counts as one molecule, as the UMI row
 *                                                        counts it (its copies stay copies).
 *                 This is the form the finish leaves label and members in, with "molecule" for "family": a molecule's
 *                 first well has its smallest id;
 *   molecule part of an accumulator: the region wd_lane_umi_molecules filled last, with its E and max_family
 *                 (wd_lane_molecules_part tells them).  A call of wd_lane_umi_molecules that fails in whatever way
 *                 with a non-null accumulator, any later call of wd_lane_dups_finish or wd_lane_near_dups_finish
 *                 with a non-null accumulator (one that is refused included) and wd_lane_dups_end forget it;
 *   keep by molecule   wd_lane_keep's definitions read with "molecule of two or more wells" for "family": a well is
 *                 kept when it is PF and either its molecule is itself alone or it is the best of its molecule.
 * Identities.  U is wd_lane_umi_molecules' lane row, K wd_lane_keep_molecules' lane row, F the finish's lane row,
 * Singles = F's classes (clusters) of one well:
 *   1. K.PF = K.Kept + K.Dropped = F.PF;
 *   2. K.Dropped = U.UmiRedundant + U.LargeWells - U.LargeFamilies;
 *   3. K.Families = U.Molecules - U.MoleculeSize[0] + U.LargeFamilies;
 *   4. K.Kept = Singles + U.Molecules + U.LargeFamilies;
 *   5. identities 2 to 5 of welldup_lanekeep.h hold as written, with molecules for families (4: SumKept + SumDropped =
 *      the sum over q of weight[bin(q)] x QHist[q]);
 *   6. with E >= U and max_family at or above the largest family, the rows and every mask byte are wd_lane_keep's;
 *   7. K.Dropped <= wd_lane_keep's Dropped; where no two wells of a family have the same score, the wells K drops are
 *      a subset of those wd_lane_keep drops;
 *   8. a lane rebuilt from the same read and UMI planes with filter & mask as its filter, then the same finish and
 *      wd_lane_umi at the same E with max_family at or above the largest family, has UmiRedundant = 0 and Molecules =
 *      Wells: two kept wells of one family lie in different components, so they are more than E apart; a Large family
 *      leaves one well;
 *   9. the rows of wd_lane_umi_molecules are wd_lane_umi's, cell for cell; nothing depends on the order or batching of
 *      the add calls, on hash_bits, on which other passes ran before, on how often the calls are made, or on what the
 *      molecule region held before.
 */
#ifndef WELLDUP_LANEMOLECULES_H
#define WELLDUP_LANEMOLECULES_H

#include "welldup_laneumi.h"
#include "welldup_lanekeep.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Device memory of a molecule region for an accumulator of max_tiles tiles of wells_per_tile wells.  Host arithmetic
 * only.  With W = max_tiles * wells_per_tile and every part rounded up to 256 bytes:
 *     4 * W                               mol: per well, the first well of its molecule
 *   + 4 * W                               molmem: per well, at a molecule's first well its other wells
 * which is 8 bytes per well of the lane.  The argument errors and limits of wd_lane_umi_scratch. */
int wd_lane_molecules_bytes(int max_tiles, int64_t wells_per_tile, size_t *bytes);

/* wd_lane_umi with its preconditions, its errors and its rows, cell for cell; it also fills mol_dev, DEVICE memory of
 * at least wd_lane_molecules_bytes(max_tiles, wells_per_tile) bytes, the caller's, whatever it holds: every word of
 * mol and molmem is written.  On success the accumulator remembers the region, max_e and max_family as its molecule
 * part; the caller keeps the region alive and untouched for as long as wd_lane_keep_molecules is to read it.  The
 * scratch is free to reuse when the call returns.
 * WD_ERR_ARG, changing nothing in device memory and leaving the accumulator without a molecule part: what wd_lane_umi
 * refuses, and a mol_dev that is null, in host memory, smaller than wd_lane_molecules_bytes or overlapping the
 * scratch. */
int wd_lane_umi_molecules(wd_lane_dups *ld, int max_e, int max_family, void *scratch_dev, size_t scratch_bytes,
                          int64_t *lane_row, int64_t *tile_rows, void *mol_dev, size_t mol_bytes);

/* The E and max_family of the accumulator's molecule part, that is of the wd_lane_umi_molecules call whose molecules
 * wd_lane_keep_molecules would read now.  Host arithmetic only.  WD_ERR_ARG: a null pointer, no molecule part. */
int wd_lane_molecules_part(wd_lane_dups *ld, int *max_e, int *max_family);

/* wd_lane_keep's contract, scratch (wd_lane_keep_scratch), rows and masks, by molecule: the call reads the molecule
 * part where wd_lane_keep reads the label array and the members.  A Large family is one molecule.
 * WD_ERR_ARG, changing nothing: what wd_lane_keep refuses, an accumulator without a molecule part, a scratch that
 * overlaps the molecule region. */
int wd_lane_keep_molecules(wd_lane_dups *ld, int min_q, void *scratch_dev, size_t scratch_bytes, int64_t *lane_row,
                           int64_t *tile_rows, uint8_t *const *keep_dev);

#ifdef __cplusplus
}
#endif
#endif /* WELLDUP_LANEMOLECULES_H */
