/*
 * welldup_laneumi.h - a lane's duplicates split by molecular identifier (libwelldup.so, the `tiledups` translation unit).
 *
 * Every figure of the lane passes rests on "two PF wells with the same read, or reads within Hamming K, are copies of
 * one molecule".  A library with a unique molecular identifier (UMI: a few random bases in an index read or at the
 * start of read 1) says more: two wells with the same insert and different UMIs are two molecules.  wd_lane_umi looks
 * into every family the last finish left and groups its wells by their UMI read: how many of the "copies" are copies.
 * Definitions, for one lane, after a successful finish of either kind (read, PF, the global id, the labels and members
 * as in welldup_lanegc.h):
 *   UMI read      of a well: its decoded bases over the U UMI cycles, 1 <= U <= WD_LANEUMI_MAX_CYCLES.  Alphabet and
 *                 packing are welldup_laneindex.h's: two uint32 of ten 3-bit codes, N a fifth symbol, N == N.  The
 *                 cycles may overlap the scanned cycles or not;
 *   d(a, b)       the number of UMI cycles at which the codes of two keys differ;
 *   family        a root r (label(r) == id(r), members(r) >= 1) with its copies: n = members(r) + 1 wells.  Gathered:
 *                 2 <= n <= max_family, max_family the caller's, 2 .. WD_LANEUMI_MAX_FAMILY.  Large: n > max_family; it
 *                 is counted in LargeFamilies / LargeWells and never looked into;
 *   molecule      within a gathered family, a connected component of its wells under "d <= E", E the caller's,
 *                 0 .. WD_LANEUMI_MAX_E.  E = 0 is equality of the UMI read; E >= 1 is single linkage, the only
 *                 error-tolerant rule whose result does not depend on an order (the count-based "directional" rule
 *                 does, and is not offered).  Its first well is its smallest global id;
 *   tile row      WD_LANEUMI_TILE_COLS = 3 int64 per tile index [Wells, UmiRedundant, Lone], each counted by the
 *                 well's own tile: Wells the wells of gathered families, UmiRedundant those that are not the first well
 *                 of their molecule, Lone those whose molecule is themselves alone.  Zero for an index never added;
 *   lane row      WD_LANEUMI_LANE_COLS = 27 int64: the three tile columns summed, then [Families, Molecules,
 *                 DistinctUmis, SplitFamilies, SplitWells, WithN, LargeFamilies, LargeWells], MolPerFamily[8],
 *                 MoleculeSize[8].  Families the gathered families; Molecules theirs; DistinctUmis the sum over gathered
 *                 families of their distinct UMI reads (Molecules at E = 0, whatever E is); SplitFamilies / SplitWells
 *                 the gathered families of two or more molecules and their wells; WithN the wells of gathered families
 *                 whose UMI read holds an N; MolPerFamily the gathered families by their number of molecules,
 *                 MoleculeSize the molecules by their number of wells, both in bins of 1, 2, 3, 4, 5-8, 9-16, 17-64 and
 *                 65 or more.
 * Identities:
 *   1. Families + LargeFamilies = the groups of two or more wells of the last finish's lane row (identity 1 of
 *      welldup_laneconsensus.h with the pairs inside Families);
 *   2. Wells + LargeWells = Classes + Redundant of that row;
 *   3. Families <= Molecules <= DistinctUmis <= Wells;
 *   4. UmiRedundant = Wells - Molecules;
 *   5. the sum of MolPerFamily = Families;
 *   6. the sum of MoleculeSize = Molecules;
 *   7. MoleculeSize[0] = Lone;
 *   8. SplitFamilies = Families - MolPerFamily[0];
 *   9. the tile rows sum to the lane row's first three columns;
 *  10. Molecules and SplitFamilies never grow with E;
 *  11. DistinctUmis does not depend on E;
 *  12. at E = 0, Molecules = DistinctUmis;
 *  13. at E >= U, Molecules = Families;
 *  14. under equality labels, UMI cycles that are a subset of the scanned cycles give Molecules = Families and Lone = 0;
 *  15. with max_family at or above the largest family and E = 0, Molecules = GroupSpans of wd_lane_index_finish over
 *      the same cycles;
 *  16. nothing depends on the order or batching of the add calls, on hash_bits, on which other passes ran before, on
 *      how often the call is made, or on the order in which a family's members landed in the list.
 */
#ifndef WELLDUP_LANEUMI_H
#define WELLDUP_LANEUMI_H

#include "welldup_lanedups.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WD_LANEUMI_MAX_CYCLES 20
#define WD_LANEUMI_MAX_E 3
#define WD_LANEUMI_MAX_FAMILY 1024
#define WD_LANEUMI_LANE_COLS 27
#define WD_LANEUMI_TILE_COLS 3
#define WD_LANEUMI_BINS 8

/* Device memory the UMI part of an accumulator of max_tiles tiles of N wells needs for UMI reads of U cycles.  Host
 * arithmetic only.  With W = max_tiles * N and every part rounded up to 256 bytes:
 *     8 * max_tiles * U                   the plane pointers of a call
 *   + 4 * max_tiles                       the tile indices of a call
 *   + 8 * W                               key: the UMI read of every well
 * which is 8 bytes per well plus the pointer tables.  The limits of wd_lane_dups_workspace hold (with U for L); U
 * outside 1 .. 20 or a null pointer: WD_ERR_ARG. */
int wd_lane_umi_workspace(int64_t N, int max_tiles, int U, size_t *bytes);

/* Gives the accumulator a UMI part: once, before any finish.  workspace_dev: DEVICE memory of at least
 * wd_lane_umi_workspace(N, max_tiles, U) bytes, the caller's until wd_lane_dups_end.  An accumulator may carry an index
 * part (welldup_laneindex.h) and a UMI part at once; neither touches the other's memory.  WD_ERR_ARG, changing nothing:
 * U outside 1 .. 20, a call after a finish, a second call, a workspace that is null, in host memory or too small. */
int wd_lane_umi_begin(wd_lane_dups *ld, int U, void *workspace_dev, size_t workspace_bytes);

/* The UMI planes of n_tiles resident tiles: umi_planes[i * U + c] is cycle c of tile tile_index[i], N bytes of DEVICE
 * memory, a plane per cycle (well_stride 1).  Independent of wd_lane_dups_add in order and batching; before any finish.
 * The planes are free to reuse when the call returns.  WD_ERR_ARG, changing nothing: a call without wd_lane_umi_begin
 * or after a finish, a tile index out of range or given twice (in this call or an earlier one), a null or host
 * pointer, well_stride 4. */
int wd_lane_umi_add(wd_lane_dups *ld, int n_tiles, const int *tile_index, const uint8_t *const *umi_planes);

/* Device memory wd_lane_umi needs.  Host arithmetic only.  With W = max_tiles * wells_per_tile and every part rounded
 * up to 256 bytes:
 *     1536 * max_tiles                    per tile index 64 copies of 3 uint64: the tile row
 *   + 16384                               64 copies of 32 uint64: the lane's counters
 *   + 8192                                64 copies of 16 uint64: what the gather counts (pairs, large families)
 *   + 256                                 the cursor of the reservation
 *   + 4 * max_tiles                       the tile indices that were added
 *   + 4 * W                               per well: where its family's range begins
 *   + 4 * W                               the member list and the family table in one region
 * which is 8 bytes per well of the lane plus the counters.
 * A negative argument or a null pointer: WD_ERR_ARG; max_tiles > 65535 or W >= 2^32 - 1: WD_ERR_UNSUPPORTED. */
int wd_lane_umi_scratch(int max_tiles, int64_t wells_per_tile, size_t *bytes);

/* After a successful finish of either kind and before wd_lane_dups_end, any number of times and with any max_e and
 * max_family, before or after every other pass.  lane_row (WD_LANEUMI_LANE_COLS int64) and tile_rows (max_tiles x
 * WD_LANEUMI_TILE_COLS int64) are HOST memory.  scratch_dev: DEVICE memory of at least wd_lane_umi_scratch(max_tiles,
 * wells_per_tile) bytes, the caller's, whatever it holds; free to reuse when the call returns.  The call reads the
 * label array, the members and the UMI keys and writes nothing but its scratch: in particular not the accumulator's
 * table, which the index part uses.  Synchronous on the context's stream.  A lane without wells or tiles: WD_OK with
 * zeros.
 * WD_ERR_ARG, changing nothing: a call before a successful finish or without wd_lane_umi_begin, a set of tiles given to
 * wd_lane_umi_add that differs from the set given to wd_lane_dups_add (wd_last_error names one such tile), max_e
 * outside 0 .. 3, max_family outside 2 .. 1024, a null lane_row or tile_rows, a scratch region that is null, in host
 * memory or too small. */
int wd_lane_umi(wd_lane_dups *ld, int max_e, int max_family, void *scratch_dev, size_t scratch_bytes,
                int64_t *lane_row, int64_t *tile_rows);

#ifdef __cplusplus
}
#endif
#endif /* WELLDUP_LANEUMI_H */
