/*
 * welldup_laneindex.h - a lane's duplication per library (libwelldup.so, the `tiledups` translation unit).
 *
 * welldup_lanedups.h and welldup_lanenear.h end in figures for a LANE.  A production lane is a pool of libraries,
 * told apart by the index reads that lie a few cycles further on in the same files; the lane's duplication is a
 * read-weighted mixture of theirs and describes none of them.  This interface groups the wells of a lane by their
 * index read, without a sample sheet, and splits what the last finish found by those groups; the classes that hold
 * wells of more than one index read - the signature of index hopping and cross-contamination - are counted too.
 * Definitions, for one lane:
 *   index read   of a well: its decoded bases over the I index cycles, 1 <= I <= WD_LANEINDEX_MAX_CYCLES, in the
 *                alphabet of welldup_tiledups.h: byte 0 is N, any other byte "ACGT"[byte & 3]; N == N; quality bits
 *                never matter.  The index cycles may overlap the scanned cycles or not;
 *   index key    two uint32 words of ten 3-bit codes each (A C G T N = 0 1 2 3 4, cycle j of a word at bits
 *                3 j .. 3 j + 2: the packed-row format of the accumulator), delivered as one uint64 with the first
 *                word low.  Codes past cycle I are zero, so equal keys <=> equal index reads;
 *   group        all PF wells of the lane with equal index reads; a non-PF well is in no group.  PF is the filter
 *                wd_lane_dups_add saw;
 *   labels       whatever the last successful finish left in the accumulator: class labels after
 *                wd_lane_dups_finish, cluster labels after wd_lane_near_dups_finish with k >= 1.  "Class" below
 *                means either;
 *   subgroup     the wells of one class that lie in one group;
 *   group row    WD_LANEINDEX_GROUP_COLS int64 [PF, InLane, InGroup, GroupRedundant, Mixed], and the group's key.
 *                InLane: the group's wells in a class; InGroup: those whose subgroup has >= 2 wells; GroupRedundant:
 *                those that are not the smallest global id of their subgroup; Mixed: those whose class holds a well
 *                of another group;
 *   lane index row  WD_LANEINDEX_LANE_COLS int64 [Groups, Listed, GroupSpans, MixedClasses, MixedWells].
 *                GroupSpans: the sum over the classes of the number of distinct groups a class touches;
 *                MixedClasses: classes touching >= 2 groups; MixedWells: the sum of Mixed;
 *   listing      a group is listed when PF >= min_pf; all other groups are summed, column by column, into one
 *                Other row.  Listed rows come in no particular order.
 * Identities: the sum of PF over the listed rows and Other is the lane's PF; the sum of InLane is InClasses; the
 * sum of GroupRedundant is InClasses - GroupSpans, the redundancy within libraries, and GroupSpans - Classes the
 * redundancy across them; GroupSpans >= Classes, with equality <=> MixedClasses = 0 <=> every Mixed = 0; a lane
 * with a single index read has one row [PF, InClasses, InClasses, Redundant, 0]; under equality labels, index
 * cycles that are a subset of the scanned cycles give Mixed = 0 everywhere.
 */
#ifndef WELLDUP_LANEINDEX_H
#define WELLDUP_LANEINDEX_H

#include "welldup_lanenear.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WD_LANEINDEX_MAX_CYCLES 20
#define WD_LANEINDEX_GROUP_COLS 5
#define WD_LANEINDEX_LANE_COLS 5

/* Device workspace of the index part of an accumulator for max_tiles tiles of N wells and I index cycles.  Host
 * arithmetic only.  With W = max_tiles * N and every part rounded up to 256 bytes:
 *     4096 + 4096 + 256                   counters: 64 copies of 8 uint64 for the lane index row and for Other,
 *                                         and the number of listed groups
 *   + 8 * max_tiles * I                   plane pointers of one wd_lane_index_add
 *   + 4 * max_tiles                       tile indices
 *   + 8 * W                               the index key of every well
 *   + 4 * W                               the group label of every well (the smallest global id of its group)
 *   + 20 * W                              5 uint32 counters per well, used at the group representatives
 * that is 32 bytes per well of capacity (a HiSeq 4000 lane, 112 x 4 309 253 wells at I = 8: 15.4 GB).  Nothing
 * else is allocated: after a finish the accumulator's own table is dead and holds the groups' table, then the
 * subgroups' table, then the list of listed groups and the rows on their way to the host; its 8-byte fingerprint
 * / slot word per well is dead too and holds a well's slot in those tables.
 * Errors as wd_lane_dups_workspace (with I for L); I outside 1 .. WD_LANEINDEX_MAX_CYCLES: WD_ERR_ARG. */
int wd_lane_index_workspace(int64_t N, int max_tiles, int I, size_t *bytes);

/* Gives the accumulator an index part of I cycles in workspace_dev (DEVICE memory of at least
 * wd_lane_index_workspace bytes, the caller's to free after wd_lane_dups_end).  Before the first wd_lane_dups_add or
 * after it, but before any finish, and once per accumulator: otherwise WD_ERR_ARG. */
int wd_lane_index_begin(wd_lane_dups *ld, int I, void *workspace_dev, size_t workspace_bytes);

/* Packs the index keys of n_tiles resident tiles: tile_index as wd_lane_dups_add takes it, index_planes n_tiles x I
 * DEVICE pointers, a plane per index cycle.  Independent of wd_lane_dups_add in order and in batching: a tile's
 * index planes may come before its reads, after them, or in another call.  When the call returns the planes may be
 * overwritten or freed.  A repeated or out-of-range tile index, a call before wd_lane_index_begin or after a
 * finish, a null or host pointer, or option "well_stride" 4: WD_ERR_ARG, and the call changes nothing. */
int wd_lane_index_add(wd_lane_dups *ld, int n_tiles, const int *tile_index, const uint8_t *const *index_planes);

/* After a successful finish of either kind and before wd_lane_dups_end, any number of times (the result is the same
 * function of min_pf and cap each time).  lane_index_row (WD_LANEINDEX_LANE_COLS int64), other_row
 * (WD_LANEINDEX_GROUP_COLS int64), group_rows (cap x WD_LANEINDEX_GROUP_COLS int64), group_keys (cap uint64) and
 * n_listed are HOST memory; group_rows and group_keys may be null when cap is 0.  min_pf <= 1 lists every group.
 * WD_ERR_ARG, changing nothing: a call before a successful finish or before wd_lane_index_begin, a null pointer, a
 * negative cap, or a set of tile indices given to wd_lane_index_add that differs from the set given to
 * wd_lane_dups_add (wd_last_error names one such tile).  More than cap groups with PF >= min_pf:
 * WD_ERR_UNSUPPORTED, their number in *n_listed and in wd_last_error, nothing else delivered. */
int wd_lane_index_finish(wd_lane_dups *ld, int64_t min_pf, int64_t cap, int64_t *lane_index_row, int64_t *other_row,
                         int64_t *group_rows, uint64_t *group_keys, int64_t *n_listed);

/* Every call is synchronous on the context's stream. */

#ifdef __cplusplus
}
#endif
#endif /* WELLDUP_LANEINDEX_H */
