/*
 * welldup_lanedups.h - read classes across all tiles of a lane (libwelldup.so, the `tiledups` translation unit).
 *
 * welldup_tiledups.h groups the PF wells of one tile by their read.  A PCR copy of a molecule lands anywhere on
 * the lane, so on a lane of 96 tiles only about one such pair in 96 falls on one tile: the duplication of the
 * library shows in the classes of the LANE.  A lane is streamed through device memory in batches of tiles
 * whose planes are gone when the next batch arrives, so this is an accumulator: wd_lane_dups_add keeps a packed
 * copy of every read (3 bits a cycle) and one hash table for the lane, and decides equality on the packed rows.
 * Definitions, for one lane and the scanned cycles:
 *   read, vertices  as welldup_tiledups.h: byte 0 is N, any other byte "ACGT"[byte & 3]; quality bits never
 *                matter, N == N; the vertices are the wells that pass the filter (byte & 1);
 *   global id    of a well: tile_index * N + well; tile_index is the caller's number for the tile, in
 *                0 .. max_tiles - 1, each used at most once;
 *   lane class   a maximal group of at least two PF wells of the lane with equal reads, on whatever tiles;
 *   label        of a well: the smallest global id of its class; its own global id for a PF well in no class;
 *                WD_INVALID_TARGET for a non-PF well (and for every well of a tile index never added);
 *   lane row     WD_LANEDUPS_LANE_COLS int64: [PF, Classes, InClasses, Redundant, CrossTileClasses, TileSpans,
 *                size bins 2..8 and >= 9].  Redundant = InClasses - Classes; TileSpans = the sum over the classes
 *                of the number of distinct tiles a class touches; CrossTileClasses = classes touching >= 2 tiles;
 *   tile row     WD_LANEDUPS_TILE_COLS int64, one per tile index (zeros for an index never added):
 *                [PF, InLane, InTile, TileRedundant, LaneRedundant].  InLane: the tile's wells in a lane class;
 *                InTile: those with a classmate on the same tile; TileRedundant: wells with a classmate of
 *                smaller well index on the same tile; LaneRedundant: wells that are not the smallest global id
 *                of their class.
 * The sum of LaneRedundant is Redundant; the sum of TileRedundant is InClasses - TileSpans, the redundancy within
 * tiles; TileSpans - Classes is the redundancy across tiles.  Per tile, InTile and TileRedundant are InClasses
 * and Redundant of wd_tile_dups on that tile.
 */
#ifndef WELLDUP_LANEDUPS_H
#define WELLDUP_LANEDUPS_H

#include "welldup_tiledups.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WD_LANEDUPS_LANE_COLS (6 + WD_DUPSET_SIZE_BINS)
#define WD_LANEDUPS_TILE_COLS 5

typedef struct wd_lane_dups wd_lane_dups;

/* Device workspace of an accumulator for max_tiles tiles of N wells and L scanned cycles.  Host arithmetic only:
 * no GPU is needed.  With W = max_tiles * N wells of capacity, R = ceil(L / 10) words of ten 3-bit codes per
 * read, S = the smallest power of two >= max(64, 2 W) slots, and every part rounded up to 256 bytes:
 *     512 * (8 * max_tiles + 16)          counters: 64 copies of 8 uint64 per tile and of 16 for the lane
 *   + 8 * max_tiles * L                   plane pointers of one wd_lane_dups_add
 *   + 8 * max_tiles + 8 * max_tiles       filter and label pointers
 *   + 4 * max_tiles                       tile indices
 *   + 8 * S                               the lane's table
 *   + 4 * R * W                           packed rows, a well's R words side by side
 *   + 8 * W + 4 * W + 4 * W               fingerprint / slot, label, members
 * (a HiSeq 4000 lane, 112 x 4 309 253 wells: 8.6 GB of table, 27.9 GB in all at 51 cycles, 47.2 GB at 151).
 * max_tiles * N >= 2^32 - 1 (labels are 32-bit), L > 1024 or max_tiles > 65535: WD_ERR_UNSUPPORTED.  A negative
 * argument or bytes == NULL: WD_ERR_ARG. */
int wd_lane_dups_workspace(int64_t N, int max_tiles, int L, size_t *bytes);

/* Starts a lane in the caller's workspace_dev (DEVICE memory of at least wd_lane_dups_workspace bytes, the
 * caller's to free after wd_lane_dups_end; too small: WD_ERR_ARG).  hash_bits as wd_tile_dups: 0 = all, 1..32 =
 * only that many bits of a read's fingerprint are used (tests); the result never depends on it.  The context
 * gains no state: the handle in *out holds the host side of the accumulator. */
int wd_lane_dups_begin(wd_ctx *ctx, int64_t N, int max_tiles, int L, void *workspace_dev, size_t workspace_bytes,
                       int hash_bits, wd_lane_dups **out);

/* Adds n_tiles resident tiles: tile_index[i] is tile i's number in the lane, planes (n_tiles x L) and filter
 * (n_tiles) are DEVICE pointers, a plane per cycle, as wd_tile_dups takes them.  No targets are needed.  Any number of
 * calls, indices in any order: the result does not depend on either.  When the call returns the planes may be
 * overwritten or freed: nothing it keeps points into them.  A repeated or out-of-range tile index, a call after
 * wd_lane_dups_finish, a null or host pointer, or option "well_stride" 4: WD_ERR_ARG, and the call changes
 * nothing. */
int wd_lane_dups_add(wd_lane_dups *ld, int n_tiles, const int *tile_index,
                     const uint8_t *const *planes, const uint8_t *const *filter);

/* Once per lane (a second call: WD_ERR_ARG; a call refused for a null row does not count): the lane row and
 * max_tiles tile rows to HOST memory.  labels_dev: nullable; else max_tiles entries, each null (skipped) or a DEVICE pointer to N
 * uint32 labels (definitions above). */
int wd_lane_dups_finish(wd_lane_dups *ld, int64_t *lane_row, int64_t *tile_rows, uint32_t *const *labels_dev);

/* Frees the host handle only (NULL is fine), at any point: an error path can drop a half-built lane. */
void wd_lane_dups_end(wd_lane_dups *ld);

/* Every call is synchronous on the context's stream. */

#ifdef __cplusplus
}
#endif
#endif /* WELLDUP_LANEDUPS_H */
