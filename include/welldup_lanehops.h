/*
 * welldup_lanehops.h - which libraries a lane's duplicate copies join (libwelldup.so, the `tiledups` translation unit).
 *
 * welldup_laneindex.h counts the classes that hold wells of more than one index read and the wells in them; it does
 * not say whether a copy's index read differs from its original's by a read error or by a whole other index, in
 * which of the two index reads, nor between which libraries the copies pass.  wd_lane_hops holds the index key of
 * every redundant well against its root's and answers all three from the labels that the last finish left and the
 * keys of the index workspace.
 * Definitions, for one lane, after a successful finish of either kind:
 *   PF wells, global id, labels   as welldup_lanemismatch.h;
 *   root, pair    the root of a PF well g is label(g); every PF well g with label(g) != g is a pair, held against its
 *                 root: exactly Redundant pairs, one per redundant well (the convention of welldup_lanemismatch.h);
 *   index key     welldup_laneindex.h's: index cycle c, 0 <= c < I, lies at bits 32 (c / 10) + 3 (c % 10) .. + 2 of
 *                 the 64-bit key, codes A C G T N = 0 .. 4, N == N;
 *   parts         split s, 1 <= s <= I: part 1 is the index cycles 0 .. s - 1, part 2 the cycles s .. I - 1; s = I is a
 *                 single index and part 2 is empty.  d1 and d2: the number of cycles of each part at which the codes
 *                 of the two keys differ;
 *   state of a part   for max_e = E, 0 <= E <= WD_LANEHOPS_MAX_E: 0 Same (d = 0), 1 Near (1 <= d <= E), 2 Far (d > E).
 *                 An empty part 2 is Same.  Near is what a demultiplexer forgives as a read error; Far is another
 *                 index;
 *   state of a pair   3 * state1 + state2, 0 .. 8;
 *   tile row      WD_LANEHOPS_TILE_COLS int64 per tile index [Pairs, SameTile, Hop1, Hop2], attributed to the tile of
 *                 the COPY g; zero for an index never added.  SameTile: the root lies on the copy's tile; Hop1: exactly
 *                 one part is Far; Hop2: both are;
 *   lane row      WD_LANEHOPS_LANE_COLS int64: the four tile columns summed over the tiles, then State[0..8];
 *   listing       M distinct index keys of the caller's, 0 <= M <= WD_LANEHOPS_MAX_LISTED.  The rank of a well is the
 *                 position of its key in that list, or M ("Other") when the key is not in it;
 *   matrix        (M + 1) x (M + 1) int64: matrix[a][b] = the pairs whose root has rank a and whose copy has rank b,
 *                 whatever their state.
 * Identities: the sum of State = Pairs = Redundant of the last finish's lane row, and per tile Pairs = LaneRedundant
 * of that finish's tile row; Hop1 = State[2] + State[5] + State[6] + State[7]; Hop2 = State[8]; the tile rows sum to
 * the lane row's first four columns; the sum of matrix = Pairs; when every PF well's key is listed, row M and column M
 * are zero and the diagonal sums to State[0] (a listed key is the whole key, so equal ranks <=> equal keys);
 * s = I gives State[k] = 0 for k % 3 != 0; E at or above a part's length gives no Far state in that part; under
 * equality labels, index cycles that are a subset of the scanned cycles give State[0] = Pairs; M = 0 gives the 1 x 1
 * matrix [Pairs]; nothing depends on the order or batching of the add calls, on hash_bits, on the order of the
 * listed keys beyond the ranks it defines, or on whether wd_lane_index_finish ran before.
 */
#ifndef WELLDUP_LANEHOPS_H
#define WELLDUP_LANEHOPS_H

#include "welldup_laneindex.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WD_LANEHOPS_MAX_E 3
#define WD_LANEHOPS_STATES 9
#define WD_LANEHOPS_TILE_COLS 4
#define WD_LANEHOPS_LANE_COLS (WD_LANEHOPS_TILE_COLS + WD_LANEHOPS_STATES)
#define WD_LANEHOPS_MAX_LISTED 1024

/* Device memory wd_lane_hops needs for an accumulator of max_tiles tiles and M listed keys.  Host arithmetic only.
 * With every part rounded up to 256 bytes:
 *     2048 * max_tiles                    per tile index 64 copies of 4 uint64: Pairs, SameTile, Hop1, Hop2
 *   + 8192                                State, 64 copies of 16 uint64 (9 used)
 *   + 4 * max_tiles                       the tile indices that were added
 *   + 8 * M                               the listed keys, sorted
 *   + 2 * M                               the rank of each sorted key: its position in the caller's list
 *   + 8 * (M + 1) * (M + 1)               the matrix, one copy: a workgroup adds to it once per occupied entry of
 *                                         its own table
 * (M = 1024: 8.4 MB and 2 KB per tile).  It does not depend on the wells of a tile.
 * A negative max_tiles, M outside 0 .. WD_LANEHOPS_MAX_LISTED or a null pointer: WD_ERR_ARG; max_tiles > 65535:
 * WD_ERR_UNSUPPORTED. */
int wd_lane_hops_scratch(int max_tiles, int M, size_t *bytes);

/* After a successful finish of either kind of an accumulator with an index part, and before wd_lane_dups_end; any
 * number of times and with any split, max_e and listing, before or after wd_lane_index_finish.  listed_keys (M
 * uint64, may be null when M is 0), lane_row (WD_LANEHOPS_LANE_COLS int64), tile_rows (max_tiles x
 * WD_LANEHOPS_TILE_COLS int64) and matrix ((M + 1) x (M + 1) int64, row = the root's rank) are HOST memory.
 * scratch_dev: DEVICE memory of at least wd_lane_hops_scratch bytes, the caller's; free to reuse when the call
 * returns.  The call reads the label array and the index workspace's keys and writes nothing but its scratch: the
 * table, the per-well slot word and the rest of the index workspace stay as they are.  Synchronous on the context's
 * stream.
 * WD_ERR_ARG, changing nothing: a call before a successful finish (a near finish refused over budget is none) or
 * without wd_lane_index_begin; a set of tile indices given to wd_lane_index_add that differs from the set given to
 * wd_lane_dups_add (wd_last_error names one such tile, in wd_lane_index_finish's words); split outside 1 .. I; max_e
 * outside 0 .. WD_LANEHOPS_MAX_E; M outside 0 .. WD_LANEHOPS_MAX_LISTED; a listed key given twice (wd_last_error
 * names it); a listed key no well can carry - a code above 4, a bit outside the codes, or a code that is not zero at
 * or past cycle I; a null pointer; a scratch region that is null, in host memory or too small. */
int wd_lane_hops(wd_lane_dups *ld, int split, int max_e, int M, const uint64_t *listed_keys, void *scratch_dev,
                 size_t scratch_bytes, int64_t *lane_row, int64_t *tile_rows, int64_t *matrix);

#ifdef __cplusplus
}
#endif
#endif /* WELLDUP_LANEHOPS_H */
