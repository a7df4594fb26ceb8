/*
 * welldup_lanequality.h - a lane's reported base quality against its duplicate copies (libwelldup.so, the `tiledups`
 * translation unit).
 *
 * welldup_lanemismatch.h reads a lane's error profile off its own copies: at which cycles and by which substitutions
 * copies of one molecule differ.  It does not say whether the instrument knew: every byte of a base-call plane
 * carries a quality in its upper six bits, and every other interface of this library throws it away.  This one keeps
 * a second packed array beside the accumulator's rows - the quality of every well at every scanned cycle, reduced to
 * the caller's bins - and, after a finish, counts the (pair, cycle) observations by the bins of the two wells, all of
 * them and those at which the two bases differ: an empirical quality table, the error rate observed among copies per
 * reported quality bin, which base-quality recalibration computes from an alignment.  It also tells whether the pairs
 * at distance 1 .. K are errors (the mismatching base is the one of low quality) or other molecules (both confident).
 * Definitions, for one lane, beside those of welldup_lanemismatch.h:
 *   quality       of a well at a scanned cycle: byte >> 2, 0 .. 63.  A no-call (byte 0) has quality 0;
 *   bins          n_bins (1 .. WD_LANEQUALITY_MAX_BINS) lower edges, ascending, edges[0] == 0, edges[i] <= 63;
 *                 bin(q) = the largest i with edges[i] <= q, so every value has a bin.  Equal edges are allowed: the
 *                 earlier of them is an empty bin.  On an instrument that reports a few quality levels the edges
 *                 are its levels and the bins are exact;
 *   QHist         WD_LANEQUALITY_VALUES int64: the (PF well, scanned cycle) observations of the tiles given to
 *                 wd_lane_qual_add by raw quality.  PF is the filter that call saw.  It depends on neither the
 *                 labels nor max_d nor the bins;
 *   pair, root, d, profiled pair, max_d     exactly as welldup_lanemismatch.h;
 *   Obs           8 x 8 int64: Obs[a][b] = the (profiled pair, scanned cycle) observations whose root's quality lies
 *                 in bin a and whose member's in bin b.  Every cycle counts, N included;
 *   Mis           8 x 8 int64: the part of Obs[a][b] at which the two codes differ;
 *   lane row      WD_LANEQUALITY_LANE_COLS int64 [Pairs, Profiled, Observations, Mismatches];
 *   tile row      WD_LANEQUALITY_TILE_COLS int64 per tile index, the same four, attributed to the tile of the MEMBER;
 *                 zero for an index never added.
 * Identities: Pairs, Profiled and Mismatches equal those of wd_lane_mismatches at the same max_d, per lane and per
 * tile; Observations = Profiled x L = the sum of Obs; the sum of Mis = Mismatches; Mis <= Obs entrywise; Obs and Mis
 * at max_d - 1 are entrywise <= those at max_d; under equality labels Mis = 0 and the sum of Obs = Pairs x L; the sum
 * of QHist = L x the PF wells of the added tiles; QHist is zero outside the values that occur; rows and columns of
 * Obs at or beyond n_bins are zero; nothing depends on the order or batching of the add calls, on hash_bits, on how
 * often wd_lane_qualities is called, or on whether wd_lane_index_finish, wd_lane_mismatches or wd_lane_distances ran
 * before.
 */
#ifndef WELLDUP_LANEQUALITY_H
#define WELLDUP_LANEQUALITY_H

#include "welldup_lanedistance.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WD_LANEQUALITY_MAX_BINS 8
#define WD_LANEQUALITY_VALUES 64
#define WD_LANEQUALITY_MAX_D WD_LANEMISMATCH_MAX_D
#define WD_LANEQUALITY_LANE_COLS 4
#define WD_LANEQUALITY_TILE_COLS 4

/* Device workspace of the quality part of an accumulator for max_tiles tiles of N wells and L cycles.  Host
 * arithmetic only.  With W = max_tiles * N, R = ceil(L / 10) and every part rounded up to 256 bytes:
 *     32768                               QHist, 64 copies of 64 uint64
 *   + 8 * max_tiles * L                   plane pointers of one wd_lane_qual_add
 *   + 8 * max_tiles                       filter pointers of one wd_lane_qual_add
 *   + 4 * max_tiles                       tile indices
 *   + 4 * R * W                           the quality rows: a well's L bin codes, three bits each, ten to a word -
 *                                         the packed rows' own format, the unused codes of the last word zero
 * (a HiSeq 4000 lane, 112 x 4 309 253 wells: 11.6 GB at 51 cycles, 30.9 GB at 151 - what the packed rows themselves
 * take).  Which tile indices got qualities is kept on the host.  Limits and errors as wd_lane_dups_workspace. */
int wd_lane_qual_workspace(int64_t N, int max_tiles, int L, size_t *bytes);

/* Gives the accumulator a quality part with the given bins in workspace_dev (DEVICE memory of at least
 * wd_lane_qual_workspace bytes, the caller's to free after wd_lane_dups_end).  Before the first wd_lane_dups_add and
 * once per accumulator.  WD_ERR_ARG: n_bins outside 1 .. WD_LANEQUALITY_MAX_BINS, edges null, not ascending, the
 * first not 0 or one above 63; a second begin; a begin after an add or a finish; a workspace that is null, in host
 * memory or too small. */
int wd_lane_qual_begin(wd_lane_dups *ld, int n_bins, const int *edges, void *workspace_dev, size_t workspace_bytes);

/* Packs the qualities of n_tiles resident tiles and counts QHist: tile_index, planes (n_tiles x L DEVICE pointers, a
 * plane per scanned cycle) and filter (n_tiles DEVICE pointers; QHist counts the wells whose filter byte has bit 0
 * set) as wd_lane_dups_add takes them - the same planes, which hold base and quality in one byte.  Independent of
 * wd_lane_dups_add in order and in batching.  When the call returns the planes may be overwritten or freed.  A
 * repeated or out-of-range tile index, a call before wd_lane_qual_begin or after a finish, a null or host pointer,
 * or option "well_stride" 4: WD_ERR_ARG, and the call changes nothing. */
int wd_lane_qual_add(wd_lane_dups *ld, int n_tiles, const int *tile_index, const uint8_t *const *planes,
                     const uint8_t *const *filter);

/* Device memory wd_lane_qualities needs.  Host arithmetic only.  With every part rounded up to 256 bytes:
 *     2048 * max_tiles                    per tile index 64 copies of 4 uint64: Pairs, Profiled, Observations,
 *                                         Mismatches
 *   + 65536                               Obs and Mis, 64 copies of 2 x 64 uint64
 *   + 4 * max_tiles                       the tile indices that were added
 * (112 tiles: 295 KB).  A negative size or a null pointer: WD_ERR_ARG; max_tiles > 65535: WD_ERR_UNSUPPORTED. */
int wd_lane_qual_scratch(int max_tiles, size_t *bytes);

/* After a successful finish of either kind and before wd_lane_dups_end, any number of times and with any max_d,
 * before or after wd_lane_index_finish, wd_lane_mismatches and wd_lane_distances.  lane_row
 * (WD_LANEQUALITY_LANE_COLS int64), tile_rows (max_tiles x WD_LANEQUALITY_TILE_COLS int64), qhist
 * (WD_LANEQUALITY_VALUES int64), obs and mis (8 x 8 int64 each, [root's bin][member's bin]) are HOST memory.
 * scratch_dev: DEVICE memory of at least wd_lane_qual_scratch bytes, the caller's; free to reuse when the call
 * returns.  The call reads the packed rows, the quality rows, the label array and the QHist counters and writes
 * nothing but its scratch.  Synchronous on the context's stream.
 * WD_ERR_ARG, changing nothing: no quality part, a call before a successful finish (a near finish refused over budget
 * is none), max_d outside 0 .. WD_LANEQUALITY_MAX_D, a null output pointer, a scratch region that is null, in host
 * memory or too small, or a tile index that was given to wd_lane_dups_add and not to wd_lane_qual_add or the reverse
 * (wd_last_error names one such tile). */
int wd_lane_qualities(wd_lane_dups *ld, int max_d, void *scratch_dev, size_t scratch_bytes, int64_t *lane_row,
                      int64_t *tile_rows, int64_t *qhist, int64_t *obs, int64_t *mis);

#ifdef __cplusplus
}
#endif
#endif /* WELLDUP_LANEQUALITY_H */
