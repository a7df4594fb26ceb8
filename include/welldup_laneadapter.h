/*
 * welldup_laneadapter.h - a lane's duplication by insert length (libwelldup.so, the `tiledups` translation unit).
 *
 * The passes after a finish say how much of a lane is duplicated, where, in which library and against which GC.
 * Nothing says whether the duplication depends on the fragment's length - the bias patterned flowcells are known for:
 * short inserts and adapter dimers seed clusters faster than long fragments, over-cluster, duplicate and fill the
 * neighbouring wells.  A read whose insert is shorter than the read runs into its adapter, and where it does is the
 * insert's length.  wd_lane_adapter searches the packed row of every well of the lane for the adapter, at every
 * position, with mismatches and with partial overlaps at the read's end, and counts the wells by where the adapter
 * begins and by what they are in their group - exactly, over every PF read, without a FASTQ or an alignment.
 * Definitions, for one lane, after a successful finish of either kind; a read r has L scanned cycles:
 *   code          of a cycle, as in the packed rows: A 0, C 1, G 2, T 3, N 4;
 *   adapter       A[0 .. m - 1] over A, C, G, T, m in WD_LANEADAPTER_MIN_LEN .. WD_LANEADAPTER_MAX_LEN (8 .. 32);
 *   E             the mismatches allowed at full overlap, 0 .. WD_LANEADAPTER_MAX_E (3);
 *   O             the minimum overlap, WD_LANEADAPTER_MIN_OVERLAP (3) .. m, and at most L;
 *   o(p)          = min(m, L - p), for a position p in 0 .. L - O;
 *   mism(p)       the number of j < o(p) with r[p + j] != A[j]; an N in the read is a mismatch;
 *   allowed(p)    E where o(p) == m, else floor(E * o(p) / m);
 *   p matches     iff mism(p) <= allowed(p); a position with L - p < O never matches;
 *   a(w)          of a PF well w: the smallest matching p, or L when none matches ("no adapter").  When the scanned
 *                 cycles start at the read's first cycle, a(w) is the insert length;
 *   first match   of a well with a(w) < L: the match at p = a(w);
 *   population    of a PF well, by label and members, exactly as in welldup_lanegc.h: Single, Root or Copy.  Under a
 *                 near finish the groups are the clusters;
 *   hist          int64 [L + 1][WD_LANEADAPTER_HIST_COLS = 4], for every a:
 *                   Single[a], Roots[a], Copies[a]   the wells of that population with a(w) = a, each by its own read;
 *                   FamilyWells[a]                   the sum of members + 1 over the roots with a(root) = a;
 *                 row L is "no adapter";
 *   lane row      WD_LANEADAPTER_LANE_COLS = 10 int64 [PF, Single, Roots, Copies, AdSingle, AdRoots, AdCopies,
 *                 AdFamilyWells, Inexact, Partial]: the Ad columns count the wells with a < L, AdFamilyWells by the
 *                 root's a; Inexact counts the wells whose first match has mism >= 1, Partial those whose first match
 *                 has o < m;
 *   tile row      WD_LANEADAPTER_TILE_COLS = 5 int64 per tile index, by the well's own tile [PF, Adapter, Copies,
 *                 CopiesAdapter, SumA]: SumA is the sum of a over the wells with a < L; zero for an index never added.
 * Identities:
 *   1. PF = Single + Roots + Copies = PF of the last finish's lane row, Roots = its Classes, Copies = its Redundant,
 *      and per tile PF = that finish's tile row's PF;
 *   2. for each of the three populations the sum over a of its column = the population;
 *   3. the Ad columns are those sums without row L;
 *   4. the sum of FamilyWells = Roots + Copies, and FamilyWells[a] >= 2 Roots[a];
 *   5. under equality labels a copy's read is its root's: Copies[a] = FamilyWells[a] - Roots[a] for every a;
 *   6. the tile rows sum to: the lane's PF; AdSingle + AdRoots + AdCopies; Copies; AdCopies; the sum over a < L of
 *      a x the three populations;
 *   7. raising E or lowering O never raises a(w): for every a the number of wells of the three populations in rows
 *      0 .. a never falls;
 *   8. with E = 0, Inexact = 0; with O = m, Partial = 0;
 *   9. nothing depends on the order or batching of the add calls, on hash_bits, on which other passes ran before, or
 *      on how often the call is made.
 */
#ifndef WELLDUP_LANEADAPTER_H
#define WELLDUP_LANEADAPTER_H

#include "welldup_lanedups.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WD_LANEADAPTER_MIN_LEN 8
#define WD_LANEADAPTER_MAX_LEN 32
#define WD_LANEADAPTER_MAX_E 3
#define WD_LANEADAPTER_MIN_OVERLAP 3
#define WD_LANEADAPTER_HIST_COLS 4
#define WD_LANEADAPTER_LANE_COLS 10
#define WD_LANEADAPTER_TILE_COLS 5

/* Device memory wd_lane_adapter needs for an accumulator of max_tiles tiles and reads of L cycles.  Host arithmetic
 * only.  With every part rounded up to 256 bytes:
 *     5632 * max_tiles                    per tile index 64 copies of 11 uint64: the lane row's ten columns of the
 *                                         tile and SumA
 *   + 2048 * (L + 1)                      hist, 64 copies of 4 uint64 per a
 *   + 4 * max_tiles                       the tile indices that were added
 *   + 1024                                the search's table: which adapter positions hold which base, and per 64
 *                                         positions of the read where 0, 1, 2 and 3 mismatches are still a match
 * (a HiSeq 4000 lane of 112 tiles at 151 cycles: 943 616 bytes).
 * A negative argument or a null pointer: WD_ERR_ARG; L > 1024 or max_tiles > 65535: WD_ERR_UNSUPPORTED. */
int wd_lane_adapter_scratch(int max_tiles, int L, size_t *bytes);

/* After a successful finish of either kind and before wd_lane_dups_end, any number of times and with any adapter,
 * before or after every other pass.  adapter: m codes 0 .. 3 (A C G T), HOST memory.  lane_row
 * (WD_LANEADAPTER_LANE_COLS int64), tile_rows (max_tiles x WD_LANEADAPTER_TILE_COLS int64) and hist ((L + 1) x
 * WD_LANEADAPTER_HIST_COLS int64) are HOST memory.  scratch_dev: DEVICE memory of at least
 * wd_lane_adapter_scratch(max_tiles, L) bytes, the caller's; free to reuse when the call returns.  The call reads the
 * label array, the members and the packed rows and writes nothing but its scratch.  Synchronous on the context's
 * stream.  A lane without wells or tiles: WD_OK with zeros.
 * WD_ERR_ARG, changing nothing: a call before a successful finish (a near finish refused over budget is none), m
 * outside 8 .. 32, max_e outside 0 .. 3, min_overlap outside 3 .. m or above L, an adapter code above 3, a null
 * adapter, lane_row, tile_rows or hist, a scratch region that is null, in host memory or too small. */
int wd_lane_adapter(wd_lane_dups *ld, const uint8_t *adapter, int m, int max_e, int min_overlap, void *scratch_dev,
                    size_t scratch_bytes, int64_t *lane_row, int64_t *tile_rows, int64_t *hist);

#ifdef __cplusplus
}
#endif
#endif /* WELLDUP_LANEADAPTER_H */
