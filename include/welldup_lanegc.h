/*
 * welldup_lanegc.h - a lane's duplication against its reads' GC content (libwelldup.so, the `tiledups` translation unit).
 *
 * The passes after a finish say how much of a lane is duplicated, in which library, where the copies differ, how far
 * apart they lie, what quality they report, whether more depth would pay and which reads they are.  Nothing says
 * whether the duplication depends on the molecule: are the GC-poor and the GC-rich fragments of a PCR-amplified
 * library over- or under-amplified?  wd_lane_gc reads the packed row of every well of the lane together with the
 * labels and the members the last finish left in the accumulator, and counts the wells by the GC of their own read
 * and by what they are in their group - exactly, over every PF read, without an alignment.
 * Definitions, for one lane, after a successful finish of either kind:
 *   code          of a cycle, as in the packed rows: A 0, C 1, G 2, T 3, N 4;
 *   g(w), n(w)    of a PF well w: the number of scanned cycles whose code is C or G, and the number whose code is N;
 *                 g + n <= L;
 *   population    of a PF well w, by label and members (global id(w) = tile index * N + well):
 *                   Single  label(w) == id(w), members(w) == 0;
 *                   Root    label(w) == id(w), members(w) >= 1: its group has members(w) + 1 wells;
 *                   Copy    label(w) != id(w).
 *                 Under a near finish the groups are the clusters;
 *   skipped       a well with n(w) > max_n, max_n the caller's, 0 .. L.  It is counted by population but kept out of
 *                 hist (an all-N read would otherwise be one huge class at GC 0); every other PF well is counted;
 *   hist          int64 [L + 1][WD_LANEGC_HIST_COLS = 4], for every g over the counted wells:
 *                   Single[g], Roots[g], Copies[g]   the wells of that population with g(w) = g, each by its own read;
 *                   FamilyWells[g]                   the sum of members + 1 over the roots with g(root) = g: the
 *                                                    group's wells by the GC of the molecule (no other well's row is
 *                                                    loaded for it);
 *   lane row      WD_LANEGC_LANE_COLS = 8 int64 [PF, Single, Roots, Copies, SkipSingle, SkipRoots, SkipCopies,
 *                 SkipFamilyWells]: the first four count every PF well, whatever its n; SkipFamilyWells is the sum of
 *                 members + 1 over the skipped roots;
 *   tile row      WD_LANEGC_TILE_COLS = 5 int64 per tile index, by the well's own tile [PF, Counted, GC, CopiesCounted,
 *                 CopiesGC]: GC and CopiesGC are the sums of g over the counted wells and over the counted copies;
 *                 zero for an index never added.
 * Identities:
 *   1. PF = Single + Roots + Copies = PF of the last finish's lane row, Roots = its Classes, Copies = its Redundant,
 *      and per tile PF = that finish's tile row's PF;
 *   2. for each of the three populations the sum over g of its column = the population - its Skip; the sum of
 *      FamilyWells + SkipFamilyWells = Roots + Copies; FamilyWells[g] >= 2 Roots[g];
 *   3. hist[g] = 0 wherever no counted well can sit: a counted well has g <= L - n(w) <= L, so there is no row beyond
 *      g = L; FamilyWells[g] = 0 wherever Roots[g] = 0; and a lane whose reads all carry one g has one row that is
 *      not zero;
 *   4. with max_n = L nothing is skipped: the four Skip columns are zero;
 *   5. every cell of hist, Counted, GC, CopiesCounted and CopiesGC grows with max_n, every Skip column falls;
 *   6. under equality labels a copy's read is its root's: Copies[g] = FamilyWells[g] - Roots[g] for every g, and
 *      SkipCopies = SkipFamilyWells - SkipRoots.  Under clusters only the sums agree, and only when nothing is
 *      skipped;
 *   7. the tile rows sum to: the lane's PF; the sum over g of the three populations (Counted); the sum over g of
 *      g x the three populations (GC); the sum over g of Copies[g]; the sum over g of g x Copies[g];
 *   8. nothing depends on the order or batching of the add calls, on hash_bits, on which other passes ran before, or
 *      on how often the call is made.
 */
#ifndef WELLDUP_LANEGC_H
#define WELLDUP_LANEGC_H

#include "welldup_lanedups.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WD_LANEGC_HIST_COLS 4
#define WD_LANEGC_LANE_COLS 8
#define WD_LANEGC_TILE_COLS 5

/* Device memory wd_lane_gc needs for an accumulator of max_tiles tiles and reads of L cycles.  Host arithmetic only.
 * With every part rounded up to 256 bytes:
 *     5120 * max_tiles                    per tile index 64 copies of 10 uint64: the lane row's eight columns of the
 *                                         tile, GC and CopiesGC
 *   + 2048 * (L + 1)                      hist, 64 copies of 4 uint64 per g
 *   + 4 * max_tiles                       the tile indices that were added
 * (a HiSeq 4000 lane of 112 tiles at 151 cycles: 885 248 bytes).
 * A negative argument or a null pointer: WD_ERR_ARG; L > 1024 or max_tiles > 65535: WD_ERR_UNSUPPORTED. */
int wd_lane_gc_scratch(int max_tiles, int L, size_t *bytes);

/* After a successful finish of either kind and before wd_lane_dups_end, any number of times and with any max_n,
 * before or after every other pass.  lane_row (WD_LANEGC_LANE_COLS int64), tile_rows (max_tiles x
 * WD_LANEGC_TILE_COLS int64) and hist ((L + 1) x WD_LANEGC_HIST_COLS int64) are HOST memory.  scratch_dev: DEVICE
 * memory of at least wd_lane_gc_scratch(max_tiles, L) bytes, the caller's; free to reuse when the call returns.  The
 * call reads the label array, the members and the packed rows and writes nothing but its scratch.  Synchronous on the
 * context's stream.  A lane without wells or tiles: WD_OK with zeros.
 * WD_ERR_ARG, changing nothing: a call before a successful finish (a near finish refused over budget is none), max_n
 * outside 0 .. L, a null lane_row, tile_rows or hist, a scratch region that is null, in host memory or too small. */
int wd_lane_gc(wd_lane_dups *ld, int max_n, void *scratch_dev, size_t scratch_bytes, int64_t *lane_row,
               int64_t *tile_rows, int64_t *hist);

#ifdef __cplusplus
}
#endif
#endif /* WELLDUP_LANEGC_H */
