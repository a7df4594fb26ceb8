// lane_consensus.inc - a lane's errors against its families' vote (include/welldup_laneconsensus.h): the members of
// every family of 3 .. max_family wells gathered in device memory, the consensus of each family per cycle, and every
// member's calls counted against it by cycle and by (consensus, own code).  Included from welldup_tiledups.hip after
// lane_gc.inc: it uses read_classes.inc (the spread counters), lane_dups.inc (the accumulator, its label, members and
// packed rows), lane_mismatch.inc's notes and lm_word and lane_pass.inc as lane_mismatch.inc does.
//
// wd_lane_consensus: three launches on the context's stream and nothing but integer adds between them.  They read
// label, members and the rows and write the caller's scratch only.  Who writes label and the rows, and that nobody does
// after a successful finish, is listed at the head of lane_mismatch.inc; members at the head of lane_gc.inc: after
// either finish members[root] = the group's size - 1, exactly members[root] other PF wells carry label == root, and
// members of a single well is 0.  These kernels join both lists as readers.
//
//   k_lc_reserve  LaneRun's grid.  A root with 3 <= n = members + 1 <= max_family reserves n - 1 consecutive words of
//                 the member list (its copies; the root itself is known from the table), notes where they begin in
//                 slot[root] and puts itself into the family table.  Pairs, large families and their wells are
//                 counted here.
//   k_lc_scatter  LaneRun's grid.  Every PF well that is not a root and whose root is voted (members[root] says so:
//                 the member of a large family reads two words and takes no atomic) puts its global id into its
//                 family's range.
//   k_lc_vote     a fixed grid; one wave per voted family, the families dealt out by wave number.
//
// The scratch keeps to 8 bytes per well of the lane: slot, a word per well, and ONE region of W = max_tiles x N words
// for the list and the table.  The list grows from the region's front and holds n - 1 words per voted family, the table
// grows from its back and holds one: together one word per well of a voted family, and those are at most W.  There is no
// room for a fill counter per family beside them, so a family's counter is the LAST word of its own range: k_lc_reserve
// clears it, each of the n - 1 copies adds one to it and takes the old value as its place, and the copy that draws
// place n - 2 - the counter's own word - is by then the last to have added (n - 2 adds came before its own, and there
// are n - 1 in all), so its store of its id over the counter loses nothing.  Neither array is cleared: every word
// that is read was written by this call (slot[root] and the counter by k_lc_reserve for exactly the roots that
// k_lc_scatter and k_lc_vote ask about, the range by k_lc_scatter), so the scratch may hold anything.
//
// Why the result is exact and does not depend on the order of execution.  The place a copy takes in its range depends
// on the schedule; a family's range ends up a permutation of its copies whatever it is (n - 1 atomic adds on one word
// return 0 .. n - 2 once each), and so does the table of roots.  Everything k_lc_vote computes of a family is symmetric
// in its members - the counts of the five codes per cycle are sums over them, d(w) depends on the member's own row and
// those counts alone, the root (FirstWellOff) is not taken from the list - and every output is a sum over families or
// over wells of such values: integer adds, which commute, into 64-bit counters in memory or into 32-bit ones in LDS
// whose bounds are given where they stand.  Each family is taken by exactly one wave (family f by wave f mod the
// number of waves), each well of it by exactly one lane of that wave.
#include "welldup_laneconsensus.h"

namespace {

constexpr int kLcMaxD = WD_LANECONSENSUS_MAX_D;
constexpr int kLcBins = WD_LANECONSENSUS_DIST_BINS;
constexpr int kLcMaxFamily = WD_LANECONSENSUS_MAX_FAMILY;
constexpr int kLcTileCnt = WD_LANECONSENSUS_TILE_COLS;      // per tile and copy: Wells, Profiled, Mismatches, WithN
constexpr int kLcLaneCnt = 16;                     // per copy: the seven below, then Dist
constexpr int kLcFamilies = 0, kLcUndecided = 1, kLcUndecidedCalls = 2, kLcFirstOff = 3, kLcPairs = 4, kLcLarge = 5,
              kLcLargeWells = 6, kLcDist = 7;
static_assert(kLcMaxD == kLmMaxD && kLcBins == kLcMaxD + 2 && kLcDist + kLcBins <= kLcLaneCnt,
              "d is noted as lane_mismatch.inc notes it; Dist has a bin per distance up to max_d and an open one");
static_assert(WD_LANECONSENSUS_LANE_COLS == 11 + kLcBins, "the lane row of welldup_laneconsensus.h");
static_assert(kLcMaxFamily < (1 << 16), "the counts of four codes share a 64-bit word, 16 bits each");
constexpr int kLcWaves = kTdBlock / kWave;         // families a workgroup has in hand
constexpr int kLcWindow = kLmWindow;               // cycles whose calls a workgroup counts in LDS
constexpr int kLcPiece = 8;                        // words of a row staged at a time: 80 cycles
constexpr int kLcStride = kLcPiece + 1;            // (odd: the lanes of a wave store to different banks)
constexpr int kLcSlots = (kLcPiece * kFpCycles + kWave - 1) / kWave;      // cycles of a piece a lane votes on
constexpr int kLcMaxWords = (kMaxCycles + kFpCycles - 1) / kFpCycles;
constexpr int kLcVoteGroups = 2048;                // workgroups of k_lc_vote at most: 8 per CU of 256
// A workgroup's LDS: the window of calls 16 000 bytes, the staged rows 4 x 64 x 9 words = 9216, consensus and decided
// mask 2 x 4 x 103 words = 3296, Dist 36: 28 548 bytes, so five workgroups - 20 waves - fit a CU's 160 KB.  The pass is
// a chain of dependent loads per family (table, slot and members, the list, the rows), so the waves in flight are what
// hides it; staging 16 words at a time would cost 37 KB and the fifth workgroup.
static_assert(kLcWindow * kLmCell * 4 + kLcWaves * kWave * kLcStride * 4 + 2 * kLcWaves * kLcMaxWords * 4 + kLcBins * 4 <= 32768,
              "five workgroups per CU");
static_assert(kLcPiece % 4 == 0, "a piece of a row that is whole 16-byte pieces is whole 16-byte pieces");

// the scratch (include/welldup_laneconsensus.h states the arithmetic)
struct LcLayout {
    size_t cnt_t, cnt_l, cursor, tidx, calls, slot, region, bytes;
    size_t cleared;                                // what a call clears: everything before slot
};

LcLayout lc_layout_of(int max_tiles, int64_t N, int L)
{
    LcLayout l;
    const size_t t = (size_t)max_tiles, wells = t * (size_t)N;
    l.cnt_t = 0;
    l.cnt_l = align256(l.cnt_t + t * kSpread * kLcTileCnt * 8);
    l.cursor = align256(l.cnt_l + (size_t)kSpread * kLcLaneCnt * 8);
    l.tidx = align256(l.cursor + 8);
    l.calls = align256(l.tidx + t * sizeof(int));
    l.slot = align256(l.calls + (size_t)L * kLmCell * 8);
    l.region = align256(l.slot + wells * 4);
    l.bytes = align256(l.region + wells * 4);
    l.cleared = l.slot;
    return l;
}

// the workgroups of k_lc_vote for a lane of `wells` wells: no more than its families can be
unsigned lc_vote_groups(size_t wells)
{
    const size_t most = (wells / 3 + kLcWaves - 1) / kLcWaves;
    return (unsigned)std::min<size_t>(std::max<size_t>(most, 1), kLcVoteGroups);
}

// The lanes of a wave wait for each other's LDS stores.  LDS traffic of one wave is processed in order; this only
// stops the compiler from moving a lane's reads above the stores of the others (scan_queue.inc's q_wave_sync).
__device__ inline void lc_wave_sync()
{
#ifdef WD_LANE_CONSENSUS_EMU
    (void)__ballot(true);                          // (the fibers of a wave meet)
#else
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#endif
}

// ---- reserve ------------------------------------------------------------------------------------
// LaneRun's grid and walk.  The cursor is one 64-bit word: the list's words taken in its low half, the families in its
// high half.  A wave sums what its voted roots need (a prefix sum by shuffles), its first lane adds the wave's total
// and its number of families to the cursor ONCE, and the lanes take their prefix of it: a lane's millions of roots
// queue as waves, not as wells.  The low half cannot carry into the high one: the words taken are the copies of voted
// families, fewer than the lane's wells < 2^32.  Family f's root goes to region[W - 1 - f]; its range is
// region[start .. start + n - 2] and ends below the table: the list holds voted wells - families words and the table
// begins at W - families.
__global__ void __launch_bounds__(kTdBlock) k_lc_reserve(const int *__restrict__ tile_idx, int64_t N,
                                                          const uint32_t *__restrict__ label,
                                                          const uint32_t *__restrict__ members, int max_family, uint32_t W,
                                                          unsigned long long *cursor, uint32_t *slot, uint32_t *region,
                                                          unsigned long long *cnt_l)
{
    const LaneRun run(tile_idx, N);
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t n_fam = 0, n_pair = 0, n_large = 0;                      // the same in every lane of a wave
    unsigned long long large_wells = 0;                               // this lane's
    run.walk([&](bool has, int64_t, size_t g64) {
        uint32_t n = 0;                                               // the wells of the family whose root this well is
        if (has && label[g64] == (uint32_t)g64)
            n = members[g64] + 1u;
        const bool voted = n >= 3u && n <= (uint32_t)max_family, large = n > (uint32_t)max_family;
        n_pair += (uint32_t)__popcll(__ballot(n == 2u));
        n_large += (uint32_t)__popcll(__ballot(large));
        if (large)
            large_wells += n;
        const unsigned long long vote = __ballot(voted);
        if (vote) {                                                   // (the same for the whole wave)
            const uint32_t need = voted ? n - 1u : 0u;
            uint32_t pre = need;                                      // the inclusive prefix of need over the wave
            for (int off = 1; off < kWave; off <<= 1) {
                const uint32_t below = (uint32_t)__shfl((int)pre, max(lane - off, 0));
                if (lane >= off)
                    pre += below;
            }
            const uint32_t total = (uint32_t)__shfl((int)pre, kWave - 1), fams = (uint32_t)__popcll(vote);
            unsigned long long base = 0;
            if (lane == 0)
                base = atomicAdd(cursor, (unsigned long long)total | (unsigned long long)fams << 32);
            const uint32_t list0 = (uint32_t)__shfl((int)(uint32_t)base, 0), fam0 = (uint32_t)__shfl((int)(uint32_t)(base >> 32), 0);
            if (voted) {
                const uint32_t start = list0 + pre - need;
                const uint32_t f = fam0 + (uint32_t)__popcll(vote & ((1ull << lane) - 1ull));
                slot[g64] = start;
                region[W - 1u - f] = (uint32_t)g64;
                region[start + n - 2u] = 0;                           // the family's fill counter: the last word of its range
            }
            n_fam += fams;
        }
    });
    for (int off = kWave / 2; off; off >>= 1) {                        // (every lane of the wave takes part)
        large_wells += (unsigned long long)(uint32_t)__shfl((int)(uint32_t)large_wells, lane ^ off) |
                       (unsigned long long)(uint32_t)__shfl((int)(uint32_t)(large_wells >> 32), lane ^ off) << 32;
    }
    if (lane == 0) {
        unsigned long long *c = spread_row(cnt_l, 0, kLcLaneCnt);
        if (n_fam)
            atomicAdd(c + kLcFamilies, (unsigned long long)n_fam);
        if (n_pair)
            atomicAdd(c + kLcPairs, (unsigned long long)n_pair);
        if (n_large) {
            atomicAdd(c + kLcLarge, (unsigned long long)n_large);
            atomicAdd(c + kLcLargeWells, large_wells);
        }
    }
}

// ---- scatter ------------------------------------------------------------------------------------
// LaneRun's grid and walk; no collectives.  A copy reads its label and its root's members; if the family is voted, its
// root's slot; one atomic add on the family's counter gives its place (the head of this file says why the counter may
// be the range's last word).  The members of one family that sit in one wave queue on that word - at most max_family
// adds per word over the whole launch; the families that would queue millions are Large and never come here.  A place
// beyond the range cannot be drawn while members is what the finish left; it is not stored if it were.
__global__ void __launch_bounds__(kTdBlock) k_lc_scatter(const int *__restrict__ tile_idx, int64_t N,
                                                          const uint32_t *__restrict__ label,
                                                          const uint32_t *__restrict__ members, int max_family,
                                                          const uint32_t *__restrict__ slot, uint32_t *region)
{
    const LaneRun run(tile_idx, N);
    run.walk([&](bool has, int64_t, size_t g64) {
        if (!has)
            return;
        const uint32_t lab = label[g64];
        if (lab == kInvalid || lab == (uint32_t)g64)
            return;
        const uint32_t n = members[lab] + 1u;
        if (n < 3u || n > (uint32_t)max_family)
            return;
        const uint32_t start = slot[lab];
        const uint32_t at = atomicAdd(&region[start + n - 2u], 1u);
        if (at < n - 1u)
            region[start + at] = (uint32_t)g64;
    });
}

// ---- vote and tally -----------------------------------------------------------------------------
// The codes of a cycle counted over a family: four 16-bit counts in a word (a family has at most 4096 wells), N's is
// what is left of n.
__device__ inline void lc_count(unsigned long long &cnt4, uint32_t code)
{
    if (code < 4u)
        cnt4 += 1ull << (16 * code);
}

// the code that strictly more than half of n wells hold, 7 for none
__device__ inline uint32_t lc_majority(unsigned long long cnt4, uint32_t n)
{
    const uint32_t c0 = (uint32_t)cnt4 & 0xFFFFu, c1 = (uint32_t)(cnt4 >> 16) & 0xFFFFu, c2 = (uint32_t)(cnt4 >> 32) & 0xFFFFu,
                   c3 = (uint32_t)(cnt4 >> 48), c4 = n - c0 - c1 - c2 - c3;
    return 2u * c0 > n ? 0u : 2u * c1 > n ? 1u : 2u * c2 > n ? 2u : 2u * c3 > n ? 3u : 2u * c4 > n ? 4u : 7u;
}

// member i of the family: the root, then the list's range
__device__ inline uint32_t lc_member(const uint32_t *__restrict__ region, uint32_t root, uint32_t start, uint32_t i)
{
    return i ? region[start + i - 1u] : root;
}

// grid (groups), groups * kLcWaves waves: wave v takes the families v, v + waves, .. of the table - the grid is fixed
// before the number of families is known (the cursor's high half, which k_lc_reserve left), so that nothing is read
// back between the launches.  Per family (root, start = slot[root], n = members[root] + 1):
//   - The vote.  The rows are taken a piece of kLcPiece words - 80 cycles - at a time, and a piece a chunk of at most
//     64 members at a time: lane j stages the piece of member j's row into LDS (16-byte loads where a row is a whole
//     number of them, as lm_compare), then the lanes turn to the cycles: lane c counts the codes of cycle c (and
//     c + 64) of the piece over the chunk's rows.  The counts stay in registers across the chunks of a family of more
//     than 64.  After the last chunk the lane has the consensus of its cycles: it ORs code and a mask of 7 into the
//     wave's consensus row and decided row in LDS (cleared per family), packed as the rows are.  A lane per cycle was
//     taken rather than three ballots per cycle: a family of three would fill 3 of a ballot's 64 lanes, and here the
//     work of a small family is a few LDS reads per lane.  (Neither has been measured against the other.)
//   - The walk.  A member per lane again, by chunks: its row against the consensus row under the decided mask, word by
//     word through lm_word (lane_mismatch.inc: d, and up to seven notes of cycle, consensus code, own code); the walk
//     of a row stops once d is beyond 7 - the open bin asks no more.  Dist goes through wave_by_key to LDS; the tile's
//     four counters through wave_by_key on the member's tile - Profiled, Mismatches and WithN of a group are popcounts
//     of ballots (d and the count of N as three bit planes each), the same in every lane -, summed in registers for the
//     tile the wave met last and added to the spread counters when another tile comes or the wave ends: the families a
//     wave takes one after the other mostly lie on one tile, which keeps a lane of small families from queueing an add
//     per family on the few words of a tile (on the lane of triples it made no difference that could be measured:
//     DESIGN 5.25 says where that lane's time goes).
//   - calls.  A profiled member adds one per note off the diagonal and takes one from the diagonal entry of the same
//     cycle and consensus; when the family is done, lane c adds P, the family's profiled wells, to the diagonal entry
//     of each of its decided cycles: the diagonal gets P - (the profiled members off it) without an add per well and
//     cycle.  Within the first kLcWindow cycles this is the workgroup's LDS histogram of 32-bit counters, flushed at
//     the end with one 64-bit atomic per entry that is not zero; a later cycle goes to memory at once, so the result
//     is exact for every L.  The 32-bit counters: an entry's true value is at most the profiled wells of the families
//     the workgroup took, which are distinct wells of the lane, fewer than 2^32; a -1 that arrives before its family's
//     + P wraps and unwraps (arithmetic modulo 2^32, and modulo 2^64 in memory, of a value that is in range).
// Work per wave and family is bounded by max_family x words (each member's row is loaded twice, piece by piece, and
// counted once per cycle), so the last wave to finish is at most one family of max_family wells behind the others:
// at 4096 wells of 16 words 0.5 MB of loads.  Splitting a family over several waves is not done.
__global__ void __launch_bounds__(kTdBlock) k_lc_vote(int64_t N, const uint32_t *__restrict__ members,
                                                       const uint32_t *__restrict__ rows, int words, int L, int max_d,
                                                       uint32_t W, int groups, const unsigned long long *__restrict__ cursor,
                                                       const uint32_t *__restrict__ slot, const uint32_t *__restrict__ region,
                                                       unsigned long long *cnt_t, unsigned long long *cnt_l,
                                                       unsigned long long *calls)
{
    __shared__ uint32_t s_hist[kLcWindow * kLmCell];
    __shared__ uint32_t s_rows[kLcWaves][kWave * kLcStride];
    __shared__ uint32_t s_cons[kLcWaves][kLcMaxWords], s_dec[kLcWaves][kLcMaxWords];
    __shared__ uint32_t s_dist[kLcBins];
    const int n_hist = min(L, kLcWindow) * kLmCell;
    for (int e = threadIdx.x; e < n_hist; e += kTdBlock)
        s_hist[e] = 0;
    if (threadIdx.x < kLcBins)
        s_dist[threadIdx.x] = 0;
    __syncthreads();
    const int wv = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    uint32_t *my_rows = s_rows[wv], *cons = s_cons[wv], *dec = s_dec[wv];
    const uint32_t n_fam = (uint32_t)(*cursor >> 32), n_waves = (uint32_t)groups * kLcWaves;
    const bool wide = (words & 3) == 0;                               // every row is whole 16-byte pieces
    unsigned long long undecided = 0, undecided_calls = 0, first_off = 0;      // the same in every lane of a wave
    uint32_t in_tile = kInvalid;                                      // the tile whose counters the wave holds, and they
    unsigned long long t_wells = 0, t_prof = 0, t_mis = 0, t_wn = 0;
    auto flush_tile = [&]() {
        if (lane == 0 && in_tile != kInvalid) {
            unsigned long long *c = spread_row(cnt_t, (size_t)in_tile, kLcTileCnt);
            atomicAdd(c, t_wells);
            if (t_prof)
                atomicAdd(c + 1, t_prof);
            if (t_mis)
                atomicAdd(c + 2, t_mis);
            if (t_wn)
                atomicAdd(c + 3, t_wn);
        }
        t_wells = t_prof = t_mis = t_wn = 0;
    };
    for (uint32_t f = blockIdx.x * kLcWaves + wv; f < n_fam; f += n_waves) {
        const uint32_t root = region[W - 1u - f];
        const uint32_t start = slot[root], n = members[root] + 1u;
        for (int k = lane; k < words; k += kWave) {
            cons[k] = 0;
            dec[k] = 0;
        }
        // the vote
        uint32_t n_undec = 0;
        for (int p0 = 0; p0 < words; p0 += kLcPiece) {
            const int pw = min(kLcPiece, words - p0), pc = min(pw * kFpCycles, L - p0 * kFpCycles);      // words and cycles of the piece
            unsigned long long cnt4[kLcSlots];
#pragma unroll
            for (int s = 0; s < kLcSlots; s++)
                cnt4[s] = 0;
            for (uint32_t i0 = 0; i0 < n; i0 += kWave) {
                const int chunk = (int)min((uint32_t)kWave, n - i0);
                lc_wave_sync();                                       // the last chunk's rows have been counted
                if (lane < chunk) {
                    const uint32_t *y = rows + (size_t)lc_member(region, root, start, i0 + lane) * words + p0;
                    uint32_t *to = my_rows + lane * kLcStride;
                    if (wide) {
                        for (int k = 0; k < pw; k += 4) {
                            const uint4 q = *(const uint4 *)(y + k);
                            to[k] = q.x;
                            to[k + 1] = q.y;
                            to[k + 2] = q.z;
                            to[k + 3] = q.w;
                        }
                    } else {
                        for (int k = 0; k < pw; k++)
                            to[k] = y[k];
                    }
                }
                lc_wave_sync();
#pragma unroll
                for (int s = 0; s < kLcSlots; s++) {
                    const int c = lane + s * kWave;
                    if (c < pc) {
                        const int k = c / kFpCycles, sh = 3 * (c - k * kFpCycles);
                        for (int r = 0; r < chunk; r++)
                            lc_count(cnt4[s], (my_rows[r * kLcStride + k] >> sh) & 7u);
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < kLcSlots; s++) {
                const int c = lane + s * kWave;
                const uint32_t a = c < pc ? lc_majority(cnt4[s], n) : 0u;
                if (c < pc && a != 7u) {
                    const int k = c / kFpCycles, sh = 3 * (c - k * kFpCycles);
                    if (a)
                        atomicOr(&cons[p0 + k], a << sh);
                    atomicOr(&dec[p0 + k], 7u << sh);
                }
                n_undec += (uint32_t)__popcll(__ballot(c < pc && a == 7u));
            }
        }
        lc_wave_sync();                                               // the consensus row is whole
        // the walk
        uint32_t n_prof = 0;
        for (uint32_t i0 = 0; i0 < n; i0 += kWave) {
            const bool active = i0 + lane < n;
            uint32_t id = 0, with_n = 0;
            int d = 0;
            LmNotes notes;
            if (active) {
                id = lc_member(region, root, start, i0 + lane);
                const uint32_t *y = rows + (size_t)id * words;
                if (wide) {
                    for (int k = 0; k < words && d <= kLcMaxD; k += 4) {
                        const uint4 q = *(const uint4 *)(y + k);
                        lm_word(k, cons[k], q.x & dec[k], d, notes);
                        lm_word(k + 1, cons[k + 1], q.y & dec[k + 1], d, notes);
                        lm_word(k + 2, cons[k + 2], q.z & dec[k + 2], d, notes);
                        lm_word(k + 3, cons[k + 3], q.w & dec[k + 3], d, notes);
                    }
                } else {
                    for (int k = 0; k < words && d <= kLcMaxD; k++)
                        lm_word(k, cons[k], y[k] & dec[k], d, notes);
                }
                d = min(d, kLcBins - 1);
            }
            const bool prof = active && d <= max_d;
            if (prof)
                for (int i = 0; i < d; i++) {
                    const uint32_t e = notes.pop();
                    const uint32_t a = (e >> 3) & 7u, b = e & 7u, cell = (e >> 6) * kLmCell + a * kLmCodes + b,
                                   diag = (e >> 6) * kLmCell + a * (kLmCodes + 1);
                    with_n += (a == 4u) | (b == 4u);
                    if (cell < (uint32_t)n_hist) {
                        atomicAdd(&s_hist[cell], 1u);
                        atomicAdd(&s_hist[diag], 0xFFFFFFFFu);
                    } else {
                        atomicAdd(calls + cell, 1ull);
                        atomicAdd(calls + diag, ~0ull);
                    }
                }
            const unsigned long long b_prof = __ballot(prof);
            const unsigned long long d0 = __ballot(d & 1), d1 = __ballot(d & 2), d2 = __ballot(d & 4);
            const unsigned long long w0 = __ballot(with_n & 1u), w1 = __ballot(with_n & 2u), w2 = __ballot(with_n & 4u);
            n_prof += (uint32_t)__popcll(b_prof);
            if (i0 == 0)
                first_off += (__ballot(active && lane == 0 && d >= 1) & 1ull);
            wave_by_key(active, (uint32_t)d, [&](uint32_t bin, unsigned long long group, bool first) {
                if (first)
                    atomicAdd(&s_dist[bin], (uint32_t)__popcll(group));
            });
            wave_by_key(active, id / (uint32_t)N, [&](uint32_t tile, unsigned long long group, bool) {
                if (tile != in_tile) {                                // (the same in every lane)
                    flush_tile();
                    in_tile = tile;
                }
                const unsigned long long gp = group & b_prof;
                t_wells += (unsigned long long)__popcll(group);
                t_prof += (unsigned long long)__popcll(gp);
                t_mis += __popcll(gp & d0) + 2ull * __popcll(gp & d1) + 4ull * __popcll(gp & d2);
                t_wn += __popcll(gp & w0) + 2ull * __popcll(gp & w1) + 4ull * __popcll(gp & w2);
            });
        }
        // the diagonal: P at every decided cycle
        if (n_prof)
            for (int c = lane; c < L; c += kWave) {
                const int k = c / kFpCycles, sh = 3 * (c - k * kFpCycles);
                if ((dec[k] >> sh) & 1u) {
                    const uint32_t diag = (uint32_t)c * kLmCell + ((cons[k] >> sh) & 7u) * (kLmCodes + 1);
                    if (diag < (uint32_t)n_hist)
                        atomicAdd(&s_hist[diag], n_prof);
                    else
                        atomicAdd(calls + diag, (unsigned long long)n_prof);
                }
            }
        undecided += n_undec;
        undecided_calls += (unsigned long long)n_undec * n_prof;
        lc_wave_sync();                                               // before the next family clears the rows
    }
    flush_tile();
    if (lane == 0) {
        unsigned long long *c = spread_row(cnt_l, 0, kLcLaneCnt);
        if (undecided) {
            atomicAdd(c + kLcUndecided, undecided);
            if (undecided_calls)
                atomicAdd(c + kLcUndecidedCalls, undecided_calls);
        }
        if (first_off)
            atomicAdd(c + kLcFirstOff, first_off);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n_hist; e += kTdBlock)
        if (s_hist[e])
            atomicAdd(calls + e, (unsigned long long)s_hist[e]);
    if (threadIdx.x < kLcBins && s_dist[threadIdx.x])
        atomicAdd(spread_row(cnt_l, 0, kLcLaneCnt) + kLcDist + threadIdx.x, (unsigned long long)s_dist[threadIdx.x]);
}

}  // namespace

#ifndef WD_LANE_CONSENSUS_EMU                      // (tools/lane_consensus_emu.cpp: the kernels above on the CPU, a fiber per lane)
extern "C" {

int wd_lane_consensus_scratch(int max_tiles, int64_t wells_per_tile, int L, size_t *bytes)
{
    if (max_tiles < 0 || wells_per_tile < 0 || L < 0 || !bytes)
        return WD_ERR_ARG;
    if (L > kMaxCycles || max_tiles > 65535 ||
        (max_tiles > 0 && (uint64_t)wells_per_tile >= (uint64_t)0xFFFFFFFFu / (uint64_t)max_tiles))
        return WD_ERR_UNSUPPORTED;
    *bytes = lc_layout_of(max_tiles, wells_per_tile, L).bytes;
    return WD_OK;
}

int wd_lane_consensus(wd_lane_dups *ld, int max_d, int max_family, void *scratch_dev, size_t scratch_bytes,
                      int64_t *lane_row, int64_t *tile_rows, int64_t *calls)
try {
    if (!ld || !lane_row || !tile_rows || !calls)
        return WD_ERR_ARG;
    wd_ctx *ctx = ld->ctx;
    const int64_t N = ld->N;
    const int T = ld->max_tiles, L = ld->L;
    LanePass p(ld);
    if (const int rc = p.finished("lane consensus comes after a successful finish of the lane"))
        return rc;
    if (max_d < 0 || max_d > kLcMaxD)
        return fail(ctx, WD_ERR_ARG, "lane consensus: max_d is 0.." + std::to_string(kLcMaxD) + ", not " +
                                         std::to_string(max_d));
    if (max_family < 3 || max_family > kLcMaxFamily)
        return fail(ctx, WD_ERR_ARG, "lane consensus: max_family is 3.." + std::to_string(kLcMaxFamily) + ", not " +
                                         std::to_string(max_family));
    const LcLayout lay = lc_layout_of(T, N, L);
    if (const int rc = p.scratch(scratch_dev, scratch_bytes, lay.bytes, "scratch smaller than wd_lane_consensus_scratch",
                                 "lane consensus: the scratch must be in device memory"))
        return rc;
    const size_t n_calls = (size_t)L * kLmCell;
    memset(lane_row, 0, WD_LANECONSENSUS_LANE_COLS * sizeof(int64_t));
    memset(tile_rows, 0, (size_t)T * kLcTileCnt * sizeof(int64_t));
    memset(calls, 0, n_calls * sizeof(int64_t));
    if (!p.start())
        return p.rc;
    uint8_t *sc = (uint8_t *)scratch_dev;
    unsigned long long *cnt_t = (unsigned long long *)(sc + lay.cnt_t);
    unsigned long long *cnt_l = (unsigned long long *)(sc + lay.cnt_l);
    unsigned long long *cursor = (unsigned long long *)(sc + lay.cursor);
    int *d_tidx = (int *)(sc + lay.tidx);
    unsigned long long *d_calls = (unsigned long long *)(sc + lay.calls);
    uint32_t *slot = (uint32_t *)(sc + lay.slot), *region = (uint32_t *)(sc + lay.region);
    const uint32_t *label = (const uint32_t *)(ld->ws + ld->lay.label), *members = (const uint32_t *)(ld->ws + ld->lay.members);
    const size_t wells = (size_t)T * (size_t)N;
    const uint32_t W = (uint32_t)wells;
    const unsigned groups = lc_vote_groups(wells);
    WD_HIP(ctx, hipMemsetAsync(sc, 0, lay.cleared, ctx->stream));
    if (const int rc = p.upload(d_tidx))
        return rc;
    hipLaunchKernelGGL(k_lc_reserve, p.grid, dim3(kTdBlock), 0, ctx->stream, d_tidx, N, label, members, max_family, W, cursor,
                       slot, region, cnt_l);
    WD_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lc_scatter, p.grid, dim3(kTdBlock), 0, ctx->stream, d_tidx, N, label, members, max_family, slot, region);
    WD_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lc_vote, dim3(groups), dim3(kTdBlock), 0, ctx->stream, N, members,
                       (const uint32_t *)(ld->ws + ld->lay.rows), ld->lay.words, L, max_d, W, (int)groups, cursor, slot, region,
                       cnt_t, cnt_l, d_calls);
    WD_HIP(ctx, hipGetLastError());
    SpreadFetch f_t(cnt_t, (size_t)T, kLcTileCnt), f_l(cnt_l, 1, kLcLaneCnt);
    if (n_calls)
        WD_HIP(ctx, hipMemcpyAsync(calls, d_calls, n_calls * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (const int rc = spread_fetch(ctx, {&f_t, &f_l}))
        return rc;
    unsigned long long c[kLcLaneCnt];
    for (int t = 0; t < T; t++) {
        f_t.sum((size_t)t, c);
        for (int f = 0; f < kLcTileCnt; f++) {
            tile_rows[(size_t)t * kLcTileCnt + f] = (int64_t)c[f];
            lane_row[1 + f] += (int64_t)c[f];
        }
    }
    f_l.sum(0, c);
    lane_row[0] = (int64_t)c[kLcFamilies];
    lane_row[5] = (int64_t)c[kLcUndecided];
    lane_row[6] = (int64_t)c[kLcUndecidedCalls];
    lane_row[7] = (int64_t)c[kLcFirstOff];
    lane_row[8] = (int64_t)c[kLcPairs];
    lane_row[9] = (int64_t)c[kLcLarge];
    lane_row[10] = (int64_t)c[kLcLargeWells];
    for (int b = 0; b < kLcBins; b++)
        lane_row[11 + b] = (int64_t)c[kLcDist + b];
    return WD_OK;
} WD_CATCH

}  // extern "C"
#endif
