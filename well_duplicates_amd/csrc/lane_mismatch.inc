// lane_mismatch.inc - where a lane's duplicate copies differ (include/welldup_lanemismatch.h): every redundant well
// of a lane compared with its root, the distances binned and the differing cycles of the near pairs counted by
// cycle and by (root's code, member's code).  Included at the end of welldup_tiledups.hip: it uses read_classes.inc
// (the spread counters), lane_dups.inc (the accumulator, its packed rows and label array), lane_near.inc's way of
// loading two rows and lane_pass.inc (the run, the grouping by key, the start of a pass and the counters' way back).
//
// wd_lane_mismatches, over the tiles that were added (grid y = tile): one kernel, k_lm_tally, and nothing else.
// It reads rows and label and writes the caller's scratch only.  That neither array changes once a finish has
// succeeded was checked where they are written: rows by k_ld_pack alone (lane_dups.inc, wd_lane_dups_add, which
// refuses after a finish); label by k_ld_resolve (ld_equality, once: `resolved`) and by k_ln_pairs /
// k_ln_pairs_long / k_ln_compress (lane_near.inc, all inside the one successful wd_lane_near_dups_finish);
// ld_count_rows, li_tally and wd_lane_index_finish (lane_index.inc) write the table, aux and the index workspace,
// and read label - which is why this pass keeps away from the table and aux; k_lg_tally (lane_distance.inc) reads
// label only, and so do k_ls_min and k_ls_tally (lane_saturation.inc).  k_lt_hist, k_lt_collect, k_lt_spread and k_lt_rows
// (lane_top.inc) read label, members and the rows.  k_lh_tally (lane_hops.inc) reads label and the index workspace's
// key, which k_li_pack alone writes (lane_index.inc, wd_lane_index_add, which refuses after a finish).  k_lgc_tally
// (lane_gc.inc) reads label, members and every row of the lane, and so does k_lad_tally (lane_adapter.inc).  k_lc_reserve and k_lc_scatter (lane_consensus.inc) read
// label and members, k_lc_vote members and the rows of the voted families.  k_lk_score and k_lk_mark (lane_keep.inc)
// read label, members and the quality rows - or, launched by wd_lane_keep_molecules, the caller's mol and molmem in
// their places, which k_lu_pairs_mol and k_lu_group_mol (lane_umi.inc) wrote from label, members and the UMI keys.
#include "welldup_lanemismatch.h"

namespace {

constexpr int kLmWindow = 160;                     // cycles whose substitutions a workgroup counts in LDS
constexpr int kLmCodes = 5;
constexpr int kLmCell = kLmCodes * kLmCodes;       // entries of Sub per cycle
constexpr int kLmMaxD = WD_LANEMISMATCH_MAX_D;
constexpr int kLmBins = WD_LANEMISMATCH_DIST_BINS;
constexpr int kLmTileCnt = WD_LANEMISMATCH_TILE_COLS;      // per tile and copy: Pairs, Profiled, Mismatches, WithN
constexpr int kLmLaneCnt = 16;                     // per copy: Dist
static_assert(kLmBins == kLmMaxD + 2 && kLmBins <= kLmLaneCnt, "Dist has a bin per distance up to max_d and an open one");
static_assert(kLmWindow % kFpCycles == 0 && kLmWindow * kLmCell * 4 <= 16384, "the window: whole words, 16 KB of LDS");
constexpr uint32_t kLmLow = 0x09249249u;             // the lowest bit of each of a word's ten codes
static_assert(kMaxCycles <= 1024, "a noted mismatch keeps its cycle in ten bits");

// the scratch (include/welldup_lanemismatch.h states the arithmetic)
struct LmLayout {
    size_t cnt_t, cnt_l, tidx, sub, bytes;
};

LmLayout lm_layout_of(int max_tiles, int L)
{
    LmLayout l;
    const size_t t = (size_t)max_tiles;
    l.cnt_t = 0;
    l.cnt_l = align256(l.cnt_t + t * kSpread * kLmTileCnt * 8);
    l.tidx = align256(l.cnt_l + (size_t)kSpread * kLmLaneCnt * 8);
    l.sub = align256(l.tidx + t * sizeof(int));
    l.bytes = align256(l.sub + (size_t)L * kLmCell * 8);
    return l;
}

// What a pair remembers of its mismatches: up to kLmMaxD of them, 16 bits each - cycle (10 bits), the root's code
// and the member's (3 bits each) - in two registers used as a 112-bit shift register: no array, so nothing is
// indexed by a variable and nothing goes to scratch.
struct LmNotes {
    unsigned long long lo = 0, hi = 0;
    __device__ void push(uint32_t e)
    {
        hi = (hi << 16) | (lo >> 48);
        lo = (lo << 16) | e;
    }
    __device__ uint32_t pop()
    {
        const uint32_t e = (uint32_t)lo & 0xFFFFu;
        lo = (lo >> 16) | (hi << 48);
        hi >>= 16;
        return e;
    }
};

// The codes of two words that differ, one bit each at the code's lowest bit (ln_diff's fold); k_lq_tally
// (lane_quality.inc) holds the same mask against the qualities.
__device__ inline uint32_t lm_fold(uint32_t x, uint32_t y)
{
    const uint32_t z = x ^ y;
    return (z | (z >> 1) | (z >> 2)) & kLmLow;
}

// Word k of the root's row (x) and of the member's (y): the differing codes, one bit each at the code's lowest bit
// (lm_fold), counted into d; while fewer than kLmMaxD are noted, each is noted.  The row format is
// k_ld_pack's: cycle 10 k + j at bits 3 j .. 3 j + 2 of word k, the unused codes of the last word zero in both
// rows - they never differ.
__device__ inline void lm_word(int k, uint32_t x, uint32_t y, int &d, LmNotes &notes)
{
    uint32_t m = lm_fold(x, y);
    if (!m)
        return;
    int n = d;
    d += __popc(m);
    for (; m && n < kLmMaxD; m &= m - 1, n++) {
        const int bit = __ffs((int)m) - 1;
        notes.push((uint32_t)(k * kFpCycles + bit / 3) << 6 | ((x >> bit) & 7u) << 3 | ((y >> bit) & 7u));
    }
}

// d of the rows of a (the root) and b, exact up to kLmMaxD and otherwise some value above it: the walk stops after
// the piece in which d passes kLmMaxD - the open bin asks no more.  The loading is rows_hamming_upto's: kLdCmpWords
// words of both rows in flight, as 16-byte pieces where a row is a whole number of them.
__device__ inline int lm_compare(const uint32_t *__restrict__ rows, int words, uint32_t a, uint32_t b, LmNotes &notes)
{
    const uint32_t *x = rows + (size_t)a * words, *y = rows + (size_t)b * words;
    int d = 0, i = 0;
    if ((words & 3) == 0) {
        for (; i + kLdCmpWords <= words; i += kLdCmpWords) {
            const uint4 p0 = *(const uint4 *)(x + i), p1 = *(const uint4 *)(x + i + 4);
            const uint4 q0 = *(const uint4 *)(y + i), q1 = *(const uint4 *)(y + i + 4);
            lm_word(i, p0.x, q0.x, d, notes);
            lm_word(i + 1, p0.y, q0.y, d, notes);
            lm_word(i + 2, p0.z, q0.z, d, notes);
            lm_word(i + 3, p0.w, q0.w, d, notes);
            lm_word(i + 4, p1.x, q1.x, d, notes);
            lm_word(i + 5, p1.y, q1.y, d, notes);
            lm_word(i + 6, p1.z, q1.z, d, notes);
            lm_word(i + 7, p1.w, q1.w, d, notes);
            if (d > kLmMaxD)
                return d;
        }
        for (; i < words; i += 4) {
            const uint4 p = *(const uint4 *)(x + i), q = *(const uint4 *)(y + i);
            lm_word(i, p.x, q.x, d, notes);
            lm_word(i + 1, p.y, q.y, d, notes);
            lm_word(i + 2, p.z, q.z, d, notes);
            lm_word(i + 3, p.w, q.w, d, notes);
        }
        return d;
    }
    for (; i + kLdCmpWords <= words; i += kLdCmpWords) {
        uint32_t p[kLdCmpWords], q[kLdCmpWords];
#pragma unroll
        for (int j = 0; j < kLdCmpWords; j++) {
            p[j] = x[i + j];
            q[j] = y[i + j];
        }
#pragma unroll
        for (int j = 0; j < kLdCmpWords; j++)
            lm_word(i + j, p[j], q[j], d, notes);
        if (d > kLmMaxD)
            return d;
    }
    for (; i < words; i++)
        lm_word(i, x[i], y[i], d, notes);
    return d;
}

// ---- tally --------------------------------------------------------------------------------------
// LaneRun's grid and walk (lane_pass.inc).  A well that is PF (it has a label) and not its own root is a pair: it
// loads its row and its root's, and d is the popcount of their folded XOR.
//   - Dist and the tile's four counters.  A lane of equal reads puts every pair into Dist[0], a lane of copies with
//     one error into Dist[1]: the pairs of a wave are grouped by bin (wave_by_key), and the first lane of a group adds
//     the group's size to the workgroup's Dist in LDS.  Pairs, Profiled and Mismatches (d x the group's size for a
//     bin <= max_d) are the same for every lane of the wave: they are summed in registers over the run, and the
//     wave's first lane adds them to LDS once.  At the end the workgroup adds what is not zero to its copy of the
//     spread counters.
//   - Sub.  A profiled pair pops its d <= 7 notes: one add each to the LDS histogram [cycle][a][b] of 32-bit
//     counters (a run adds at most 7 x kLaneRun to an entry), flushed with one 64-bit atomic per entry that is not
//     zero.  The histogram holds the first kLmWindow cycles - 16 000 bytes, so that eight workgroups, all 2048
//     lanes of a CU, keep within its 160 KB and occupancy is not what bounds the pass; a mismatch at a later cycle
//     is added to Sub in memory at once, so the result is exact for every L the accumulator takes.  WithN is
//     counted where the notes are popped.
// Why the result is exact and does not depend on the order of execution: every output is a sum of ones (or of d)
// over wells, each well is visited by exactly one lane of one workgroup, integer adds commute and none can
// overflow (a 32-bit LDS counter takes at most 7 x kLaneRun, the memory counters are 64-bit); what a lane reads -
// label and rows - was written by launches that ended before this one began, and nothing writes them after a
// successful finish (the head of this file says where that was checked); a root's label is a global id of a PF
// well of an added tile, whose row k_ld_pack wrote.
__global__ void __launch_bounds__(kTdBlock) k_lm_tally(const int *__restrict__ tile_idx, int64_t N,
                                                        const uint32_t *__restrict__ label,
                                                        const uint32_t *__restrict__ rows, int words, int L, int max_d,
                                                        unsigned long long *cnt_t, unsigned long long *cnt_l,
                                                        unsigned long long *sub)
{
    __shared__ uint32_t s_hist[kLmWindow * kLmCell];
    __shared__ uint32_t s_cnt[kLmTileCnt + kLmBins];                  // Pairs, Profiled, Mismatches, WithN, Dist
    const int n_hist = min(L, kLmWindow) * kLmCell;
    for (int e = threadIdx.x; e < n_hist; e += kTdBlock)
        s_hist[e] = 0;
    if (threadIdx.x < kLmTileCnt + kLmBins)
        s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const LaneRun run(tile_idx, N);
    const int ti = run.ti, lane = threadIdx.x & (kWave - 1);
    uint32_t n_pairs = 0, n_prof = 0, n_mis = 0, with_n = 0;         // the first three: the same in every lane of a wave
    run.walk([&](bool has, int64_t, size_t g64) {
        bool pair = false;
        int d = 0;
        LmNotes notes;
        if (has) {
            const uint32_t lab = label[g64];
            if (lab != kInvalid && lab != (uint32_t)g64) {
                pair = true;
                d = min(lm_compare(rows, words, lab, (uint32_t)g64, notes), kLmBins - 1);
            }
        }
        wave_by_key(pair, (uint32_t)d, [&](uint32_t d0, unsigned long long group, bool first) {
            const uint32_t n = (uint32_t)__popcll(group);
            if (first)
                atomicAdd(&s_cnt[kLmTileCnt + d0], n);
            n_pairs += n;
            if (d0 <= (uint32_t)max_d) {
                n_prof += n;
                n_mis += n * d0;
            }
        });
        if (pair && d <= max_d)
            for (int i = 0; i < d; i++) {
                const uint32_t e = notes.pop();
                const uint32_t a = (e >> 3) & 7u, b = e & 7u, cell = (e >> 6) * kLmCell + a * kLmCodes + b;
                with_n += (a == 4u) | (b == 4u);
                if (cell < (uint32_t)n_hist)
                    atomicAdd(&s_hist[cell], 1u);
                else
                    atomicAdd(sub + cell, 1ull);
            }
    });
    if (lane == 0) {
        if (n_pairs)
            atomicAdd(&s_cnt[0], n_pairs);
        if (n_prof)
            atomicAdd(&s_cnt[1], n_prof);
        if (n_mis)
            atomicAdd(&s_cnt[2], n_mis);
    }
    if (with_n)
        atomicAdd(&s_cnt[3], with_n);
    __syncthreads();
    for (int e = threadIdx.x; e < n_hist; e += kTdBlock)
        if (s_hist[e])
            atomicAdd(sub + e, (unsigned long long)s_hist[e]);
    if (threadIdx.x < kLmTileCnt + kLmBins && s_cnt[threadIdx.x]) {
        const unsigned long long v = s_cnt[threadIdx.x];
        if (threadIdx.x < kLmTileCnt)
            atomicAdd(spread_row(cnt_t, (size_t)ti, kLmTileCnt) + threadIdx.x, v);
        else
            atomicAdd(spread_row(cnt_l, 0, kLmLaneCnt) + (threadIdx.x - kLmTileCnt), v);
    }
}

}  // namespace

#ifndef WD_LANE_MISMATCH_EMU                       // (tools/lane_mismatch_emu.cpp: the kernel above on the CPU, a fiber per lane)
extern "C" {

int wd_lane_mismatch_scratch(int max_tiles, int L, size_t *bytes)
{
    if (max_tiles < 0 || L < 0 || !bytes)
        return WD_ERR_ARG;
    if (L > kMaxCycles || max_tiles > 65535)
        return WD_ERR_UNSUPPORTED;
    *bytes = lm_layout_of(max_tiles, L).bytes;
    return WD_OK;
}

int wd_lane_mismatches(wd_lane_dups *ld, int max_d, void *scratch_dev, size_t scratch_bytes, int64_t *lane_row,
                       int64_t *tile_rows, int64_t *sub)
try {
    if (!ld || !lane_row || !tile_rows || !sub)
        return WD_ERR_ARG;
    wd_ctx *ctx = ld->ctx;
    const int64_t N = ld->N;
    const int T = ld->max_tiles, L = ld->L;
    LanePass p(ld);
    if (const int rc = p.finished("lane mismatches come after a successful finish of the lane"))
        return rc;
    if (max_d < 0 || max_d > kLmMaxD)
        return fail(ctx, WD_ERR_ARG, "lane mismatches: max_d is 0.." + std::to_string(kLmMaxD) + ", not " +
                                         std::to_string(max_d));
    const LmLayout lay = lm_layout_of(T, L);
    if (const int rc = p.scratch(scratch_dev, scratch_bytes, lay.bytes, "scratch smaller than wd_lane_mismatch_scratch",
                                 "lane mismatches: the scratch must be in device memory"))
        return rc;
    const size_t n_sub = (size_t)L * kLmCell;
    memset(lane_row, 0, WD_LANEMISMATCH_LANE_COLS * sizeof(int64_t));
    memset(tile_rows, 0, (size_t)T * kLmTileCnt * sizeof(int64_t));
    memset(sub, 0, n_sub * sizeof(int64_t));
    if (!p.start())
        return p.rc;
    uint8_t *sc = (uint8_t *)scratch_dev;
    unsigned long long *cnt_t = (unsigned long long *)(sc + lay.cnt_t);
    unsigned long long *cnt_l = (unsigned long long *)(sc + lay.cnt_l);
    int *d_tidx = (int *)(sc + lay.tidx);
    unsigned long long *d_sub = (unsigned long long *)(sc + lay.sub);
    WD_HIP(ctx, hipMemsetAsync(sc, 0, lay.bytes, ctx->stream));
    if (const int rc = p.upload(d_tidx))
        return rc;
    hipLaunchKernelGGL(k_lm_tally, p.grid, dim3(kTdBlock), 0, ctx->stream, d_tidx, N,
                       (const uint32_t *)(ld->ws + ld->lay.label), (const uint32_t *)(ld->ws + ld->lay.rows), ld->lay.words, L,
                       max_d, cnt_t, cnt_l, d_sub);
    WD_HIP(ctx, hipGetLastError());
    SpreadFetch f_t(cnt_t, (size_t)T, kLmTileCnt), f_l(cnt_l, 1, kLmLaneCnt);
    if (n_sub)
        WD_HIP(ctx, hipMemcpyAsync(sub, d_sub, n_sub * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (const int rc = spread_fetch(ctx, {&f_t, &f_l}))
        return rc;
    lane_pass_rows(f_t, T, tile_rows, lane_row, &f_l, kLmBins);
    return WD_OK;
} WD_CATCH

}  // extern "C"
#endif
