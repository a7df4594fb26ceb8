// lane_quality.inc - a lane's reported base quality against its duplicate copies (include/welldup_lanequality.h):
// a second packed array beside the accumulator's rows, the quality of every well at every scanned cycle reduced to
// the caller's bins, and after a finish the (pair, cycle) observations counted by the bins of root and member, all of
// them and those at which the bases differ.  Included at the end of welldup_tiledups.hip, after lane_distance.inc: it
// uses read_classes.inc (the plane loads, the spread counters), lane_dups.inc (the accumulator, its packed rows and
// label array, the staged store of k_ld_pack, ld_tiles_added), lane_mismatch.inc (lm_compare, lm_fold) and, for
// wd_lane_qualities, lane_pass.inc as lane_mismatch.inc does.
//
// wd_lane_qual_add, per batch of tiles (grid y = tile of the batch):
//   k_lq_pack        the pass of k_ld_pack over the same planes; of every byte it keeps the bin of byte >> 2 where
//                    k_ld_pack keeps the base, and it counts the raw qualities of the PF wells (QHist)
// wd_lane_qualities, over the tiles that were added (grid y = tile): one kernel, k_lq_tally, and nothing else.  It
// reads rows, label and the quality rows and writes the caller's scratch only.  rows and label do not change once a
// finish has succeeded (the head of lane_mismatch.inc says where that was checked; this pass joins that list as a
// reader); the quality rows are written by k_lq_pack alone, in wd_lane_qual_add, which refuses after a finish.
#include "welldup_lanequality.h"

namespace {

constexpr int kLqBins = WD_LANEQUALITY_MAX_BINS;
constexpr int kLqCells = kLqBins * kLqBins;        // entries of Obs, and of Mis
constexpr int kLqValues = WD_LANEQUALITY_VALUES;
constexpr int kLqTileCnt = WD_LANEQUALITY_TILE_COLS;       // per tile and copy: Pairs, Profiled, Observations, Mismatches
static_assert(kLqBins == 8, "a bin is a 3-bit code of a packed row");
static_assert(WD_LANEQUALITY_MAX_D == kLmMaxD, "a profiled pair is lane_mismatch.inc's");
static_assert((unsigned long long)kLaneRun * kMaxCycles < (1ull << 32), "a 32-bit LDS counter must hold a run's observations");

// the scratch of wd_lane_qualities (include/welldup_lanequality.h states the arithmetic)
struct LqScratch {
    size_t cnt_t, cells, tidx, bytes;
};

LqScratch lq_scratch_of(int max_tiles)
{
    LqScratch l;
    const size_t t = (size_t)max_tiles;
    l.cnt_t = 0;
    l.cells = align256(l.cnt_t + t * kSpread * kLqTileCnt * 8);
    l.tidx = align256(l.cells + (size_t)kSpread * 2 * kLqCells * 8);
    l.bytes = align256(l.tidx + t * sizeof(int));
    return l;
}

// The cell a lane is counting into and what it has for it, in three registers: a pair's observations are added to
// LDS when the cell changes and when the pair ends.
struct LqCell {
    uint32_t cell = 0, obs = 0, mis = 0;
    __device__ void flush(uint32_t *s_hist)
    {
        if (obs)
            atomicAdd(&s_hist[cell], obs);
        if (mis)
            atomicAdd(&s_hist[kLqCells + cell], mis);
        obs = mis = 0;
    }
};

// the codes of word k that are cycles (the unused codes of the last word are zero in all four rows and are no
// observations), one bit each at the code's lowest bit
__device__ inline uint32_t lq_valid(int k, int L)
{
    const int n = min(kFpCycles, L - k * kFpCycles);
    return kLmLow & (0x3FFFFFFFu >> (3 * (kFpCycles - n)));
}

// One word of a profiled pair: valid = its codes that are cycles, m = those at which the bases differ (lm_fold),
// xq and yq the root's and the member's quality codes.  The lowest code not yet counted names a cell (a, b); the
// codes of the word with the same (a, b) are found at once - XOR with a and with b broadcast to all ten codes
// leaves zero exactly there, and the fold of lm_fold turns that into a bit per code - and are counted by two
// popcounts.  A word of one quality pair is one trip, a word of binned real qualities a few.
__device__ inline void lq_word(uint32_t valid, uint32_t m, uint32_t xq, uint32_t yq, LqCell &cur, uint32_t *s_hist)
{
    uint32_t rest = valid;
    while (rest) {
        const int bit = __ffs((int)rest) - 1;
        const uint32_t a = (xq >> bit) & 7u, b = (yq >> bit) & 7u, cell = a * kLqBins + b;
        const uint32_t same = rest & ~(lm_fold(xq, a * kLmLow) | lm_fold(yq, b * kLmLow));
        if (cell != cur.cell) {
            cur.flush(s_hist);
            cur.cell = cell;
        }
        cur.obs += (uint32_t)__popc(same);
        cur.mis += (uint32_t)__popc(same & m);
        rest &= ~same;
    }
}

// The L observations of the pair (a the root, b the member) into the workgroup's histogram: four rows side by side,
// as 16-byte pieces where a row is a whole number of them, else four words of each in flight.
__device__ inline void lq_pair(const uint32_t *__restrict__ rows, const uint32_t *__restrict__ qrows, int words, int L,
                               uint32_t a, uint32_t b, uint32_t *s_hist)
{
    const uint32_t *x = rows + (size_t)a * words, *y = rows + (size_t)b * words;
    const uint32_t *xq = qrows + (size_t)a * words, *yq = qrows + (size_t)b * words;
    LqCell cur;
    int i = 0;
    if ((words & 3) == 0) {
        for (; i < words; i += 4) {
            const uint4 p = *(const uint4 *)(x + i), q = *(const uint4 *)(y + i);
            const uint4 pq = *(const uint4 *)(xq + i), qq = *(const uint4 *)(yq + i);
            lq_word(lq_valid(i, L), lm_fold(p.x, q.x), pq.x, qq.x, cur, s_hist);
            lq_word(lq_valid(i + 1, L), lm_fold(p.y, q.y), pq.y, qq.y, cur, s_hist);
            lq_word(lq_valid(i + 2, L), lm_fold(p.z, q.z), pq.z, qq.z, cur, s_hist);
            lq_word(lq_valid(i + 3, L), lm_fold(p.w, q.w), pq.w, qq.w, cur, s_hist);
        }
    } else {
        for (; i + 4 <= words; i += 4) {
            uint32_t p[4], q[4], pq[4], qq[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                p[j] = x[i + j];
                q[j] = y[i + j];
                pq[j] = xq[i + j];
                qq[j] = yq[i + j];
            }
#pragma unroll
            for (int j = 0; j < 4; j++)
                lq_word(lq_valid(i + j, L), lm_fold(p[j], q[j]), pq[j], qq[j], cur, s_hist);
        }
        for (; i < words; i++)
            lq_word(lq_valid(i, L), lm_fold(x[i], y[i]), xq[i], yq[i], cur, s_hist);
    }
    cur.flush(s_hist);
}

// ---- tally --------------------------------------------------------------------------------------
// LaneRun's grid and walk (lane_pass.inc), k_lm_tally's pairs: a well that is PF (it has a label) and not its own
// root; d is lm_compare's.
//   - Pairs, Profiled, Observations and Mismatches.  The pairs of a wave are grouped by d (wave_by_key): Profiled and
//     Mismatches (d x the group's size for d <= max_d) are the same for every lane of the wave, are summed in
//     registers over the run and added to LDS once by the wave's first lane.  Observations is Profiled x L; what
//     lq_pair counted cell by cell must add up to it, which the tests hold it to.
//   - Obs and Mis.  A profiled pair walks its four rows (lq_pair) and counts into an LDS histogram of 2 x 64 32-bit
//     counters (a run adds at most kLaneRun x 1024 to one).  The worst lane is one of equal reads with one quality
//     value: every well is a profiled pair and every observation lands in one cell.  An LDS add per observation
//     would put 64 lanes on one word L times per pair; counted as lq_word counts, such a pair costs one add, and a
//     pair of binned real qualities a handful.
// At the end the workgroup adds what is not zero to its copy of the spread counters.
// Why the result is exact and does not depend on the order of execution: k_lm_tally's argument - every output is a
// sum over wells, each well is visited by exactly one lane of one workgroup, integer adds commute and none can
// overflow; label, rows and the quality rows were written by launches that ended before this one began; a root's
// label is a global id of a PF well of an added tile, whose rows k_ld_pack and k_lq_pack wrote (the host refuses a
// tile that has the one and not the other).
__global__ void __launch_bounds__(kTdBlock) k_lq_tally(const int *__restrict__ tile_idx, int64_t N,
                                                        const uint32_t *__restrict__ label,
                                                        const uint32_t *__restrict__ rows,
                                                        const uint32_t *__restrict__ qrows, int words, int L, int max_d,
                                                        unsigned long long *cnt_t, unsigned long long *cells)
{
    __shared__ uint32_t s_hist[2 * kLqCells];                          // Obs, then Mis
    __shared__ uint32_t s_cnt[kLqTileCnt];
    if (threadIdx.x < 2 * kLqCells)
        s_hist[threadIdx.x] = 0;
    if (threadIdx.x < kLqTileCnt)
        s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const LaneRun run(tile_idx, N);
    const int ti = run.ti, lane = threadIdx.x & (kWave - 1);
    uint32_t n_pairs = 0, n_prof = 0, n_mis = 0;                     // the same in every lane of a wave
    run.walk([&](bool has, int64_t, size_t g64) {
        bool pair = false;
        int d = 0;
        uint32_t lab = kInvalid;
        if (has) {
            lab = label[g64];
            if (lab != kInvalid && lab != (uint32_t)g64) {
                LmNotes notes;
                pair = true;
                d = min(lm_compare(rows, words, lab, (uint32_t)g64, notes), kLmBins - 1);
            }
        }
        wave_by_key(pair, (uint32_t)d, [&](uint32_t d0, unsigned long long group, bool) {
            const uint32_t n = (uint32_t)__popcll(group);
            n_pairs += n;
            if (d0 <= (uint32_t)max_d) {
                n_prof += n;
                n_mis += n * d0;
            }
        });
        if (pair && d <= max_d)
            lq_pair(rows, qrows, words, L, lab, (uint32_t)g64, s_hist);
    });
    if (lane == 0) {
        if (n_pairs)
            atomicAdd(&s_cnt[0], n_pairs);
        if (n_prof) {
            atomicAdd(&s_cnt[1], n_prof);
            atomicAdd(&s_cnt[2], n_prof * (uint32_t)L);
        }
        if (n_mis)
            atomicAdd(&s_cnt[3], n_mis);
    }
    __syncthreads();
    if (threadIdx.x < 2 * kLqCells && s_hist[threadIdx.x])
        atomicAdd(spread_row(cells, 0, 2 * kLqCells) + threadIdx.x, (unsigned long long)s_hist[threadIdx.x]);
    if (threadIdx.x < kLqTileCnt && s_cnt[threadIdx.x])
        atomicAdd(spread_row(cnt_t, (size_t)ti, kLqTileCnt) + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

}  // namespace

#ifndef WD_LANE_QUALITY_EMU                        // (tools/lane_quality_emu.cpp: the kernel above on the CPU, a fiber per lane)
namespace {

// the quality workspace (include/welldup_lanequality.h states the arithmetic)
struct LqLayout {
    size_t qhist, planes, filt, tidx, qrows, bytes;
};

LqLayout lq_layout_of(int64_t N, int max_tiles, int L)
{
    LqLayout l;
    const size_t t = (size_t)max_tiles, wells = (size_t)N * t;
    const int words = (L + kFpCycles - 1) / kFpCycles;
    l.qhist = 0;
    l.planes = align256(l.qhist + (size_t)kSpread * kLqValues * 8);
    l.filt = align256(l.planes + t * (size_t)L * sizeof(void *));
    l.tidx = align256(l.filt + t * sizeof(void *));
    l.qrows = align256(l.tidx + t * sizeof(int));
    l.bytes = align256(l.qrows + wells * (size_t)words * 4);
    return l;
}

// ---- pack ---------------------------------------------------------------------------------------
// The table quality -> bin, 64 entries of three bits, as three 64-bit words: bit q of p[i] is bit i of bin(q).  They
// are kernel arguments, the same for every lane, and a lookup is three shifts by q: no array is indexed.
struct LqTable {
    unsigned long long p0, p1, p2;
};

__device__ inline uint32_t lq_bin(const LqTable &t, uint32_t q)
{
    return ((uint32_t)(t.p0 >> q) & 1u) | ((uint32_t)(t.p1 >> q) & 1u) << 1 | ((uint32_t)(t.p2 >> q) & 1u) << 2;
}

// QHist of a lane's PF wells: the quality it saw last and how often in a row, added to the workgroup's histogram
// when another value comes and at the end.  A lane of one quality value - or an instrument that reports a few levels,
// most bases at the highest - would otherwise put 64 lanes on one LDS word for every byte of the planes.
struct LqRunLength {
    uint32_t q = 0, n = 0;
    __device__ void add(uint32_t v, uint32_t *s_qh)
    {
        if (v != q) {
            flush(s_qh);
            q = v;
        }
        n++;
    }
    __device__ void flush(uint32_t *s_qh)
    {
        if (n)
            atomicAdd(&s_qh[q], n);
        n = 0;
    }
};

// plane_word4 for the qualities: one word of wells w .. w + 3 from dword loads, planes c .. c1 - 1 (FULL: ten, all in
// flight); pf: bit i set if well w + i passes the filter.  A no-call is byte 0: its quality is 0 as it stands.
template <bool FULL>
__device__ inline void lq_word4(const uint8_t *const *pl, int c, int c1, int64_t w, uint32_t pf, const LqTable &tbl,
                                LqRunLength &run, uint32_t *s_qh, uint32_t (&acc)[4])
{
    uint32_t v[kFpCycles];
    const int n = FULL ? kFpCycles : c1 - c;
#pragma unroll
    for (int j = 0; j < kFpCycles; j++)
        if (FULL || j < n)                                 // (non-temporal: the planes are streamed)
            v[j] = __builtin_nontemporal_load((const uint32_t *)(pl[c + j] + w));
#pragma unroll
    for (int q = 0; q < 4; q++)
        acc[q] = 0;
#pragma unroll
    for (int j = 0; j < kFpCycles; j++)
        if (FULL || j < n) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint32_t qual = (v[j] >> (8 * q + 2)) & 0x3Fu;
                acc[q] |= lq_bin(tbl, qual) << (3 * j);
                if (pf >> q & 1u)
                    run.add(qual, s_qh);
            }
        }
}

// one well, byte loads: unaligned planes, and the last N % 4 wells of a tile
__device__ inline void lq_pack_well(const uint8_t *const *pl, bool pf, int L, int words, int64_t w, size_t g,
                                    const LqTable &tbl, LqRunLength &run, uint32_t *s_qh, uint32_t *__restrict__ qrows)
{
    for (int c = 0, k = 0; c < L; c += kFpCycles, k++) {
        uint32_t acc = 0;
        for (int j = 0; j < kFpCycles && c + j < L; j++) {
            const uint32_t qual = (uint32_t)pl[c + j][w] >> 2;
            acc |= lq_bin(tbl, qual) << (3 * j);
            if (pf)
                run.add(qual, s_qh);
        }
        qrows[g * words + k] = acc;
    }
}

// k_ld_pack's grids, loads and stores (see there: a workgroup of the VEC4 kernel is one wave that stages kLdChunk
// words of its 256 wells in LDS and writes them out as pieces of rows).  QHist: a lane counts its PF wells' raw
// qualities by run length into the workgroup's 64 LDS counters (at most 256 x 1024 each), which go to the
// workgroup's copy of the spread counters at the end.
template <bool VEC4>
__global__ void __launch_bounds__(VEC4 ? kWave : kTdBlock) k_lq_pack(const uint8_t *const *__restrict__ planes,
                                                                      const uint8_t *const *__restrict__ filt,
                                                                      const int *__restrict__ tile_idx, int L, int words,
                                                                      int64_t N, LqTable tbl, uint32_t *__restrict__ qrows,
                                                                      unsigned long long *qhist)
{
    __shared__ uint32_t s_qh[kLqValues];
    __shared__ __attribute__((aligned(16))) uint32_t s_words[VEC4 ? kLdChunk * kLdStride : 4];
    if (threadIdx.x < kLqValues)
        s_qh[threadIdx.x] = 0;
    __syncthreads();
    const int tile = blockIdx.y;
    const uint8_t *const *pl = planes + (size_t)tile * L;
    const uint8_t *f = filt[tile];
    const size_t tile_base = (size_t)tile_idx[tile] * (size_t)N;
    LqRunLength run;
    if constexpr (!VEC4) {
        const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
        if (w < N)
            lq_pack_well(pl, f[w] & 1u, L, words, w, tile_base + (size_t)w, tbl, run, s_qh, qrows);
    } else {
        const int lane = threadIdx.x;
        const int64_t wave0 = (int64_t)blockIdx.x * kLdWaveWells;              // (< N: the grid is cut to the tile)
        const int64_t w0 = wave0 + 4 * lane;
        const bool quad = w0 + 4 <= N;                                         // else: past the tile, or in its last N % 4 wells
        const int n_quad = (int)(min((int64_t)kLdWaveWells, N - wave0) & ~(int64_t)3);
        uint32_t *out = qrows + (tile_base + (size_t)wave0) * words;
        uint32_t pf = 0;
        if (quad)
            pf = (f[w0] & 1u) | (f[w0 + 1] & 1u) << 1 | (f[w0 + 2] & 1u) << 2 | (f[w0 + 3] & 1u) << 3;
        for (int c = 0, k = 0; c < L;) {
            int kc = 0;                                                        // words staged (the same for every lane)
            for (; kc < kLdChunk && c < L; kc++, c += kFpCycles) {
                if (quad) {
                    uint32_t acc[4];
                    if (c + kFpCycles <= L)
                        lq_word4<true>(pl, c, L, w0, pf, tbl, run, s_qh, acc);
                    else
                        lq_word4<false>(pl, c, L, w0, pf, tbl, run, s_qh, acc);
                    *(uint4 *)(s_words + kc * kLdStride + 4 * lane) = make_uint4(acc[0], acc[1], acc[2], acc[3]);
                }
            }
            __syncthreads();
            ld_store_staged(s_words, out, words, k, kc, n_quad, lane);
            k += kc;
            __syncthreads();
        }
        if (!quad)
            for (int64_t w = w0; w < N; w++)                                   // (nothing for a lane past the tile)
                lq_pack_well(pl, f[w] & 1u, L, words, w, tile_base + (size_t)w, tbl, run, s_qh, qrows);
    }
    run.flush(s_qh);
    __syncthreads();
    if (threadIdx.x < kLqValues && s_qh[threadIdx.x])
        atomicAdd(spread_row(qhist, 0, kLqValues) + threadIdx.x, (unsigned long long)s_qh[threadIdx.x]);
}

}  // namespace

// the quality part of an accumulator: the host side (the device side is the caller's quality workspace)
struct wd_lane_quality {
    int n_bins;
    LqTable tbl;
    LqLayout lay;
    uint8_t *ws;
    std::vector<char> added;                       // by tile index: qualities given
};

extern "C" {

int wd_lane_qual_workspace(int64_t N, int max_tiles, int L, size_t *bytes)
{
    size_t ws = 0;
    if (!bytes)
        return WD_ERR_ARG;
    if (const int rc = wd_lane_dups_workspace(N, max_tiles, L, &ws))       // (the limits of a lane)
        return rc;
    *bytes = lq_layout_of(N, max_tiles, L).bytes;
    return WD_OK;
}

int wd_lane_qual_begin(wd_lane_dups *ld, int n_bins, const int *edges, void *workspace_dev, size_t workspace_bytes)
try {
    if (!ld)
        return WD_ERR_ARG;
    wd_ctx *ctx = ld->ctx;
    if (n_bins < 1 || n_bins > kLqBins || !edges)
        return fail(ctx, WD_ERR_ARG, "lane qualities: 1.." + std::to_string(kLqBins) + " bins, not " + std::to_string(n_bins));
    for (int i = 0; i < n_bins; i++)
        if (edges[i] < 0 || edges[i] >= kLqValues || (i == 0 ? edges[0] != 0 : edges[i] < edges[i - 1]))
            return fail(ctx, WD_ERR_ARG, "lane qualities: the bins' lower edges ascend from 0 and end at most at 63; edge " +
                                             std::to_string(i) + " is " + std::to_string(edges[i]));
    if (ld->finished || ld->resolved)
        return fail(ctx, WD_ERR_ARG, "lane qualities: begin after finish");
    if (ld->qual)
        return fail(ctx, WD_ERR_ARG, "lane qualities: begin is called once");
    if (!ld_tiles_added(ld).empty())
        return fail(ctx, WD_ERR_ARG, "lane qualities: begin comes before the first wd_lane_dups_add");
    const LqLayout lay = lq_layout_of(ld->N, ld->max_tiles, ld->L);
    if (!workspace_dev || workspace_bytes < lay.bytes)
        return fail(ctx, WD_ERR_ARG, "workspace smaller than wd_lane_qual_workspace");
    if (!on_device(workspace_dev))
        return fail(ctx, WD_ERR_ARG, "lane qualities: the workspace must be in device memory");
    if (bind_device(ctx))
        return WD_ERR_HIP;
    auto lq = std::make_shared<wd_lane_quality>();
    lq->n_bins = n_bins;
    lq->tbl = LqTable{0, 0, 0};
    for (int q = 0, b = 0; q < kLqValues; q++) {
        while (b + 1 < n_bins && edges[b + 1] <= q)
            b++;
        lq->tbl.p0 |= (unsigned long long)(b & 1) << q;
        lq->tbl.p1 |= (unsigned long long)(b >> 1 & 1) << q;
        lq->tbl.p2 |= (unsigned long long)(b >> 2 & 1) << q;
    }
    lq->lay = lay;
    lq->ws = (uint8_t *)workspace_dev;
    lq->added.assign((size_t)ld->max_tiles, 0);
    WD_HIP(ctx, hipMemsetAsync(lq->ws + lay.qhist, 0, lay.planes - lay.qhist, ctx->stream));
    WD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ld->qual = lq;
    return WD_OK;
} WD_CATCH

int wd_lane_qual_add(wd_lane_dups *ld, int n_tiles, const int *tile_index, const uint8_t *const *planes,
                     const uint8_t *const *filter)
try {
    wd_lane_quality *lq = ld ? ld->qual.get() : nullptr;
    std::vector<char> seen;
    if (const int rc = lane_add_open(ld, lq ? &lq->added : nullptr, n_tiles, tile_index, filter && (planes || !ld || ld->L <= 0),
                                     {"lane qualities", "lane qualities: add before wd_lane_qual_begin",
                                      "lane qualities read a plane per cycle (well_stride 1)",
                                      "null tile index, plane or filter table"},
                                     seen))
        return rc;
    if (n_tiles == 0)
        return WD_OK;
    wd_ctx *ctx = ld->ctx;
    const int L = ld->L;
    const int64_t N = ld->N;
    bool aligned4;
    if (const int rc = check_tables(ctx, "lane qualities: ", n_tiles, L, planes, filter, nullptr, &aligned4))
        return rc;
    if (bind_device(ctx))
        return WD_ERR_HIP;
    if (N > 0) {
        const LqLayout &lay = lq->lay;
        uint8_t *ws = lq->ws;
        const uint8_t **d_planes = (const uint8_t **)(ws + lay.planes);
        const uint8_t **d_filt = (const uint8_t **)(ws + lay.filt);
        int *d_tidx = (int *)(ws + lay.tidx);
        uint32_t *qrows = (uint32_t *)(ws + lay.qrows);
        unsigned long long *qhist = (unsigned long long *)(ws + lay.qhist);
        if (const int rc = upload_tables(ctx, n_tiles, L, planes, d_planes, filter, d_filt))
            return rc;
        WD_HIP(ctx, hipMemcpyAsync(d_tidx, tile_index, n_tiles * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        if (aligned4)
            hipLaunchKernelGGL(k_lq_pack<true>, dim3((unsigned)((N + kLdWaveWells - 1) / kLdWaveWells), (unsigned)n_tiles),
                               dim3(kWave), 0, ctx->stream, d_planes, d_filt, d_tidx, L, ld->lay.words, N, lq->tbl, qrows,
                               qhist);
        else
            hipLaunchKernelGGL(k_lq_pack<false>, dim3((unsigned)((N + kTdBlock - 1) / kTdBlock), (unsigned)n_tiles),
                               dim3(kTdBlock), 0, ctx->stream, d_planes, d_filt, d_tidx, L, ld->lay.words, N, lq->tbl, qrows,
                               qhist);
        WD_HIP(ctx, hipGetLastError());
        // (the pointer tables are the next call's too, and the caller may reuse the planes at once)
        WD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    lq->added.swap(seen);
    return WD_OK;
} WD_CATCH

int wd_lane_qual_scratch(int max_tiles, size_t *bytes)
{
    if (max_tiles < 0 || !bytes)
        return WD_ERR_ARG;
    if (max_tiles > 65535)
        return WD_ERR_UNSUPPORTED;
    *bytes = lq_scratch_of(max_tiles).bytes;
    return WD_OK;
}

int wd_lane_qualities(wd_lane_dups *ld, int max_d, void *scratch_dev, size_t scratch_bytes, int64_t *lane_row,
                      int64_t *tile_rows, int64_t *qhist, int64_t *obs, int64_t *mis)
try {
    if (!ld || !lane_row || !tile_rows || !qhist || !obs || !mis)
        return WD_ERR_ARG;
    wd_ctx *ctx = ld->ctx;
    wd_lane_quality *lq = ld->qual.get();
    const int64_t N = ld->N;
    const int T = ld->max_tiles, L = ld->L;
    if (!lq)
        return fail(ctx, WD_ERR_ARG, "lane qualities come after wd_lane_qual_begin");
    LanePass p(ld);
    if (const int rc = p.finished("lane qualities come after a successful finish of the lane"))
        return rc;
    if (max_d < 0 || max_d > kLmMaxD)
        return fail(ctx, WD_ERR_ARG, "lane qualities: max_d is 0.." + std::to_string(kLmMaxD) + ", not " +
                                         std::to_string(max_d));
    const LqScratch lay = lq_scratch_of(T);
    if (const int rc = p.scratch(scratch_dev, scratch_bytes, lay.bytes, "scratch smaller than wd_lane_qual_scratch",
                                 "lane qualities: the scratch must be in device memory"))
        return rc;
    if (const int rc = lane_part_tiles(ld, lq->added, "lane qualities", "qualities"))
        return rc;
    memset(lane_row, 0, WD_LANEQUALITY_LANE_COLS * sizeof(int64_t));
    memset(tile_rows, 0, (size_t)T * kLqTileCnt * sizeof(int64_t));
    memset(qhist, 0, kLqValues * sizeof(int64_t));
    memset(obs, 0, kLqCells * sizeof(int64_t));
    memset(mis, 0, kLqCells * sizeof(int64_t));
    if (!p.start())
        return p.rc;
    uint8_t *sc = (uint8_t *)scratch_dev;
    unsigned long long *cnt_t = (unsigned long long *)(sc + lay.cnt_t);
    unsigned long long *cells = (unsigned long long *)(sc + lay.cells);
    int *d_tidx = (int *)(sc + lay.tidx);
    WD_HIP(ctx, hipMemsetAsync(sc, 0, lay.bytes, ctx->stream));
    if (const int rc = p.upload(d_tidx))
        return rc;
    hipLaunchKernelGGL(k_lq_tally, p.grid, dim3(kTdBlock), 0, ctx->stream, d_tidx, N,
                       (const uint32_t *)(ld->ws + ld->lay.label), (const uint32_t *)(ld->ws + ld->lay.rows),
                       (const uint32_t *)(lq->ws + lq->lay.qrows), ld->lay.words, L, max_d, cnt_t, cells);
    WD_HIP(ctx, hipGetLastError());
    SpreadFetch f_t(cnt_t, (size_t)T, kLqTileCnt), f_c(cells, 1, 2 * kLqCells), f_q(lq->ws + lq->lay.qhist, 1, kLqValues);
    if (const int rc = spread_fetch(ctx, {&f_t, &f_c, &f_q}))
        return rc;
    lane_pass_rows(f_t, T, tile_rows, lane_row);
    unsigned long long c[2 * kLqCells], q[kLqValues];
    f_c.sum(0, c);
    f_q.sum(0, q);
    for (int e = 0; e < kLqCells; e++) {
        obs[e] = (int64_t)c[e];
        mis[e] = (int64_t)c[kLqCells + e];
    }
    for (int v = 0; v < kLqValues; v++)
        qhist[v] = (int64_t)q[v];
    return WD_OK;
} WD_CATCH

}  // extern "C"

// The unit ends with the line that includes this file (tests/test_lanequality_host.py holds it to that), so what
// comes after it in the unit is included from here: a lane's distinct reads against its depth
// (include/welldup_lanesaturation.h), which uses nothing of this file.
#include "lane_saturation.inc"
#endif
