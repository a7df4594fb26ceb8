// lane_gc.inc - a lane's duplication against its reads' GC content (include/welldup_lanegc.h): every PF well of a
// lane counted by the GC of its own read and by what it is in its group - a lone read, the first well of a group, or
// a copy -, with the group's size summed at the root's GC.  Included at the end of welldup_tiledups.hip, after
// lane_distance.inc and before lane_quality.inc and what that includes: it uses read_classes.inc (the spread
// counters), lane_dups.inc (the accumulator, its label, members and packed rows), lane_mismatch.inc's kLmLow and
// lane_pass.inc as lane_mismatch.inc does.
//
// wd_lane_gc, over the tiles that were added (grid y = tile): one kernel, k_lgc_tally, and nothing else.  It reads
// label, members and the rows and writes the caller's scratch only.  Who writes label and the rows, and that nobody
// does after a successful finish, is listed at the head of lane_mismatch.inc; this pass joins that list as a reader.
// members: k_ld_pack clears it, k_ld_resolve counts it at the representatives (the equality finish, once); the near
// finish - checked there, lane_near.inc, wd_lane_near_dups_finish - clears it again in k_ln_compress and recounts it
// at the clusters' roots in k_ln_members (near_core.inc, near_members: one add per wave and root of the wells whose
// label is not their own id), both before that finish returns and only when it succeeds: a finish refused over
// budget returns before them and leaves `finished` unset.  So after either finish members[root] = the group's size
// - 1 and members of a single well is 0, which lane_top.inc relies on as well.
//
// This is the first pass after a finish that reads every row of the lane (30.9 GB at 112 tiles x 151 cycles), so how
// it loads them decides its time: see k_lgc_tally.
#include "welldup_lanegc.h"

namespace {

constexpr int kLgcCols = WD_LANEGC_HIST_COLS;      // Single, Roots, Copies, FamilyWells
constexpr int kLgcWindow = 768;                    // values of g a workgroup counts in LDS
constexpr int kLgcTileCnt = 10;                    // per tile and copy: the lane row's eight columns, GC, CopiesGC
constexpr int kLgcGc = 8, kLgcCopiesGc = 9;
constexpr int kLgcSkip = 4;                        // the Skip columns follow the populations in the same order
static_assert(WD_LANEGC_LANE_COLS == 8 && WD_LANEGC_TILE_COLS == 5, "the rows of welldup_lanegc.h");
static_assert(kLgcWindow * kLgcCols * 4 + 2 * kTdBlock * 4 + kLgcTileCnt * 4 <= 16384,
              "the histogram, the wells' sums and the counters: 16 KB of LDS, k_lm_tally's budget");
static_assert(kMaxCycles <= 1024 && kMaxCycles < (1 << 15), "g and n of a well share a 32-bit word, 16 bits each");

// the scratch (include/welldup_lanegc.h states the arithmetic)
struct LgcLayout {
    size_t cnt_t, hist, tidx, bytes;
};

LgcLayout lgc_layout_of(int max_tiles, int L)
{
    LgcLayout l;
    const size_t t = (size_t)max_tiles;
    l.cnt_t = 0;
    l.hist = align256(l.cnt_t + t * kSpread * kLgcTileCnt * 8);
    l.tidx = align256(l.hist + (size_t)(L + 1) * kSpread * kLgcCols * 8);
    l.bytes = align256(l.tidx + t * sizeof(int));
    return l;
}

// a row of the histogram in memory: the workgroup's copy (WD_LGC_ONE_COPY, measurements only: everybody's first copy)
__device__ inline unsigned long long *lgc_hist_row(unsigned long long *hist, uint32_t g)
{
#ifdef WD_LGC_ONE_COPY
    return hist + (size_t)g * kSpread * kLgcCols;
#else
    return spread_row(hist, (size_t)g, kLgcCols);
#endif
}

// g and n of the ten codes of a word, g in the low half and n in the high: a code is C or G when its two low bits
// differ and its high bit is clear, N when the high bit is set (A 000, C 001, G 010, T 011, N 100).  The unused
// codes of a row's last word are zero - A - and count as neither.
__device__ inline uint32_t lgc_count(uint32_t w)
{
    const uint32_t lo = w & kLmLow, mid = (w >> 1) & kLmLow, hi = (w >> 2) & kLmLow;
    return (uint32_t)__popc((lo ^ mid) & ~hi) | (uint32_t)__popc(hi) << 16;
}

// Words v .. v + 3 of the rows, rows + v on a 16-byte boundary: one 16-byte load where the piece lies inside the
// trip's span [s0, s1), and word by word what of it does at the span's two ends - nothing outside the span is read,
// so nothing outside the rows is.
__device__ inline uint4 lgc_piece(const uint32_t *__restrict__ rows, int64_t v, int64_t s0, int64_t s1)
{
    if (v >= s0 && v + 4 <= s1)
        return *(const uint4 *)(rows + v);
    uint4 p = make_uint4(0, 0, 0, 0);
    if (v >= s0 && v < s1)
        p.x = rows[v];
    if (v + 1 >= s0 && v + 1 < s1)
        p.y = rows[v + 1];
    if (v + 2 >= s0 && v + 2 < s1)
        p.z = rows[v + 2];
    if (v + 3 >= s0 && v + 3 < s1)
        p.w = rows[v + 3];
    return p;
}

// The counts of a piece added to its wells' sums: word i of the span (i0 .. i0 + 3 here, those in 0 .. ns - 1)
// belongs to well i / words of the trip.  One division per piece; the words of one well are added up before they go
// to LDS, so a piece inside a row is one add.
__device__ inline void lgc_add(uint32_t *s_well, const uint4 &p, int i0, int ns, int words)
{
    const int first = max(i0, 0);
    int well = (int)((uint32_t)first / (uint32_t)words), r = first - well * words;
    uint32_t acc = 0;
    auto word = [&](int i, uint32_t w) {
        if (i < 0 || i >= ns)
            return;
        acc += lgc_count(w);
        if (++r == words) {
            if (acc)
                atomicAdd(&s_well[well], acc);
            acc = 0;
            r = 0;
            well++;
        }
    };
    word(i0, p.x);
    word(i0 + 1, p.y);
    word(i0 + 2, p.z);
    word(i0 + 3, p.w);
    if (acc)
        atomicAdd(&s_well[well], acc);
}

// ---- tally --------------------------------------------------------------------------------------
// LaneRun's grid and walk (lane_pass.inc).  A trip of the walk is 256 consecutive wells of a tile, and their rows are
// one contiguous span of 256 x words 32-bit words: every well's row is needed, PF or not being known only from label.
//   - Loading the rows.  The span is read as 16-byte pieces on 16-byte boundaries, neighbouring lanes neighbouring
//     pieces, two pieces per lane in flight: a wave's load instruction asks for 1024 contiguous bytes, each 128-byte
//     line once.  A lane walking its own row would ask for 64 lines per instruction at a stride of 4 x words bytes
//     and come back to each line 32 / words .. times (lane_dups.inc records what that shape cost on the store side,
//     0.94 ms against 0.40 ms per tile).  A tile's first row is only 4-byte aligned when N x words is odd, and the
//     rows' base is whatever the caller's workspace gives: the pieces are cut by the ADDRESS (mis = the words the
//     base lies past a 16-byte boundary), and the words of the first and last piece that lie inside the span are
//     loaded one by one (lgc_piece).  Compile with WD_LGC_ROW_PER_LANE for the row-per-lane shape (measurements only).
//   - From words to wells.  A lane counts g and n of its piece's words (lgc_count) and adds them to the sums of the
//     wells they belong to, s_well[256] in LDS, g and n in the halves of a word (each at most 1024 < 2^16): the
//     reverse of ld_store_staged.  The sums are double-buffered by the trip's parity, so a trip costs one barrier: a
//     lane reads and clears its own well's sum after the barrier, and the adds of the trip after the next, which come
//     into the same buffer, are behind the next trip's barrier.
//   - The histogram.  A counted well's key is 4 g + its population; the wells of a wave are grouped by key
//     (wave_by_key: a lane of equal reads has every well of a wave on one key), and the first lane of a group adds
//     the group's size to the workgroup's hist [kLgcWindow][4] in LDS.  A root adds members + 1 to FamilyWells of its
//     g by itself.  g >= kLgcWindow (only reads of more than 767 cycles have it) goes to the workgroup's copy in
//     memory at once, so the result is exact for every L the accumulator takes.
//   - The counters.  The seven counts of the lane row are ballots, the same in every lane of a wave, summed in
//     registers over the run; SkipFamilyWells, GC and CopiesGC are summed per lane and added up over the wave by
//     shuffles at the end.  Counted and CopiesCounted of the tile row are differences the host takes.
// At the end the workgroup adds what is not zero to its copy of the spread counters (spread_row): some 59 000
// workgroups of a lane flushing about 150 entries each onto one copy would be 9 M atomics on a few hundred addresses.
// Bounds: a 32-bit LDS word takes at most kLaneRun ones per run, at most kLaneRun x 1024 of GC, and family sizes
// summed anywhere are sizes of distinct groups, which sum to at most the lane's wells < 2^32; the memory counters are
// 64-bit.  Why the result is exact and does not depend on the order of execution: every output is a sum over wells of
// a value that depends on that well's row, label and members alone, each well is visited by exactly one lane of one
// workgroup and each word of its row by exactly one lane of that workgroup in that trip, integer adds commute and
// none can overflow; what a lane reads was written by launches that ended before this one began, and nothing writes
// it after a successful finish (the head of this file and of lane_mismatch.inc say where that was checked).
__global__ void __launch_bounds__(kTdBlock) k_lgc_tally(const int *__restrict__ tile_idx, int64_t N,
                                                         const uint32_t *__restrict__ label,
                                                         const uint32_t *__restrict__ members,
                                                         const uint32_t *__restrict__ rows, int words, int L, int max_n,
                                                         unsigned long long *cnt_t, unsigned long long *hist)
{
    __shared__ uint32_t s_hist[kLgcWindow * kLgcCols];
    __shared__ uint32_t s_well[2][kTdBlock];
    __shared__ uint32_t s_cnt[kLgcTileCnt];
    const int n_hist = min(L + 1, kLgcWindow) * kLgcCols;
    for (int e = threadIdx.x; e < n_hist; e += kTdBlock)
        s_hist[e] = 0;
    s_well[0][threadIdx.x] = 0;
    s_well[1][threadIdx.x] = 0;
    if (threadIdx.x < kLgcTileCnt)
        s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const LaneRun run(tile_idx, N);
    const int ti = run.ti, lane = threadIdx.x & (kWave - 1);
    const int mis = (int)(((uintptr_t)rows >> 2) & 3);               // words the rows' base lies past a 16-byte boundary
    uint32_t n_pop[3] = {0, 0, 0}, n_skip[3] = {0, 0, 0};             // the same in every lane of a wave
    uint32_t skip_fam = 0, gc_all = 0, gc_copies = 0;                 // this lane's
    int buf = 0;
    run.walk([&](bool has, int64_t w, size_t g64) {
        uint32_t lab = kInvalid, mem = 0;
        if (has) {
            lab = label[g64];
            if (lab == (uint32_t)g64)
                mem = members[g64];
        }
        uint32_t *sw = s_well[buf];
#ifndef WD_LGC_ROW_PER_LANE
        const int64_t w0 = w - threadIdx.x;
        const int64_t s0 = (int64_t)(run.base + (size_t)w0) * words, s1 = s0 + (min(w0 + kTdBlock, run.run1) - w0) * words;
        const int64_t va0 = (s0 + mis) & ~(int64_t)3;                 // (in words from the boundary before the base)
        const int ns = (int)(s1 - s0), np = (int)((s1 + mis - va0 + 3) >> 2);
        for (int q = threadIdx.x; q < np; q += 2 * kTdBlock) {
            const int64_t va = va0 + 4 * (int64_t)q - mis, vb = va + 4 * kTdBlock;
            const bool two = q + kTdBlock < np;
            const uint4 pa = lgc_piece(rows, va, s0, s1);
            const uint4 pb = two ? lgc_piece(rows, vb, s0, s1) : make_uint4(0, 0, 0, 0);
            lgc_add(sw, pa, (int)(va - s0), ns, words);
            if (two)
                lgc_add(sw, pb, (int)(vb - s0), ns, words);
        }
        __syncthreads();
        const uint32_t c = sw[threadIdx.x];
        sw[threadIdx.x] = 0;
#else
        uint32_t c = 0;
        if (has)
            for (int k = 0; k < words; k++)
                c += lgc_count(rows[g64 * words + k]);
#endif
        buf ^= 1;
        const bool pf = lab != kInvalid;
        const uint32_t g = c & 0xFFFFu, n = c >> 16;
        const int pop = !pf ? -1 : lab != (uint32_t)g64 ? 2 : mem ? 1 : 0;
        const bool skip = pf && n > (uint32_t)max_n, counted = pf && !skip;
#pragma unroll
        for (int p = 0; p < 3; p++) {
            n_pop[p] += (uint32_t)__popcll(__ballot(pop == p));
            n_skip[p] += (uint32_t)__popcll(__ballot(pop == p && skip));
        }
        if (counted) {
            gc_all += g;
            if (pop == 2)
                gc_copies += g;
        }
        if (pop == 1) {
            if (skip)
                skip_fam += mem + 1u;
            else if (g < (uint32_t)kLgcWindow)
                atomicAdd(&s_hist[g * kLgcCols + 3], mem + 1u);
            else
                atomicAdd(lgc_hist_row(hist, g) + 3, (unsigned long long)(mem + 1u));
        }
        wave_by_key(counted, g * kLgcCols + (uint32_t)pop, [&](uint32_t k0, unsigned long long group, bool first) {
            if (first) {
                const uint32_t cnt = (uint32_t)__popcll(group);
                if (k0 < (uint32_t)(kLgcWindow * kLgcCols))
                    atomicAdd(&s_hist[k0], cnt);
                else
                    atomicAdd(lgc_hist_row(hist, k0 / kLgcCols) + k0 % kLgcCols, (unsigned long long)cnt);
            }
        });
    });
    for (int off = kWave / 2; off; off >>= 1) {                        // (every lane of the wave takes part)
        skip_fam += (uint32_t)__shfl((int)skip_fam, lane ^ off);
        gc_all += (uint32_t)__shfl((int)gc_all, lane ^ off);
        gc_copies += (uint32_t)__shfl((int)gc_copies, lane ^ off);
    }
    if (lane == 0) {
        const uint32_t v[kLgcTileCnt] = {n_pop[0] + n_pop[1] + n_pop[2], n_pop[0], n_pop[1], n_pop[2], n_skip[0], n_skip[1],
                                         n_skip[2], skip_fam, gc_all, gc_copies};
#pragma unroll
        for (int f = 0; f < kLgcTileCnt; f++)
            if (v[f])
                atomicAdd(&s_cnt[f], v[f]);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n_hist; e += kTdBlock)
        if (s_hist[e])
            atomicAdd(lgc_hist_row(hist, (uint32_t)e / kLgcCols) + e % kLgcCols, (unsigned long long)s_hist[e]);
    if (threadIdx.x < kLgcTileCnt && s_cnt[threadIdx.x])
        atomicAdd(spread_row(cnt_t, (size_t)ti, kLgcTileCnt) + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

}  // namespace

#ifndef WD_LANE_GC_EMU                             // (tools/lane_gc_emu.cpp: the kernel above on the CPU, a fiber per lane)
extern "C" {

int wd_lane_gc_scratch(int max_tiles, int L, size_t *bytes)
{
    if (max_tiles < 0 || L < 0 || !bytes)
        return WD_ERR_ARG;
    if (L > kMaxCycles || max_tiles > 65535)
        return WD_ERR_UNSUPPORTED;
    *bytes = lgc_layout_of(max_tiles, L).bytes;
    return WD_OK;
}

int wd_lane_gc(wd_lane_dups *ld, int max_n, void *scratch_dev, size_t scratch_bytes, int64_t *lane_row,
               int64_t *tile_rows, int64_t *hist)
try {
    if (!ld || !lane_row || !tile_rows || !hist)
        return WD_ERR_ARG;
    wd_ctx *ctx = ld->ctx;
    const int64_t N = ld->N;
    const int T = ld->max_tiles, L = ld->L;
    LanePass p(ld);
    if (const int rc = p.finished("lane gc comes after a successful finish of the lane"))
        return rc;
    if (max_n < 0 || max_n > L)
        return fail(ctx, WD_ERR_ARG, "lane gc: max_n is 0.." + std::to_string(L) + ", not " + std::to_string(max_n));
    const LgcLayout lay = lgc_layout_of(T, L);
    if (const int rc = p.scratch(scratch_dev, scratch_bytes, lay.bytes, "scratch smaller than wd_lane_gc_scratch",
                                 "lane gc: the scratch must be in device memory"))
        return rc;
    memset(lane_row, 0, WD_LANEGC_LANE_COLS * sizeof(int64_t));
    memset(tile_rows, 0, (size_t)T * WD_LANEGC_TILE_COLS * sizeof(int64_t));
    memset(hist, 0, (size_t)(L + 1) * kLgcCols * sizeof(int64_t));
    if (!p.start())
        return p.rc;
    uint8_t *sc = (uint8_t *)scratch_dev;
    unsigned long long *cnt_t = (unsigned long long *)(sc + lay.cnt_t);
    unsigned long long *d_hist = (unsigned long long *)(sc + lay.hist);
    int *d_tidx = (int *)(sc + lay.tidx);
    WD_HIP(ctx, hipMemsetAsync(sc, 0, lay.bytes, ctx->stream));
    if (const int rc = p.upload(d_tidx))
        return rc;
    hipLaunchKernelGGL(k_lgc_tally, p.grid, dim3(kTdBlock), 0, ctx->stream, d_tidx, N,
                       (const uint32_t *)(ld->ws + ld->lay.label), (const uint32_t *)(ld->ws + ld->lay.members),
                       (const uint32_t *)(ld->ws + ld->lay.rows), ld->lay.words, L, max_n, cnt_t, d_hist);
    WD_HIP(ctx, hipGetLastError());
    SpreadFetch f_t(cnt_t, (size_t)T, kLgcTileCnt), f_h(d_hist, (size_t)(L + 1), kLgcCols);
    if (const int rc = spread_fetch(ctx, {&f_t, &f_h}))
        return rc;
    unsigned long long c[kLgcTileCnt];
    for (int t = 0; t < T; t++) {
        f_t.sum((size_t)t, c);
        for (int f = 0; f < WD_LANEGC_LANE_COLS; f++)
            lane_row[f] += (int64_t)c[f];
        int64_t *row = tile_rows + (size_t)t * WD_LANEGC_TILE_COLS;
        row[0] = (int64_t)c[0];
        row[1] = (int64_t)(c[0] - c[kLgcSkip] - c[kLgcSkip + 1] - c[kLgcSkip + 2]);
        row[2] = (int64_t)c[kLgcGc];
        row[3] = (int64_t)(c[3] - c[kLgcSkip + 2]);
        row[4] = (int64_t)c[kLgcCopiesGc];
    }
    for (int g = 0; g <= L; g++) {
        f_h.sum((size_t)g, c);
        for (int f = 0; f < kLgcCols; f++)
            hist[(size_t)g * kLgcCols + f] = (int64_t)c[f];
    }
    return WD_OK;
} WD_CATCH

}  // extern "C"
#endif
