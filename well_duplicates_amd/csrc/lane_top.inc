// lane_top.inc - a lane's most frequent reads and their spread (include/welldup_lanetop.h): the duplication levels of
// the whole lane, and the n_top largest groups with their wells per tile, their wells of exactly the root's read, and
// the read.  Included at the end of lane_saturation.inc, after everything of it: it uses read_classes.inc (the spread
// counters), lane_dups.inc (the accumulator, its label, members and rows) and lane_pass.inc as lane_mismatch.inc does.
//
// wd_lane_top, over the tiles that were added (grid y = tile): k_lt_hist once or a few times, k_lt_collect, a sort on
// the host, k_lt_spread and k_lt_rows.  They read label, members and the rows and write the caller's scratch only
// (who writes label is listed at the head of lane_mismatch.inc; members and the rows are written by k_ld_pack,
// k_ld_resolve and the near finish, all before a finish returns).
//
// The selection.  The order of welldup_lanetop.h is the descending order of the 64-bit key
//     key(root) = size << 32 | ~root        (size >= 2; keys are distinct since roots are)
// and the list is the n_top largest keys.  k_lt_hist counts, per pass, the roots whose key lies in a range in nb <=
// kLtBins bins, and the roots above the range.  The host walks the bins from the top to the bin b* that holds the
// n_top-th key; the roots above it (fewer than n_top) are in the list for certain, those below it are not.  If the
// roots at or above b* fit the candidate buffer the selection ends: k_lt_collect gathers exactly them and the host
// sorts.  Otherwise the next pass takes b* as its range.  Why that is exact: the count of a bin is a sum of ones over
// roots, every well is visited by exactly one lane, so "the n_top-th key lies in b*" is a fact, not an estimate; the
// candidates are a superset of the list with every key above the threshold present, so sorting them gives the list.
// The passes: the first bins the SIZE on a log-linear scale - a bin per size below 8, two per power of two above:
// 8, 12, 16, 24, 32, 48, ... - and fills the 16 levels besides.  Its widest bin is 2^30 sizes, 2^62 keys.  Every
// later pass cuts its range into 2^11 bins, so after the linear passes with shifts 51, 40, 29, 18, 7 and 0 a bin is
// one key and holds at most one root: above + 1 <= n_top <= capacity, the selection has ended.  That is
// 1 + ceil(62 / 11) = 7 passes whatever the data; kLaneTopMaxPasses = 8 is stated and the host asserts it.  When the
// size is pinned to one value the same passes refine on ~root among the roots of that size: the smallest ids win.
// If the first pass finds no more groups than the buffer holds, no refinement runs at all.
#include "welldup_lanetop.h"

namespace {

constexpr int kLtBins = 2048;                      // bins of a linear pass
constexpr int kLtBinBits = 11;
constexpr int kLtLevels = WD_LANETOP_LEVELS;
constexpr int kLtHead = WD_LANETOP_HEAD_COLS;
constexpr int kLtAbove = kLtBins;                  // per copy: the bins, the roots above the range, a spare word,
constexpr int kLtLev = kLtBins + 2;                // Groups[16], Wells[16]
constexpr int kLtRow = kLtLev + 2 * kLtLevels;
constexpr int kLtSlots = 2 * WD_LANETOP_MAX;       // the listed roots' table
constexpr int kLtFirstBins = 8 + 2 * 29;           // the first pass: sizes 0 .. 7, then two bins for each of 2^3 .. 2^31
constexpr int kLtFirstWidthBits = 30 + 32;         // its widest bin, in keys
static_assert(1 << kLtBinBits == kLtBins, "a linear pass takes kLtBinBits bits off the range");
static_assert(1 + (kLtFirstWidthBits + kLtBinBits - 1) / kLtBinBits <= kLaneTopMaxPasses, "the bound on the passes");
static_assert(kLaneTopMaxPasses == WD_LANETOP_MAX_PASSES, "the header states the bound");
static_assert(kLtFirstBins <= kLtBins && kLtSlots % kTdBlock == 0, "");
static_assert((kLtSlots & (kLtSlots - 1)) == 0 && kLtSlots >= 2 * WD_LANETOP_MAX, "half of the table stays free");

// the scratch (include/welldup_lanetop.h states the arithmetic)
struct LtLayout {
    size_t hist, cand, count, tab, list, tcnt, exact, rowbuf, tidx, bytes;
    int words;
    int64_t cap;
};

LtLayout lt_layout_of(int max_tiles, int L, int n_top, int64_t cand_capacity)
{
    LtLayout l;
    const size_t t = (size_t)max_tiles, n = (size_t)n_top;
    l.words = (L + kFpCycles - 1) / kFpCycles;
    l.cap = cand_capacity > 0 ? cand_capacity : std::max<int64_t>(WD_LANETOP_DEFAULT_CAPACITY, n_top);
    l.hist = 0;
    l.cand = align256(l.hist + (size_t)kSpread * kLtRow * 8);
    l.count = align256(l.cand + (size_t)l.cap * 8);
    l.tab = align256(l.count + 8);
    l.list = align256(l.tab + (size_t)kLtSlots * 8);
    l.tcnt = align256(l.list + n * 4);
    l.exact = align256(l.tcnt + n * t * 4);
    l.rowbuf = align256(l.exact + n * 4);
    l.tidx = align256(l.rowbuf + n * (size_t)l.words * 4);
    l.bytes = align256(l.tidx + t * sizeof(int));
    return l;
}

// The first pass's bin of a size, and the sizes of a bin [lt_first_lo(b), lt_first_lo(b + 1)).
__host__ __device__ inline uint32_t lt_first_bin(uint32_t s)
{
    if (s < 8)
        return s;
    const int e = 31 - __builtin_clz(s);
    return 8u + 2u * (uint32_t)(e - 3) + ((s >> (e - 1)) & 1u);
}

inline unsigned long long lt_first_lo(int b)        // (b = kLtFirstBins: 2^32, one past the largest size)
{
    if (b < 8)
        return (unsigned long long)b;
    const int e = 3 + (b - 8) / 2;
    return (2ull + (unsigned long long)((b - 8) & 1)) << (e - 1);
}

// The level of a size >= 1: edges 1 .. 10, 50, 100, 500, 1000, 5000, 10000.
__host__ __device__ inline uint32_t lt_level(uint32_t s)
{
    if (s < 10)
        return s - 1;
    return 9u + (s >= 50) + (s >= 100) + (s >= 500) + (s >= 1000) + (s >= 5000) + (s >= 10000);
}

__device__ inline unsigned long long lt_key(uint32_t size, uint32_t root)
{
    return ((unsigned long long)size << 32) | (uint32_t)~root;
}

// ---- the histograms -------------------------------------------------------------------------------
// LaneRun's grid and walk (lane_pass.inc).  A lane loads label, and - of a well that is its own label, a root or a PF
// well in no group - members: 8 bytes a well, both coalesced.
//   first pass (first != 0): wells in no group are counted by ballot into level 0; a root adds one to the bin of its
//     size, one to Groups and its size to Wells of its level.
//   later passes: a root of key >= lo adds one to bin (key - lo) >> shift, or to `above` when that is >= nb.
// The adds go to the workgroup's LDS words (32-bit: a run adds at most kLaneRun ones to a word, and sizes that are
// summed anywhere sum to at most the lane's wells, < 2^32); the lanes of a wave that carry the same size (first
// pass) or name the same word (later) as the wave's first root add once - a lane of pairs has every root in one bin,
// and 32 LDS atomics on one word per trip would queue.  At the end the workgroup adds what is not zero to its copy of
// the spread counters: no global atomic per well.
// Exact whatever the order of execution: every output is a sum over wells, each well is visited by exactly one lane
// of one workgroup, integer adds commute, and label and members were written before this launch began.
__global__ void __launch_bounds__(kTdBlock) k_lt_hist(const int *__restrict__ tile_idx, int64_t N,
                                                       const uint32_t *__restrict__ label,
                                                       const uint32_t *__restrict__ members, int first,
                                                       unsigned long long lo, int shift, uint32_t nb,
                                                       unsigned long long *hist)
{
    __shared__ uint32_t s_cnt[kLtRow];
    for (int i = threadIdx.x; i < kLtRow; i += kTdBlock)
        s_cnt[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t n_single = 0;                                             // the same in every lane of a wave
    LaneRun(tile_idx, N).walk([&](bool has, int64_t, size_t g64) {
        bool single = false, root = false;
        uint32_t size = 0, word = 0;
        if (has && label[g64] == (uint32_t)g64) {
            size = members[g64] + 1u;
            single = size == 1u;
            if (!single) {
                if (first) {
                    root = true;
                    word = lt_first_bin(size);
                } else {
                    const unsigned long long key = lt_key(size, (uint32_t)g64);
                    if (key >= lo) {
                        const unsigned long long b = (key - lo) >> shift;
                        root = true;
                        word = b < nb ? (uint32_t)b : (uint32_t)kLtAbove;
                    }
                }
            }
        }
        if (first)
            n_single += (uint32_t)__popcll(__ballot(single));
        const unsigned long long act = __ballot(root);
        if (act) {                                                     // (the same for the wave)
            const int leader = __ffsll((long long)act) - 1;
            const uint32_t mine = first ? size : word;
            const uint32_t theirs = (uint32_t)__shfl((int)mine, leader);      // (every lane of the wave takes part)
            const bool same = root && mine == theirs;
            const uint32_t n = (uint32_t)__popcll(__ballot(same));
            if (root && (!same || lane == leader)) {
                const uint32_t add = same ? n : 1u;
                atomicAdd(&s_cnt[word], add);
                if (first) {
                    const uint32_t lev = lt_level(size);
                    atomicAdd(&s_cnt[kLtLev + lev], add);
                    atomicAdd(&s_cnt[kLtLev + kLtLevels + lev], add * size);
                }
            }
        }
    });
    if (first && lane == 0 && n_single) {
        atomicAdd(&s_cnt[kLtLev], n_single);
        atomicAdd(&s_cnt[kLtLev + kLtLevels], n_single);
    }
    __syncthreads();
    unsigned long long *out = spread_row(hist, 0, kLtRow);
    for (int i = threadIdx.x; i < kLtRow; i += kTdBlock)
        if (s_cnt[i])
            atomicAdd(out + i, (unsigned long long)s_cnt[i]);
}

// ---- compaction -----------------------------------------------------------------------------------
// The same grid.  A root of key >= thr is appended {root, size} to cand: the wave's roots take consecutive places
// behind one atomic add of the wave's first lane (ballot, the lanes below counted by mbcnt).  A place past the
// capacity is not written; the count says so and the host refuses.  The order of the candidates depends on the
// order of execution; the host sorts them.
__global__ void __launch_bounds__(kTdBlock) k_lt_collect(const int *__restrict__ tile_idx, int64_t N,
                                                          const uint32_t *__restrict__ label,
                                                          const uint32_t *__restrict__ members, unsigned long long thr,
                                                          uint2 *__restrict__ cand, uint32_t capacity, uint32_t *count)
{
    const int lane = threadIdx.x & (kWave - 1);
    LaneRun(tile_idx, N).walk([&](bool has, int64_t, size_t g64) {
        bool take = false;
        uint32_t size = 0;
        if (has && label[g64] == (uint32_t)g64) {
            size = members[g64] + 1u;
            take = size >= 2u && lt_key(size, (uint32_t)g64) >= thr;
        }
        const unsigned long long m = __ballot(take);
        if (!m)                                                        // (the same for the wave)
            return;
        const int leader = __ffsll((long long)m) - 1;
        uint32_t at = 0;
        if (lane == leader)
            at = atomicAdd(count, (uint32_t)__popcll(m));
        at = (uint32_t)__shfl((int)at, leader);
        const uint32_t pos = at + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (take && pos >= at && pos < capacity)                       // (pos >= at: the count has not wrapped)
            cand[pos] = make_uint2((uint32_t)g64, size);
    });
}

// ---- spread and exactness -------------------------------------------------------------------------
// The same grid.  tab: the n listed roots in an open-addressing table of kLtSlots slots {root, rank}, free slots
// {kInvalid, 0}, filled by the host (slot of a root: lt_slot, then the next free one) and copied into LDS by every
// workgroup - 16 KB out of L2 against the 64 KB of labels of its run.  Every PF well looks its label up there; at most
// half of the slots are taken, so a miss ends after a step or two.  (welldup_lanetop.h's members[label] >= the
// smallest listed size would tell the same with a random global read per redundant well; the LDS probe is exact by
// itself and cheaper, so members is not read here.)  A well whose label is listed counts itself in the workgroup's
// row s_cnt [n] - a workgroup lies in one tile, so the row is part of the tile's column - and, when its packed row
// equals the root's (all `words` words; the root's own trivially), in s_eq.  The lanes of a wave that name the same
// rank add once (wave_by_key): a lane of equal reads puts 256 wells a trip on one word.  What is not zero is
// flushed with global atomics: tile_count[rank][tile], exact[rank].
// Exact: sums of ones over wells as in k_lt_hist; the rows were written before the finish and nobody writes them.
__device__ inline uint32_t lt_slot(uint32_t root) { return (root * 0x9E3779B1u) >> (32 - kLtBinBits); }
static_assert(1 << kLtBinBits == kLtSlots, "lt_slot keeps the top bits of the product");

__global__ void __launch_bounds__(kTdBlock) k_lt_spread(const int *__restrict__ tile_idx, int64_t N, int max_tiles,
                                                         const uint32_t *__restrict__ label,
                                                         const uint32_t *__restrict__ rows, int words,
                                                         const uint2 *__restrict__ tab, int n, uint32_t *tile_count,
                                                         uint32_t *exact)
{
    __shared__ uint2 s_tab[kLtSlots];
    __shared__ uint32_t s_cnt[WD_LANETOP_MAX], s_eq[WD_LANETOP_MAX];
    for (int i = threadIdx.x; i < kLtSlots; i += kTdBlock)
        s_tab[i] = tab[i];
    for (int i = threadIdx.x; i < n; i += kTdBlock) {
        s_cnt[i] = 0;
        s_eq[i] = 0;
    }
    __syncthreads();
    const LaneRun run(tile_idx, N);
    const int ti = run.ti;
    run.walk([&](bool has, int64_t, size_t g64) {
        bool listed = false, equal = false;
        uint32_t rank = 0;
        if (has) {
            const uint32_t lab = label[g64];
            if (lab != kInvalid) {
                uint32_t h = lt_slot(lab);
                uint2 e = s_tab[h];
                while (e.x != lab && e.x != kInvalid) {                // (a free slot comes: half of them are)
                    h = (h + 1u) & (uint32_t)(kLtSlots - 1);
                    e = s_tab[h];
                }
                if (e.x == lab) {
                    listed = true;
                    rank = e.y;
                    equal = true;
                    if (lab != (uint32_t)g64) {
                        const uint32_t *x = rows + g64 * (size_t)words, *y = rows + (size_t)lab * (size_t)words;
                        uint32_t diff = 0;
                        for (int k = 0; k < words; k++)
                            diff |= x[k] ^ y[k];
                        equal = diff == 0;
                    }
                }
            }
        }
        wave_by_key(listed, rank, [&](uint32_t r0, unsigned long long group, bool first) {
            const unsigned long long eq = __ballot(listed && rank == r0 && equal);
            if (first) {
                atomicAdd(&s_cnt[r0], (uint32_t)__popcll(group));
                if (eq)
                    atomicAdd(&s_eq[r0], (uint32_t)__popcll(eq));
            }
        });
    });
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kTdBlock) {
        if (s_cnt[i])
            atomicAdd(tile_count + (size_t)i * max_tiles + ti, s_cnt[i]);
        if (s_eq[i])
            atomicAdd(exact + i, s_eq[i]);
    }
}

// the packed rows of the n listed roots, side by side: a lane a word
__global__ void __launch_bounds__(kTdBlock) k_lt_rows(const uint32_t *__restrict__ list, int n, int words,
                                                       const uint32_t *__restrict__ rows, uint32_t *__restrict__ out)
{
    const int i = (int)(blockIdx.x * kTdBlock + threadIdx.x);
    if (i < n * words)
        out[i] = rows[(size_t)list[i / words] * (size_t)words + (size_t)(i % words)];
}

}  // namespace

#ifndef WD_LANE_TOP_EMU                            // (tools/lane_top_emu.cpp: the kernels above on the CPU, a fiber per lane)
namespace {

struct LtCand {
    uint32_t root, size;
};

// one histogram pass; h: the summed row
int lt_hist_pass(wd_ctx *ctx, const dim3 &grid, const int *d_tidx, int64_t N, const uint32_t *label,
                 const uint32_t *members, bool first, unsigned long long lo, int shift, uint32_t nb,
                 unsigned long long *d_hist, SpreadFetch &copies, unsigned long long *h)
{
    WD_HIP(ctx, hipMemsetAsync(d_hist, 0, (size_t)kSpread * kLtRow * 8, ctx->stream));
    hipLaunchKernelGGL(k_lt_hist, grid, dim3(kTdBlock), 0, ctx->stream, d_tidx, N, label, members, first ? 1 : 0, lo, shift,
                       nb, d_hist);
    WD_HIP(ctx, hipGetLastError());
    if (const int rc = spread_fetch(ctx, {&copies}))
        return rc;
    copies.sum(0, h);
    return WD_OK;
}

}  // namespace

extern "C" {

int wd_lane_top_scratch(int64_t N, int max_tiles, int L, int n_top, int64_t cand_capacity, size_t *bytes)
{
    if (N < 0 || max_tiles < 0 || L < 0 || !bytes || n_top < 1 || n_top > WD_LANETOP_MAX || cand_capacity < 0 ||
        (cand_capacity > 0 && cand_capacity < n_top))
        return WD_ERR_ARG;
    if (max_tiles > 65535 || L > kMaxCycles)
        return WD_ERR_UNSUPPORTED;
    *bytes = lt_layout_of(max_tiles, L, n_top, cand_capacity).bytes;
    return WD_OK;
}

int wd_lane_top(wd_lane_dups *ld, int n_top, int64_t cand_capacity, void *scratch_dev, size_t scratch_bytes,
                int64_t *head_row, int64_t *levels, uint32_t *root, uint32_t *size, uint32_t *exact,
                uint32_t *tile_count, char *reads)
try {
    if (!ld || !head_row || !levels || !root || !size || !exact || !tile_count || !reads)
        return WD_ERR_ARG;
    wd_ctx *ctx = ld->ctx;
    const int64_t N = ld->N;
    const int T = ld->max_tiles, L = ld->L;
    LanePass p(ld);
    if (const int rc = p.finished("lane top comes after a successful finish of the lane"))
        return rc;
    if (n_top < 1 || n_top > WD_LANETOP_MAX)
        return fail(ctx, WD_ERR_ARG, "lane top: 1.." + std::to_string(WD_LANETOP_MAX) + " groups, not " + std::to_string(n_top));
    if (cand_capacity < 0 || (cand_capacity > 0 && cand_capacity < n_top))
        return fail(ctx, WD_ERR_ARG, "lane top: the candidate capacity is 0 or at least n_top, not " +
                                         std::to_string(cand_capacity));
    const LtLayout lay = lt_layout_of(T, L, n_top, cand_capacity);
    if (lay.cap > 0xFFFFFFFFll)
        return fail(ctx, WD_ERR_ARG, "lane top: the candidate capacity is below 2^32");
    if (const int rc = p.scratch(scratch_dev, scratch_bytes, lay.bytes, "scratch smaller than wd_lane_top_scratch",
                                 "lane top: the scratch must be in device memory"))
        return rc;
    const size_t n = (size_t)n_top;
    memset(head_row, 0, kLtHead * sizeof(int64_t));
    memset(levels, 0, 2 * kLtLevels * sizeof(int64_t));
    memset(root, 0, n * 4);
    memset(size, 0, n * 4);
    memset(exact, 0, n * 4);
    memset(tile_count, 0, n * (size_t)T * 4);
    memset(reads, 0, n * (size_t)L);
    ctx->lane_top_passes = 0;
    if (!p.start())
        return p.rc;
    uint8_t *sc = (uint8_t *)scratch_dev;
    unsigned long long *d_hist = (unsigned long long *)(sc + lay.hist);
    uint2 *d_cand = (uint2 *)(sc + lay.cand);
    uint32_t *d_count = (uint32_t *)(sc + lay.count);
    uint2 *d_tab = (uint2 *)(sc + lay.tab);
    uint32_t *d_list = (uint32_t *)(sc + lay.list);
    uint32_t *d_tcnt = (uint32_t *)(sc + lay.tcnt);
    uint32_t *d_exact = (uint32_t *)(sc + lay.exact);
    uint32_t *d_rowbuf = (uint32_t *)(sc + lay.rowbuf);
    int *d_tidx = (int *)(sc + lay.tidx);
    const uint32_t *label = (const uint32_t *)(ld->ws + ld->lay.label);
    const uint32_t *members = (const uint32_t *)(ld->ws + ld->lay.members);
    const uint32_t *rows = (const uint32_t *)(ld->ws + ld->lay.rows);
    const int words = lay.words;
    if (const int rc = p.upload(d_tidx))
        return rc;
    const dim3 &grid = p.grid;

    // the first pass: the levels, and the sizes on the log-linear scale
    SpreadFetch copies(d_hist, 1, kLtRow);
    unsigned long long h[kLtRow];
    if (const int rc = lt_hist_pass(ctx, grid, d_tidx, N, label, members, true, 0, 0, kLtFirstBins, d_hist, copies, h))
        return rc;
    int passes = 1;
    ctx->lane_top_passes = passes;
    unsigned long long groups2 = 0;
    for (int i = 0; i < kLtLevels; i++) {
        levels[i] = (int64_t)h[kLtLev + i];
        levels[kLtLevels + i] = (int64_t)h[kLtLev + kLtLevels + i];
        head_row[0] += levels[kLtLevels + i];
        if (i > 0)
            groups2 += h[kLtLev + i];
    }
    head_row[1] = (int64_t)groups2;
    if (groups2 == 0)
        return WD_OK;

    // the threshold: the smallest key a candidate has, and how many candidates that makes
    unsigned long long thr = lt_first_lo(2) << 32, promised = groups2;
    if (groups2 > (unsigned long long)lay.cap) {                      // (then groups2 > n_top: an n_top-th group exists)
        unsigned long long above = 0, lo = 0, width = 0;               // `above`: roots of keys >= lo + width
        int shift = 0;
        uint32_t nb = kLtFirstBins;
        bool first = true;
        for (;;) {
            unsigned long long cum = above;
            int b = (int)nb - 1;
            for (; b >= 0; b--) {                                      // the bin of the n_top-th key from the top
                if (cum + h[b] >= (unsigned long long)n_top)
                    break;
                cum += h[b];
            }
            if (b < 0 || (!first && h[kLtAbove] != above))
                return fail(ctx, WD_ERR_STATE, "lane top: the histograms of two passes disagree");
            const unsigned long long b_lo = first ? lt_first_lo(b) << 32 : lo + ((unsigned long long)b << shift);
            const unsigned long long b_hi = first ? (b + 1 == kLtFirstBins ? 0 : lt_first_lo(b + 1) << 32)       // (0: 2^64)
                                                  : (b + 1 == (int)nb ? lo + width : lo + ((unsigned long long)(b + 1) << shift));
            if (cum + h[b] <= (unsigned long long)lay.cap) {
                thr = b_lo;
                promised = cum + h[b];
                break;
            }
            if (passes >= kLaneTopMaxPasses || b_hi - b_lo <= 1)       // (a bin of one key holds one root: it fitted)
                return fail(ctx, WD_ERR_STATE, "lane top: the selection has not ended in " + std::to_string(passes) + " passes");
            above = cum;
            lo = b_lo;
            width = b_hi - b_lo;                                       // (mod 2^64: right for b_hi = 2^64 too)
            first = false;
            shift = 0;
            while (((width - 1) >> shift) + 1 > (unsigned long long)kLtBins)
                shift++;
            nb = (uint32_t)(((width - 1) >> shift) + 1);
            if (const int rc = lt_hist_pass(ctx, grid, d_tidx, N, label, members, false, lo, shift, nb, d_hist, copies, h))
                return rc;
            ctx->lane_top_passes = ++passes;
        }
    }

    // the candidates, sorted
    WD_HIP(ctx, hipMemsetAsync(d_count, 0, 4, ctx->stream));
    hipLaunchKernelGGL(k_lt_collect, grid, dim3(kTdBlock), 0, ctx->stream, d_tidx, N, label, members, thr, d_cand,
                       (uint32_t)lay.cap, d_count);
    WD_HIP(ctx, hipGetLastError());
    uint32_t n_cand = 0;
    WD_HIP(ctx, hipMemcpyAsync(&n_cand, d_count, 4, hipMemcpyDeviceToHost, ctx->stream));
    WD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (n_cand != promised || n_cand > (unsigned long long)lay.cap)
        return fail(ctx, WD_ERR_STATE, "lane top: " + std::to_string(n_cand) + " candidates where the histograms promised " +
                                           std::to_string(promised));
    std::vector<LtCand> cand(n_cand);
    static_assert(sizeof(LtCand) == sizeof(uint2), "");
    WD_HIP(ctx, hipMemcpyAsync(cand.data(), d_cand, (size_t)n_cand * 8, hipMemcpyDeviceToHost, ctx->stream));
    WD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::sort(cand.begin(), cand.end(),
              [](const LtCand &a, const LtCand &b) { return a.size != b.size ? a.size > b.size : a.root < b.root; });
    const int listed = (int)std::min<size_t>(cand.size(), n);
    head_row[2] = listed;

    // the listed roots: their table, then the spread, the exact wells and the rows
    std::vector<uint2> tab(kLtSlots, make_uint2(kInvalid, 0));
    std::vector<uint32_t> h_list((size_t)listed);
    for (int r = 0; r < listed; r++) {
        h_list[r] = cand[r].root;
        uint32_t s = (cand[r].root * 0x9E3779B1u) >> (32 - kLtBinBits);          // lt_slot
        while (tab[s].x != kInvalid)
            s = (s + 1u) & (uint32_t)(kLtSlots - 1);
        tab[s] = make_uint2(cand[r].root, (uint32_t)r);
    }
    WD_HIP(ctx, hipMemcpyAsync(d_tab, tab.data(), (size_t)kLtSlots * 8, hipMemcpyHostToDevice, ctx->stream));
    WD_HIP(ctx, hipMemcpyAsync(d_list, h_list.data(), (size_t)listed * 4, hipMemcpyHostToDevice, ctx->stream));
    WD_HIP(ctx, hipMemsetAsync(sc + lay.tcnt, 0, lay.rowbuf - lay.tcnt, ctx->stream));
    hipLaunchKernelGGL(k_lt_spread, grid, dim3(kTdBlock), 0, ctx->stream, d_tidx, N, T, label, rows, words, d_tab, listed,
                       d_tcnt, d_exact);
    WD_HIP(ctx, hipGetLastError());
    std::vector<uint32_t> h_rows((size_t)listed * (size_t)words);
    if (words > 0) {
        hipLaunchKernelGGL(k_lt_rows, dim3((unsigned)((listed * words + kTdBlock - 1) / kTdBlock)), dim3(kTdBlock), 0,
                           ctx->stream, d_list, listed, words, rows, d_rowbuf);
        WD_HIP(ctx, hipGetLastError());
        WD_HIP(ctx, hipMemcpyAsync(h_rows.data(), d_rowbuf, h_rows.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (T > 0)
        WD_HIP(ctx, hipMemcpyAsync(tile_count, d_tcnt, (size_t)listed * (size_t)T * 4, hipMemcpyDeviceToHost, ctx->stream));
    WD_HIP(ctx, hipMemcpyAsync(exact, d_exact, (size_t)listed * 4, hipMemcpyDeviceToHost, ctx->stream));
    WD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int r = 0; r < listed; r++) {
        root[r] = cand[r].root;
        size[r] = cand[r].size;
        head_row[3] += cand[r].size;
        for (int c = 0; c < L; c++) {
            const uint32_t code = (h_rows[(size_t)r * words + c / kFpCycles] >> (3 * (c % kFpCycles))) & 7u;
            reads[(size_t)r * L + c] = "ACGTN"[std::min(code, 4u)];
        }
    }
    return WD_OK;
} WD_CATCH

}  // extern "C"

// What comes after this file in the unit is included from here, as lane_saturation.inc includes this file: the best
// well of each of a lane's families (include/welldup_lanekeep.h), which reads the quality part of lane_quality.inc and
// uses nothing of this file.
#include "lane_keep.inc"
#endif
