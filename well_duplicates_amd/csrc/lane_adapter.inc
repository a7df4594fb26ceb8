// lane_adapter.inc - a lane's duplication by insert length (include/welldup_laneadapter.h): every PF well of a lane
// counted by the position at which its own read runs into the adapter - with mismatches, and with partial overlaps at
// the read's end - and by what it is in its group: a lone read, the first well of a group, or a copy.  Included in
// welldup_tiledups.hip after lane_gc.inc: it uses read_classes.inc (the spread counters), lane_dups.inc (the
// accumulator, its label, members and packed rows), lane_mismatch.inc's kLmLow, lane_gc.inc's lgc_piece and
// lane_pass.inc as lane_gc.inc does.
//
// wd_lane_adapter, over the tiles that were added (grid y = tile): one kernel, k_lad_tally, and nothing else.  It
// reads label, members and the rows and writes the caller's scratch only.  Who writes label, members and the rows,
// and that nobody does after a successful finish, is listed at the heads of lane_mismatch.inc and lane_gc.inc; this
// pass joins those lists as a reader.
//
// Like lane_gc.inc it reads every row of the lane (30.9 GB at 112 tiles x 151 cycles), but a popcount per word does
// not answer its question: it looks at every position of every read for a pattern with mismatches - L x m compares a
// read done code by code.  k_lad_tally does them 64 positions at a time: see lad_search.
#include "welldup_laneadapter.h"

namespace {

constexpr int kLadCols = WD_LANEADAPTER_HIST_COLS; // Single, Roots, Copies, FamilyWells
constexpr int kLadWindow = 256;                    // values of a a workgroup counts in LDS
constexpr int kLadTileCnt = 11;                    // per tile and copy: the lane row's ten columns, SumA
constexpr int kLadSumA = 10;
constexpr int kLadStage = kTdBlock * 17;           // words of the staging block: a trip's rows of up to 16 words
constexpr int kLadPosWords = (kMaxCycles + 63) / 64;      // 64-bit words of positions a read can have
constexpr int kLadParAmask = 0, kLadParCodes = 4, kLadParGe = 8;      // the search's table, in uint64
constexpr int kLadParWords = kLadParGe + 4 * kLadPosWords;
static_assert(WD_LANEADAPTER_LANE_COLS == 10 && WD_LANEADAPTER_TILE_COLS == 5, "the rows of welldup_laneadapter.h");
static_assert(WD_LANEADAPTER_MAX_LEN <= 32 && WD_LANEADAPTER_MAX_E <= 3,
              "a match spans two 64-bit position words at most; the counter tells 0, 1, 2, 3 and more");
static_assert(kLadParWords * 8 <= 1024, "the table's part of the scratch");
static_assert(kLadStage * 4 + kLadWindow * kLadCols * 4 + kLadTileCnt * 4 <= 24576,
              "the staging block, the histogram and the counters: 24 KB of LDS, six workgroups a CU");
static_assert(kLadStage >= 2 * ((kMaxCycles + 9) / 10 | 1), "a sub-trip holds a row of the longest read");
static_assert(kLaneRun / kTdBlock < 256, "a lane's counts of a run fit a byte each");

// the scratch (include/welldup_laneadapter.h states the arithmetic)
struct LadLayout {
    size_t cnt_t, hist, tidx, par, bytes;
};

LadLayout lad_layout_of(int max_tiles, int L)
{
    LadLayout l;
    const size_t t = (size_t)max_tiles;
    l.cnt_t = 0;
    l.hist = align256(l.cnt_t + t * kSpread * kLadTileCnt * 8);
    l.tidx = align256(l.hist + (size_t)(L + 1) * kSpread * kLadCols * 8);
    l.par = align256(l.tidx + t * sizeof(int));
    l.bytes = align256(l.par + 1024);
    return l;
}

// ---- the host's half of the search ----------------------------------------------------------------------
// allowed(p) of the header; -1 where p cannot match (L - p < O)
inline int lad_allowed(int L, int m, int E, int O, int p)
{
    const int o = std::min(m, L - p);
    return o < O ? -1 : o == m ? E : E * o / m;
}

// positions 0 .. L - O in 64-bit words
__host__ __device__ inline int lad_pos_words(int L, int O) { return (L - O + 1 + 63) / 64; }

// The table k_lad_tally searches by, kLadParWords uint64: [c] for c = A, C, G, T the adapter positions j that hold c,
// bit j; [4] the adapter's codes, two bits each (the code-by-code form reads them); [8 + 4 q + e] for the positions
// 64 q .. 64 q + 63 and e = 0 .. 3: bit p - 64 q set where allowed(p) >= e and p <= L - O.
inline void lad_table(const uint8_t *adapter, int L, int m, int E, int O, unsigned long long *par)
{
    for (int i = 0; i < kLadParWords; i++)
        par[i] = 0;
    for (int j = 0; j < m; j++) {
        par[kLadParAmask + adapter[j]] |= 1ull << j;
        par[kLadParCodes] |= (unsigned long long)adapter[j] << (2 * j);
    }
    for (int p = 0; p <= L - O; p++)
        for (int e = 0; e <= lad_allowed(L, m, E, O, p); e++)
            par[kLadParGe + 4 * (p / 64) + e] |= 1ull << (p % 64);
}

// ---- the device's -----------------------------------------------------------------------------------------
// a row of the histogram in memory: the workgroup's copy
__device__ inline unsigned long long *lad_hist_row(unsigned long long *hist, uint32_t a)
{
    return spread_row(hist, (size_t)a, kLadCols);
}

// the row stride of the staging block: odd, so that the 64 lanes of a wave reading word k of their own rows ask 64
// different banks (an odd stride is prime to the 64 banks); and the wells of a sub-trip
__host__ __device__ inline int lad_stride(int words) { return words | 1; }
__host__ __device__ inline int lad_sub_wells(int words)
{
    const int fit = kLadStage / lad_stride(words);
    return fit < kTdBlock ? fit : kTdBlock;
}

// The words of a piece stored into their wells' rows of the staging block: word i of the sub-trip's span (i0 .. i0 +
// 3 here, those in 0 .. ns - 1) is word i % words of well i / words.  One division per piece.  ns = the sub-trip's
// wells x words and a sub-trip has at most lad_sub_wells wells, so every store lies below lad_sub_wells x stride.
__device__ inline void lad_store(uint32_t *stage, const uint4 &p, int i0, int ns, int words, int stride)
{
    const int first = max(i0, 0);
    int well = (int)((uint32_t)first / (uint32_t)words), r = first - well * words;
    auto word = [&](int i, uint32_t w) {
        if (i < 0 || i >= ns)
            return;
        stage[well * stride + r] = w;
        if (++r == words) {
            r = 0;
            well++;
        }
    };
    word(i0, p.x);
    word(i0 + 1, p.y);
    word(i0 + 2, p.z);
    word(i0 + 3, p.w);
}

// bits 0, 3, 6 .. 27 of x (and nothing else set) moved to bits 0 .. 9
__device__ inline uint32_t lad_squeeze(uint32_t x)
{
    x = (x | (x >> 2)) & 0x030C30C3u;
    x = (x | (x >> 4)) & 0x0300F00Fu;
    x = (x | (x >> 8)) & 0x030000FFu;
    return (x | (x >> 16)) & 0x3FFu;
}

// bits n .. 63 (n <= 0: all; n >= 64: none)
__device__ inline unsigned long long lad_from(int n) { return n <= 0 ? ~0ull : n >= 64 ? 0ull : ~0ull << n; }

// a(w) of the read in `row` (words of ten codes: cycle 10 k + j at bits 3 j .. 3 j + 2 of word k, the unused codes of
// the last word zero - k_ld_pack's layout, lane_dups.inc), and of its first match mism in bits 16, 17: a | mism << 16,
// a = L without a match.
#ifndef WD_LAD_NAIVE
// Bit-parallel over positions.  The read is three bit planes over its cycles - bit p of plane b is bit b of cycle p's
// code -, made from the row a word of ten codes at a time (lad_squeeze) and kept as a window of two 64-bit words: the
// positions 64 q .. 64 q + 63 under way and the 64 after, which a match of up to 32 bases that begins among the first
// reaches into.  `filled` bits of the window are made; it, the row word k and everything else that steers the loops
// are the same in every lane, so the control flow is scalar.  A cycle p mismatches base c where its code is not c:
// (plane 0 ^ c's bit 0) | (plane 1 ^ c's bit 1) | plane 2 - an N, code 4, mismatches every base - and nowhere at or
// beyond L: a position past the read's end matches anything, which makes a partial overlap a full-length one with
// nothing to count past the end.  For every adapter position j that holds c (the table's bit sets, c by c: integer
// adds commute, the order of j is free) the mismatch vector shifted down by j - its low 64 bits, the shift carrying
// from the window's second word - is added to a bit-sliced counter per position: two planes and a sticky overflow
// plane, 0, 1, 2, 3 and more.  The positions that match are those whose count is e where allowed(p) >= e (the
// table's ge words; they are clear beyond L - O), the first set bit of the first such word is a(w), and its count is
// read from the two planes at that bit.
__device__ inline uint32_t lad_search(const uint32_t *row, int words, int L, int m, int E, int O,
                                      const unsigned long long *__restrict__ par)
{
    (void)m, (void)E;
    unsigned long long p0l = 0, p0h = 0, p1l = 0, p1h = 0, p2l = 0, p2h = 0;
    int k = 0, filled = 0;
    uint32_t found = (uint32_t)L;
    const int nq = lad_pos_words(L, O);
    for (int q = 0; q < nq; q++) {
        while (filled <= 118 && k < words) {       // room for ten more
            const uint32_t w = row[k++];
            const unsigned long long b0 = lad_squeeze(w & kLmLow), b1 = lad_squeeze((w >> 1) & kLmLow),
                                     b2 = lad_squeeze((w >> 2) & kLmLow);
            if (filled < 64) {
                p0l |= b0 << filled;
                p1l |= b1 << filled;
                p2l |= b2 << filled;
                if (filled > 54) {
                    p0h |= b0 >> (64 - filled);
                    p1h |= b1 >> (64 - filled);
                    p2h |= b2 >> (64 - filled);
                }
            } else {
                p0h |= b0 << (filled - 64);
                p1h |= b1 << (filled - 64);
                p2h |= b2 << (filled - 64);
            }
            filled += 10;
        }
        const unsigned long long in_l = ~lad_from(L - 64 * q), in_h = ~lad_from(L - 64 * q - 64);
        unsigned long long c0 = 0, c1 = 0, ov = 0;
#pragma unroll 1
        for (int c = 0; c < 4; c++) {
            const unsigned long long f0 = 0ull - (unsigned long long)(c & 1), f1 = 0ull - (unsigned long long)(c >> 1);
            const unsigned long long ml = ((p0l ^ f0) | (p1l ^ f1) | p2l) & in_l, mh = ((p0h ^ f0) | (p1h ^ f1) | p2h) & in_h;
            for (uint32_t js = ((const uint32_t *)par)[2 * (kLadParAmask + c)]; js; js &= js - 1) {
                const int j = __ffs((int)js) - 1;
#ifdef WD_LAD_DROP_CARRY                           // (tools/lane_adapter_emu.cpp: the bug it must notice)
                const unsigned long long v = ml >> j;
#else
                const unsigned long long v = (ml >> j) | (mh << (63 - j) << 1);
#endif
                const unsigned long long k0 = c0 & v;
                c0 ^= v;
                const unsigned long long k1 = c1 & k0;
                c1 ^= k0;
                ov |= k1;
            }
        }
        const unsigned long long *ge = par + kLadParGe + 4 * q;
        const unsigned long long match = ~ov & ((~c0 & ~c1 & ge[0]) | (c0 & ~c1 & ge[1]) | (~c0 & c1 & ge[2]) | (c0 & c1 & ge[3]));
        if (found == (uint32_t)L && match) {
            const int b = __ffsll((long long)match) - 1;
            found = (uint32_t)(64 * q + b) | (uint32_t)((c0 >> b) & 1) << 16 | (uint32_t)((c1 >> b) & 1) << 17;
        }
        p0l = p0h, p1l = p1h, p2l = p2h;
        p0h = p1h = p2h = 0;
        filled = max(filled - 64, 0);
    }
    return found;
}
#else
// Position after position, code by code, on the same staged row (measurements, and the emulator's second form).
__device__ inline uint32_t lad_search(const uint32_t *row, int words, int L, int m, int E, int O,
                                      const unsigned long long *__restrict__ par)
{
    (void)words;
    const unsigned long long codes = par[kLadParCodes];
    for (int p = 0; p <= L - O; p++) {
        const int o = min(m, L - p), allowed = o == m ? E : E * o / m;
        int mism = 0;
        for (int j = 0; j < o && mism <= allowed; j++) {
            const int c = p + j;
            mism += ((row[c / 10] >> (3 * (c % 10))) & 7u) != (uint32_t)((codes >> (2 * j)) & 3);
        }
        if (mism <= allowed)
            return (uint32_t)p | (uint32_t)mism << 16;
    }
    return (uint32_t)L;
}
#endif

// ---- tally --------------------------------------------------------------------------------------
// LaneRun's grid and walk (lane_pass.inc).  A trip of the walk is 256 consecutive wells of a tile; three steps.
//   - Stage.  The rows of a trip are one contiguous span, loaded as k_lgc_tally loads it: 16-byte pieces cut by the
//     address, neighbouring lanes neighbouring pieces, two per lane in flight, the words of the first and last piece
//     inside the span one by one (lgc_piece) - nothing outside the span is read.  The pieces go into the staging block
//     in LDS, row by row at a stride of lad_stride(words) words (lad_store).  A trip of rows of up to 16 words fits
//     the block whole; longer rows (L up to 1024, 103 words) are walked in sub-trips of lad_sub_wells wells - 42 at
//     103 words -, each between two barriers: one before the block is written again, one before it is read.  How many
//     sub-trips a trip has depends on the run alone, so every lane meets every barrier.
//   - Search.  After the barrier a lane whose well is in the sub-trip and PF reads its own row from LDS (word k of 64
//     rows: 64 banks) and finds a(w): lad_search.  No collective is inside, so lanes may stay out.
//   - Tally.  Once per trip, in every lane, as k_lgc_tally: a counted well's key is 4 a + its population; the wells of
//     a wave are grouped by key (wave_by_key) and the first lane of a group adds the group's size to the workgroup's
//     hist [kLadWindow][4] in LDS; a root adds members + 1 to FamilyWells of its a by itself; a >= kLadWindow goes to
//     the workgroup's copy in memory at once, so the result is exact for every L the accumulator takes.  The counts
//     of the lane row are summed per lane over the run - eight of them a byte each in two registers, a lane having 32
//     wells a run -, AdFamilyWells and SumA in a register each, and added up over the wave by shuffles at the end.
// At the end the workgroup adds what is not zero to its copy of the spread counters (spread_row).
// Bounds: a 32-bit LDS word takes at most kLaneRun ones per run, at most kLaneRun x 1023 < 2^23 of SumA, and family
// sizes summed anywhere are sizes of distinct groups, which sum to at most the lane's wells < 2^32; the memory counters
// are 64-bit.  Why the result is exact and does not depend on the order of execution: every output is a sum over
// wells of a value that depends on that well's row, label and members and on the call's arguments alone; each well is
// visited by exactly one lane of one workgroup, each word of its row is stored into the staging block by exactly one
// lane of that workgroup in that sub-trip and read by the well's lane between the two barriers that keep the block
// still; integer adds commute and none can overflow; what a lane reads from memory was written by launches that
// ended before this one began, and nothing writes it after a successful finish.
__global__ void __launch_bounds__(kTdBlock) k_lad_tally(const int *__restrict__ tile_idx, int64_t N,
                                                         const uint32_t *__restrict__ label,
                                                         const uint32_t *__restrict__ members,
                                                         const uint32_t *__restrict__ rows, int words, int L, int m, int E,
                                                         int O, const unsigned long long *__restrict__ par,
                                                         unsigned long long *cnt_t, unsigned long long *hist)
{
    __shared__ uint32_t s_hist[kLadWindow * kLadCols];
    __shared__ uint32_t s_cnt[kLadTileCnt];
#ifdef WD_LANE_ADAPTER_EMU                         // (the emulator's staging block: a heap block of exactly its size)
    uint32_t *const s_stage = lad_emu_stage;
#else
    __shared__ uint32_t s_stage[kLadStage];
#endif
    const int n_hist = min(L + 1, kLadWindow) * kLadCols;
    for (int e = threadIdx.x; e < n_hist; e += kTdBlock)
        s_hist[e] = 0;
    if (threadIdx.x < kLadTileCnt)
        s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const LaneRun run(tile_idx, N);
    const int ti = run.ti, lane = threadIdx.x & (kWave - 1);
    const int stride = lad_stride(words), sub_wells = lad_sub_wells(words);
    // this lane's: the wells of populations 0, 1, 2 and the inexact ones, a byte each (a lane has kLaneRun / kTdBlock =
    // 32 wells a run); those of them with adapter and the partial ones; AdFamilyWells; SumA
    uint32_t n_all = 0, n_ad = 0, ad_fam = 0, sum_a = 0;
    run.walk([&](bool has, int64_t w, size_t g64) {
        uint32_t lab = kInvalid, mem = 0;
        if (has) {
            lab = label[g64];
            if (lab == (uint32_t)g64)
                mem = members[g64];
        }
        const bool pf = lab != kInvalid;
        const int64_t w0 = w - threadIdx.x;
        const int n_trip = (int)(min(w0 + kTdBlock, run.run1) - w0);
        uint32_t res = (uint32_t)L;
        for (int sub0 = 0; sub0 < n_trip; sub0 += sub_wells) {
            const int n_sub = min(sub_wells, n_trip - sub0);
            // the sub-trip's span: ns words from rs, which lies `mis` words past a 16-byte boundary; np pieces
            const uint32_t *__restrict__ rs = rows + (run.base + (size_t)(w0 + sub0)) * (size_t)words;
            const int mis = (int)(((uintptr_t)rs >> 2) & 3), ns = n_sub * words, np = (ns + mis + 3) >> 2;
            __syncthreads();                                          // the searches before are done with the block
            for (int q = threadIdx.x; q < np; q += 2 * kTdBlock) {
                const int va = 4 * q - mis, vb = va + 4 * kTdBlock;
                const bool two = q + kTdBlock < np;
                const uint4 pa = lgc_piece(rs, va, 0, ns);
                const uint4 pb = two ? lgc_piece(rs, vb, 0, ns) : make_uint4(0, 0, 0, 0);
                lad_store(s_stage, pa, va, ns, words, stride);
                if (two)
                    lad_store(s_stage, pb, vb, ns, words, stride);
            }
            __syncthreads();
            const int t = (int)threadIdx.x - sub0;
            if (pf && t >= 0 && t < n_sub)
                res = lad_search(s_stage + t * stride, words, L, m, E, O, par);
        }
        const uint32_t a = res & 0xFFFFu, mism = res >> 16;
        const int pop = !pf ? -1 : lab != (uint32_t)g64 ? 2 : mem ? 1 : 0;
        const bool ad = pf && a < (uint32_t)L;
        if (pf) {
            n_all += 1u << (8 * pop);
            if (ad)
                n_all += (uint32_t)(mism != 0) << 24, n_ad += (1u << (8 * pop)) + ((uint32_t)(a + (uint32_t)m > (uint32_t)L) << 24);
        }
        if (ad)
            sum_a += a;
        if (pop == 1) {
            if (ad)
                ad_fam += mem + 1u;
            if (a < (uint32_t)kLadWindow)
                atomicAdd(&s_hist[a * kLadCols + 3], mem + 1u);
            else
                atomicAdd(lad_hist_row(hist, a) + 3, (unsigned long long)(mem + 1u));
        }
        wave_by_key(pf, a * kLadCols + (uint32_t)pop, [&](uint32_t k0, unsigned long long group, bool first) {
            if (first) {
                const uint32_t cnt = (uint32_t)__popcll(group);
                if (k0 < (uint32_t)(kLadWindow * kLadCols))
                    atomicAdd(&s_hist[k0], cnt);
                else
                    atomicAdd(lad_hist_row(hist, k0 / kLadCols) + k0 % kLadCols, (unsigned long long)cnt);
            }
        });
    });
    uint32_t v[kLadTileCnt] = {0, n_all & 255u, (n_all >> 8) & 255u, (n_all >> 16) & 255u, n_ad & 255u, (n_ad >> 8) & 255u,
                               (n_ad >> 16) & 255u, ad_fam, n_all >> 24, n_ad >> 24, sum_a};
    v[0] = v[1] + v[2] + v[3];
#pragma unroll
    for (int f = 0; f < kLadTileCnt; f++) {
        for (int off = kWave / 2; off; off >>= 1)                      // (every lane of the wave takes part)
            v[f] += (uint32_t)__shfl((int)v[f], lane ^ off);
        if (lane == 0 && v[f])
            atomicAdd(&s_cnt[f], v[f]);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n_hist; e += kTdBlock)
        if (s_hist[e])
            atomicAdd(lad_hist_row(hist, (uint32_t)e / kLadCols) + e % kLadCols, (unsigned long long)s_hist[e]);
    if (threadIdx.x < kLadTileCnt && s_cnt[threadIdx.x])
        atomicAdd(spread_row(cnt_t, (size_t)ti, kLadTileCnt) + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

}  // namespace

#ifndef WD_LANE_ADAPTER_EMU                        // (tools/lane_adapter_emu.cpp: the kernel above on the CPU, a fiber per lane)
extern "C" {

int wd_lane_adapter_scratch(int max_tiles, int L, size_t *bytes)
{
    if (max_tiles < 0 || L < 0 || !bytes)
        return WD_ERR_ARG;
    if (L > kMaxCycles || max_tiles > 65535)
        return WD_ERR_UNSUPPORTED;
    *bytes = lad_layout_of(max_tiles, L).bytes;
    return WD_OK;
}

int wd_lane_adapter(wd_lane_dups *ld, const uint8_t *adapter, int m, int max_e, int min_overlap, void *scratch_dev,
                    size_t scratch_bytes, int64_t *lane_row, int64_t *tile_rows, int64_t *hist)
try {
    if (!ld || !adapter || !lane_row || !tile_rows || !hist)
        return WD_ERR_ARG;
    wd_ctx *ctx = ld->ctx;
    const int64_t N = ld->N;
    const int T = ld->max_tiles, L = ld->L;
    LanePass p(ld);
    if (const int rc = p.finished("lane adapter comes after a successful finish of the lane"))
        return rc;
    if (m < WD_LANEADAPTER_MIN_LEN || m > WD_LANEADAPTER_MAX_LEN)
        return fail(ctx, WD_ERR_ARG, "lane adapter: an adapter has " + std::to_string(WD_LANEADAPTER_MIN_LEN) + ".." +
                                         std::to_string(WD_LANEADAPTER_MAX_LEN) + " bases, not " + std::to_string(m));
    if (max_e < 0 || max_e > WD_LANEADAPTER_MAX_E)
        return fail(ctx, WD_ERR_ARG, "lane adapter: max_e is 0.." + std::to_string(WD_LANEADAPTER_MAX_E) + ", not " +
                                         std::to_string(max_e));
    if (min_overlap < WD_LANEADAPTER_MIN_OVERLAP || min_overlap > m || min_overlap > L)
        return fail(ctx, WD_ERR_ARG, "lane adapter: min_overlap is " + std::to_string(WD_LANEADAPTER_MIN_OVERLAP) +
                                         ".." + std::to_string(std::min(m, L)) + ", not " + std::to_string(min_overlap));
    for (int j = 0; j < m; j++)
        if (adapter[j] > 3)
            return fail(ctx, WD_ERR_ARG, "lane adapter: the adapter's codes are 0..3 (A C G T), not " +
                                             std::to_string((int)adapter[j]) + " at " + std::to_string(j));
    const LadLayout lay = lad_layout_of(T, L);
    if (const int rc = p.scratch(scratch_dev, scratch_bytes, lay.bytes, "scratch smaller than wd_lane_adapter_scratch",
                                 "lane adapter: the scratch must be in device memory"))
        return rc;
    memset(lane_row, 0, WD_LANEADAPTER_LANE_COLS * sizeof(int64_t));
    memset(tile_rows, 0, (size_t)T * WD_LANEADAPTER_TILE_COLS * sizeof(int64_t));
    memset(hist, 0, (size_t)(L + 1) * kLadCols * sizeof(int64_t));
    if (!p.start())
        return p.rc;
    uint8_t *sc = (uint8_t *)scratch_dev;
    unsigned long long *cnt_t = (unsigned long long *)(sc + lay.cnt_t);
    unsigned long long *d_hist = (unsigned long long *)(sc + lay.hist);
    int *d_tidx = (int *)(sc + lay.tidx);
    unsigned long long *d_par = (unsigned long long *)(sc + lay.par);
    unsigned long long par[kLadParWords];
    lad_table(adapter, L, m, max_e, min_overlap, par);
    WD_HIP(ctx, hipMemsetAsync(sc, 0, lay.bytes, ctx->stream));
    if (const int rc = p.upload(d_tidx))
        return rc;
    WD_HIP(ctx, hipMemcpyAsync(d_par, par, sizeof(par), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_lad_tally, p.grid, dim3(kTdBlock), 0, ctx->stream, d_tidx, N,
                       (const uint32_t *)(ld->ws + ld->lay.label), (const uint32_t *)(ld->ws + ld->lay.members),
                       (const uint32_t *)(ld->ws + ld->lay.rows), ld->lay.words, L, m, max_e, min_overlap, d_par, cnt_t,
                       d_hist);
    WD_HIP(ctx, hipGetLastError());
    SpreadFetch f_t(cnt_t, (size_t)T, kLadTileCnt), f_h(d_hist, (size_t)(L + 1), kLadCols);
    if (const int rc = spread_fetch(ctx, {&f_t, &f_h}))
        return rc;
    unsigned long long c[kLadTileCnt];
    for (int t = 0; t < T; t++) {
        f_t.sum((size_t)t, c);
        for (int f = 0; f < WD_LANEADAPTER_LANE_COLS; f++)
            lane_row[f] += (int64_t)c[f];
        int64_t *row = tile_rows + (size_t)t * WD_LANEADAPTER_TILE_COLS;
        row[0] = (int64_t)c[0];
        row[1] = (int64_t)(c[4] + c[5] + c[6]);
        row[2] = (int64_t)c[3];
        row[3] = (int64_t)c[6];
        row[4] = (int64_t)c[kLadSumA];
    }
    for (int a = 0; a <= L; a++) {
        f_h.sum((size_t)a, c);
        for (int f = 0; f < kLadCols; f++)
            hist[(size_t)a * kLadCols + f] = (int64_t)c[f];
    }
    return WD_OK;
} WD_CATCH

}  // extern "C"
#endif
