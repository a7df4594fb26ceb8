// lane_keep.inc - the best well of each of a lane's families (include/welldup_lanekeep.h): every PF well gets a score,
// the sum of its reported base qualities at or above min_q as the quality rows bin them, and of every family - a Root
// with its Copies, a class or a cluster - the well with the largest score is kept, the smallest id among equals; the
// others are dropped.  The result is a byte per well for the caller's filter files, with the counts of what moved.
// Included at the end of lane_top.inc, after everything of it, and so after everything of lane_quality.inc, whose
// quality part it reads (welldup_tiledups.hip's last line is pinned to lane_quality.inc, which includes
// lane_saturation.inc, which includes lane_top.inc).  It uses read_classes.inc (the spread counters), lane_dups.inc (the
// accumulator, its label and members), lane_gc.inc (lgc_piece: the 16-byte pieces of a span of packed rows),
// lane_quality.inc (the quality part: its rows, its table, which tiles got qualities) and lane_pass.inc as
// lane_saturation.inc does.
//
// wd_lane_keep, over the tiles that were added (grid y = tile): a memset and two kernels, k_lk_score and k_lk_mark.
// They read label, members and the quality rows and write the caller's scratch and the caller's masks only.  Who
// writes label and members, and that nobody does after a successful finish, is said at the head of lane_mismatch.inc
// and of lane_gc.inc; the quality rows are written by k_lq_pack alone, in wd_lane_qual_add, which refuses after a
// finish.  This pass joins those lists as a reader.
// wd_lane_keep_molecules (include/welldup_lanemolecules.h) is the same host body and the same two kernels with the
// accumulator's molecule part - mol and molmem, written by wd_lane_umi_molecules (lane_umi.inc) in the form of label
// and members - in the places of label and members: "family" then reads "UMI molecule of two or more wells".
#include "welldup_lanekeep.h"

namespace {

constexpr int kLkTileCnt = WD_LANEKEEP_TILE_COLS;          // per tile and copy: PF, Kept, Dropped, MovedIn, SumKept, SumDropped
constexpr int kLkGainBins = WD_LANEKEEP_GAIN_BINS;
constexpr int kLkLaneCnt = WD_LANEKEEP_LANE_COLS - kLkTileCnt;     // per copy: Families, Moved, SumRoots, GainBins
constexpr int kLkFamilies = 0, kLkMoved = 1, kLkSumRoots = 2, kLkGain = 3;
constexpr int kLkScoreBits = 16;
constexpr uint32_t kLkMaxScore = 0xFFFFu;
static_assert(kLkLaneCnt == 3 + kLkGainBins && kLkTileCnt == 6, "the rows of welldup_lanekeep.h");
static_assert(WD_LANEKEEP_MAX_Q * kMaxCycles <= (int)kLkMaxScore, "a score - at most 63 a cycle - fits 16 bits for every L the accumulator takes");
static_assert((unsigned long long)kLaneRun * kLkMaxScore < (1ull << 32), "a 32-bit LDS counter holds a run's scores");
static_assert(kLkTileCnt + kLkLaneCnt <= kTdBlock, "a lane per counter when the workgroup flushes");

// the scratch (include/welldup_lanekeep.h states the arithmetic)
struct LkLayout {
    size_t best, score, cnt_t, cnt_l, tidx, maskp, bytes;
};

LkLayout lk_layout_of(int64_t N, int max_tiles)
{
    LkLayout l;
    const size_t t = (size_t)max_tiles, wells = t * (size_t)N;
    l.best = 0;
    l.score = align256(l.best + 8 * wells);
    l.cnt_t = align256(l.score + 2 * wells);
    l.cnt_l = align256(l.cnt_t + t * kSpread * kLkTileCnt * 8);
    l.tidx = align256(l.cnt_l + (size_t)kSpread * kLkLaneCnt * 8);
    l.maskp = align256(l.tidx + t * sizeof(int));
    l.bytes = align256(l.maskp + t * sizeof(void *));
    return l;
}

// The eight weights as the kernels take them: kernel arguments, not a table in memory.  A weight is a function of a
// code's three bits b0, b1, b2, and every such function with weight(0) = 0 is a sum over the seven non-empty sets S of
// bits of a[S] x (every bit of S is set) - a[S] = the sum over the subsets T of S of (-1)^(|S| - |T|) weight(T), in
// integers, some of them negative.  Summed over the ten codes of a word "every bit of S is set" is a popcount of the
// word's bit planes ANDed together, so a word's score is seven popcounts and seven multiplies, whatever the weights: no
// code is looked up one by one (ten shifts and selects a word, measured at 1.5 x k_lgc_tally's time on the planted
// lane, DESIGN 5.28).  The unused codes of a row's last word are zero - bin 0, which weighs nothing.
struct LkWeights {
    int a[8];                                      // by S as a mask of the bits; a[0] is not used
};

LkWeights lk_weights_of(const int (&weight)[8])
{
    LkWeights k;
    for (int s = 0; s < 8; s++) {
        k.a[s] = 0;
        for (int t = 0; t < 8; t++)
            if ((t & s) == t)
                k.a[s] += (__builtin_popcount((unsigned)(s ^ t)) & 1) ? -weight[t] : weight[t];
    }
    return k;
}

__device__ inline uint32_t lk_word(uint32_t w, const LkWeights &k)
{
    const uint32_t b0 = w & kLmLow, b1 = (w >> 1) & kLmLow, b2 = (w >> 2) & kLmLow;
    return (uint32_t)(k.a[1] * __popc(b0) + k.a[2] * __popc(b1) + k.a[4] * __popc(b2) + k.a[3] * __popc(b0 & b1) +
                      k.a[5] * __popc(b0 & b2) + k.a[6] * __popc(b1 & b2) + k.a[7] * __popc(b0 & b1 & b2));
}

// lgc_add's walk for the scores: word i of the span (i0 .. i0 + 3 here, those in 0 .. ns - 1) belongs to well
// i / words of the trip; the words of one well are added up before they go to LDS.
__device__ inline void lk_add(uint32_t *s_well, const uint4 &p, int i0, int ns, int words, const LkWeights &k)
{
    const int first = max(i0, 0);
    int well = (int)((uint32_t)first / (uint32_t)words), r = first - well * words;
    uint32_t acc = 0;
    auto word = [&](int i, uint32_t w) {
        if (i < 0 || i >= ns)
            return;
        acc += lk_word(w, k);
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

// the key of a well in its family's word: the smallest key is the largest score, the smallest id among equals
__device__ inline unsigned long long lk_key(uint32_t score, uint32_t id)
{
    return (unsigned long long)(kLkMaxScore - score) << 32 | id;
}

// ---- the scores and the families' best ------------------------------------------------------------
// LaneRun's grid and walk (lane_pass.inc).  best: a 64-bit word per well of the lane, all ones when the kernel starts
// (a memset on the same stream); score: 16 bits per well.
//   - Loading the quality rows: k_lgc_tally's way (lane_gc.inc, which records what a lane walking its own row costs,
//     as lane_dups.inc does on the store side).  A trip's 256 rows are one contiguous span of 256 x words words, read
//     as 16-byte pieces cut by the ADDRESS (lgc_piece: nothing outside the span is read), neighbouring lanes
//     neighbouring pieces, two pieces per lane in flight; a lane sums the weights of its pieces' words (lk_word) and
//     adds them to the sums of the wells they belong to, s_well[256] in LDS, double-buffered by the trip's parity so
//     that a trip costs one barrier.
//   - The score of every well of the run is stored, PF or not: k_lk_mark reads its own well's only.
//   - A PF well of a family - a Copy, or a Root with members >= 1 - brings best[label] down to its key (lk_key) by
//     a 64-bit atomicMin.  The candidates of a wave are grouped by label (wave_by_key).  A group of one lane - the
//     usual case - has its key at hand; of a larger group the lanes that hold the largest score are found bit by bit
//     from the top with sixteen ballots, and the lowest of them holds the smallest id, since ids ascend with the lane
//     in a trip.  The group's first lane issues one atomicMin of that key; nobody waits for it.
//   - Two skips, k_ls_min's.  A well is a candidate only where its key is smaller than a plain read of the word.  And a
//     wave remembers the label it served last and the key it left there: a group of the same label with no smaller key
//     is skipped - and a well of that label with no smaller key does not even read the word (on a lane of equal reads
//     every wave of the device would otherwise read one address on every trip).  On a lane of equal reads - one label
//     for every well - a wave then issues an atomic only when its running best improves: with one quality once, at
//     the latest, with random qualities a few times, never once per well.
// Why the read before the atomic is safe: a word of best is written by atomicMin alone after the memset, so it only
// ever falls.  A stale value read before the atomic is therefore >= the word's value at any later time; skipping when
// key >= stale value skips only an atomicMin that could not have lowered the word, and when the test passes the
// atomicMin itself decides.  The same holds for the wave's own last key: its atomicMin has already brought the word
// that low.  Why the result is exact and does not depend on the order of execution: the smallest key of a group
// stands for all of them, minima commute, every well is visited by exactly one lane of one workgroup and each word
// of its row by exactly one lane of that workgroup in that trip, the LDS adds commute and cannot overflow (a well's
// sum is at most 64 512); keys are distinct since ids are, so the word ends as the one smallest key of the family;
// label, members and the quality rows were written by launches that ended before this one began; a root's label is
// a global id of a PF well of an added tile, so it indexes best.
__global__ void __launch_bounds__(kTdBlock) k_lk_score(const int *__restrict__ tile_idx, int64_t N,
                                                        const uint32_t *__restrict__ label,
                                                        const uint32_t *__restrict__ members,
                                                        const uint32_t *__restrict__ qrows, int words, LkWeights wts,
                                                        uint16_t *__restrict__ score, unsigned long long *best)
{
    __shared__ uint32_t s_well[2][kTdBlock];
    s_well[0][threadIdx.x] = 0;
    s_well[1][threadIdx.x] = 0;
    __syncthreads();
    const LaneRun run(tile_idx, N);
    const int mis = (int)(((uintptr_t)qrows >> 2) & 3);               // words the rows' base lies past a 16-byte boundary
    uint32_t last_root = kInvalid;                                    // the same in every lane of a wave
    unsigned long long last_key = 0;
    int buf = 0;
    run.walk([&](bool has, int64_t w, size_t g64) {
        uint32_t lab = kInvalid, mem = 0;
        if (has) {
            lab = label[g64];
            if (lab == (uint32_t)g64)
                mem = members[g64];
        }
        uint32_t *sw = s_well[buf];
        const int64_t w0 = w - threadIdx.x;
        const int64_t s0 = (int64_t)(run.base + (size_t)w0) * words, s1 = s0 + (min(w0 + kTdBlock, run.run1) - w0) * words;
        const int64_t va0 = (s0 + mis) & ~(int64_t)3;                 // (in words from the boundary before the base)
        const int ns = (int)(s1 - s0), np = (int)((s1 + mis - va0 + 3) >> 2);
        for (int q = threadIdx.x; q < np; q += 2 * kTdBlock) {
            const int64_t va = va0 + 4 * (int64_t)q - mis, vb = va + 4 * kTdBlock;
            const bool two = q + kTdBlock < np;
            const uint4 pa = lgc_piece(qrows, va, s0, s1);
            const uint4 pb = two ? lgc_piece(qrows, vb, s0, s1) : make_uint4(0, 0, 0, 0);
            lk_add(sw, pa, (int)(va - s0), ns, words, wts);
            if (two)
                lk_add(sw, pb, (int)(vb - s0), ns, words, wts);
        }
        __syncthreads();
        const uint32_t c = sw[threadIdx.x];
        sw[threadIdx.x] = 0;
        buf ^= 1;
        bool cand = false;
        if (has) {
            score[g64] = (uint16_t)c;
            if (lab != kInvalid && (lab != (uint32_t)g64 || mem)) {
                const unsigned long long key = lk_key(c, (uint32_t)g64);
                if (lab != last_root || key < last_key)                // (else this wave has left the word that low: no read)
                    cand = key < best[lab];
            }
        }
        const uint32_t inv = kLkMaxScore - c;
        wave_by_key(cand, lab, [&](uint32_t r0, unsigned long long group, bool first) {
            unsigned long long low = group;                            // the lanes of the group that hold its largest score
            if (group & (group - 1))                                   // more lanes than the first
                for (int bit = kLkScoreBits - 1; bit >= 0; bit--) {
                    const unsigned long long zero = __ballot(((inv >> bit) & 1u) == 0) & low;
                    if (zero)
                        low = zero;
                }
            const int src = __ffsll((long long)low) - 1;               // the lowest of them: the smallest id
            const uint32_t hi = (uint32_t)__shfl((int)inv, src), id = (uint32_t)__shfl((int)(uint32_t)g64, src);
            const unsigned long long k = (unsigned long long)hi << 32 | id;
            if (r0 != last_root || k < last_key) {
                if (first)
                    atomicMin(&best[r0], k);
                last_root = r0;
                last_key = k;
            }
        });
    });
}

// the bin of a family's gain: 0, 1-9, 10-19, 20-49, 50-99, 100-199, 200-499, >= 500
__device__ inline int lk_gain_bin(uint32_t gain)
{
    return gain == 0 ? 0 : gain < 10 ? 1 : gain < 20 ? 2 : gain < 50 ? 3 : gain < 100 ? 4 : gain < 200 ? 5 : gain < 500 ? 6 : 7;
}

// ---- kept or dropped ------------------------------------------------------------------------------
// The same grid, after k_lk_score on the same stream: every word of best and every score is final.  A well reads its
// label, its members where it is its own root, its own score and, in a family, best[label]: it is kept when it is
// Single or when the low half of that word is its own id.  The mask byte of every well of the run goes to the tile's
// mask, where it has one (maskp, by tile index; a byte store per lane, 64 contiguous bytes per wave).
//   - The counts - PF, Kept, Dropped, MovedIn, and at the roots Families, Moved and the gain bins - are ballots, the
//     same in every lane of a wave, summed in registers over the run; the eight ballots of the gain bins are taken
//     only on a trip whose wave holds a root.
//   - The sums of scores are summed per lane and added up over the wave by shuffles at the end.
// At the end the workgroup adds what is not zero to its copy of the spread counters, once.  Bounds: a count is at most
// kLaneRun per workgroup; a lane sums at most kLaneRun / 256 = 32 scores of at most 65 535, a wave 64 such lanes, the
// workgroup four waves: below 2^29; the memory counters are 64-bit.  Why the result is exact and does not depend on
// the order of execution: every output is a sum over wells of a value that depends on that well's label, members and
// score and its family's word alone, which are final; each well is visited by exactly one lane of one workgroup; adds
// commute and none can overflow; a mask byte is written by its own well's lane alone.
__global__ void __launch_bounds__(kTdBlock) k_lk_mark(const int *__restrict__ tile_idx, int64_t N,
                                                       const uint32_t *__restrict__ label,
                                                       const uint32_t *__restrict__ members,
                                                       const uint16_t *__restrict__ score,
                                                       const unsigned long long *__restrict__ best,
                                                       uint8_t *const *__restrict__ maskp, unsigned long long *cnt_t,
                                                       unsigned long long *cnt_l)
{
    __shared__ uint32_t s_cnt[kLkTileCnt + kLkLaneCnt];
    if (threadIdx.x < kLkTileCnt + kLkLaneCnt)
        s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const LaneRun run(tile_idx, N);
    const int ti = run.ti, lane = threadIdx.x & (kWave - 1);
    uint8_t *mask = maskp[ti];
    uint32_t n_pf = 0, n_kept = 0, n_in = 0, n_fam = 0, n_moved = 0;   // the same in every lane of a wave
    uint32_t n_gain[kLkGainBins] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t sum_kept = 0, sum_dropped = 0, sum_roots = 0;            // this lane's
    run.walk([&](bool has, int64_t w, size_t g64) {
        bool pf = false, kept = false, root = false, copy = false, moved = false;
        int gbin = -1;
        if (has) {
            const uint32_t lab = label[g64];
            if (lab != kInvalid) {
                pf = true;
                const uint32_t sc = score[g64];
                copy = lab != (uint32_t)g64;
                root = !copy && members[g64] != 0;
                kept = !copy && !root;
                if (copy || root) {
                    const unsigned long long b = best[lab];
                    kept = (uint32_t)b == (uint32_t)g64;
                    if (root) {
                        moved = !kept;
                        gbin = lk_gain_bin(kLkMaxScore - (uint32_t)(b >> 32) - sc);
                        sum_roots += sc;
                    }
                }
                if (kept)
                    sum_kept += sc;
                else
                    sum_dropped += sc;
            }
            if (mask)
                mask[w] = kept ? 1 : 0;
        }
        n_pf += (uint32_t)__popcll(__ballot(pf));
        n_kept += (uint32_t)__popcll(__ballot(kept));
        n_in += (uint32_t)__popcll(__ballot(kept && copy));
        const uint32_t roots = (uint32_t)__popcll(__ballot(root));
        if (roots) {                                                   // (the same in every lane of the wave)
            n_fam += roots;
            n_moved += (uint32_t)__popcll(__ballot(moved));
#pragma unroll
            for (int b = 0; b < kLkGainBins; b++)
                n_gain[b] += (uint32_t)__popcll(__ballot(gbin == b));
        }
    });
    for (int off = kWave / 2; off; off >>= 1) {                        // (every lane of the wave takes part)
        sum_kept += (uint32_t)__shfl((int)sum_kept, lane ^ off);
        sum_dropped += (uint32_t)__shfl((int)sum_dropped, lane ^ off);
        sum_roots += (uint32_t)__shfl((int)sum_roots, lane ^ off);
    }
    if (lane == 0) {
        const uint32_t v[kLkTileCnt + kLkLaneCnt] = {n_pf, n_kept, n_pf - n_kept, n_in, sum_kept, sum_dropped, n_fam, n_moved,
                                                     sum_roots, n_gain[0], n_gain[1], n_gain[2], n_gain[3], n_gain[4],
                                                     n_gain[5], n_gain[6], n_gain[7]};
#pragma unroll
        for (int f = 0; f < kLkTileCnt + kLkLaneCnt; f++)
            if (v[f])
                atomicAdd(&s_cnt[f], v[f]);
    }
    __syncthreads();
    if (threadIdx.x < kLkTileCnt) {
        if (s_cnt[threadIdx.x])
            atomicAdd(spread_row(cnt_t, (size_t)ti, kLkTileCnt) + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
    } else if (threadIdx.x < kLkTileCnt + kLkLaneCnt) {
        if (s_cnt[threadIdx.x])
            atomicAdd(spread_row(cnt_l, 0, kLkLaneCnt) + (threadIdx.x - kLkTileCnt), (unsigned long long)s_cnt[threadIdx.x]);
    }
}

}  // namespace

#ifndef WD_LANE_KEEP_EMU                           // (tools/lane_keep_emu.cpp: the kernels above on the CPU, a fiber per lane)
extern "C" {

int wd_lane_keep_scratch(int max_tiles, int64_t wells_per_tile, size_t *bytes)
{
    const int64_t N = wells_per_tile;
    if (max_tiles < 0 || N < 0 || !bytes)
        return WD_ERR_ARG;
    if (max_tiles > 65535)
        return WD_ERR_UNSUPPORTED;
    if (N > 0 && (uint64_t)max_tiles >= (0xFFFFFFFFull + (uint64_t)N - 1) / (uint64_t)N)      // max_tiles * N >= 2^32 - 1
        return WD_ERR_UNSUPPORTED;
    *bytes = lk_layout_of(N, max_tiles).bytes;
    return WD_OK;
}

}  // extern "C"

namespace {

// wd_lane_keep and wd_lane_keep_molecules: one body.  label and members are the finish's, or the mol and molmem of the
// molecule part, which have their form (lane_umi.inc).
int lk_run(wd_lane_dups *ld, int min_q, void *scratch_dev, size_t scratch_bytes, int64_t *lane_row, int64_t *tile_rows,
           uint8_t *const *keep_dev, const uint32_t *label, const uint32_t *members)
{
    wd_ctx *ctx = ld->ctx;
    wd_lane_quality *lq = ld->qual.get();
    const int64_t N = ld->N;
    const int T = ld->max_tiles;
    if (!lq)
        return fail(ctx, WD_ERR_ARG, "lane keep comes after wd_lane_qual_begin");
    LanePass p(ld);
    if (const int rc = p.finished("lane keep comes after a successful finish of the lane"))
        return rc;
    if (min_q < 0 || min_q > WD_LANEKEEP_MAX_Q)
        return fail(ctx, WD_ERR_ARG, "lane keep: min_q is 0.." + std::to_string(WD_LANEKEEP_MAX_Q) + ", not " +
                                         std::to_string(min_q));
    const LkLayout lay = lk_layout_of(N, T);
    if (const int rc = p.scratch(scratch_dev, scratch_bytes, lay.bytes, "scratch smaller than wd_lane_keep_scratch",
                                 "lane keep: the scratch must be in device memory"))
        return rc;
    if (const int rc = lane_part_tiles(ld, lq->added, "lane keep", "qualities"))
        return rc;
    std::vector<uint8_t *> h_mask((size_t)T, nullptr);
    if (keep_dev && N > 0)
        for (int t = 0; t < T; t++) {
            h_mask[t] = keep_dev[t];
            if (h_mask[t] && !on_device(h_mask[t]))
                return fail(ctx, WD_ERR_ARG, "lane keep: the mask of tile index " + std::to_string(t) + " must be in device memory");
        }
    // The weights: bin b's lower edge is the smallest quality the table sends to b (an empty bin never occurs in a
    // row and weighs nothing); it counts from min_q on.
    int weight[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int q = kLqValues - 1; q >= 0; q--) {
        const int b = (int)((lq->tbl.p0 >> q) & 1u) | (int)((lq->tbl.p1 >> q) & 1u) << 1 | (int)((lq->tbl.p2 >> q) & 1u) << 2;
        weight[b] = q >= min_q ? q : 0;
    }
    const LkWeights wts = lk_weights_of(weight);
    memset(lane_row, 0, WD_LANEKEEP_LANE_COLS * sizeof(int64_t));
    memset(tile_rows, 0, (size_t)T * kLkTileCnt * sizeof(int64_t));
    if (!p.start()) {
        if (p.rc != WD_OK || N == 0 || !keep_dev)
            return p.rc;
        if (bind_device(ctx))                                          // wells but no tile: every mask given is zeros
            return WD_ERR_HIP;
        for (int t = 0; t < T; t++)
            if (h_mask[t])
                WD_HIP(ctx, hipMemsetAsync(h_mask[t], 0, (size_t)N, ctx->stream));
        WD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return WD_OK;
    }
    uint8_t *sc = (uint8_t *)scratch_dev;
    unsigned long long *best = (unsigned long long *)(sc + lay.best);
    uint16_t *score = (uint16_t *)(sc + lay.score);
    unsigned long long *cnt_t = (unsigned long long *)(sc + lay.cnt_t);
    unsigned long long *cnt_l = (unsigned long long *)(sc + lay.cnt_l);
    int *d_tidx = (int *)(sc + lay.tidx);
    uint8_t **d_maskp = (uint8_t **)(sc + lay.maskp);
    WD_HIP(ctx, hipMemsetAsync(best, 0xFF, 8 * (size_t)T * (size_t)N, ctx->stream));
    WD_HIP(ctx, hipMemsetAsync(sc + lay.cnt_t, 0, lay.tidx - lay.cnt_t, ctx->stream));
    for (int t = 0; t < T; t++)                                        // a tile never added: its mask is zeros
        if (h_mask[t] && !ld->added[t])
            WD_HIP(ctx, hipMemsetAsync(h_mask[t], 0, (size_t)N, ctx->stream));
    if (const int rc = p.upload(d_tidx))
        return rc;
    WD_HIP(ctx, hipMemcpyAsync(d_maskp, h_mask.data(), (size_t)T * sizeof(void *), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_lk_score, p.grid, dim3(kTdBlock), 0, ctx->stream, d_tidx, N, label, members,
                       (const uint32_t *)(lq->ws + lq->lay.qrows), ld->lay.words, wts, score, best);
    WD_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lk_mark, p.grid, dim3(kTdBlock), 0, ctx->stream, d_tidx, N, label, members, (const uint16_t *)score,
                       (const unsigned long long *)best, (uint8_t *const *)d_maskp, cnt_t, cnt_l);
    WD_HIP(ctx, hipGetLastError());
    SpreadFetch f_t(cnt_t, (size_t)T, kLkTileCnt), f_l(cnt_l, 1, kLkLaneCnt);
    if (const int rc = spread_fetch(ctx, {&f_t, &f_l}))               // (h_mask is alive until the stream is synchronised)
        return rc;
    lane_pass_rows(f_t, T, tile_rows, lane_row, &f_l, kLkLaneCnt);
    return WD_OK;
}

}  // namespace

extern "C" {

int wd_lane_keep(wd_lane_dups *ld, int min_q, void *scratch_dev, size_t scratch_bytes, int64_t *lane_row,
                 int64_t *tile_rows, uint8_t *const *keep_dev)
try {
    if (!ld || !lane_row || !tile_rows)
        return WD_ERR_ARG;
    return lk_run(ld, min_q, scratch_dev, scratch_bytes, lane_row, tile_rows, keep_dev,
                  (const uint32_t *)(ld->ws + ld->lay.label), (const uint32_t *)(ld->ws + ld->lay.members));
} WD_CATCH

int wd_lane_keep_molecules(wd_lane_dups *ld, int min_q, void *scratch_dev, size_t scratch_bytes, int64_t *lane_row,
                           int64_t *tile_rows, uint8_t *const *keep_dev)
try {
    if (!ld || !lane_row || !tile_rows)
        return WD_ERR_ARG;
    if (!ld->mol)
        return fail(ld->ctx, WD_ERR_ARG, "lane keep by molecule comes after a successful wd_lane_umi_molecules since the finish");
    const LmolLayout ml = lmol_layout_of(ld->max_tiles, ld->N);
    const uintptr_t m0 = (uintptr_t)ld->mol, s0 = (uintptr_t)scratch_dev;
    if (scratch_dev && m0 < s0 + scratch_bytes && s0 < m0 + ml.bytes)
        return fail(ld->ctx, WD_ERR_ARG, "lane keep: the scratch overlaps the molecule region");
    return lk_run(ld, min_q, scratch_dev, scratch_bytes, lane_row, tile_rows, keep_dev, (const uint32_t *)(ld->mol + ml.mol),
                  (const uint32_t *)(ld->mol + ml.molmem));
} WD_CATCH

}  // extern "C"
#endif
