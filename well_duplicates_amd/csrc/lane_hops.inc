// lane_hops.inc - which libraries a lane's duplicate copies join (include/welldup_lanehops.h): the index key of
// every redundant well of a lane held against its root's - the two index reads' distances put into nine states,
// and the pair counted in the matrix cell [root's library][copy's library] of the caller's listing.  Included from
// welldup_tiledups.hip after lane_index.inc (the index part and its keys) and lane_mismatch.inc (lm_fold): it uses
// read_classes.inc (the spread counters), lane_dups.inc (the accumulator and its label array) and lane_pass.inc
// (the run, the grouping by key, the start of a pass and the counters' way back).
//
// wd_lane_hops, over the tiles that were added (grid y = tile): one kernel, k_lh_tally, and nothing else.  It reads
// label and the index workspace's key and writes the caller's scratch only; who writes those two, and when, stands
// at the head of lane_mismatch.inc.
#include "welldup_lanehops.h"

namespace {

constexpr int kLhMaxE = WD_LANEHOPS_MAX_E;
constexpr int kLhStates = WD_LANEHOPS_STATES;
constexpr int kLhTileCnt = WD_LANEHOPS_TILE_COLS;          // per tile and copy: Pairs, SameTile, Hop1, Hop2
constexpr int kLhLaneCnt = 16;                     // per copy: State
constexpr int kLhMaxListed = WD_LANEHOPS_MAX_LISTED;
constexpr int kLhSlots = 1024;                     // entries of a workgroup's table of matrix cells
constexpr int kLhProbe = 8;
static_assert(kLhStates <= kLhLaneCnt, "State has a counter per state");
static_assert((kLhSlots & (kLhSlots - 1)) == 0, "the LDS table is a power of two");
static_assert((uint64_t)(kLhMaxListed + 1) * (kLhMaxListed + 1) < 0xFFFFFFFFull, "a pair code is 32 bits and never kInvalid");
static_assert(kLhMaxListed < 65536, "a rank is 16 bits");
// the listed keys 8 bytes and their ranks 2, the table 8 an entry, the counters: eight workgroups within a CU's 160 KB
static_assert(kLhMaxListed * 10 + kLhSlots * 8 + (kLhTileCnt + kLhStates) * 4 <= 20480, "20 KB of LDS a workgroup");

// the scratch (include/welldup_lanehops.h states the arithmetic)
struct LhLayout {
    size_t cnt_t, cnt_l, tidx, keys, rank, matrix, bytes;
};

LhLayout lh_layout_of(int max_tiles, int M)
{
    LhLayout l;
    const size_t t = (size_t)max_tiles, m = (size_t)M;
    l.cnt_t = 0;
    l.cnt_l = align256(l.cnt_t + t * kSpread * kLhTileCnt * 8);
    l.tidx = align256(l.cnt_l + (size_t)kSpread * kLhLaneCnt * 8);
    l.keys = align256(l.tidx + t * sizeof(int));
    l.rank = align256(l.keys + m * 8);
    l.matrix = align256(l.rank + m * 2);
    l.bytes = align256(l.matrix + (m + 1) * (m + 1) * 8);
    return l;
}

// The state of a part: d cycles of it differ.
__device__ inline uint32_t lh_state(int d, int max_e) { return d == 0 ? 0u : d <= max_e ? 1u : 2u; }

// The rank of a key: its position in the caller's list, M when it is not there.  The listed keys lie in LDS as a
// sorted list with the caller's position of each beside it, and a lookup is a binary search - not an open-addressing
// table: at M = 1024 a table that is at most half full takes 2048 x 8 bytes for the keys alone, and with the ranks
// and the table of matrix cells the workgroup would pass its 20 KB; the sorted list takes 10 bytes a key, needs no
// empty value (every 64-bit word but the keys' unused bits could be a key), and a lookup is at most eleven LDS
// loads whatever the keys are, where a chain of probes depends on them.  Only a pair looks up, and a pair whose two
// keys are equal - every pair of a lane without mixed classes - looks up once.
__device__ inline uint32_t lh_rank(const unsigned long long *s_keys, const uint16_t *s_rank, int M, unsigned long long k)
{
    int lo = 0, hi = M;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_keys[mid] < k)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < M && s_keys[lo] == k ? s_rank[lo] : (uint32_t)M;
}

// ---- tally --------------------------------------------------------------------------------------
// LaneRun's grid and walk (lane_pass.inc), one well per lane and trip.  A well that is PF (it has a label) and not
// its own root is a pair: it loads its key and its root's - one 8-byte gather -, and d1 and d2 are the popcounts of
// the two words' folded XOR (lm_fold: one bit per differing code) under the two masks the host built from the split.
//   - State and the tile's four counters.  A lane of one library puts every pair into State[0]: the pairs of a wave
//     are grouped by state (wave_by_key) and the first lane of a group adds the group's size to the workgroup's State
//     in LDS.  Pairs, Hop1 and Hop2 follow from the groups and SameTile from one ballot, so they are the same in
//     every lane of a wave: they are summed in registers over the run, and the wave's first lane adds them to LDS
//     once.  At the end the workgroup adds what is not zero to its copy of the spread counters.
//   - The matrix.  The pair code a (M + 1) + b - a the root's rank, b the copy's - is grouped the same way: a lane of
//     one library has one code in the whole lane, a lane of a thousand libraries a million.  The group's first lane
//     adds the group's size to the workgroup's table in LDS: open addressing keyed by the code, kLhSlots entries of
//     {code, count}, k_li_tally's scheme.  An add that finds kLhProbe entries in a row taken by other codes goes
//     to the cell in memory at once (it is already wave-grouped), so the result is exact for any number of distinct
//     pairs; at the end an occupied entry is flushed with one global atomic.
// Why the result is exact and does not depend on the order of execution: every output is a sum of ones over wells,
// each well is visited by exactly one lane of one workgroup, integer adds commute and none can overflow (a 32-bit
// LDS counter takes at most kLaneRun, the memory counters are 64-bit); an entry of the table is claimed once by a
// compare-and-swap and never freed, so every add of a code goes to the one entry that holds it or, past kLhProbe
// foreign entries, to the cell itself - which of the two depends on the order, their sum does not; what a lane
// reads - label, key and the listing - was written by launches and copies that ended before this launch began, and
// nothing writes label or key after a successful finish (the head of lane_mismatch.inc says where that was
// checked); a root's label is a global id of a PF well of an added tile, whose key k_li_pack wrote - the host
// refuses a lane whose index planes cover other tiles than its reads; a rank is at most M, so a code lies inside
// the matrix.
__global__ void __launch_bounds__(kTdBlock) k_lh_tally(const int *__restrict__ tile_idx, int64_t N,
                                                        const uint32_t *__restrict__ label,
                                                        const uint2 *__restrict__ key, unsigned long long mask1,
                                                        unsigned long long mask2, int max_e, int M,
                                                        const unsigned long long *__restrict__ listed,
                                                        const uint16_t *__restrict__ rank, unsigned long long *cnt_t,
                                                        unsigned long long *cnt_l, unsigned long long *matrix)
{
    __shared__ unsigned long long s_keys[kLhMaxListed];
    __shared__ uint16_t s_rank[kLhMaxListed];
    __shared__ uint32_t s_code[kLhSlots], s_n[kLhSlots];
    __shared__ uint32_t s_cnt[kLhTileCnt + kLhStates];                 // Pairs, SameTile, Hop1, Hop2, State
    for (int e = threadIdx.x; e < M; e += kTdBlock) {
        s_keys[e] = listed[e];
        s_rank[e] = rank[e];
    }
    for (int e = threadIdx.x; e < kLhSlots; e += kTdBlock) {
        s_code[e] = kInvalid;
        s_n[e] = 0;
    }
    if (threadIdx.x < kLhTileCnt + kLhStates)
        s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const LaneRun run(tile_idx, N);
    const int ti = run.ti, lane = threadIdx.x & (kWave - 1);
    const uint32_t width = (uint32_t)M + 1u;
    uint32_t n_pairs = 0, n_same = 0, n_hop1 = 0, n_hop2 = 0;          // the same in every lane of a wave
    run.walk([&](bool has, int64_t, size_t g64) {
        bool pair = false, same_tile = false;
        uint32_t state = 0, code = 0;
        if (has) {
            const uint32_t lab = label[g64];
            if (lab != kInvalid && lab != (uint32_t)g64) {
                pair = true;
                const uint2 kr = key[lab], kc = key[g64];
                const unsigned long long diff = (unsigned long long)lm_fold(kr.y, kc.y) << 32 | lm_fold(kr.x, kc.x);
                state = 3u * lh_state(__popcll(diff & mask1), max_e) + lh_state(__popcll(diff & mask2), max_e);
                same_tile = (size_t)lab >= run.base && (size_t)lab - run.base < (size_t)N;
                const uint32_t a = lh_rank(s_keys, s_rank, M, (unsigned long long)kr.y << 32 | kr.x);
                const uint32_t b = diff ? lh_rank(s_keys, s_rank, M, (unsigned long long)kc.y << 32 | kc.x) : a;
                code = a * width + b;
            }
        }
        wave_by_key(pair, state, [&](uint32_t s0, unsigned long long group, bool first) {
            const uint32_t n = (uint32_t)__popcll(group);
            if (first)
                atomicAdd(&s_cnt[kLhTileCnt + s0], n);
            n_pairs += n;
            const uint32_t far = (s0 / 3u == 2u) + (s0 % 3u == 2u);
            n_hop1 += far == 1u ? n : 0u;
            n_hop2 += far == 2u ? n : 0u;
        });
        n_same += (uint32_t)__popcll(__ballot(pair && same_tile));
        wave_by_key(pair, code, [&](uint32_t c0, unsigned long long group, bool first) {
            if (!first)
                return;
            const uint32_t n = (uint32_t)__popcll(group);
            uint32_t e = (c0 * 0x9E3779B1u) >> 22 & (kLhSlots - 1);
            int p = 0;
            for (; p < kLhProbe; p++, e = (e + 1) & (kLhSlots - 1)) {
                const uint32_t old = atomicCAS(&s_code[e], kInvalid, c0);
                if (old == kInvalid || old == c0)
                    break;
            }
            if (p < kLhProbe)
                atomicAdd(&s_n[e], n);
            else
                atomicAdd(matrix + c0, (unsigned long long)n);
        });
    });
    if (lane == 0) {
        if (n_pairs)
            atomicAdd(&s_cnt[0], n_pairs);
        if (n_same)
            atomicAdd(&s_cnt[1], n_same);
        if (n_hop1)
            atomicAdd(&s_cnt[2], n_hop1);
        if (n_hop2)
            atomicAdd(&s_cnt[3], n_hop2);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kLhSlots; e += kTdBlock)
        if (s_code[e] != kInvalid)
            atomicAdd(matrix + s_code[e], (unsigned long long)s_n[e]);
    if (threadIdx.x < kLhTileCnt + kLhStates && s_cnt[threadIdx.x]) {
        const unsigned long long v = s_cnt[threadIdx.x];
        if (threadIdx.x < kLhTileCnt)
            atomicAdd(spread_row(cnt_t, (size_t)ti, kLhTileCnt) + threadIdx.x, v);
        else
            atomicAdd(spread_row(cnt_l, 0, kLhLaneCnt) + (threadIdx.x - kLhTileCnt), v);
    }
}

// the bit of lm_fold for each of the index cycles c0 .. c1 - 1 of a 64-bit key
unsigned long long lh_mask(int c0, int c1)
{
    unsigned long long m = 0;
    for (int c = c0; c < c1; c++)
        m |= 1ull << (32 * (c / kFpCycles) + 3 * (c % kFpCycles));
    return m;
}

}  // namespace

#ifndef WD_LANE_HOPS_EMU                           // (tools/lane_hops_emu.cpp: the kernel above on the CPU, a fiber per lane)
namespace {

std::string lh_hex(uint64_t k)
{
    char buf[24];
    snprintf(buf, sizeof buf, "0x%016llx", (unsigned long long)k);
    return buf;
}

// a key a well of I index cycles can carry: codes 0..4 in the first I places, every other bit zero
bool lh_key_possible(uint64_t k, int I)
{
    for (int c = 0; c < 2 * kFpCycles; c++) {
        const unsigned code = (unsigned)(k >> (32 * (c / kFpCycles) + 3 * (c % kFpCycles))) & 7u;
        if (code > 4u || (c >= I && code))
            return false;
    }
    return !(k & 0xC0000000C0000000ull);
}

}  // namespace

extern "C" {

int wd_lane_hops_scratch(int max_tiles, int M, size_t *bytes)
{
    if (max_tiles < 0 || M < 0 || M > kLhMaxListed || !bytes)
        return WD_ERR_ARG;
    if (max_tiles > 65535)
        return WD_ERR_UNSUPPORTED;
    *bytes = lh_layout_of(max_tiles, M).bytes;
    return WD_OK;
}

int wd_lane_hops(wd_lane_dups *ld, int split, int max_e, int M, const uint64_t *listed_keys, void *scratch_dev,
                 size_t scratch_bytes, int64_t *lane_row, int64_t *tile_rows, int64_t *matrix)
try {
    if (!ld || !lane_row || !tile_rows || !matrix)
        return WD_ERR_ARG;
    wd_ctx *ctx = ld->ctx;
    const int64_t N = ld->N;
    const int T = ld->max_tiles;
    LanePass p(ld);
    if (const int rc = p.finished("lane hops come after a successful finish of the lane"))
        return rc;
    wd_lane_index *li = ld->index.get();
    if (!li)
        return fail(ctx, WD_ERR_ARG, "lane hops: the lane has no index part (wd_lane_index_begin)");
    if (const int rc = lane_part_tiles(ld, li->added, "lane index", "index planes"))      // (the part's head, not the pass's)
        return rc;
    const int I = li->cycles;
    if (split < 1 || split > I)
        return fail(ctx, WD_ERR_ARG, "lane hops: split is 1.." + std::to_string(I) + ", not " + std::to_string(split));
    if (max_e < 0 || max_e > kLhMaxE)
        return fail(ctx, WD_ERR_ARG, "lane hops: max_e is 0.." + std::to_string(kLhMaxE) + ", not " + std::to_string(max_e));
    if (M < 0 || M > kLhMaxListed)
        return fail(ctx, WD_ERR_ARG, "lane hops: 0.." + std::to_string(kLhMaxListed) + " listed keys, not " + std::to_string(M));
    if (M > 0 && !listed_keys)
        return fail(ctx, WD_ERR_ARG, "lane hops: null list of keys");
    // the listing sorted by key, each key with its place in the caller's list
    std::vector<std::pair<uint64_t, uint16_t>> order((size_t)M);
    for (int i = 0; i < M; i++) {
        if (!lh_key_possible(listed_keys[i], I))
            return fail(ctx, WD_ERR_ARG, "lane hops: listed key " + lh_hex(listed_keys[i]) + " is no index read of " +
                                             std::to_string(I) + " cycles");
        order[(size_t)i] = {listed_keys[i], (uint16_t)i};
    }
    std::sort(order.begin(), order.end());
    for (int i = 1; i < M; i++)
        if (order[(size_t)i].first == order[(size_t)i - 1].first)
            return fail(ctx, WD_ERR_ARG, "lane hops: listed key " + lh_hex(order[(size_t)i].first) + " is given twice");
    const LhLayout lay = lh_layout_of(T, M);
    if (const int rc = p.scratch(scratch_dev, scratch_bytes, lay.bytes, "scratch smaller than wd_lane_hops_scratch",
                                 "lane hops: the scratch must be in device memory"))
        return rc;
    const size_t cells = ((size_t)M + 1) * ((size_t)M + 1);
    memset(lane_row, 0, WD_LANEHOPS_LANE_COLS * sizeof(int64_t));
    memset(tile_rows, 0, (size_t)T * kLhTileCnt * sizeof(int64_t));
    memset(matrix, 0, cells * sizeof(int64_t));
    if (!p.start())
        return p.rc;
    uint8_t *sc = (uint8_t *)scratch_dev;
    unsigned long long *cnt_t = (unsigned long long *)(sc + lay.cnt_t);
    unsigned long long *cnt_l = (unsigned long long *)(sc + lay.cnt_l);
    int *d_tidx = (int *)(sc + lay.tidx);
    unsigned long long *d_keys = (unsigned long long *)(sc + lay.keys);
    uint16_t *d_rank = (uint16_t *)(sc + lay.rank);
    unsigned long long *d_matrix = (unsigned long long *)(sc + lay.matrix);
    std::vector<unsigned long long> h_keys((size_t)M);
    std::vector<uint16_t> h_rank((size_t)M);
    for (int i = 0; i < M; i++) {
        h_keys[(size_t)i] = order[(size_t)i].first;
        h_rank[(size_t)i] = order[(size_t)i].second;
    }
    WD_HIP(ctx, hipMemsetAsync(sc, 0, lay.bytes, ctx->stream));
    if (const int rc = p.upload(d_tidx))
        return rc;
    if (M > 0) {
        WD_HIP(ctx, hipMemcpyAsync(d_keys, h_keys.data(), (size_t)M * 8, hipMemcpyHostToDevice, ctx->stream));
        WD_HIP(ctx, hipMemcpyAsync(d_rank, h_rank.data(), (size_t)M * 2, hipMemcpyHostToDevice, ctx->stream));
    }
    hipLaunchKernelGGL(k_lh_tally, p.grid, dim3(kTdBlock), 0, ctx->stream, d_tidx, N,
                       (const uint32_t *)(ld->ws + ld->lay.label), (const uint2 *)(li->ws + li->lay.key), lh_mask(0, split),
                       lh_mask(split, I), max_e, M, d_keys, d_rank, cnt_t, cnt_l, d_matrix);
    WD_HIP(ctx, hipGetLastError());
    SpreadFetch f_t(cnt_t, (size_t)T, kLhTileCnt), f_l(cnt_l, 1, kLhLaneCnt);
    WD_HIP(ctx, hipMemcpyAsync(matrix, d_matrix, cells * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (const int rc = spread_fetch(ctx, {&f_t, &f_l}))      // (h_keys and h_rank live until the stream is drained)
        return rc;
    lane_pass_rows(f_t, T, tile_rows, lane_row, &f_l, kLhStates);
    return WD_OK;
} WD_CATCH

}  // extern "C"
#endif
