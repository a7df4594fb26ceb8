// lane_distance.inc - how far apart a lane's duplicate copies lie (include/welldup_lanedistance.h): every redundant
// well of a lane against its root, by where the two sit - same tile or not, and for the same tile the squared
// distance of their coordinates binned by powers of four and held against the caller's radius.  Included at the end
// of welldup_tiledups.hip, after lane_mismatch.inc: it uses read_classes.inc (the spread counters), lane_dups.inc
// (the accumulator, its label array) and lane_pass.inc as lane_mismatch.inc does, with its coordinate check.
//
// wd_lane_distances, over the tiles that were added (grid y = tile): one kernel, k_lg_tally, and nothing else.  It
// reads label and writes the caller's scratch only.  Who writes label, and that nobody does after a successful
// finish, is listed at the head of lane_mismatch.inc; this pass joins that list as a reader: it touches neither the
// rows nor the table, aux or the index workspace.
#include "welldup_lanedistance.h"

namespace {

constexpr int kLgBins = WD_LANEDISTANCE_DIST_BINS;
constexpr int kLgTileCnt = WD_LANEDISTANCE_TILE_COLS;      // per tile and copy: Pairs, SameTile, Local
constexpr int kLgLaneCnt = 16;                     // per copy: Dist
constexpr int kLgHist = WD_LANEDISTANCE_MATRIX_MAX_TILES;  // root tiles a workgroup counts in LDS
constexpr int kLgCrossKey = 16;                    // grouping key of a cross-tile pair: kLgCrossKey + its root's tile
static_assert(kLgBins <= kLgLaneCnt && kLgBins <= kLgCrossKey, "a bin is a key below the cross-tile keys");
static_assert(kLgHist * 4 <= 16384, "the root-tile histogram: 16 KB of LDS, k_lm_tally's budget");

// the scratch (include/welldup_lanedistance.h states the arithmetic)
struct LgLayout {
    size_t xy, cnt_t, cnt_l, tidx, pairs, bytes;
};

LgLayout lg_layout_of(int64_t N, int max_tiles, bool matrix)
{
    LgLayout l;
    const size_t t = (size_t)max_tiles;
    l.xy = 0;
    l.cnt_t = align256(l.xy + (size_t)N * 8);
    l.cnt_l = align256(l.cnt_t + t * kSpread * kLgTileCnt * 8);
    l.tidx = align256(l.cnt_l + (size_t)kSpread * kLgLaneCnt * 8);
    l.pairs = align256(l.tidx + t * sizeof(int));
    l.bytes = matrix ? align256(l.pairs + t * t * 8) : l.pairs;
    return l;
}

// The bin of q: 0 below 2^10, b for 2^(8 + 2b) <= q < 2^(10 + 2b), the last from 2^28 on - read off the position
// h of q's highest bit (bits 8 + 2b and 9 + 2b belong to bin b; q | 256 lifts every q below 2^8 to h = 8, bin 0,
// and changes no h above).
__device__ inline int lg_bin(unsigned long long q)
{
    const int h = 63 - __clzll((long long)(q | 256ull));
    return min((h - 8) >> 1, kLgBins - 1);
}

// ---- tally --------------------------------------------------------------------------------------
// LaneRun's grid and walk (lane_pass.inc).  A well that is PF (it has a label) and not its own root is a pair.  Its
// root lies on the same tile when label - base < N (the root is the smaller id, so it is never beyond the tile): no
// division.  A same-tile pair loads its own (x, y) - coalesced - and its root's - anywhere in the 8 N bytes of the
// table -, forms q in 64 bits and takes its bin from q's highest bit.  Only a cross-tile pair divides, for its root's
// tile, and only when the matrix is wanted (n_hist > 0).
//   - Pairs, SameTile and Local are three ballots per trip, the same in every lane of the wave: summed in registers
//     over the run, added to LDS once by the wave's first lane.
//   - Dist and the root tiles.  A lane of equal reads puts every pair on one root - one bin, or one root tile -, a
//     lane of copies beside their originals puts every pair into Dist[0].  So the pairs of a wave are grouped by key
//     (wave_by_key: the bin, or kLgCrossKey + the root's tile), and the first lane of a group adds the group's size to
//     the workgroup's Dist or to its histogram of root tiles [kLgHist] in LDS (32-bit: a run adds at most kLaneRun).
//     SameTile goes to the tile's own entry of the histogram - the diagonal of TilePairs.
// At the end the workgroup adds what is not zero: the counters to its copy of the spread rows, the histogram to
// column tile of TilePairs with one 64-bit atomic per root tile it met.
// Why the result is exact and does not depend on the order of execution: every output is a sum of ones over wells,
// each well is visited by exactly one lane of one workgroup, integer adds commute and none can overflow; q < 2^49
// is exact in 64 bits (coordinates below 2^24, checked on the host); label and the coordinates were written before
// this launch began; a root's label is a global id of a PF well of an added tile, so a same-tile root's offset is a
// well of the table.
__global__ void __launch_bounds__(kTdBlock) k_lg_tally(const int *__restrict__ tile_idx, int64_t N,
                                                        const uint32_t *__restrict__ label,
                                                        const int2 *__restrict__ xy, unsigned long long radius2,
                                                        int n_hist, unsigned long long *cnt_t,
                                                        unsigned long long *cnt_l, unsigned long long *tile_pairs)
{
    __shared__ uint32_t s_hist[kLgHist];
    __shared__ uint32_t s_cnt[kLgTileCnt + kLgBins];                  // Pairs, SameTile, Local, Dist
    for (int e = threadIdx.x; e < n_hist; e += kTdBlock)
        s_hist[e] = 0;
    if (threadIdx.x < kLgTileCnt + kLgBins)
        s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const LaneRun run(tile_idx, N);
    const int ti = run.ti, lane = threadIdx.x & (kWave - 1);
    uint32_t n_pairs = 0, n_same = 0, n_local = 0;                   // the same in every lane of a wave
    run.walk([&](bool has, int64_t w, size_t g64) {
        bool pair = false, same = false, local = false;
        int key = -1;                                                  // (-1: nothing to group)
        if (has) {
            const uint32_t lab = label[g64];
            if (lab != kInvalid && lab != (uint32_t)g64) {
                pair = true;
                const int64_t off = (int64_t)lab - (int64_t)run.base;
                same = off >= 0 && off < N;
                if (same) {
                    const int2 a = xy[w], b = xy[off];
                    const int64_t dx = (int64_t)a.x - b.x, dy = (int64_t)a.y - b.y;
                    const unsigned long long q = (unsigned long long)(dx * dx + dy * dy);
                    key = lg_bin(q);
                    local = q < radius2;
                } else if (n_hist) {
                    key = kLgCrossKey + (int)(lab / (uint32_t)N);
                }
            }
        }
        n_pairs += (uint32_t)__popcll(__ballot(pair));
        n_same += (uint32_t)__popcll(__ballot(same));
        n_local += (uint32_t)__popcll(__ballot(local));
        wave_by_key(key >= 0, (uint32_t)key, [&](uint32_t k0, unsigned long long group, bool first) {
            if (first) {
                const uint32_t n = (uint32_t)__popcll(group);
                if (k0 < (uint32_t)kLgCrossKey)
                    atomicAdd(&s_cnt[kLgTileCnt + k0], n);
                else
                    atomicAdd(&s_hist[k0 - kLgCrossKey], n);
            }
        });
    });
    if (lane == 0) {
        if (n_pairs)
            atomicAdd(&s_cnt[0], n_pairs);
        if (n_same) {
            atomicAdd(&s_cnt[1], n_same);
            if (n_hist)
                atomicAdd(&s_hist[ti], n_same);
        }
        if (n_local)
            atomicAdd(&s_cnt[2], n_local);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < n_hist; e += kTdBlock)
        if (s_hist[e])
            atomicAdd(tile_pairs + (size_t)e * (size_t)n_hist + ti, (unsigned long long)s_hist[e]);
    if (threadIdx.x < kLgTileCnt + kLgBins && s_cnt[threadIdx.x]) {
        const unsigned long long v = s_cnt[threadIdx.x];
        if (threadIdx.x < kLgTileCnt)
            atomicAdd(spread_row(cnt_t, (size_t)ti, kLgTileCnt) + threadIdx.x, v);
        else
            atomicAdd(spread_row(cnt_l, 0, kLgLaneCnt) + (threadIdx.x - kLgTileCnt), v);
    }
}

}  // namespace

#ifndef WD_LANE_DISTANCE_EMU                       // (tools/lane_distance_emu.cpp: the kernel above on the CPU, a fiber per lane)
extern "C" {

int wd_lane_distance_scratch(int64_t N, int max_tiles, int matrix, size_t *bytes)
{
    if (N < 0 || max_tiles < 0 || !bytes)
        return WD_ERR_ARG;
    if (max_tiles > 65535 || (matrix && max_tiles > kLgHist))
        return WD_ERR_UNSUPPORTED;
    *bytes = lg_layout_of(N, max_tiles, matrix != 0).bytes;
    return WD_OK;
}

int wd_lane_distances(wd_lane_dups *ld, const int32_t *x, const int32_t *y, int64_t radius, void *scratch_dev,
                      size_t scratch_bytes, int64_t *lane_row, int64_t *tile_rows, int64_t *tile_pairs)
try {
    if (!ld || !x || !y || !lane_row || !tile_rows)
        return WD_ERR_ARG;
    wd_ctx *ctx = ld->ctx;
    const int64_t N = ld->N;
    const int T = ld->max_tiles;
    const bool matrix = tile_pairs != nullptr;
    LanePass p(ld);
    if (const int rc = p.finished("lane distances come after a successful finish of the lane"))
        return rc;
    if (const int rc = lane_pass_radius(ctx, "lane distances", radius))
        return rc;
    if (matrix && T > kLgHist)
        return fail(ctx, WD_ERR_UNSUPPORTED, "lane distances: TilePairs takes at most " + std::to_string(kLgHist) + " tiles");
    const LgLayout lay = lg_layout_of(N, T, matrix);
    if (const int rc = p.scratch(scratch_dev, scratch_bytes, lay.bytes, "scratch smaller than wd_lane_distance_scratch",
                                 "lane distances: the scratch must be in device memory"))
        return rc;
    std::vector<int2> h_xy;
    if (const int rc = lane_pass_coords(ctx, "lane distances", x, y, N, h_xy))
        return rc;
    memset(lane_row, 0, WD_LANEDISTANCE_LANE_COLS * sizeof(int64_t));
    memset(tile_rows, 0, (size_t)T * kLgTileCnt * sizeof(int64_t));
    if (matrix)
        memset(tile_pairs, 0, (size_t)T * T * sizeof(int64_t));
    if (!p.start())
        return p.rc;
    uint8_t *sc = (uint8_t *)scratch_dev;
    unsigned long long *cnt_t = (unsigned long long *)(sc + lay.cnt_t);
    unsigned long long *cnt_l = (unsigned long long *)(sc + lay.cnt_l);
    int *d_tidx = (int *)(sc + lay.tidx);
    unsigned long long *d_pairs = (unsigned long long *)(sc + lay.pairs);
    WD_HIP(ctx, hipMemcpyAsync(sc + lay.xy, h_xy.data(), (size_t)N * 8, hipMemcpyHostToDevice, ctx->stream));
    WD_HIP(ctx, hipMemsetAsync(sc + lay.cnt_t, 0, lay.bytes - lay.cnt_t, ctx->stream));
    if (const int rc = p.upload(d_tidx))
        return rc;
    hipLaunchKernelGGL(k_lg_tally, p.grid, dim3(kTdBlock), 0, ctx->stream, d_tidx, N,
                       (const uint32_t *)(ld->ws + ld->lay.label), (const int2 *)(sc + lay.xy),
                       (unsigned long long)radius * (unsigned long long)radius, matrix ? T : 0, cnt_t, cnt_l, d_pairs);
    WD_HIP(ctx, hipGetLastError());
    SpreadFetch f_t(cnt_t, (size_t)T, kLgTileCnt), f_l(cnt_l, 1, kLgLaneCnt);
    if (matrix)
        WD_HIP(ctx, hipMemcpyAsync(tile_pairs, d_pairs, (size_t)T * T * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (const int rc = spread_fetch(ctx, {&f_t, &f_l}))
        return rc;
    lane_pass_rows(f_t, T, tile_rows, lane_row, &f_l, kLgBins);
    return WD_OK;
} WD_CATCH

}  // extern "C"
#endif
