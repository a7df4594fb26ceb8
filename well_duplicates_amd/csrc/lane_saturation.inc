// lane_saturation.inc - a lane's distinct reads against its depth (include/welldup_lanesaturation.h): every PF well
// of a lane gets a pseudo-random step from its global id, and per step the wells and the distinct reads that the
// step brings are counted - the lane's saturation curve, exact, optionally without the local copies
// lane_distance.inc counts.  Included at the end of welldup_tiledups.hip, after everything of lane_quality.inc (from
// that file's last lines: the unit's own last line is pinned): it uses read_classes.inc (the spread counters),
// lane_dups.inc (the accumulator, its label array) and lane_pass.inc as lane_distance.inc does.
//
// wd_lane_saturation, over the tiles that were added (grid y = tile): a memset and two kernels, k_ls_min and
// k_ls_tally.  They read label and write the caller's scratch only.  Who writes label, and that nobody does after a
// successful finish, is listed at the head of lane_mismatch.inc; this pass joins that list as a reader: it touches
// neither the rows nor the table, aux, the index workspace or the quality workspace.
#include "welldup_lanesaturation.h"

namespace {

constexpr int kLsSteps = WD_LANESATURATION_MAX_STEPS;
constexpr int kLsHead = WD_LANESATURATION_HEAD_COLS;       // per copy: PF, Dropped
constexpr int kLsStepBits = 6;                     // a step is below 2^6
static_assert(kLsSteps <= 1 << kLsStepBits, "the smallest step of a wave's group is found bit by bit");
static_assert(2 * kLsSteps <= kTdBlock, "a lane per bin when the workgroup adds its histogram");

// the scratch (include/welldup_lanesaturation.h states the arithmetic)
struct LsLayout {
    size_t cls, xy, cnt, head, tidx, bytes;
};

LsLayout ls_layout_of(int64_t N, int max_tiles, bool with_coords)
{
    LsLayout l;
    const size_t t = (size_t)max_tiles;
    l.cls = 0;
    l.xy = align256(l.cls + 4 * t * (size_t)N);
    l.cnt = with_coords ? align256(l.xy + (size_t)N * 8) : l.xy;
    l.head = align256(l.cnt + (size_t)kSpread * 2 * kLsSteps * 8);
    l.tidx = align256(l.head + (size_t)kSpread * kLsHead * 8);
    l.bytes = align256(l.tidx + t * sizeof(int));
    return l;
}

// The step of global id g: salt = seed * 0x9E3779B9 (formed on the host), the finalizer of MurmurHash3, and the
// high word of h * S - uniform over 0 .. S - 1 up to one part in 2^32 / S.
__device__ inline uint32_t ls_step(uint32_t g, uint32_t salt, uint32_t S)
{
    uint32_t h = g + salt;
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return (uint32_t)(((unsigned long long)h * S) >> 32);
}

// Is the pair (well w of the tile at base, label lab) dropped?  k_lg_tally's test of Local: the root lies on the
// same tile when lab - base is in 0 .. N - 1 (no division), then two 8-byte loads and q in 64 bits.  radius2 = 0
// (no radius, or no coordinates: xy is null then): nothing is dropped and nothing is loaded.
__device__ inline bool ls_dropped(int64_t w, uint32_t lab, size_t base, int64_t N, const int2 *__restrict__ xy,
                                  unsigned long long radius2)
{
    if (!radius2)
        return false;
    const int64_t off = (int64_t)lab - (int64_t)base;
    if (off < 0 || off >= N)
        return false;
    const int2 a = xy[w], b = xy[off];
    const int64_t dx = (int64_t)a.x - b.x, dy = (int64_t)a.y - b.y;
    return (unsigned long long)(dx * dx + dy * dy) < radius2;
}

// ---- the class steps ------------------------------------------------------------------------------
// LaneRun's grid and walk (lane_pass.inc).  cls: a word per well of the lane, all 0xFFFFFFFF when the kernel starts
// (a memset on the same stream).  A counted well that is a pair (PF, not its own root, not dropped) forms its step and
// reads its root's word - every lane of the wave at once -; it is a candidate only where its step is smaller.  Roots
// and wells in no class write nothing: k_ls_tally takes the minimum with their own step.  A dropped well takes no
// part.
//   - The candidates of a wave are grouped by root (wave_by_key), and the group's first lane issues one atomicMin of
//     the group's smallest step; nobody waits for it.  A group of one lane - the usual case: a class has few members
//     and they lie anywhere - has its step at hand; of a larger group the smallest step is found bit by bit from the
//     top with six ballots (a step is below 64).  A lane of equal reads puts every pair on one root: with one
//     atomicMin per candidate k_ls_min took 3.4 ms on three such tiles, 40 times the planted lane's time per tile
//     (DESIGN 5.18).
//   - A wave remembers the root it served last and the step it left there: a group of the same root with no smaller
//     step is skipped - this wave's own atomicMin has already brought the word that low, whatever a stale read says.
//     On a lane of equal reads a wave then issues an atomic only when its running minimum falls.
// Why the read before the atomic is safe: a word is written by atomicMin alone, so it only ever falls.  A stale
// value read before the atomic is therefore >= the word's value at any later time; skipping when step >= stale value
// skips only an atomicMin that could not have lowered the word, and when the test passes the atomicMin itself
// decides.  The word ends as the exact minimum over the class's counted pairs whatever the order of execution: the
// minimum of a group's steps stands for all of them, minima commute, every well is visited by exactly one lane of
// one workgroup, label and the coordinates were written before this launch began, and a root's label is a global id
// of a PF well of an added tile, so lab indexes cls and a same-tile root's offset is a well of the coordinate table.
__global__ void __launch_bounds__(kTdBlock) k_ls_min(const int *__restrict__ tile_idx, int64_t N,
                                                      const uint32_t *__restrict__ label,
                                                      const int2 *__restrict__ xy, unsigned long long radius2,
                                                      uint32_t steps, uint32_t salt, uint32_t *cls)
{
    const LaneRun run(tile_idx, N);
    uint32_t last_root = kInvalid, last_step = 0;                     // the same in every lane of a wave
    run.walk([&](bool has, int64_t w, size_t g64) {
        bool cand = false;
        uint32_t lab = kInvalid, s = 0;
        if (has) {
            lab = label[g64];
            if (lab != kInvalid && lab != (uint32_t)g64 && !ls_dropped(w, lab, run.base, N, xy, radius2)) {
                s = ls_step((uint32_t)g64, salt, steps);
                cand = s < cls[lab];
            }
        }
        wave_by_key(cand, lab, [&](uint32_t r0, unsigned long long group, bool first) {
            uint32_t m = (uint32_t)__shfl((int)s, __ffsll((long long)group) - 1);
            if (group & (group - 1)) {                                 // more lanes than the first
                unsigned long long low = group;                        // the lanes of the group that hold its smallest step
                m = 0;
                for (int bit = kLsStepBits - 1; bit >= 0; bit--) {
                    const unsigned long long zero = __ballot(((s >> bit) & 1u) == 0) & low;
                    if (zero)
                        low = zero;
                    else
                        m |= 1u << bit;
                }
            }
            if (r0 != last_root || m < last_step) {
                if (first)
                    atomicMin(&cls[r0], m);
                last_root = r0;
                last_step = m;
            }
        });
    });
}

// ---- tally ----------------------------------------------------------------------------------------
// The same grid, after k_ls_min on the same stream: every word of cls is final.  A counted well adds one to
// NewReads[its step]; a well with label = own id (a root, or a PF well in no class - never dropped) also adds one to
// NewDistinct[min(its word, its own step)].  Both are counted in the workgroup's LDS histogram [2][kLsSteps] (32-bit:
// a run adds at most kLaneRun to a bin); PF and Dropped are two ballots per trip, the same in every lane of the wave,
// summed in registers over the run as k_lg_tally sums Pairs.  At the end the workgroup adds what is not zero to its
// copy of the spread counters.
// No wave_by_key as in k_lg_tally: there the keys follow the data - a lane of equal reads puts every pair
// into one bin -, here the key is a hash of the well's id, whatever the reads are, and spreads a wave's 64 wells
// evenly over the S steps, so no bin is hot beyond what a small S makes of it (S = 1: the 64 adds of a wave queue on
// one LDS word; a lane's worth of that is still LDS traffic only).
// Why the result is exact and does not depend on the order of execution: every output is a sum of ones over wells,
// each well is visited by exactly one lane of one workgroup, integer adds commute and none can overflow; the step
// is a function of the id alone; the two launches are ordered by the stream.
__global__ void __launch_bounds__(kTdBlock) k_ls_tally(const int *__restrict__ tile_idx, int64_t N,
                                                        const uint32_t *__restrict__ label,
                                                        const int2 *__restrict__ xy, unsigned long long radius2,
                                                        uint32_t steps, uint32_t salt, const uint32_t *__restrict__ cls,
                                                        unsigned long long *cnt, unsigned long long *head)
{
    __shared__ uint32_t s_hist[2 * kLsSteps];                         // NewReads, NewDistinct
    __shared__ uint32_t s_head[kLsHead];                              // PF, Dropped
    if (threadIdx.x < 2 * kLsSteps)
        s_hist[threadIdx.x] = 0;
    if (threadIdx.x < kLsHead)
        s_head[threadIdx.x] = 0;
    __syncthreads();
    const LaneRun run(tile_idx, N);
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t n_pf = 0, n_dropped = 0;                                 // the same in every lane of a wave
    run.walk([&](bool has, int64_t w, size_t g64) {
        bool pf = false, dropped = false;
        if (has) {
            const uint32_t lab = label[g64];
            if (lab != kInvalid) {
                pf = true;
                const bool own = lab == (uint32_t)g64;
                dropped = !own && ls_dropped(w, lab, run.base, N, xy, radius2);
                if (!dropped) {
                    const uint32_t s = ls_step((uint32_t)g64, salt, steps);
                    atomicAdd(&s_hist[s], 1u);
                    if (own)
                        atomicAdd(&s_hist[kLsSteps + min(cls[g64], s)], 1u);
                }
            }
        }
        n_pf += (uint32_t)__popcll(__ballot(pf));
        n_dropped += (uint32_t)__popcll(__ballot(dropped));
    });
    if (lane == 0) {
        if (n_pf)
            atomicAdd(&s_head[0], n_pf);
        if (n_dropped)
            atomicAdd(&s_head[1], n_dropped);
    }
    __syncthreads();
    if (threadIdx.x < 2 * kLsSteps && s_hist[threadIdx.x])
        atomicAdd(spread_row(cnt, 0, 2 * kLsSteps) + threadIdx.x, (unsigned long long)s_hist[threadIdx.x]);
    if (threadIdx.x < kLsHead && s_head[threadIdx.x])
        atomicAdd(spread_row(head, 0, kLsHead) + threadIdx.x, (unsigned long long)s_head[threadIdx.x]);
}

}  // namespace

#ifndef WD_LANE_SATURATION_EMU                     // (tools/lane_saturation_emu.cpp: the kernels above on the CPU, a fiber per lane)
extern "C" {

int wd_lane_saturation_scratch(int64_t N, int max_tiles, int with_coords, size_t *bytes)
{
    if (N < 0 || max_tiles < 0 || !bytes)
        return WD_ERR_ARG;
    if (max_tiles > 65535)
        return WD_ERR_UNSUPPORTED;
    *bytes = ls_layout_of(N, max_tiles, with_coords != 0).bytes;
    return WD_OK;
}

int wd_lane_saturation(wd_lane_dups *ld, int steps, uint32_t seed, const int32_t *x, const int32_t *y, int64_t radius,
                       void *scratch_dev, size_t scratch_bytes, int64_t *head_row, int64_t *new_reads,
                       int64_t *new_distinct)
try {
    if (!ld || !head_row || !new_reads || !new_distinct)
        return WD_ERR_ARG;
    wd_ctx *ctx = ld->ctx;
    const int64_t N = ld->N;
    const int T = ld->max_tiles;
    const bool coords = x != nullptr;
    LanePass p(ld);
    if (const int rc = p.finished("lane saturation comes after a successful finish of the lane"))
        return rc;
    if (steps < 1 || steps > kLsSteps)
        return fail(ctx, WD_ERR_ARG, "lane saturation: 1.." + std::to_string(kLsSteps) + " steps, not " + std::to_string(steps));
    if (const int rc = lane_pass_radius(ctx, "lane saturation", radius))
        return rc;
    if ((x == nullptr) != (y == nullptr))
        return fail(ctx, WD_ERR_ARG, "lane saturation: x and y come together or not at all");
    if (radius > 0 && !coords)
        return fail(ctx, WD_ERR_ARG, "lane saturation: a radius needs the coordinates");
    const LsLayout lay = ls_layout_of(N, T, coords);
    if (const int rc = p.scratch(scratch_dev, scratch_bytes, lay.bytes, "scratch smaller than wd_lane_saturation_scratch",
                                 "lane saturation: the scratch must be in device memory"))
        return rc;
    std::vector<int2> h_xy;
    if (coords)
        if (const int rc = lane_pass_coords(ctx, "lane saturation", x, y, N, h_xy))
            return rc;
    memset(head_row, 0, kLsHead * sizeof(int64_t));
    memset(new_reads, 0, (size_t)steps * sizeof(int64_t));
    memset(new_distinct, 0, (size_t)steps * sizeof(int64_t));
    if (!p.start())
        return p.rc;
    uint8_t *sc = (uint8_t *)scratch_dev;
    uint32_t *cls = (uint32_t *)(sc + lay.cls);
    unsigned long long *cnt = (unsigned long long *)(sc + lay.cnt);
    unsigned long long *head = (unsigned long long *)(sc + lay.head);
    int *d_tidx = (int *)(sc + lay.tidx);
    const bool drop = coords && radius > 0;
    const int2 *d_xy = drop ? (const int2 *)(sc + lay.xy) : nullptr;
    const unsigned long long radius2 = drop ? (unsigned long long)radius * (unsigned long long)radius : 0;
    const uint32_t salt = seed * 0x9E3779B9u;
    const uint32_t *label = (const uint32_t *)(ld->ws + ld->lay.label);
    WD_HIP(ctx, hipMemsetAsync(cls, 0xFF, 4 * (size_t)T * (size_t)N, ctx->stream));
    if (drop)
        WD_HIP(ctx, hipMemcpyAsync(sc + lay.xy, h_xy.data(), (size_t)N * 8, hipMemcpyHostToDevice, ctx->stream));
    WD_HIP(ctx, hipMemsetAsync(sc + lay.cnt, 0, lay.tidx - lay.cnt, ctx->stream));
    if (const int rc = p.upload(d_tidx))
        return rc;
    hipLaunchKernelGGL(k_ls_min, p.grid, dim3(kTdBlock), 0, ctx->stream, d_tidx, N, label, d_xy, radius2, (uint32_t)steps, salt,
                       cls);
    WD_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_ls_tally, p.grid, dim3(kTdBlock), 0, ctx->stream, d_tidx, N, label, d_xy, radius2, (uint32_t)steps,
                       salt, (const uint32_t *)cls, cnt, head);
    WD_HIP(ctx, hipGetLastError());
    SpreadFetch f_c(cnt, 1, 2 * kLsSteps), f_h(head, 1, kLsHead);
    if (const int rc = spread_fetch(ctx, {&f_c, &f_h}))
        return rc;
    unsigned long long c[2 * kLsSteps], h[kLsHead];
    f_c.sum(0, c);
    f_h.sum(0, h);
    for (int j = 0; j < steps; j++) {
        new_reads[j] = (int64_t)c[j];
        new_distinct[j] = (int64_t)c[kLsSteps + j];
    }
    for (int f = 0; f < kLsHead; f++)
        head_row[f] = (int64_t)h[f];
    return WD_OK;
} WD_CATCH

}  // extern "C"

// What comes after this file in the unit is included from here, as lane_quality.inc includes this file: a lane's
// most frequent reads and their spread (include/welldup_lanetop.h), which uses nothing of this file.
#include "lane_top.inc"
#endif
