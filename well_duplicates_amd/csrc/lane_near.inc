// lane_near.inc - near-duplicate read clusters of a lane (include/welldup_lanenear.h): the PF wells of all tiles
// of a lane linked by Hamming distance <= K, single linkage.  Included at the end of welldup_tiledups.hip: the
// method, its kernels' bodies and the argument for its exactness stand in near_core.inc.  Here are the lane's
// space, its kernels and its host call; it also uses read_classes.inc (Fp, mix64, the spread counters) and
// lane_dups.inc (the accumulator, ld_equality, ld_count_rows).
//
// wd_lane_near_dups_finish, over the tiles that were added (grid y = tile):
//   ld_equality       the classes, as wd_lane_dups_finish; their representatives are the vertices.  The lane's table
//                     and aux, dead from there on, take a segment's buckets and {next, rank} of every well's chain
//   then for every segment s = K..0: k_ln_bucket, k_ln_bound, and the host refuses a lane over budget
//   then per segment s = 0..K (s > 0: k_ln_bucket again, and k_ln_bound if the segment has a long slot):
//   k_ln_scatter, k_ln_pairs, k_ln_pairs_long
//   k_ln_compress, k_ln_members, then k_ld_classes, k_ld_span_count, k_ld_span_sum on zeroed counters (by label only)
// The lane's space: a vertex id is the well's global id g = tile index * N + well and every array is the lane's,
// so a bucket's members lie on any tiles.  Particular to it:
// - Bounds before any label changes.  All K + 1 bounds are taken first, nothing quadratic run and no label
//   touched, so a refused call leaves the equality results valid; going down leaves segment 0's buckets in the
//   table for the pairs.
// - No stored fingerprints.  A segment's fingerprint is folded from the packed row whenever it is asked for, so
//   a pair is tested on the distance first: nearly every candidate fails it, and only a pair within K pays for
//   the fingerprints.
// - Tiles from different wd_lane_dups_add calls: nothing changes.  Bucketing happens entirely inside this call,
//   from the packed rows and the resolved labels, neither of which records when a tile came.
#include "welldup_lanenear.h"

namespace {

static_assert(WD_LANENEAR_MAX_K == kTnMaxK, "the lane's and the tile's largest distance differ");

// the scratch (include/welldup_lanenear.h states the arithmetic)
struct LnLayout {
    size_t bound, near, list, bytes;
};

LnLayout ln_layout_of(int64_t N, int max_tiles)
{
    LnLayout l;
    l.bound = 0;                                                       // per segment {candidate pairs, long members}
    l.near = align256(l.bound + (size_t)(kTnMaxK + 1) * 2 * 8);
    l.list = align256(l.near + (size_t)kSpread * 8);
    l.bytes = align256(l.list + (size_t)N * (size_t)max_tiles * 4);
    return l;
}

// Fingerprint of segment s of nseg of a packed row: its words with the codes of other segments masked out (a
// segment's ends fall inside words), so equal segments give equal fingerprints.
__device__ inline uint32_t ln_seg_fp(const uint32_t *__restrict__ row, int L, int nseg, int s)
{
    const int c0 = seg_begin(L, nseg, s), c1 = seg_begin(L, nseg, s + 1);
    Fp g;
    for (int k = c0 / kFpCycles; k * kFpCycles < c1; k++) {
        const int lo = max(c0 - k * kFpCycles, 0), hi = min(c1 - k * kFpCycles, kFpCycles);
        g.fold(row[k] & ((1u << (3 * hi)) - 1u) & ~((1u << (3 * lo)) - 1u));
    }
    return g.a ^ (g.b * 0x9E3779B1u);
}

// Mismatching cycles of two packed rows, counted no further than the piece in which they pass k: XOR, the three
// bits of a code folded to one, popcount.  kLdCmpWords words of both rows are loaded before the first is looked
// at - as 16-byte pieces where a row is a whole number of them (151 cycles: 64 bytes, rows 256-byte aligned).
__device__ inline int ln_diff(uint32_t x, uint32_t y)
{
    const uint32_t d = x ^ y;
    return __popc((d | (d >> 1) | (d >> 2)) & 0x09249249u);
}

__device__ inline int rows_hamming_upto(const uint32_t *__restrict__ rows, int words, uint32_t a, uint32_t b, int k)
{
    const uint32_t *x = rows + (size_t)a * words, *y = rows + (size_t)b * words;
    int d = 0, i = 0;
    if ((words & 3) == 0) {
        for (; i + kLdCmpWords <= words; i += kLdCmpWords) {
            const uint4 p0 = *(const uint4 *)(x + i), p1 = *(const uint4 *)(x + i + 4);
            const uint4 q0 = *(const uint4 *)(y + i), q1 = *(const uint4 *)(y + i + 4);
            d += ln_diff(p0.x, q0.x) + ln_diff(p0.y, q0.y) + ln_diff(p0.z, q0.z) + ln_diff(p0.w, q0.w) +
                 ln_diff(p1.x, q1.x) + ln_diff(p1.y, q1.y) + ln_diff(p1.z, q1.z) + ln_diff(p1.w, q1.w);
            if (d > k)
                return d;
        }
        for (; i < words; i += 4) {
            const uint4 p = *(const uint4 *)(x + i), q = *(const uint4 *)(y + i);
            d += ln_diff(p.x, q.x) + ln_diff(p.y, q.y) + ln_diff(p.z, q.z) + ln_diff(p.w, q.w);
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
            d += ln_diff(p[j], q[j]);
        if (d > k)
            return d;
    }
    for (; i < words; i++)
        d += ln_diff(x[i], y[i]);
    return d;
}

// The lane's space, for the tile of blockIdx.y (max_tiles * N < 2^32 - 1).  link[2 g] = next, link[2 g + 1] = rank,
// in the bytes of aux: the kernels hand the bodies link and link + 1.  A kernel fills what its body asks for and
// leaves the rest zero: bound slot_mask alone; bucket and scatter tile_idx .. nseg; pairs all but labels_out;
// pairs_long, which never asks for id(), slot_mask .. cnt; compress tile_idx and N; members those and labels_out.
struct LnSpace {
    using slot_t = unsigned long long;
    static constexpr bool kDistanceFirst = true;
    static constexpr bool kChainFirst = true;
    const int *tile_idx;
    int64_t N;
    unsigned long long slot_mask;
    uint32_t fmask;
    const uint32_t *rows;
    int words, L, nseg;
    unsigned long long *cnt;
    uint32_t *const *labels_out;

    __device__ uint32_t id(int64_t w) const { return (uint32_t)((size_t)tile_idx[blockIdx.y] * (size_t)N + (size_t)w); }
    __device__ size_t at(uint32_t id) const { return id; }
    __device__ size_t link(uint32_t id) const { return 2 * (size_t)id; }
    __device__ size_t slot_base() const { return 0; }
    __device__ size_t aux_at() const { return 0; }
    __device__ unsigned long long *near() const { return spread_row(cnt, 0, 1); }
    __device__ uint32_t seg_fp(uint32_t id, int seg) const { return ln_seg_fp(rows + (size_t)id * words, L, nseg, seg); }
    __device__ const uint32_t *reads() const { return rows; }
    __device__ int distance_upto(const uint32_t *r, uint32_t a, uint32_t b, int k) const
    {
        return rows_hamming_upto(r, words, a, b, k);
    }
    __device__ void clear_more(size_t) const {}
    __device__ void label_out(int64_t w, uint32_t lab) const
    {
        const int ti = tile_idx[blockIdx.y];
        if (labels_out && labels_out[ti])
            labels_out[ti][w] = lab;
    }
};

// The slots are the bytes of the lane's table; the grids are near_core.inc's, y over the tiles added.
__global__ void __launch_bounds__(kTdBlock) k_ln_bucket(const int *__restrict__ tile_idx, int64_t N, int L, int nseg,
                                                         int seg, bool by_label, const uint32_t *__restrict__ label,
                                                         const uint32_t *__restrict__ rows, int words, uint32_t fmask,
                                                         unsigned long long slot_mask, uint32_t *slots,
                                                         uint32_t *__restrict__ link)
{
    near_bucket(LnSpace{tile_idx, N, slot_mask, fmask, rows, words, L, nseg}, seg, by_label, label, slots, link, link + 1);
}

__global__ void __launch_bounds__(kTdBlock) k_ln_bound(uint32_t *__restrict__ slots, unsigned long long slot_mask,
                                                        unsigned long long *aux)
{
    near_bound(LnSpace{nullptr, 0, slot_mask}, slots, aux);
}

__global__ void __launch_bounds__(kTdBlock) k_ln_scatter(const int *__restrict__ tile_idx, int64_t N, int L, int nseg,
                                                          int seg, const uint32_t *__restrict__ rows, int words,
                                                          uint32_t fmask, unsigned long long slot_mask,
                                                          const uint32_t *__restrict__ slots,
                                                          const uint32_t *__restrict__ link, uint32_t *__restrict__ list)
{
    near_scatter(LnSpace{tile_idx, N, slot_mask, fmask, rows, words, L, nseg}, seg, link, link + 1, slots, list);
}

__global__ void __launch_bounds__(kTdBlock) k_ln_pairs(const int *__restrict__ tile_idx, int64_t N, int L, int k, int seg,
                                                        const uint32_t *__restrict__ rows, int words, uint32_t fmask,
                                                        unsigned long long slot_mask, const uint32_t *__restrict__ slots,
                                                        const uint32_t *__restrict__ link, uint32_t *label,
                                                        unsigned long long *near)
{
    near_pairs(LnSpace{tile_idx, N, slot_mask, fmask, rows, words, L, k + 1, near}, k, seg, slots, link, label);
}

__global__ void __launch_bounds__(kTdBlock) k_ln_pairs_long(int L, int k, int seg, const uint32_t *__restrict__ rows,
                                                             int words, uint32_t fmask, unsigned long long slot_mask,
                                                             const uint32_t *__restrict__ slots,
                                                             const uint32_t *__restrict__ list,
                                                             const unsigned long long *__restrict__ aux, uint32_t *label,
                                                             unsigned long long *near)
{
    near_pairs_long(LnSpace{nullptr, 0, slot_mask, fmask, rows, words, L, k + 1, near}, k, seg, slots, list, aux, label);
}

__global__ void __launch_bounds__(kTdBlock) k_ln_compress(const int *__restrict__ tile_idx, int64_t N, uint32_t *label,
                                                           uint32_t *__restrict__ members)
{
    near_compress(LnSpace{tile_idx, N}, label, members);
}

__global__ void __launch_bounds__(kTdBlock) k_ln_members(const int *__restrict__ tile_idx, int64_t N,
                                                          const uint32_t *__restrict__ label, uint32_t *members,
                                                          uint32_t *const *__restrict__ labels_out)
{
    LnSpace sp{tile_idx, N};
    sp.labels_out = labels_out;
    near_members(sp, label, members);
}

}  // namespace

#ifndef WD_TILEDUPS_EMU                            // (tools/read_classes_emu.cpp, tools/near_emu.cpp: the kernels above on the CPU, a fiber per lane)
extern "C" {

int wd_lane_near_dups_scratch(int64_t N, int max_tiles, int L, int k, size_t *bytes)
{
    size_t ws = 0;
    if (const int rc = wd_lane_dups_workspace(N, max_tiles, L, &ws))
        return rc;
    if (k < 0 || k > kTnMaxK || !bytes)
        return WD_ERR_ARG;
    *bytes = k == 0 ? 0 : ln_layout_of(N, max_tiles).bytes;
    return WD_OK;
}

int wd_lane_near_dups_finish(wd_lane_dups *ld, int k, void *scratch_dev, size_t scratch_bytes, int64_t pair_budget,
                             int64_t *lane_row, int64_t *tile_rows, uint32_t *const *labels_dev,
                             int64_t *near_lane_row, int64_t *near_tile_rows, uint32_t *const *near_labels_dev)
try {
    if (ld)
        ld->mol = nullptr;                                             // (the molecule part does not outlive a call of a finish)
    if (!ld || !lane_row || !tile_rows || !near_lane_row || !near_tile_rows)
        return WD_ERR_ARG;
    wd_ctx *ctx = ld->ctx;
    const int64_t N = ld->N;
    const int T = ld->max_tiles, L = ld->L;
    if (ld->finished)
        return fail(ctx, WD_ERR_ARG, "lane duplicates: finish is called once");
    if (k < 0 || k > kTnMaxK)
        return fail(ctx, WD_ERR_ARG, "lane near-duplicates: the distance is 0.." + std::to_string(kTnMaxK));
    if (L < k + 1)
        return fail(ctx, WD_ERR_ARG, "lane near-duplicates: fewer cycles than segments");
    if (pair_budget < 0)
        return fail(ctx, WD_ERR_ARG, "lane near-duplicates: negative pair budget");
    const size_t wells = (size_t)N * (size_t)T;
    const LnLayout nl = ln_layout_of(N, T);
    if (k > 0 && wells > 0 && (!scratch_dev || scratch_bytes < nl.bytes))
        return fail(ctx, WD_ERR_ARG, "scratch smaller than wd_lane_near_dups_scratch");
    if (k > 0 && wells > 0 && !on_device(scratch_dev))
        return fail(ctx, WD_ERR_ARG, "lane near-duplicates: the scratch must be in device memory");
    if (const int rc = ld_check_labels(ld, labels_dev))
        return rc;
    if (const int rc = ld_check_labels(ld, near_labels_dev))
        return rc;

    if (const int rc = ld_equality(ld, lane_row, tile_rows, labels_dev))
        return rc;
    const std::vector<int> tiles = ld_tiles_added(ld);
    if (k == 0 || wells == 0 || tiles.empty()) {                       // the classes, NearPairs = 0
        ld->finished = true;
        near_row(lane_row, 6, WD_LANEDUPS_LANE_COLS, 0, near_lane_row);
        std::copy(tile_rows, tile_rows + (size_t)T * WD_LANEDUPS_TILE_COLS, near_tile_rows);
        if (wells > 0) {
            if (const int rc = ld_copy_labels(ld, near_labels_dev, true))
                return rc;
            WD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        return WD_OK;
    }
    const unsigned long long budget = near_budget(pair_budget, wells);      // the per-tile rule at lane scale

    const LdLayout &lay = ld->lay;
    uint8_t *ws = ld->ws, *sc = (uint8_t *)scratch_dev;
    int *d_tidx = (int *)(ws + lay.tidx);
    uint32_t **d_lbl = (uint32_t **)(ws + lay.lbl);
    uint32_t *slots = (uint32_t *)(ws + lay.table);                    // the table's bytes, now that it is resolved
    uint32_t *link = (uint32_t *)(ws + lay.aux);                       // the slot words' bytes
    const uint32_t *rows = (const uint32_t *)(ws + lay.rows);
    uint32_t *label = (uint32_t *)(ws + lay.label);
    uint32_t *members = (uint32_t *)(ws + lay.members);
    unsigned long long *aux = (unsigned long long *)(sc + nl.bound);
    unsigned long long *near = (unsigned long long *)(sc + nl.near);
    uint32_t *list = (uint32_t *)(sc + nl.list);
    const unsigned long long slot_mask = lay.slots - 1;
    // (a read's fingerprint is masked to hash_bits bits; a segment's has 32)
    const uint32_t fmask = (uint32_t)std::min<unsigned long long>(ld->fp_mask, 0xFFFFFFFFull);
    const int nseg = k + 1, words = lay.words;
    const dim3 wgrid((unsigned)((N + kTdBlock - 1) / kTdBlock), (unsigned)tiles.size()), blk(kTdBlock);
    const dim3 sgrid((unsigned)((lay.slots + kTnBoundSlots - 1) / kTnBoundSlots));

    WD_HIP(ctx, hipMemcpyAsync(d_tidx, tiles.data(), tiles.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    WD_HIP(ctx, hipMemsetAsync(sc, 0, nl.list, ctx->stream));
    // the bounds of all segments, the last one first: segment 0's buckets stay for the pairs
    for (int seg = nseg - 1; seg >= 0; seg--) {
        WD_HIP(ctx, hipMemsetAsync(slots, 0xFF, lay.slots * 8, ctx->stream));
        hipLaunchKernelGGL(k_ln_bucket, wgrid, blk, 0, ctx->stream, d_tidx, N, L, nseg, seg, true, label, rows, words, fmask,
                           slot_mask, slots, link);
        hipLaunchKernelGGL(k_ln_bound, sgrid, blk, 0, ctx->stream, slots, slot_mask, aux + 2 * seg);
    }
    WD_HIP(ctx, hipGetLastError());
    unsigned long long h_aux[2 * (kTnMaxK + 1)];
    WD_HIP(ctx, hipMemcpyAsync(h_aux, aux, sizeof(h_aux), hipMemcpyDeviceToHost, ctx->stream));
    WD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int seg = 0; seg < nseg; seg++)
        if (h_aux[2 * seg] > budget)
            return fail(ctx, WD_ERR_UNSUPPORTED, near_refusal("lane near-duplicates: ", L, nseg, seg, h_aux[2 * seg], budget));

    ld->finished = true;                                               // from here on the labels change
    for (int seg = 0; seg < nseg; seg++) {
        unsigned long long *aux_s = aux + 2 * seg;
        const unsigned long long longest = h_aux[2 * seg + 1];         // (the buckets are the same as in the pass above)
        if (seg > 0) {
            WD_HIP(ctx, hipMemsetAsync(slots, 0xFF, lay.slots * 8, ctx->stream));
            hipLaunchKernelGGL(k_ln_bucket, wgrid, blk, 0, ctx->stream, d_tidx, N, L, nseg, seg, false, label, rows, words,
                               fmask, slot_mask, slots, link);
            if (longest > 0) {                                         // the ranges of the long slots, once more
                WD_HIP(ctx, hipMemsetAsync(aux_s, 0, 16, ctx->stream));
                hipLaunchKernelGGL(k_ln_bound, sgrid, blk, 0, ctx->stream, slots, slot_mask, aux_s);
            }
        }
        if (longest > 0)
            hipLaunchKernelGGL(k_ln_scatter, wgrid, blk, 0, ctx->stream, d_tidx, N, L, nseg, seg, rows, words, fmask, slot_mask,
                               slots, link, list);
        hipLaunchKernelGGL(k_ln_pairs, wgrid, blk, 0, ctx->stream, d_tidx, N, L, k, seg, rows, words, fmask, slot_mask, slots,
                           link, label, near);
        if (longest > 0)
            hipLaunchKernelGGL(k_ln_pairs_long, dim3((unsigned)((longest + kTdBlock / kWave - 1) / (kTdBlock / kWave))), blk, 0,
                               ctx->stream, L, k, seg, rows, words, fmask, slot_mask, slots, list, aux_s, label, near);
    }
    if (near_labels_dev) {
        if (const int rc = ld_copy_labels(ld, near_labels_dev, false))
            return rc;
        WD_HIP(ctx, hipMemcpyAsync(d_lbl, near_labels_dev, T * sizeof(void *), hipMemcpyHostToDevice, ctx->stream));
    }
    hipLaunchKernelGGL(k_ln_compress, wgrid, blk, 0, ctx->stream, d_tidx, N, label, members);
    hipLaunchKernelGGL(k_ln_members, wgrid, blk, 0, ctx->stream, d_tidx, N, label, members,
                       near_labels_dev ? d_lbl : nullptr);
    WD_HIP(ctx, hipGetLastError());
    // the rows of the clusters: the counters start again from zero, PF per tile carries over from the classes
    WD_HIP(ctx, hipMemsetAsync(ws + lay.cnt_t, 0, lay.planes - lay.cnt_t, ctx->stream));
    unsigned long long h_near[kSpread];
    WD_HIP(ctx, hipMemcpyAsync(h_near, near, sizeof(h_near), hipMemcpyDeviceToHost, ctx->stream));
    int64_t cluster_row[WD_LANEDUPS_LANE_COLS];
    if (const int rc = ld_count_rows(ld, tiles, cluster_row, near_tile_rows))
        return rc;
    for (int t = 0; t < T; t++)
        near_tile_rows[(size_t)t * WD_LANEDUPS_TILE_COLS] = tile_rows[(size_t)t * WD_LANEDUPS_TILE_COLS];
    cluster_row[0] = lane_row[0];
    unsigned long long near_pairs = 0;
    sum_spread(h_near, 0, 1, &near_pairs);
    near_row(cluster_row, 6, WD_LANEDUPS_LANE_COLS, (int64_t)near_pairs, near_lane_row);
    return WD_OK;
} WD_CATCH

}  // extern "C"
#endif
