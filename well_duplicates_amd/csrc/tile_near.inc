// tile_near.inc - near-duplicate read clusters of every tile (include/welldup_tilenear.h): PF wells linked by
// Hamming distance <= K anywhere on the tile, single linkage.  Included by welldup_tiledups.hip after
// near_core.inc: the method, its kernels' bodies and the argument for its exactness stand there.  Here are the
// tile's space, its kernels and its host call; it also uses read_classes.inc (plane_pass, compare_wells), that
// unit's k_td_insert / k_td_resolve / k_td_local / k_td_levels, its counter layout and its host helpers.
//
// Per batch of tiles (grid y = tile):
//   k_tn_fingerprint  the pass of k_td_fingerprint cut at the segments' ends: their fingerprints and the read's
//   k_td_insert, k_td_resolve   equality classes; their representatives are the vertices
//   then per segment s = 0..K: k_tn_bucket, k_tn_bound (the host refuses a tile over budget here), k_tn_scatter,
//   k_tn_pairs, k_tn_pairs_long
//   k_tn_compress, k_tn_members, then k_td_local, k_td_levels as for the classes, on cluster labels
// The tile's space: a vertex id is the well's index on its tile and every array is [n_tiles][N], so a tile's
// unions never leave it; the segment fingerprints are stored (k_tn_fingerprint has the planes in hand anyway), and
// a pair is tested on them before sixteen planes of both reads are loaded for the distance.
#include "welldup_tilenear.h"

namespace {

// what the near path needs beyond the layout of wd_tile_dups: per segment and tile {bound, long members}
// uint64, and the segment fingerprints [K + 1][n_tiles * N] uint32.  Inside the shared layout: next and rank
// live in the 64-bit fingerprints (dead after k_td_insert), the slots' heads and member counts in the table (dead after
// k_td_resolve), the members of long slots in the first-level array (written again by k_tn_compress).
struct NearLayout {
    Layout base;
    size_t aux, segfp, bytes;
};

NearLayout near_layout_of(int64_t N, int n_tiles, int k)
{
    NearLayout l;
    l.base = layout_of(N, n_tiles);
    l.aux = l.base.bytes;
    l.segfp = align256(l.aux + (size_t)(k + 1) * n_tiles * 2 * 8);
    l.bytes = align256(l.segfp + (size_t)(k + 1) * n_tiles * (size_t)N * 4);
    return l;
}

// grid as k_td_fingerprint: its pass, once per segment.  segfp[s][tile * N + w]; also clears the members array.
template <bool VEC4>
__global__ void __launch_bounds__(kTdBlock) k_tn_fingerprint(const uint8_t *const *__restrict__ planes, int L, int nseg,
                                                              int64_t N, size_t seg_stride,
                                                              unsigned long long *__restrict__ fp,
                                                              uint32_t *__restrict__ segfp, uint32_t *__restrict__ members)
{
    constexpr int V = VEC4 ? 4 : 1;
    const int tile = blockIdx.y;
    const int64_t w0 = ((int64_t)blockIdx.x * kTdBlock + threadIdx.x) * V;
    if (w0 >= N)
        return;
    const uint8_t *const *pl = planes + (size_t)tile * L;
    fp += (size_t)tile * N;
    segfp += (size_t)tile * N;
    members += (size_t)tile * N;
    if (VEC4 && w0 + 4 <= N) {
        Fp whole[4];
        for (int s = 0; s < nseg; s++) {
            const int end = seg_begin(L, nseg, s + 1);       // (the 30-bit word is flushed at the segment's end)
            Fp g[4];
            plane_pass<true>(pl, seg_begin(L, nseg, s), end, w0, [&](int, const uint32_t(&acc)[4]) {
#pragma unroll
                for (int q = 0; q < 4; q++)
                    g[q].fold(acc[q]);
            });
#pragma unroll
            for (int q = 0; q < 4; q++) {
                segfp[s * seg_stride + w0 + q] = g[q].a ^ (g[q].b * 0x9E3779B1u);
                whole[q].fold(g[q].a);
                whole[q].fold(g[q].b);
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            fp[w0 + q] = whole[q].value();
            members[w0 + q] = 0;
        }
        return;
    }
    for (int64_t w = w0; w < N && w < w0 + V; w++) {         // unaligned planes, and the last wells of a tile
        Fp whole;
        for (int s = 0; s < nseg; s++) {
            const int end = seg_begin(L, nseg, s + 1);
            Fp g;
            plane_pass<false>(pl, seg_begin(L, nseg, s), end, w, [&](int, const uint32_t(&acc)[1]) { g.fold(acc[0]); });
            segfp[s * seg_stride + w] = g.a ^ (g.b * 0x9E3779B1u);
            whole.fold(g.a);
            whole.fold(g.b);
        }
        fp[w] = whole.value();
        members[w] = 0;
    }
}

// The tile's space, for the tile of blockIdx.y.  segfp[seg * seg_stride + id]: a kernel that gets one segment's row
// alone says stride 0.  A kernel fills what its body asks for and leaves the rest zero: bound slot_mask alone; bucket
// and scatter N .. segfp; pairs and pairs_long N .. cnt; compress N and first; members N and labels_out.
struct TnSpace {
    using slot_t = uint32_t;
    static constexpr bool kDistanceFirst = false;
    static constexpr bool kChainFirst = false;
    int64_t N;
    uint32_t slot_mask, fmask;
    const uint32_t *segfp;
    size_t seg_stride;
    const uint8_t *const *planes;
    int L;
    unsigned long long *cnt;
    uint32_t *first;                               // the first levels, cleared for k_td_local
    uint32_t *const *labels_out;

    __device__ uint32_t id(int64_t w) const { return (uint32_t)w; }
    __device__ size_t at(uint32_t id) const { return (size_t)blockIdx.y * N + id; }
    __device__ size_t link(uint32_t id) const { return at(id); }
    __device__ size_t slot_base() const { return (size_t)blockIdx.y * ((size_t)slot_mask + 1); }
    __device__ size_t aux_at() const { return 2 * (size_t)blockIdx.y; }
    __device__ unsigned long long *near() const { return cnt_row(cnt, blockIdx.y) + kCntNear; }
    __device__ uint32_t seg_fp(uint32_t id, int seg) const { return segfp[seg * seg_stride + at(id)]; }
    __device__ const uint8_t *const *reads() const { return planes + (size_t)blockIdx.y * L; }
    __device__ int distance_upto(const uint8_t *const *pl, uint32_t a, uint32_t b, int k) const
    {
        return hamming_upto(pl, L, a, b, k);
    }
    __device__ void clear_more(size_t i) const { first[i] = kNoLevel; }
    __device__ void label_out(int64_t w, uint32_t lab) const
    {
        if (labels_out)
            labels_out[blockIdx.y][w] = lab;
    }
};

// The slots are the bytes of the table of k_td_insert, [n_tiles][slots]; the grids are near_core.inc's.
__global__ void __launch_bounds__(kTdBlock) k_tn_bucket(const uint32_t *__restrict__ label, int seg, int64_t N,
                                                         const uint32_t *__restrict__ segfp, uint32_t fmask,
                                                         uint32_t slot_mask, uint32_t *slots,
                                                         uint32_t *__restrict__ next, uint32_t *__restrict__ rank)
{
    near_bucket(TnSpace{N, slot_mask, fmask, segfp}, seg, seg == 0, label, slots, next, rank);
}

__global__ void __launch_bounds__(kTdBlock) k_tn_bound(uint32_t *__restrict__ slots, uint32_t slot_mask,
                                                        unsigned long long *aux)
{
    near_bound(TnSpace{0, slot_mask}, slots, aux);
}

__global__ void __launch_bounds__(kTdBlock) k_tn_scatter(const uint32_t *__restrict__ next, int64_t N,
                                                          const uint32_t *__restrict__ segfp, uint32_t fmask,
                                                          uint32_t slot_mask, const uint32_t *__restrict__ slots,
                                                          const uint32_t *__restrict__ rank, uint32_t *__restrict__ list)
{
    near_scatter(TnSpace{N, slot_mask, fmask, segfp}, 0, next, rank, slots, list);
}

__global__ void __launch_bounds__(kTdBlock) k_tn_pairs(const uint8_t *const *__restrict__ planes, int L, int k, int seg,
                                                        int64_t N, const uint32_t *__restrict__ segfp0, size_t seg_stride,
                                                        uint32_t fmask, uint32_t slot_mask,
                                                        const uint32_t *__restrict__ slots,
                                                        const uint32_t *__restrict__ next, uint32_t *label,
                                                        unsigned long long *cnt)
{
    near_pairs(TnSpace{N, slot_mask, fmask, segfp0, seg_stride, planes, L, cnt}, k, seg, slots, next, label);
}

__global__ void __launch_bounds__(kTdBlock) k_tn_pairs_long(const uint8_t *const *__restrict__ planes, int L, int k,
                                                             int seg, int64_t N, const uint32_t *__restrict__ segfp0,
                                                             size_t seg_stride, uint32_t fmask, uint32_t slot_mask,
                                                             const uint32_t *__restrict__ slots,
                                                             const uint32_t *__restrict__ list,
                                                             const unsigned long long *__restrict__ aux, uint32_t *label,
                                                             unsigned long long *cnt)
{
    near_pairs_long(TnSpace{N, slot_mask, fmask, segfp0, seg_stride, planes, L, cnt}, k, seg, slots, list, aux, label);
}

__global__ void __launch_bounds__(kTdBlock) k_tn_compress(uint32_t *label, int64_t N, uint32_t *__restrict__ members,
                                                           uint32_t *__restrict__ first)
{
    TnSpace sp{N};
    sp.first = first;
    near_compress(sp, label, members);
}

__global__ void __launch_bounds__(kTdBlock) k_tn_members(const uint32_t *__restrict__ label, int64_t N, uint32_t *members,
                                                          uint32_t *const *__restrict__ labels_out)
{
    TnSpace sp{N};
    sp.labels_out = labels_out;
    near_members(sp, label, members);
}

}  // namespace

#ifndef WD_TILEDUPS_EMU                            // (tools/read_classes_emu.cpp, tools/near_emu.cpp: the kernels above on the CPU, a fiber per lane)
extern "C" {

int wd_tile_near_dups_workspace(int64_t N, int n_tiles, int k, size_t *bytes)
{
    if (N < 0 || n_tiles < 0 || k < 0 || k > kTnMaxK || !bytes)
        return WD_ERR_ARG;
    *bytes = k == 0 ? layout_of(N, n_tiles).bytes : near_layout_of(N, n_tiles, k).bytes;
    return WD_OK;
}

int wd_tile_near_dups(wd_ctx *ctx, int n_tiles, int L, const uint8_t *const *planes, const uint8_t *const *filter,
                      int64_t N, int k, void *workspace_dev, size_t workspace_bytes, int hash_bits, int64_t pair_budget,
                      int64_t *out_rows, uint32_t *const *labels_dev)
try {
    if (!ctx || !out_rows || n_tiles < 0 || N < 0 || L < 0 || hash_bits < 0 || hash_bits > 32 || k < 0 ||
        k > kTnMaxK || L < k + 1 || pair_budget < 0)
        return WD_ERR_ARG;
    const int levels = ctx->levels;
    const size_t nrow_eq = 4 + 2 * (size_t)levels + kBins, nrow = nrow_eq + 1;
    if (k == 0) {                                                      // the classes, NearPairs = 0
        std::vector<int64_t> eq((size_t)n_tiles * nrow_eq);
        const int rc = wd_tile_dups(ctx, n_tiles, L, planes, filter, N, workspace_dev, workspace_bytes, hash_bits,
                                    eq.data(), labels_dev);
        if (rc != WD_OK)
            return rc;
        for (int i = 0; i < n_tiles; i++)
            near_row(eq.data() + (size_t)i * nrow_eq, 4, nrow_eq, 0, out_rows + (size_t)i * nrow);
        return WD_OK;
    }
    if (const int rc = check_tile_call(ctx, n_tiles, L, N, planes, filter, workspace_dev, workspace_bytes,
                                       [&] { return near_layout_of(N, n_tiles, k).bytes; }, "wd_tile_near_dups_workspace"))
        return rc;
    const NearLayout nl = near_layout_of(N, n_tiles, k);
    const Layout &lay = nl.base;
    memset(out_rows, 0, (size_t)n_tiles * nrow * sizeof(int64_t));
    if (n_tiles == 0 || N == 0)
        return WD_OK;
    bool aligned4;
    if (const int rc = check_tables(ctx, "tile duplicates: ", n_tiles, L, planes, filter, labels_dev, &aligned4))
        return rc;
    const unsigned long long budget = near_budget(pair_budget, (unsigned long long)N);

    const View v(lay, workspace_dev);
    unsigned long long *aux = (unsigned long long *)((uint8_t *)workspace_dev + nl.aux);
    uint32_t *segfp = (uint32_t *)((uint8_t *)workspace_dev + nl.segfp);
    const size_t wells = (size_t)n_tiles * N, all_slots = (size_t)n_tiles * lay.slots;
    uint32_t *slots = (uint32_t *)v.table;                             // the table's bytes, once it is resolved
    uint32_t *next = (uint32_t *)v.fp, *rank = next + wells;           // the fingerprints' bytes, once inserted
    uint32_t *list = v.first;
    const uint32_t slot_mask = v.slot_mask;
    const unsigned long long fp_mask = hash_bits == 0 ? ~0ull : (1ull << hash_bits) - 1;
    const uint32_t fmask = hash_bits == 0 || hash_bits == 32 ? ~0u : (1u << hash_bits) - 1;
    const int nseg = k + 1;

    if (const int rc = clear_workspace(ctx, lay, v, n_tiles))
        return rc;
    WD_HIP(ctx, hipMemsetAsync(aux, 0, (size_t)nseg * n_tiles * 2 * 8, ctx->stream));
    std::vector<uint32_t *> h_lbl;
    if (const int rc = upload_tables(ctx, n_tiles, L, planes, v.planes, filter, v.filt, labels_dev, v.lbl, &h_lbl))
        return rc;

    const unsigned wblocks = (unsigned)((N + kTdBlock - 1) / kTdBlock);
    const dim3 wgrid(wblocks, (unsigned)n_tiles), blk(kTdBlock);
    const dim3 sgrid((unsigned)((lay.slots + kTnBoundSlots - 1) / kTnBoundSlots), (unsigned)n_tiles);
    hipLaunchKernelGGL(k_td_check_centres, dim3(wblocks), blk, 0, ctx->stream, ctx->d_centre, ctx->T, v.flags);
    if (aligned4)
        hipLaunchKernelGGL(k_tn_fingerprint<true>, dim3((unsigned)((N + 4 * kTdBlock - 1) / (4 * kTdBlock)), (unsigned)n_tiles),
                           blk, 0, ctx->stream, v.planes, L, nseg, N, wells, v.fp, segfp, v.members);
    else
        hipLaunchKernelGGL(k_tn_fingerprint<false>, wgrid, blk, 0, ctx->stream, v.planes, L, nseg, N, wells, v.fp, segfp,
                           v.members);
    hipLaunchKernelGGL(k_td_insert, wgrid, blk, 0, ctx->stream, v.planes, v.filt, L, N, v.fp, fp_mask, v.table, slot_mask,
                       v.label);
    hipLaunchKernelGGL(k_td_resolve, wgrid, blk, 0, ctx->stream, v.table, slot_mask, N, v.label, v.members, v.first,
                       (uint32_t *const *)nullptr, v.cnt);
    std::vector<unsigned long long> h_aux((size_t)n_tiles * 2);
    for (int seg = 0; seg < nseg; seg++) {
        unsigned long long *aux_s = aux + (size_t)seg * n_tiles * 2;
        const uint32_t *segfp_s = segfp + (size_t)seg * wells;
        WD_HIP(ctx, hipMemsetAsync(slots, 0xFF, all_slots * 8, ctx->stream));
        hipLaunchKernelGGL(k_tn_bucket, wgrid, blk, 0, ctx->stream, v.label, seg, N, segfp_s, fmask, slot_mask, slots, next,
                           rank);
        hipLaunchKernelGGL(k_tn_bound, sgrid, blk, 0, ctx->stream, slots, slot_mask, aux_s);
        WD_HIP(ctx, hipGetLastError());
        WD_HIP(ctx, hipMemcpyAsync(h_aux.data(), aux_s, h_aux.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        WD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        unsigned long long longest = 0;
        for (int i = 0; i < n_tiles; i++) {
            if (h_aux[2 * i] > budget)
                return fail(ctx, WD_ERR_UNSUPPORTED,
                            near_refusal("tile near-duplicates: tile " + std::to_string(i) + ", ", L, nseg, seg, h_aux[2 * i],
                                         budget));
            longest = std::max(longest, h_aux[2 * i + 1]);
        }
        if (longest > 0)
            hipLaunchKernelGGL(k_tn_scatter, wgrid, blk, 0, ctx->stream, next, N, segfp_s, fmask, slot_mask, slots, rank,
                               list);
        hipLaunchKernelGGL(k_tn_pairs, wgrid, blk, 0, ctx->stream, v.planes, L, k, seg, N, segfp, wells, fmask, slot_mask,
                           slots, next, v.label, v.cnt);
        if (longest > 0)
            hipLaunchKernelGGL(k_tn_pairs_long,
                               dim3((unsigned)((longest + kTdBlock / kWave - 1) / (kTdBlock / kWave)), (unsigned)n_tiles),
                               blk, 0, ctx->stream, v.planes, L, k, seg, N, segfp, wells, fmask, slot_mask, slots, list, aux_s,
                               v.label, v.cnt);
    }
    hipLaunchKernelGGL(k_tn_compress, wgrid, blk, 0, ctx->stream, v.label, N, v.members, v.first);
    hipLaunchKernelGGL(k_tn_members, wgrid, blk, 0, ctx->stream, v.label, N, v.members, labels_dev ? v.lbl : nullptr);
    hipLaunchKernelGGL(k_td_local, wgrid, blk, 0, ctx->stream, v.label, v.members, N, ctx->d_lvl_off, ctx->d_nbr, levels,
                       v.first, v.cnt);
    hipLaunchKernelGGL(k_td_levels, wgrid, blk, 0, ctx->stream, v.first, N, levels, v.cnt);
    return finish_tile_rows(ctx, v, n_tiles, true, out_rows);
} WD_CATCH

}  // extern "C"
#endif
