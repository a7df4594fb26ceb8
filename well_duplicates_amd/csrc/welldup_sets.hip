// welldup_sets.hip - duplicate sets of every tile (include/welldup_sets.h): the wells of a tile grouped by
// single linkage over the duplicate pairs the scan finds, when every well is a centre.
//
// The edges are the scan's own hit log (one wd_hit {tile, target, slot, dist} per duplicate, from every
// scan path: the dense chain, the queue kernel, the line walk, the generic Levenshtein kernel), so no
// compare kernel changes.  The scan is driven through the public entry points (wd_hitlog_enable,
// wd_count_tiles); this unit reads the context (wd_ctx.h) and keeps no state of its own in it.  Per batch of
// tiles, one launch each:
//   k_sets_init      parent[w] = w for PF wells, INVALID for the rest; first level touched = none
//   k_sets_edges     one lane per hit record: drop it unless both ends pass the filter and differ (a well that
//                    names itself is no pair), find its level from
//                    the target's lvl_off row, rewrite the record in place as {tile, a, b, level},
//                    atomicMin both ends' first level
//   k_sets_union     one launch per level, in increasing order: lock-free union-find over that level's edges
//   k_sets_compress  every well's root (= its label), InSets from the first levels
//   k_sets_count     members per root (memset first), k_sets_bins the set-size histogram and the labels
// The kernels, their constants and layouts and the fold of the counters into a sets row are csrc/dup_sets.inc; this
// file is the host side.
#include "wd_ctx.h"
#include "welldup_sets.h"

#ifndef WD_UNIT_ID
#define WD_UNIT_ID "unknown"
#endif
namespace wd { const char *unit_id_sets() { return WD_UNIT_ID; } }      // hash of this unit's sources (wd_build_id)

namespace {

using namespace wd;

#include "dup_sets.inc"                            // the device half and sets_fold_row (tools/dup_sets_emu.cpp runs it on the CPU)

// ---- host side --------------------------------------------------------------------------------
// Leaves the hit log disabled however the call ends.
struct HitlogOff {
    wd_ctx *ctx;
    ~HitlogOff() { (void)wd_hitlog_enable(ctx, 0); }
};

int64_t hit_total(wd_ctx *ctx)
{
    int64_t total = 0;
    if (wd_hitlog_fetch(ctx, nullptr, 0, &total) != WD_OK)
        return -1;
    return total;
}

int64_t dups_of(const int64_t *row, int levels)
{
    int64_t s = 0;
    for (int l = 0; l < levels; l++)
        s += row[1 + levels + l];
    return s;
}

// edges of the records in the hit log, then the union passes of every level
int process_edges(wd_ctx *ctx, int64_t n, int tile0, int n_tiles, int64_t N, uint8_t *ws, const Layout &lay)
{
    if (n <= 0)
        return WD_OK;
    const unsigned blocks = (unsigned)((n + kSetsBlock - 1) / kSetsBlock);
    int4 *rec = (int4 *)ctx->d_hits;
    uint32_t *parent = (uint32_t *)(ws + lay.parent);
    uint32_t *aux = (uint32_t *)(ws + lay.aux);
    unsigned long long *cnt = (unsigned long long *)(ws + lay.cnt);
    uint32_t *flags = (uint32_t *)(ws + lay.flags);
    hipLaunchKernelGGL(k_sets_edges, dim3(blocks), dim3(kSetsBlock), 0, ctx->stream, rec, n, tile0, n_tiles,
                       ctx->d_lvl_off, ctx->d_nbr, ctx->levels, N, parent, aux, flags);
    for (int l = 0; l < ctx->levels; l++)
        hipLaunchKernelGGL(k_sets_union, dim3(blocks), dim3(kSetsBlock), 0, ctx->stream, rec, n, l, N, parent, cnt);
    WD_HIP(ctx, hipGetLastError());
    return WD_OK;
}

bool on_device(const void *p)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

}  // namespace

extern "C" {

int wd_dup_sets_workspace(int64_t N, int n_tiles, size_t *bytes)
{
    if (N < 0 || n_tiles < 0 || !bytes)
        return WD_ERR_ARG;
    *bytes = layout_of(N, n_tiles).bytes;
    return WD_OK;
}

int wd_dup_sets(wd_ctx *ctx, int n_tiles, int L, int mode, int k, const uint8_t *const *planes,
                const uint8_t *const *filter, int64_t N, void *workspace_dev, size_t workspace_bytes, int64_t edge_cap,
                int64_t *out_tile, int64_t *out_sets, uint32_t *const *labels_dev, int64_t *edges_out)
try {
    if (!ctx || !out_tile || !out_sets || n_tiles < 0 || N < 0 || edge_cap < 0)
        return WD_ERR_ARG;
    if (!ctx->has_targets)
        return fail(ctx, WD_ERR_STATE, "wd_set_targets has not been called");
    const int levels = ctx->levels;
    if ((int64_t)ctx->T != N || levels < 1)
        return fail(ctx, WD_ERR_ARG, "duplicate sets need every well as a target (T == N)");
    if (N >= (int64_t)kInvalid)
        return fail(ctx, WD_ERR_UNSUPPORTED, "duplicate sets: more than 2^32 - 1 wells");
    const Layout lay = layout_of(N, n_tiles);
    if (n_tiles > 0 && (!workspace_dev || workspace_bytes < lay.bytes))
        return fail(ctx, WD_ERR_ARG, "workspace smaller than wd_dup_sets_workspace");
    if (n_tiles > 65535)
        return fail(ctx, WD_ERR_UNSUPPORTED, "duplicate sets: more than 65535 tiles in one call");
    if (n_tiles > 0 && !filter)
        return fail(ctx, WD_ERR_ARG, "null filter table");
    if (bind_device(ctx))
        return WD_ERR_HIP;
    HitlogOff off{ctx};
    if (edges_out)
        *edges_out = 0;
    if (n_tiles == 0 || N == 0) {
        int rc = wd_count_tiles(ctx, n_tiles, L, mode, k, planes, filter, N, out_tile, nullptr);
        if (rc)
            return rc;
        const size_t ns = 1 + 3 * (size_t)levels + kBins;
        memset(out_sets, 0, (size_t)n_tiles * ns * sizeof(int64_t));
        return WD_OK;
    }
    for (int i = 0; i < n_tiles; i++)
        if (!filter[i] || !on_device(filter[i]))
            return fail(ctx, WD_ERR_ARG, "duplicate sets: the filters must be in device memory");

    uint8_t *ws = (uint8_t *)workspace_dev;
    uint32_t *parent = (uint32_t *)(ws + lay.parent);
    uint32_t *aux = (uint32_t *)(ws + lay.aux);
    unsigned long long *cnt = (unsigned long long *)(ws + lay.cnt);
    uint32_t *flags = (uint32_t *)(ws + lay.flags);
    uint32_t **lbl = (uint32_t **)(ws + lay.lbl);
    const uint8_t **filt = (const uint8_t **)(ws + lay.filt);

    // targets must be every well, each its own target: centre[t] == t
    WD_HIP(ctx, hipMemsetAsync(ws + lay.cnt, 0, lay.lbl - lay.cnt, ctx->stream));
    hipLaunchKernelGGL(k_sets_check_centres, dim3((unsigned)((N + kSetsBlock - 1) / kSetsBlock)), dim3(kSetsBlock), 0,
                       ctx->stream, ctx->d_centre, ctx->T, flags);
    WD_HIP(ctx, hipGetLastError());
    uint32_t h_flags[2] = {0, 0};
    WD_HIP(ctx, hipMemcpyAsync(h_flags, flags, sizeof(h_flags), hipMemcpyDeviceToHost, ctx->stream));
    WD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_flags[kFlagCentres])
        return fail(ctx, WD_ERR_ARG, "duplicate sets need target t to be centred on well t");

    // 1. scan with the caller's edge capacity, or what the log holds already, or an eighth of the wells
    const int64_t wells = (int64_t)n_tiles * N;
    int64_t cap = edge_cap > 0 ? edge_cap : std::max<int64_t>({(int64_t)ctx->hit_alloc, wells / 8, 1024});
    if (int rc = wd_hitlog_enable(ctx, cap))
        return rc;
    if (int rc = wd_count_tiles(ctx, n_tiles, L, mode, k, planes, filter, N, out_tile, nullptr))
        return rc;
    const size_t ncnt = 1 + 5 * (size_t)levels;
    int64_t total = hit_total(ctx), dups = 0;
    for (int i = 0; i < n_tiles; i++)
        dups += dups_of(out_tile + (size_t)i * ncnt, levels);
    if (total != dups)
        return fail(ctx, WD_ERR_STATE, "hit log total " + std::to_string(total) + " != Dups " + std::to_string(dups));

    // the sets' own state (the scan did not touch it)
    std::vector<uint32_t *> h_lbl(n_tiles, nullptr);
    if (labels_dev)
        for (int i = 0; i < n_tiles; i++)
            h_lbl[i] = labels_dev[i];
    std::vector<const uint8_t *> h_filt(filter, filter + n_tiles);
    WD_HIP(ctx, hipMemcpyAsync(lbl, h_lbl.data(), n_tiles * sizeof(void *), hipMemcpyHostToDevice, ctx->stream));
    WD_HIP(ctx, hipMemcpyAsync(filt, h_filt.data(), n_tiles * sizeof(void *), hipMemcpyHostToDevice, ctx->stream));
    const dim3 wgrid((unsigned)((N + kSetsBlock - 1) / kSetsBlock), (unsigned)n_tiles);
    hipLaunchKernelGGL(k_sets_init, wgrid, dim3(kSetsBlock), 0, ctx->stream, filt, N, parent, aux, cnt);
    WD_HIP(ctx, hipGetLastError());

    int64_t processed = 0;
    if (total <= cap) {
        if (int rc = process_edges(ctx, total, 0, n_tiles, N, ws, lay))
            return rc;
        processed = total;
    } else {
        size_t free_b = 0, all_b = 0;
        WD_HIP(ctx, hipMemGetInfo(&free_b, &all_b));
        const double room = ((double)free_b + (double)ctx->hit_alloc * sizeof(wd_hit)) / 2;   // (the log's own buffer is freed first)
        if ((double)total * sizeof(wd_hit) <= room) {
            // 2. a sizing retry: the log grows to the total, the resident batch is scanned again
            if (int rc = wd_hitlog_enable(ctx, total))
                return rc;
            std::vector<int64_t> again((size_t)n_tiles * ncnt);
            if (int rc = wd_count_tiles(ctx, n_tiles, L, mode, k, planes, filter, N, again.data(), nullptr))
                return rc;
            if (hit_total(ctx) != total || memcmp(again.data(), out_tile, again.size() * sizeof(int64_t)) != 0)
                return fail(ctx, WD_ERR_STATE, "the second scan of the batch differs from the first");
            if (int rc = process_edges(ctx, total, 0, n_tiles, N, ws, lay))
                return rc;
            processed = total;
        } else {
            // 3. tile by tile (records carry tile 0, tile0 = i; no test reaches it on a 288 GB card: tools/dup_sets_emu.cpp
            // launches the kernels this way on the CPU, and nothing else exercises it)
            std::vector<int64_t> row(ncnt);
            for (int i = 0; i < n_tiles; i++) {
                const int64_t need = dups_of(out_tile + (size_t)i * ncnt, levels);
                WD_HIP(ctx, hipMemGetInfo(&free_b, &all_b));
                const double room_i = ((double)free_b + (double)ctx->hit_alloc * sizeof(wd_hit)) / 2;
                if ((double)need * sizeof(wd_hit) > room_i)
                    return fail(ctx, WD_ERR_NOMEM, "duplicate sets: the " + std::to_string(need) +
                                                       " duplicates of tile " + std::to_string(i) +
                                                       " do not fit in half the free device memory");
                if (need == 0)
                    continue;
                if (int rc = wd_hitlog_enable(ctx, need))
                    return rc;
                if (int rc = wd_count_tiles(ctx, 1, L, mode, k, planes ? planes + (size_t)i * L : nullptr, filter + i, N,
                                            row.data(), nullptr))
                    return rc;
                if (hit_total(ctx) != need || memcmp(row.data(), out_tile + (size_t)i * ncnt, ncnt * sizeof(int64_t)) != 0)
                    return fail(ctx, WD_ERR_STATE, "the scan of tile " + std::to_string(i) + " alone differs from the batch's");
                if (int rc = process_edges(ctx, need, i, n_tiles, N, ws, lay))
                    return rc;
                processed += need;
            }
        }
    }

    // finish: labels, InSets, set sizes
    hipLaunchKernelGGL(k_sets_compress, wgrid, dim3(kSetsBlock), 0, ctx->stream, parent, aux, N, levels, cnt);
    WD_HIP(ctx, hipMemsetAsync(aux, 0, (size_t)wells * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(k_sets_count, wgrid, dim3(kSetsBlock), 0, ctx->stream, parent, N, aux);
    hipLaunchKernelGGL(k_sets_bins, wgrid, dim3(kSetsBlock), 0, ctx->stream, parent, aux, N,
                       labels_dev ? lbl : nullptr, cnt);
    WD_HIP(ctx, hipGetLastError());
    std::vector<unsigned long long> h_cnt((size_t)n_tiles * kSpread * kCnt);
    WD_HIP(ctx, hipMemcpyAsync(h_cnt.data(), cnt, h_cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                               ctx->stream));
    WD_HIP(ctx, hipMemcpyAsync(h_flags, flags, sizeof(h_flags), hipMemcpyDeviceToHost, ctx->stream));
    WD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_flags[kFlagRecord])
        return fail(ctx, WD_ERR_STATE, "a hit record names a slot outside its target's rings");

    const size_t ns = 1 + 3 * (size_t)levels + kBins;
    for (int i = 0; i < n_tiles; i++)
        sets_fold_row(h_cnt.data(), i, levels, out_sets + (size_t)i * ns);
    if (edges_out)
        *edges_out = processed;
    return WD_OK;
} WD_CATCH

}  // extern "C"
