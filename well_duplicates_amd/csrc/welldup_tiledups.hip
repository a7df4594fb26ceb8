// welldup_tiledups.hip - read classes of every tile (include/welldup_tiledups.h): the PF wells of a tile
// grouped by their whole read, wherever on the tile they lie, and the share of each ring level in it.
//
// Per batch of tiles, one launch each (grid y = tile):
//   k_td_fingerprint  streams the L planes once: a lane folds four consecutive wells from dword loads,
//                     ten planes in flight, into a 64-bit fingerprint of the decoded codes per well
//   k_td_insert       one lane per PF well into the tile's open-addressing table (below); remembers the slot
//   k_td_resolve      label = the slot's representative; members counted at the representative
//   k_td_local        classes, wells in them, size bins, RingWells; the rings of a well in a class are walked
//                     and the level of every classmate met there is taken for both ends
//   k_td_levels       histogram of the first levels (the host accumulates it into Local)
// This unit reads the context (targets, stream) and keeps no state in it.  Its constants, the layout of the workspace and
// these kernels stand in tile_classes.inc (included after read_classes.inc), the host half of a call here.
// tile_near.inc (included at the end, after the near_core.inc it shares with lane_near.inc) builds the
// near-duplicate clusters of welldup_tilenear.h on these parts, lane_dups.inc (after it) the classes across all
// tiles of a lane of welldup_lanedups.h, lane_near.inc (after it) the near-duplicate clusters of a lane of
// welldup_lanenear.h, lane_pass.inc (after it) what the passes that follow a lane's finish share - the walk over a run
// of wells, the grouping of a wave by key, the start of a pass and the counters' way back -, lane_index.inc (after
// it) a lane's duplication per index read of welldup_laneindex.h,
// lane_mismatch.inc (after it) where a lane's duplicate copies differ of welldup_lanemismatch.h, lane_hops.inc (after
// it: it folds two keys with lane_mismatch.inc's lm_fold) which libraries they join of welldup_lanehops.h, lane_distance.inc
// (last) how far apart they lie of welldup_lanedistance.h: all of these work on the accumulator as lane_dups.inc laid
// it out.  lane_quality.inc, behind them, gives it a second packed array - the reported base qualities - and holds
// them against the copies: welldup_lanequality.h.  lane_saturation.inc, which lane_quality.inc includes at its
// end, reads the labels alone: the lane's distinct reads against its depth of welldup_lanesaturation.h.
// lane_top.inc, which lane_saturation.inc includes at its end, reads the labels, the members and the rows: the lane's
// most frequent reads and their spread of welldup_lanetop.h.  lane_gc.inc (after lane_distance.inc) reads the labels, the members
// and every row of the lane: its duplication against its reads' GC content of welldup_lanegc.h.  lane_adapter.inc (after
// it, with its piece loads) searches every row for the adapter: the duplication by insert length of
// welldup_laneadapter.h.  lane_consensus.inc (after
// it) gathers the members of every family and counts their calls against the family's vote: welldup_laneconsensus.h.
// lane_umi.inc (after it) groups the wells of every family by their UMI read, packed by lane_index.inc's kernel and
// gathered by lane_consensus.inc's: welldup_laneumi.h.  lane_keep.inc, which lane_top.inc includes at its end and
// which so comes after all of lane_quality.inc, reads the labels, the members and the quality rows: the best well of
// each family as a keep mask of welldup_lanekeep.h.
#include <memory>

#include "wd_ctx.h"
#include "wd_tiledups.h"
#include "welldup_tiledups.h"

#ifndef WD_UNIT_ID
#define WD_UNIT_ID "unknown"
#endif
namespace wd { const char *unit_id_tiledups() { return WD_UNIT_ID; } }      // hash of this unit's sources (wd_build_id)

#include "read_classes.inc"    // the encoding, the plane pass, the table, the compare loop, the grouped add, the counters

#include "tile_classes.inc"    // the unit's constants, the workspace layout, the kernels k_td_*

namespace {

bool on_device(const void *p)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeDevice || at.type == hipMemoryTypeManaged;
}

// ---- host: what the entry points of the unit share ------------------------------------------------------
// Every plane, filter and (if asked for) label pointer of a call: none null, planes and filters in device
// memory.  aligned4: every plane is 4-byte aligned.  prefix is "tile duplicates: " or "lane duplicates: ".
int check_tables(wd_ctx *ctx, const char *prefix, int n_tiles, int L, const uint8_t *const *planes,
                 const uint8_t *const *filter, uint32_t *const *labels, bool *aligned4)
{
    *aligned4 = true;
    for (size_t i = 0; i < (size_t)n_tiles * L; i++) {
        if (!planes[i])
            return fail(ctx, WD_ERR_ARG, "null plane pointer");
        *aligned4 = *aligned4 && ((uintptr_t)planes[i] & 3u) == 0;
    }
    for (int i = 0; i < n_tiles; i++) {
        if (!filter[i] || !on_device(filter[i]) || (L > 0 && !on_device(planes[(size_t)i * L])))
            return fail(ctx, WD_ERR_ARG, std::string(prefix) + "planes and filters must be in device memory");
        if (labels && !labels[i])
            return fail(ctx, WD_ERR_ARG, "null label pointer");
    }
    return WD_OK;
}

// What wd_tile_dups and wd_tile_near_dups ask before anything runs: every well a target, a plane per cycle,
// the limits, a workspace of need() bytes (asked once the limits hold; size_fn names the function that
// states them), tables, targets inside the tile.  Binds the device.
template <class Need>
int check_tile_call(wd_ctx *ctx, int n_tiles, int L, int64_t N, const uint8_t *const *planes,
                    const uint8_t *const *filter, const void *workspace, size_t workspace_bytes, Need &&need,
                    const char *size_fn)
{
    if (!ctx->has_targets)
        return fail(ctx, WD_ERR_STATE, "wd_set_targets has not been called");
    if ((int64_t)ctx->T != N || ctx->levels < 1)
        return fail(ctx, WD_ERR_ARG, "tile duplicates need every well as a target (T == N)");
    if (ctx->well_stride != 1)
        return fail(ctx, WD_ERR_UNSUPPORTED, "tile duplicates read a plane per cycle (well_stride 1)");
    if (N >= ((int64_t)1 << 31))
        return fail(ctx, WD_ERR_UNSUPPORTED, "tile duplicates: more than 2^31 - 1 wells");
    if (L > kMaxCycles)
        return fail(ctx, WD_ERR_UNSUPPORTED, "tile duplicates: more than 1024 cycles");
    if (n_tiles > 65535)
        return fail(ctx, WD_ERR_UNSUPPORTED, "tile duplicates: more than 65535 tiles in one call");
    if (n_tiles > 0 && (!workspace || workspace_bytes < need()))
        return fail(ctx, WD_ERR_ARG, std::string("workspace smaller than ") + size_fn);
    if (n_tiles > 0 && (!filter || (L > 0 && !planes)))
        return fail(ctx, WD_ERR_ARG, "null plane or filter table");
    if (ctx->T > 0 && n_tiles > 0 && (ctx->idx_min < 0 || ctx->idx_max >= N))
        return fail(ctx, WD_ERR_INDEX, "a target names a well outside the tile");
    return bind_device(ctx) ? WD_ERR_HIP : WD_OK;
}

// The pointer tables of a call into the workspace.  With d_lbl, the label table goes too (all null if labels is
// null), from h_lbl, which the caller keeps until it has synchronised the stream.
int upload_tables(wd_ctx *ctx, int n_tiles, int L, const uint8_t *const *planes, const uint8_t **d_planes,
                  const uint8_t *const *filter, const uint8_t **d_filt, uint32_t *const *labels = nullptr,
                  uint32_t **d_lbl = nullptr, std::vector<uint32_t *> *h_lbl = nullptr)
{
    if (L > 0)
        WD_HIP(ctx, hipMemcpyAsync(d_planes, planes, (size_t)n_tiles * L * sizeof(void *), hipMemcpyHostToDevice,
                                   ctx->stream));
    WD_HIP(ctx, hipMemcpyAsync(d_filt, filter, n_tiles * sizeof(void *), hipMemcpyHostToDevice, ctx->stream));
    if (d_lbl) {
        h_lbl->assign(n_tiles, nullptr);
        if (labels)
            std::copy(labels, labels + n_tiles, h_lbl->begin());
        WD_HIP(ctx, hipMemcpyAsync(d_lbl, h_lbl->data(), n_tiles * sizeof(void *), hipMemcpyHostToDevice, ctx->stream));
    }
    return WD_OK;
}

// counters and flags clear, every slot of the tables free
int clear_workspace(wd_ctx *ctx, const Layout &lay, const View &v, int n_tiles)
{
    WD_HIP(ctx, hipMemsetAsync(v.cnt, 0, lay.planes - lay.cnt, ctx->stream));
    WD_HIP(ctx, hipMemsetAsync(v.table, 0xFF, (size_t)n_tiles * lay.slots * 8, ctx->stream));
    return WD_OK;
}

// The end of a per-tile call: counters and flags come down, the centres are checked, the copies summed and
// the rows filled - [PF, Classes, InClasses, Redundant, (NearPairs if near,) Local[levels], RingWells[levels],
// bins].
int finish_tile_rows(wd_ctx *ctx, const View &v, int n_tiles, bool near, int64_t *out_rows)
{
    const int levels = ctx->levels;
    WD_HIP(ctx, hipGetLastError());
    std::vector<unsigned long long> h_cnt((size_t)n_tiles * kSpread * kCnt);
    uint32_t h_flags[4] = {0, 0, 0, 0};
    WD_HIP(ctx, hipMemcpyAsync(h_cnt.data(), v.cnt, h_cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                               ctx->stream));
    WD_HIP(ctx, hipMemcpyAsync(h_flags, v.flags, sizeof(h_flags), hipMemcpyDeviceToHost, ctx->stream));
    WD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_flags[kFlagCentres])
        return fail(ctx, WD_ERR_ARG, "tile duplicates need target t to be centred on well t");
    const size_t first = near ? 5 : 4, nrow = first + 2 * (size_t)levels + kBins;
    for (int i = 0; i < n_tiles; i++) {
        unsigned long long c[kCnt];
        sum_spread(h_cnt.data(), (size_t)i, kCnt, c);
        int64_t *o = out_rows + (size_t)i * nrow;
        o[0] = (int64_t)c[kCntPf];
        o[1] = (int64_t)c[kCntClasses];
        o[2] = (int64_t)c[kCntInClasses];
        o[3] = o[2] - o[1];
        if (near)
            o[4] = (int64_t)c[kCntNear];
        int64_t local = 0;
        for (int l = 0; l < levels; l++) {
            local += (int64_t)c[kCntFirst + l];
            o[first + l] = local;
            o[first + levels + l] = (int64_t)c[kCntRing + l];
        }
        for (int b = 0; b < kBins; b++)
            o[first + 2 * levels + b] = (int64_t)c[kCntBins + b];
    }
    return WD_OK;
}

}  // namespace

extern "C" {

int wd_tile_dups_workspace(int64_t N, int n_tiles, size_t *bytes)
{
    if (N < 0 || n_tiles < 0 || !bytes)
        return WD_ERR_ARG;
    *bytes = layout_of(N, n_tiles).bytes;
    return WD_OK;
}

int wd_tile_dups(wd_ctx *ctx, int n_tiles, int L, const uint8_t *const *planes, const uint8_t *const *filter,
                 int64_t N, void *workspace_dev, size_t workspace_bytes, int hash_bits, int64_t *out_rows,
                 uint32_t *const *labels_dev)
try {
    if (!ctx || !out_rows || n_tiles < 0 || N < 0 || L < 0 || hash_bits < 0 || hash_bits > 32)
        return WD_ERR_ARG;
    if (const int rc = check_tile_call(ctx, n_tiles, L, N, planes, filter, workspace_dev, workspace_bytes,
                                       [&] { return layout_of(N, n_tiles).bytes; }, "wd_tile_dups_workspace"))
        return rc;
    const Layout lay = layout_of(N, n_tiles);
    const int levels = ctx->levels;
    memset(out_rows, 0, (size_t)n_tiles * (4 + 2 * (size_t)levels + kBins) * sizeof(int64_t));
    if (n_tiles == 0 || N == 0)
        return WD_OK;
    bool aligned4;
    if (const int rc = check_tables(ctx, "tile duplicates: ", n_tiles, L, planes, filter, labels_dev, &aligned4))
        return rc;
    const View v(lay, workspace_dev);
    const unsigned long long fp_mask = hash_bits == 0 ? ~0ull : (1ull << hash_bits) - 1;
    if (const int rc = clear_workspace(ctx, lay, v, n_tiles))
        return rc;
    std::vector<uint32_t *> h_lbl;
    if (const int rc = upload_tables(ctx, n_tiles, L, planes, v.planes, filter, v.filt, labels_dev, v.lbl, &h_lbl))
        return rc;

    const unsigned wblocks = (unsigned)((N + kTdBlock - 1) / kTdBlock);
    const dim3 wgrid(wblocks, (unsigned)n_tiles), blk(kTdBlock);
    hipLaunchKernelGGL(k_td_check_centres, dim3(wblocks), blk, 0, ctx->stream, ctx->d_centre, ctx->T, v.flags);
    if (aligned4)
        hipLaunchKernelGGL(k_td_fingerprint<true>, dim3((unsigned)((N + 4 * kTdBlock - 1) / (4 * kTdBlock)), (unsigned)n_tiles),
                           blk, 0, ctx->stream, v.planes, L, N, v.fp, v.members);
    else
        hipLaunchKernelGGL(k_td_fingerprint<false>, wgrid, blk, 0, ctx->stream, v.planes, L, N, v.fp, v.members);
    hipLaunchKernelGGL(k_td_insert, wgrid, blk, 0, ctx->stream, v.planes, v.filt, L, N, v.fp, fp_mask, v.table, v.slot_mask,
                       v.label);
    hipLaunchKernelGGL(k_td_resolve, wgrid, blk, 0, ctx->stream, v.table, v.slot_mask, N, v.label, v.members, v.first,
                       labels_dev ? v.lbl : nullptr, v.cnt);
    hipLaunchKernelGGL(k_td_local, wgrid, blk, 0, ctx->stream, v.label, v.members, N, ctx->d_lvl_off, ctx->d_nbr, levels,
                       v.first, v.cnt);
    hipLaunchKernelGGL(k_td_levels, wgrid, blk, 0, ctx->stream, v.first, N, levels, v.cnt);
    return finish_tile_rows(ctx, v, n_tiles, false, out_rows);
} WD_CATCH

}  // extern "C"

#include "near_core.inc"      // what the two near-duplicate passes below share: the method, its kernels' bodies
#include "tile_near.inc"      // near-duplicate clusters (include/welldup_tilenear.h) on the parts above
#include "lane_dups.inc"      // read classes across the tiles of a lane (include/welldup_lanedups.h)
#include "lane_near.inc"      // near-duplicate clusters of a lane (include/welldup_lanenear.h) on all of the above
#include "lane_pass.inc"      // what the passes after a lane's finish share: the walk, the grouping, the host's steps
#include "lane_index.inc"     // a lane's classes split by index read (include/welldup_laneindex.h)
#include "lane_mismatch.inc"  // where a lane's duplicate copies differ (include/welldup_lanemismatch.h)
#include "lane_hops.inc"      // which libraries a lane's duplicate copies join (include/welldup_lanehops.h)
#include "lane_distance.inc"  // how far apart a lane's duplicate copies lie (include/welldup_lanedistance.h)
#include "lane_gc.inc"        // a lane's duplication against its reads' GC content (include/welldup_lanegc.h)
#include "lane_adapter.inc"   // a lane's duplication by insert length (include/welldup_laneadapter.h)
#include "lane_consensus.inc" // a lane's errors against its families' vote (include/welldup_laneconsensus.h)
#include "lane_umi.inc"       // a lane's duplicates split by molecular identifier (include/welldup_laneumi.h)
#include "lane_quality.inc"   // reported base quality against a lane's duplicate copies (include/welldup_lanequality.h)
