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
#include "wd_ctx.h"
#include "welldup_sets.h"

#ifndef WD_UNIT_ID
#define WD_UNIT_ID "unknown"
#endif
namespace wd { const char *unit_id_sets() { return WD_UNIT_ID; } }      // hash of this unit's sources (wd_build_id)

namespace {

using namespace wd;

constexpr uint32_t kInvalid = WD_INVALID_TARGET;   // parent of a non-PF well
constexpr uint32_t kNoLevel = 0xFFFFFFFFu;         // first level of a well no edge touches
constexpr int kBins = WD_DUPSET_SIZE_BINS;
constexpr int kSetsBlock = 256;

// per-tile counters in the workspace, [n_tiles][kSpread][kCnt] uint64: a workgroup adds its sums to copy
// blockIdx.x % kSpread (the host adds the copies up).  With one copy per tile, the ~17 000 workgroups of a
// 4.3 M-well tile queue up on the same few addresses: 0.8 ms per 16 tiles for each kernel that counts
// (rocprofv3 kernel trace), where the bytes it moves take about 0.1 ms.
constexpr int kSpread = 64;
constexpr int kCntInSets = 0;                      // wells whose first level is l (histogram)
constexpr int kCntHooks = kCntInSets + kMaxLevels; // successful hooks at level l
constexpr int kCntBins = kCntHooks + kMaxLevels;   // sets of size 2..8, >= 9 (outermost level)
constexpr int kCntPf = kCntBins + kBins;           // PF wells
constexpr int kCnt = kCntPf + 8;                   // (padded to a multiple of 8)

// workspace layout: parent [n_tiles][N] uint32 | first level / member count [n_tiles][N] uint32 |
// counters | flags | label pointer table | filter pointer table
struct Layout {
    size_t parent, aux, cnt, flags, lbl, filt, bytes;
};

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

Layout layout_of(int64_t N, int n_tiles)
{
    Layout l;
    const size_t wells = (size_t)N * (size_t)n_tiles;
    l.parent = 0;
    l.aux = align256(l.parent + wells * 4);
    l.cnt = align256(l.aux + wells * 4);
    l.flags = align256(l.cnt + (size_t)n_tiles * kSpread * kCnt * 8);
    l.lbl = align256(l.flags + 16);
    l.filt = align256(l.lbl + (size_t)n_tiles * sizeof(void *));
    l.bytes = align256(l.filt + (size_t)n_tiles * sizeof(void *));
    return l;
}

// the copy of tile `tile`'s counters this workgroup adds to
__device__ inline unsigned long long *cnt_row(unsigned long long *cnt, int tile)
{
    return cnt + ((size_t)tile * kSpread + blockIdx.x % kSpread) * kCnt;
}

// flags[0]: a centre is not its own target index; flags[1]: a hit record the targets cannot place
constexpr int kFlagCentres = 0, kFlagRecord = 1;

// ---- parent pointers -------------------------------------------------------------------------
// Memory model (MI355X): the per-XCD L2s are not coherent with each other and one CU's L1 is never
// refreshed by another CU's stores, so inside a kernel every parent pointer is read with an agent-scope
// relaxed atomic load (served by L2, not a possibly stale L1 line), roots are hooked with an agent-scope
// CAS, and path shortcuts are agent-scope relaxed atomic stores.  Nothing needs ordering beyond that:
//   - every value a parent pointer ever holds is an ancestor of the well (a hook adds a root above a
//     root, a shortcut points further up the same path), and pointers only go from a larger index to a
//     smaller one, so the forest stays acyclic and every walk ends;
//   - a stale read therefore yields an ancestor, or a "root" that has since been hooked: the CAS, which
//     expects parent[r] == r, fails on such a root and returns its parent, and the union goes on from
//     there.  Each successful CAS hooks a root a under b < a, and b's tree cannot contain a (its paths only
//     descend in index from b), so it merges two distinct trees: the count of successful CASes of
//     the levels <= l is the number of merges, Redundant[l], whatever order the edges run in;
//   - hooks point from the larger root to the smaller, so a root is the smallest index of its tree: the
//     label comes out with no extra work.
// Kernel boundaries order the passes (levels, then compression) as stream-ordered launches.
__device__ inline uint32_t load_parent(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x, splitting the path on the way (each visited pointer is moved to its grandparent)
__device__ inline uint32_t find_split(uint32_t *par, uint32_t x)
{
    uint32_t y = load_parent(par + x);
    while (y != x) {
        const uint32_t z = load_parent(par + y);
        if (z == y)
            return y;
        __hip_atomic_store(par + x, z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // z: an ancestor of x
        x = y;
        y = z;
    }
    return x;
}

// root of x, read-only (the compression pass: only well x's own lane writes parent[x] there)
__device__ inline uint32_t find_ro(const uint32_t *par, uint32_t x)
{
    uint32_t y = load_parent(par + x);
    while (y != x) {
        x = y;
        y = load_parent(par + x);
    }
    return x;
}

// true if this call merged two trees
__device__ inline bool unite(uint32_t *par, uint32_t a, uint32_t b)
{
    a = find_split(par, a);
    b = find_split(par, b);
    while (a != b) {
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        uint32_t expect = a;                     // hook the larger root under the smaller
        if (__hip_atomic_compare_exchange_strong(par + a, &expect, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return true;
        a = find_split(par, expect);             // a was hooked meanwhile: go on from its parent
        b = find_split(par, b);
    }
    return false;
}

// ---- kernels ----------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSetsBlock) k_sets_check_centres(const int32_t *__restrict__ centre, int T,
                                                                     uint32_t *flags)
{
    const int t = blockIdx.x * kSetsBlock + threadIdx.x;
    if (t < T && centre[t] != t)
        atomicOr(flags + kFlagCentres, 1u);
}

// grid (wells / 256, n_tiles)
__global__ void __launch_bounds__(kSetsBlock) k_sets_init(const uint8_t *const *__restrict__ filt, int64_t N,
                                                            uint32_t *__restrict__ parent, uint32_t *__restrict__ first,
                                                            unsigned long long *cnt)
{
    __shared__ uint32_t s_pf;
    if (threadIdx.x == 0)
        s_pf = 0;
    __syncthreads();
    const int tile = blockIdx.y;
    const int64_t w = (int64_t)blockIdx.x * kSetsBlock + threadIdx.x;
    if (w < N) {
        const bool pf = filt[tile][w] & 1u;                              // bcl_direct_reader.py:246
        const size_t i = (size_t)tile * N + w;
        parent[i] = pf ? (uint32_t)w : kInvalid;
        first[i] = kNoLevel;
        const unsigned long long b = __ballot(pf);
        if ((threadIdx.x & (kWave - 1)) == 0 && b)
            atomicAdd(&s_pf, (uint32_t)__popcll(b));
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_pf)
        atomicAdd(cnt_row(cnt, tile) + kCntPf, (unsigned long long)s_pf);
}

// one lane per hit record; records are rewritten in place as {tile, a, b, level} (level -1: dropped)
__global__ void __launch_bounds__(kSetsBlock) k_sets_edges(int4 *__restrict__ rec, int64_t n, int tile0, int n_tiles,
                                                             const int32_t *__restrict__ lvl_off,
                                                             const int32_t *__restrict__ nbr, int levels, int64_t N,
                                                             const uint32_t *__restrict__ parent, uint32_t *first,
                                                             uint32_t *flags)
{
    const int64_t i = (int64_t)blockIdx.x * kSetsBlock + threadIdx.x;
    if (i >= n)
        return;
    const int4 h = rec[i];                       // wd_hit {tile, target, slot, dist}
    const int tile = h.x + tile0;
    const int a = h.y;                           // target index == centre well (checked)
    const int slot = h.z;
    int lev = -1, b = -1;
    if (tile >= 0 && tile < n_tiles && a >= 0 && a < N) {
        const int32_t *o = lvl_off + (size_t)a * (levels + 1);
        for (int l = 0; l < levels; l++)
            if (slot >= o[l] && slot < o[l + 1]) {
                lev = l;
                break;
            }
        if (lev >= 0)
            b = nbr[slot];
    }
    if (lev < 0 || b < 0 || b >= N) {
        atomicOr(flags + kFlagRecord, 1u);
        rec[i] = make_int4(tile, a, b, -1);
        return;
    }
    const size_t base = (size_t)tile * N;
    // non-PF wells belong to no set (the scan records a duplicate for a PF centre whatever its neighbour's filter)
    if (parent[base + a] == kInvalid || parent[base + b] == kInvalid) {
        rec[i] = make_int4(tile, a, b, -1);
        return;
    }
    // a well that names itself is no pair: a set has at least two wells (the scan counts the record all the same)
    if (a == b) {
        rec[i] = make_int4(tile, a, b, -1);
        return;
    }
    rec[i] = make_int4(tile, a, b, lev);
    atomicMin(first + base + a, (uint32_t)lev);
    atomicMin(first + base + b, (uint32_t)lev);
}

// one pass per level, in increasing level order, over that level's edges
__global__ void __launch_bounds__(kSetsBlock) k_sets_union(const int4 *__restrict__ rec, int64_t n, int lev, int64_t N,
                                                             uint32_t *parent, unsigned long long *cnt)
{
    __shared__ uint32_t s_hooks;
    __shared__ int s_tile;
    const int64_t b0 = (int64_t)blockIdx.x * kSetsBlock;
    if (threadIdx.x == 0) {
        s_hooks = 0;
        s_tile = rec[b0].x;                      // records of one tile mostly come together: count those in LDS
    }
    __syncthreads();
    const int64_t i = b0 + threadIdx.x;
    if (i < n) {
        const int4 e = rec[i];
        if (e.w == lev && unite(parent + (size_t)e.x * N, (uint32_t)e.y, (uint32_t)e.z)) {
            if (e.x == s_tile)
                atomicAdd(&s_hooks, 1u);
            else
                atomicAdd(cnt_row(cnt, e.x) + kCntHooks + lev, 1ull);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_hooks)
        atomicAdd(cnt_row(cnt, s_tile) + kCntHooks + lev, (unsigned long long)s_hooks);
}

// every well's root; InSets histogram from the first levels.  grid (wells / 256, n_tiles)
__global__ void __launch_bounds__(kSetsBlock) k_sets_compress(uint32_t *parent, const uint32_t *__restrict__ first,
                                                                int64_t N, int levels, unsigned long long *cnt)
{
    __shared__ uint32_t s_hist[kMaxLevels];
    if (threadIdx.x < kMaxLevels)
        s_hist[threadIdx.x] = 0;
    __syncthreads();
    const int tile = blockIdx.y;
    const int64_t w = (int64_t)blockIdx.x * kSetsBlock + threadIdx.x;
    if (w < N) {
        uint32_t *par = parent + (size_t)tile * N;
        const uint32_t p = load_parent(par + w);
        if (p != kInvalid && p != (uint32_t)w) {
            const uint32_t r = find_ro(par, p);
            if (r != p)
                __hip_atomic_store(par + w, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const uint32_t f = first[(size_t)tile * N + w];
        if (f < (uint32_t)levels)
            atomicAdd(&s_hist[f], 1u);
    }
    __syncthreads();
    if (threadIdx.x < levels && s_hist[threadIdx.x])
        atomicAdd(cnt_row(cnt, tile) + kCntInSets + threadIdx.x, (unsigned long long)s_hist[threadIdx.x]);
}

// members of every set other than its root, counted at the root (the aux array zeroed before)
__global__ void __launch_bounds__(kSetsBlock) k_sets_count(const uint32_t *__restrict__ parent, int64_t N,
                                                             uint32_t *members)
{
    const int tile = blockIdx.y;
    const int64_t w = (int64_t)blockIdx.x * kSetsBlock + threadIdx.x;
    if (w >= N)
        return;
    const size_t base = (size_t)tile * N;
    const uint32_t p = parent[base + w];
    if (p != kInvalid && p != (uint32_t)w)
        atomicAdd(members + base + p, 1u);
}

// set-size histogram at the roots, labels out
__global__ void __launch_bounds__(kSetsBlock) k_sets_bins(const uint32_t *__restrict__ parent,
                                                            const uint32_t *__restrict__ members, int64_t N,
                                                            uint32_t *const *__restrict__ labels, unsigned long long *cnt)
{
    __shared__ uint32_t s_bins[kBins];
    if (threadIdx.x < kBins)
        s_bins[threadIdx.x] = 0;
    __syncthreads();
    const int tile = blockIdx.y;
    const int64_t w = (int64_t)blockIdx.x * kSetsBlock + threadIdx.x;
    if (w < N) {
        const size_t i = (size_t)tile * N + w;
        const uint32_t p = parent[i];
        if (labels)
            labels[tile][w] = p;
        if (p == (uint32_t)w) {
            const uint32_t m = members[i];
            if (m > 0)
                atomicAdd(&s_bins[min(m + 1u, (uint32_t)(kBins + 1)) - 2u], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < kBins && s_bins[threadIdx.x])
        atomicAdd(cnt_row(cnt, tile) + kCntBins + threadIdx.x, (unsigned long long)s_bins[threadIdx.x]);
}

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
            // 3. tile by tile
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
    for (int i = 0; i < n_tiles; i++) {
        unsigned long long c[kCnt] = {};
        for (int r = 0; r < kSpread; r++)
            for (int f = 0; f < kCnt; f++)
                c[f] += h_cnt[((size_t)i * kSpread + r) * kCnt + f];
        int64_t *o = out_sets + (size_t)i * ns;
        o[0] = (int64_t)c[kCntPf];
        int64_t in_sets = 0, redundant = 0;
        for (int l = 0; l < levels; l++) {
            in_sets += (int64_t)c[kCntInSets + l];
            redundant += (int64_t)c[kCntHooks + l];
            o[1 + l] = in_sets - redundant;                  // Sets
            o[1 + levels + l] = in_sets;                     // InSets
            o[1 + 2 * levels + l] = redundant;               // Redundant
        }
        for (int b = 0; b < kBins; b++)
            o[1 + 3 * levels + b] = (int64_t)c[kCntBins + b];
    }
    if (edges_out)
        *edges_out = processed;
    return WD_OK;
} WD_CATCH

}  // extern "C"
