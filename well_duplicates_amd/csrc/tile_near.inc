// tile_near.inc - near-duplicate read clusters of every tile (include/welldup_tilenear.h): PF wells linked by
// Hamming distance <= K anywhere on the tile, single linkage.  Included at the end of welldup_tiledups.hip:
// it uses read_classes.inc (plane_pass, compare_wells, wave_grouped), that unit's k_td_insert / k_td_resolve /
// k_td_local / k_td_levels, its counter layout and its host helpers.
//
// Per batch of tiles (grid y = tile):
//   k_tn_fingerprint  the pass of k_td_fingerprint, cut at K + 1 segment boundaries: a 32-bit fingerprint per
//                     segment and well, and the 64-bit fingerprint of the whole read folded from them
//   k_td_insert, k_td_resolve   equality classes; only their representatives are vertices below, and the label
//                     array (label[w] <= w, a representative its own label) is the union-find's parent array
//   then per segment s = 0..K, over the representatives:
//   k_tn_bucket       rank = members[slot]++, next[w] = exchange(head[slot], w): a chain and its length per slot
//   k_tn_bound        sum over slots of c (c - 1) / 2 = the pair steps the segment would cost; the host refuses
//                     the call before anything quadratic runs if it exceeds the budget.  A slot of more than
//                     kTnLong representatives gets a range of the member array instead of its chain
//   k_tn_scatter      members of long slots into their range, at their rank
//   k_tn_pairs        a lane per representative of a short slot walks the chain behind itself
//   k_tn_pairs_long   a wave per member of a long slot, its lanes over the members of lower rank
//   k_tn_compress, k_tn_members   label = root, members recounted at the roots
//   k_td_local, k_td_levels       as for the classes, on cluster labels
// A pair is compared at the first segment whose fingerprints agree (pigeonhole: within K mismatches one of
// K + 1 segments is equal, so its fingerprints are), on the reads, once.
#include "welldup_tilenear.h"

namespace {

constexpr int kTnMaxK = 3;
constexpr uint32_t kTnLong = 32;                   // chains up to this length are one lane's walk
constexpr uint32_t kNil = 0xFFFFFFFFu;             // end of a chain

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

__host__ __device__ inline int seg_begin(int L, int nseg, int s) { return (int)((long long)L * s / nseg); }

__device__ inline uint32_t seg_slot(uint32_t f, uint32_t slot_mask) { return (uint32_t)mix64(f) & slot_mask; }

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

// A slot of a segment's table is two uint32 side by side (one cache line for both atomics of k_tn_bucket):
// [0] the head of its chain, [1] all ones minus the number of its members - so one fill with 0xFF empties the
// table.  [n_tiles][slots] of them: the bytes of the table of k_td_insert.
__device__ inline uint32_t slot_count(const uint32_t *slots, size_t i) { return ~slots[2 * i + 1]; }

// grid (ceil(N / 256), n_tiles): the representatives into the chains of segment `seg`
__global__ void __launch_bounds__(kTdBlock) k_tn_bucket(const uint32_t *__restrict__ label, int seg, int64_t N,
                                                         const uint32_t *__restrict__ segfp, uint32_t fmask,
                                                         uint32_t slot_mask, uint32_t *slots,
                                                         uint32_t *__restrict__ next, uint32_t *__restrict__ rank)
{
    const int tile = blockIdx.y;
    const int64_t w64 = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    if (w64 >= N)
        return;
    const uint32_t w = (uint32_t)w64;
    const size_t base = (size_t)tile * N, sbase = (size_t)tile * ((size_t)slot_mask + 1);
    // Vertices are the representatives of the classes: label[w] == w before the first union (a non-PF
    // well's label is kInvalid).  The unions move labels, so segment 0 marks every other well with
    // next[w] == w, which no chain produces, and the later segments go by that mark.
    if (seg == 0 ? label[base + w] != w : next[base + w] == w) {
        next[base + w] = w;
        return;
    }
    const uint32_t s = seg_slot(segfp[base + w] & fmask, slot_mask);
    uint32_t *slot = slots + 2 * (sbase + s);
    rank[base + w] = ~__hip_atomic_fetch_sub(slot + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    next[base + w] = __hip_atomic_exchange(slot, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (ceil(slots / kTnBoundSlots), n_tiles), a lane two slots per load.  aux[tile] = {sum of c (c - 1) / 2,
// members of long slots}; the head of a long slot becomes the start of its range in the member array (its
// chain is not walked).
constexpr uint32_t kTnBoundSlots = 4096;           // (a workgroup per 256 slots was all launch: 8.1 ms per 16 tiles)

__global__ void __launch_bounds__(kTdBlock) k_tn_bound(uint32_t *__restrict__ slots, uint32_t slot_mask,
                                                        unsigned long long *aux)
{
    __shared__ unsigned long long s_sum;
    if (threadIdx.x == 0)
        s_sum = 0;
    __syncthreads();
    const int tile = blockIdx.y;
    const size_t sbase = (size_t)tile * ((size_t)slot_mask + 1);
    unsigned long long sum = 0;
    for (uint32_t i = 2 * threadIdx.x; i < kTnBoundSlots; i += 2 * kTdBlock) {
        const size_t s = (size_t)blockIdx.x * kTnBoundSlots + i;      // (slots are a multiple of 64: s + 1 is one too)
        if (s > slot_mask)
            break;
        const uint4 v = *(const uint4 *)(slots + 2 * (sbase + s));
        const unsigned long long c[2] = {~v.y, ~v.w};
#pragma unroll
        for (int j = 0; j < 2; j++)
            if (c[j] > 1) {
                sum += c[j] * (c[j] - 1) / 2;
                if (c[j] > kTnLong)
                    slots[2 * (sbase + s + j)] = (uint32_t)atomicAdd(aux + 2 * tile + 1, c[j]);
            }
    }
    if (sum)
        atomicAdd(&s_sum, sum);
    __syncthreads();
    if (threadIdx.x == 0 && s_sum)
        atomicAdd(aux + 2 * tile, s_sum);
}

// grid (ceil(N / 256), n_tiles): members of long slots into list[head[slot] + rank]
__global__ void __launch_bounds__(kTdBlock) k_tn_scatter(const uint32_t *__restrict__ next, int64_t N,
                                                          const uint32_t *__restrict__ segfp, uint32_t fmask,
                                                          uint32_t slot_mask, const uint32_t *__restrict__ slots,
                                                          const uint32_t *__restrict__ rank, uint32_t *__restrict__ list)
{
    const int tile = blockIdx.y;
    const int64_t w64 = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    if (w64 >= N)
        return;
    const uint32_t w = (uint32_t)w64;
    const size_t base = (size_t)tile * N, sbase = (size_t)tile * ((size_t)slot_mask + 1);
    if (next[base + w] == w)                                          // no vertex
        return;
    const uint32_t s = seg_slot(segfp[base + w] & fmask, slot_mask);
    if (slot_count(slots, sbase + s) > kTnLong)
        list[base + slots[2 * (sbase + s)] + rank[base + w]] = w;            // (ranges add up to <= N per tile)
}

// Union-find on the label array, as the parent pointers of welldup_sets.hip (the argument there holds word
// for word: a pointer only ever names a smaller index of the same tree, every read inside the kernel is an
// agent-scope atomic, a successful CAS hooks a root under a smaller root of another tree).  Before the first
// segment label[w] is the representative of w's class: representatives are the roots, and only they are united.
// (tn_find / tn_unite are a copy of that unit's: sharing them would change the sets unit and detach its evidence)
__device__ inline uint32_t tn_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ inline uint32_t tn_find(uint32_t *par, uint32_t x)         // (splits the path on the way)
{
    uint32_t y = tn_load(par + x);
    while (y != x) {
        const uint32_t z = tn_load(par + y);
        if (z == y)
            return y;
        __hip_atomic_store(par + x, z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = y;
        y = z;
    }
    return x;
}

__device__ inline void tn_unite(uint32_t *par, uint32_t a, uint32_t b)
{
    a = tn_find(par, a);
    b = tn_find(par, b);
    while (a != b) {
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        uint32_t expect = a;                                           // hook the larger root under the smaller
        if (__hip_atomic_compare_exchange_strong(par + a, &expect, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            return;
        a = tn_find(par, expect);
        b = tn_find(par, b);
    }
}

// The pair (a, b) of one slot of segment seg: theirs to compare here if the fingerprints of seg agree and
// those of no earlier segment do.  True if the reads are within k (then united).
__device__ inline bool tn_pair(const uint8_t *const *pl, int L, int k, int seg, const uint32_t *__restrict__ segfp0,
                               size_t seg_stride, uint32_t fmask, size_t base, uint32_t a, uint32_t b, uint32_t *par)
{
    const uint32_t *fa = segfp0 + base + a, *fb = segfp0 + base + b;
    if ((fa[seg * seg_stride] ^ fb[seg * seg_stride]) & fmask)
        return false;
    for (int s = 0; s < seg; s++)
        if (!((fa[s * seg_stride] ^ fb[s * seg_stride]) & fmask))
            return false;                                              // visited at segment s
    if (hamming_upto(pl, L, a, b, k) > k)
        return false;
    tn_unite(par, a, b);
    return true;
}

__device__ inline void tn_add_near(uint32_t *s_near, uint32_t found, unsigned long long *cnt, int tile)
{
    if (found)
        atomicAdd(s_near, found);
    __syncthreads();
    if (threadIdx.x == 0 && *s_near)
        atomicAdd(cnt_row(cnt, tile) + kCntNear, (unsigned long long)*s_near);
}

// grid (ceil(N / 256), n_tiles): at most kTnLong - 1 steps per lane
__global__ void __launch_bounds__(kTdBlock) k_tn_pairs(const uint8_t *const *__restrict__ planes, int L, int k, int seg,
                                                        int64_t N, const uint32_t *__restrict__ segfp0, size_t seg_stride,
                                                        uint32_t fmask, uint32_t slot_mask,
                                                        const uint32_t *__restrict__ slots,
                                                        const uint32_t *__restrict__ next, uint32_t *label,
                                                        unsigned long long *cnt)
{
    __shared__ uint32_t s_near;
    if (threadIdx.x == 0)
        s_near = 0;
    __syncthreads();
    const int tile = blockIdx.y;
    const int64_t w64 = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    const size_t base = (size_t)tile * N, sbase = (size_t)tile * ((size_t)slot_mask + 1);
    uint32_t found = 0;
    if (w64 < N) {
        const uint32_t w = (uint32_t)w64;
        const uint32_t c = next[base + w] == w                          // no vertex
                               ? 0u
                               : slot_count(slots, sbase + seg_slot(segfp0[seg * seg_stride + base + w] & fmask, slot_mask));
        if (c > 1 && c <= kTnLong) {
            const uint8_t *const *pl = planes + (size_t)tile * L;
            uint32_t steps = 0;
            for (uint32_t m = next[base + w]; m != kNil && steps < kTnLong; m = next[base + m], steps++)
                found += tn_pair(pl, L, k, seg, segfp0, seg_stride, fmask, base, w, m, label + base);
        }
    }
    tn_add_near(&s_near, found, cnt, tile);
}

// grid (ceil(max members / 4), n_tiles), a wave per member of a long slot
__global__ void __launch_bounds__(kTdBlock) k_tn_pairs_long(const uint8_t *const *__restrict__ planes, int L, int k,
                                                             int seg, int64_t N, const uint32_t *__restrict__ segfp0,
                                                             size_t seg_stride, uint32_t fmask, uint32_t slot_mask,
                                                             const uint32_t *__restrict__ slots,
                                                             const uint32_t *__restrict__ list,
                                                             const unsigned long long *__restrict__ aux, uint32_t *label,
                                                             unsigned long long *cnt)
{
    __shared__ uint32_t s_near;
    if (threadIdx.x == 0)
        s_near = 0;
    __syncthreads();
    const int tile = blockIdx.y;
    const size_t base = (size_t)tile * N, sbase = (size_t)tile * ((size_t)slot_mask + 1);
    const unsigned long long i = (unsigned long long)blockIdx.x * (kTdBlock / kWave) + threadIdx.x / kWave;
    uint32_t found = 0;
    if (i < aux[2 * tile + 1]) {
        const uint32_t a = list[base + i];
        const uint32_t off = slots[2 * (sbase + seg_slot(segfp0[seg * seg_stride + base + a] & fmask, slot_mask))];
        const uint32_t r = (uint32_t)i - off;                          // a's rank: the members before it
        const uint8_t *const *pl = planes + (size_t)tile * L;
        for (uint32_t j = threadIdx.x & (kWave - 1); j < r; j += kWave)
            found += tn_pair(pl, L, k, seg, segfp0, seg_stride, fmask, base, a, list[base + off + j], label + base);
    }
    tn_add_near(&s_near, found, cnt, tile);
}

// grid (ceil(N / 256), n_tiles): label = root (only well w's lane writes label[w]; what it writes is an
// ancestor), members and first levels cleared for the recount
__global__ void __launch_bounds__(kTdBlock) k_tn_compress(uint32_t *label, int64_t N, uint32_t *__restrict__ members,
                                                           uint32_t *__restrict__ first)
{
    const int tile = blockIdx.y;
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    if (w >= N)
        return;
    uint32_t *par = label + (size_t)tile * N;
    const uint32_t p = tn_load(par + w);
    if (p != kInvalid && p != (uint32_t)w) {
        uint32_t x = p, y = tn_load(par + x);
        while (y != x) {
            x = y;
            y = tn_load(par + x);
        }
        if (x != p)
            __hip_atomic_store(par + w, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    members[(size_t)tile * N + w] = 0;
    first[(size_t)tile * N + w] = kNoLevel;
}

// grid (ceil(N / 256), n_tiles): members counted at the roots (wave_grouped, as k_td_resolve), labels out
__global__ void __launch_bounds__(kTdBlock) k_tn_members(const uint32_t *__restrict__ label, int64_t N, uint32_t *members,
                                                          uint32_t *const *__restrict__ labels_out)
{
    const int tile = blockIdx.y;
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    const size_t base = (size_t)tile * N;
    uint32_t lab = kInvalid;
    if (w < N) {
        lab = label[base + w];
        if (labels_out)
            labels_out[tile][w] = lab;
    }
    const uint32_t add = wave_grouped(lab != kInvalid && lab != (uint32_t)w, lab);
    if (add)
        atomicAdd(members + base + lab, add);
}

}  // namespace

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
        for (int i = 0; i < n_tiles; i++) {
            const int64_t *e = eq.data() + (size_t)i * nrow_eq;
            int64_t *o = out_rows + (size_t)i * nrow;
            std::copy(e, e + 4, o);
            o[4] = 0;
            std::copy(e + 4, e + nrow_eq, o + 5);
        }
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
    // the default budget: DESIGN 5.9 (the worst admitted segment stays well under a second per tile)
    const int64_t budget = pair_budget > 0 ? pair_budget : std::max<int64_t>(16 * N, (int64_t)1 << 24);

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
            if (h_aux[2 * i] > (unsigned long long)budget)
                return fail(ctx, WD_ERR_UNSUPPORTED,
                            "tile near-duplicates: tile " + std::to_string(i) + ", segment " + std::to_string(seg) +
                                " (cycles " + std::to_string(seg_begin(L, nseg, seg)) + ".." +
                                std::to_string(seg_begin(L, nseg, seg + 1) - 1) + "): " + std::to_string(h_aux[2 * i]) +
                                " candidate pairs exceed the pair budget of " + std::to_string(budget) +
                                " (reads of low diversity in that segment)");
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
