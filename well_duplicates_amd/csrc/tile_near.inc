// tile_near.inc - near-duplicate read clusters of every tile (include/welldup_tilenear.h): PF wells linked by
// Hamming distance <= K anywhere on the tile, single linkage.  Included at the end of welldup_tiledups.hip:
// it uses that unit's fingerprint words, table, code_of, k_td_insert / k_td_resolve / k_td_local / k_td_levels
// and counter layout.
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

constexpr int kCntNear = kCntRing + kMaxLevels;    // pairs of distinct reads within K (a spare counter of the row)
static_assert(kCntNear < kCnt, "the counter row has no room for NearPairs");
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

// grid as k_td_fingerprint.  segfp[s][tile * N + w]; also clears the members array.
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
            const int end = seg_begin(L, nseg, s + 1);
            int c = seg_begin(L, nseg, s);
            Fp g[4];
            for (; c + kFpCycles <= end; c += kFpCycles) {
                uint32_t v[kFpCycles];
#pragma unroll
                for (int j = 0; j < kFpCycles; j++)
                    v[j] = __builtin_nontemporal_load((const uint32_t *)(pl[c + j] + w0));
                uint32_t acc[4] = {0, 0, 0, 0};
#pragma unroll
                for (int j = 0; j < kFpCycles; j++)
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        acc[q] |= code_of((v[j] >> (8 * q)) & 0xFFu) << (3 * j);
#pragma unroll
                for (int q = 0; q < 4; q++)
                    g[q].fold(acc[q]);
            }
            if (c < end) {                                   // the 30-bit word is flushed at the segment's end
                uint32_t acc[4] = {0, 0, 0, 0};
                for (int j = 0; c + j < end; j++) {
                    const uint32_t v = __builtin_nontemporal_load((const uint32_t *)(pl[c + j] + w0));
#pragma unroll
                    for (int q = 0; q < 4; q++)
                        acc[q] |= code_of((v >> (8 * q)) & 0xFFu) << (3 * j);
                }
#pragma unroll
                for (int q = 0; q < 4; q++)
                    g[q].fold(acc[q]);
            }
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
            for (int c = seg_begin(L, nseg, s); c < end; c += kFpCycles) {
                uint32_t acc = 0;
                for (int j = 0; j < kFpCycles && c + j < end; j++)
                    acc |= code_of(pl[c + j][w]) << (3 * j);
                g.fold(acc);
            }
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

// mismatching cycles of wells a and b, counted no further than the block in which they pass k
__device__ inline int hamming_upto(const uint8_t *const *pl, int L, uint32_t a, uint32_t b, int k)
{
    int d = 0, c = 0;
    for (; c + kCmpCycles <= L; c += kCmpCycles) {
        uint32_t x[kCmpCycles], y[kCmpCycles];
#pragma unroll
        for (int j = 0; j < kCmpCycles; j++) {
            const uint8_t *p = pl[c + j];
            x[j] = p[a];
            y[j] = p[b];
        }
#pragma unroll
        for (int j = 0; j < kCmpCycles; j++)
            d += code_of(x[j]) != code_of(y[j]);
        if (d > k)
            return d;
    }
    for (; c < L; c++) {
        const uint8_t *p = pl[c];
        d += code_of(p[a]) != code_of(p[b]);
    }
    return d;
}

// Union-find on the label array, as the parent pointers of welldup_sets.hip (the argument there holds word
// for word: a pointer only ever names a smaller index of the same tree, every read inside the kernel is an
// agent-scope atomic, a successful CAS hooks a root under a smaller root of another tree).  Before the first
// segment label[w] is the representative of w's class: representatives are the roots, and only they are united.
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

// grid (ceil(N / 256), n_tiles): members counted at the roots (lanes of a wave that name the root of the
// first of them add once, as k_td_resolve), labels out
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
    const bool member = lab != kInvalid && lab != (uint32_t)w;
    const unsigned long long joiners = __ballot(member);
    if (joiners) {
        const int lane = threadIdx.x & (kWave - 1), leader = __ffsll((long long)joiners) - 1;
        const uint32_t lab0 = (uint32_t)__shfl((int)lab, leader);
        const bool same = member && lab == lab0;
        const unsigned long long group = __ballot(same);
        if (lane == leader)
            atomicAdd(members + base + lab0, (uint32_t)__popcll(group));
        else if (member && !same)
            atomicAdd(members + base + lab, 1u);
    }
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
    if (!ctx->has_targets)
        return fail(ctx, WD_ERR_STATE, "wd_set_targets has not been called");
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
    if ((int64_t)ctx->T != N || levels < 1)
        return fail(ctx, WD_ERR_ARG, "tile duplicates need every well as a target (T == N)");
    if (ctx->well_stride != 1)
        return fail(ctx, WD_ERR_UNSUPPORTED, "tile duplicates read a plane per cycle (well_stride 1)");
    if (N >= ((int64_t)1 << 31))
        return fail(ctx, WD_ERR_UNSUPPORTED, "tile duplicates: more than 2^31 - 1 wells");
    if (L > kMaxCycles)
        return fail(ctx, WD_ERR_UNSUPPORTED, "tile duplicates: more than 1024 cycles");
    if (n_tiles > 65535)
        return fail(ctx, WD_ERR_UNSUPPORTED, "tile duplicates: more than 65535 tiles in one call");
    const NearLayout nl = near_layout_of(N, n_tiles, k);
    const Layout &lay = nl.base;
    if (n_tiles > 0 && (!workspace_dev || workspace_bytes < nl.bytes))
        return fail(ctx, WD_ERR_ARG, "workspace smaller than wd_tile_near_dups_workspace");
    if (n_tiles > 0 && (!filter || !planes))
        return fail(ctx, WD_ERR_ARG, "null plane or filter table");
    if (ctx->T > 0 && n_tiles > 0 && (ctx->idx_min < 0 || ctx->idx_max >= N))
        return fail(ctx, WD_ERR_INDEX, "a target names a well outside the tile");
    if (bind_device(ctx))
        return WD_ERR_HIP;
    memset(out_rows, 0, (size_t)n_tiles * nrow * sizeof(int64_t));
    if (n_tiles == 0 || N == 0)
        return WD_OK;
    bool aligned4 = true;
    for (size_t i = 0; i < (size_t)n_tiles * L; i++) {
        if (!planes[i])
            return fail(ctx, WD_ERR_ARG, "null plane pointer");
        aligned4 = aligned4 && ((uintptr_t)planes[i] & 3u) == 0;
    }
    for (int i = 0; i < n_tiles; i++) {
        if (!filter[i] || !on_device(filter[i]) || !on_device(planes[(size_t)i * L]))
            return fail(ctx, WD_ERR_ARG, "tile duplicates: planes and filters must be in device memory");
        if (labels_dev && !labels_dev[i])
            return fail(ctx, WD_ERR_ARG, "null label pointer");
    }
    // the default budget: DESIGN 5.9 (the worst admitted segment stays well under a second per tile)
    const int64_t budget = pair_budget > 0 ? pair_budget : std::max<int64_t>(16 * N, (int64_t)1 << 24);

    uint8_t *ws = (uint8_t *)workspace_dev;
    unsigned long long *cnt = (unsigned long long *)(ws + lay.cnt);
    uint32_t *flags = (uint32_t *)(ws + lay.flags);
    const uint8_t **d_planes = (const uint8_t **)(ws + lay.planes);
    const uint8_t **d_filt = (const uint8_t **)(ws + lay.filt);
    uint32_t **d_lbl = (uint32_t **)(ws + lay.lbl);
    unsigned long long *table = (unsigned long long *)(ws + lay.table);
    unsigned long long *fp = (unsigned long long *)(ws + lay.fp);
    uint32_t *label = (uint32_t *)(ws + lay.label);
    uint32_t *members = (uint32_t *)(ws + lay.members);
    uint32_t *first = (uint32_t *)(ws + lay.first);
    unsigned long long *aux = (unsigned long long *)(ws + nl.aux);
    uint32_t *segfp = (uint32_t *)(ws + nl.segfp);
    const size_t wells = (size_t)n_tiles * N, all_slots = (size_t)n_tiles * lay.slots;
    uint32_t *slots = (uint32_t *)table;                               // the table's bytes, once it is resolved
    uint32_t *next = (uint32_t *)fp, *rank = next + wells;             // the fingerprints' bytes, once inserted
    uint32_t *list = first;
    const uint32_t slot_mask = (uint32_t)(lay.slots - 1);
    const unsigned long long fp_mask = hash_bits == 0 ? ~0ull : (1ull << hash_bits) - 1;
    const uint32_t fmask = hash_bits == 0 || hash_bits == 32 ? ~0u : (1u << hash_bits) - 1;
    const int nseg = k + 1;

    std::vector<uint32_t *> h_lbl(n_tiles, nullptr);
    if (labels_dev)
        for (int i = 0; i < n_tiles; i++)
            h_lbl[i] = labels_dev[i];
    WD_HIP(ctx, hipMemsetAsync(ws + lay.cnt, 0, lay.planes - lay.cnt, ctx->stream));          // counters and flags
    WD_HIP(ctx, hipMemsetAsync(aux, 0, (size_t)nseg * n_tiles * 2 * 8, ctx->stream));
    WD_HIP(ctx, hipMemsetAsync(table, 0xFF, all_slots * 8, ctx->stream));                      // every slot free
    WD_HIP(ctx, hipMemcpyAsync(d_planes, planes, (size_t)n_tiles * L * sizeof(void *), hipMemcpyHostToDevice, ctx->stream));
    WD_HIP(ctx, hipMemcpyAsync(d_filt, filter, n_tiles * sizeof(void *), hipMemcpyHostToDevice, ctx->stream));
    WD_HIP(ctx, hipMemcpyAsync(d_lbl, h_lbl.data(), n_tiles * sizeof(void *), hipMemcpyHostToDevice, ctx->stream));

    const unsigned wblocks = (unsigned)((N + kTdBlock - 1) / kTdBlock);
    const dim3 wgrid(wblocks, (unsigned)n_tiles), blk(kTdBlock);
    const dim3 sgrid((unsigned)((lay.slots + kTnBoundSlots - 1) / kTnBoundSlots), (unsigned)n_tiles);
    hipLaunchKernelGGL(k_td_check_centres, dim3(wblocks), blk, 0, ctx->stream, ctx->d_centre, ctx->T, flags);
    if (aligned4)
        hipLaunchKernelGGL(k_tn_fingerprint<true>, dim3((unsigned)((N + 4 * kTdBlock - 1) / (4 * kTdBlock)), (unsigned)n_tiles),
                           blk, 0, ctx->stream, d_planes, L, nseg, N, wells, fp, segfp, members);
    else
        hipLaunchKernelGGL(k_tn_fingerprint<false>, wgrid, blk, 0, ctx->stream, d_planes, L, nseg, N, wells, fp, segfp,
                           members);
    hipLaunchKernelGGL(k_td_insert, wgrid, blk, 0, ctx->stream, d_planes, d_filt, L, N, fp, fp_mask, table, slot_mask, label);
    hipLaunchKernelGGL(k_td_resolve, wgrid, blk, 0, ctx->stream, table, slot_mask, N, label, members, first,
                       (uint32_t *const *)nullptr, cnt);
    std::vector<unsigned long long> h_aux((size_t)n_tiles * 2);
    for (int seg = 0; seg < nseg; seg++) {
        unsigned long long *aux_s = aux + (size_t)seg * n_tiles * 2;
        const uint32_t *segfp_s = segfp + (size_t)seg * wells;
        WD_HIP(ctx, hipMemsetAsync(slots, 0xFF, all_slots * 8, ctx->stream));
        hipLaunchKernelGGL(k_tn_bucket, wgrid, blk, 0, ctx->stream, label, seg, N, segfp_s, fmask, slot_mask, slots, next,
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
        hipLaunchKernelGGL(k_tn_pairs, wgrid, blk, 0, ctx->stream, d_planes, L, k, seg, N, segfp, wells, fmask, slot_mask,
                           slots, next, label, cnt);
        if (longest > 0)
            hipLaunchKernelGGL(k_tn_pairs_long,
                               dim3((unsigned)((longest + kTdBlock / kWave - 1) / (kTdBlock / kWave)), (unsigned)n_tiles),
                               blk, 0, ctx->stream, d_planes, L, k, seg, N, segfp, wells, fmask, slot_mask, slots, list, aux_s,
                               label, cnt);
    }
    hipLaunchKernelGGL(k_tn_compress, wgrid, blk, 0, ctx->stream, label, N, members, first);
    hipLaunchKernelGGL(k_tn_members, wgrid, blk, 0, ctx->stream, label, N, members, labels_dev ? d_lbl : nullptr);
    hipLaunchKernelGGL(k_td_local, wgrid, blk, 0, ctx->stream, label, members, N, ctx->d_lvl_off, ctx->d_nbr, levels, first,
                       cnt);
    hipLaunchKernelGGL(k_td_levels, wgrid, blk, 0, ctx->stream, first, N, levels, cnt);
    WD_HIP(ctx, hipGetLastError());
    std::vector<unsigned long long> h_cnt((size_t)n_tiles * kSpread * kCnt);
    uint32_t h_flags[4] = {0, 0, 0, 0};
    WD_HIP(ctx, hipMemcpyAsync(h_cnt.data(), cnt, h_cnt.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                               ctx->stream));
    WD_HIP(ctx, hipMemcpyAsync(h_flags, flags, sizeof(h_flags), hipMemcpyDeviceToHost, ctx->stream));
    WD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_flags[kFlagCentres])
        return fail(ctx, WD_ERR_ARG, "tile duplicates need target t to be centred on well t");

    for (int i = 0; i < n_tiles; i++) {
        unsigned long long c[kCnt] = {};
        for (int r = 0; r < kSpread; r++)
            for (int f = 0; f < kCnt; f++)
                c[f] += h_cnt[((size_t)i * kSpread + r) * kCnt + f];
        int64_t *o = out_rows + (size_t)i * nrow;
        o[0] = (int64_t)c[kCntPf];
        o[1] = (int64_t)c[kCntClasses];
        o[2] = (int64_t)c[kCntInClasses];
        o[3] = o[2] - o[1];
        o[4] = (int64_t)c[kCntNear];
        int64_t local = 0;
        for (int l = 0; l < levels; l++) {
            local += (int64_t)c[kCntFirst + l];
            o[5 + l] = local;
            o[5 + levels + l] = (int64_t)c[kCntRing + l];
        }
        for (int b = 0; b < kBins; b++)
            o[5 + 2 * levels + b] = (int64_t)c[kCntBins + b];
    }
    return WD_OK;
} WD_CATCH

}  // extern "C"
