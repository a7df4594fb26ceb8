// lane_near.inc - near-duplicate read clusters of a lane (include/welldup_lanenear.h): the PF wells of all tiles
// of a lane linked by Hamming distance <= K, single linkage.  Included at the end of welldup_tiledups.hip: it uses
// read_classes.inc (Fp, mix64, wave_grouped, the spread counters), tile_near.inc (seg_begin, the union-find on a
// label array, kTnLong, kNil, kTnBoundSlots) and lane_dups.inc (the accumulator, ld_equality, ld_count_rows).
//
// wd_lane_near_dups_finish, over the tiles that were added (grid y = tile, a well's place is its global id g):
//   ld_equality       the classes, as wd_lane_dups_finish: after k_ld_resolve label[g] is the representative of g's
//                     class (label[g] <= g, a representative its own label) - the parent array of the union-find.
//                     The lane's table and the 8-byte word per well (aux) are dead from there on: the table takes
//                     the buckets of a segment, aux[g] = {next, rank} of g's chain
//   then, only the representatives being vertices, for every segment s = K..0 (nothing quadratic, no label changed):
//   k_ln_bucket       the segment's fingerprint from the packed row (masks at the segment's ends), then
//                     rank = count[slot]++, next = exchange(head[slot], g)
//   k_ln_bound        sum over slots of c (c - 1) / 2; a slot of more than kTnLong gets a range of the member array
//   (the host refuses the call here if a segment exceeds the budget; segment 0's buckets are still in the table)
//   then per segment s = 0..K (s > 0: k_ln_bucket again, and k_ln_bound if the segment has a long slot):
//   k_ln_scatter      members of long slots into their range, at their rank
//   k_ln_pairs        a lane per representative of a short slot walks the chain behind itself
//   k_ln_pairs_long   a wave per member of a long slot, its lanes over the members of lower rank
//   k_ln_compress, k_ln_members   label = root, members recounted at the roots
//   k_ld_classes, k_ld_span_count, k_ld_span_sum   unchanged, on zeroed counters: they are keyed by label only
//
// Why it is exact.  (1) Completeness: two reads within K mismatches agree on one of K + 1 segments (pigeonhole),
// hence on that segment's masked words of the packed row, hence on its fingerprint (masked by hash_bits or not),
// hence on a slot; within the slot either the chain walk (every member meets every member behind it) or the ranks
// (every member meets every member of lower rank) visit each unordered pair once per segment, and the rule "the
// first segment whose fingerprints agree" picks exactly one of those visits: each true pair is united and counted
// once.  (2) Soundness: distance is counted on the packed rows, a bijective image of the decoded reads; a fingerprint only saves
// comparisons.  (3) The union-find is that of tile_near.inc with "global id" for "well index": pointers only ever
// name a smaller id of the same tree, every access to a parent inside a kernel is an agent-scope atomic, a
// successful CAS hooks a root under a smaller root of another tree - roots are smallest ids and the components do
// not depend on the order.  Non-representatives point at their representative and are not touched before
// k_ln_compress.  (4) Every loop is bounded: the chain walk by kTnLong, the long path by the budget, find / unite by
// the forest's depth.  Chains, ranks, bounds and rows are read only after the kernel that wrote them.
// Tiles that arrived in different wd_lane_dups_add calls: nothing changes.  Bucketing happens entirely inside this
// call, from the packed rows and the resolved labels, neither of which records when a tile came; a bucket's
// members lie on any tiles and every kernel takes global ids throughout.
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

__device__ inline unsigned long long ln_slot(uint32_t f, uint32_t fmask, unsigned long long slot_mask)
{
    return mix64(f & fmask) & slot_mask;
}

// A slot of a segment's table: tile_near.inc's word - [0] the head of its chain, [1] all ones minus the number of
// its members, one 0xFF fill empties the table - in the bytes of the lane's table.  link[2 g] = next, [2 g + 1] =
// rank, in the bytes of aux.  grid (ceil(N / 256), tiles added): the representatives into the chains of `seg`.
// Vertices are the representatives: label[g] == g as long as no union has run (by_label).  The unions move
// labels, so every pass marks the other wells with next == g, which no chain produces, and the passes after the
// first union go by that mark.
__global__ void __launch_bounds__(kTdBlock) k_ln_bucket(const int *__restrict__ tile_idx, int64_t N, int L, int nseg,
                                                         int seg, bool by_label, const uint32_t *__restrict__ label,
                                                         const uint32_t *__restrict__ rows, int words, uint32_t fmask,
                                                         unsigned long long slot_mask, uint32_t *slots,
                                                         uint32_t *__restrict__ link)
{
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    if (w >= N)
        return;
    const size_t g64 = (size_t)tile_idx[blockIdx.y] * (size_t)N + (size_t)w;
    const uint32_t g = (uint32_t)g64;                                  // (max_tiles * N < 2^32 - 1)
    uint32_t *nx = link + 2 * g64;
    if (by_label ? label[g64] != g : nx[0] == g) {
        nx[0] = g;
        return;
    }
    uint32_t *slot = slots + 2 * ln_slot(ln_seg_fp(rows + g64 * words, L, nseg, seg), fmask, slot_mask);
    nx[1] = ~__hip_atomic_fetch_sub(slot + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    nx[0] = __hip_atomic_exchange(slot, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// grid (ceil(slots / kTnBoundSlots)), a lane two slots per 16-byte load, sixteen slots in all.  aux = {sum of
// c (c - 1) / 2, members of long slots}, 64-bit (one slot of a whole lane is about 1.2e17 pairs); the head of a long slot
// becomes the start of its range in the member array (its chain is not walked).
__global__ void __launch_bounds__(kTdBlock) k_ln_bound(uint32_t *__restrict__ slots, unsigned long long slot_mask,
                                                        unsigned long long *aux)
{
    __shared__ unsigned long long s_sum;
    if (threadIdx.x == 0)
        s_sum = 0;
    __syncthreads();
    unsigned long long sum = 0;
    for (uint32_t i = 2 * threadIdx.x; i < kTnBoundSlots; i += 2 * kTdBlock) {
        const unsigned long long s = (unsigned long long)blockIdx.x * kTnBoundSlots + i;      // (slots: a multiple of 64)
        if (s > slot_mask)
            break;
        const uint4 v = *(const uint4 *)(slots + 2 * s);
        const unsigned long long c[2] = {~v.y, ~v.w};
#pragma unroll
        for (int j = 0; j < 2; j++)
            if (c[j] > 1) {
                sum += c[j] * (c[j] - 1) / 2;
                if (c[j] > kTnLong)
                    slots[2 * (s + j)] = (uint32_t)atomicAdd(aux + 1, c[j]);       // (ranges add up to <= W < 2^32)
            }
    }
    if (sum)
        atomicAdd(&s_sum, sum);
    __syncthreads();
    if (threadIdx.x == 0 && s_sum)
        atomicAdd(aux, s_sum);
}

// grid as k_ln_bucket: members of long slots into list[head[slot] + rank]
__global__ void __launch_bounds__(kTdBlock) k_ln_scatter(const int *__restrict__ tile_idx, int64_t N, int L, int nseg,
                                                          int seg, const uint32_t *__restrict__ rows, int words,
                                                          uint32_t fmask, unsigned long long slot_mask,
                                                          const uint32_t *__restrict__ slots,
                                                          const uint32_t *__restrict__ link, uint32_t *__restrict__ list)
{
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    if (w >= N)
        return;
    const size_t g64 = (size_t)tile_idx[blockIdx.y] * (size_t)N + (size_t)w;
    if (link[2 * g64] == (uint32_t)g64)                                // no vertex
        return;
    const unsigned long long s = ln_slot(ln_seg_fp(rows + g64 * words, L, nseg, seg), fmask, slot_mask);
    if (slot_count(slots, s) > kTnLong)
        list[(size_t)slots[2 * s] + link[2 * g64 + 1]] = (uint32_t)g64;            // (a range holds its slot's ranks)
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

// The pair (a, b) of one slot of segment seg.  True if the reads are within k and the pair is this segment's: the
// fingerprints of seg agree and those of no earlier segment do (then united).  The distance comes first: nearly
// every candidate fails it, and only a pair within k pays for the fingerprints.
__device__ inline bool ln_pair(const uint32_t *__restrict__ rows, int words, int L, int k, int seg, uint32_t fmask,
                               uint32_t a, uint32_t b, uint32_t *par)
{
    if (rows_hamming_upto(rows, words, a, b, k) > k)
        return false;
    const uint32_t *x = rows + (size_t)a * words, *y = rows + (size_t)b * words;
    if ((ln_seg_fp(x, L, k + 1, seg) ^ ln_seg_fp(y, L, k + 1, seg)) & fmask)
        return false;
    for (int s = 0; s < seg; s++)
        if (!((ln_seg_fp(x, L, k + 1, s) ^ ln_seg_fp(y, L, k + 1, s)) & fmask))
            return false;                                              // visited at segment s
    tn_unite(par, a, b);
    return true;
}

__device__ inline void ln_add_near(uint32_t *s_near, uint32_t found, unsigned long long *near)
{
    if (found)
        atomicAdd(s_near, found);
    __syncthreads();
    if (threadIdx.x == 0 && *s_near)
        atomicAdd(spread_row(near, 0, 1), (unsigned long long)*s_near);
}

// grid as k_ln_bucket: at most kTnLong - 1 steps per lane
__global__ void __launch_bounds__(kTdBlock) k_ln_pairs(const int *__restrict__ tile_idx, int64_t N, int L, int k, int seg,
                                                        const uint32_t *__restrict__ rows, int words, uint32_t fmask,
                                                        unsigned long long slot_mask, const uint32_t *__restrict__ slots,
                                                        const uint32_t *__restrict__ link, uint32_t *label,
                                                        unsigned long long *near)
{
    __shared__ uint32_t s_near;
    if (threadIdx.x == 0)
        s_near = 0;
    __syncthreads();
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    uint32_t found = 0;
    if (w < N) {
        const size_t g64 = (size_t)tile_idx[blockIdx.y] * (size_t)N + (size_t)w;
        const uint32_t g = (uint32_t)g64, first = link[2 * g64];
        if (first != g && first != kNil) {                             // a vertex with a member behind it
            const uint32_t c = slot_count(slots, ln_slot(ln_seg_fp(rows + g64 * words, L, k + 1, seg), fmask, slot_mask));
            if (c <= kTnLong) {
                uint32_t steps = 0;
                for (uint32_t m = first; m != kNil && steps < kTnLong; m = link[2 * (size_t)m], steps++)
                    found += ln_pair(rows, words, L, k, seg, fmask, g, m, label);
            }
        }
    }
    ln_add_near(&s_near, found, near);
}

// grid (ceil(members of long slots / 4)), a wave per member of a long slot
__global__ void __launch_bounds__(kTdBlock) k_ln_pairs_long(int L, int k, int seg, const uint32_t *__restrict__ rows,
                                                             int words, uint32_t fmask, unsigned long long slot_mask,
                                                             const uint32_t *__restrict__ slots,
                                                             const uint32_t *__restrict__ list,
                                                             const unsigned long long *__restrict__ aux, uint32_t *label,
                                                             unsigned long long *near)
{
    __shared__ uint32_t s_near;
    if (threadIdx.x == 0)
        s_near = 0;
    __syncthreads();
    const unsigned long long i = (unsigned long long)blockIdx.x * (kTdBlock / kWave) + threadIdx.x / kWave;
    uint32_t found = 0;
    if (i < aux[1]) {
        const uint32_t a = list[i];
        const uint32_t off = slots[2 * ln_slot(ln_seg_fp(rows + (size_t)a * words, L, k + 1, seg), fmask, slot_mask)];
        const uint32_t r = (uint32_t)i - off;                          // a's rank: the members before it
        for (uint32_t j = threadIdx.x & (kWave - 1); j < r; j += kWave)
            found += ln_pair(rows, words, L, k, seg, fmask, a, list[(size_t)off + j], label);
    }
    ln_add_near(&s_near, found, near);
}

// grid as k_ln_bucket: label = root (only well g's lane writes label[g]; what it writes is an ancestor), members
// cleared for the recount
__global__ void __launch_bounds__(kTdBlock) k_ln_compress(const int *__restrict__ tile_idx, int64_t N, uint32_t *label,
                                                           uint32_t *__restrict__ members)
{
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    if (w >= N)
        return;
    const size_t g64 = (size_t)tile_idx[blockIdx.y] * (size_t)N + (size_t)w;
    const uint32_t p = tn_load(label + g64);
    if (p != kInvalid && p != (uint32_t)g64) {
        uint32_t x = p, y = tn_load(label + x);
        while (y != x) {
            x = y;
            y = tn_load(label + x);
        }
        if (x != p)
            __hip_atomic_store(label + g64, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    members[g64] = 0;
}

// grid as k_ln_bucket: members counted at the roots, once per wave and root (as k_ld_resolve), labels out
__global__ void __launch_bounds__(kTdBlock) k_ln_members(const int *__restrict__ tile_idx, int64_t N,
                                                          const uint32_t *__restrict__ label, uint32_t *members,
                                                          uint32_t *const *__restrict__ labels_out)
{
    const int ti = tile_idx[blockIdx.y];
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    const size_t g = (size_t)ti * (size_t)N + (size_t)w;
    uint32_t lab = kInvalid;
    if (w < N) {
        lab = label[g];
        if (labels_out && labels_out[ti])
            labels_out[ti][w] = lab;
    }
    const uint32_t add = wave_grouped(lab != kInvalid && lab != (uint32_t)g, lab);
    if (add)
        atomicAdd(members + lab, add);
}

// the cluster rows from the class rows' layout: NearPairs goes in front of the size bins
void ln_near_row(const int64_t *lane_row, int64_t near_pairs, int64_t *near_lane_row)
{
    std::copy(lane_row, lane_row + 6, near_lane_row);
    near_lane_row[6] = near_pairs;
    std::copy(lane_row + 6, lane_row + WD_LANEDUPS_LANE_COLS, near_lane_row + 7);
}

}  // namespace

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
        ln_near_row(lane_row, 0, near_lane_row);
        std::copy(tile_rows, tile_rows + (size_t)T * WD_LANEDUPS_TILE_COLS, near_tile_rows);
        if (wells > 0) {
            if (const int rc = ld_copy_labels(ld, near_labels_dev, true))
                return rc;
            WD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        }
        return WD_OK;
    }
    // the default budget: the per-tile rule of tile_near.inc at lane scale (DESIGN 5.12)
    const unsigned long long budget =
        pair_budget > 0 ? (unsigned long long)pair_budget : std::max<unsigned long long>(16ull * wells, 1ull << 24);

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
            return fail(ctx, WD_ERR_UNSUPPORTED,
                        "lane near-duplicates: segment " + std::to_string(seg) + " (cycles " +
                            std::to_string(seg_begin(L, nseg, seg)) + ".." + std::to_string(seg_begin(L, nseg, seg + 1) - 1) +
                            "): " + std::to_string(h_aux[2 * seg]) + " candidate pairs exceed the pair budget of " +
                            std::to_string(budget) + " (reads of low diversity in that segment)");

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
    ln_near_row(cluster_row, (int64_t)near_pairs, near_lane_row);
    return WD_OK;
} WD_CATCH

}  // extern "C"
