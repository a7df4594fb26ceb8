// near_core.inc - what the two near-duplicate passes of the tiledups unit share: tile_near.inc (the clusters of
// every tile, include/welldup_tilenear.h) and lane_near.inc (those of a lane, include/welldup_lanenear.h).
// Included by welldup_tiledups.hip after its own kernels and before tile_near.inc, and by nothing outside that
// unit.  It uses read_classes.inc (mix64, wave_grouped) and the unit's kTdBlock, kWave and kInvalid.
//
// The method.  Vertices are the representatives of the equality classes, the label array (label[v] <= v, a
// representative its own label) is the parent array of a union-find, and an edge joins two reads within K
// mismatches.  The cycles are cut into K + 1 segments; per segment
//   bucket       every vertex into the slot of its segment fingerprint: rank = count[slot]++,
//                next = exchange(head[slot], vertex id) - a chain and its length per slot
//   bound        sum over slots of c (c - 1) / 2 = the pair steps the segment costs (over budget, the host refuses
//                before anything quadratic runs); a slot of more than kTnLong vertices gets a range of the member array
//   scatter      vertices of long slots into their range, at their rank
//   pairs        a lane per vertex of a short slot walks the chain behind itself
//   pairs_long   a wave per vertex of a long slot, its lanes over the vertices of lower rank
// and at the end compress (label = root) and members (members recounted at the roots, labels out).
//
// Why it is exact.  (1) Completeness: two reads within K mismatches agree on one of K + 1 segments (pigeonhole),
// hence on that segment's fingerprint (masked by hash_bits or not), hence on a slot; within the slot either the
// chain walk (every vertex meets every vertex behind it) or the ranks (every vertex meets every vertex of lower
// rank) visit each unordered pair once per segment, and the rule "the first segment whose fingerprints agree"
// picks exactly one of those visits: each true pair is united and counted once.  (2) Soundness: the distance is
// counted on the reads themselves (the planes, or packed rows that are a bijective image of them); a fingerprint
// only saves comparisons.  (3) The union-find is that of welldup_sets.hip on vertex ids: a pointer only ever names
// a smaller id of the same tree, every access to a parent inside a kernel is an agent-scope atomic, a successful
// CAS hooks a root under a smaller root of another tree - roots are smallest ids and the components do not depend
// on the order.  Before the first union label[v] is the representative of v's class: representatives are the
// roots, and only they are united; the other wells point at their representative and are not touched before
// compress, after a kernel boundary.  (4) Every loop is bounded: the chain walk by kTnLong, the long path by the
// budget, find / unite by the forest's depth.  Chains, ranks, bounds and ranges are read only after the kernel
// that wrote them.
//
// A space (TnSpace, LnSpace) is a plain struct of pointers and scalars that a kernel makes from its parameters,
// by value, and lends to the bodies (const S &: they are inlined into it).  It answers what differs between a tile and a lane, for the block's blockIdx.y:
//   slot_t, slot_mask, fmask   the width of a slot index, the table's mask, the fingerprints' mask
//   id(w)                      the vertex id of well w: what chains and labels carry
//   at(id), link(id)           where id lives in the label, member and list arrays; in the next and rank arrays
//   slot_base(), aux_at(), near()   the first slot of its table; its {bound, long members} pair; its NearPairs counter
//   seg_fp(id, seg)            stored or folded from the read: the cost differs, the value's meaning does not
//   reads(), distance_upto(reads, a, b, k), kDistanceFirst      where the reads are, taken once per walk; the
//                              distance on them; whether a pair is tested on it first
//   kChainFirst                whether pairs looks at the chain before it asks for the slot's count
//   clear_more(at)             what compress clears besides members
//   label_out(w, label)        where members writes a label out
// The arrays a body reads or writes are its own parameters, const where it only reads.

namespace {

constexpr int kTnMaxK = 3;
constexpr uint32_t kTnLong = 32;                   // chains up to this length are one lane's walk
constexpr uint32_t kNil = 0xFFFFFFFFu;             // end of a chain
constexpr uint32_t kTnBoundSlots = 4096;           // per workgroup of bound (one per 256 slots was all launch: 8.1 ms per 16 tiles)

__host__ __device__ inline int seg_begin(int L, int nseg, int s) { return (int)((long long)L * s / nseg); }

// A slot of a segment's table is two uint32 side by side (one cache line for both atomics of bucket): [0] the
// head of its chain, [1] all ones minus the number of its vertices - so one fill with 0xFF empties the table.
__device__ inline uint32_t slot_count(const uint32_t *slots, size_t i) { return ~slots[2 * i + 1]; }

template <class S>
__device__ inline size_t near_slot(const S &sp, uint32_t id, int seg)
{
    return sp.slot_base() + ((typename S::slot_t)mix64(sp.seg_fp(id, seg) & sp.fmask) & sp.slot_mask);
}

// (tn_find / tn_unite are a copy of welldup_sets.hip's: sharing them would change the sets unit and detach its evidence)
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

// The bodies.  Grids: bucket, scatter, pairs, compress and members (ceil(N / kTdBlock), tiles), a lane per well;
// bound (ceil(slots / kTnBoundSlots), tiles or 1); pairs_long (ceil(long members / 4), tiles or 1).

// The vertices into the chains of `seg`.  Vertices are the representatives: label == id as long as no union has
// run (by_label).  The unions move labels, so every pass marks the other wells with next == id, which no chain
// produces, and the passes after the first union go by that mark.
template <class S>
__device__ inline void near_bucket(const S &sp, int seg, bool by_label, const uint32_t *label, uint32_t *slots,
                                   uint32_t *next, uint32_t *rank)
{
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    if (w >= sp.N)
        return;
    const uint32_t v = sp.id(w);
    if (by_label ? label[sp.at(v)] != v : next[sp.link(v)] == v) {
        next[sp.link(v)] = v;
        return;
    }
    uint32_t *slot = slots + 2 * near_slot(sp, v, seg);
    rank[sp.link(v)] = ~__hip_atomic_fetch_sub(slot + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    next[sp.link(v)] = __hip_atomic_exchange(slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A lane two slots per 16-byte load, sixteen slots in all.  aux = {sum of c (c - 1) / 2, vertices of long slots},
// 64-bit (one slot of a whole lane is about 1.2e17 pairs); the head of a long slot becomes the start of its
// range in the member array (its chain is not walked; the ranges add up to no more than the vertices).
template <class S>
__device__ inline void near_bound(const S &sp, uint32_t *slots, unsigned long long *aux)
{
    __shared__ unsigned long long s_sum;
    if (threadIdx.x == 0)
        s_sum = 0;
    __syncthreads();
    slots += 2 * sp.slot_base();
    aux += sp.aux_at();
    unsigned long long sum = 0;
    for (uint32_t i = 2 * threadIdx.x; i < kTnBoundSlots; i += 2 * kTdBlock) {
        const size_t s = (size_t)blockIdx.x * kTnBoundSlots + i;      // (slots are a multiple of 64: s + 1 is one too)
        if (s > sp.slot_mask)
            break;
        const uint4 v = *(const uint4 *)(slots + 2 * s);
        const unsigned long long c[2] = {~v.y, ~v.w};
#pragma unroll
        for (int j = 0; j < 2; j++)
            if (c[j] > 1) {
                sum += c[j] * (c[j] - 1) / 2;
                if (c[j] > kTnLong)
                    slots[2 * (s + j)] = (uint32_t)atomicAdd(aux + 1, c[j]);
            }
    }
    if (sum)
        atomicAdd(&s_sum, sum);
    __syncthreads();
    if (threadIdx.x == 0 && s_sum)
        atomicAdd(aux, s_sum);
}

template <class S>
__device__ inline void near_scatter(const S &sp, int seg, const uint32_t *next, const uint32_t *rank,
                                    const uint32_t *slots, uint32_t *list)
{
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    if (w >= sp.N)
        return;
    const uint32_t v = sp.id(w);
    if (next[sp.link(v)] == v)                                         // no vertex
        return;
    const size_t s = near_slot(sp, v, seg);
    if (slot_count(slots, s) > kTnLong)
        list[sp.at(slots[2 * s]) + rank[sp.link(v)]] = v;
}

// The pair (a, b) of one slot of segment seg: this segment's if the fingerprints of seg agree and those of no
// earlier segment do.  True if it is, and the reads are within k (then united).
template <class S, class R>
__device__ inline bool near_pair(const S &sp, R reads, int k, int seg, uint32_t a, uint32_t b, uint32_t *par)
{
    if (S::kDistanceFirst && sp.distance_upto(reads, a, b, k) > k)
        return false;
    if ((sp.seg_fp(a, seg) ^ sp.seg_fp(b, seg)) & sp.fmask)
        return false;
    for (int s = 0; s < seg; s++)
        if (!((sp.seg_fp(a, s) ^ sp.seg_fp(b, s)) & sp.fmask))
            return false;                                              // visited at segment s
    if (!S::kDistanceFirst && sp.distance_upto(reads, a, b, k) > k)
        return false;
    tn_unite(par, a, b);
    return true;
}

__device__ inline void near_add(uint32_t *s_near, uint32_t found, unsigned long long *near)
{
    if (found)
        atomicAdd(s_near, found);
    __syncthreads();
    if (threadIdx.x == 0 && *s_near)
        atomicAdd(near, (unsigned long long)*s_near);
}

// at most kTnLong - 1 steps per lane.  kChainFirst: a vertex with nothing behind it - nearly all - leaves before it
// asks for its slot (the lane folds a row for that).  (Without it, reads() before the walk, k_tn_pairs keeps 60 VGPRs.)
template <class S>
__device__ inline void near_pairs(const S &sp, int k, int seg, const uint32_t *slots, const uint32_t *next,
                                  uint32_t *label)
{
    __shared__ uint32_t s_near;
    if (threadIdx.x == 0)
        s_near = 0;
    __syncthreads();
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    uint32_t found = 0;
    if (w < sp.N) {
        const uint32_t v = sp.id(w), first = next[sp.link(v)];
        const bool asks = first != v && !(S::kChainFirst && first == kNil);      // (first == v: no vertex)
        const uint32_t c = asks ? slot_count(slots, near_slot(sp, v, seg)) : 0u;
        if (c > 1 && c <= kTnLong) {
            const auto reads = sp.reads();
            uint32_t steps = 0;
            for (uint32_t m = first; m != kNil && steps < kTnLong; m = next[sp.link(m)], steps++)
                found += near_pair(sp, reads, k, seg, v, m, label + sp.at(0));
        }
    }
    near_add(&s_near, found, sp.near());
}

template <class S>
__device__ inline void near_pairs_long(const S &sp, int k, int seg, const uint32_t *slots, const uint32_t *list,
                                       const unsigned long long *aux, uint32_t *label)
{
    __shared__ uint32_t s_near;
    if (threadIdx.x == 0)
        s_near = 0;
    __syncthreads();
    const unsigned long long i = (unsigned long long)blockIdx.x * (kTdBlock / kWave) + threadIdx.x / kWave;
    uint32_t found = 0;
    if (i < aux[sp.aux_at() + 1]) {
        const uint32_t a = list[sp.at(0) + i];
        const uint32_t off = slots[2 * near_slot(sp, a, seg)];
        const uint32_t r = (uint32_t)i - off;                          // a's rank: the vertices before it
        const auto reads = sp.reads();
        for (uint32_t j = threadIdx.x & (kWave - 1); j < r; j += kWave)
            found += near_pair(sp, reads, k, seg, a, list[sp.at(off) + j], label + sp.at(0));
    }
    near_add(&s_near, found, sp.near());
}

// label = root (only well w's lane writes its label; what it writes is an ancestor), members cleared for the recount
template <class S>
__device__ inline void near_compress(const S &sp, uint32_t *label, uint32_t *members)
{
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    if (w >= sp.N)
        return;
    const uint32_t v = sp.id(w);
    uint32_t *par = label + sp.at(0);
    const uint32_t p = tn_load(par + v);
    if (p != kInvalid && p != v) {
        uint32_t x = p, y = tn_load(par + x);
        while (y != x) {
            x = y;
            y = tn_load(par + x);
        }
        if (x != p)
            __hip_atomic_store(par + v, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    members[sp.at(v)] = 0;
    sp.clear_more(sp.at(v));
}

// members counted at the roots, once per wave and root (wave_grouped, as k_td_resolve), labels out
template <class S>
__device__ inline void near_members(const S &sp, const uint32_t *label, uint32_t *members)
{
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    const uint32_t v = sp.id(w);
    uint32_t lab = kInvalid;
    if (w < sp.N) {
        lab = label[sp.at(v)];
        sp.label_out(w, lab);
    }
    const uint32_t add = wave_grouped(lab != kInvalid && lab != v, lab);
    if (add)
        atomicAdd(members + sp.at(lab), add);
}

// On the host, what wd_tile_near_dups and wd_lane_near_dups_finish both say: the default budget (DESIGN 5.9, 5.12: the worst admitted segment stays well under a second per tile)
unsigned long long near_budget(int64_t pair_budget, unsigned long long wells)
{
    return pair_budget > 0 ? (unsigned long long)pair_budget : std::max<unsigned long long>(16ull * wells, 1ull << 24);
}

// the refusal of a segment over budget, after the caller's prefix (which names the tile, if there is one)
std::string near_refusal(const std::string &prefix, int L, int nseg, int seg, unsigned long long pairs,
                         unsigned long long budget)
{
    return prefix + "segment " + std::to_string(seg) + " (cycles " + std::to_string(seg_begin(L, nseg, seg)) + ".." +
           std::to_string(seg_begin(L, nseg, seg + 1) - 1) + "): " + std::to_string(pairs) +
           " candidate pairs exceed the pair budget of " + std::to_string(budget) +
           " (reads of low diversity in that segment)";
}

// a row of the classes' layout with NearPairs put in as column `at`
void near_row(const int64_t *row, size_t at, size_t cols, int64_t near_pairs, int64_t *out)
{
    std::copy(row, row + at, out);
    out[at] = near_pairs;
    std::copy(row + at, row + cols, out + at + 1);
}

}  // namespace
