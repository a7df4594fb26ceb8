// dup_sets.inc - the device half of welldup_sets.hip: the constants, the counters' layout, the workspace layout, the
// parent pointers (load_parent, find_split, find_ro, unite) and the seven k_sets_* kernels, and the fold of the
// counters' copies into a sets row (sets_fold_row: plain host code).  It needs no HIP header, so that
// tools/dup_sets_emu.cpp compiles it as it stands for the CPU (tools/wave_emu.h) and runs the kernels under shuffled
// schedules; welldup_sets.hip includes it inside its unnamed namespace, after wd_ctx.h and welldup_sets.h.
// Wants: kMaxLevels, kWave, WD_INVALID_TARGET, WD_DUPSET_SIZE_BINS.

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

// ---- the sets row (host) ------------------------------------------------------------------------
// Tile `tile`'s kSpread copies of the counters (h_cnt: the counters of every tile as they lie in the workspace) added
// up and folded into row[1 + 3 * levels + kBins]: PF wells, Sets, InSets and Redundant cumulative over the levels
// (Sets[l] = InSets[l] - Redundant[l]: every merge makes one set fewer than the wells that joined one), the size bins.
inline void sets_fold_row(const unsigned long long *h_cnt, int tile, int levels, int64_t *row)
{
    unsigned long long c[kCnt] = {};
    for (int r = 0; r < kSpread; r++)
        for (int f = 0; f < kCnt; f++)
            c[f] += h_cnt[((size_t)tile * kSpread + r) * kCnt + f];
    row[0] = (int64_t)c[kCntPf];
    int64_t in_sets = 0, redundant = 0;
    for (int l = 0; l < levels; l++) {
        in_sets += (int64_t)c[kCntInSets + l];
        redundant += (int64_t)c[kCntHooks + l];
        row[1 + l] = in_sets - redundant;                  // Sets
        row[1 + levels + l] = in_sets;                     // InSets
        row[1 + 2 * levels + l] = redundant;               // Redundant
    }
    for (int b = 0; b < kBins; b++)
        row[1 + 3 * levels + b] = (int64_t)c[kCntBins + b];
}
