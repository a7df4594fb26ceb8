// tile_classes.inc - the device half of welldup_tiledups.hip: the unit's constants, the layout of a per-tile call's
// workspace and the kernels k_td_* (welldup_tiledups.hip's head says what each does).  Included by
// welldup_tiledups.hip after read_classes.inc and by nothing else in the library; it needs no HIP header, so
// tools/read_classes_emu.cpp and tools/near_emu.cpp include it too and run the kernels on the CPU, a fiber per lane
// (tools/wave_emu.h).  The host half - the checks, the uploads, the entry points - stays in welldup_tiledups.hip.

namespace {

constexpr uint32_t kInvalid = WD_INVALID_TARGET;   // label of a non-PF well; slot of a well not in the table
constexpr uint32_t kNoLevel = 0xFFFFFFFFu;         // first level of a well with no classmate in any ring
constexpr int kBins = WD_DUPSET_SIZE_BINS;
constexpr int kTdBlock = 256;

// per-tile counters in the workspace, [n_tiles][kSpread][kCnt] uint64 (spread_row)
constexpr int kCntPf = 0, kCntClasses = 1, kCntInClasses = 2;
constexpr int kCntBins = 3;                        // classes of size 2..8, >= 9
constexpr int kCntFirst = kCntBins + kBins;        // wells whose first level is l (histogram)
constexpr int kCntRing = kCntFirst + kMaxLevels;   // RingWells[l]
constexpr int kCntNear = kCntRing + kMaxLevels;    // pairs of distinct reads within K (tile_near.inc)
constexpr int kCnt = (kCntRing + kMaxLevels + 7) / 8 * 8;
static_assert(kCntNear < kCnt, "the counter row has no room for NearPairs");

// flags[0]: a centre is not its own target index
constexpr int kFlagCentres = 0;

// workspace layout: counters | flags | pointer tables (planes, filters, labels) | per tile: the table
// [slots] uint64 | fingerprints [N] uint64 | slot, then label [N] uint32 | members [N] uint32 |
// first level [N] uint32
struct Layout {
    size_t cnt, flags, planes, filt, lbl, table, fp, label, members, first, bytes;
    uint64_t slots;                                // per tile, a power of two
};

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

constexpr int kMaxCycles = 1024;                   // rows of the plane pointer table a tile has room for

Layout layout_of(int64_t N, int n_tiles)
{
    Layout l;
    const size_t t = (size_t)n_tiles, wells = (size_t)N * t;
    l.slots = 64;
    while (l.slots < 2 * (uint64_t)N)
        l.slots <<= 1;
    l.cnt = 0;
    l.flags = align256(l.cnt + t * kSpread * kCnt * 8);
    l.planes = align256(l.flags + 16);
    l.filt = align256(l.planes + t * kMaxCycles * sizeof(void *));
    l.lbl = align256(l.filt + t * sizeof(void *));
    l.table = align256(l.lbl + t * sizeof(void *));
    l.fp = align256(l.table + t * l.slots * 8);
    l.label = align256(l.fp + wells * 8);
    l.members = align256(l.label + wells * 4);
    l.first = align256(l.members + wells * 4);
    l.bytes = align256(l.first + wells * 4);
    return l;
}

// the typed pointers of a workspace laid out by layout_of
struct View {
    unsigned long long *cnt;
    uint32_t *flags;
    const uint8_t **planes, **filt;
    uint32_t **lbl;
    unsigned long long *table, *fp;
    uint32_t *label, *members, *first;
    uint32_t slot_mask;
    View(const Layout &l, void *workspace)
    {
        uint8_t *ws = (uint8_t *)workspace;
        cnt = (unsigned long long *)(ws + l.cnt);
        flags = (uint32_t *)(ws + l.flags);
        planes = (const uint8_t **)(ws + l.planes);
        filt = (const uint8_t **)(ws + l.filt);
        lbl = (uint32_t **)(ws + l.lbl);
        table = (unsigned long long *)(ws + l.table);
        fp = (unsigned long long *)(ws + l.fp);
        label = (uint32_t *)(ws + l.label);
        members = (uint32_t *)(ws + l.members);
        first = (uint32_t *)(ws + l.first);
        slot_mask = (uint32_t)(l.slots - 1);
    }
};

__device__ inline unsigned long long *cnt_row(unsigned long long *cnt, int tile) { return spread_row(cnt, (size_t)tile, kCnt); }

// grid (ceil(N / (V * 256)), n_tiles).  VEC4: every plane is 4-byte aligned, a lane folds wells 4 i .. 4 i + 3
// (plane_pass).  Also clears the members array (k_td_resolve counts into it).
template <bool VEC4>
__global__ void __launch_bounds__(kTdBlock) k_td_fingerprint(const uint8_t *const *__restrict__ planes, int L,
                                                              int64_t N, unsigned long long *__restrict__ fp,
                                                              uint32_t *__restrict__ members)
{
    constexpr int V = VEC4 ? 4 : 1;
    const int tile = blockIdx.y;
    const int64_t w0 = ((int64_t)blockIdx.x * kTdBlock + threadIdx.x) * V;
    if (w0 >= N)
        return;
    const uint8_t *const *pl = planes + (size_t)tile * L;
    fp += (size_t)tile * N;
    members += (size_t)tile * N;
    if (VEC4 && w0 + 4 <= N) {
        Fp h[4];
        plane_pass<true>(pl, 0, L, w0, [&](int, const uint32_t(&acc)[4]) {
#pragma unroll
            for (int q = 0; q < 4; q++)
                h[q].fold(acc[q]);
        });
#pragma unroll
        for (int q = 0; q < 4; q++) {
            fp[w0 + q] = h[q].value();
            members[w0 + q] = 0;
        }
        return;
    }
    for (int64_t w = w0; w < N && w < w0 + V; w++) {         // unaligned planes, and the last wells of a tile
        Fp h;
        plane_pass<false>(pl, 0, L, w, [&](int, const uint32_t(&acc)[1]) { h.fold(acc[0]); });
        fp[w] = h.value();
        members[w] = 0;
    }
}

// grid (ceil(N / 256), n_tiles), one lane per PF well into the tile's table (claim_or_join: id = well index,
// equality decided on the reads); slot_of[w] = the well's slot, kInvalid for a non-PF well
__global__ void __launch_bounds__(kTdBlock) k_td_insert(const uint8_t *const *__restrict__ planes,
                                                         const uint8_t *const *__restrict__ filt, int L, int64_t N,
                                                         const unsigned long long *__restrict__ fp,
                                                         unsigned long long fp_mask, unsigned long long *table,
                                                         uint32_t slot_mask, uint32_t *__restrict__ slot_of)
{
    const int tile = blockIdx.y;
    const int64_t w64 = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    if (w64 >= N)
        return;
    const uint32_t w = (uint32_t)w64;
    const size_t base = (size_t)tile * N;
    if (!(filt[tile][w] & 1u)) {                                       // bcl_direct_reader.py:246
        slot_of[base + w] = kInvalid;
        return;
    }
    const uint8_t *const *pl = planes + (size_t)tile * L;
    unsigned long long *tab = table + (size_t)tile * ((size_t)slot_mask + 1);
    const unsigned long long m = mix64(fp[base + w] & fp_mask);
    const unsigned long long tag = m & 0xFFFFFFFF00000000ull;
    slot_of[base + w] = claim_or_join(tab, slot_mask, m, tag, w, [=](unsigned long long cur) {       // (>= 2 N slots)
        return (cur & 0xFFFFFFFF00000000ull) == tag && reads_equal(pl, L, w, (uint32_t)cur);
    });
}

// grid (ceil(N / 256), n_tiles): slot -> label (in place), members counted at the representative
__global__ void __launch_bounds__(kTdBlock) k_td_resolve(const unsigned long long *__restrict__ table,
                                                          uint32_t slot_mask, int64_t N, uint32_t *__restrict__ label,
                                                          uint32_t *members, uint32_t *__restrict__ first,
                                                          uint32_t *const *__restrict__ labels_out,
                                                          unsigned long long *cnt)
{
    __shared__ uint32_t s_pf;
    if (threadIdx.x == 0)
        s_pf = 0;
    __syncthreads();
    const int tile = blockIdx.y;
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    const size_t base = (size_t)tile * N;
    uint32_t s = kInvalid, lab = kInvalid;
    if (w < N) {
        s = label[base + w];
        if (s != kInvalid) {
            lab = (uint32_t)table[(size_t)tile * ((size_t)slot_mask + 1) + s];
            label[base + w] = lab;
        }
        first[base + w] = kNoLevel;
        if (labels_out)
            labels_out[tile][w] = lab;
    }
    const uint32_t add = wave_grouped(lab != kInvalid && lab != (uint32_t)w, lab);
    if (add)
        atomicAdd(members + base + lab, add);
    const unsigned long long pf = __ballot(s != kInvalid);
    if ((threadIdx.x & (kWave - 1)) == 0 && pf)
        atomicAdd(&s_pf, (uint32_t)__popcll(pf));
    __syncthreads();
    if (threadIdx.x == 0 && s_pf)
        atomicAdd(cnt_row(cnt, tile) + kCntPf, (unsigned long long)s_pf);
}

// grid (ceil(N / 256), n_tiles).  Target t is well t (checked by the caller).  The wells in classes are few
// (a lane per well walking 35 slots one after the other was bound by the latency of its two dependent
// loads per slot: 3 ms per 16 tiles): a workgroup lists those among its 256 wells in LDS and then takes
// them kTdGroup lanes to a well, a lane every kTdGroup-th slot of the well's rings.
constexpr int kTdGroup = 16;

__global__ void __launch_bounds__(kTdBlock) k_td_local(const uint32_t *__restrict__ label,
                                                        const uint32_t *__restrict__ members, int64_t N,
                                                        const int32_t *__restrict__ lvl_off,
                                                        const int32_t *__restrict__ nbr, int levels, uint32_t *first,
                                                        unsigned long long *cnt)
{
    // [0] classes, [1] wells in classes, then the size bins, then RingWells per level
    __shared__ unsigned long long s_sum[2 + kBins + kMaxLevels];
    __shared__ uint32_t s_list[kTdBlock];
    __shared__ uint32_t s_n;
    for (int i = threadIdx.x; i < 2 + kBins + kMaxLevels; i += kTdBlock)
        s_sum[i] = 0;
    if (threadIdx.x == 0)
        s_n = 0;
    __syncthreads();
    const int tile = blockIdx.y;
    const size_t base = (size_t)tile * N;
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    if (w < N) {
        const uint32_t lab = label[base + w];
        const uint32_t m = lab == (uint32_t)w ? members[base + w] : 0u;
        if (m > 0) {                                                   // the representative of a class of m + 1
            atomicAdd(&s_sum[0], 1ull);
            atomicAdd(&s_sum[2 + min(m + 1u, (uint32_t)(kBins + 1)) - 2u], 1ull);
        }
        if (lab != kInvalid && (lab != (uint32_t)w || m > 0))
            s_list[atomicAdd(&s_n, 1u)] = (uint32_t)w;
    }
    __syncthreads();
    const uint32_t n_list = s_n;
    const int sub = threadIdx.x % kTdGroup;
    for (uint32_t e = threadIdx.x / kTdGroup; e < n_list; e += kTdBlock / kTdGroup) {
        const uint32_t v = s_list[e];
        const uint32_t lab = label[base + v];
        const int32_t *o = lvl_off + (size_t)v * (levels + 1);
        const int o0 = o[0], o_end = o[levels];
        if (sub == 0) {
            atomicAdd(&s_sum[1], 1ull);
            for (int l = 0; l < levels; l++)
                if (o[l + 1] > o0)
                    atomicAdd(&s_sum[2 + kBins + l], (unsigned long long)(o[l + 1] - o0));
        }
        uint32_t mine = kNoLevel;
        int l = 0;
        for (int s = o0 + sub; s < o_end; s += kTdGroup) {
            while (s >= o[l + 1])                                      // (s < o[levels]: l stays below levels)
                l++;
            const int b = nbr[s];
            if (b >= 0 && b < N && (uint32_t)b != v && label[base + b] == lab) {
                mine = min(mine, (uint32_t)l);
                atomicMin(first + base + b, (uint32_t)l);              // (b has its classmate v with b in v's ring l)
            }
        }
        if (mine != kNoLevel)
            atomicMin(first + base + v, mine);
    }
    __syncthreads();
    unsigned long long *row = cnt_row(cnt, tile);
    for (int i = threadIdx.x; i < 2 + kBins + levels; i += kTdBlock) {
        const unsigned long long v = s_sum[i];
        if (v)
            atomicAdd(row + (i == 0 ? kCntClasses : i == 1 ? kCntInClasses : i < 2 + kBins ? kCntBins + (i - 2)
                                                                                           : kCntRing + (i - 2 - kBins)),
                      v);
    }
}

// grid (ceil(N / 256), n_tiles): histogram of the first levels
__global__ void __launch_bounds__(kTdBlock) k_td_levels(const uint32_t *__restrict__ first, int64_t N, int levels,
                                                         unsigned long long *cnt)
{
    __shared__ uint32_t s_hist[kMaxLevels];
    if (threadIdx.x < kMaxLevels)
        s_hist[threadIdx.x] = 0;
    __syncthreads();
    const int tile = blockIdx.y;
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    if (w < N) {
        const uint32_t f = first[(size_t)tile * N + w];
        if (f < (uint32_t)levels)
            atomicAdd(&s_hist[f], 1u);
    }
    __syncthreads();
    if (threadIdx.x < levels && s_hist[threadIdx.x])
        atomicAdd(cnt_row(cnt, tile) + kCntFirst + threadIdx.x, (unsigned long long)s_hist[threadIdx.x]);
}

__global__ void __launch_bounds__(kTdBlock) k_td_check_centres(const int32_t *__restrict__ centre, int T,
                                                                uint32_t *flags)
{
    const int t = blockIdx.x * kTdBlock + threadIdx.x;
    if (t < T && centre[t] != t)
        atomicOr(flags + kFlagCentres, 1u);
}

}  // namespace
