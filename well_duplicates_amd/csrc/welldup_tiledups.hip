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
// This unit reads the context (targets, stream) and keeps no state in it.
// tile_near.inc (included at the end) builds the near-duplicate clusters of welldup_tilenear.h on these parts,
// lane_dups.inc (after it) the classes across all tiles of a lane of welldup_lanedups.h.
#include "wd_ctx.h"
#include "wd_tiledups.h"
#include "welldup_tiledups.h"

#ifndef WD_UNIT_ID
#define WD_UNIT_ID "unknown"
#endif
namespace wd { const char *unit_id_tiledups() { return WD_UNIT_ID; } }      // hash of this unit's sources (wd_build_id)

namespace {

using namespace wd;

constexpr uint32_t kInvalid = WD_INVALID_TARGET;   // label of a non-PF well; slot of a well not in the table
constexpr uint32_t kNoLevel = 0xFFFFFFFFu;         // first level of a well with no classmate in any ring
constexpr unsigned long long kEmpty = ~0ull;       // a free slot (no entry looks like it: a well index is < kInvalid)
constexpr int kBins = WD_DUPSET_SIZE_BINS;
constexpr int kTdBlock = 256;
constexpr int kFpCycles = 10;                      // cycles folded per 30-bit word, and planes in flight per lane

// per-tile counters in the workspace, [n_tiles][kSpread][kCnt] uint64: a workgroup adds its sums to copy
// blockIdx.x % kSpread and the host adds the copies up (one copy per tile serialises the ~17 000
// workgroups of a 4.3 M-well tile on a few addresses: welldup_sets.hip)
constexpr int kSpread = 64;
constexpr int kCntPf = 0, kCntClasses = 1, kCntInClasses = 2;
constexpr int kCntBins = 3;                        // classes of size 2..8, >= 9
constexpr int kCntFirst = kCntBins + kBins;        // wells whose first level is l (histogram)
constexpr int kCntRing = kCntFirst + kMaxLevels;   // RingWells[l]
constexpr int kCnt = (kCntRing + kMaxLevels + 7) / 8 * 8;

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

__device__ inline unsigned long long *cnt_row(unsigned long long *cnt, int tile)
{
    return cnt + ((size_t)tile * kSpread + blockIdx.x % kSpread) * kCnt;
}

// the reference's alphabet: byte 0 is N (4), any other byte its low two bits (bcl_direct_reader.py:352-361)
__device__ inline uint32_t code_of(uint32_t byte) { return byte ? (byte & 3u) : 4u; }

// ---- fingerprint ------------------------------------------------------------------------------
// Ten cycles, three bits each, make a 30-bit word; the words of a read go through two 32-bit
// multiplicative hashes (a 64-bit multiply per word and well would make the pass compute bound).
// Whatever this hash cannot tell apart is told apart on the reads by k_td_insert.
struct Fp {
    uint32_t a = 0x811C9DC5u, b = 0x01000193u;
    __device__ inline void fold(uint32_t w)
    {
        a = (a ^ w) * 0x9E3779B1u;
        a ^= a >> 15;
        b = (b + w) * 0x85EBCA6Bu;
        b ^= b >> 13;
    }
    __device__ inline unsigned long long value() const { return ((unsigned long long)a << 32) | b; }
};

__device__ inline unsigned long long mix64(unsigned long long x)      // (the murmur3 finaliser)
{
    x ^= x >> 33;
    x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33;
    x *= 0xC4CEB9FE1A85EC53ull;
    x ^= x >> 33;
    return x;
}

// grid (ceil(N / (V * 256)), n_tiles).  VEC4: every plane is 4-byte aligned, a lane folds wells 4 i .. 4 i + 3
// from dword loads.  The plane pointers are the same for every lane: they come through the scalar cache.
// Also clears the members array (k_td_resolve counts into it).
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
        int c = 0;
        for (; c + kFpCycles <= L; c += kFpCycles) {
            uint32_t v[kFpCycles];
#pragma unroll
            for (int j = 0; j < kFpCycles; j++)             // (non-temporal: the planes are streamed)
                v[j] = __builtin_nontemporal_load((const uint32_t *)(pl[c + j] + w0));
            uint32_t acc[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < kFpCycles; j++)
#pragma unroll
                for (int q = 0; q < 4; q++)
                    acc[q] |= code_of((v[j] >> (8 * q)) & 0xFFu) << (3 * j);
#pragma unroll
            for (int q = 0; q < 4; q++)
                h[q].fold(acc[q]);
        }
        if (c < L) {
            uint32_t acc[4] = {0, 0, 0, 0};
            for (int j = 0; c + j < L; j++) {
                const uint32_t v = __builtin_nontemporal_load((const uint32_t *)(pl[c + j] + w0));
#pragma unroll
                for (int q = 0; q < 4; q++)
                    acc[q] |= code_of((v >> (8 * q)) & 0xFFu) << (3 * j);
            }
#pragma unroll
            for (int q = 0; q < 4; q++)
                h[q].fold(acc[q]);
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            fp[w0 + q] = h[q].value();
            members[w0 + q] = 0;
        }
        return;
    }
    for (int64_t w = w0; w < N && w < w0 + V; w++) {         // unaligned planes, and the last wells of a tile
        Fp h;
        for (int c = 0; c < L; c += kFpCycles) {
            uint32_t acc = 0;
            for (int j = 0; j < kFpCycles && c + j < L; j++)
                acc |= code_of(pl[c + j][w]) << (3 * j);
            h.fold(acc);
        }
        fp[w] = h.value();
        members[w] = 0;
    }
}

// ---- the table ----------------------------------------------------------------------------------
// A slot is one 64-bit word (tag << 32) | representative, all ones = free.  Memory model as for the parent
// pointers of welldup_sets.hip (per-XCD L2s, L1s that other CUs' stores never refresh): inside the kernel a
// slot is only touched by agent-scope atomics - a relaxed load, a CAS that claims a free slot with tag and
// own index at once, an atomic min that lowers the representative.  Why the outcome does not depend on the
// order of execution:
//   - a slot is claimed once and never freed, and every well that joins it has been compared with its
//     representative on the reads and found equal: all wells a slot ever names belong to one class, so a
//     stale representative is still a member of that class and decides a comparison the same way;
//   - a load that sees a free slot is followed by the CAS, which fails on a slot claimed meanwhile and
//     returns what it holds: the lane then treats the same slot as it would have, had it seen that value;
//   - every well of a class therefore passes the same slots (those of other classes on its probe path,
//     which never change class) and stops at the first that is free or its own class's: a class has
//     exactly one slot, and the min leaves its smallest index there, whichever lane came first.
// Equality is decided by reads_equal, never by the tag: a tag only saves comparisons.
// (kCmpCycles cycles of both wells are loaded before the first is looked at: a lane that compared cycle by
// cycle waited for two dependent loads 150 times over, and its wave with it)
constexpr int kCmpCycles = 16;

__device__ inline bool reads_equal(const uint8_t *const *pl, int L, uint32_t a, uint32_t b)
{
    int c = 0;
    for (; c + kCmpCycles <= L; c += kCmpCycles) {
        uint32_t x[kCmpCycles], y[kCmpCycles];
#pragma unroll
        for (int j = 0; j < kCmpCycles; j++) {
            const uint8_t *p = pl[c + j];
            x[j] = p[a];
            y[j] = p[b];
        }
        uint32_t diff = 0;
#pragma unroll
        for (int j = 0; j < kCmpCycles; j++)
            diff |= code_of(x[j]) ^ code_of(y[j]);
        if (diff)
            return false;
    }
    for (; c < L; c++) {
        const uint8_t *p = pl[c];
        if (code_of(p[a]) != code_of(p[b]))
            return false;
    }
    return true;
}

// grid (ceil(N / 256), n_tiles); slot_of[w] = the well's slot, kInvalid for a non-PF well
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
    const unsigned long long tag = m & 0xFFFFFFFF00000000ull, mine = tag | w;
    uint32_t s = (uint32_t)m & slot_mask;
    for (;;) {
        // (a load first: a CAS straight away saved 6 % of this kernel on a tile of mostly unique reads, and
        // on a tile of equal reads put 4.3 M of them on one word - 49 ms instead of 3)
        unsigned long long cur = __hip_atomic_load(tab + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kEmpty &&
            __hip_atomic_compare_exchange_strong(tab + s, &cur, mine, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            break;                                                     // claimed (else cur = what the slot holds now)
        if ((cur & 0xFFFFFFFF00000000ull) == tag && reads_equal(pl, L, w, (uint32_t)cur)) {
            if (w < (uint32_t)cur)                                     // (the word only ever goes down)
                __hip_atomic_fetch_min(tab + s, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
        s = (s + 1) & slot_mask;                                       // the table has >= 2 N slots: a free one comes
    }
    slot_of[base + w] = s;
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
    // members: the lanes of a wave that name the same representative as the first of them add once (wells
    // of one class lie side by side when a tile's reads are all equal: 4.3 M adds to one word took 49 ms)
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
    if (!ctx->has_targets)
        return fail(ctx, WD_ERR_STATE, "wd_set_targets has not been called");
    const int levels = ctx->levels;
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
    const Layout lay = layout_of(N, n_tiles);
    if (n_tiles > 0 && (!workspace_dev || workspace_bytes < lay.bytes))
        return fail(ctx, WD_ERR_ARG, "workspace smaller than wd_tile_dups_workspace");
    if (n_tiles > 0 && (!filter || (L > 0 && !planes)))
        return fail(ctx, WD_ERR_ARG, "null plane or filter table");
    if (ctx->T > 0 && n_tiles > 0 && (ctx->idx_min < 0 || ctx->idx_max >= N))
        return fail(ctx, WD_ERR_INDEX, "a target names a well outside the tile");
    if (bind_device(ctx))
        return WD_ERR_HIP;
    const size_t nrow = 4 + 2 * (size_t)levels + kBins;
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
        if (!filter[i] || !on_device(filter[i]) || (L > 0 && !on_device(planes[(size_t)i * L])))
            return fail(ctx, WD_ERR_ARG, "tile duplicates: planes and filters must be in device memory");
        if (labels_dev && !labels_dev[i])
            return fail(ctx, WD_ERR_ARG, "null label pointer");
    }

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
    const uint32_t slot_mask = (uint32_t)(lay.slots - 1);
    const unsigned long long fp_mask = hash_bits == 0 ? ~0ull : (1ull << hash_bits) - 1;

    std::vector<uint32_t *> h_lbl(n_tiles, nullptr);
    if (labels_dev)
        for (int i = 0; i < n_tiles; i++)
            h_lbl[i] = labels_dev[i];
    WD_HIP(ctx, hipMemsetAsync(ws + lay.cnt, 0, lay.planes - lay.cnt, ctx->stream));          // counters and flags
    WD_HIP(ctx, hipMemsetAsync(table, 0xFF, (size_t)n_tiles * lay.slots * 8, ctx->stream));   // every slot free
    if (L > 0)
        WD_HIP(ctx, hipMemcpyAsync(d_planes, planes, (size_t)n_tiles * L * sizeof(void *), hipMemcpyHostToDevice,
                                   ctx->stream));
    WD_HIP(ctx, hipMemcpyAsync(d_filt, filter, n_tiles * sizeof(void *), hipMemcpyHostToDevice, ctx->stream));
    WD_HIP(ctx, hipMemcpyAsync(d_lbl, h_lbl.data(), n_tiles * sizeof(void *), hipMemcpyHostToDevice, ctx->stream));

    const unsigned wblocks = (unsigned)((N + kTdBlock - 1) / kTdBlock);
    const dim3 wgrid(wblocks, (unsigned)n_tiles);
    hipLaunchKernelGGL(k_td_check_centres, dim3(wblocks), dim3(kTdBlock), 0, ctx->stream, ctx->d_centre, ctx->T, flags);
    if (aligned4)
        hipLaunchKernelGGL(k_td_fingerprint<true>, dim3((unsigned)((N + 4 * kTdBlock - 1) / (4 * kTdBlock)), (unsigned)n_tiles),
                           dim3(kTdBlock), 0, ctx->stream, d_planes, L, N, fp, members);
    else
        hipLaunchKernelGGL(k_td_fingerprint<false>, wgrid, dim3(kTdBlock), 0, ctx->stream, d_planes, L, N, fp, members);
    hipLaunchKernelGGL(k_td_insert, wgrid, dim3(kTdBlock), 0, ctx->stream, d_planes, d_filt, L, N, fp, fp_mask, table,
                       slot_mask, label);
    hipLaunchKernelGGL(k_td_resolve, wgrid, dim3(kTdBlock), 0, ctx->stream, table, slot_mask, N, label, members, first,
                       labels_dev ? d_lbl : nullptr, cnt);
    hipLaunchKernelGGL(k_td_local, wgrid, dim3(kTdBlock), 0, ctx->stream, label, members, N, ctx->d_lvl_off, ctx->d_nbr,
                       levels, first, cnt);
    hipLaunchKernelGGL(k_td_levels, wgrid, dim3(kTdBlock), 0, ctx->stream, first, N, levels, cnt);
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
        int64_t local = 0;
        for (int l = 0; l < levels; l++) {
            local += (int64_t)c[kCntFirst + l];
            o[4 + l] = local;
            o[4 + levels + l] = (int64_t)c[kCntRing + l];
        }
        for (int b = 0; b < kBins; b++)
            o[4 + 2 * levels + b] = (int64_t)c[kCntBins + b];
    }
    return WD_OK;
} WD_CATCH

}  // extern "C"

#include "tile_near.inc"      // near-duplicate clusters (include/welldup_tilenear.h) on the parts above
#include "lane_dups.inc"      // read classes across the tiles of a lane (include/welldup_lanedups.h)
