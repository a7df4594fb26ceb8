// lane_dups.inc - read classes across all tiles of a lane (include/welldup_lanedups.h): an accumulator that
// outlives the batches a lane is streamed through device memory in, and stays exact.  Included at the end of
// welldup_tiledups.hip: it uses read_classes.inc (plane_pass, claim_or_join, wave_grouped, the spread counters)
// and that unit's block size and host checks.
//
// In the caller's workspace, for W = max_tiles * N wells of capacity (a well's place is its global id
// g = tile_index * N + well): one table for the lane, the packed rows [W][R] (R = ceil(L / 10) words of ten 3-bit
// codes), aux [W] uint64 (fingerprint, then slot, then slot of the second table), label [W], members [W].
//
// wd_lane_dups_add, per batch of tiles (grid y = tile of the batch):
//   k_ld_pack        the pass of k_td_fingerprint over the planes; the 30-bit words it folds are also stored as the
//                    well's packed row - after this kernel nothing reads the planes again
//   k_ld_insert      one lane per PF well into the lane's table; equality is decided on the packed rows
// wd_lane_dups_finish (ld_equality, which lane_near.inc calls too), over the tiles that were added:
//   k_ld_resolve     slot -> label; members counted at the representative; PF per tile
//   (the table is dead now: it is cleared and used again, keyed by (label, tile))
//   k_ld_classes     classes, size bins, InLane, LaneRedundant; a well in a class enters the second table, whose
//                    slot keeps the smallest member of its (class, tile) group
//   k_ld_span_count  members of a group counted in the upper half of its slot
//   k_ld_span_sum    at a group's smallest member: TileSpans, InTile, TileRedundant, CrossTileClasses
//
// Row layout: a well's R words lie side by side (64 bytes at 151 cycles).  The reader that matters is the
// confirm step of k_ld_insert, which fetches the whole row of ONE far-away representative: side by side that
// is one or two cache lines, word-major ([R][W]) it would be R lines of which four bytes each are used.  The
// writer pays instead: k_ld_pack produces a word of four wells at a time, and turns eight of them round in
// LDS so that what it stores are 32-byte pieces of rows (see there).
#include "welldup_lanedups.h"

namespace {

constexpr unsigned long long kNoSlot = ~0ull;      // aux of a well that is in no table
constexpr int kLdTileCnt = 8;                      // per tile and copy: the tile row's columns
constexpr int kLdPf = 0, kLdInLane = 1, kLdInTile = 2, kLdTileRed = 3, kLdLaneRed = 4;
constexpr int kLdLaneCnt = 16;                     // per copy: the lane's own counters
constexpr int kLdClasses = 0, kLdCross = 1, kLdSpans = 2, kLdBins = 3;
static_assert(kLdBins + kBins <= kLdLaneCnt, "the lane's counter row has no room for the size bins");
constexpr int kLdCmpWords = 8;                     // words of both rows loaded before the first is looked at

// workspace layout (include/welldup_lanedups.h states the arithmetic)
struct LdLayout {
    size_t cnt_t, cnt_l, planes, filt, lbl, tidx, table, rows, aux, label, members, bytes;
    uint64_t slots;                                // a power of two
    int words;
};

LdLayout ld_layout_of(int64_t N, int max_tiles, int L)
{
    LdLayout l;
    const size_t t = (size_t)max_tiles, wells = (size_t)N * t;
    l.words = (L + kFpCycles - 1) / kFpCycles;
    l.slots = 64;
    while (l.slots < 2 * (uint64_t)wells)
        l.slots <<= 1;
    l.cnt_t = 0;
    l.cnt_l = align256(l.cnt_t + t * kSpread * kLdTileCnt * 8);
    l.planes = align256(l.cnt_l + (size_t)kSpread * kLdLaneCnt * 8);
    l.filt = align256(l.planes + t * (size_t)L * sizeof(void *));
    l.lbl = align256(l.filt + t * sizeof(void *));
    l.tidx = align256(l.lbl + t * sizeof(void *));
    l.table = align256(l.tidx + t * sizeof(int));
    l.rows = align256(l.table + l.slots * 8);
    l.aux = align256(l.rows + wells * (size_t)l.words * 4);
    l.label = align256(l.aux + wells * 8);
    l.members = align256(l.label + wells * 4);
    l.bytes = align256(l.members + wells * 4);
    return l;
}

__device__ inline unsigned long long *ld_tile_cnt(unsigned long long *cnt_t, int tile_index)
{
    return spread_row(cnt_t, (size_t)tile_index, kLdTileCnt);
}

// ---- pack ---------------------------------------------------------------------------------------
// The words of plane_pass (plane_word4 one at a time: the wave stops every kLdChunk words) stored as the wells'
// rows as well.  Also clears the wells' members
// (k_ld_resolve counts into them).
// A lane that stored its four wells' words as they come writes four bytes each to four rows, 64 rows per
// store instruction: at 150 cycles that is 69 M four-byte write requests per tile, and they, not the bytes,
// set the kernel's time (0.83 ms per tile where the fingerprint pass alone takes 0.15).  So a workgroup is one
// wave, and the wave stages kLdChunk words of its 256 wells in LDS, word-major as the lanes produce them
// (one 16-byte LDS store per lane and word), and writes them out well-major: consecutive lanes store
// consecutive words of a row, 32-byte pieces that the memory pipeline takes as one request each.
// The LDS row stride of 260 words keeps both sides free of bank conflicts: a lane group of the transposed
// read holds words j = 0..7 of wells w .. w + 3, at banks (4 j + w) mod 32, all different.
// (Measured on 16 full tiles, add per tile at 150 / 51 cycles: words stored as they come 0.94 ms / -; chunks of
// 4 words 0.46 / 0.28, of 8 0.43-0.46 / 0.25-0.26, of 16 0.40 / 0.26 at twice the LDS: 8 it is.)
constexpr int kLdChunk = 8;                        // words of a row staged before they are stored
constexpr int kLdWaveWells = 4 * kWave;            // wells of a workgroup of k_ld_pack<true>
constexpr int kLdStride = kLdWaveWells + 32 / kLdChunk;

// one well, byte loads: unaligned planes, and the last N % 4 wells of a tile
__device__ inline void ld_pack_well(const uint8_t *const *pl, int L, int words, int64_t w, size_t g,
                                    uint32_t *__restrict__ rows, unsigned long long *__restrict__ fp,
                                    uint32_t *__restrict__ members)
{
    Fp h;
    plane_pass<false>(pl, 0, L, w, [&](int k, const uint32_t(&acc)[1]) {
        h.fold(acc[0]);
        rows[g * words + k] = acc[0];
    });
    fp[g] = h.value();
    members[g] = 0;
}

// The kc words staged word-major in s_words, written out as words k .. k + kc - 1 of the wave's first n_quad rows
// (k_lq_pack, lane_quality.inc, stores its quality rows the same way).
__device__ inline void ld_store_staged(const uint32_t *s_words, uint32_t *__restrict__ out, int words, int k, int kc,
                                       int n_quad, int lane)
{
    if (kc == kLdChunk) {
        for (int e = lane; e < n_quad * kLdChunk; e += kWave) {
            const int well = e / kLdChunk, j = e % kLdChunk;
            out[(size_t)well * words + k + j] = s_words[j * kLdStride + well];
        }
    } else {                                                               // the last words of a row
        for (int e = lane; e < n_quad * kc; e += kWave) {
            const int well = e / kc, j = e - well * kc;
            out[(size_t)well * words + k + j] = s_words[j * kLdStride + well];
        }
    }
}

// VEC4 (every plane 4-byte aligned): grid (ceil(N / 256), n_tiles of the batch), 64 threads, a lane folds wells
// 4 i .. 4 i + 3.  Else: grid (ceil(N / 256), n_tiles), 256 threads, a lane one well.
template <bool VEC4>
__global__ void __launch_bounds__(VEC4 ? kWave : kTdBlock) k_ld_pack(const uint8_t *const *__restrict__ planes,
                                                                      const int *__restrict__ tile_idx, int L, int words,
                                                                      int64_t N, uint32_t *__restrict__ rows,
                                                                      unsigned long long *__restrict__ fp,
                                                                      uint32_t *__restrict__ members)
{
    const int tile = blockIdx.y;
    const uint8_t *const *pl = planes + (size_t)tile * L;
    const size_t tile_base = (size_t)tile_idx[tile] * (size_t)N;
    if constexpr (!VEC4) {
        const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
        if (w < N)
            ld_pack_well(pl, L, words, w, tile_base + (size_t)w, rows, fp, members);
        return;
    }
    __shared__ __attribute__((aligned(16))) uint32_t s_words[kLdChunk * kLdStride];
    const int lane = threadIdx.x;
    const int64_t wave0 = (int64_t)blockIdx.x * kLdWaveWells;              // (< N: the grid is cut to the tile)
    const int64_t w0 = wave0 + 4 * lane;
    const bool quad = w0 + 4 <= N;                                         // else: past the tile, or in its last N % 4 wells
    const int n_quad = (int)(min((int64_t)kLdWaveWells, N - wave0) & ~(int64_t)3);      // wells of the wave in whole quads
    uint32_t *out = rows + (tile_base + (size_t)wave0) * words;
    Fp h[4];
    for (int c = 0, k = 0; c < L;) {
        int kc = 0;                                                        // words staged (the same for every lane)
        for (; kc < kLdChunk && c < L; kc++, c += kFpCycles) {
            if (quad) {
                uint32_t acc[4];
                if (c + kFpCycles <= L)
                    plane_word4<true>(pl, c, L, w0, acc);
                else
                    plane_word4<false>(pl, c, L, w0, acc);
#pragma unroll
                for (int q = 0; q < 4; q++)
                    h[q].fold(acc[q]);
                *(uint4 *)(s_words + kc * kLdStride + 4 * lane) = make_uint4(acc[0], acc[1], acc[2], acc[3]);
            }
        }
        __syncthreads();
        ld_store_staged(s_words, out, words, k, kc, n_quad, lane);
        k += kc;
        __syncthreads();
    }
    if (quad) {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            fp[tile_base + w0 + q] = h[q].value();
            members[tile_base + w0 + q] = 0;
        }
    } else {
        for (int64_t w = w0; w < N; w++)                                   // (nothing for a lane past the tile)
            ld_pack_well(pl, L, words, w, tile_base + (size_t)w, rows, fp, members);
    }
}

// ---- the lane's table -----------------------------------------------------------------------------
// claim_or_join with id = global id, equality decided on the packed rows (rows_equal).
// Across wd_lane_dups_add calls in any order: none of the three points of its argument speaks of when a lane
// runs.  The table persists between the calls and is never cleared or rehashed before the finish, so the lanes
// of a later call are to those of an earlier one what late lanes of one launch are to early ones - and the
// order of lanes inside a launch is already arbitrary.  What a comparison reads is fixed before it runs: the packed rows of
// this batch and of every earlier one were written by k_ld_pack launches that ended before this kernel began,
// and no kernel writes a row twice (a tile index is taken once).
__device__ inline bool rows_equal(const uint32_t *__restrict__ rows, int words, uint32_t a, uint32_t b)
{
    const uint32_t *x = rows + (size_t)a * words, *y = rows + (size_t)b * words;
    int k = 0;
    for (; k + kLdCmpWords <= words; k += kLdCmpWords) {
        uint32_t p[kLdCmpWords], q[kLdCmpWords];
#pragma unroll
        for (int j = 0; j < kLdCmpWords; j++) {
            p[j] = x[k + j];
            q[j] = y[k + j];
        }
        uint32_t diff = 0;
#pragma unroll
        for (int j = 0; j < kLdCmpWords; j++)
            diff |= p[j] ^ q[j];
        if (diff)
            return false;
    }
    for (; k < words; k++)
        if (x[k] != y[k])
            return false;
    return true;
}

// grid (ceil(N / 256), n_tiles of the batch); aux[g]: the well's fingerprint in, its slot out (kNoSlot for
// a non-PF well)
__global__ void __launch_bounds__(kTdBlock) k_ld_insert(const uint8_t *const *__restrict__ filt,
                                                         const int *__restrict__ tile_idx, int words, int64_t N,
                                                         const uint32_t *__restrict__ rows, unsigned long long *aux,
                                                         unsigned long long fp_mask, unsigned long long *table,
                                                         unsigned long long slot_mask)
{
    const int tile = blockIdx.y;
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    if (w >= N)
        return;
    const size_t g64 = (size_t)tile_idx[tile] * (size_t)N + (size_t)w;
    if (!(filt[tile][w] & 1u)) {                                       // bcl_direct_reader.py:246
        aux[g64] = kNoSlot;
        return;
    }
    const uint32_t g = (uint32_t)g64;                                  // (max_tiles * N < 2^32 - 1)
    const unsigned long long m = mix64(aux[g64] & fp_mask);
    const unsigned long long tag = m & 0xFFFFFFFF00000000ull;
    aux[g64] = claim_or_join(table, slot_mask, m, tag, g, [=](unsigned long long cur) {             // (>= 2 W slots)
        return (cur & 0xFFFFFFFF00000000ull) == tag && rows_equal(rows, words, g, (uint32_t)cur);
    });
}

// ---- finish ---------------------------------------------------------------------------------------
// All four: grid (ceil(N / 256), tiles added), tile_idx = their tile indices.

// slot -> label, members counted at the representative, PF per tile
__global__ void __launch_bounds__(kTdBlock) k_ld_resolve(const unsigned long long *__restrict__ table,
                                                          const int *__restrict__ tile_idx, int64_t N,
                                                          const unsigned long long *__restrict__ aux,
                                                          uint32_t *__restrict__ label, uint32_t *members,
                                                          uint32_t *const *__restrict__ labels_out,
                                                          unsigned long long *cnt_t)
{
    __shared__ uint32_t s_pf;
    if (threadIdx.x == 0)
        s_pf = 0;
    __syncthreads();
    const int ti = tile_idx[blockIdx.y];
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    const size_t g = (size_t)ti * (size_t)N + (size_t)w;
    uint32_t lab = kInvalid;
    if (w < N) {
        const unsigned long long s = aux[g];
        if (s != kNoSlot)
            lab = (uint32_t)table[s];
        label[g] = lab;
        if (labels_out && labels_out[ti])
            labels_out[ti][w] = lab;
    }
    const uint32_t add = wave_grouped(lab != kInvalid && lab != (uint32_t)g, lab);
    if (add)
        atomicAdd(members + lab, add);
    const unsigned long long pf = __ballot(lab != kInvalid);
    if ((threadIdx.x & (kWave - 1)) == 0 && pf)
        atomicAdd(&s_pf, (uint32_t)__popcll(pf));
    __syncthreads();
    if (threadIdx.x == 0 && s_pf)
        atomicAdd(ld_tile_cnt(cnt_t, ti) + kLdPf, (unsigned long long)s_pf);
}

// Classes, size bins, InLane, LaneRedundant.  A well in a class enters the second table: a slot is
// (label << 32) | the smallest global id of the (label, tile) group seen so far.  The tile of an entry is that of
// the id it holds, so two groups of one class are told apart by where that id lies: claim_or_join again, with
// equality of (label, tile) decided exactly on the word itself.
// aux[g] = the group's slot, kNoSlot for a well in no class.
__global__ void __launch_bounds__(kTdBlock) k_ld_classes(const int *__restrict__ tile_idx, int64_t N,
                                                          const uint32_t *__restrict__ label,
                                                          const uint32_t *__restrict__ members,
                                                          unsigned long long *__restrict__ aux, unsigned long long *table,
                                                          unsigned long long slot_mask, unsigned long long *cnt_t,
                                                          unsigned long long *cnt_l)
{
    __shared__ uint32_t s_sum[3 + kBins];                              // classes, InLane, LaneRedundant, bins
    if (threadIdx.x < 3 + kBins)
        s_sum[threadIdx.x] = 0;
    __syncthreads();
    const int ti = tile_idx[blockIdx.y];
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    const size_t g64 = (size_t)ti * (size_t)N + (size_t)w;
    if (w < N) {
        const uint32_t g = (uint32_t)g64, lab = label[g64];
        const uint32_t m = lab != kInvalid ? members[lab] : 0u;        // (the class has m + 1 wells)
        unsigned long long s = kNoSlot;
        if (m > 0) {
            atomicAdd(&s_sum[1], 1u);
            if (lab == g) {
                atomicAdd(&s_sum[0], 1u);
                atomicAdd(&s_sum[3 + min(m + 1u, (uint32_t)(kBins + 1)) - 2u], 1u);
            } else {
                atomicAdd(&s_sum[2], 1u);
            }
            const unsigned long long base = (unsigned long long)ti * (unsigned long long)N;
            const unsigned long long key = (unsigned long long)lab << 32;
            // (groups <= wells in classes <= W: a free slot comes; & not &&: one branch for the three tests)
            s = claim_or_join(table, slot_mask, mix64(key | (uint32_t)ti), key, g, [=](unsigned long long cur) {
                const unsigned long long id = cur & 0xFFFFFFFFull;
                return ((cur >> 32) == lab) & (id >= base) & (id - base < (unsigned long long)N);
            });
        }
        aux[g64] = s;
    }
    __syncthreads();
    if (threadIdx.x < 3 + kBins && s_sum[threadIdx.x]) {
        const unsigned long long v = s_sum[threadIdx.x];
        const int i = threadIdx.x;
        if (i == 1 || i == 2)
            atomicAdd(ld_tile_cnt(cnt_t, ti) + (i == 1 ? kLdInLane : kLdLaneRed), v);
        else
            atomicAdd(spread_row(cnt_l, 0, kLdLaneCnt) + (i == 0 ? kLdClasses : kLdBins + (i - 3)), v);
    }
}

// Every member of a group but its smallest adds 2^32 to the group's slot: the upper half then holds label +
// members - 1 (mod 2^32), the lower half - all this kernel's loads use - stays the smallest member.
__global__ void __launch_bounds__(kTdBlock) k_ld_span_count(const int *__restrict__ tile_idx, int64_t N,
                                                             const unsigned long long *__restrict__ aux,
                                                             unsigned long long *table)
{
    const int ti = tile_idx[blockIdx.y];
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    const size_t g64 = (size_t)ti * (size_t)N + (size_t)w;
    unsigned long long s = kNoSlot;
    uint32_t gmin = kInvalid;
    if (w < N) {
        s = aux[g64];
        if (s != kNoSlot)
            gmin = (uint32_t)__hip_atomic_load(table + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // (a group has one slot and one smallest member: lanes that name the same one name the same slot)
    const uint32_t add = wave_grouped(s != kNoSlot && gmin != (uint32_t)g64, gmin);
    if (add)
        __hip_atomic_fetch_add(table + s, (unsigned long long)add << 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// At a group's smallest member, n = the others of the group: TileSpans += 1, TileRedundant += n, InTile += n + 1
// if n > 0.  A class's representative is the smallest member of its own tile's group: the class touches
// another tile exactly when that group is smaller than the class.
__global__ void __launch_bounds__(kTdBlock) k_ld_span_sum(const int *__restrict__ tile_idx, int64_t N,
                                                           const unsigned long long *__restrict__ aux,
                                                           const unsigned long long *__restrict__ table,
                                                           const uint32_t *__restrict__ label,
                                                           const uint32_t *__restrict__ members,
                                                           unsigned long long *cnt_t, unsigned long long *cnt_l)
{
    __shared__ unsigned long long s_sum[4];                            // TileSpans, CrossTileClasses, InTile, TileRedundant
    if (threadIdx.x < 4)
        s_sum[threadIdx.x] = 0;
    __syncthreads();
    const int ti = tile_idx[blockIdx.y];
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    const size_t g64 = (size_t)ti * (size_t)N + (size_t)w;
    if (w < N) {
        const unsigned long long s = aux[g64];
        if (s != kNoSlot) {
            const unsigned long long cur = table[s];
            if ((uint32_t)cur == (uint32_t)g64) {
                const uint32_t lab = label[g64];
                const uint32_t n = (uint32_t)(cur >> 32) - lab;
                atomicAdd(&s_sum[0], 1ull);
                if (n) {
                    atomicAdd(&s_sum[2], (unsigned long long)n + 1);
                    atomicAdd(&s_sum[3], (unsigned long long)n);
                }
                if (lab == (uint32_t)g64 && n != members[g64])
                    atomicAdd(&s_sum[1], 1ull);
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_sum[threadIdx.x]) {
        const unsigned long long v = s_sum[threadIdx.x];
        if (threadIdx.x < 2)
            atomicAdd(spread_row(cnt_l, 0, kLdLaneCnt) + (threadIdx.x == 0 ? kLdSpans : kLdCross), v);
        else
            atomicAdd(ld_tile_cnt(cnt_t, ti) + (threadIdx.x == 2 ? kLdInTile : kLdTileRed), v);
    }
}

}  // namespace

#ifndef WD_TILEDUPS_EMU                            // (tools/read_classes_emu.cpp, tools/near_emu.cpp: the kernels above on the CPU, a fiber per lane)
struct wd_lane_index;                              // lane_index.inc: the index part of an accumulator
struct wd_lane_quality;                            // lane_quality.inc: the quality part of an accumulator
struct wd_lane_umi_part;                           // lane_umi.inc: the UMI part of an accumulator

// the host side of an accumulator (the device side is the caller's workspace)
struct wd_lane_dups {
    wd_ctx *ctx;
    int64_t N;
    int max_tiles, L;
    LdLayout lay;
    uint8_t *ws;
    unsigned long long fp_mask;
    std::vector<char> added;                       // by tile index
    bool finished;
    // the classes, once k_ld_resolve has run (lane_near.inc delivers them again after a refusal)
    bool resolved;
    std::vector<int64_t> eq_lane, eq_tiles;
    std::shared_ptr<wd_lane_index> index;          // null unless wd_lane_index_begin has been called
    std::shared_ptr<wd_lane_quality> qual;         // null unless wd_lane_qual_begin has been called
    std::shared_ptr<wd_lane_umi_part> umi;         // null unless wd_lane_umi_begin has been called
    // the molecule part: the caller's region wd_lane_umi_molecules filled last, with its max_e and max_family; null
    // after a call of it that failed and after a later finish of either kind (include/welldup_lanemolecules.h)
    uint8_t *mol = nullptr;
    int mol_e = 0, mol_family = 0;
};

namespace {

int ld_check_labels(wd_lane_dups *ld, uint32_t *const *labels_dev)
{
    if (labels_dev)
        for (int t = 0; t < ld->max_tiles; t++)
            if (labels_dev[t] && ld->N > 0 && !on_device(labels_dev[t]))
                return fail(ld->ctx, WD_ERR_ARG, "lane duplicates: labels must be in device memory");
    return WD_OK;
}

std::vector<int> ld_tiles_added(const wd_lane_dups *ld)
{
    std::vector<int> tiles;
    for (int t = 0; t < ld->max_tiles; t++)
        if (ld->added[t])
            tiles.push_back(t);
    return tiles;
}

// ---- what the accumulator's parts share ------------------------------------------------------------------
// Beside its reads an accumulator carries up to three side parts - the index keys and the UMI keys (lane_index.inc),
// the packed qualities (lane_quality.inc) -, each fed by an add of its own that records the tiles it was given.
// The phrases of a part that do not compose from its head are handed over whole, as LanePass's are (lane_pass.inc).
struct LanePartSay {
    const char *head;                              // "lane index": what the composed messages begin with
    const char *unbegun, *stride, *tables;         // add: the part was never begun, an interleaved layout, a null table
    const char *cycles, *small;                    // begin of a key part: "index" cycles, a workspace too small
};

// What the four adds open with, in the order they have always checked - a call wrong in two ways fails on the same
// one.  added: the part's tiles so far, null for a part never begun; tables: the entry's other tables are there.
// WD_OK with n_tiles > 0: `seen` is `added` with the call's tiles marked, which the entry swaps in once it has succeeded.
int lane_add_open(wd_lane_dups *ld, const std::vector<char> *added, int n_tiles, const int *tile_index, bool tables,
                  const LanePartSay &say, std::vector<char> &seen)
{
    if (!ld || n_tiles < 0)
        return WD_ERR_ARG;
    wd_ctx *ctx = ld->ctx;
    const std::string head = std::string(say.head) + ": ";
    if (!added)
        return fail(ctx, WD_ERR_ARG, say.unbegun);
    if (ld->finished || ld->resolved)                                  // (resolved: a near finish was refused)
        return fail(ctx, WD_ERR_ARG, head + "add after finish");
    if (ctx->well_stride != 1)
        return fail(ctx, WD_ERR_ARG, say.stride);
    if (n_tiles == 0)
        return WD_OK;
    if (!tile_index || !tables)
        return fail(ctx, WD_ERR_ARG, say.tables);
    if (n_tiles > ld->max_tiles)
        return fail(ctx, WD_ERR_ARG, head + "more tiles than the lane has room for");
    seen = *added;
    for (int i = 0; i < n_tiles; i++) {
        const int t = tile_index[i];
        if (t < 0 || t >= ld->max_tiles)
            return fail(ctx, WD_ERR_ARG, head + "tile index " + std::to_string(t) + " out of range");
        if (seen[t])
            return fail(ctx, WD_ERR_ARG, head + "tile index " + std::to_string(t) + " used twice");
        seen[t] = 1;
    }
    return WD_OK;
}

// The part's tiles are the lane's tiles: a pass that reads a part reads it at the wells the finish labelled.
// head: the caller's, what = "index planes", "UMI planes" or "qualities".
int lane_part_tiles(const wd_lane_dups *ld, const std::vector<char> &added, const std::string &head, const std::string &what)
{
    for (int t = 0; t < ld->max_tiles; t++)
        if (added[t] != ld->added[t])
            return fail(ld->ctx, WD_ERR_ARG, head + ": tile index " + std::to_string(t) +
                                                 (ld->added[t] ? " was added without " + what : " got " + what + " but was never added"));
    return WD_OK;
}

// The rows of the label array as it stands (class representatives, or the cluster roots of lane_near.inc, with
// the members counted at them), over the tiles in d_tidx: the table is cleared and keyed by (label, tile),
// k_ld_classes / k_ld_span_count / k_ld_span_sum add to the counters, which come down and are summed.  PF per
// tile is what the counters hold (k_ld_resolve's).  Synchronises the stream.
int ld_count_rows(wd_lane_dups *ld, const std::vector<int> &tiles, int64_t *lane_row, int64_t *tile_rows)
{
    wd_ctx *ctx = ld->ctx;
    const int64_t N = ld->N;
    const int T = ld->max_tiles;
    const LdLayout &lay = ld->lay;
    uint8_t *ws = ld->ws;
    unsigned long long *cnt_t = (unsigned long long *)(ws + lay.cnt_t);
    unsigned long long *cnt_l = (unsigned long long *)(ws + lay.cnt_l);
    std::vector<unsigned long long> h_t((size_t)T * kSpread * kLdTileCnt, 0), h_l((size_t)kSpread * kLdLaneCnt, 0);
    if (!tiles.empty()) {
        int *d_tidx = (int *)(ws + lay.tidx);
        unsigned long long *table = (unsigned long long *)(ws + lay.table);
        unsigned long long *aux = (unsigned long long *)(ws + lay.aux);
        uint32_t *label = (uint32_t *)(ws + lay.label);
        uint32_t *members = (uint32_t *)(ws + lay.members);
        const unsigned long long slot_mask = lay.slots - 1;
        const dim3 wgrid((unsigned)((N + kTdBlock - 1) / kTdBlock), (unsigned)tiles.size());
        WD_HIP(ctx, hipMemsetAsync(table, 0xFF, lay.slots * 8, ctx->stream));        // the second table: every slot free
        hipLaunchKernelGGL(k_ld_classes, wgrid, dim3(kTdBlock), 0, ctx->stream, d_tidx, N, label, members, aux, table,
                           slot_mask, cnt_t, cnt_l);
        hipLaunchKernelGGL(k_ld_span_count, wgrid, dim3(kTdBlock), 0, ctx->stream, d_tidx, N, aux, table);
        hipLaunchKernelGGL(k_ld_span_sum, wgrid, dim3(kTdBlock), 0, ctx->stream, d_tidx, N, aux, table, label, members,
                           cnt_t, cnt_l);
        WD_HIP(ctx, hipGetLastError());
        WD_HIP(ctx, hipMemcpyAsync(h_t.data(), cnt_t, h_t.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        WD_HIP(ctx, hipMemcpyAsync(h_l.data(), cnt_l, h_l.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    WD_HIP(ctx, hipStreamSynchronize(ctx->stream));

    memset(lane_row, 0, WD_LANEDUPS_LANE_COLS * sizeof(int64_t));
    for (int t = 0; t < T; t++) {
        unsigned long long c[kLdTileCnt];
        sum_spread(h_t.data(), (size_t)t, kLdTileCnt, c);
        int64_t *o = tile_rows + (size_t)t * WD_LANEDUPS_TILE_COLS;
        o[0] = (int64_t)c[kLdPf];
        o[1] = (int64_t)c[kLdInLane];
        o[2] = (int64_t)c[kLdInTile];
        o[3] = (int64_t)c[kLdTileRed];
        o[4] = (int64_t)c[kLdLaneRed];
        lane_row[0] += o[0];
        lane_row[2] += o[1];
    }
    unsigned long long c[kLdLaneCnt];
    sum_spread(h_l.data(), 0, kLdLaneCnt, c);
    lane_row[1] = (int64_t)c[kLdClasses];
    lane_row[4] = (int64_t)c[kLdCross];
    lane_row[5] = (int64_t)c[kLdSpans];
    for (int b = 0; b < kBins; b++)
        lane_row[6 + b] = (int64_t)c[kLdBins + b];
    lane_row[3] = lane_row[2] - lane_row[1];
    return WD_OK;
}

// labels_dev[t] = the label array's part of tile index t (all ones for an index never added); not synchronised
int ld_copy_labels(wd_lane_dups *ld, uint32_t *const *labels_dev, bool added_too)
{
    wd_ctx *ctx = ld->ctx;
    const size_t bytes = (size_t)ld->N * 4;
    const uint32_t *label = (const uint32_t *)(ld->ws + ld->lay.label);
    if (labels_dev && bytes)
        for (int t = 0; t < ld->max_tiles; t++) {
            if (!labels_dev[t])
                continue;
            if (!ld->added[t])                                         // a tile index never added has no PF well
                WD_HIP(ctx, hipMemsetAsync(labels_dev[t], 0xFF, bytes, ctx->stream));
            else if (added_too)
                WD_HIP(ctx, hipMemcpyAsync(labels_dev[t], label + (size_t)t * ld->N, bytes, hipMemcpyDeviceToDevice,
                                           ctx->stream));
        }
    return WD_OK;
}

// The classes of the lane: rows to host memory, labels to labels_dev (checked by the caller).  The first call
// resolves the table (k_ld_resolve: from then on the label array holds the class representatives) and keeps the
// rows; a later one - lane_near.inc calls again after a refusal - delivers the same rows and labels from them.
int ld_equality(wd_lane_dups *ld, int64_t *lane_row, int64_t *tile_rows, uint32_t *const *labels_dev)
{
    wd_ctx *ctx = ld->ctx;
    const int64_t N = ld->N;
    const int T = ld->max_tiles;
    const size_t lane_bytes = WD_LANEDUPS_LANE_COLS * sizeof(int64_t);
    const size_t tile_bytes = (size_t)T * WD_LANEDUPS_TILE_COLS * sizeof(int64_t);
    memset(lane_row, 0, lane_bytes);
    memset(tile_rows, 0, tile_bytes);
    if (N == 0 || T == 0)
        return WD_OK;
    if (bind_device(ctx))
        return WD_ERR_HIP;
    if (ld->resolved) {
        memcpy(lane_row, ld->eq_lane.data(), lane_bytes);
        memcpy(tile_rows, ld->eq_tiles.data(), tile_bytes);
        if (const int rc = ld_copy_labels(ld, labels_dev, true))
            return rc;
        WD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return WD_OK;
    }
    if (const int rc = ld_copy_labels(ld, labels_dev, false))
        return rc;
    const std::vector<int> tiles = ld_tiles_added(ld);
    const LdLayout &lay = ld->lay;
    uint8_t *ws = ld->ws;
    if (!tiles.empty()) {
        uint32_t **d_lbl = (uint32_t **)(ws + lay.lbl);
        int *d_tidx = (int *)(ws + lay.tidx);
        if (labels_dev)
            WD_HIP(ctx, hipMemcpyAsync(d_lbl, labels_dev, T * sizeof(void *), hipMemcpyHostToDevice, ctx->stream));
        WD_HIP(ctx, hipMemcpyAsync(d_tidx, tiles.data(), tiles.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        const dim3 wgrid((unsigned)((N + kTdBlock - 1) / kTdBlock), (unsigned)tiles.size());
        hipLaunchKernelGGL(k_ld_resolve, wgrid, dim3(kTdBlock), 0, ctx->stream, (unsigned long long *)(ws + lay.table),
                           d_tidx, N, (unsigned long long *)(ws + lay.aux), (uint32_t *)(ws + lay.label),
                           (uint32_t *)(ws + lay.members), labels_dev ? d_lbl : nullptr,
                           (unsigned long long *)(ws + lay.cnt_t));
    }
    if (const int rc = ld_count_rows(ld, tiles, lane_row, tile_rows))
        return rc;
    ld->eq_lane.assign(lane_row, lane_row + WD_LANEDUPS_LANE_COLS);
    ld->eq_tiles.assign(tile_rows, tile_rows + (size_t)T * WD_LANEDUPS_TILE_COLS);
    ld->resolved = true;
    return WD_OK;
}

}  // namespace

extern "C" {

int wd_lane_dups_workspace(int64_t N, int max_tiles, int L, size_t *bytes)
{
    if (N < 0 || max_tiles < 0 || L < 0 || !bytes)
        return WD_ERR_ARG;
    if (L > kMaxCycles || max_tiles > 65535)
        return WD_ERR_UNSUPPORTED;
    if (N > 0 && (uint64_t)max_tiles >= (0xFFFFFFFFull + (uint64_t)N - 1) / (uint64_t)N)      // max_tiles * N >= 2^32 - 1
        return WD_ERR_UNSUPPORTED;
    *bytes = ld_layout_of(N, max_tiles, L).bytes;
    return WD_OK;
}

int wd_lane_dups_begin(wd_ctx *ctx, int64_t N, int max_tiles, int L, void *workspace_dev, size_t workspace_bytes,
                       int hash_bits, wd_lane_dups **out)
try {
    if (!ctx || !out || hash_bits < 0 || hash_bits > 32)
        return WD_ERR_ARG;
    *out = nullptr;
    size_t need = 0;
    const int rc = wd_lane_dups_workspace(N, max_tiles, L, &need);
    if (rc == WD_ERR_UNSUPPORTED)
        return fail(ctx, rc, "lane duplicates: at most 2^32 - 2 wells, 1024 cycles and 65535 tiles in a lane");
    if (rc != WD_OK)
        return fail(ctx, rc, "lane duplicates: negative size");
    if (!workspace_dev || workspace_bytes < need)
        return fail(ctx, WD_ERR_ARG, "workspace smaller than wd_lane_dups_workspace");
    if (!on_device(workspace_dev))
        return fail(ctx, WD_ERR_ARG, "lane duplicates: the workspace must be in device memory");
    if (bind_device(ctx))
        return WD_ERR_HIP;
    wd_lane_dups *ld = new wd_lane_dups;
    ld->ctx = ctx;
    ld->N = N;
    ld->max_tiles = max_tiles;
    ld->L = L;
    ld->lay = ld_layout_of(N, max_tiles, L);
    ld->ws = (uint8_t *)workspace_dev;
    ld->fp_mask = hash_bits == 0 ? ~0ull : (1ull << hash_bits) - 1;
    ld->added.assign((size_t)max_tiles, 0);
    ld->finished = false;
    ld->resolved = false;
    hipError_t e = hipMemsetAsync(ld->ws + ld->lay.cnt_t, 0, ld->lay.planes - ld->lay.cnt_t, ctx->stream);      // counters
    if (e == hipSuccess)
        e = hipMemsetAsync(ld->ws + ld->lay.table, 0xFF, ld->lay.slots * 8, ctx->stream);                       // every slot free
    if (e == hipSuccess)
        e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        delete ld;
        return fail(ctx, WD_ERR_HIP, std::string("wd_lane_dups_begin: ") + hipGetErrorString(e));
    }
    *out = ld;
    return WD_OK;
} WD_CATCH

int wd_lane_dups_add(wd_lane_dups *ld, int n_tiles, const int *tile_index, const uint8_t *const *planes,
                     const uint8_t *const *filter)
try {
    std::vector<char> seen;
    if (const int rc = lane_add_open(ld, ld ? &ld->added : nullptr, n_tiles, tile_index, filter && (planes || !ld || ld->L <= 0),
                                     {"lane duplicates", nullptr, "lane duplicates read a plane per cycle (well_stride 1)",
                                      "null tile index, plane or filter table"},
                                     seen))
        return rc;
    if (n_tiles == 0)
        return WD_OK;
    wd_ctx *ctx = ld->ctx;
    const int L = ld->L;
    const int64_t N = ld->N;
    bool aligned4;
    if (const int rc = check_tables(ctx, "lane duplicates: ", n_tiles, L, planes, filter, nullptr, &aligned4))
        return rc;
    if (bind_device(ctx))
        return WD_ERR_HIP;
    if (N > 0) {
        const LdLayout &lay = ld->lay;
        uint8_t *ws = ld->ws;
        const uint8_t **d_planes = (const uint8_t **)(ws + lay.planes);
        const uint8_t **d_filt = (const uint8_t **)(ws + lay.filt);
        int *d_tidx = (int *)(ws + lay.tidx);
        uint32_t *rows = (uint32_t *)(ws + lay.rows);
        unsigned long long *aux = (unsigned long long *)(ws + lay.aux);
        if (const int rc = upload_tables(ctx, n_tiles, L, planes, d_planes, filter, d_filt))
            return rc;
        WD_HIP(ctx, hipMemcpyAsync(d_tidx, tile_index, n_tiles * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        const dim3 wgrid((unsigned)((N + kTdBlock - 1) / kTdBlock), (unsigned)n_tiles);
        if (aligned4)
            hipLaunchKernelGGL(k_ld_pack<true>, dim3((unsigned)((N + kLdWaveWells - 1) / kLdWaveWells), (unsigned)n_tiles),
                               dim3(kWave), 0, ctx->stream, d_planes, d_tidx, L, lay.words, N, rows, aux,
                               (uint32_t *)(ws + lay.members));
        else
            hipLaunchKernelGGL(k_ld_pack<false>, wgrid, dim3(kTdBlock), 0, ctx->stream, d_planes, d_tidx, L, lay.words, N,
                               rows, aux, (uint32_t *)(ws + lay.members));
        hipLaunchKernelGGL(k_ld_insert, wgrid, dim3(kTdBlock), 0, ctx->stream, d_filt, d_tidx, lay.words, N, rows, aux,
                           ld->fp_mask, (unsigned long long *)(ws + lay.table), (unsigned long long)(lay.slots - 1));
        WD_HIP(ctx, hipGetLastError());
        // (the pointer tables are the next call's too, and the caller may reuse the planes at once)
        WD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    ld->added.swap(seen);
    return WD_OK;
} WD_CATCH

int wd_lane_dups_finish(wd_lane_dups *ld, int64_t *lane_row, int64_t *tile_rows, uint32_t *const *labels_dev)
try {
    if (ld)
        ld->mol = nullptr;                                             // (the molecule part does not outlive a call of a finish)
    if (!ld || !lane_row || !tile_rows)
        return WD_ERR_ARG;
    wd_ctx *ctx = ld->ctx;
    if (ld->finished)
        return fail(ctx, WD_ERR_ARG, "lane duplicates: finish is called once");
    if (const int rc = ld_check_labels(ld, labels_dev))
        return rc;
    ld->finished = true;
    return ld_equality(ld, lane_row, tile_rows, labels_dev);
} WD_CATCH

void wd_lane_dups_end(wd_lane_dups *ld)
{
    delete ld;
}

}  // extern "C"
#endif
