// lane_index.inc - a lane's classes split by index read (include/welldup_laneindex.h): the wells of a lane grouped
// by the bases of their index cycles, and what the last finish found counted per group.  Included at the end of
// welldup_tiledups.hip: it uses read_classes.inc (plane_pass, mix64, claim_or_join, the spread counters) and
// lane_dups.inc (the accumulator, its label and member arrays, k_ld_span_count); k_li_tally walks LaneRun's runs and
// the counters come back through spread_fetch (lane_pass.inc).
//
// In the caller's index workspace, for W = max_tiles * N wells of capacity: key [W] uint2 (the index read, two words
// of ten 3-bit codes), glabel [W] (the smallest global id of the well's group), cnt [W][5] uint32 (a group's row, at
// its representative).  Everything else lives in regions of the accumulator that are dead after a finish: the
// lane's table, and aux, the 8-byte word per well.
//
// wd_lane_index_add, per batch of tiles (grid y = tile of the batch):
//   k_li_pack        plane_pass over the I index planes; the one or two words are the well's key
// wd_lane_index_finish, over the tiles that were added; the first call runs
//   k_li_group       every PF well into the (cleared) table, keyed by mix64(key); the slot keeps the smallest id
//   k_li_glabel      slot -> group label
//   k_li_sub         (table cleared again) every well in a class enters keyed by (label, group label): the slot keeps
//                    the smallest id of the subgroup - k_ld_classes' (label, tile) scheme with the tile test replaced
//   k_ld_span_count  unchanged: the members of a subgroup counted in the upper half of its slot
//   k_li_tally       the group rows, aggregated in LDS per workgroup, and the lane index row
// and every call
//   k_li_emit        the representatives with PF >= min_pf compacted into a list, the others summed into Other
//   k_li_rows        the listed groups' rows and keys, a chunk at a time, on their way to the host
#include "welldup_laneindex.h"

namespace {

constexpr int kLiCols = WD_LANEINDEX_GROUP_COLS;   // PF, InLane, InGroup, GroupRedundant, Mixed
constexpr int kLiLaneCnt = 8;                      // per copy: the lane index row's counters
constexpr int kLiGroups = 0, kLiSpans = 1, kLiMixedClasses = 2;
constexpr int kLiOtherCnt = 8;                     // per copy: the Other row
constexpr int kLiStage = kLiCols + 1;              // uint64 per listed group on its way to the host: the row, the key

// a key part's share of its workspace (LaneKeyPart below): the plane pointers and the tile indices of an add, the
// keys, and the whole's size
struct LaneKeyLayout {
    size_t planes, tidx, key, bytes;
};

// the index workspace (include/welldup_laneindex.h states the arithmetic)
struct LiLayout {
    size_t cnt_l, other, listed, planes, tidx, key, glabel, cnt, bytes;
};

LiLayout li_layout_of(int64_t N, int max_tiles, int I)
{
    LiLayout l;
    const size_t t = (size_t)max_tiles, wells = (size_t)N * t;
    l.cnt_l = 0;
    l.other = align256(l.cnt_l + (size_t)kSpread * kLiLaneCnt * 8);
    l.listed = align256(l.other + (size_t)kSpread * kLiOtherCnt * 8);
    l.planes = align256(l.listed + 8);
    l.tidx = align256(l.planes + t * (size_t)I * sizeof(void *));
    l.key = align256(l.tidx + t * sizeof(int));
    l.glabel = align256(l.key + wells * 8);
    l.cnt = align256(l.glabel + wells * 4);
    l.bytes = align256(l.cnt + wells * (size_t)kLiCols * 4);
    return l;
}

// ---- pack ---------------------------------------------------------------------------------------
// The key pack of both key parts of an accumulator (LaneKeyPart below): lane_key_add launches it for the index read
// into the index workspace and for the UMI read into the UMI workspace (lane_umi.inc).
// I <= 20 cycles are at most two words of plane_pass: they stay in registers and are stored as the well's key, eight
// bytes a well - a lane of the VEC4 kernel stores 32 consecutive bytes, no staging in LDS is needed.
// VEC4 (every plane 4-byte aligned): grid (ceil(N / 1024), n_tiles of the batch), a lane packs wells 4 i .. 4 i + 3.
// Else: grid (ceil(N / 256), n_tiles), a lane one well.
__device__ inline void li_pack_well(const uint8_t *const *pl, int I, int64_t w, uint2 *__restrict__ key)
{
    uint32_t k0 = 0, k1 = 0;
    plane_pass<false>(pl, 0, I, w, [&](int k, const uint32_t(&acc)[1]) {
        if (k == 0)
            k0 = acc[0];
        else
            k1 = acc[0];
    });
    *key = make_uint2(k0, k1);
}

template <bool VEC4>
__global__ void __launch_bounds__(kTdBlock) k_li_pack(const uint8_t *const *__restrict__ planes,
                                                       const int *__restrict__ tile_idx, int I, int64_t N,
                                                       uint2 *__restrict__ key)
{
    const int tile = blockIdx.y;
    const uint8_t *const *pl = planes + (size_t)tile * I;
    uint2 *out = key + (size_t)tile_idx[tile] * (size_t)N;
    const int64_t i = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    if constexpr (!VEC4) {
        if (i < N)
            li_pack_well(pl, I, i, out + i);
        return;
    }
    const int64_t w0 = 4 * i;
    if (w0 + 4 <= N) {
        uint32_t k0[4] = {0, 0, 0, 0}, k1[4] = {0, 0, 0, 0};
        plane_pass<true>(pl, 0, I, w0, [&](int k, const uint32_t(&acc)[4]) {
            if (k == 0) {
#pragma unroll
                for (int q = 0; q < 4; q++)
                    k0[q] = acc[q];
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++)
                    k1[q] = acc[q];
            }
        });
#pragma unroll
        for (int q = 0; q < 4; q++)
            out[w0 + q] = make_uint2(k0[q], k1[q]);
    } else {
        for (int64_t w = w0; w < N; w++)                               // the last N % 4 wells (nothing past the tile)
            li_pack_well(pl, I, w, out + w);
    }
}

// ---- groups -------------------------------------------------------------------------------------
// All three: grid (ceil(N / 256), tiles added), tile_idx = their tile indices.  A well is PF exactly when the
// finish gave it a label.
//
// claim_or_join with id = global id into the lane's table, dead and cleared; equality is decided on the stored keys
// of the two ids, never on the tag.  Why the outcome does not depend on the order of execution - the argument of
// read_classes.inc, verbatim: a slot is claimed once and never freed, and every id that joins it has been compared
// with its representative and found to have the same key, so all ids a slot ever names belong to one group and a
// stale representative decides a comparison the same way; a load that sees a free slot is followed by the CAS,
// which fails on a slot claimed meanwhile and returns what it holds; every id of a group therefore passes the same
// slots and stops at the first that is free or its own group's: a group has exactly one slot, and the min leaves
// its smallest id there, whichever lane came first.  The keys were written by k_li_pack launches that ended before
// this kernel began.  aux[g] = the slot.
__global__ void __launch_bounds__(kTdBlock) k_li_group(const int *__restrict__ tile_idx, int64_t N,
                                                        const uint32_t *__restrict__ label,
                                                        const uint2 *__restrict__ key, unsigned long long *aux,
                                                        unsigned long long *table, unsigned long long slot_mask)
{
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    if (w >= N)
        return;
    const size_t g64 = (size_t)tile_idx[blockIdx.y] * (size_t)N + (size_t)w;
    if (label[g64] == kInvalid) {
        aux[g64] = kNoSlot;
        return;
    }
    const uint2 mine = key[g64];
    const unsigned long long m = mix64(((unsigned long long)mine.y << 32) | mine.x);
    const unsigned long long tag = m & 0xFFFFFFFF00000000ull;
    aux[g64] = claim_or_join(table, slot_mask, m, tag, (uint32_t)g64, [=](unsigned long long cur) {      // (>= 2 W slots)
        if ((cur & 0xFFFFFFFF00000000ull) != tag)
            return false;
        const uint2 other = key[(uint32_t)cur];
        return other.x == mine.x && other.y == mine.y;
    });
}

// slot -> group label; the group's counters start from zero
__global__ void __launch_bounds__(kTdBlock) k_li_glabel(const int *__restrict__ tile_idx, int64_t N,
                                                         const unsigned long long *__restrict__ aux,
                                                         const unsigned long long *__restrict__ table,
                                                         uint32_t *__restrict__ glabel, uint32_t *__restrict__ cnt)
{
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    if (w >= N)
        return;
    const size_t g64 = (size_t)tile_idx[blockIdx.y] * (size_t)N + (size_t)w;
    const unsigned long long s = aux[g64];
    const uint32_t gl = s != kNoSlot ? (uint32_t)table[s] : kInvalid;
    glabel[g64] = gl;
    if (gl == (uint32_t)g64)
#pragma unroll
        for (int c = 0; c < kLiCols; c++)
            cnt[g64 * kLiCols + c] = 0;
}

// A well in a class enters the table again: a slot is (label << 32) | the smallest global id of the (label, group)
// subgroup seen so far.  The group of an entry is that of the id it holds, so two subgroups of one class are told
// apart by the group label of that id: equality of (label, group) is decided exactly, on the word and on glabel,
// which the kernel before wrote.  aux[g] = the subgroup's slot, kNoSlot for a well in no class.
__global__ void __launch_bounds__(kTdBlock) k_li_sub(const int *__restrict__ tile_idx, int64_t N,
                                                      const uint32_t *__restrict__ label,
                                                      const uint32_t *__restrict__ members,
                                                      const uint32_t *__restrict__ glabel, unsigned long long *aux,
                                                      unsigned long long *table, unsigned long long slot_mask)
{
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    if (w >= N)
        return;
    const size_t g64 = (size_t)tile_idx[blockIdx.y] * (size_t)N + (size_t)w;
    const uint32_t lab = label[g64];
    unsigned long long s = kNoSlot;
    if (lab != kInvalid && members[lab] > 0) {                         // (the class has members + 1 wells)
        const uint32_t gl = glabel[g64];
        const unsigned long long k = (unsigned long long)lab << 32;
        // (subgroups <= wells in classes <= W: a free slot comes)
        s = claim_or_join(table, slot_mask, mix64(k | gl), k, (uint32_t)g64, [=](unsigned long long cur) {
            return (cur >> 32) == lab && glabel[(uint32_t)cur] == gl;
        });
    }
    aux[g64] = s;
}

// ---- tally --------------------------------------------------------------------------------------
// Every PF well adds up to five ones to the row of its group, and a lane of 96 libraries has 5 M wells for each of
// ~100 rows (a single-index lane 480 M for one): added to memory one by one they would queue on a handful of
// addresses (4.3 M adds to one word: 49 ms, read_classes.inc).  So a workgroup takes a run of kLaneRun consecutive
// wells of a tile (LaneRun, lane_pass.inc) and adds them up in LDS first:
//   - within a wave the lanes of the first active lane's group are counted by ballots and added once, by that
//     lane (the wave-grouped add, for five columns at a time): a single-index lane costs a wave one LDS add per
//     column, not 64 on one LDS word;
//   - the LDS table is open addressing keyed by group label, kLiSlots entries of {label, PF, the four class
//     columns as 16-bit fields of one uint64}: 16 bytes an entry, 8 KB, so that eight workgroups - all 2048 lanes -
//     fit the 160 KB of a CU with room to spare, and 512 entries hold the few hundred libraries of a pool plus the
//     keys with a sequencing error that a run of 8192 wells brings (a few per cent of it);
//   - a field counts at most kLaneRun = 8192 < 2^16 wells, so no field carries into the next;
//   - an add that finds kLiProbe entries in a row taken by other groups goes to the group's row in memory at once
//     (it is already wave-grouped), so the result is exact whatever the number of groups;
//   - at the end an occupied entry is flushed with one global atomic per column that is not zero.
// The lane index row goes through registers, LDS and the kSpread copies.
constexpr int kLiSlots = 512;
constexpr int kLiProbe = 8;
static_assert(kLaneRun < 65536, "a 16-bit field must hold a run's wells");
static_assert((kLiSlots & (kLiSlots - 1)) == 0, "the LDS table is a power of two");

// the entry of the LDS table at which the probes of group gl begin
__device__ inline uint32_t li_home(uint32_t gl) { return (gl * 0x9E3779B1u) >> 23 & (kLiSlots - 1); }

__device__ inline void li_add_row(uint32_t *row, uint32_t pf, unsigned long long cls)
{
    if (pf)
        atomicAdd(row, pf);
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const uint32_t v = (uint32_t)(cls >> (16 * c)) & 0xFFFFu;
        if (v)
            atomicAdd(row + 1 + c, v);
    }
}

// LaneRun's grid and walk
__global__ void __launch_bounds__(kTdBlock) k_li_tally(const int *__restrict__ tile_idx, int64_t N,
                                                        const uint32_t *__restrict__ label,
                                                        const uint32_t *__restrict__ members,
                                                        const uint32_t *__restrict__ glabel,
                                                        const unsigned long long *__restrict__ aux,
                                                        const unsigned long long *__restrict__ table, uint32_t *cnt,
                                                        unsigned long long *cnt_l)
{
    __shared__ uint32_t s_key[kLiSlots], s_pf[kLiSlots];
    __shared__ unsigned long long s_cls[kLiSlots];
    __shared__ uint32_t s_lane[3];                                     // Groups, GroupSpans, MixedClasses
    for (int e = threadIdx.x; e < kLiSlots; e += kTdBlock) {
        s_key[e] = kInvalid;
        s_pf[e] = 0;
        s_cls[e] = 0;
    }
    if (threadIdx.x < 3)
        s_lane[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t groups = 0, spans = 0, mixed_classes = 0;
    LaneRun(tile_idx, N).walk([&](bool has, int64_t, size_t g64) {
        bool pf = false, in_lane = false, in_group = false, redundant = false, mixed = false;
        uint32_t gl = kInvalid;
        if (has) {
            const uint32_t g = (uint32_t)g64, lab = label[g64];
            if (lab != kInvalid) {
                pf = true;
                gl = glabel[g64];
                groups += gl == g;
                const unsigned long long s = aux[g64];
                if (s != kNoSlot) {
                    const unsigned long long cur = table[s];
                    const uint32_t n = (uint32_t)(cur >> 32) - lab;    // the others of the subgroup (k_ld_span_count)
                    in_lane = true;
                    in_group = n > 0;
                    redundant = (uint32_t)cur != g;
                    mixed = n != members[lab];                         // the subgroup is smaller than the class
                    spans += !redundant;
                    mixed_classes += lab == g && mixed;
                }
            }
        }
        // the wave-grouped add: the first active lane's group by ballots, every other lane its own ones
        uint32_t add_pf = pf;
        unsigned long long add_cls = (unsigned long long)in_lane | (unsigned long long)in_group << 16 |
                                     (unsigned long long)redundant << 32 | (unsigned long long)mixed << 48;
        const unsigned long long act = __ballot(pf);
        if (act) {
            const int leader = __ffsll((long long)act) - 1;
            const uint32_t gl0 = (uint32_t)__shfl((int)gl, leader);
            const bool same = pf && gl == gl0;
            const unsigned long long n_pf = __popcll(__ballot(same)), n_lane = __popcll(__ballot(same && in_lane)),
                                     n_grp = __popcll(__ballot(same && in_group)),
                                     n_red = __popcll(__ballot(same && redundant)),
                                     n_mix = __popcll(__ballot(same && mixed));
            if (lane == leader) {
                add_pf = (uint32_t)n_pf;
                add_cls = n_lane | n_grp << 16 | n_red << 32 | n_mix << 48;
            } else if (same) {
                add_pf = 0;
            }
        }
        if (add_pf) {
            uint32_t e = li_home(gl);
            int p = 0;
            for (; p < kLiProbe; p++, e = (e + 1) & (kLiSlots - 1)) {
                const uint32_t old = atomicCAS(&s_key[e], kInvalid, gl);
                if (old == kInvalid || old == gl)
                    break;
            }
            if (p < kLiProbe) {
                atomicAdd(&s_pf[e], add_pf);
                if (add_cls)
                    atomicAdd(&s_cls[e], add_cls);
            } else {
                li_add_row(cnt + (size_t)gl * kLiCols, add_pf, add_cls);
            }
        }
    });
    if (groups)
        atomicAdd(&s_lane[0], groups);
    if (spans)
        atomicAdd(&s_lane[1], spans);
    if (mixed_classes)
        atomicAdd(&s_lane[2], mixed_classes);
    __syncthreads();
    for (int e = threadIdx.x; e < kLiSlots; e += kTdBlock)
        if (s_key[e] != kInvalid)
            li_add_row(cnt + (size_t)s_key[e] * kLiCols, s_pf[e], s_cls[e]);
    if (threadIdx.x < 3 && s_lane[threadIdx.x])
        atomicAdd(spread_row(cnt_l, 0, kLiLaneCnt) + threadIdx.x, (unsigned long long)s_lane[threadIdx.x]);
}

// ---- emit ---------------------------------------------------------------------------------------
// grid (ceil(N / 256), tiles added).  A representative with PF >= min_pf takes a place in the list: the places of a
// wave are claimed with one atomic, a lane's place among them is the number of listed lanes below it (ballot,
// mbcnt).  The list has room for every well, so the count is exact when it exceeds the caller's cap.  The other
// representatives are summed into Other.
__global__ void __launch_bounds__(kTdBlock) k_li_emit(const int *__restrict__ tile_idx, int64_t N,
                                                       const uint32_t *__restrict__ glabel,
                                                       const uint32_t *__restrict__ cnt, unsigned long long min_pf,
                                                       uint32_t *__restrict__ list, unsigned long long *n_listed,
                                                       unsigned long long *other)
{
    __shared__ unsigned long long s_other[kLiCols];
    if (threadIdx.x < kLiCols)
        s_other[threadIdx.x] = 0;
    __syncthreads();
    const int64_t w = (int64_t)blockIdx.x * kTdBlock + threadIdx.x;
    const size_t g64 = (size_t)tile_idx[blockIdx.y] * (size_t)N + (size_t)w;
    const bool rep = w < N && glabel[g64] == (uint32_t)g64;
    const uint32_t *row = cnt + g64 * kLiCols;
    const bool listed = rep && row[0] >= min_pf;
    const unsigned long long ballot = __ballot(listed);
    if (ballot) {
        const int lane = threadIdx.x & (kWave - 1), leader = __ffsll((long long)ballot) - 1;
        unsigned long long first = 0;
        if (lane == leader)
            first = atomicAdd(n_listed, (unsigned long long)__popcll(ballot));
        first = __shfl(first, leader);
        if (listed)
            list[first + __builtin_amdgcn_mbcnt_hi((uint32_t)(ballot >> 32),
                                                   __builtin_amdgcn_mbcnt_lo((uint32_t)ballot, 0u))] = (uint32_t)g64;
    }
    if (rep && !listed)
#pragma unroll
        for (int c = 0; c < kLiCols; c++)
            if (row[c])
                atomicAdd(&s_other[c], (unsigned long long)row[c]);
    __syncthreads();
    if (threadIdx.x < kLiCols && s_other[threadIdx.x])
        atomicAdd(spread_row(other, 0, kLiOtherCnt) + threadIdx.x, s_other[threadIdx.x]);
}

// grid (ceil(n / 256)): stage[i] = the row and the key of the group list[i]
__global__ void __launch_bounds__(kTdBlock) k_li_rows(const uint32_t *__restrict__ list, unsigned long long n,
                                                       const uint32_t *__restrict__ cnt, const uint2 *__restrict__ key,
                                                       unsigned long long *__restrict__ stage)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * kTdBlock + threadIdx.x;
    if (i >= n)
        return;
    const uint32_t g = list[i];
#pragma unroll
    for (int c = 0; c < kLiCols; c++)
        stage[i * kLiStage + c] = cnt[(size_t)g * kLiCols + c];
    const uint2 k = key[g];
    stage[i * kLiStage + kLiCols] = ((unsigned long long)k.y << 32) | k.x;
}

}  // namespace

#ifndef WD_LANE_INDEX_EMU                          // (tools/lane_index_emu.cpp: the kernels above on the CPU, a fiber per lane)
// ---- the key part -----------------------------------------------------------------------------------------
// An accumulator's index part and its UMI part (lane_umi.inc) are one thing twice: a key of up to two words per well,
// packed by k_li_pack from the planes of 1 .. WD_LANEINDEX_MAX_CYCLES cycles into a workspace of the caller's that
// holds the two pointer tables of an add and the key array.  This is the host side of it; the four entries
// wd_lane_index_begin / _add and wd_lane_umi_begin / _add hand their phrases to the two bodies below.
struct LaneKeyPart {
    int cycles = 0;
    LaneKeyLayout at = {};
    uint8_t *ws = nullptr;
    std::vector<char> added;                       // by tile index: planes given
};

// the index part of an accumulator: the key part, and the groups' side of the index workspace
struct wd_lane_index : LaneKeyPart {
    LiLayout lay;
    bool tallied = false;                          // the group rows stand at the representatives
    int64_t groups = 0, spans = 0, mixed_classes = 0;
};

namespace {

LaneKeyLayout li_key_layout_of(int64_t N, int max_tiles, int I)
{
    const LiLayout l = li_layout_of(N, max_tiles, I);
    return {l.planes, l.tidx, l.key, l.bytes};
}

// wd_lane_index_begin and wd_lane_umi_begin: `slot` is the part's place in the accumulator, which gets a new part.
template <class Part>
int lane_key_begin(wd_lane_dups *ld, std::shared_ptr<Part> wd_lane_dups::*slot, int cycles, int max_cycles,
                   LaneKeyLayout (*layout_of)(int64_t, int, int), void *workspace_dev, size_t workspace_bytes,
                   const LanePartSay &say)
{
    if (!ld)
        return WD_ERR_ARG;
    wd_ctx *ctx = ld->ctx;
    const std::string head = std::string(say.head) + ": ";
    if (cycles < 1 || cycles > max_cycles)
        return fail(ctx, WD_ERR_ARG, head + "1.." + std::to_string(max_cycles) + " " + say.cycles + " cycles, not " +
                                         std::to_string(cycles));
    if (ld->finished || ld->resolved)
        return fail(ctx, WD_ERR_ARG, head + "begin after finish");
    if (ld->*slot)
        return fail(ctx, WD_ERR_ARG, head + "begin is called once");
    const LaneKeyLayout lay = layout_of(ld->N, ld->max_tiles, cycles);
    if (!workspace_dev || workspace_bytes < lay.bytes)
        return fail(ctx, WD_ERR_ARG, say.small);
    if (!on_device(workspace_dev))
        return fail(ctx, WD_ERR_ARG, head + "the workspace must be in device memory");
    auto part = std::make_shared<Part>();
    part->cycles = cycles;
    part->at = lay;
    part->ws = (uint8_t *)workspace_dev;
    part->added.assign((size_t)ld->max_tiles, 0);
    ld->*slot = part;
    return WD_OK;
}

// wd_lane_index_add and wd_lane_umi_add: the keys of a batch of tiles.  part: null when the part was never begun.
int lane_key_add(wd_lane_dups *ld, LaneKeyPart *part, int n_tiles, const int *tile_index, const uint8_t *const *planes,
                 const LanePartSay &say)
{
    std::vector<char> seen;
    if (const int rc = lane_add_open(ld, part ? &part->added : nullptr, n_tiles, tile_index, planes != nullptr, say, seen))
        return rc;
    if (n_tiles == 0)
        return WD_OK;
    wd_ctx *ctx = ld->ctx;
    const int64_t N = ld->N;
    const int I = part->cycles;
    bool aligned4 = true;
    for (size_t i = 0; i < (size_t)n_tiles * I; i++) {
        if (!planes[i])
            return fail(ctx, WD_ERR_ARG, "null plane pointer");
        aligned4 = aligned4 && ((uintptr_t)planes[i] & 3u) == 0;
    }
    for (int i = 0; i < n_tiles; i++)
        if (N > 0 && !on_device(planes[(size_t)i * I]))
            return fail(ctx, WD_ERR_ARG, std::string(say.head) + ": planes must be in device memory");
    if (bind_device(ctx))
        return WD_ERR_HIP;
    if (N > 0) {
        const uint8_t **d_planes = (const uint8_t **)(part->ws + part->at.planes);
        int *d_tidx = (int *)(part->ws + part->at.tidx);
        uint2 *key = (uint2 *)(part->ws + part->at.key);
        WD_HIP(ctx, hipMemcpyAsync(d_planes, planes, (size_t)n_tiles * I * sizeof(void *), hipMemcpyHostToDevice, ctx->stream));
        WD_HIP(ctx, hipMemcpyAsync(d_tidx, tile_index, n_tiles * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        if (aligned4)
            hipLaunchKernelGGL(k_li_pack<true>, dim3((unsigned)((N + 4 * kTdBlock - 1) / (4 * kTdBlock)), (unsigned)n_tiles),
                               dim3(kTdBlock), 0, ctx->stream, d_planes, d_tidx, I, N, key);
        else
            hipLaunchKernelGGL(k_li_pack<false>, dim3((unsigned)((N + kTdBlock - 1) / kTdBlock), (unsigned)n_tiles),
                               dim3(kTdBlock), 0, ctx->stream, d_planes, d_tidx, I, N, key);
        WD_HIP(ctx, hipGetLastError());
        // (the pointer tables are the next call's too, and the caller may reuse the planes at once)
        WD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    part->added.swap(seen);
    return WD_OK;
}

const LanePartSay kLiSay = {"lane index", "lane index: add before wd_lane_index_begin",
                            "lane index reads a plane per cycle (well_stride 1)", "null tile index or plane table",
                            "index", "workspace smaller than wd_lane_index_workspace"};

// Groups, subgroups and the tally, once: the labels cannot change after a successful finish.
int li_tally(wd_lane_dups *ld, const std::vector<int> &tiles)
{
    wd_ctx *ctx = ld->ctx;
    wd_lane_index *li = ld->index.get();
    const int64_t N = ld->N;
    const LdLayout &lay = ld->lay;
    uint8_t *ws = ld->ws, *iws = li->ws;
    int *d_tidx = (int *)(iws + li->lay.tidx);
    unsigned long long *table = (unsigned long long *)(ws + lay.table);
    unsigned long long *aux = (unsigned long long *)(ws + lay.aux);
    const uint32_t *label = (const uint32_t *)(ws + lay.label);
    const uint32_t *members = (const uint32_t *)(ws + lay.members);
    const uint2 *key = (const uint2 *)(iws + li->lay.key);
    uint32_t *glabel = (uint32_t *)(iws + li->lay.glabel);
    uint32_t *cnt = (uint32_t *)(iws + li->lay.cnt);
    unsigned long long *cnt_l = (unsigned long long *)(iws + li->lay.cnt_l);
    const unsigned long long slot_mask = lay.slots - 1;
    const dim3 wgrid((unsigned)((N + kTdBlock - 1) / kTdBlock), (unsigned)tiles.size()), blk(kTdBlock);
    const dim3 rgrid((unsigned)((N + kLaneRun - 1) / kLaneRun), (unsigned)tiles.size());

    WD_HIP(ctx, hipMemcpyAsync(d_tidx, tiles.data(), tiles.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    WD_HIP(ctx, hipMemsetAsync(cnt_l, 0, (size_t)kSpread * kLiLaneCnt * 8, ctx->stream));
    WD_HIP(ctx, hipMemsetAsync(table, 0xFF, lay.slots * 8, ctx->stream));            // the groups' table: every slot free
    hipLaunchKernelGGL(k_li_group, wgrid, blk, 0, ctx->stream, d_tidx, N, label, key, aux, table, slot_mask);
    hipLaunchKernelGGL(k_li_glabel, wgrid, blk, 0, ctx->stream, d_tidx, N, aux, table, glabel, cnt);
    WD_HIP(ctx, hipMemsetAsync(table, 0xFF, lay.slots * 8, ctx->stream));            // the subgroups' table
    hipLaunchKernelGGL(k_li_sub, wgrid, blk, 0, ctx->stream, d_tidx, N, label, members, glabel, aux, table, slot_mask);
    hipLaunchKernelGGL(k_ld_span_count, wgrid, blk, 0, ctx->stream, d_tidx, N, aux, table);
    hipLaunchKernelGGL(k_li_tally, rgrid, blk, 0, ctx->stream, d_tidx, N, label, members, glabel, aux, table, cnt, cnt_l);
    WD_HIP(ctx, hipGetLastError());
    SpreadFetch f_l(cnt_l, 1, kLiLaneCnt);
    unsigned long long c[kLiLaneCnt];
    if (const int rc = spread_fetch(ctx, {&f_l}))
        return rc;
    f_l.sum(0, c);
    li->groups = (int64_t)c[kLiGroups];
    li->spans = (int64_t)c[kLiSpans];
    li->mixed_classes = (int64_t)c[kLiMixedClasses];
    li->tallied = true;
    return WD_OK;
}

}  // namespace

extern "C" {

int wd_lane_index_workspace(int64_t N, int max_tiles, int I, size_t *bytes)
{
    size_t ws = 0;
    if (!bytes)
        return WD_ERR_ARG;
    if (const int rc = wd_lane_dups_workspace(N, max_tiles, I, &ws))       // (the limits of a lane, with I for L)
        return rc;
    if (I < 1 || I > WD_LANEINDEX_MAX_CYCLES)
        return WD_ERR_ARG;
    *bytes = li_layout_of(N, max_tiles, I).bytes;
    return WD_OK;
}

int wd_lane_index_begin(wd_lane_dups *ld, int I, void *workspace_dev, size_t workspace_bytes)
try {
    if (const int rc = lane_key_begin(ld, &wd_lane_dups::index, I, WD_LANEINDEX_MAX_CYCLES, li_key_layout_of, workspace_dev,
                                      workspace_bytes, kLiSay))
        return rc;
    ld->index->lay = li_layout_of(ld->N, ld->max_tiles, I);
    return WD_OK;
} WD_CATCH

int wd_lane_index_add(wd_lane_dups *ld, int n_tiles, const int *tile_index, const uint8_t *const *index_planes)
try {
    return lane_key_add(ld, ld ? ld->index.get() : nullptr, n_tiles, tile_index, index_planes, kLiSay);
} WD_CATCH

int wd_lane_index_finish(wd_lane_dups *ld, int64_t min_pf, int64_t cap, int64_t *lane_index_row, int64_t *other_row,
                         int64_t *group_rows, uint64_t *group_keys, int64_t *n_listed)
try {
    if (!ld || !lane_index_row || !other_row || !n_listed || cap < 0 || (cap > 0 && (!group_rows || !group_keys)))
        return WD_ERR_ARG;
    wd_ctx *ctx = ld->ctx;
    wd_lane_index *li = ld->index.get();
    if (!li)
        return fail(ctx, WD_ERR_ARG, "lane index: finish before wd_lane_index_begin");
    if (!ld->finished)
        return fail(ctx, WD_ERR_ARG, "lane index: finish comes after a successful finish of the lane");
    if (const int rc = lane_part_tiles(ld, li->added, "lane index", "index planes"))
        return rc;
    const std::vector<int> tiles = ld_tiles_added(ld);
    const int64_t N = ld->N;
    unsigned long long h_other[kLiOtherCnt] = {0}, listed = 0;
    std::vector<unsigned long long> h_stage;
    if (N > 0 && !tiles.empty()) {
        if (bind_device(ctx))
            return WD_ERR_HIP;
        if (!li->tallied)
            if (const int rc = li_tally(ld, tiles))
                return rc;
        const LdLayout &lay = ld->lay;
        uint8_t *iws = li->ws;
        int *d_tidx = (int *)(iws + li->lay.tidx);
        const uint2 *key = (const uint2 *)(iws + li->lay.key);
        const uint32_t *glabel = (const uint32_t *)(iws + li->lay.glabel);
        const uint32_t *cnt = (const uint32_t *)(iws + li->lay.cnt);
        unsigned long long *other = (unsigned long long *)(iws + li->lay.other);
        unsigned long long *d_listed = (unsigned long long *)(iws + li->lay.listed);
        // the table's bytes once more: the list (a uint32 per well of capacity), behind it the rows on their way out
        const size_t wells = (size_t)N * (size_t)ld->max_tiles, stage_at = align256(wells * 4);
        uint32_t *list = (uint32_t *)(ld->ws + lay.table);
        unsigned long long *stage = (unsigned long long *)(ld->ws + lay.table + stage_at);
        const size_t chunk = (lay.slots * 8 - stage_at) / (kLiStage * 8);              // (>= 5: 8 S >= max(512, 16 W))
        const dim3 wgrid((unsigned)((N + kTdBlock - 1) / kTdBlock), (unsigned)tiles.size()), blk(kTdBlock);
        WD_HIP(ctx, hipMemsetAsync(other, 0, li->lay.planes - li->lay.other, ctx->stream));      // Other and the count
        hipLaunchKernelGGL(k_li_emit, wgrid, blk, 0, ctx->stream, d_tidx, N, glabel, cnt,
                           (unsigned long long)std::max<int64_t>(min_pf, 0), list, d_listed, other);
        WD_HIP(ctx, hipGetLastError());
        SpreadFetch f_o(other, 1, kLiOtherCnt);
        WD_HIP(ctx, hipMemcpyAsync(&listed, d_listed, 8, hipMemcpyDeviceToHost, ctx->stream));
        if (const int rc = spread_fetch(ctx, {&f_o}))
            return rc;
        f_o.sum(0, h_other);
        if (listed <= (unsigned long long)cap) {
            h_stage.resize((size_t)listed * kLiStage);
            for (size_t off = 0; off < listed; off += chunk) {
                const size_t n = std::min<size_t>(chunk, listed - off);
                hipLaunchKernelGGL(k_li_rows, dim3((unsigned)((n + kTdBlock - 1) / kTdBlock)), blk, 0, ctx->stream, list + off,
                                   (unsigned long long)n, cnt, key, stage);
                WD_HIP(ctx, hipGetLastError());
                WD_HIP(ctx, hipMemcpyAsync(h_stage.data() + off * kLiStage, stage, n * kLiStage * 8, hipMemcpyDeviceToHost,
                                           ctx->stream));
                WD_HIP(ctx, hipStreamSynchronize(ctx->stream));
            }
        }
    }
    *n_listed = (int64_t)listed;
    if (listed > (unsigned long long)cap)
        return fail(ctx, WD_ERR_UNSUPPORTED, "lane index: " + std::to_string(listed) + " groups of at least " +
                                                 std::to_string(min_pf) + " PF wells, room for " + std::to_string(cap));
    int64_t mixed_wells = h_other[4];
    for (size_t i = 0; i < listed; i++) {
        for (int c = 0; c < kLiCols; c++)
            group_rows[i * kLiCols + c] = (int64_t)h_stage[i * kLiStage + c];
        group_keys[i] = h_stage[i * kLiStage + kLiCols];
        mixed_wells += group_rows[i * kLiCols + 4];
    }
    for (int c = 0; c < kLiCols; c++)
        other_row[c] = (int64_t)h_other[c];
    lane_index_row[0] = li->groups;
    lane_index_row[1] = (int64_t)listed;
    lane_index_row[2] = li->spans;
    lane_index_row[3] = li->mixed_classes;
    lane_index_row[4] = mixed_wells;
    return WD_OK;
} WD_CATCH

}  // extern "C"
#endif
