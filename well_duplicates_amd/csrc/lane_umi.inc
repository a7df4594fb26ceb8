// lane_umi.inc - a lane's duplicates split by molecular identifier (include/welldup_laneumi.h): the wells of every
// family the last finish left grouped by their UMI read, and the molecules counted.  Included from welldup_tiledups.hip
// after lane_consensus.inc: it uses read_classes.inc (the spread counters), near_core.inc (tn_find, tn_unite),
// lane_dups.inc (the accumulator, its label and members), lane_pass.inc, lane_index.inc (k_li_pack: the UMI read is
// packed as an index read is, by the same kernel), lane_mismatch.inc (lm_fold) and lane_consensus.inc (k_lc_reserve,
// k_lc_scatter, lc_member, lc_wave_sync: the families are gathered as the consensus pass gathers them, by the same
// kernels).
//
// wd_lane_umi_add, per batch of tiles: k_li_pack over the U UMI planes into the UMI workspace's key array.
// wd_lane_umi: four launches on the context's stream and nothing but integer adds between them.  They read label,
// members and the UMI keys and write the caller's scratch only - not the accumulator's table, which is the index
// part's after a finish.
//
//   k_lu_pairs    LaneRun's grid.  Most families are pairs, and a pair needs no list: the copy of a family of two
//                 loads its own key and its root's, decides d <= E and accounts for both wells.
//   k_lc_reserve, k_lc_scatter   as wd_lane_consensus launches them (max_family may be 2: then nothing is gathered).
//                 Their pair and large counters land in a counter block of this scratch that is theirs alone: it gives
//                 LargeFamilies and LargeWells.
//   k_lu_group    a fixed grid; one wave per gathered family of three or more wells, dealt out by wave number as
//                 k_lc_vote deals them.
//
// Why the result is exact and does not depend on the order of execution.  A family's range is a permutation of its
// copies, whatever the schedule (lane_consensus.inc).  A molecule is a connected component of the family's wells under
// "d <= E", which is a property of the set of wells; its first well is the smallest global id in it, never a place in
// the list.  In a family of up to 64 wells every lane's label converges to the smallest global id reachable from its
// well - the rounds are those of a label propagation, which has one fixed point.  In a larger one the union-find is
// near_core.inc's on member numbers: a successful compare-and-swap hooks a root under a smaller root of another tree,
// so the components are those of the edges whatever the order of the unions; which member number ends up the root of
// a component does depend on where the members landed in the list, and nothing is counted of it - each component's
// smallest global id and size are gathered at it by an atomic minimum and adds.  Every output is a sum over families,
// molecules or wells of such values: integer adds, which commute.
//
// wd_lane_umi_molecules (include/welldup_lanemolecules.h): the same four launches with k_lu_pairs_mol and k_lu_group_mol
// in the places of k_lu_pairs and k_lu_group - the same device bodies, instantiated with kEmit -, which also write the
// caller's mol and molmem, a word per well each: the molecule's first well, and at that well the molecule's other
// wells, in the form the finish leaves label and members, so that k_lk_score and k_lk_mark (lane_keep.inc) run on them
// as they stand.  Who writes which word - every word of both arrays is written in a call exactly once, so the region
// may hold anything before and nothing clears it:
//   - a well of a tile never added: a memset of the tile's part of each array, queued by the host;
//   - a well of a pair (a family of two): the lane of k_lu_pairs_mol that walks the COPY, which holds both keys and d.
//     It writes both wells' entries; the lane that walks the pair's root writes nothing;
//   - a well of a gathered family of 3 .. max_family wells: the lane of k_lu_group_mol that holds the member - a
//     family is one wave's, its range holds each member once (lane_consensus.inc), and a member is one lane's in the
//     closure (n <= 64) and in the last loop (n > 64).  The lane of k_lu_pairs_mol that walks it writes nothing;
//   - every other well of an added tile - not PF, Single, or of a Large family -: the lane of k_lu_pairs_mol that
//     walks it (a well of a run is walked by one lane of one workgroup).
// The four cases partition the wells by label and members[label] alone, which no launch of the call writes, so two
// launches never disagree about whose a well is.  Why the values are exact and do not depend on the order of
// execution: a pair's entries are a function of its two keys; in a family of up to 64 wells the label a lane ends with
// is the fixed point said above and the size a popcount over the wave; in a larger one mn[r] and sz[r] are final
// after the wave has met, whichever member number r is.  A molecule's first well has its smallest id, and a Large
// family's root the smallest of the family, so "a root has the smallest id of its family" (lane_keep.inc) holds for
// molecules too.
#include "welldup_lanemolecules.h"

namespace {

constexpr int kLuMaxE = WD_LANEUMI_MAX_E;
constexpr int kLuMaxFamily = WD_LANEUMI_MAX_FAMILY;
constexpr int kLuBins = WD_LANEUMI_BINS;
constexpr int kLuTileCnt = WD_LANEUMI_TILE_COLS;   // per tile and copy: Wells, UmiRedundant, Lone
constexpr int kLuLaneCnt = 32;                     // per copy: the six below, then the two histograms
constexpr int kLuFamilies = 0, kLuMolecules = 1, kLuDistinct = 2, kLuSplitFamilies = 3, kLuSplitWells = 4, kLuWithN = 5,
              kLuPerFamily = 6, kLuSize = kLuPerFamily + kLuBins;
static_assert(kLuSize + kLuBins <= kLuLaneCnt, "the lane's counters: six and two histograms");
static_assert(WD_LANEUMI_LANE_COLS == kLuTileCnt + 8 + 2 * kLuBins, "the lane row of welldup_laneumi.h");
static_assert(kLuMaxFamily <= kLcMaxFamily, "the families are gathered by k_lc_reserve and k_lc_scatter");
static_assert(WD_LANEUMI_MAX_CYCLES == WD_LANEINDEX_MAX_CYCLES, "the UMI read is packed by k_li_pack");
constexpr int kLuWaves = kTdBlock / kWave;         // families a workgroup has in hand
constexpr int kLuGroups = 2048;                    // workgroups of k_lu_group at most
// A workgroup's LDS: per wave the union-find of a family of more than 64 wells - the parent, the smallest global id
// and the size of a component, a word per member each: 3 x 1024 x 4 = 12 KB -, 48 KB for the four waves, and the two
// histograms, 64 bytes.  Three workgroups - 12 waves - fit a CU's 160 KB.  The families of up to 64 wells, which are
// nearly all, do not touch it: they pay for it in waves in flight (the pass is a chain of dependent loads per
// family: table, slot and members, the list, the keys).  A grouping kernel of its own for the large families would
// give the small ones their occupancy back; it has not been tried.
static_assert(kLuWaves * 3 * kLuMaxFamily * 4 + 2 * kLuBins * 4 <= 53 * 1024, "three workgroups per CU");

// the UMI workspace (include/welldup_laneumi.h states the arithmetic): the index workspace without its counters in front
LaneKeyLayout lu_ws_layout_of(int64_t N, int max_tiles, int U)
{
    LaneKeyLayout l;
    const size_t t = (size_t)max_tiles, wells = (size_t)N * t;
    l.planes = 0;
    l.tidx = align256(l.planes + t * (size_t)U * sizeof(void *));
    l.key = align256(l.tidx + t * sizeof(int));
    l.bytes = align256(l.key + wells * 8);
    return l;
}

// the scratch of a call
struct LuLayout {
    size_t cnt_t, cnt_l, cnt_r, cursor, tidx, slot, region, bytes;
    size_t cleared;                                // what a call clears: everything before slot
};

LuLayout lu_layout_of(int max_tiles, int64_t N)
{
    LuLayout l;
    const size_t t = (size_t)max_tiles, wells = t * (size_t)N;
    l.cnt_t = 0;
    l.cnt_l = align256(l.cnt_t + t * kSpread * kLuTileCnt * 8);
    l.cnt_r = align256(l.cnt_l + (size_t)kSpread * kLuLaneCnt * 8);      // k_lc_reserve's: kLcLaneCnt counters per copy
    l.cursor = align256(l.cnt_r + (size_t)kSpread * kLcLaneCnt * 8);
    l.tidx = align256(l.cursor + 8);
    l.slot = align256(l.tidx + t * sizeof(int));
    l.region = align256(l.slot + wells * 4);
    l.bytes = align256(l.region + wells * 4);
    l.cleared = l.slot;
    return l;
}

// the molecule region of a call (include/welldup_lanemolecules.h states the arithmetic)
struct LmolLayout {
    size_t mol, molmem, bytes;
};

LmolLayout lmol_layout_of(int max_tiles, int64_t N)
{
    LmolLayout l;
    const size_t wells = (size_t)max_tiles * (size_t)N;
    l.mol = 0;
    l.molmem = align256(l.mol + wells * 4);
    l.bytes = align256(l.molmem + wells * 4);
    return l;
}

// the workgroups of k_lu_group for a lane of `wells` wells: no more than its families of three can be
unsigned lu_group_groups(size_t wells)
{
    const size_t most = (wells / 3 + kLuWaves - 1) / kLuWaves;
    return (unsigned)std::min<size_t>(std::max<size_t>(most, 1), kLuGroups);
}

// d(a, b): XOR, the fold of the 3-bit codes to a bit each (lm_fold), a popcount over both words.  The codes beyond
// the U cycles are zero in every key and never differ.
__device__ inline int lu_dist(uint2 a, uint2 b) { return __popc(lm_fold(a.x, b.x)) + __popc(lm_fold(a.y, b.y)); }

// the key holds an N: a code of 4, the codes' highest bit
__device__ inline bool lu_with_n(uint2 k) { return ((k.x | k.y) & (kLmLow << 2)) != 0; }

// the bin of a count >= 1: 1, 2, 3, 4, 5-8, 9-16, 17-64, 65 or more
__device__ inline uint32_t lu_bin(uint32_t v) { return v <= 4u ? v - 1u : v <= 8u ? 4u : v <= 16u ? 5u : v <= 64u ? 6u : 7u; }

// A tile's three counters in the registers of a wave - the same in every lane -, for the tile the wave met last.
struct LuTile {
    uint32_t tile = kInvalid;
    unsigned long long wells = 0, red = 0, lone = 0;
    __device__ void flush(unsigned long long *cnt_t, int lane)
    {
        if (lane == 0 && tile != kInvalid && wells) {
            unsigned long long *c = spread_row(cnt_t, (size_t)tile, kLuTileCnt);
            atomicAdd(c, wells);
            if (red)
                atomicAdd(c + 1, red);
            if (lone)
                atomicAdd(c + 2, lone);
        }
        wells = red = lone = 0;
    }
    __device__ void add(unsigned long long *cnt_t, int lane, uint32_t t, unsigned long long w, unsigned long long r,
                        unsigned long long l)
    {
        if (t != tile) {                                              // (the same in every lane)
            flush(cnt_t, lane);
            tile = t;
        }
        wells += w;
        red += r;
        lone += l;
    }
};

// ---- the molecules as an array (include/welldup_lanemolecules.h) -----------------------------------
// the one store of a well's entry (the emulator counts them: every word is written once)
__device__ inline void lu_emit(uint32_t *mol, uint32_t *molmem, uint32_t g, uint32_t first, uint32_t more)
{
#ifdef WD_LANE_MOL_EMU_STORE
    WD_LANE_MOL_EMU_STORE(g);
#endif
    mol[g] = first;
    molmem[g] = more;
}

// What the pairs walk writes for a well g of its run that is not the copy of a pair: not PF, Single, or of a Large
// family, which counts as one molecule as the finish left it.  A pair's root is left to its copy's lane, a member of
// a gathered family of three or more to k_lu_group_mol.
__device__ inline void lu_emit_rest(uint32_t *mol, uint32_t *molmem, uint32_t g, uint32_t lab,
                                    const uint32_t *__restrict__ members, int max_family)
{
    if (lab == kInvalid) {
        lu_emit(mol, molmem, g, kInvalid, 0u);
        return;
    }
    const uint32_t mem = members[lab];
    if (mem == 0u || mem + 1u > (uint32_t)max_family)                // (mem == 0: lab == g, a Single)
        lu_emit(mol, molmem, g, lab, lab == g ? mem : 0u);
}

// ---- pairs --------------------------------------------------------------------------------------
// LaneRun's grid and walk.  The copy of a family of two (a PF well that is not its root and whose root has one
// member) loads its own key and key[label] and accounts for both wells of the pair.  The first well of a molecule
// is its smallest global id: of a pair that is one molecule, the larger id is the redundant one.  No atomic per well
// lands on a shared word: everything is a popcount of a ballot, summed in registers - the lane's counters and both
// histograms over the whole walk, the copy's own tile likewise (a run lies on one tile), the root's tile through
// wave_by_key on label / N for the tile the wave met last - and added once per wave, or once per wave and change of
// the root's tile.  The pairs fill two bins of each histogram: one molecule of two wells, or two of one.
template <bool kEmit>
__device__ inline void lu_pairs(const int *__restrict__ tile_idx, int64_t N, const uint32_t *__restrict__ label,
                                const uint32_t *__restrict__ members, const uint2 *__restrict__ key, int max_e,
                                unsigned long long *cnt_t, unsigned long long *cnt_l, int max_family, uint32_t *mol,
                                uint32_t *molmem)
{
    const LaneRun run(tile_idx, N);
    const int lane = threadIdx.x & (kWave - 1);
    unsigned long long n_pair = 0, n_joined = 0, n_equal = 0, n_with_n = 0;      // the same in every lane of a wave
    LuTile own, far;                                                  // the copy's tile (the run's) and the root's
    own.tile = (uint32_t)run.ti;
    run.walk([&](bool has, int64_t, size_t g64) {
        bool pair = false, joined = false, equal = false, wn_a = false, wn_b = false;
        uint32_t lab = kInvalid;
        if (has) {
            lab = label[g64];
            if (lab != kInvalid && lab != (uint32_t)g64 && members[lab] == 1u) {
                const uint2 a = key[g64], b = key[lab];
                const int d = lu_dist(a, b);
                pair = true;
                joined = d <= max_e;
                equal = d == 0;
                wn_a = lu_with_n(a);
                wn_b = lu_with_n(b);
                if constexpr (kEmit) {                                 // both wells of the pair are this lane's
                    const uint32_t lo = min(lab, (uint32_t)g64), hi = max(lab, (uint32_t)g64);
                    lu_emit(mol, molmem, lo, lo, joined ? 1u : 0u);
                    lu_emit(mol, molmem, hi, joined ? lo : hi, 0u);
                }
            } else if constexpr (kEmit)
                lu_emit_rest(mol, molmem, (uint32_t)g64, lab, members, max_family);
        }
        const unsigned long long b_pair = __ballot(pair);
        if (!b_pair)                                                  // (the same for the whole wave)
            return;
        const unsigned long long b_joined = __ballot(joined), b_up = __ballot(pair && (uint32_t)g64 > lab);
        n_pair += (unsigned long long)__popcll(b_pair);
        n_joined += (unsigned long long)__popcll(b_joined);
        n_equal += (unsigned long long)__popcll(__ballot(equal));
        n_with_n += (unsigned long long)(__popcll(__ballot(wn_a)) + __popcll(__ballot(wn_b)));
        own.wells += (unsigned long long)__popcll(b_pair);
        own.red += (unsigned long long)__popcll(b_joined & b_up);
        own.lone += (unsigned long long)__popcll(b_pair & ~b_joined);
        wave_by_key(pair, lab / (uint32_t)N, [&](uint32_t tile, unsigned long long group, bool) {
            far.add(cnt_t, lane, tile, (unsigned long long)__popcll(group), (unsigned long long)__popcll(group & b_joined & ~b_up),
                    (unsigned long long)__popcll(group & ~b_joined));
        });
    });
    own.flush(cnt_t, lane);
    far.flush(cnt_t, lane);
    if (lane == 0 && n_pair) {
        unsigned long long *c = spread_row(cnt_l, 0, kLuLaneCnt);
        const unsigned long long n_split = n_pair - n_joined;
        atomicAdd(c + kLuFamilies, n_pair);
        atomicAdd(c + kLuMolecules, n_pair + n_split);
        atomicAdd(c + kLuDistinct, 2ull * n_pair - n_equal);
        if (n_with_n)
            atomicAdd(c + kLuWithN, n_with_n);
        if (n_joined) {
            atomicAdd(c + kLuPerFamily + 0, n_joined);                // one molecule
            atomicAdd(c + kLuSize + 1, n_joined);                     // of two wells
        }
        if (n_split) {
            atomicAdd(c + kLuSplitFamilies, n_split);
            atomicAdd(c + kLuSplitWells, 2ull * n_split);
            atomicAdd(c + kLuPerFamily + 1, n_split);                 // two molecules
            atomicAdd(c + kLuSize + 0, 2ull * n_split);               // of one well each
        }
    }
}

__global__ void __launch_bounds__(kTdBlock) k_lu_pairs(const int *__restrict__ tile_idx, int64_t N,
                                                        const uint32_t *__restrict__ label,
                                                        const uint32_t *__restrict__ members,
                                                        const uint2 *__restrict__ key, int max_e,
                                                        unsigned long long *cnt_t, unsigned long long *cnt_l)
{
    lu_pairs<false>(tile_idx, N, label, members, key, max_e, cnt_t, cnt_l, 0, nullptr, nullptr);
}

// k_lu_pairs, and every well of the run that is not of a gathered family gets its entry of mol and molmem (the head
// of the file says who writes which word).
__global__ void __launch_bounds__(kTdBlock) k_lu_pairs_mol(const int *__restrict__ tile_idx, int64_t N,
                                                            const uint32_t *__restrict__ label,
                                                            const uint32_t *__restrict__ members,
                                                            const uint2 *__restrict__ key, int max_e, int max_family,
                                                            unsigned long long *cnt_t, unsigned long long *cnt_l,
                                                            uint32_t *mol, uint32_t *molmem)
{
    lu_pairs<true>(tile_idx, N, label, members, key, max_e, cnt_t, cnt_l, max_family, mol, molmem);
}

// ---- grouping -----------------------------------------------------------------------------------
// What a chunk of up to 64 members adds once the molecules stand: `first` = the member is its molecule's first well,
// size = the wells of its molecule.  The tile's counters go through wave_by_key on the member's own tile into the
// registers of the wave (LuTile), MoleculeSize through wave_by_key on the bin of the first wells into LDS.
__device__ inline void lu_tally(bool active, uint32_t id, bool first, uint32_t size, int64_t N, int lane, LuTile &tl,
                                unsigned long long *cnt_t, uint32_t *s_hist)
{
    const unsigned long long b_red = __ballot(active && !first), b_lone = __ballot(active && size == 1u);
    wave_by_key(active, id / (uint32_t)N, [&](uint32_t tile, unsigned long long group, bool) {
        tl.add(cnt_t, lane, tile, (unsigned long long)__popcll(group), (unsigned long long)__popcll(group & b_red),
               (unsigned long long)__popcll(group & b_lone));
    });
    wave_by_key(active && first, lu_bin(size), [&](uint32_t bin, unsigned long long group, bool lowest) {
        if (lowest)
            atomicAdd(&s_hist[kLuBins + bin], (uint32_t)__popcll(group));
    });
}

// grid (groups), groups * kLuWaves waves: wave v takes the families v, v + waves, .. of the table k_lc_reserve left
// (the family count is the cursor's high half; nothing is read back between the launches).  Per family (root, start
// = slot[root], n = members[root] + 1 >= 3):
//   - n <= 64: a member per lane; id and key stay in registers.  n shuffles of the key give the lane its adjacency
//     mask (bit j: d(own, member j) <= E) and, on the way, the smallest global id among its neighbours, itself
//     included - its label.  At E = 0 adjacency is equality, a clique, and that label is the molecule's first well: no
//     round follows.  At E >= 1 the closure: a round gives every lane the smallest label among its neighbours (n
//     shuffles of the label, taken under the mask), until a ballot says that no lane changed; a label moves a hop per
//     round, so at most n - 1 rounds change something.  The molecule's size is the popcount of the lanes with the same
//     label (wave_by_key).
//   - 64 < n <= 1024: the members are taken in chunks of 64 against the chunks at or below their own: lane i of chunk a
//     holds its member's key and meets, by shuffles, the keys of chunk b's members of lower member number.  Each edge
//     d <= E is a tn_unite on the wave's parent array in LDS (near_core.inc's union-find as it stands: hook the larger
//     root under the smaller, by compare-and-swap), on member numbers.  A member that meets an earlier one with the SAME
//     key unites with it and stops.  Nothing is lost: the members are met in ascending member number, so the one it
//     stops at is the first member of its key - its key's representative -, which itself stops nowhere and meets every
//     member below it; for an edge (x, y) the representatives of the two keys are as far apart as x and y, the later
//     of the two unites them, and x and y hang on them.  That keeps a family of equal UMIs at one union per member.
//     Then every member takes its root and gives it its global id (an
//     atomic minimum) and a one (an add): the component's first well and size, read back after the wave has met.
// DistinctUmis: the members with no earlier member (by member number) of the same key.
// Work per family is bounded by max_family^2 / 64 key comparisons per lane (n / 64 chunks, each against at most n
// members; at n <= 64 n comparisons and at most n rounds of n shuffles), so the last wave to finish is at most one
// family of max_family wells behind the others: at 1024 wells 16 384 comparisons per lane.
template <bool kEmit>
__device__ inline void lu_group(int64_t N, const uint32_t *__restrict__ members, const uint2 *__restrict__ key, int max_e,
                                uint32_t W, int groups, const unsigned long long *__restrict__ cursor,
                                const uint32_t *__restrict__ slot, const uint32_t *__restrict__ region,
                                unsigned long long *cnt_t, unsigned long long *cnt_l, uint32_t *mol, uint32_t *molmem)
{
    __shared__ uint32_t s_par[kLuWaves][kLuMaxFamily], s_min[kLuWaves][kLuMaxFamily], s_size[kLuWaves][kLuMaxFamily];
    __shared__ uint32_t s_hist[2 * kLuBins];                          // MolPerFamily, MoleculeSize
    if (threadIdx.x < 2 * kLuBins)
        s_hist[threadIdx.x] = 0;
    __syncthreads();
    const int wv = threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    uint32_t *par = s_par[wv], *mn = s_min[wv], *sz = s_size[wv];
    const uint32_t n_fam = (uint32_t)(*cursor >> 32), n_waves = (uint32_t)groups * kLuWaves;
    unsigned long long families = 0, molecules = 0, distinct = 0, split_f = 0, split_w = 0, with_n = 0;      // the same in every lane
    LuTile tl;
    for (uint32_t f = blockIdx.x * kLuWaves + wv; f < n_fam; f += n_waves) {
        const uint32_t root = region[W - 1u - f];
        const uint32_t start = slot[root], n = members[root] + 1u;
        uint32_t m = 0;                                               // the family's molecules
        if (n <= (uint32_t)kWave) {
            const bool active = (uint32_t)lane < n;
            const uint32_t id = active ? lc_member(region, root, start, (uint32_t)lane) : kInvalid;
            const uint2 k = active ? key[id] : make_uint2(0u, 0u);
            unsigned long long adj = 0;
            uint32_t lab = id;
            bool dup = false;
            for (uint32_t j = 0; j < n; j++) {
                const uint2 kj = make_uint2((uint32_t)__shfl((int)k.x, (int)j), (uint32_t)__shfl((int)k.y, (int)j));
                const uint32_t idj = (uint32_t)__shfl((int)id, (int)j);
                const int d = lu_dist(k, kj);
                if (d <= max_e) {
                    adj |= 1ull << j;
                    lab = min(lab, idj);
                }
                dup = dup || (d == 0 && j < (uint32_t)lane);
            }
            if (max_e > 0)
                for (;;) {
                    uint32_t next = lab;
                    for (uint32_t j = 0; j < n; j++) {
                        const uint32_t lj = (uint32_t)__shfl((int)lab, (int)j);
                        if ((adj >> j) & 1ull)
                            next = min(next, lj);
                    }
                    const unsigned long long changed = __ballot(active && next != lab);
                    lab = next;
                    if (!changed)
                        break;
                }
            uint32_t size = 0;
            wave_by_key(active, lab, [&](uint32_t l0, unsigned long long group, bool) {
                if (lab == l0)
                    size = (uint32_t)__popcll(group);
            });
            const bool first = active && lab == id;
            m = (uint32_t)__popcll(__ballot(first));
            distinct += (unsigned long long)__popcll(__ballot(active && !dup));
            with_n += (unsigned long long)__popcll(__ballot(active && lu_with_n(k)));
            lu_tally(active, id, first, size, N, lane, tl, cnt_t, s_hist);
            if constexpr (kEmit)
                if (active)
                    lu_emit(mol, molmem, id, lab, first ? size - 1u : 0u);
        } else {
            for (uint32_t i = (uint32_t)lane; i < n; i += kWave) {
                par[i] = i;
                mn[i] = kInvalid;
                sz[i] = 0;
            }
            lc_wave_sync();
            for (uint32_t a0 = 0; a0 < n; a0 += kWave) {
                const uint32_t ia = a0 + (uint32_t)lane;
                const bool active = ia < n;
                const uint2 ka = active ? key[lc_member(region, root, start, ia)] : make_uint2(0u, 0u);
                bool dup = false;                                     // an earlier member holds the same key
                for (uint32_t b0 = 0; b0 <= a0; b0 += kWave) {
                    const uint32_t ib = b0 + (uint32_t)lane, cnt = min((uint32_t)kWave, n - b0);
                    const uint2 kb = ib < n ? key[lc_member(region, root, start, ib)] : make_uint2(0u, 0u);
                    for (uint32_t j = 0; j < cnt; j++) {
                        const uint2 kj = make_uint2((uint32_t)__shfl((int)kb.x, (int)j), (uint32_t)__shfl((int)kb.y, (int)j));
                        if (active && !dup && b0 + j < ia) {
                            const int d = lu_dist(ka, kj);
                            if (d <= max_e)
                                tn_unite(par, ia, b0 + j);
                            dup = d == 0;
                        }
                    }
                }
                distinct += (unsigned long long)__popcll(__ballot(active && !dup));
                with_n += (unsigned long long)__popcll(__ballot(active && lu_with_n(ka)));
            }
            lc_wave_sync();                                           // the unions are done
            for (uint32_t ia = (uint32_t)lane; ia < n; ia += kWave) {
                const uint32_t r = tn_find(par, ia);
                atomicMin(&mn[r], lc_member(region, root, start, ia));
                atomicAdd(&sz[r], 1u);
            }
            lc_wave_sync();                                           // every component's first well and size stand
            for (uint32_t a0 = 0; a0 < n; a0 += kWave) {
                const uint32_t ia = a0 + (uint32_t)lane;
                const bool active = ia < n;
                uint32_t id = kInvalid, size = 0;
                bool first = false;
                if (active) {
                    const uint32_t r = tn_find(par, ia);
                    id = lc_member(region, root, start, ia);
                    first = mn[r] == id;
                    size = sz[r];
                    if constexpr (kEmit)
                        lu_emit(mol, molmem, id, mn[r], first ? size - 1u : 0u);
                }
                m += (uint32_t)__popcll(__ballot(first));
                lu_tally(active, id, first, size, N, lane, tl, cnt_t, s_hist);
            }
            lc_wave_sync();                                           // before the next family clears the arrays
        }
        families++;
        molecules += m;
        if (m >= 2u) {
            split_f++;
            split_w += n;
        }
        if (lane == 0)
            atomicAdd(&s_hist[lu_bin(m)], 1u);
    }
    tl.flush(cnt_t, lane);
    if (lane == 0 && families) {
        unsigned long long *c = spread_row(cnt_l, 0, kLuLaneCnt);
        atomicAdd(c + kLuFamilies, families);
        atomicAdd(c + kLuMolecules, molecules);
        atomicAdd(c + kLuDistinct, distinct);
        if (split_f) {
            atomicAdd(c + kLuSplitFamilies, split_f);
            atomicAdd(c + kLuSplitWells, split_w);
        }
        if (with_n)
            atomicAdd(c + kLuWithN, with_n);
    }
    __syncthreads();
    if (threadIdx.x < 2 * kLuBins && s_hist[threadIdx.x])
        atomicAdd(spread_row(cnt_l, 0, kLuLaneCnt) + kLuPerFamily + threadIdx.x, (unsigned long long)s_hist[threadIdx.x]);
}

__global__ void __launch_bounds__(kTdBlock) k_lu_group(int64_t N, const uint32_t *__restrict__ members,
                                                        const uint2 *__restrict__ key, int max_e, uint32_t W, int groups,
                                                        const unsigned long long *__restrict__ cursor,
                                                        const uint32_t *__restrict__ slot, const uint32_t *__restrict__ region,
                                                        unsigned long long *cnt_t, unsigned long long *cnt_l)
{
    lu_group<false>(N, members, key, max_e, W, groups, cursor, slot, region, cnt_t, cnt_l, nullptr, nullptr);
}

// k_lu_group, and every member of a gathered family of three or more wells gets its entry of mol and molmem.
__global__ void __launch_bounds__(kTdBlock) k_lu_group_mol(int64_t N, const uint32_t *__restrict__ members,
                                                            const uint2 *__restrict__ key, int max_e, uint32_t W, int groups,
                                                            const unsigned long long *__restrict__ cursor,
                                                            const uint32_t *__restrict__ slot,
                                                            const uint32_t *__restrict__ region, unsigned long long *cnt_t,
                                                            unsigned long long *cnt_l, uint32_t *mol, uint32_t *molmem)
{
    lu_group<true>(N, members, key, max_e, W, groups, cursor, slot, region, cnt_t, cnt_l, mol, molmem);
}

}  // namespace

#ifndef WD_LANE_UMI_EMU                            // (tools/lane_umi_emu.cpp: the kernels above on the CPU, a fiber per lane)
// the UMI part of an accumulator: lane_index.inc's key part, in the caller's UMI workspace
struct wd_lane_umi_part : LaneKeyPart {};

const LanePartSay kLuSay = {"lane umi", "lane umi: add before wd_lane_umi_begin", "lane umi reads a plane per cycle (well_stride 1)",
                            "null tile index or plane table", "UMI", "workspace smaller than wd_lane_umi_workspace"};

extern "C" {

int wd_lane_umi_workspace(int64_t N, int max_tiles, int U, size_t *bytes)
{
    size_t ws = 0;
    if (!bytes)
        return WD_ERR_ARG;
    if (const int rc = wd_lane_dups_workspace(N, max_tiles, U, &ws))       // (the limits of a lane, with U for L)
        return rc;
    if (U < 1 || U > WD_LANEUMI_MAX_CYCLES)
        return WD_ERR_ARG;
    *bytes = lu_ws_layout_of(N, max_tiles, U).bytes;
    return WD_OK;
}

int wd_lane_umi_begin(wd_lane_dups *ld, int U, void *workspace_dev, size_t workspace_bytes)
try {
    return lane_key_begin(ld, &wd_lane_dups::umi, U, WD_LANEUMI_MAX_CYCLES, lu_ws_layout_of, workspace_dev, workspace_bytes,
                          kLuSay);
} WD_CATCH

int wd_lane_umi_add(wd_lane_dups *ld, int n_tiles, const int *tile_index, const uint8_t *const *umi_planes)
try {
    return lane_key_add(ld, ld ? ld->umi.get() : nullptr, n_tiles, tile_index, umi_planes, kLuSay);
} WD_CATCH

int wd_lane_umi_scratch(int max_tiles, int64_t wells_per_tile, size_t *bytes)
{
    if (max_tiles < 0 || wells_per_tile < 0 || !bytes)
        return WD_ERR_ARG;
    if (max_tiles > 65535 || (max_tiles > 0 && (uint64_t)wells_per_tile >= (uint64_t)0xFFFFFFFFu / (uint64_t)max_tiles))
        return WD_ERR_UNSUPPORTED;
    *bytes = lu_layout_of(max_tiles, wells_per_tile).bytes;
    return WD_OK;
}

int wd_lane_molecules_bytes(int max_tiles, int64_t wells_per_tile, size_t *bytes)
{
    size_t scratch = 0;
    if (!bytes)
        return WD_ERR_ARG;
    if (const int rc = wd_lane_umi_scratch(max_tiles, wells_per_tile, &scratch))
        return rc;
    *bytes = lmol_layout_of(max_tiles, wells_per_tile).bytes;
    return WD_OK;
}

}  // extern "C"

namespace {

// wd_lane_umi and wd_lane_umi_molecules: one body.  Without `emit` the counting kernels run and mol_dev is not looked at.
int lu_run(wd_lane_dups *ld, int max_e, int max_family, void *scratch_dev, size_t scratch_bytes, int64_t *lane_row,
           int64_t *tile_rows, bool emit, void *mol_dev, size_t mol_bytes)
{
    wd_ctx *ctx = ld->ctx;
    const int64_t N = ld->N;
    const int T = ld->max_tiles;
    wd_lane_umi_part *lu = ld->umi.get();
    LanePass p(ld);
    if (!lu)
        return fail(ctx, WD_ERR_ARG, "lane umi: the pass needs wd_lane_umi_begin");
    if (const int rc = p.finished("lane umi comes after a successful finish of the lane"))
        return rc;
    if (const int rc = lane_part_tiles(ld, lu->added, "lane umi", "UMI planes"))
        return rc;
    if (max_e < 0 || max_e > kLuMaxE)
        return fail(ctx, WD_ERR_ARG, "lane umi: max_e is 0.." + std::to_string(kLuMaxE) + ", not " + std::to_string(max_e));
    if (max_family < 2 || max_family > kLuMaxFamily)
        return fail(ctx, WD_ERR_ARG, "lane umi: max_family is 2.." + std::to_string(kLuMaxFamily) + ", not " +
                                         std::to_string(max_family));
    const LuLayout lay = lu_layout_of(T, N);
    if (const int rc = p.scratch(scratch_dev, scratch_bytes, lay.bytes, "scratch smaller than wd_lane_umi_scratch",
                                 "lane umi: the scratch must be in device memory"))
        return rc;
    const LmolLayout ml = lmol_layout_of(T, N);
    if (emit) {
        if (!mol_dev || mol_bytes < ml.bytes)
            return fail(ctx, WD_ERR_ARG, "lane umi: the molecule region is smaller than wd_lane_molecules_bytes");
        if (!on_device(mol_dev))
            return fail(ctx, WD_ERR_ARG, "lane umi: the molecule region must be in device memory");
        const uintptr_t m0 = (uintptr_t)mol_dev, s0 = (uintptr_t)scratch_dev;
        if (m0 < s0 + scratch_bytes && s0 < m0 + mol_bytes)
            return fail(ctx, WD_ERR_ARG, "lane umi: the molecule region overlaps the scratch");
    }
    uint32_t *mol = emit ? (uint32_t *)((uint8_t *)mol_dev + ml.mol) : nullptr;
    uint32_t *molmem = emit ? (uint32_t *)((uint8_t *)mol_dev + ml.molmem) : nullptr;
    memset(lane_row, 0, WD_LANEUMI_LANE_COLS * sizeof(int64_t));
    memset(tile_rows, 0, (size_t)T * kLuTileCnt * sizeof(int64_t));
    if (!p.start()) {
        if (p.rc != WD_OK || !emit || N == 0 || T == 0)
            return p.rc;
        if (bind_device(ctx))                                          // wells but no tile: no well is PF
            return WD_ERR_HIP;
        WD_HIP(ctx, hipMemsetAsync(mol, 0xFF, 4 * (size_t)T * (size_t)N, ctx->stream));
        WD_HIP(ctx, hipMemsetAsync(molmem, 0, 4 * (size_t)T * (size_t)N, ctx->stream));
        WD_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return WD_OK;
    }
    uint8_t *sc = (uint8_t *)scratch_dev;
    unsigned long long *cnt_t = (unsigned long long *)(sc + lay.cnt_t);
    unsigned long long *cnt_l = (unsigned long long *)(sc + lay.cnt_l);
    unsigned long long *cnt_r = (unsigned long long *)(sc + lay.cnt_r);
    unsigned long long *cursor = (unsigned long long *)(sc + lay.cursor);
    int *d_tidx = (int *)(sc + lay.tidx);
    uint32_t *slot = (uint32_t *)(sc + lay.slot), *region = (uint32_t *)(sc + lay.region);
    const uint32_t *label = (const uint32_t *)(ld->ws + ld->lay.label), *members = (const uint32_t *)(ld->ws + ld->lay.members);
    const uint2 *key = (const uint2 *)(lu->ws + lu->at.key);
    const size_t wells = (size_t)T * (size_t)N;
    const uint32_t W = (uint32_t)wells;
    const unsigned groups = lu_group_groups(wells);
    WD_HIP(ctx, hipMemsetAsync(sc, 0, lay.cleared, ctx->stream));
    if (const int rc = p.upload(d_tidx))
        return rc;
    if (emit) {
        for (int t = 0; t < T; t++)                                    // a tile never added: no well of it is PF
            if (!ld->added[t]) {
                WD_HIP(ctx, hipMemsetAsync(mol + (size_t)t * (size_t)N, 0xFF, 4 * (size_t)N, ctx->stream));
                WD_HIP(ctx, hipMemsetAsync(molmem + (size_t)t * (size_t)N, 0, 4 * (size_t)N, ctx->stream));
            }
        hipLaunchKernelGGL(k_lu_pairs_mol, p.grid, dim3(kTdBlock), 0, ctx->stream, d_tidx, N, label, members, key, max_e,
                           max_family, cnt_t, cnt_l, mol, molmem);
    } else
        hipLaunchKernelGGL(k_lu_pairs, p.grid, dim3(kTdBlock), 0, ctx->stream, d_tidx, N, label, members, key, max_e, cnt_t,
                           cnt_l);
    WD_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lc_reserve, p.grid, dim3(kTdBlock), 0, ctx->stream, d_tidx, N, label, members, max_family, W, cursor,
                       slot, region, cnt_r);
    WD_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lc_scatter, p.grid, dim3(kTdBlock), 0, ctx->stream, d_tidx, N, label, members, max_family, slot, region);
    WD_HIP(ctx, hipGetLastError());
    if (emit)
        hipLaunchKernelGGL(k_lu_group_mol, dim3(groups), dim3(kTdBlock), 0, ctx->stream, N, members, key, max_e, W, (int)groups,
                           cursor, slot, region, cnt_t, cnt_l, mol, molmem);
    else
        hipLaunchKernelGGL(k_lu_group, dim3(groups), dim3(kTdBlock), 0, ctx->stream, N, members, key, max_e, W, (int)groups,
                           cursor, slot, region, cnt_t, cnt_l);
    WD_HIP(ctx, hipGetLastError());
    SpreadFetch f_t(cnt_t, (size_t)T, kLuTileCnt), f_l(cnt_l, 1, kLuLaneCnt), f_r(cnt_r, 1, kLcLaneCnt);
    if (const int rc = spread_fetch(ctx, {&f_t, &f_l, &f_r}))
        return rc;
    unsigned long long c[kLuLaneCnt];
    for (int t = 0; t < T; t++) {
        f_t.sum((size_t)t, c);
        for (int f = 0; f < kLuTileCnt; f++) {
            tile_rows[(size_t)t * kLuTileCnt + f] = (int64_t)c[f];
            lane_row[f] += (int64_t)c[f];
        }
    }
    f_l.sum(0, c);
    for (int f = 0; f < 6; f++)
        lane_row[kLuTileCnt + f] = (int64_t)c[kLuFamilies + f];
    for (int b = 0; b < 2 * kLuBins; b++)
        lane_row[kLuTileCnt + 8 + b] = (int64_t)c[kLuPerFamily + b];
    f_r.sum(0, c);
    lane_row[kLuTileCnt + 6] = (int64_t)c[kLcLarge];
    lane_row[kLuTileCnt + 7] = (int64_t)c[kLcLargeWells];
    return WD_OK;
}

}  // namespace

extern "C" {

int wd_lane_umi(wd_lane_dups *ld, int max_e, int max_family, void *scratch_dev, size_t scratch_bytes, int64_t *lane_row,
                int64_t *tile_rows)
try {
    if (!ld || !lane_row || !tile_rows)
        return WD_ERR_ARG;
    return lu_run(ld, max_e, max_family, scratch_dev, scratch_bytes, lane_row, tile_rows, false, nullptr, 0);
} WD_CATCH

int wd_lane_umi_molecules(wd_lane_dups *ld, int max_e, int max_family, void *scratch_dev, size_t scratch_bytes,
                          int64_t *lane_row, int64_t *tile_rows, void *mol_dev, size_t mol_bytes)
try {
    if (ld)
        ld->mol = nullptr;                                             // a call that fails, in whatever way, leaves no molecule part
    if (!ld || !lane_row || !tile_rows)
        return WD_ERR_ARG;
    if (const int rc = lu_run(ld, max_e, max_family, scratch_dev, scratch_bytes, lane_row, tile_rows, true, mol_dev, mol_bytes))
        return rc;
    ld->mol = (uint8_t *)mol_dev;
    ld->mol_e = max_e;
    ld->mol_family = max_family;
    return WD_OK;
} WD_CATCH

int wd_lane_molecules_part(wd_lane_dups *ld, int *max_e, int *max_family)
try {
    if (!ld || !max_e || !max_family)
        return WD_ERR_ARG;
    if (!ld->mol)
        return fail(ld->ctx, WD_ERR_ARG, "lane molecules: the accumulator has no molecule part");
    *max_e = ld->mol_e;
    *max_family = ld->mol_family;
    return WD_OK;
} WD_CATCH

}  // extern "C"
#endif
