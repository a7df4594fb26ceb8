// near_emu.cpp - the near-duplicate kernels (csrc/near_core.inc under csrc/tile_near.inc and csrc/lane_near.inc, with
// k_td_insert / k_td_resolve of csrc/tile_classes.inc and k_ld_insert / k_ld_resolve of csrc/lane_dups.inc before
// them) run on the CPU under shuffled schedules: the sources are compiled as they stand, the 256 lanes of a workgroup
// are fibers (tools/wave_emu.h), and every atomic is a point at which the schedule may hand over to another lane - so
// the retry loop of tn_unite, the path splitting of tn_find under concurrent hooks and the "claimed meanwhile" branch
// of claim_or_join run, which the order of a GPU leaves to chance.
// The tile chain is launched as wd_tile_near_dups launches it, the lane chain as wd_lane_near_dups_finish does (all
// bounds first, segment K down to 0, by_label as the host sets it; the tiles added in two calls, one tile index never
// added).  A case is a kind of reads (tools/emu_reads.h), K, L and a fingerprint mask; it runs under eleven schedules,
// and each must give the definitions computed directly: the label of a PF well the smallest id of its single-linkage
// cluster, none for a non-PF well, members at the smallest ids, NearPairs the unordered pairs of distinct reads within
// K - and, after every scatter, every vertex of a slot of more than 32 vertices exactly once inside its slot's range.
// Prints a line per case with the scheduling points passed and the compare-and-swaps lost, MISMATCH and exit 1 on a
// difference.  tests/test_near_emu.py builds and runs it, a second time with -DWAVE_EMU_TORN_CAS (a compare-and-swap
// broken on purpose), which must end in MISMATCH.  The emulation is sequentially consistent and says nothing about
// time or about caches.
//
//   g++ -O1 -g -std=c++17 -fsanitize=undefined -Iinclude tools/near_emu.cpp -o near_emu
#define WAVE_EMU_UNIT_DEFS
#include "wave_emu.h"
#include "emu_reads.h"
#include "welldup_lanenear.h"
namespace wd {}
constexpr int kMaxLevels = WD_MAX_LEVELS;
#define WD_TILEDUPS_EMU
#include "../well_duplicates_amd/csrc/read_classes.inc"
#include "../well_duplicates_amd/csrc/tile_classes.inc"
#include "../well_duplicates_amd/csrc/near_core.inc"
#include "../well_duplicates_amd/csrc/tile_near.inc"
#include "../well_duplicates_amd/csrc/lane_dups.inc"
#include "../well_duplicates_amd/csrc/lane_near.inc"

constexpr int kTiles = 3;                          // tile indices; index 1 is never added
constexpr int64_t kN = 300;                        // a full workgroup and a partial one
static const int kAdded[2] = {2, 0};               // in the order of the add calls

struct Result { std::vector<uint32_t> label, members; long near_pairs = 0, long_slots = 0; bool s32 = false, s33 = false; };
static int g_case;
static bool fail_(const char *what, long a, long b, long c) { printf("MISMATCH case %d: %s %ld: %ld want %ld\n", g_case, what, a, b, c); return false; }

// every vertex of a long slot once inside its slot's range: `list` after scatter; slot(v) and head(slot) as the kernels see them
template <class SlotOf>
static bool check_scatter(const std::vector<uint32_t> &vertices, const uint32_t *slots, const uint32_t *list, size_t list_base, SlotOf slot_of, Result &res)
{
    std::map<size_t, std::vector<uint32_t>> by_slot;
    for (uint32_t v : vertices) by_slot[slot_of(v)].push_back(v);
    for (auto &[s, vs] : by_slot) {
        const uint32_t c = ~slots[2 * s + 1];
        if (c != vs.size()) return fail_("slot count", (long)s, c, (long)vs.size());
        res.s32 |= c == 32; res.s33 |= c == 33;
        if (c <= kTnLong) continue;
        res.long_slots++;
        std::vector<uint32_t> in(list + list_base + slots[2 * s], list + list_base + slots[2 * s] + c);
        std::sort(in.begin(), in.end()); std::sort(vs.begin(), vs.end());
        if (in != vs) return fail_("members of long slot", (long)s, (long)in[0], (long)vs[0]);
    }
    return true;
}

// ---- the tile chain -------------------------------------------------------------------------------------------
struct TileArgs {
    const uint8_t *const *planes, *const *filt; int L, nseg, k, seg; int64_t N; size_t wells;
    unsigned long long *fp, fp_mask, *table, *cnt, *aux_s; uint32_t fmask, slot_mask, *slots, *next, *rank, *list, *segfp, *label, *members, *first;
};
static TileArgs TA;
static bool t_vec4;
static void t_fingerprint() { if (t_vec4) k_tn_fingerprint<true>(TA.planes, TA.L, TA.nseg, TA.N, TA.wells, TA.fp, TA.segfp, TA.members); else k_tn_fingerprint<false>(TA.planes, TA.L, TA.nseg, TA.N, TA.wells, TA.fp, TA.segfp, TA.members); }
static void t_insert() { k_td_insert(TA.planes, TA.filt, TA.L, TA.N, TA.fp, TA.fp_mask, TA.table, TA.slot_mask, TA.label); }
static void t_resolve() { k_td_resolve(TA.table, TA.slot_mask, TA.N, TA.label, TA.members, TA.first, (uint32_t *const *)nullptr, TA.cnt); }
static void t_bucket() { k_tn_bucket(TA.label, TA.seg, TA.N, TA.segfp + (size_t)TA.seg * TA.wells, TA.fmask, TA.slot_mask, TA.slots, TA.next, TA.rank); }
static void t_bound() { k_tn_bound(TA.slots, TA.slot_mask, TA.aux_s); }
static void t_scatter() { k_tn_scatter(TA.next, TA.N, TA.segfp + (size_t)TA.seg * TA.wells, TA.fmask, TA.slot_mask, TA.slots, TA.rank, TA.list); }
static void t_pairs() { k_tn_pairs(TA.planes, TA.L, TA.k, TA.seg, TA.N, TA.segfp, TA.wells, TA.fmask, TA.slot_mask, TA.slots, TA.next, TA.label, TA.cnt); }
static void t_pairs_long() { k_tn_pairs_long(TA.planes, TA.L, TA.k, TA.seg, TA.N, TA.segfp, TA.wells, TA.fmask, TA.slot_mask, TA.slots, TA.list, TA.aux_s, TA.label, TA.cnt); }
static void t_compress() { k_tn_compress(TA.label, TA.N, TA.members, TA.first); }
static void t_members() { k_tn_members(TA.label, TA.N, TA.members, (uint32_t *const *)nullptr); }

// two tiles (the batch); reads[i] those of tile i.  Returns per-tile results, false after a MISMATCH.
static bool run_tile_chain(const Reads (&reads)[2], int k, int hash_bits, bool unaligned, bool permute, Result (&res)[2])
{
    const int n_tiles = 2, L = reads[0].L, nseg = k + 1;
    const int64_t N = kN;
    const NearLayout nl = near_layout_of(N, n_tiles, k);
    const Layout &lay = nl.base;
    Buf<uint8_t> ws(nl.bytes);                                         // the workspace, laid out as the host lays it out
    const View v(lay, ws.p);
    const size_t wells = (size_t)n_tiles * N, stride = ((size_t)N + 3) & ~(size_t)3;
    Buf<uint8_t> store((size_t)n_tiles * (L + 1) * stride + 4);
    std::mt19937 rng(7);
    std::vector<const uint8_t *> planes((size_t)n_tiles * L), filt(n_tiles);
    for (int t = 0; t < n_tiles; t++) {
        for (int c = 0; c <= L; c++) {
            uint8_t *p = store.p + ((size_t)t * (L + 1) + c) * stride + (unaligned ? 1 : 0);
            for (int64_t w = 0; w < N; w++) p[w] = c < L ? byte_of(reads[t].code.at(w)[c], rng) : (uint8_t)((rng() & 0xFE) | reads[t].pf.at(w));
            (c < L ? planes[(size_t)t * L + c] : filt[t]) = p;
        }
    }
    memset(v.cnt, 0, lay.planes - lay.cnt);                            // clear_workspace
    memset(v.table, 0xFF, (size_t)n_tiles * lay.slots * 8);
    unsigned long long *aux = (unsigned long long *)(ws.p + nl.aux);
    memset(aux, 0, (size_t)nseg * n_tiles * 2 * 8);
    TA = TileArgs{planes.data(), filt.data(), L, nseg, k, 0, N, wells, v.fp, hash_bits == 0 ? ~0ull : (1ull << hash_bits) - 1, v.table, v.cnt, aux,
                 hash_bits == 0 || hash_bits == 32 ? ~0u : (1u << hash_bits) - 1, v.slot_mask, (uint32_t *)v.table, (uint32_t *)v.fp, (uint32_t *)v.fp + wells,
                 v.first, (uint32_t *)(ws.p + nl.segfp), v.label, v.members, v.first};
    t_vec4 = !unaligned;
    const unsigned wblocks = (unsigned)((N + kTdBlock - 1) / kTdBlock), sblocks = (unsigned)((lay.slots + kTnBoundSlots - 1) / kTnBoundSlots);
    run_grid(t_vec4 ? (unsigned)((N + 4 * kTdBlock - 1) / (4 * kTdBlock)) : wblocks, n_tiles, t_fingerprint, permute);
    emu_cas_tag = kEmuTable;
    run_grid(wblocks, n_tiles, t_insert, permute);
    run_grid(wblocks, n_tiles, t_resolve, permute);
    emu_cas_tag = kEmuUnion;
    std::vector<uint32_t> vertices[2];                                 // the representatives, before any union
    for (int t = 0; t < n_tiles; t++) for (int64_t w = 0; w < N; w++) if (v.label[(size_t)t * N + w] == (uint32_t)w) vertices[t].push_back((uint32_t)w);
    for (int seg = 0; seg < nseg; seg++) {
        TA.seg = seg; TA.aux_s = aux + (size_t)seg * n_tiles * 2;
        memset(TA.slots, 0xFF, (size_t)n_tiles * lay.slots * 8);
        run_grid(wblocks, n_tiles, t_bucket, permute);
        run_grid(sblocks, n_tiles, t_bound, permute);
        unsigned long long longest = 0;
        for (int t = 0; t < n_tiles; t++) longest = std::max(longest, TA.aux_s[2 * t + 1]);
        if (longest > 0) run_grid(wblocks, n_tiles, t_scatter, permute);
        for (int t = 0; t < n_tiles; t++) {
            const size_t base = (size_t)t * (lay.slots), wbase = (size_t)t * N;
            const uint32_t *fps = TA.segfp + (size_t)seg * wells + wbase;
            if (!check_scatter(vertices[t], TA.slots + 2 * base, TA.list, wbase,
                               [&](uint32_t x) { return (size_t)((uint32_t)mix64(fps[x] & TA.fmask) & TA.slot_mask); }, res[t]))
                return false;
        }
        run_grid(wblocks, n_tiles, t_pairs, permute);
        if (longest > 0) run_grid((unsigned)((longest + kTdBlock / kWave - 1) / (kTdBlock / kWave)), n_tiles, t_pairs_long, permute);
    }
    run_grid(wblocks, n_tiles, t_compress, permute);
    run_grid(wblocks, n_tiles, t_members, permute);
    for (int t = 0; t < n_tiles; t++) {
        res[t].label.assign(v.label + (size_t)t * N, v.label + (size_t)(t + 1) * N);
        res[t].members.assign(v.members + (size_t)t * N, v.members + (size_t)(t + 1) * N);
        unsigned long long c[kCnt];
        sum_spread(v.cnt, (size_t)t, kCnt, c);
        res[t].near_pairs = (long)c[kCntNear];
    }
    return true;
}

// ---- the lane chain -------------------------------------------------------------------------------------------
struct LaneArgs {
    const uint8_t *const *filt; const int *tile_idx; int words, L, nseg, k, seg; bool by_label; int64_t N; const uint32_t *rows;
    unsigned long long *aux, fp_mask, *table, slot_mask, *cnt_t, *bound_s, *near; uint32_t fmask, *slots, *link, *list, *label, *members;
};
static LaneArgs A;
static void l_insert() { k_ld_insert(A.filt, A.tile_idx, A.words, A.N, A.rows, A.aux, A.fp_mask, A.table, A.slot_mask); }
static void l_resolve() { k_ld_resolve(A.table, A.tile_idx, A.N, A.aux, A.label, A.members, (uint32_t *const *)nullptr, A.cnt_t); }
static void l_bucket() { k_ln_bucket(A.tile_idx, A.N, A.L, A.nseg, A.seg, A.by_label, A.label, A.rows, A.words, A.fmask, A.slot_mask, A.slots, A.link); }
static void l_bound() { k_ln_bound(A.slots, A.slot_mask, A.bound_s); }
static void l_scatter() { k_ln_scatter(A.tile_idx, A.N, A.L, A.nseg, A.seg, A.rows, A.words, A.fmask, A.slot_mask, A.slots, A.link, A.list); }
static void l_pairs() { k_ln_pairs(A.tile_idx, A.N, A.L, A.k, A.seg, A.rows, A.words, A.fmask, A.slot_mask, A.slots, A.link, A.label, A.near); }
static void l_pairs_long() { k_ln_pairs_long(A.L, A.k, A.seg, A.rows, A.words, A.fmask, A.slot_mask, A.slots, A.list, A.bound_s, A.label, A.near); }
static void l_compress() { k_ln_compress(A.tile_idx, A.N, A.label, A.members); }
static void l_members() { k_ln_members(A.tile_idx, A.N, A.label, A.members, (uint32_t *const *)nullptr); }

// `reads` by global id over the tiles of kAdded.  Labels and members of the whole lane, kInvalid where nothing was added.
static bool run_lane_chain(const Reads &reads, int k, int hash_bits, bool permute, Result &res)
{
    const int L = reads.L, nseg = k + 1;
    const int64_t N = kN;
    const LdLayout lay = ld_layout_of(N, kTiles, L);
    const LnLayout nl = ln_layout_of(N, kTiles);
    Buf<uint8_t> ws(lay.bytes), sc(nl.bytes), filt_store((size_t)kTiles * N);
    const size_t W = (size_t)N * kTiles;
    const int words = lay.words;
    uint32_t *rows = (uint32_t *)(ws.p + lay.rows), *label = (uint32_t *)(ws.p + lay.label), *members = (uint32_t *)(ws.p + lay.members);
    unsigned long long *aux = (unsigned long long *)(ws.p + lay.aux), *table = (unsigned long long *)(ws.p + lay.table);
    memset(ws.p + lay.cnt_t, 0, lay.planes - lay.cnt_t);               // wd_lane_dups_begin
    memset(table, 0xFF, lay.slots * 8);
    std::mt19937 rng(9);
    for (const auto &[g, r] : reads.code) {                            // what k_ld_pack leaves: the packed row, the fingerprint, members 0
        Fp h;
        for (int w = 0; w < words; w++) {
            uint32_t word = 0;
            for (int c = w * kFpCycles; c < L && c < (w + 1) * kFpCycles; c++) word |= (uint32_t)r[c] << (3 * (c % kFpCycles));
            rows[g * words + w] = word; h.fold(word);
        }
        aux[g] = h.value(); members[g] = 0;
        filt_store[g] = (uint8_t)((rng() & 0xFE) | reads.pf.at(g));
    }
    const unsigned long long fp_mask = hash_bits == 0 ? ~0ull : (1ull << hash_bits) - 1;
    A = LaneArgs{nullptr, nullptr, words, L, nseg, k, 0, true, N, rows, aux, fp_mask, table, lay.slots - 1, (unsigned long long *)(ws.p + lay.cnt_t),
                 (unsigned long long *)(sc.p + nl.bound), (unsigned long long *)(sc.p + nl.near), (uint32_t)std::min<unsigned long long>(fp_mask, 0xFFFFFFFFull),
                 (uint32_t *)table, (uint32_t *)aux, (uint32_t *)(sc.p + nl.list), label, members};
    const unsigned wblocks = (unsigned)((N + kTdBlock - 1) / kTdBlock), sblocks = (unsigned)((lay.slots + kTnBoundSlots - 1) / kTnBoundSlots);
    emu_cas_tag = kEmuTable;
    for (int call = 0; call < 2; call++) {                             // two add calls of one tile each
        const uint8_t *f = filt_store.p + (size_t)kAdded[call] * N;
        A.filt = &f; A.tile_idx = &kAdded[call];
        run_grid(wblocks, 1, l_insert, permute);
    }
    const int tiles[2] = {std::min(kAdded[0], kAdded[1]), std::max(kAdded[0], kAdded[1])};      // ld_tiles_added: ascending
    A.filt = nullptr; A.tile_idx = tiles;
    for (size_t g = 0; g < W; g++) label[g] = kInvalid;                // (a tile index never added: what ld_copy_labels gives out)
    run_grid(wblocks, 2, l_resolve, permute);
    std::vector<uint32_t> vertices;
    for (int t : tiles) for (int64_t w = 0; w < N; w++) { const size_t g = (size_t)t * N + w; if (label[g] == (uint32_t)g) vertices.push_back((uint32_t)g); }
    emu_cas_tag = kEmuUnion;
    memset(sc.p, 0, nl.list);
    unsigned long long *bound = A.bound_s;
    for (int seg = nseg - 1; seg >= 0; seg--) {                        // the bounds of all segments, the last one first
        memset(A.slots, 0xFF, lay.slots * 8);
        A.seg = seg; A.by_label = true; A.bound_s = bound + 2 * seg;
        run_grid(wblocks, 2, l_bucket, permute);
        run_grid(sblocks, 1, l_bound, permute);
    }
    unsigned long long h_aux[2 * (kTnMaxK + 1)];
    memcpy(h_aux, bound, sizeof(h_aux));
    for (int seg = 0; seg < nseg; seg++) {
        A.seg = seg; A.by_label = false; A.bound_s = bound + 2 * seg;
        const unsigned long long longest = h_aux[2 * seg + 1];
        if (seg > 0) {
            memset(A.slots, 0xFF, lay.slots * 8);
            run_grid(wblocks, 2, l_bucket, permute);
            if (longest > 0) { memset(A.bound_s, 0, 16); run_grid(sblocks, 1, l_bound, permute); }
        }
        if (longest > 0) run_grid(wblocks, 2, l_scatter, permute);
        if (!check_scatter(vertices, A.slots, A.list, 0,
                           [&](uint32_t x) { return (size_t)(mix64(ln_seg_fp(rows + (size_t)x * words, L, nseg, seg) & A.fmask) & A.slot_mask); }, res))
            return false;
        run_grid(wblocks, 2, l_pairs, permute);
        if (longest > 0) run_grid((unsigned)((longest + kTdBlock / kWave - 1) / (kTdBlock / kWave)), 1, l_pairs_long, permute);
    }
    run_grid(wblocks, 2, l_compress, permute);
    run_grid(wblocks, 2, l_members, permute);
    res.label.assign(label, label + W);
    res.members.assign(members, members + W);
    unsigned long long np = 0;
    sum_spread(A.near, 0, 1, &np);
    res.near_pairs = (long)np;
    return true;
}

// `ids` of the space against the definitions; a well outside `ids` (a tile index never added) has no label
static bool check(const Result &res, const Truth &t, size_t space)
{
    for (size_t g = 0; g < space; g++) {
        const bool in = t.cluster_label.count(g) != 0;
        const uint32_t want = in ? t.cluster_label.at(g) : kNoLabel;
        if (res.label[g] != want) return fail_("label of well", (long)g, res.label[g], want);
        if (in && res.members[g] != t.cluster_members.at(g)) return fail_("members at well", (long)g, res.members[g], t.cluster_members.at(g));
    }
    if (res.near_pairs != t.near_pairs) return fail_("NearPairs", 0, res.near_pairs, t.near_pairs);
    return true;
}

int main()
{
    const int masks[3] = {1, 4, 0};                                    // hash_bits: 1 bit, 4 bits, full
    struct Case { int lane; ReadKind kind; int k, L, bits; };
    std::vector<Case> cases;
    for (int lane = 0; lane < 2; lane++) {
        for (int k = 1; k <= kTnMaxK; k++) {
            const int Ls[5] = {k + 1, 13, 21, 30, 31};
            // the families: every K with every L; the mask of 1 bit - two slots for all vertices, every pair of them a
            // candidate: by far the slowest here - once per K and path, at another L each time; 4 bits and full by turns
            for (int j = 0; j < 5; j++) cases.push_back({lane, kFamilies, k, Ls[j], j == (k - 1 + 2 * lane) % 5 ? 1 : masks[1 + (j + k + lane) % 2]});
            // the chains and the slots need room for their reads: L >= 13
            cases.push_back({lane, kChainPermuted, k, Ls[1 + (k + lane) % 4], masks[1 + (k + lane) % 2]});
            cases.push_back({lane, kChainDescending, k, Ls[1 + (k + lane + 2) % 4], masks[1 + (k + lane + 1) % 2]});
            cases.push_back({lane, kSlots, k, Ls[1 + (k + lane + 1) % 4], 0});      // (slots of exactly 32 and 33: the full mask)
            cases.push_back({lane, kEqual, k, Ls[(k + lane) % 5], masks[k % 3]});
        }
        cases.push_back({lane, kNoPf, 1, 13, 0});
        cases.push_back({lane, kNoPf, 3, 4, 1});
    }
    for (g_case = 0; g_case < (int)cases.size(); g_case++) {
        const Case &c = cases[g_case];
        const int seg0 = seg_begin(c.L, c.k + 1, 1);
        std::vector<size_t> tile_ids, lane_ids;
        for (int64_t w = 0; w < kN; w++) tile_ids.push_back((size_t)w);
        for (int t : {0, 2}) for (int64_t w = 0; w < kN; w++) lane_ids.push_back((size_t)t * kN + w);
        long points = 0, lost_t = 0, lost_u = 0, never_lost = 0, long_slots = 0, unions = 0, near_pairs = 0, classes = 0;
        bool s32 = false, s33 = false;
        std::vector<std::vector<uint32_t>> first;                       // the labels of the first schedule
        for (unsigned draw = 0;; draw++) {                              // (kSlots: until a slot of 32 and one of 33 are there)
            const unsigned seed = 1000u * g_case + draw;
            Reads r[2]; Truth tr[2];
            if (c.lane) { r[0] = make_reads(c.kind, seed, lane_ids, c.L, seg0); tr[0] = truth_of(r[0], c.k); }
            else for (int t = 0; t < 2; t++) { r[t] = make_reads(c.kind, seed + 500 * t, tile_ids, c.L, seg0); tr[t] = truth_of(r[t], c.k); }
            bool redraw = false;
            for (int s = 0; s < kSchedules && !redraw; s++) {
                const bool permute = set_schedule(s, seed);
                Result res[2];
                std::vector<std::vector<uint32_t>> labels;
                if (c.lane) {
                    if (!run_lane_chain(r[0], c.k, c.bits, permute, res[0]) || !check(res[0], tr[0], (size_t)kN * kTiles)) return 1;
                    labels = {res[0].label};
                } else {
                    if (!run_tile_chain(r, c.k, c.bits, g_case % 2 == 1, permute, res)) return 1;
                    for (int t = 0; t < 2; t++) if (!check(res[t], tr[t], (size_t)kN)) return 1;
                    labels = {res[0].label, res[1].label};
                }
                if (s == 0) {
                    s32 = res[0].s32 || res[1].s32; s33 = res[0].s33 || res[1].s33;
                    if (c.kind == kSlots && !(s32 && s33) && draw < 200) { redraw = true; break; }
                    first = labels; never_lost = emu_counts.lost[0] + emu_counts.lost[1];
                    long_slots = res[0].long_slots + res[1].long_slots;
                    unions = tr[0].unions + tr[1].unions; near_pairs = tr[0].near_pairs + tr[1].near_pairs; classes = tr[0].classes + tr[1].classes;
                } else if (labels != first) {
                    printf("MISMATCH case %d: schedule %d gives other labels than schedule 0\n", g_case, s); return 1;
                }
                if (s >= 3) { lost_t += emu_counts.lost[kEmuTable]; lost_u += emu_counts.lost[kEmuUnion]; }
                points += emu_counts.points;
            }
            if (!redraw) break;
        }
        printf("case %d ok: path %s kind %s K %d L %d bits %d schedules %d classes %ld unions %ld near_pairs %ld long_slots %ld s32 %d s33 %d points %ld "
               "never_lost %ld lost_table %ld lost_union %ld\n", g_case, c.lane ? "lane" : "tile", kReadKindName[c.kind], c.k, c.L, c.bits, kSchedules, classes,
               unions, near_pairs, long_slots, (int)s32, (int)s33, points, never_lost, lost_t, lost_u);
        fflush(stdout);
    }
    return 0;
}
