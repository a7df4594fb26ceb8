// read_classes_emu.cpp - the lock-free class table (claim_or_join, csrc/read_classes.inc) under the kernels that use
// it, run on the CPU under shuffled schedules: the sources are compiled as they stand, the 256 lanes of a workgroup are
// fibers (tools/wave_emu.h), and every atomic is a point at which the schedule may hand over to another lane - so a
// slot is claimed between a lane's load and its compare-and-swap, representatives go down while others compare with
// them, and the minimum races, which the order of a GPU leaves to chance.
//   tile path   k_td_fingerprint -> k_td_insert -> k_td_resolve (csrc/tile_classes.inc) on planes of 1, 10, 11,
//               16, 17 and 151 cycles: the ends of the 30-bit words and of the 16-cycle blocks of compare_wells
//   lane path   k_ld_insert -> k_ld_resolve -> k_ld_classes -> k_ld_span_count (csrc/lane_dups.inc) on packed rows of 1, 2, 3 and 16
//               words, the two tiles added in two calls in both orders, one tile index never added
// with fingerprints masked to 2 bits (four tags: the reads decide everything) and whole, and tables of the size the
// host gives them, so that probe paths wrap.  A case runs under eleven schedules, and each must give the definitions
// computed directly: the label of a PF well the smallest id with the same read, no slot and no label for a non-PF well,
// members at the representatives, as many slots in use as there are classes - and in the lane's second table one slot
// per (class, tile) group, holding the group's smallest member and, on top of the label, its size less one.  Prints a line per case with the scheduling points
// passed and the compare-and-swaps lost, MISMATCH and exit 1 on a difference.  tests/test_readclasses_emu.py builds and
// runs it, a second time with -DWAVE_EMU_TORN_CAS (a compare-and-swap broken on purpose), which must end in MISMATCH.
// The emulation is sequentially consistent and says nothing about time or about caches.
//
//   g++ -O1 -g -std=c++17 -fsanitize=undefined -Iinclude tools/read_classes_emu.cpp -o read_classes_emu
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

struct Result { std::vector<uint32_t> label; long wrapped = 0; };
static int g_case;
static bool fail_(const char *what, long a, long b, long c) { printf("MISMATCH case %d: %s %ld: %ld want %ld\n", g_case, what, a, b, c); return false; }

// ---- the tile path ----------------------------------------------------------------------------------------------
struct TileArgs { const uint8_t *const *planes, *const *filt; int L; int64_t N; unsigned long long *fp, fp_mask, *table, *cnt; uint32_t slot_mask, *label, *members, *first; };
static TileArgs TA;
static bool t_vec4;
static void t_fingerprint() { if (t_vec4) k_td_fingerprint<true>(TA.planes, TA.L, TA.N, TA.fp, TA.members); else k_td_fingerprint<false>(TA.planes, TA.L, TA.N, TA.fp, TA.members); }
static void t_insert() { k_td_insert(TA.planes, TA.filt, TA.L, TA.N, TA.fp, TA.fp_mask, TA.table, TA.slot_mask, TA.label); }
static void t_resolve() { k_td_resolve(TA.table, TA.slot_mask, TA.N, TA.label, TA.members, TA.first, (uint32_t *const *)nullptr, TA.cnt); }

static bool run_tile_path(const Reads (&reads)[2], const Truth (&truth)[2], int hash_bits, bool unaligned, bool permute, Result &res)
{
    const int n_tiles = 2, L = reads[0].L;
    const int64_t N = kN;
    const Layout lay = layout_of(N, n_tiles);
    Buf<uint8_t> ws(lay.bytes);                                        // the workspace, laid out as the host lays it out
    const View v(lay, ws.p);
    const size_t stride = ((size_t)N + 3) & ~(size_t)3;
    Buf<uint8_t> store((size_t)n_tiles * (L + 1) * stride + 4);
    std::mt19937 rng(7);
    std::vector<const uint8_t *> planes((size_t)n_tiles * L), filt(n_tiles);
    for (int t = 0; t < n_tiles; t++)
        for (int c = 0; c <= L; c++) {
            uint8_t *p = store.p + ((size_t)t * (L + 1) + c) * stride + (unaligned ? 1 : 0);
            for (int64_t w = 0; w < N; w++) p[w] = c < L ? byte_of(reads[t].code.at(w)[c], rng) : (uint8_t)((rng() & 0xFE) | reads[t].pf.at(w));
            (c < L ? planes[(size_t)t * L + c] : filt[t]) = p;
        }
    memset(v.cnt, 0, lay.planes - lay.cnt);                            // clear_workspace
    memset(v.table, 0xFF, (size_t)n_tiles * lay.slots * 8);
    TA = TileArgs{planes.data(), filt.data(), L, N, v.fp, hash_bits == 0 ? ~0ull : (1ull << hash_bits) - 1, v.table, v.cnt, v.slot_mask, v.label, v.members, v.first};
    t_vec4 = !unaligned;
    const unsigned wblocks = (unsigned)((N + kTdBlock - 1) / kTdBlock);
    run_grid(t_vec4 ? (unsigned)((N + 4 * kTdBlock - 1) / (4 * kTdBlock)) : wblocks, n_tiles, t_fingerprint, permute);
    std::vector<unsigned long long> fp(v.fp, v.fp + (size_t)n_tiles * N);
    emu_cas_tag = kEmuTable;
    run_grid(wblocks, n_tiles, t_insert, permute);
    for (int t = 0; t < n_tiles; t++) {
        long used = 0;
        for (uint64_t s = 0; s < lay.slots; s++) used += v.table[(size_t)t * lay.slots + s] != kEmpty;
        if (used != truth[t].classes) return fail_("slots in use of tile", t, used, truth[t].classes);
        for (int64_t w = 0; w < N; w++) {
            const uint32_t s = v.label[(size_t)t * N + w];             // (the slot, until k_td_resolve)
            const bool pf = reads[t].pf.at(w);
            if (pf ? s > v.slot_mask : s != kInvalid) return fail_("slot of well", (long)w, s, pf ? 0 : (long)kInvalid);
            if (pf) res.wrapped += s < ((uint32_t)mix64(fp[(size_t)t * N + w] & TA.fp_mask) & v.slot_mask);
        }
    }
    run_grid(wblocks, n_tiles, t_resolve, permute);
    for (int t = 0; t < n_tiles; t++) {
        long pf = 0;
        for (int64_t w = 0; w < N; w++) {
            const size_t i = (size_t)t * N + w;
            pf += reads[t].pf.at(w);
            if (v.label[i] != truth[t].class_label.at(w)) return fail_("label of well", (long)w, v.label[i], truth[t].class_label.at(w));
            if (v.members[i] != truth[t].class_members.at(w)) return fail_("members at well", (long)w, v.members[i], truth[t].class_members.at(w));
        }
        unsigned long long c[kCnt];
        sum_spread(v.cnt, (size_t)t, kCnt, c);
        if ((long)c[kCntPf] != pf) return fail_("PF of tile", t, (long)c[kCntPf], pf);
    }
    res.label.assign(v.label, v.label + (size_t)n_tiles * N);
    return true;
}

// ---- the lane path ----------------------------------------------------------------------------------------------
struct LaneArgs { const uint8_t *const *filt; const int *tile_idx; int words; int64_t N; const uint32_t *rows; unsigned long long *aux, fp_mask, *table, slot_mask, *cnt_t, *cnt_l; uint32_t *label, *members; };
static LaneArgs A;
static void l_insert() { k_ld_insert(A.filt, A.tile_idx, A.words, A.N, A.rows, A.aux, A.fp_mask, A.table, A.slot_mask); }
static void l_resolve() { k_ld_resolve(A.table, A.tile_idx, A.N, A.aux, A.label, A.members, (uint32_t *const *)nullptr, A.cnt_t); }
static void l_classes() { k_ld_classes(A.tile_idx, A.N, A.label, A.members, A.aux, A.table, A.slot_mask, A.cnt_t, A.cnt_l); }
static void l_span_count() { k_ld_span_count(A.tile_idx, A.N, A.aux, A.table); }

// `reads` by global id over tile indices 0 and 2, added in the order `added`
static bool run_lane_path(const Reads &reads, const Truth &truth, const int (&added)[2], int hash_bits, bool permute, Result &res)
{
    const int L = reads.L;
    const int64_t N = kN;
    const LdLayout lay = ld_layout_of(N, kTiles, L);
    Buf<uint8_t> ws(lay.bytes), filt_store((size_t)kTiles * N);
    const size_t W = (size_t)N * kTiles;
    const int words = lay.words;
    uint32_t *rows = (uint32_t *)(ws.p + lay.rows), *label = (uint32_t *)(ws.p + lay.label), *members = (uint32_t *)(ws.p + lay.members);
    unsigned long long *aux = (unsigned long long *)(ws.p + lay.aux), *table = (unsigned long long *)(ws.p + lay.table);
    memset(ws.p + lay.cnt_t, 0, lay.planes - lay.cnt_t);               // wd_lane_dups_begin
    memset(table, 0xFF, lay.slots * 8);
    std::mt19937 rng(9);
    std::map<size_t, unsigned long long> fp;
    for (const auto &[g, r] : reads.code) {                            // what k_ld_pack leaves: the packed row, the fingerprint, members 0
        Fp h;
        for (int w = 0; w < words; w++) {
            uint32_t word = 0;
            for (int c = w * kFpCycles; c < L && c < (w + 1) * kFpCycles; c++) word |= (uint32_t)r[c] << (3 * (c % kFpCycles));
            rows[g * words + w] = word; h.fold(word);
        }
        aux[g] = fp[g] = h.value(); members[g] = 0;
        filt_store[g] = (uint8_t)((rng() & 0xFE) | reads.pf.at(g));
    }
    A = LaneArgs{nullptr, nullptr, words, N, rows, aux, hash_bits == 0 ? ~0ull : (1ull << hash_bits) - 1, table, lay.slots - 1,
                 (unsigned long long *)(ws.p + lay.cnt_t), (unsigned long long *)(ws.p + lay.cnt_l), label, members};
    const unsigned wblocks = (unsigned)((N + kTdBlock - 1) / kTdBlock);
    emu_cas_tag = kEmuTable;
    for (int call = 0; call < 2; call++) {                             // two add calls of one tile each
        const uint8_t *f = filt_store.p + (size_t)added[call] * N;
        A.filt = &f; A.tile_idx = &added[call];
        run_grid(wblocks, 1, l_insert, permute);
    }
    long used = 0;
    for (uint64_t s = 0; s < lay.slots; s++) used += table[s] != kEmpty;
    if (used != truth.classes) return fail_("slots in use of the lane", 0, used, truth.classes);
    for (const auto &[g, pf] : reads.pf) {
        if (pf ? aux[g] > A.slot_mask : aux[g] != kNoSlot) return fail_("slot of well", (long)g, (long)aux[g], pf ? 0 : -1);
        if (pf) res.wrapped += aux[g] < (mix64(fp[g] & A.fp_mask) & A.slot_mask);
    }
    const int tiles[2] = {0, 2};                                       // ld_tiles_added: ascending
    A.filt = nullptr; A.tile_idx = tiles;
    for (size_t g = 0; g < W; g++) label[g] = kInvalid;                // (a tile index never added: what ld_copy_labels gives out)
    run_grid(wblocks, 2, l_resolve, permute);
    for (size_t g = 0; g < W; g++) {
        const bool in = truth.class_label.count(g) != 0;
        const uint32_t want = in ? truth.class_label.at(g) : kNoLabel;
        if (label[g] != want) return fail_("label of well", (long)g, label[g], want);
        if (in && members[g] != truth.class_members.at(g)) return fail_("members at well", (long)g, members[g], truth.class_members.at(g));
    }
    // the second table: a slot per (class of two or more, tile) group, holding the group's smallest member
    memset(table, 0xFF, lay.slots * 8);
    run_grid(wblocks, 2, l_classes, permute);
    std::map<std::pair<uint32_t, int>, uint32_t> smallest;
    for (const auto &[g, lab] : truth.class_label)
        if (lab != kNoLabel && truth.class_members.at(lab) > 0 && !smallest.count({lab, (int)(g / N)})) smallest[{lab, (int)(g / N)}] = (uint32_t)g;
    used = 0;
    for (uint64_t s = 0; s < lay.slots; s++) used += table[s] != kEmpty;
    if (used != (long)smallest.size()) return fail_("slots in use of the second table", 0, used, (long)smallest.size());
    for (const auto &[g, lab] : truth.class_label) {
        const bool in = lab != kNoLabel && truth.class_members.at(lab) > 0;
        if (in ? aux[g] > A.slot_mask : aux[g] != kNoSlot) return fail_("group slot of well", (long)g, (long)aux[g], in ? 0 : -1);
        if (in && table[aux[g]] != ((unsigned long long)lab << 32 | smallest[{lab, (int)(g / N)}]))
            return fail_("smallest member of the group of well", (long)g, (long)(uint32_t)table[aux[g]], smallest[{lab, (int)(g / N)}]);
    }
    // ... and, once k_ld_span_count has run, the group's size less one on top of the label in the slot's upper half
    run_grid(wblocks, 2, l_span_count, permute);
    std::map<std::pair<uint32_t, int>, uint32_t> size;
    for (const auto &[g, lab] : truth.class_label) if (lab != kNoLabel && truth.class_members.at(lab) > 0) size[{lab, (int)(g / N)}]++;
    for (const auto &[key, first] : smallest) {
        const unsigned long long want = (unsigned long long)(uint32_t)(key.first + size[key] - 1) << 32 | first;
        if (table[aux[first]] != want) return fail_("members counted in the group of well", (long)first, (long)(table[aux[first]] >> 32), (long)(want >> 32));
    }
    res.label.assign(label, label + W);
    return true;
}

int main()
{
    struct Case { int lane; ReadKind kind; int L, bits, order; };
    const ReadKind others[5] = {kChainPermuted, kEqual, kChainDescending, kNoPf, kEqual};
    const int tile_L[6] = {1, 10, 11, 16, 17, 151}, lane_L[4] = {7, 20, 25, 151};       // rows of 1, 2, 3 and 16 words
    std::vector<Case> cases;
    int i = 0;
    for (int L : tile_L) for (int bits : {2, 0}) { cases.push_back({0, kFamilies, L, bits, 0}); cases.push_back({0, others[i++ % 5], L, bits, 0}); }
    for (int L : lane_L) for (int bits : {2, 0}) for (int order : {0, 1}) { cases.push_back({1, kFamilies, L, bits, order}); cases.push_back({1, others[i++ % 5], L, bits, order}); }
    std::vector<size_t> tile_ids, lane_ids;
    for (int64_t w = 0; w < kN; w++) tile_ids.push_back((size_t)w);
    for (int t : {0, 2}) for (int64_t w = 0; w < kN; w++) lane_ids.push_back((size_t)t * kN + w);
    for (g_case = 0; g_case < (int)cases.size(); g_case++) {
        const Case &c = cases[g_case];
        const unsigned seed = 1000u * g_case;
        Reads r[2]; Truth tr[2];
        if (c.lane) { r[0] = make_reads(c.kind, seed, lane_ids, c.L, 0); tr[0] = truth_of(r[0], 0); }
        else for (int t = 0; t < 2; t++) { r[t] = make_reads(c.kind, seed + 500 * t, tile_ids, c.L, 0); tr[t] = truth_of(r[t], 0); }
        const int added[2][2] = {{2, 0}, {0, 2}};
        long points = 0, lost = 0, never_lost = 0, wrapped = 0, pf = 0;
        for (int t = 0; t < 2; t++) for (const auto &[g, p] : r[t].pf) pf += p;
        std::vector<uint32_t> first;
        for (int s = 0; s < kSchedules; s++) {
            const bool permute = set_schedule(s, seed);
            Result res;
            if (c.lane ? !run_lane_path(r[0], tr[0], added[c.order], c.bits, permute, res) : !run_tile_path(r, tr, c.bits, g_case % 4 >= 2, permute, res)) return 1;
            if (s == 0) { first = res.label; never_lost = emu_counts.lost[0] + emu_counts.lost[1]; }
            else if (res.label != first) { printf("MISMATCH case %d: schedule %d gives other labels than schedule 0\n", g_case, s); return 1; }
            if (s >= 3) lost += emu_counts.lost[kEmuTable];
            points += emu_counts.points; wrapped += res.wrapped;
        }
        printf("case %d ok: path %s kind %s L %d words %d bits %d order %d schedules %d pf %ld classes %ld wrapped %ld points %ld never_lost %ld lost_table %ld\n",
               g_case, c.lane ? "lane" : "tile", kReadKindName[c.kind], c.L, (c.L + kFpCycles - 1) / kFpCycles, c.bits, c.order, kSchedules, pf,
               tr[0].classes + tr[1].classes, wrapped, points, never_lost, lost);
        fflush(stdout);
    }
    return 0;
}
