// lane_index_emu.cpp - the seven kernels of csrc/lane_index.inc run on the CPU under shuffled schedules: the sources
// are compiled as they stand, the 256 lanes of a workgroup are fibers (tools/wave_emu.h), and every atomic is a point
// at which the schedule may hand over to another lane.  What that reaches here: the two claim_or_join tables with
// closures of their own (k_li_group on the keys of two ids, k_li_sub on (label, glabel[id])), the LDS table of
// k_li_tally - claimed by a plain atomicCAS, left for memory after kLiProbe foreign entries, four 16-bit fields in a
// word -, k_li_emit's places per wave and k_li_rows' chunks.  The launches are those of wd_lane_index_add, li_tally
// and wd_lane_index_finish, in their order and on their grids, in workspaces laid out by ld_layout_of and li_layout_of
// and filled with a pattern; tile index 1 of 3 is never added, the index planes are bytes (N = 0, a base under a
// quality that is not 0), label and members are computed by their definitions.
//   pool       12 libraries (two pairs of keys that differ in the first word alone and in the second alone), 2-5 % of
//              the wells one substitution away, ~10 % non-PF, planted classes of 2 to 40 wells inside one library and
//              across two and three, on one tile and on both; N = 700 and 9000, I = 1, 8, 10, 11, 16, 20
//   one key    every well PF with the same index read, all in one class and all in classes of two, N = kLaneRun and
//              kLaneRun + 1: a workgroup's 16-bit fields reach 8192
//   distinct   every key another, I = 20, N = 9000: the overflow path carries most adds, and the list is longer than
//              a chunk of k_li_rows
//   probe      kLiProbe, kLiProbe + 1 and kLiProbe + 4 groups whose representatives share li_home() - found among the
//              ids of a run with the kernel's own function -, nothing PF below the first of them, every later PF well
//              one of their keys: with kLiProbe groups nothing overflows, with one more one group does, and which
//              one depends on the schedule
//   edges      no PF well; N < 256; N % 4 = 1, 2, 3 with planes 4-byte aligned (VEC4's tail) and at odd addresses
// Every case is finished with min_pf = 0, 1, 2, 3 and more than any group has, and with a cap one below the number listed.
// A case runs under the eleven schedules of emu_reads.h, and after each the keys, glabel, the slots in use of both
// tables, the group rows (as a map by key), Other, the lane index row and n_listed must equal the definitions of
// include/welldup_laneindex.h computed directly, glabel the same under every schedule.  Prints a line per case with
// the scheduling points passed and the compare-and-swaps lost, MISMATCH and exit 1 on a difference.
// tests/test_laneindex_emu.py builds and runs it, and again with -DWAVE_EMU_TORN_CAS (the table's claim torn) and
// -DWAVE_EMU_TORN_CAS=3 (the LDS claim alone), which must end in MISMATCH.  The emulation is sequentially consistent
// and says nothing about time or about caches.
//
//   g++ -O1 -g -std=c++17 -fsanitize=undefined -Iinclude tools/lane_index_emu.cpp -o lane_index_emu
#define WAVE_EMU_UNIT_DEFS
#include "wave_emu.h"
#include "emu_reads.h"
#include <array>
#include <set>
#include "welldup_lanenear.h"
namespace wd {}
constexpr int kMaxLevels = WD_MAX_LEVELS;
#define WD_TILEDUPS_EMU
#include "../well_duplicates_amd/csrc/read_classes.inc"
#include "../well_duplicates_amd/csrc/tile_classes.inc"
#include "../well_duplicates_amd/csrc/near_core.inc"
#include "../well_duplicates_amd/csrc/tile_near.inc"
#include "../well_duplicates_amd/csrc/lane_dups.inc"
#define WD_LANE_PASS_EMU
#include "../well_duplicates_amd/csrc/lane_pass.inc"
#define WD_LANE_INDEX_EMU
#include "../well_duplicates_amd/csrc/lane_index.inc"

constexpr int kTiles = 3;                          // tile indices; index 1 is never added
static const int kAddedAsc[2] = {0, 2};            // ld_tiles_added: ascending
static const int kBatch[2] = {2, 0};               // the one wd_lane_index_add call: its tiles in this order
static int g_case;
static bool fail_(const char *what, long a, long long b, long long c) { printf("MISMATCH case %d: %s %ld: %lld want %lld\n", g_case, what, a, b, c); return false; }

// ---- a lane: by global id over the three tile indices (those of index 1 stay empty)
typedef std::vector<uint8_t> Codes;
typedef std::array<long long, kLiCols> Row;
struct Lane {
    int I = 0; int64_t N = 0;
    std::vector<Codes> code; std::vector<char> pf; std::vector<long> cls;      // cls: wells with the same one hold the same read
    std::vector<uint32_t> label, members;
    std::vector<size_t> ids;                                                   // the wells of the added tiles, ascending
    Lane(int I_, int64_t N_) : I(I_), N(N_), code((size_t)N_ * kTiles), pf((size_t)N_ * kTiles, 0), cls((size_t)N_ * kTiles, -1)
    {
        for (int t : kAddedAsc) for (int64_t w = 0; w < N; w++) { ids.push_back((size_t)t * N + w); cls[ids.back()] = (long)ids.back(); }
    }
};
static unsigned long long key_of(const Codes &c) { unsigned long long k = 0; for (size_t i = 0; i < c.size(); i++) k |= (unsigned long long)c[i] << (32 * (i / 10) + 3 * (i % 10)); return k; }

// label: the smallest global id of the class, kInvalid for a non-PF well; members[label]: the others of the class
static void label_lane(Lane &ln)
{
    const size_t W = ln.code.size();
    ln.label.assign(W, kInvalid); ln.members.assign(W, 0);
    std::map<long, uint32_t> rep;
    for (size_t g : ln.ids) if (ln.pf[g]) {
        if (!rep.count(ln.cls[g])) rep[ln.cls[g]] = (uint32_t)g;
        ln.label[g] = rep[ln.cls[g]];
        if (ln.label[g] != g) ln.members[ln.label[g]]++;
    }
}

// classes of 2 to 40 wells on tile 0, on tile 2 or on both; libs: the members take the keys of one, two or three of them
static void plant_classes(Lane &ln, std::mt19937 &rng, int count, const std::vector<Codes> *libs)
{
    long next = (long)ln.code.size();
    for (int i = 0; i < count; i++) {
        const int size = 2 + (i < 2 ? 38 * i : (int)(rng() % 39)), nk = 1 + i % 3, where = (i / 3) % 3, x = (int)(rng() % 64);
        for (int j = 0; j < size; j++) {
            const int t = where == 2 ? kAddedAsc[rng() % 2] : kAddedAsc[where];
            const size_t g = (size_t)t * ln.N + rng() % ln.N;
            ln.cls[g] = next;
            if (libs) ln.code[g] = (*libs)[(size_t)(x + j % nk) % libs->size()];
        }
        next++;
    }
}

static std::vector<Codes> libraries(std::mt19937 &rng, int I)
{
    std::vector<Codes> lib;
    const size_t n = I == 1 ? 4 : 12;
    std::set<unsigned long long> have;
    while (lib.size() < n) {
        Codes c(I);
        for (int i = 0; i < I; i++) c[i] = I > 1 && rng() % 20 == 0 ? 4 : rng() % 4;
        if (I > 1 && lib.size() == 1) { c = lib[0]; const int at = (int)(rng() % std::min(I, 10)); c[at] = (uint8_t)((c[at] + 1) % 4); }      // the first word alone
        if (I > 10 && lib.size() == 2) { c = lib[0]; const int at = 10 + (int)(rng() % (I - 10)); c[at] = (uint8_t)((c[at] + 1) % 4); }       // the second alone
        if (have.insert(key_of(c)).second) lib.push_back(c);
    }
    return lib;
}

static Lane pool_lane(unsigned seed, int I, int64_t N, bool any_pf = true)
{
    std::mt19937 rng(seed);
    Lane ln(I, N);
    const std::vector<Codes> lib = libraries(rng, I);
    const int err = 20 + (int)(rng() % 31);                            // one well in 20 to 50
    for (size_t g : ln.ids) {
        size_t l = 0;
        while (l + 1 < lib.size() && rng() % 3 == 0) l++;              // skewed shares
        if (rng() % 2) l = rng() % lib.size();
        ln.code[g] = lib[l];
        if (rng() % err == 0) ln.code[g][rng() % I] = (uint8_t)(rng() % 5);
        ln.pf[g] = any_pf && rng() % 10 != 0;
    }
    plant_classes(ln, rng, std::max(6, (int)(N / 35)), &lib);
    label_lane(ln);
    return ln;
}

static Lane one_key_lane(int64_t N, bool pairs)
{
    Lane ln(8, N);
    const Codes c = {2, 0, 3, 1, 4, 2, 2, 0};
    for (size_t i = 0; i < ln.ids.size(); i++) { const size_t g = ln.ids[i]; ln.code[g] = c; ln.pf[g] = 1; ln.cls[g] = pairs ? (long)(i / 2) : 0; }
    label_lane(ln);
    return ln;
}

static Lane distinct_lane(unsigned seed, int64_t N)
{
    std::mt19937 rng(seed);
    Lane ln(20, N);
    for (size_t g : ln.ids) {
        Codes c(20, 0);
        for (int j = 0; j < 10; j++) c[j] = c[10 + j] = (uint8_t)((g >> (2 * j)) & 3);      // the id in base 4, in both words
        c[9] = (uint8_t)(g % 5); c[19] = (uint8_t)(g / 5 % 5);
        ln.code[g] = c; ln.pf[g] = rng() % 10 != 0;
    }
    plant_classes(ln, rng, (int)(N / 35), nullptr);
    label_lane(ln);
    return ln;
}

// n_groups representatives with one home entry in the first run of tile 0; *slot: that entry
static Lane probe_lane(unsigned seed, int I, int64_t N, int n_groups, int *slot)
{
    std::mt19937 rng(seed);
    Lane ln(I, N);
    const int64_t run = std::min<int64_t>(N, kLaneRun);
    std::vector<std::vector<uint32_t>> by_home(kLiSlots);
    for (int64_t w = 0; w < run; w++) by_home[li_home((uint32_t)w)].push_back((uint32_t)w);      // (tile 0: the global id is the well)
    int best = -1;
    for (int h = 0; h < kLiSlots; h++)
        if ((int)by_home[h].size() >= n_groups && (best < 0 || by_home[h][n_groups - 1] < by_home[best][n_groups - 1])) best = h;
    *slot = best;
    if (best < 0) return ln;
    const std::vector<uint32_t> reps(by_home[best].begin(), by_home[best].begin() + n_groups);
    std::vector<Codes> keys; std::set<unsigned long long> have;
    while ((int)keys.size() < n_groups) { Codes c(I); for (int i = 0; i < I; i++) c[i] = rng() % 16 == 0 ? 4 : rng() % 4; if (have.insert(key_of(c)).second) keys.push_back(c); }
    for (size_t g : ln.ids) {
        size_t below = 0;                                              // the representatives below this well: whose keys it may carry
        while (below < reps.size() && reps[below] < g) below++;
        const size_t at = std::find(reps.begin(), reps.end(), (uint32_t)g) - reps.begin();
        ln.pf[g] = at < reps.size() || (below > 0 && rng() % 10 != 0);
        ln.code[g] = keys[at < reps.size() ? at : below ? rng() % below : 0];
    }
    plant_classes(ln, rng, (int)(N / 35), nullptr);
    label_lane(ln);
    return ln;
}

// ---- the definitions, directly
struct Want {
    std::vector<unsigned long long> key;           // by id
    std::vector<uint32_t> glabel;
    std::map<unsigned long long, Row> rows;
    std::map<unsigned long long, uint32_t> first;
    long long pf = 0, groups = 0, spans = 0, mixed_classes = 0, mixed_wells = 0;
};
static Want want_of(const Lane &ln)
{
    Want w;
    const size_t W = ln.code.size();
    w.key.assign(W, 0); w.glabel.assign(W, kInvalid);
    for (size_t g : ln.ids) {
        w.key[g] = key_of(ln.code[g]);
        if (!ln.pf[g]) continue;
        if (!w.first.count(w.key[g])) { w.first[w.key[g]] = (uint32_t)g; w.rows[w.key[g]] = Row{0, 0, 0, 0, 0}; }
        w.rows[w.key[g]][0]++; w.pf++;
    }
    for (size_t g : ln.ids) if (ln.pf[g]) w.glabel[g] = w.first[w.key[g]];
    w.groups = (long long)w.rows.size();
    std::map<uint32_t, std::vector<size_t>> classes;
    for (size_t g : ln.ids) if (ln.pf[g]) classes[ln.label[g]].push_back(g);
    for (const auto &[lab, wells] : classes) {
        if (wells.size() < 2) continue;
        std::map<unsigned long long, long long> sub;                   // the subgroups: group -> wells of the class in it
        for (size_t g : wells) sub[w.key[g]]++;
        w.spans += (long long)sub.size(); w.mixed_classes += sub.size() >= 2;
        for (const auto &[k, n] : sub) {
            Row &r = w.rows[k];
            r[1] += n; r[2] += n >= 2 ? n : 0; r[3] += n - 1; r[4] += sub.size() >= 2 ? n : 0;
        }
    }
    for (const auto &[k, r] : w.rows) w.mixed_wells += r[4];
    return w;
}

// ---- the launches
struct Args { const uint8_t *const *planes; const int *tile_idx; int I; int64_t N; uint2 *key; const uint32_t *label, *members; uint32_t *glabel, *cnt;
              unsigned long long *aux, *table, slot_mask, *cnt_l, min_pf; uint32_t *list; unsigned long long *n_listed, *other;
              const uint32_t *rows_list; unsigned long long rows_n, *stage; };
static Args A;
static void e_pack4() { k_li_pack<true>(A.planes, A.tile_idx, A.I, A.N, A.key); }
static void e_pack1() { k_li_pack<false>(A.planes, A.tile_idx, A.I, A.N, A.key); }
static void e_group() { k_li_group(A.tile_idx, A.N, A.label, A.key, A.aux, A.table, A.slot_mask); }
static void e_glabel() { k_li_glabel(A.tile_idx, A.N, A.aux, A.table, A.glabel, A.cnt); }
static void e_sub() { k_li_sub(A.tile_idx, A.N, A.label, A.members, A.glabel, A.aux, A.table, A.slot_mask); }
static void e_span_count() { k_ld_span_count(A.tile_idx, A.N, A.aux, A.table); }
static void e_tally() { k_li_tally(A.tile_idx, A.N, A.label, A.members, A.glabel, A.aux, A.table, A.cnt, A.cnt_l); }
static void e_emit() { k_li_emit(A.tile_idx, A.N, A.glabel, A.cnt, A.min_pf, A.list, A.n_listed, A.other); }
static void e_rows() { k_li_rows(A.rows_list, A.rows_n, A.cnt, A.key, A.stage); }

struct Finish { long long min_pf, cap; };
struct Ran { std::vector<uint32_t> glabel; long long listed_most = 0, chunk = 0; };

static bool run_lane(const Lane &ln, const Want &want, bool unaligned, const std::vector<Finish> &finishes, bool permute, Ran &ran)
{
    const int I = ln.I;
    const int64_t N = ln.N;
    const size_t W = (size_t)N * kTiles;
    const LdLayout lay = ld_layout_of(N, kTiles, I);
    const LiLayout il = li_layout_of(N, kTiles, I);
    Buf<uint8_t> ws(lay.bytes), iws(il.bytes);                         // the two workspaces, as the host lays them out
    unsigned long long *table = (unsigned long long *)(ws.p + lay.table), *aux = (unsigned long long *)(ws.p + lay.aux);
    uint32_t *label = (uint32_t *)(ws.p + lay.label), *members = (uint32_t *)(ws.p + lay.members);
    int *d_tidx = (int *)(iws.p + il.tidx);
    uint2 *key = (uint2 *)(iws.p + il.key);
    uint32_t *glabel = (uint32_t *)(iws.p + il.glabel), *cnt = (uint32_t *)(iws.p + il.cnt);
    unsigned long long *cnt_l = (unsigned long long *)(iws.p + il.cnt_l), *other = (unsigned long long *)(iws.p + il.other);
    unsigned long long *d_listed = (unsigned long long *)(iws.p + il.listed);
    for (size_t g : ln.ids) { label[g] = ln.label[g]; members[g] = ln.members[g]; }       // what the finish left (tile index 1: the pattern)
    // the planes: bytes, every one 4-byte aligned or every one at an odd address
    const size_t stride = (((size_t)N + 3) & ~(size_t)3) + 4;
    Buf<uint8_t> store(2 * (size_t)I * stride);
    std::mt19937 rng(11);
    std::vector<const uint8_t *> planes(2 * (size_t)I);
    for (int b = 0; b < 2; b++)
        for (int c = 0; c < I; c++) {
            uint8_t *p = store.p + ((size_t)b * I + c) * stride + (unaligned ? 1 : 0);
            for (int64_t w = 0; w < N; w++) p[w] = byte_of(ln.code[(size_t)kBatch[b] * N + w][c], rng);
            planes[(size_t)b * I + c] = p;
        }
    A = Args{(const uint8_t *const *)(iws.p + il.planes), d_tidx, I, N, key, label, members, glabel, cnt, aux, table, lay.slots - 1, cnt_l, 0,
             (uint32_t *)(ws.p + lay.table), d_listed, other, nullptr, 0, nullptr};
    const unsigned wblocks = (unsigned)((N + kTdBlock - 1) / kTdBlock);
    // wd_lane_index_add
    memcpy(iws.p + il.planes, planes.data(), planes.size() * sizeof(void *));
    memcpy(d_tidx, kBatch, sizeof kBatch);
    if (!unaligned) run_grid((unsigned)((N + 4 * kTdBlock - 1) / (4 * kTdBlock)), 2, e_pack4, permute);
    else run_grid(wblocks, 2, e_pack1, permute);
    for (size_t g : ln.ids) {
        const unsigned long long k = (unsigned long long)key[g].y << 32 | key[g].x;
        if (k != want.key[g]) return fail_("key of well", (long)g, (long long)k, (long long)want.key[g]);
    }
    // li_tally
    memcpy(d_tidx, kAddedAsc, sizeof kAddedAsc);
    memset(cnt_l, 0, (size_t)kSpread * kLiLaneCnt * 8);
    memset(table, 0xFF, lay.slots * 8);
    emu_cas_tag = kEmuTable;
    run_grid(wblocks, 2, e_group, permute);
    long long used = 0;
    for (uint64_t s = 0; s < lay.slots; s++) used += table[s] != kEmpty;
    if (used != want.groups) return fail_("slots in use of the groups' table", 0, used, want.groups);
    for (size_t g : ln.ids)
        if (ln.pf[g] ? aux[g] > A.slot_mask : aux[g] != kNoSlot) return fail_("group slot of well", (long)g, (long long)aux[g], ln.pf[g] ? 0 : -1);
    run_grid(wblocks, 2, e_glabel, permute);
    for (size_t g : ln.ids) if (glabel[g] != want.glabel[g]) return fail_("glabel of well", (long)g, glabel[g], want.glabel[g]);
    memset(table, 0xFF, lay.slots * 8);
    run_grid(wblocks, 2, e_sub, permute);
    used = 0;
    for (uint64_t s = 0; s < lay.slots; s++) used += table[s] != kEmpty;
    if (used != want.spans) return fail_("slots in use of the subgroups' table", 0, used, want.spans);
    run_grid(wblocks, 2, e_span_count, permute);
    run_grid((unsigned)((N + kLaneRun - 1) / kLaneRun), 2, e_tally, permute);
    unsigned long long c[kLiLaneCnt];
    sum_spread(cnt_l, 0, kLiLaneCnt, c);
    if ((long long)c[kLiGroups] != want.groups) return fail_("Groups", 0, (long long)c[kLiGroups], want.groups);
    if ((long long)c[kLiSpans] != want.spans) return fail_("GroupSpans", 0, (long long)c[kLiSpans], want.spans);
    if ((long long)c[kLiMixedClasses] != want.mixed_classes) return fail_("MixedClasses", 0, (long long)c[kLiMixedClasses], want.mixed_classes);
    for (const auto &[k, r] : want.rows)
        for (int f = 0; f < kLiCols; f++)
            if (cnt[(size_t)want.first.at(k) * kLiCols + f] != r[f]) return fail_("column of the row at representative", (long)want.first.at(k) * 10 + f, cnt[(size_t)want.first.at(k) * kLiCols + f], r[f]);
    // wd_lane_index_finish, once per (min_pf, cap)
    const size_t stage_at = align256(W * 4);
    unsigned long long *stage = (unsigned long long *)(ws.p + lay.table + stage_at);
    const size_t chunk = (lay.slots * 8 - stage_at) / (kLiStage * 8);
    ran.chunk = (long long)chunk;
    for (const Finish &f : finishes) {
        memset(other, 0, il.planes - il.other);                        // Other and the count
        A.min_pf = (unsigned long long)std::max<long long>(f.min_pf, 0);
        run_grid(wblocks, 2, e_emit, permute);
        const unsigned long long listed = *d_listed;
        unsigned long long h_other[kLiOtherCnt];
        sum_spread(other, 0, kLiOtherCnt, h_other);
        Row want_other{0, 0, 0, 0, 0}; long long want_listed = 0;
        for (const auto &[k, r] : want.rows) {
            if (r[0] >= f.min_pf) { want_listed++; continue; }
            for (int q = 0; q < kLiCols; q++) want_other[q] += r[q];
        }
        if ((long long)listed != want_listed) return fail_("n_listed at min_pf", (long)f.min_pf, (long long)listed, want_listed);
        ran.listed_most = std::max(ran.listed_most, (long long)listed);
        if (listed > (unsigned long long)f.cap) continue;              // (WD_ERR_UNSUPPORTED: the count, nothing else)
        std::vector<unsigned long long> h_stage((size_t)listed * kLiStage);
        for (size_t off = 0; off < listed; off += chunk) {
            const size_t n = std::min<size_t>(chunk, listed - off);
            A.rows_list = A.list + off; A.rows_n = n; A.stage = stage;
            run_grid((unsigned)((n + kTdBlock - 1) / kTdBlock), 1, e_rows, permute);
            memcpy(h_stage.data() + off * kLiStage, stage, n * kLiStage * 8);
        }
        std::map<unsigned long long, Row> got;
        long long mixed_wells = (long long)h_other[4];
        for (size_t i = 0; i < listed; i++) {
            Row r;
            for (int q = 0; q < kLiCols; q++) r[q] = (long long)h_stage[i * kLiStage + q];
            if (!got.insert({h_stage[i * kLiStage + kLiCols], r}).second) return fail_("a key listed twice, place", (long)i, 0, 0);
            mixed_wells += r[4];
        }
        for (const auto &[k, r] : want.rows) {
            if (r[0] < f.min_pf) continue;
            const auto it = got.find(k);
            if (it == got.end()) return fail_("listed group missing, representative", (long)want.first.at(k), 0, 1);
            for (int q = 0; q < kLiCols; q++) if (it->second[q] != r[q]) return fail_("column of the listed row at representative", (long)want.first.at(k) * 10 + q, it->second[q], r[q]);
        }
        for (int q = 0; q < kLiCols; q++) if ((long long)h_other[q] != want_other[q]) return fail_("Other column", q, (long long)h_other[q], want_other[q]);
        if (mixed_wells != want.mixed_wells) return fail_("MixedWells at min_pf", (long)f.min_pf, mixed_wells, want.mixed_wells);
    }
    ran.glabel.assign(glabel, glabel + W);
    for (size_t g = (size_t)N; g < 2 * (size_t)N; g++) ran.glabel[g] = 0;      // (tile index 1: never written)
    return true;
}

int main()
{
    // what li_home gives for a fixed list of ids: tests/test_laneindex_emu.py holds the GPU tests' copy against it
    printf("homes:");
    for (uint32_t id : {0u, 1u, 2u, 255u, 256u, 700u, 8191u, 8192u, 9000u, 17999u, 18000u, 26999u, 123456789u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFEu})
        printf(" %u=%u", id, li_home(id));
    printf("\n");
    struct Case { const char *family; int I; int64_t N; bool unaligned; int k; };
    std::vector<Case> cases;
    int n = 0;
    // (the probe edge first: two groups meet on one free entry there, and a torn LDS claim ends the run at once)
    for (int extra : {0, 1, 4}) cases.push_back({"probe", 8, 9000, false, kLiProbe + extra});
    cases.push_back({"probe", 20, 9000, true, kLiProbe + 1});
    for (int64_t N : {700, 9000}) for (int I : {1, 8, 10, 11, 16, 20}) cases.push_back({"pool", I, N, n++ % 2 == 1, 0});
    for (int64_t N : {kLaneRun, kLaneRun + 1}) for (const char *f : {"one_class", "pairs"}) cases.push_back({f, 8, N, false, 0});
    cases.push_back({"distinct", 20, 9000, false, 0});
    cases.push_back({"no_pf", 8, 300, false, 0});
    cases.push_back({"small", 11, 100, false, 0});
    cases.push_back({"small", 8, 255, true, 0});
    const int tail_I[6] = {11, 20, 8, 20, 11, 1};
    for (int i = 0; i < 6; i++) cases.push_back({"tail", tail_I[i], 301 + i % 3, i >= 3, 0});
    for (g_case = 0; g_case < (int)cases.size(); g_case++) {
        const Case &c = cases[g_case];
        const std::string fam = c.family;
        const unsigned seed = 1000u * g_case + 7;
        int slot = -1;
        const Lane ln = fam == "one_class" ? one_key_lane(c.N, false) : fam == "pairs" ? one_key_lane(c.N, true) : fam == "distinct" ? distinct_lane(seed, c.N)
                      : fam == "probe" ? probe_lane(seed, c.I, c.N, c.k, &slot) : pool_lane(seed, c.I, c.N, fam != "no_pf");
        if (fam == "probe" && slot < 0) { printf("MISMATCH case %d: no %d ids of a run share a home entry\n", g_case, c.k); return 1; }
        const Want want = want_of(ln);
        const long long W = (long long)c.N * kTiles;
        std::vector<Finish> finishes = {{0, W}, {1, W}, {3, W}, {1ll << 40, 0}};
        if (want.groups > 0) finishes.push_back({1, want.groups - 1});         // a cap below the number listed
        finishes.push_back({2, W});
        long long points = 0, never_lost = 0, lost_table = 0, lost_lds = 0, listed_most = 0, chunk = 0;
        std::vector<uint32_t> first;
        for (int s = 0; s < kSchedules; s++) {
            const bool permute = set_schedule(s, seed);
            Ran ran;
            if (!run_lane(ln, want, c.unaligned, finishes, permute, ran)) { printf("  (schedule %d %s, seed %u)\n", s, schedule_name(s), seed); return 1; }
            if (s == 0) { first = ran.glabel; never_lost = emu_counts.lost[kEmuTable] + emu_counts.lost[kEmuUnion] + emu_counts.lost[kEmuLds]; }
            else if (ran.glabel != first) { printf("MISMATCH case %d: schedule %d gives another glabel than schedule 0\n", g_case, s); return 1; }
            if (s >= 3) { lost_table += emu_counts.lost[kEmuTable]; lost_lds += emu_counts.lost[kEmuLds]; }
            points += emu_counts.points; listed_most = ran.listed_most; chunk = ran.chunk;
        }
        long long most = 0;                                            // the largest field a workgroup of k_li_tally adds up
        for (const auto &[k, r] : want.rows) most = std::max(most, std::min<long long>(*std::max_element(r.begin(), r.end()), std::min<long long>(c.N, kLaneRun)));
        printf("case %d ok: family %s I %d N %ld unaligned %d k %d slot %d schedules %d pf %lld groups %lld spans %lld mixed_classes %lld mixed_wells %lld "
               "field %lld listed %lld chunk %lld points %lld never_lost %lld lost_table %lld lost_lds %lld\n",
               g_case, c.family, c.I, (long)c.N, (int)c.unaligned, c.k, slot, kSchedules, want.pf, want.groups, want.spans, want.mixed_classes,
               want.mixed_wells, most, listed_most, chunk, points, never_lost, lost_table, lost_lds);
        fflush(stdout);
    }
    return 0;
}
