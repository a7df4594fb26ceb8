// dup_sets_emu.cpp - the union-find of the duplicate sets (find_split, find_ro, unite and the seven k_sets_* kernels of
// csrc/dup_sets.inc) run on the CPU under shuffled schedules: the source is compiled as it stands, the 256 lanes of a
// workgroup are fibers (tools/wave_emu.h), and every atomic - the relaxed loads and stores of the parent pointers among
// them - is a point at which the schedule may hand over to another lane.  So path splitting races with hooks and with
// other splitters, unite retries from the value a lost compare-and-swap returns, and the count of successful
// compare-and-swaps per level - the product's Redundant[l] - is taken under orders a GPU leaves to chance.
// It needs no reads.  A case is a graph turned into a target table (centre[t] = t, lvl_off, nbr: a naming (a, b, l) puts
// well b into ring l of well a), a filter per tile and a list of hit records {tile, target, slot, dist}.  The kernels are
// launched as wd_dup_sets launches them - the memset of counters and flags, k_sets_check_centres, k_sets_init,
// k_sets_edges, k_sets_union once per level in increasing order, k_sets_compress, the memset of aux, k_sets_count,
// k_sets_bins with labels, sets_fold_row - in three ways: (a) one pass over the batch, the records sorted by tile; (b)
// the same with the records shuffled, so that workgroups hold several tiles and both paths of the hook counter run; (c)
// tile by tile, records carrying tile 0 and tile0 = i: the host's third path, which no GPU test reaches.  Every way runs
// under the eleven schedules of tools/emu_reads.h, and each run must give the definitions computed directly and
// sequentially (sets_truth_of below), the same labels and rows as every other run of the case, and after every k_sets_union
// launch: parent[x] <= x for every PF well, every walk ends, and the roots are exactly the PF wells less the hooks
// counted so far.  Records the targets cannot place must raise kFlagRecord and change nothing else.
// Prints a line per case and way with the scheduling points passed and the compare-and-swaps lost, MISMATCH and exit 1
// on a difference.  tests/test_dup_sets_emu.py builds and runs it, and again with -DWAVE_EMU_TORN_CAS and
// -DWAVE_EMU_TORN_CAS=2 (a compare-and-swap broken on purpose), which must end in MISMATCH.  The emulation is
// sequentially consistent and says nothing about time or about caches.
//
//   g++ -O1 -g -std=c++17 -fsanitize=undefined -Iinclude tools/dup_sets_emu.cpp -o dup_sets_emu
#define WAVE_EMU_UNIT_DEFS
#include "wave_emu.h"
#include "emu_reads.h"
#include "welldup_sets.h"
constexpr int kMaxLevels = WD_MAX_LEVELS;
#include "../well_duplicates_amd/csrc/dup_sets.inc"
#include <numeric>
static_assert(sizeof(wd_hit) == sizeof(int4), "the hit log is read as int4");

// Three tiles of 700 wells: a launch per level and workgroups of 256 fibers make the run time go with levels x records,
// and at 1 500 wells the run took eight times near_emu's; at 700 every case still fills 6 to 22 workgroups per launch
// (3 to 9 tile by tile), leaves the last one ragged and loses compare-and-swaps where it should.
constexpr int kTiles = 3;
constexpr int kN = 700;                            // 2 workgroups and 188 wells: the last wave of a tile has 60 lanes

struct Naming { int a, b, l; };
struct Rec { int tile, target, slot, scan; };      // scan: the tile whose scan logged it (way c takes them scan by scan)
struct Table { std::vector<int32_t> centre, lvl_off, nbr; std::vector<int> slot_of; };      // slot_of[i]: naming i's slot
struct Case {
    std::string family; int levels = 1; bool bad = false;
    std::vector<Naming> nam; Table tb;
    std::vector<uint8_t> pf[kTiles];
    std::vector<Rec> recs;
};
struct SetsTruth { std::vector<uint32_t> label; std::vector<int64_t> rows; long kept = 0, merges = 0, sets = 0; };
struct Result { std::vector<uint32_t> label; std::vector<int64_t> rows; uint32_t flag_record = 0; long lds_hooks = 0, global_hooks = 0; };

static int g_case;
static char g_way;
static int g_schedule;
static bool fail_(const char *what, long at, long got, long want)
{
    printf("MISMATCH case %d way %c schedule %d: %s %ld: %ld want %ld\n", g_case, g_way, g_schedule, what, at, got, want);
    return false;
}

// ---- the graphs ---------------------------------------------------------------------------------------------------
static Table table_of(const std::vector<Naming> &nam, int levels)
{
    Table tb;
    std::vector<int> order(nam.size());
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int i, int j) { return nam[i].a * levels + nam[i].l < nam[j].a * levels + nam[j].l; });
    tb.centre.resize(kN); tb.lvl_off.assign((size_t)kN * (levels + 1), 0); tb.nbr.resize(nam.size()); tb.slot_of.resize(nam.size());
    std::vector<int> count((size_t)kN * levels, 0);
    for (const Naming &n : nam) count[(size_t)n.a * levels + n.l]++;
    int at = 0;
    for (int t = 0; t < kN; t++) {
        tb.centre[t] = t;
        for (int l = 0; l < levels; l++) { tb.lvl_off[(size_t)t * (levels + 1) + l] = at; at += count[(size_t)t * levels + l]; }
        tb.lvl_off[(size_t)t * (levels + 1) + levels] = at;
    }
    for (size_t s = 0; s < order.size(); s++) { tb.nbr[s] = nam[order[s]].b; tb.slot_of[order[s]] = (int)s; }
    return tb;
}

static void both_ends(std::vector<Naming> &nam) { const size_t n = nam.size(); for (size_t i = 0; i < n; i++) nam.push_back({nam[i].b, nam[i].a, nam[i].l}); }

static void add_gnm(std::vector<Naming> &nam, int lo, int levels, double degree, std::mt19937 &rng)
{
    const int n = kN - lo, m = (int)(degree * n / 2);
    for (int i = 0; i < m; i++) {
        const int u = lo + (int)(rng() % n), v = lo + (int)(rng() % n);
        if (u != v) nam.push_back({std::min(u, v), std::max(u, v), (int)(rng() % levels)});
    }
}

static const char *const kGraphFamilies[] = {"path_asc", "path_desc", "path_perm", "star_first", "star_last", "ladder", "late_merge", "cliques",
                                        "gnm_low", "gnm_high", "corners", "bad_slot", "bad_tile", "bad_target", "bad_nbr"};
// (contended, and asked by the test to lose compare-and-swaps under the schedules at 1/3: star_last, path_desc, gnm_high)

static Case make_case(const std::string &family, int levels, unsigned seed)
{
    Case c; c.family = family; c.levels = levels; c.bad = family.compare(0, 4, "bad_") == 0;
    std::mt19937 rng(seed);
    std::vector<Naming> &nam = c.nam;
    // the filters: tile 0 all wells, tile 1 a quarter knocked out, tile 2 a tenth (and half its records, below)
    for (int t = 0; t < kTiles; t++) { c.pf[t].assign(kN, 1); for (int w = 0; w < kN; w++) if (t && rng() % (t == 1 ? 4 : 10) == 0) c.pf[t][w] = 0; }
    const bool background = family == "corners" || c.bad;      // the corners and the bad records: a few wells beside a G(n, m) of mean degree 1.6
    if (family.compare(0, 5, "path_") == 0) {
        // the wells in a row, the level cycling along it, every edge declared from both ends (its two records race for one
        // root).  Descending: every union hooks a fresh root under the next - the deepest forest there is
        std::vector<int> v(kN);
        std::iota(v.begin(), v.end(), 0);
        if (family == "path_desc") std::reverse(v.begin(), v.end());
        if (family == "path_perm") std::shuffle(v.begin(), v.end(), rng);
        for (int i = 0; i + 1 < kN; i++) nam.push_back({v[i], v[i + 1], i % levels});
        both_ends(nam);
    } else if (family.compare(0, 5, "star_") == 0) {
        // every well names the hub and the hub names it back.  Hub last: every edge tries to hook the same root under
        // another smaller one - the worst case for unite's retry.  Tile 1: the hub fails the filter, no set at all
        const int hub = family == "star_last" ? kN - 1 : 0;
        for (int w = 0, i = 0; w < kN; w++) if (w != hub) nam.push_back({w, hub, i++ % levels});
        both_ends(nam);
        c.pf[0][hub] = c.pf[2][hub] = 1; c.pf[1][hub] = 0;
    } else if (family == "ladder") {
        // level l joins neighbouring blocks of 2^l wells by one edge between a random well of each: Sets[l] halves
        for (int l = 0; l < levels && (1 << l) < kN; l++) {
            const int s = 1 << l;
            for (int left = 0; left + s < kN; left += 2 * s)
                nam.push_back({left + (int)(rng() % s), left + s + (int)(rng() % std::min(s, kN - left - s)), l});
        }
        both_ends(nam);
    } else if (family == "late_merge") {
        // a random recursive tree on the lower half and a path on the upper half at level 0, one edge between them at the
        // outermost level: Sets falls from 2 to 1 there
        const int h = kN / 2;
        for (int kid = 1; kid < h; kid++) nam.push_back({(int)(rng() % kid), kid, 0});
        for (int w = h; w + 1 < kN; w++) nam.push_back({w + 1, w, 0});
        nam.push_back({h / 2, kN - 1, levels - 1});
        both_ends(nam);
        for (int t = 0; t < kTiles; t++) c.pf[t][h / 2] = c.pf[t][kN - 1] = 1;
    } else if (family == "cliques") {
        // runs of 2 .. 12 wells, every pair of a run named, a single well between two runs: the size bins, 9+ among them
        for (int pos = 0, rep = 0; pos + 13 <= kN; rep++)
            for (int s = 2; s <= 12 && pos + s + 1 <= kN; pos += s + 1, s++)
                for (int i = 0; i < s; i++) for (int j = i + 1; j < s; j++) nam.push_back({pos + i, pos + j, (i + j + rep) % levels});
    } else if (family == "gnm_low") add_gnm(nam, 0, levels, 0.8, rng), both_ends(nam);
    else if (family == "gnm_high") add_gnm(nam, 0, levels, 3.0, rng);
    if (background) add_gnm(nam, 100, levels, 1.6, rng), both_ends(nam);
    const size_t plain = nam.size();
    if (family == "corners") {
        const int o = levels - 1;                  // (the outermost ring: 2 at three levels, as in tests/dupsets_graphs.py)
        const Naming corners[] = {{10, 11, 0}, {10, 11, o},                  // the same pair in two rings of one well
                                  {20, 21, o}, {21, 20, 0},                  // the outermost level from one end, level 0 from the other
                                  {30, 30, 1},                               // a == b, and nothing else
                                  {33, 33, 0}, {33, 34, o},                  // a == b in a well that joins a set later
                                  {40, 41, 0}, {41, 42, 0}};                 // 41 fails the filter: 40 - 41 - 42 stay apart
        nam.insert(nam.end(), std::begin(corners), std::end(corners));
        for (int w = 0; w < 100; w++) c.pf[0][w] = c.pf[2][w] = 1;
        c.pf[0][41] = c.pf[2][41] = 0;
        c.pf[1].assign(kN, 0);                     // a tile with no PF well (and every record)
    }
    if (family == "bad_nbr") { nam.push_back({50, -1, 0}); nam.push_back({51, kN, levels - 1}); }      // a slot that names no well
    c.tb = table_of(nam, levels);
    const Table &tb = c.tb;
    for (int t = 0; t < kTiles; t++) {
        if (family == "corners" && t == 2) continue;                        // a tile with no record
        size_t before = c.recs.size();
        for (size_t i = 0; i < nam.size(); i++) if (t != 2 || i >= plain || rng() % 2) c.recs.push_back({t, nam[i].a, tb.slot_of[i], t});
        if (family == "corners") for (int d = 0; d < 50; d++) { const Rec r = c.recs[before + rng() % (c.recs.size() - before)]; c.recs.push_back(r); }      // duplicate records
        while ((c.recs.size() - before) % kSetsBlock == 0) { const Rec r = c.recs[before]; c.recs.push_back(r); }      // the last workgroup of a scan: ragged
    }
    auto row = [&](int t, int l) { return tb.lvl_off[(size_t)t * (levels + 1) + l]; };
    if (family == "bad_slot") {
        // slots outside their target's rings: none, the one before its first, the one after its last (another target's,
        // or past the end of nbr for the last target), far out
        c.recs.push_back({0, 300, -1, 0});
        c.recs.push_back({1, 300, row(300, 0) - 1, 1});
        c.recs.push_back({1, 301, row(301, levels), 1});
        c.recs.push_back({2, kN - 1, row(kN - 1, levels), 2});
        c.recs.push_back({2, 5, 0x7FFFFFFF, 2});
    } else if (family == "bad_tile") {
        c.recs.push_back({-1, 300, row(300, 0), 0});
        c.recs.push_back({kTiles, 301, row(301, 0), 1});
        c.recs.push_back({0x7FFFFFF0, 302, row(302, 0), 2});
    } else if (family == "bad_target") {
        c.recs.push_back({0, -1, 0, 0});
        c.recs.push_back({1, kN, 0, 1});
        c.recs.push_back({2, (int)0x80000000, 3, 2});
    }
    while (c.recs.size() % kSetsBlock == 0) { const Rec r = c.recs[0]; c.recs.push_back(r); }               // and of the batch
    return c;
}

// ---- the definitions, directly and sequentially (include/welldup_sets.h) -------------------------------------------
static SetsTruth sets_truth_of(const Case &c)
{
    const int levels = c.levels;
    const size_t ns = 1 + 3 * (size_t)levels + kBins;
    SetsTruth t;
    t.label.assign((size_t)kTiles * kN, kNoLabel); t.rows.assign(kTiles * ns, 0);
    std::vector<std::vector<std::pair<int, int>>> edges((size_t)kTiles * levels);
    for (const Rec &r : c.recs) {
        // kept: it can be placed - tile and target exist, the slot lies in one of the target's rings (that ring is its
        // level), the slot names a well -, both ends pass the filter and differ
        if (r.tile < 0 || r.tile >= kTiles || r.target < 0 || r.target >= kN) continue;
        int lev = -1;
        for (int l = 0; l < levels; l++) if (r.slot >= c.tb.lvl_off[(size_t)r.target * (levels + 1) + l] && r.slot < c.tb.lvl_off[(size_t)r.target * (levels + 1) + l + 1]) { lev = l; break; }
        if (lev < 0) continue;
        const int b = c.tb.nbr[r.slot];
        if (b < 0 || b >= kN || !c.pf[r.tile][r.target] || !c.pf[r.tile][b] || b == r.target) continue;
        edges[(size_t)r.tile * levels + lev].push_back({r.target, b});
        t.kept++;
    }
    for (int tile = 0; tile < kTiles; tile++) {
        int64_t *row = t.rows.data() + tile * ns;
        std::vector<int> root(kN), size(kN, 1);
        std::vector<char> touched(kN, 0);
        std::iota(root.begin(), root.end(), 0);
        auto find = [&](int x) { while (root[x] != x) x = root[x] = root[root[x]]; return x; };
        for (int w = 0; w < kN; w++) row[0] += c.pf[tile][w];
        int64_t in_sets = 0, components = 0;       // of the wells an edge has touched
        for (int l = 0; l < levels; l++) {
            for (const auto &[a, b] : edges[(size_t)tile * levels + l]) {
                for (int x : {a, b}) if (!touched[x]) { touched[x] = 1; in_sets++; components++; }
                const int ra = find(a), rb = find(b);
                if (ra != rb) { root[ra] = rb; size[rb] += size[ra]; components--; }
            }
            row[1 + l] = components;                               // Sets: every touched well is in a component of two or more
            row[1 + levels + l] = in_sets;
            row[1 + 2 * levels + l] = in_sets - components;        // Redundant: the sum of (size - 1)
        }
        std::vector<int> smallest(kN, -1);
        for (int w = 0; w < kN; w++) {
            const int r = find(w);
            if (smallest[r] < 0) { smallest[r] = w; if (size[r] >= 2) row[1 + 3 * levels + std::min(size[r], kBins + 1) - 2]++; }
            if (c.pf[tile][w]) t.label[(size_t)tile * kN + w] = (uint32_t)smallest[r];
        }
        t.merges += row[3 * levels]; t.sets += row[levels];
    }
    return t;
}

// ---- the launches, as wd_dup_sets and process_edges make them ------------------------------------------------------
struct Args {
    const int32_t *centre, *lvl_off, *nbr; int levels, tile0, lev; int64_t n; const uint8_t *const *filt;
    uint32_t *parent, *aux, *flags; unsigned long long *cnt; int4 *rec; uint32_t *const *labels;
};
static Args A;
static void l_check() { k_sets_check_centres(A.centre, kN, A.flags); }
static void l_init() { k_sets_init(A.filt, kN, A.parent, A.aux, A.cnt); }
static void l_edges() { k_sets_edges(A.rec, A.n, A.tile0, kTiles, A.lvl_off, A.nbr, A.levels, kN, A.parent, A.aux, A.flags); }
static void l_union() { k_sets_union(A.rec, A.n, A.lev, kN, A.parent, A.cnt); }
static void l_compress() { k_sets_compress(A.parent, A.aux, kN, A.levels, A.cnt); }
static void l_count() { k_sets_count(A.parent, kN, A.aux); }
static void l_bins() { k_sets_bins(A.parent, A.aux, kN, A.labels, A.cnt); }

// which of k_sets_union's two counters a workgroup's hooks went to: seen from outside, in what the workgroup added
static Result *g_res;
static std::vector<unsigned long long> g_seen;     // the hook counters of the level, as they stood before the workgroup
static unsigned long long *hook_cell(int tile, unsigned bx) { return A.cnt + ((size_t)tile * kSpread + bx % kSpread) * kCnt + kCntHooks + A.lev; }
static void after_union_block(unsigned bx, unsigned)
{
    const int s_tile = A.rec[(size_t)bx * kSetsBlock].x;
    for (int t = 0; t < kTiles; t++) {
        unsigned long long &seen = g_seen[(size_t)t * kSpread + bx % kSpread], now = *hook_cell(t, bx);
        (t == s_tile ? g_res->lds_hooks : g_res->global_hooks) += (long)(now - seen);
        seen = now;
    }
}

// after a k_sets_union launch: pointers descend, every walk ends, the roots are the PF wells less the hooks counted
static bool check_forest(const Case &c)
{
    std::vector<uint32_t> root(kN);
    for (int t = 0; t < kTiles; t++) {
        long roots = 0, pf = 0, hooks = 0;
        for (int w = 0; w < kN; w++) {
            const uint32_t p = A.parent[(size_t)t * kN + w];
            if (!c.pf[t][w]) { if (p != kInvalid) return fail_("parent of non-PF well", w, p, kInvalid); continue; }
            pf++;
            if (p > (uint32_t)w) return fail_("parent above well", w, p, w);
            if (p != (uint32_t)w && !c.pf[t][p]) return fail_("parent of well is no PF well", w, p, -1);
            root[w] = p == (uint32_t)w ? p : root[p];              // (p < w: its root is known, so the walk from w ends)
            roots += p == (uint32_t)w;
        }
        for (int r = 0; r < kSpread; r++) for (int l = 0; l < c.levels; l++) hooks += (long)A.cnt[((size_t)t * kSpread + r) * kCnt + kCntHooks + l];
        if (roots != pf - hooks) return fail_("roots of tile", t, roots, pf - hooks);
    }
    return true;
}

static bool process_edges(const Case &c, const std::vector<int4> &recs, int tile0, bool permute, Buf<int4> &rec)
{
    if (recs.empty()) return true;
    memcpy((void *)rec.p, recs.data(), recs.size() * sizeof(int4));
    const unsigned blocks = (unsigned)((recs.size() + kSetsBlock - 1) / kSetsBlock);
    A.rec = rec.p; A.n = (int64_t)recs.size(); A.tile0 = tile0;
    run_grid(blocks, 1, l_edges, permute);
    for (int l = 0; l < c.levels; l++) {
        A.lev = l;
        for (int t = 0; t < kTiles; t++) for (int r = 0; r < kSpread; r++) g_seen[(size_t)t * kSpread + r] = *hook_cell(t, (unsigned)r);
        emu_after_block = after_union_block;
        run_grid(blocks, 1, l_union, permute);
        emu_after_block = nullptr;
        if (!check_forest(c)) return false;
    }
    return true;
}

static bool run(const Case &c, char way, const std::vector<Rec> &order, bool permute, Result &res)
{
    const int levels = c.levels;
    const Layout lay = layout_of(kN, kTiles);
    Buf<uint8_t> ws(lay.bytes), filt_store((size_t)kTiles * kN);
    Buf<uint32_t> labels((size_t)kTiles * kN);
    Buf<int4> rec(order.size());
    std::mt19937 rng(5);
    uint32_t **lbl = (uint32_t **)(ws.p + lay.lbl);
    const uint8_t **filt = (const uint8_t **)(ws.p + lay.filt);
    for (int t = 0; t < kTiles; t++) {
        for (int w = 0; w < kN; w++) filt_store[(size_t)t * kN + w] = (uint8_t)((rng() & 0xFE) | c.pf[t][w]);
        lbl[t] = labels.p + (size_t)t * kN; filt[t] = filt_store.p + (size_t)t * kN;
    }
    A = Args{c.tb.centre.data(), c.tb.lvl_off.data(), c.tb.nbr.data(), levels, 0, 0, 0, filt, (uint32_t *)(ws.p + lay.parent), (uint32_t *)(ws.p + lay.aux),
             (uint32_t *)(ws.p + lay.flags), (unsigned long long *)(ws.p + lay.cnt), rec.p, lbl};
    g_res = &res; g_seen.assign((size_t)kTiles * kSpread, 0);
    emu_cas_tag = kEmuUnion;                       // (the hooks of unite: the only compare-and-swaps here)
    const unsigned wblocks = (unsigned)((kN + kSetsBlock - 1) / kSetsBlock);
    memset(ws.p + lay.cnt, 0, lay.lbl - lay.cnt);
    run_grid(wblocks, 1, l_check, permute);
    if (A.flags[kFlagCentres]) return fail_("flag", kFlagCentres, A.flags[kFlagCentres], 0);
    run_grid(wblocks, kTiles, l_init, permute);
    if (way != 'c') {
        std::vector<int4> recs;
        for (const Rec &r : order) recs.push_back(make_int4(r.tile, r.target, r.slot, 0));
        if (!process_edges(c, recs, 0, permute, rec)) return false;
    } else {
        for (int i = 0; i < kTiles; i++) {         // the scan of tile i alone: its records carry tile 0
            std::vector<int4> recs;
            for (const Rec &r : order) if (r.scan == i) recs.push_back(make_int4(r.tile - i, r.target, r.slot, 0));
            if (!process_edges(c, recs, i, permute, rec)) return false;
        }
    }
    run_grid(wblocks, kTiles, l_compress, permute);
    memset(A.aux, 0, (size_t)kTiles * kN * sizeof(uint32_t));
    run_grid(wblocks, kTiles, l_count, permute);
    run_grid(wblocks, kTiles, l_bins, permute);
    const size_t ns = 1 + 3 * (size_t)levels + kBins;
    res.rows.assign(kTiles * ns, 0);
    for (int t = 0; t < kTiles; t++) sets_fold_row(A.cnt, t, levels, res.rows.data() + t * ns);
    res.label.assign(labels.p, labels.p + (size_t)kTiles * kN);
    res.flag_record = A.flags[kFlagRecord];
    return true;
}

static bool check(const Case &c, const Result &res, const SetsTruth &t)
{
    for (size_t g = 0; g < t.label.size(); g++) if (res.label[g] != t.label[g]) return fail_("label of well", (long)g, res.label[g], t.label[g]);
    for (size_t i = 0; i < t.rows.size(); i++) if (res.rows[i] != t.rows[i]) return fail_("rows, column", (long)i, (long)res.rows[i], (long)t.rows[i]);
    if (res.flag_record != (c.bad ? 1u : 0u)) return fail_("flag", kFlagRecord, res.flag_record, c.bad);
    return true;
}

int main()
{
    const int all_levels[4] = {1, 3, 8, kMaxLevels};
    g_case = 0;
    for (const char *family : kGraphFamilies) for (int levels : all_levels) {
        const std::string f = family;
        if (levels < 3 && (f == "ladder" || f == "late_merge" || f == "corners")) continue;      // (they need an inner and an outer level)
        if (f.compare(0, 4, "bad_") == 0 && levels != 1 && levels != 8) continue;
        const unsigned seed = 1000u * g_case;
        Case c = make_case(f, levels, seed);
        const SetsTruth truth = sets_truth_of(c);
        if (c.bad) {                               // "changes nothing else": the definitions of the case without its bad records
            Case plain = c;
            plain.recs.clear();
            for (const Rec &r : c.recs) if (r.tile >= 0 && r.tile < kTiles && r.target >= 0 && r.target < kN && r.slot >= 0 && r.slot < (int)c.tb.nbr.size() &&
                                            c.tb.nbr[r.slot] >= 0 && c.tb.nbr[r.slot] < kN && r.slot >= c.tb.lvl_off[(size_t)r.target * (levels + 1)] &&
                                            r.slot < c.tb.lvl_off[(size_t)r.target * (levels + 1) + levels]) plain.recs.push_back(r);
            const SetsTruth pt = sets_truth_of(plain);
            if (plain.recs.size() + 2 > c.recs.size() || pt.label != truth.label || pt.rows != truth.rows) { printf("MISMATCH case %d: the bad records of the case are not what they should be\n", g_case); return 1; }
        }
        Result first;
        for (char way : {'a', 'b', 'c'}) {
            g_way = way;
            std::vector<Rec> order = c.recs;
            std::stable_sort(order.begin(), order.end(), [](const Rec &x, const Rec &y) { return std::make_pair(x.scan, x.target) < std::make_pair(y.scan, y.target); });
            if (way == 'b') { std::mt19937 rng(seed + 77); std::shuffle(order.begin(), order.end(), rng); }
            long points = 0, never_lost = 0, lost = 0, lds = 0, glob = 0, wgs = 0, ragged = 1;
            for (int i = 0; i < kTiles; i++) {
                const long n = way == 'c' ? (long)std::count_if(order.begin(), order.end(), [&](const Rec &r) { return r.scan == i; }) : i ? 0 : (long)order.size();
                wgs = std::max(wgs, (n + kSetsBlock - 1) / kSetsBlock);
                if (n && n % kSetsBlock == 0) ragged = 0;
            }
            for (int s = 0; s < kSchedules; s++) {
                g_schedule = s;
                const bool permute = set_schedule(s, seed);
                Result res;
                if (!run(c, way, order, permute, res) || !check(c, res, truth)) return 1;
                if (way == 'a' && s == 0) first = res;
                else if (res.label != first.label || res.rows != first.rows) { printf("MISMATCH case %d way %c schedule %d: other labels or rows than way a's schedule 0\n", g_case, way, s); return 1; }
                if (s == 0) never_lost = emu_counts.lost[kEmuUnion];
                if (s >= 3) lost += emu_counts.lost[kEmuUnion];
                points += emu_counts.points; lds += res.lds_hooks; glob += res.global_hooks;
            }
            if (lds + glob != truth.merges * kSchedules) return !fail_("hooks seen per workgroup", 0, lds + glob, truth.merges * kSchedules);
            if (way == 'b' && truth.merges && !(lds && glob)) { printf("MISMATCH case %d way b: one of the two hook counters never ran (LDS %ld, global %ld)\n", g_case, lds, glob); return 1; }
            if (way == 'c' && glob) return !fail_("hooks counted globally, tile by tile", 0, glob, 0);
            printf("case %d ok: family %s levels %d way %c schedules %d records %zu wgs %ld ragged %ld kept %ld merges %ld sets %ld flag %d lds_hooks %ld "
                   "global_hooks %ld points %ld never_lost %ld lost %ld\n", g_case, family, levels, way, kSchedules, order.size(), wgs, ragged, truth.kept,
                   truth.merges, truth.sets, (int)c.bad, lds, glob, points, never_lost, lost);
            fflush(stdout);
        }
        g_case++;
    }
    return 0;
}
