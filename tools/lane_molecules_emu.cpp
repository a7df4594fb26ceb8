// lane_molecules_emu.cpp - k_lu_pairs_mol and k_lu_group_mol (csrc/lane_umi.inc), behind k_lc_reserve and k_lc_scatter
// (csrc/lane_consensus.inc), and then k_lk_score and k_lk_mark (csrc/lane_keep.inc) on what they wrote, run on the CPU
// under shuffled schedules: the kernels' source is compiled as it stands, the 256 lanes of a workgroup are fibers
// (tools/wave_emu.h), and the launches follow each other as wd_lane_umi_molecules and wd_lane_keep_molecules queue them -
// the memsets of a tile never added, LaneRun's grid for the pairs, the reservation and the scatter, lu_group_groups for
// the grouping, LaneRun's grid again for the scores and the marks with mol and molmem in the places of label and
// members.  Every buffer is a heap block of exactly its size (the address sanitizer sees a word beyond it), mol and
// molmem hold a pattern before every run, and every store to them is counted (WD_LANE_MOL_EMU_STORE in lu_emit): each
// word must have been written exactly once.  Under each of the eleven schedules of tools/emu_reads.h every word of mol
// and molmem, every cell of the UMI rows, every mask byte and every cell of the keep rows must be what the definitions
// of include/welldup_lanemolecules.h give, computed directly (a union by brute force over a family's pairs, the best of
// a molecule by a loop) - so every schedule gives the same.
// Cases: UMI reads of 1, 8, 10, 11 and 20 cycles; E = 0..3 and E >= U; N % 4 = 1, 2 and 3, tiles of less than a run and
// of a run and a bit; families of 2, 3, 63, 64, 65, 128, max_family and max_family + 1 wells (and many small ones)
// spread over both tiles; chains of 3, 64, 65 and 200 UMIs each one apart, ids ascending, descending and permuted
// (every length in every order where max_family lets a chain of 200 be gathered);
// equal UMIs throughout, every UMI distinct, UMIs with N; max_family 2, 70 and 1024; wells all of one score (the
// smallest id of a molecule must win) among random ones.
// Prints MISMATCH and exits 1 on a difference.  With -DWAVE_EMU_TORN_CAS (the union's compare-and-swap torn) it must do
// so: tests/test_lanemolecules_emu.py builds and runs both.  No GPU is involved, and nothing here says anything about
// time.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -Iinclude tools/lane_molecules_emu.cpp -o lane_molecules_emu
#define WAVE_EMU_UNIT_DEFS
#include "wave_emu.h"
#include "emu_reads.h"
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
#define WD_LANE_MISMATCH_EMU
#include "../well_duplicates_amd/csrc/lane_mismatch.inc"
#define WD_LANE_GC_EMU
#include "../well_duplicates_amd/csrc/lane_gc.inc"
#define WD_LANE_CONSENSUS_EMU
#include "../well_duplicates_amd/csrc/lane_consensus.inc"
static std::vector<int> emu_mol_stores;             // per well: the calls of lu_emit (and the host's memsets, below)
#define WD_LANE_MOL_EMU_STORE(g) (emu_mol_stores[(g)]++)
#define WD_LANE_UMI_EMU
#include "../well_duplicates_amd/csrc/lane_umi.inc"
#define WD_LANE_KEEP_EMU
#include "../well_duplicates_amd/csrc/lane_keep.inc"

// a heap block of exactly n elements, holding a pattern no kernel may depend on
template <class T> struct Heap {
    T *p; size_t n;
    explicit Heap(size_t count) : p((T *)malloc(count * sizeof(T))), n(count) { fill(0xA5); }
    ~Heap() { free((void *)p); }
    Heap(const Heap &) = delete;
    void fill(int byte) { if (n) memset((void *)p, byte, n * sizeof(T)); }
    T &operator[](size_t i) { return p[i]; }
};

struct Args {
    const int *tile_idx; int64_t N; const uint32_t *label, *members; const uint2 *key; int max_e, max_family; uint32_t W; int groups;
    unsigned long long *cursor, *cnt_t, *cnt_l, *cnt_r; uint32_t *slot, *region, *mol, *molmem;
    const uint32_t *qrows; int words; LkWeights wts; uint16_t *score; unsigned long long *best; uint8_t *const *maskp;
    unsigned long long *kcnt_t, *kcnt_l;
};
static Args A;
static void pairs() { k_lu_pairs_mol(A.tile_idx, A.N, A.label, A.members, A.key, A.max_e, A.max_family, A.cnt_t, A.cnt_l, A.mol, A.molmem); }
static void reserve() { k_lc_reserve(A.tile_idx, A.N, A.label, A.members, A.max_family, A.W, A.cursor, A.slot, A.region, A.cnt_r); }
static void scatter() { k_lc_scatter(A.tile_idx, A.N, A.label, A.members, A.max_family, A.slot, A.region); }
static void group() { k_lu_group_mol(A.N, A.members, A.key, A.max_e, A.W, A.groups, A.cursor, A.slot, A.region, A.cnt_t, A.cnt_l, A.mol, A.molmem); }
static void score_() { k_lk_score(A.tile_idx, A.N, A.mol, A.molmem, A.qrows, A.words, A.wts, A.score, A.best); }
static void mark_() { k_lk_mark(A.tile_idx, A.N, A.mol, A.molmem, A.score, A.best, A.maskp, A.kcnt_t, A.kcnt_l); }

static int fail_(const char *what, int trial, int s, long a, long long got, long long want)
{
    printf("MISMATCH trial %d schedule %d (%s): %s %ld: %lld want %lld\n", trial, s, schedule_name(s), what, a, got, want);
    return 1;
}

typedef std::vector<uint8_t> Umi;
static int bin_of(long v) { return v <= 4 ? (int)v - 1 : v <= 8 ? 4 : v <= 16 ? 5 : v <= 64 ? 6 : 7; }
static int gain_bin(long g) { return g == 0 ? 0 : g < 10 ? 1 : g < 20 ? 2 : g < 50 ? 3 : g < 100 ? 4 : g < 200 ? 5 : g < 500 ? 6 : 7; }
static int dist_of(const Umi &a, const Umi &b) { int d = 0; for (size_t c = 0; c < a.size(); c++) d += a[c] != b[c]; return d; }

// n UMIs, each one cycle from the last: step i changes cycle i % U
static std::vector<Umi> chain_of(std::mt19937 &rng, int U, int n)
{
    std::vector<Umi> out;
    Umi r = random_read(rng, U, 0);
    for (int i = 0; i < n; i++) {
        if (i) { const int c = i % U; r[c] = (uint8_t)((r[c] + 1 + rng() % 3) % 4); }
        out.push_back(r);
    }
    return out;
}

struct Trial { int U, E; int64_t N; int max_family, L; };

int main()
{
    std::mt19937 rng(31);
    const int edges[8] = {0, 2, 8, 14, 20, 26, 32, 38};
    const Trial trials[] = {{1, 0, 1001, 70, 9},  {8, 1, 9002, 1024, 25}, {10, 2, 1003, 70, 12}, {11, 3, 9001, 1024, 9},
                            {20, 0, 1002, 70, 25}, {1, 1, 1001, 70, 12},   {20, 1, 1003, 2, 9},   {8, 2, 1002, 70, 12}};
    const int n_trials = (int)(sizeof(trials) / sizeof(trials[0]));
    for (int trial = 0; trial < n_trials; trial++) {
        const int U = trials[trial].U, E = trials[trial].E, max_family = trials[trial].max_family, L = trials[trial].L, T = 3;
        const int words = (L + 9) / 10, min_q = trial % 3 == 2 ? 0 : 15;
        const int64_t N = trials[trial].N;
        int tiles[2] = {2, 0};                              // tile index 1 never added
        const size_t W = (size_t)N * T;
        int w8[8];
        for (int b = 0; b < 8; b++) w8[b] = edges[b] >= min_q ? edges[b] : 0;
        const LkWeights wts = lk_weights_of(w8);
        std::vector<uint32_t> label(W, kInvalid), members(W, 0);
        std::vector<Umi> umi(W);
        std::vector<std::vector<uint8_t>> code(W);          // the quality bin of every cycle, per well of an added tile
        std::vector<size_t> free_pf;
        for (int ti : tiles) for (int64_t w = 0; w < N; w++) {
            const size_t g = (size_t)ti * N + w;
            umi[g] = random_read(rng, U, 15);
            code[g].resize(L);
            const bool flat = rng() % 3 == 0;               // a third of the wells all of one bin: equal scores
            for (int c = 0; c < L; c++) code[g][c] = flat ? 5 : (uint8_t)(rng() % 8);
            if (rng() % 10) { label[g] = (uint32_t)g; free_pf.push_back(g); }
        }
        std::shuffle(free_pf.begin(), free_pf.end(), rng);  // (a family's wells lie anywhere on both tiles)
        // the families: the sizes and the chains every case has, then small ones while the wells last (a fifth is left single)
        struct Plan { int n, kind; };                       // kind 0: equal UMIs; 1: every UMI random; 2: a few centres with errors; 3: with N; 4, 5, 6: a chain, ids ascending, descending, permuted
        std::vector<Plan> plan = {{2, 0}, {2, 1}, {3, 2}, {63, 2}, {64, 2}, {65, 2}, {128, 2}, {max_family, 2}, {max_family + 1, 1},
                                  {3, 4}, {3, 5}, {64, 6}, {65, 5}, {65, 6}, {200, 4 + trial % 3}, {64, 0}, {65, 0}, {64, 1}, {65, 1}, {66, 3}, {9, 3}};
        if (max_family >= 200)                              // where a chain of 200 is gathered: every order of it, and of the short ones
            for (const Plan &p : {Plan{200, 4}, Plan{200, 5}, Plan{200, 6}, Plan{3, 6}, Plan{64, 4}, Plan{64, 5}, Plan{65, 4}}) plan.push_back(p);
        size_t need = 0; for (const Plan &p : plan) need += p.n;
        while (need + 6 < free_pf.size() * 4 / 5) { const int n = 2 + (int)(rng() % 4) * (int)(rng() % 2); plan.push_back(Plan{n, (int)(rng() % 4)}); need += n; }
        std::vector<std::vector<size_t>> fam;
        size_t used = 0;
        long chains = 0, chains_200 = 0;                     // the chains that are gathered (a Large family's UMIs are never looked at); those of 200: a bit per order
        for (const Plan &p : plan) {
            const int n = p.n;
            if (n < 2 || used + n > free_pf.size()) continue;
            std::vector<size_t> m(free_pf.begin() + used, free_pf.begin() + used + n); used += n;
            std::sort(m.begin(), m.end());
            std::vector<Umi> u(n);
            if (p.kind >= 4) {
                u = chain_of(rng, U, n);
                if (n <= max_family) { chains++; if (n == 200) chains_200 |= 1 << (p.kind - 4); }
                if (p.kind == 5) std::reverse(u.begin(), u.end());
                if (p.kind == 6) std::shuffle(u.begin(), u.end(), rng);
            } else {
                std::vector<Umi> centre;
                for (int i = 0; i < 3; i++) centre.push_back(random_read(rng, U, p.kind == 3 ? 3 : 0));
                for (int j = 0; j < n; j++) {
                    if (p.kind == 0) u[j] = centre[0];
                    else if (p.kind == 1) u[j] = random_read(rng, U, 0);
                    else { u[j] = centre[rng() % 3]; if (rng() % 3 == 0) u[j][rng() % U] = (uint8_t)(rng() % (p.kind == 3 ? 5 : 4)); }
                }
            }
            for (int j = 0; j < n; j++) { umi[m[j]] = u[j]; label[m[j]] = (uint32_t)m[0]; }
            members[m[0]] = (uint32_t)(n - 1);
            fam.push_back(m);
        }
        std::vector<uint2> key(W, make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu));
        std::vector<uint32_t> qrows(W * words, 0xFFFFFFFFu);
        for (size_t g = 0; g < W; g++) if (!umi[g].empty()) {
            uint32_t k[2] = {0, 0};
            for (int c = 0; c < U; c++) k[c / 10] |= (uint32_t)umi[g][c] << (3 * (c % 10));
            key[g] = make_uint2(k[0], k[1]);
            for (int q = 0; q < words; q++) qrows[g * words + q] = 0;
            for (int c = 0; c < L; c++) qrows[g * words + c / 10] |= (uint32_t)code[g][c] << (3 * (c % 10));
        }
        // the definitions, directly: the molecules and the UMI rows
        std::vector<uint32_t> want_mol(W, kInvalid), want_mem(W, 0);
        for (size_t g = 0; g < W; g++) if (label[g] != kInvalid) want_mol[g] = (uint32_t)g;      // a Single, unless a family says otherwise
        std::vector<long long> want_l(27, 0), want_t((size_t)T * 3, 0);
        long n_largest = 0, big = 0, joined_pairs = 0, split_pairs = 0;
        for (const auto &m : fam) {
            const int n = (int)m.size();
            if (n > max_family) {                           // one molecule, as the finish left it
                want_l[9]++; want_l[10] += n;
                for (size_t g : m) want_mol[g] = (uint32_t)m[0];
                want_mem[m[0]] = (uint32_t)(n - 1);
                continue;
            }
            n_largest = std::max<long>(n_largest, n);
            big += n > 64;
            std::vector<int> root(n);
            for (int i = 0; i < n; i++) root[i] = i;
            auto find = [&](int x) { while (root[x] != x) x = root[x] = root[root[x]]; return x; };
            std::set<Umi> distinct;
            for (int i = 0; i < n; i++) {
                distinct.insert(umi[m[i]]);
                for (int j = 0; j < i; j++)
                    if (dist_of(umi[m[i]], umi[m[j]]) <= E) root[find(i)] = find(j);
            }
            std::map<int, std::vector<size_t>> comp;
            for (int i = 0; i < n; i++) comp[find(i)].push_back(m[i]);      // (m ascends: a component's first entry is its smallest id)
            const long mols = (long)comp.size();
            if (n == 2) (mols == 1 ? joined_pairs : split_pairs)++;
            want_l[3]++; want_l[4] += mols; want_l[5] += (long long)distinct.size();
            if (mols >= 2) { want_l[6]++; want_l[7] += n; }
            want_l[11 + bin_of(mols)]++;
            for (const auto &[r, wells] : comp) {
                want_l[19 + bin_of((long)wells.size())]++;
                want_mem[wells[0]] = (uint32_t)(wells.size() - 1);
                for (size_t g : wells) {
                    want_mol[g] = (uint32_t)wells[0];
                    long long *t = &want_t[(g / (size_t)N) * 3];
                    t[0]++; t[1] += g != wells[0]; t[2] += wells.size() == 1;
                }
            }
            for (size_t g : m) want_l[8] += std::count(umi[g].begin(), umi[g].end(), 4) > 0;
        }
        for (int t = 0; t < T; t++) for (int f = 0; f < 3; f++) want_l[f] += want_t[(size_t)t * 3 + f];
        // the keep by molecule, and by family for what it would have dropped
        std::vector<long long> sc(W, 0), kwant_t((size_t)T * kLkTileCnt, 0), kwant_l(kLkLaneCnt, 0);
        std::vector<uint8_t> want_mask(W, 0);
        std::map<uint32_t, std::vector<size_t>> molecules, families;
        for (size_t g = 0; g < W; g++) if (!code[g].empty()) {
            for (int c = 0; c < L; c++) sc[g] += w8[code[g][c]];
            if (label[g] != kInvalid) { molecules[want_mol[g]].push_back(g); families[label[g]].push_back(g); }
        }
        long dropped = 0, dropped_by_family = 0, ties = 0;
        for (const auto &[root, wells] : families) dropped_by_family += (long)wells.size() - 1;
        for (const auto &[first, wells] : molecules) {
            size_t best = wells[0];
            for (size_t g : wells) { if (sc[g] > sc[best]) best = g; else if (g != best && sc[g] == sc[best]) ties++; }      // (ascending: the first of the largest is the smallest id)
            if (wells.size() > 1) {
                kwant_l[kLkFamilies]++; kwant_l[kLkMoved] += best != first; kwant_l[kLkSumRoots] += sc[first];
                kwant_l[kLkGain + gain_bin((long)(sc[best] - sc[first]))]++;
            }
            for (size_t g : wells) {
                long long *t = &kwant_t[(g / N) * kLkTileCnt];
                const bool kept = g == best;
                t[0]++; t[kept ? 1 : 2]++; t[3] += kept && g != first; t[kept ? 4 : 5] += sc[g];
                want_mask[g] = kept; dropped += !kept;
            }
        }
        for (const auto &[root, wells] : families) {        // identity 7: whatever a family keeps, its molecule keeps
            size_t best = wells[0];
            for (size_t g : wells) if (sc[g] > sc[best]) best = g;
            if (!want_mask[best]) return fail_("the family's kept well, dropped by molecule", trial, 0, (long)best, 0, 1);
        }
        if (dropped > dropped_by_family) return fail_("wells dropped by molecule against by family", trial, 0, 0, dropped, dropped_by_family);
        // the buffers: heap blocks of exactly their sizes
        const LuLayout lay = lu_layout_of(T, N);            // (for what a call clears; the parts are blocks of their own here)
        (void)lay;
        Heap<unsigned long long> cnt_t((size_t)T * kSpread * kLuTileCnt), cnt_l((size_t)kSpread * kLuLaneCnt), cnt_r((size_t)kSpread * kLcLaneCnt), cursor(1);
        Heap<uint32_t> slot(W), region(W), mol(W), molmem(W);
        Heap<uint16_t> score(W);
        Heap<unsigned long long> best(W), kcnt_t((size_t)T * kSpread * kLkTileCnt), kcnt_l((size_t)kSpread * kLkLaneCnt);
        Heap<uint8_t> mask(W);
        Heap<int> tidx(T);
        const unsigned gx = (unsigned)((N + kLaneRun - 1) / kLaneRun), groups = lu_group_groups(W);
        long points = 0, lost = 0;
        for (int s = 0; s < kSchedules; s++) {
            const int dirt = s % 2 ? 0x5A : 0xA5;
            slot.fill(dirt); region.fill(dirt); mol.fill(dirt); molmem.fill(dirt); score.fill(dirt); mask.fill(0xA5); tidx.fill(dirt);
            cnt_t.fill(0); cnt_l.fill(0); cnt_r.fill(0); cursor.fill(0);      // what the host call clears
            memcpy(tidx.p, tiles, sizeof(tiles));
            emu_mol_stores.assign(W, 0);
            for (int t = 0; t < T; t++) if (t != tiles[0] && t != tiles[1])   // the host's memsets of a tile never added
                for (int64_t w = 0; w < N; w++) { const size_t g = (size_t)t * N + w; mol[g] = kInvalid; molmem[g] = 0; emu_mol_stores[g]++; }
            uint8_t *maskp[T] = {mask.p, nullptr, mask.p + 2 * N};
            A = Args{tidx.p, N, label.data(), members.data(), key.data(), E, max_family, (uint32_t)W, (int)groups, cursor.p, cnt_t.p, cnt_l.p,
                     cnt_r.p, slot.p, region.p, mol.p, molmem.p, qrows.data(), words, wts, score.p, best.p, maskp, kcnt_t.p, kcnt_l.p};
            const bool permute = set_schedule(s, (unsigned)trial);
            emu_cas_tag = kEmuUnion;
            run_grid(gx, 2, pairs, permute);
            run_grid(gx, 2, reserve, permute);
            run_grid(gx, 2, scatter, permute);
            run_grid(groups, 1, group, permute);
            for (size_t g = 0; g < W; g++) {
                if (emu_mol_stores[g] != 1) return fail_("stores to the entry of well", trial, s, (long)g, emu_mol_stores[g], 1);
                if (mol[g] != want_mol[g]) return fail_("mol of well", trial, s, (long)g, mol[g], want_mol[g]);
                if (molmem[g] != want_mem[g]) return fail_("molmem of well", trial, s, (long)g, molmem[g], want_mem[g]);
            }
            std::vector<long long> got_l(27, 0);
            for (int t = 0; t < T; t++) for (int f = 0; f < 3; f++) {
                unsigned long long v = 0; for (int r = 0; r < kSpread; r++) v += cnt_t[((size_t)t * kSpread + r) * 3 + f];
                if ((long long)v != want_t[(size_t)t * 3 + f]) return fail_("umi tile counter", trial, s, t * 3 + f, (long long)v, want_t[(size_t)t * 3 + f]);
                got_l[f] += (long long)v;
            }
            unsigned long long c[kLuLaneCnt], r[kLcLaneCnt];
            for (int f = 0; f < kLuLaneCnt; f++) { c[f] = 0; for (int q = 0; q < kSpread; q++) c[f] += cnt_l[(size_t)q * kLuLaneCnt + f]; }
            for (int f = 0; f < kLcLaneCnt; f++) { r[f] = 0; for (int q = 0; q < kSpread; q++) r[f] += cnt_r[(size_t)q * kLcLaneCnt + f]; }
            for (int f = 0; f < 6; f++) got_l[3 + f] = (long long)c[kLuFamilies + f];
            got_l[9] = (long long)r[kLcLarge]; got_l[10] = (long long)r[kLcLargeWells];
            for (int b = 0; b < 16; b++) got_l[11 + b] = (long long)c[kLuPerFamily + b];
            for (int f = 0; f < 27; f++) if (got_l[f] != want_l[f]) return fail_("umi lane row column", trial, s, f, got_l[f], want_l[f]);
            // the keep on what they wrote, as wd_lane_keep_molecules launches it
            best.fill(0xFF); kcnt_t.fill(0); kcnt_l.fill(0);
            run_grid(gx, 2, score_, permute);
            run_grid(gx, 2, mark_, permute);
            points += emu_counts.points; lost += emu_counts.lost[kEmuUnion];
            for (size_t g = 0; g < W; g++) {
                const bool added = !code[g].empty();
                const uint8_t want = added ? want_mask[g] : 0xA5;
                if (mask[g] != want) return fail_("mask of well", trial, s, (long)g, mask[g], want);
            }
            for (int t = 0; t < T; t++) for (int f = 0; f < kLkTileCnt; f++) {
                unsigned long long v = 0; for (int q = 0; q < kSpread; q++) v += kcnt_t[((size_t)t * kSpread + q) * kLkTileCnt + f];
                if ((long long)v != kwant_t[(size_t)t * kLkTileCnt + f]) return fail_("keep tile counter", trial, s, t * 100 + f, (long long)v, kwant_t[(size_t)t * kLkTileCnt + f]);
            }
            for (int f = 0; f < kLkLaneCnt; f++) {
                unsigned long long v = 0; for (int q = 0; q < kSpread; q++) v += kcnt_l[(size_t)q * kLkLaneCnt + f];
                if ((long long)v != kwant_l[f]) return fail_("keep lane counter", trial, s, f, (long long)v, kwant_l[f]);
            }
        }
        printf("case %d ok: U %d E %d N %ld max_family %d schedules %d wells %lld molecules %lld redundant %lld large %lld largest %ld big %ld "
               "chains %ld chains_200 %ld joined_pairs %ld split_pairs %ld kept_molecules %lld moved %lld dropped %ld dropped_by_family %ld ties %ld points %ld lost %ld\n",
               trial, U, E, (long)N, max_family, kSchedules, want_l[0], want_l[4], want_l[1], want_l[9], n_largest, big, chains, chains_200, joined_pairs,
               split_pairs, kwant_l[kLkFamilies], kwant_l[kLkMoved], dropped, dropped_by_family, ties, points, lost);
    }
    return 0;
}
