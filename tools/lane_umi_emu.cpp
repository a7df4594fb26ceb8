// lane_umi_emu.cpp - k_lu_pairs and k_lu_group (csrc/lane_umi.inc), behind k_lc_reserve and k_lc_scatter
// (csrc/lane_consensus.inc), run on the CPU under shuffled schedules: the kernels' source is compiled as it stands, the
// 256 lanes of a workgroup are fibers (tools/wave_emu.h) that meet at every barrier, ballot and shuffle, LDS is the
// kernels' static storage, and the four launches follow each other as wd_lane_umi launches them (LaneRun's grid for the
// first three, lu_group_groups for the last) on a scratch that is cleared as far as the host call clears it and holds a
// pattern beyond.  Where a copy lands in its family's range, and which member number becomes the root of a component of
// the union-find in LDS, depend on the schedule, so every case runs under the eleven schedules of tools/emu_reads.h:
// under each, every output must be what the definitions of include/welldup_laneumi.h give, computed directly (a
// union by brute force over a family's pairs) - so every schedule gives the same.
// Cases: UMI reads of 1, 8, 10, 11 and 20 cycles (d inside one word, across the word boundary, in the second word
// alone); E = 0..3; tiles of less than a run and of a run and a bit; families of 2, 3, 63, 64, 65, 128, max_family and
// max_family + 1 wells (and many small ones) spread over both tiles; chains of 3, 64, 65 and 200 UMIs each one apart,
// the wells' ids ascending, descending and permuted along the chain; equal UMIs throughout, every UMI distinct, UMIs
// with N; max_family 2, 70, 130 and 1024.
// Prints MISMATCH and exits 1 on a difference.  With -DWAVE_EMU_TORN_CAS (the union's compare-and-swap torn: another
// fiber may hook the same root between its load and its store) it must do so: tests/test_laneumi_emu.py builds and runs
// both.  No GPU is involved, and nothing here says anything about time.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -Iinclude tools/lane_umi_emu.cpp -o lane_umi_emu
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
#define WD_LANE_CONSENSUS_EMU
#include "../well_duplicates_amd/csrc/lane_consensus.inc"
#define WD_LANE_UMI_EMU
#include "../well_duplicates_amd/csrc/lane_umi.inc"

struct Args {
    const int *tile_idx; int64_t N; const uint32_t *label, *members; const uint2 *key; int max_e, max_family; uint32_t W; int groups;
    unsigned long long *cursor, *cnt_t, *cnt_l, *cnt_r; uint32_t *slot, *region;
};
static Args A;
static void pairs() { k_lu_pairs(A.tile_idx, A.N, A.label, A.members, A.key, A.max_e, A.cnt_t, A.cnt_l); }
static void reserve() { k_lc_reserve(A.tile_idx, A.N, A.label, A.members, A.max_family, A.W, A.cursor, A.slot, A.region, A.cnt_r); }
static void scatter() { k_lc_scatter(A.tile_idx, A.N, A.label, A.members, A.max_family, A.slot, A.region); }
static void group() { k_lu_group(A.N, A.members, A.key, A.max_e, A.W, A.groups, A.cursor, A.slot, A.region, A.cnt_t, A.cnt_l); }

static int fail_(const char *what, int trial, int s, long a, long got, long want)
{
    printf("MISMATCH trial %d schedule %d (%s): %s %ld: %ld want %ld\n", trial, s, schedule_name(s), what, a, got, want);
    return 1;
}

typedef std::vector<uint8_t> Umi;
static int bin_of(long v) { return v <= 4 ? (int)v - 1 : v <= 8 ? 4 : v <= 16 ? 5 : v <= 64 ? 6 : 7; }
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

struct Trial { int U, E; int64_t N; int max_family; };

int main()
{
    std::mt19937 rng(17);
    const Trial trials[] = {{1, 0, 1000, 70}, {8, 1, 9000, 1024}, {10, 2, 1000, 130}, {11, 3, 9000, 130}, {20, 0, 1000, 130},
                            {1, 1, 9000, 70}, {8, 2, 1000, 130}, {10, 3, 1000, 70},   {11, 1, 1000, 130}, {20, 2, 9000, 130},
                            {20, 1, 1000, 2}, {10, 0, 9000, 130}};
    const int n_trials = (int)(sizeof(trials) / sizeof(trials[0]));
    for (int trial = 0; trial < n_trials; trial++) {
        const int U = trials[trial].U, E = trials[trial].E, max_family = trials[trial].max_family, T = 3;
        const int64_t N = trials[trial].N;
        int tiles[2] = {2, 0};                              // tile index 1 never added
        const size_t W = (size_t)N * T;
        std::vector<uint32_t> label(W, kInvalid), members(W, 0);
        std::vector<Umi> umi(W);
        std::vector<size_t> free_pf;
        for (int ti : tiles) for (int64_t w = 0; w < N; w++) {
            const size_t g = (size_t)ti * N + w;
            umi[g] = random_read(rng, U, 15);
            if (rng() % 10) { label[g] = (uint32_t)g; free_pf.push_back(g); }
        }
        std::shuffle(free_pf.begin(), free_pf.end(), rng);  // (a family's wells lie anywhere on both tiles)
        // the families: the sizes and the chains every case has, then small ones while the wells last (a fifth is left single)
        struct Plan { int n, kind; };                       // kind 0: equal UMIs; 1: every UMI random; 2: a few centres with errors; 3: with N; 4, 5, 6: a chain, ids ascending, descending, permuted
        std::vector<Plan> plan = {{2, 0}, {2, 1}, {3, 2}, {63, 2}, {64, 2}, {65, 2}, {128, 2}, {max_family, 2}, {max_family + 1, 1},
                                  {3, 4}, {3, 5}, {64, 6}, {65, 5}, {65, 6}, {200, 4 + trial % 3}, {64, 0}, {65, 0}, {64, 1}, {65, 1}, {66, 3}, {9, 3}};
        size_t need = 0; for (const Plan &p : plan) need += p.n;
        while (need + 6 < free_pf.size() * 4 / 5) { const int n = 2 + (int)(rng() % 4) * (int)(rng() % 2); plan.push_back(Plan{n, (int)(rng() % 4)}); need += n; }
        std::vector<std::vector<size_t>> fam;
        size_t used = 0;
        long chains = 0;
        for (const Plan &p : plan) {
            const int n = p.n;
            if (n < 2 || used + n > free_pf.size()) continue;
            std::vector<size_t> m(free_pf.begin() + used, free_pf.begin() + used + n); used += n;
            std::sort(m.begin(), m.end());
            std::vector<Umi> u(n);
            if (p.kind >= 4) {
                u = chain_of(rng, U, n); chains++;
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
        for (size_t g = 0; g < W; g++) if (!umi[g].empty()) {
            uint32_t k[2] = {0, 0};
            for (int c = 0; c < U; c++) k[c / 10] |= (uint32_t)umi[g][c] << (3 * (c % 10));
            key[g] = make_uint2(k[0], k[1]);
        }
        // the definitions, directly
        std::vector<long long> want_l(27, 0), want_t((size_t)T * 3, 0);
        long second_word = 0, n_largest = 0;
        for (const auto &m : fam) {
            const int n = (int)m.size();
            if (n > max_family) { want_l[9]++; want_l[10] += n; continue; }
            n_largest = std::max<long>(n_largest, n);
            std::vector<int> root(n);
            for (int i = 0; i < n; i++) root[i] = i;
            auto find = [&](int x) { while (root[x] != x) x = root[x] = root[root[x]]; return x; };
            std::set<Umi> distinct;
            for (int i = 0; i < n; i++) {
                distinct.insert(umi[m[i]]);
                for (int j = 0; j < i; j++) {
                    const int d = dist_of(umi[m[i]], umi[m[j]]);
                    if (d > E) continue;
                    if (d > 0 && U > 10 && std::equal(umi[m[i]].begin(), umi[m[i]].begin() + 10, umi[m[j]].begin())) second_word++;
                    root[find(i)] = find(j);
                }
            }
            std::map<int, std::vector<size_t>> comp;
            for (int i = 0; i < n; i++) comp[find(i)].push_back(m[i]);      // (m ascends: a component's first entry is its smallest id)
            const long mols = (long)comp.size();
            want_l[3]++; want_l[4] += mols; want_l[5] += (long long)distinct.size();
            if (mols >= 2) { want_l[6]++; want_l[7] += n; }
            want_l[11 + bin_of(mols)]++;
            for (const auto &[r, wells] : comp) {
                want_l[19 + bin_of((long)wells.size())]++;
                for (size_t g : wells) {
                    long long *t = &want_t[(g / (size_t)N) * 3];
                    t[0]++; t[1] += g != wells[0]; t[2] += wells.size() == 1;
                }
            }
            for (size_t g : m) want_l[8] += std::count(umi[g].begin(), umi[g].end(), 4) > 0;
        }
        for (int t = 0; t < T; t++) for (int f = 0; f < 3; f++) want_l[f] += want_t[(size_t)t * 3 + f];
        // the scratch: cleared as far as the host call clears it, a pattern beyond
        const LuLayout lay = lu_layout_of(T, N);
        Buf<uint8_t> sc(lay.bytes);
        const unsigned gx = (unsigned)((N + kLaneRun - 1) / kLaneRun), groups = lu_group_groups(W);
        long points = 0, lost = 0;
        for (int s = 0; s < kSchedules; s++) {
            sc.fill(s % 2 ? 0x5A : 0xA5);
            memset(sc.p, 0, lay.cleared);
            memcpy(sc.p + lay.tidx, tiles, sizeof(tiles));
            A = Args{(const int *)(sc.p + lay.tidx), N, label.data(), members.data(), key.data(), E, max_family, (uint32_t)W, (int)groups,
                     (unsigned long long *)(sc.p + lay.cursor), (unsigned long long *)(sc.p + lay.cnt_t), (unsigned long long *)(sc.p + lay.cnt_l),
                     (unsigned long long *)(sc.p + lay.cnt_r), (uint32_t *)(sc.p + lay.slot), (uint32_t *)(sc.p + lay.region)};
            const bool permute = set_schedule(s, (unsigned)trial);
            emu_cas_tag = kEmuUnion;
            run_grid(gx, 2, pairs, permute);
            run_grid(gx, 2, reserve, permute);
            run_grid(gx, 2, scatter, permute);
            run_grid(groups, 1, group, permute);
            points += emu_counts.points; lost += emu_counts.lost[kEmuUnion];
            std::vector<long long> got_l(27, 0);
            for (int t = 0; t < T; t++) for (int f = 0; f < 3; f++) {
                unsigned long long v = 0; for (int r = 0; r < kSpread; r++) v += A.cnt_t[((size_t)t * kSpread + r) * 3 + f];
                if ((long long)v != want_t[(size_t)t * 3 + f]) return fail_("tile counter", trial, s, t * 3 + f, (long)v, (long)want_t[(size_t)t * 3 + f]);
                got_l[f] += (long long)v;
            }
            unsigned long long c[kLuLaneCnt], r[kLcLaneCnt];
            for (int f = 0; f < kLuLaneCnt; f++) { c[f] = 0; for (int q = 0; q < kSpread; q++) c[f] += A.cnt_l[(size_t)q * kLuLaneCnt + f]; }
            for (int f = 0; f < kLcLaneCnt; f++) { r[f] = 0; for (int q = 0; q < kSpread; q++) r[f] += A.cnt_r[(size_t)q * kLcLaneCnt + f]; }
            for (int f = 0; f < 6; f++) got_l[3 + f] = (long long)c[kLuFamilies + f];
            got_l[9] = (long long)r[kLcLarge]; got_l[10] = (long long)r[kLcLargeWells];
            for (int b = 0; b < 16; b++) got_l[11 + b] = (long long)c[kLuPerFamily + b];
            for (int f = 0; f < 27; f++) if (got_l[f] != want_l[f]) return fail_("lane row column", trial, s, f, (long)got_l[f], (long)want_l[f]);
        }
        printf("case %d ok: U %d E %d N %ld max_family %d schedules %d wells %lld redundant %lld lone %lld families %lld molecules %lld distinct %lld "
               "split %lld with_n %lld large %lld largest %ld chains %ld second_word %ld big_molecules %lld points %ld lost %ld\n",
               trial, U, E, (long)N, max_family, kSchedules, want_l[0], want_l[1], want_l[2], want_l[3], want_l[4], want_l[5], want_l[6], want_l[8],
               want_l[9], n_largest, chains, second_word, want_l[26], points, lost);
    }
    return 0;
}
