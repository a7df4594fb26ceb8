// lane_consensus_emu.cpp - k_lc_reserve, k_lc_scatter and k_lc_vote (csrc/lane_consensus.inc) run on the CPU: the
// kernels' source is compiled as it stands, the 256 lanes of a workgroup are fibers (tools/wave_emu.h) that meet at every
// barrier, ballot and shuffle, LDS is the kernels' static storage, and the three launches follow each other with the
// grids the host call gives them (LaneRun's for the first two, lc_vote_groups for the third) on a scratch that is cleared
// as far as the host call clears it and holds a pattern beyond.  Where a copy lands in its family's range depends on
// the schedule, so every case runs under the eleven schedules of tools/emu_reads.h: under each, every family's range
// must be a permutation of its copies, the table a permutation of the voted roots, and every output what the
// definitions of include/welldup_laneconsensus.h give, computed directly - so every schedule gives the same.
// Cases: rows of 1, 3, 4, 6, 16 and 103 words; tiles of less than a run and of a run and a bit; families of 2, 3, 4, 63,
// 64, 65, max_family and max_family + 1 wells (and many small ones) spread over both tiles, with errors, no-calls,
// ties (2 / 2, 2 / 2 / 1, three codes in three wells) and members further than 7 from the vote; every max_d.
// Prints MISMATCH and exits 1 on a difference.  With -DWAVE_EMU_TORN_ADD (an add that another fiber may cut in two) it
// must do so: tests/test_laneconsensus_emu.py builds and runs both.  No GPU is involved, and nothing here says
// anything about time.
//
//   g++ -O1 -g -std=c++17 -fsanitize=undefined -Iinclude tools/lane_consensus_emu.cpp -o lane_consensus_emu
#include "wave_emu.h"
#include "emu_reads.h"
#define WD_LANE_MISMATCH_EMU
#include "../well_duplicates_amd/csrc/lane_mismatch.inc"
#define WD_LANE_CONSENSUS_EMU
#include "../well_duplicates_amd/csrc/lane_consensus.inc"

struct Args {
    const int *tile_idx; int64_t N; const uint32_t *label, *members, *rows; int words, L, max_d, max_family; uint32_t W; int groups;
    unsigned long long *cursor, *cnt_t, *cnt_l, *calls; uint32_t *slot, *region;
};
static Args A;
static void reserve() { k_lc_reserve(A.tile_idx, A.N, A.label, A.members, A.max_family, A.W, A.cursor, A.slot, A.region, A.cnt_l); }
static void scatter() { k_lc_scatter(A.tile_idx, A.N, A.label, A.members, A.max_family, A.slot, A.region); }
static void vote() { k_lc_vote(A.N, A.members, A.rows, A.words, A.L, A.max_d, A.W, A.groups, A.cursor, A.slot, A.region, A.cnt_t, A.cnt_l, A.calls); }

static int fail_(const char *what, int trial, int s, long a, long got, long want)
{
    printf("MISMATCH trial %d schedule %d (%s): %s %ld: %ld want %ld\n", trial, s, schedule_name(s), what, a, got, want);
    return 1;
}

int main()
{
    std::mt19937 rng(11);
    const int Ls[] = {9, 25, 40, 51, 151, 1024};            // rows of 1, 3, 4, 6, 16 and 103 words
    for (int trial = 0; trial < 12; trial++) {
        const int i = trial % 6, round = trial / 6;
        const int L = Ls[i], words = (L + 9) / 10, T = 3, max_d = (trial * 3 + 1) % 8;
        const int64_t N = (i + round) % 2 ? 9000 : 700;     // two runs per tile, the second partial; or a partial one
        const int max_family = trial == 1 ? 4096 : trial % 3 == 0 ? 64 : 70;       // (trial 1: N 9000, L 25)
        int tiles[2] = {2, 0};                              // tile index 1 never added
        const size_t W = (size_t)N * T;
        std::vector<uint32_t> label(W, kInvalid), members(W, 0), rows(W * words, 0xFFFFFFFFu);
        std::vector<std::vector<uint8_t>> code(W);
        std::vector<size_t> free_pf;
        for (int ti : tiles) for (int64_t w = 0; w < N; w++) {
            const size_t g = (size_t)ti * N + w;
            code[g] = random_read(rng, L, 40);
            if (rng() % 10) { label[g] = (uint32_t)g; free_pf.push_back(g); }
        }
        std::shuffle(free_pf.begin(), free_pf.end(), rng);
        // the families: the sizes every case has, then small ones while the wells last (a third of them is left single)
        std::vector<int> sizes = {2, 3, 4, 63, 64, 65, max_family, max_family + 1, 2, 2, 3, 3, 4, 4, 5, 5, 9};
        size_t need = 0; for (int n : sizes) need += n;
        while (need + 6 < free_pf.size() * 2 / 3) { const int n = 2 + (int)(rng() % 5); sizes.push_back(n); need += n; }
        std::vector<std::vector<size_t>> fam;
        size_t used = 0;
        for (int n : sizes) {
            if (used + n > free_pf.size()) break;
            std::vector<size_t> m(free_pf.begin() + used, free_pf.begin() + used + n); used += n;
            std::sort(m.begin(), m.end());
            const std::vector<uint8_t> base = random_read(rng, L, 30);
            const int kind = (int)(rng() % 6);              // 0: equal reads; 1, 2: sparse errors; 3: a tie; 4: three codes; 5: one member far off
            for (size_t j = 0; j < m.size(); j++) {
                std::vector<uint8_t> r = base;
                if (kind != 0 && rng() % 3 == 0) for (int e = 1 + (int)(rng() % 2); e > 0; e--) r[rng() % L] = (uint8_t)(rng() % 5);
                if (kind == 3 && j < m.size() / 2) r[0] = (uint8_t)((base[0] + 1) % 5);              // (even n: exactly half against half)
                if (kind == 4 && j < 2) r[L - 1] = (uint8_t)((base[L - 1] + 1 + j) % 5);
                if (kind == 5 && j == m.size() - 1) for (int c = 0; c < std::min(L, 12); c++) r[c] = (uint8_t)((base[c] + 1) % 5);
                if (kind == 5 && j == 0 && rng() % 2) r[L / 2] = (uint8_t)((base[L / 2] + 2) % 5);      // the root itself errs
                code[m[j]] = r;
                label[m[j]] = (uint32_t)m[0];
            }
            members[m[0]] = (uint32_t)(n - 1);
            fam.push_back(m);
        }
        for (size_t g = 0; g < W; g++) if (!code[g].empty()) {
            for (int k = 0; k < words; k++) rows[g * words + k] = 0;
            for (int c = 0; c < L; c++) rows[g * words + c / 10] |= (uint32_t)code[g][c] << (3 * (c % 10));
        }
        // the definitions, directly
        const size_t n_calls = (size_t)L * 25;
        std::vector<long long> want_l(20, 0), want_t((size_t)T * 4, 0), want_c(n_calls, 0);
        long beyond = 0, voted_roots = 0;
        for (const auto &m : fam) {
            const int n = (int)m.size();
            if (n == 2) { want_l[8]++; continue; }
            if (n > max_family) { want_l[9]++; want_l[10] += n; continue; }
            want_l[0]++; voted_roots++;
            std::vector<int> cons(L, -1);
            int undec = 0;
            for (int c = 0; c < L; c++) {
                int cnt[5] = {0, 0, 0, 0, 0};
                for (size_t g : m) cnt[code[g][c]]++;
                for (int a = 0; a < 5; a++) if (2 * cnt[a] > n) cons[c] = a;
                undec += cons[c] < 0;
            }
            long prof = 0;
            for (size_t g : m) {
                int d = 0, wn = 0;
                for (int c = 0; c < L; c++) if (cons[c] >= 0 && code[g][c] != cons[c]) { d++; wn += cons[c] == 4 || code[g][c] == 4; }
                long long *t = &want_t[(g / (size_t)N) * 4];
                t[0]++; want_l[11 + std::min(d, 8)]++;
                if (g == m[0] && d >= 1) want_l[7]++;
                if (d > max_d) continue;
                prof++; t[1]++; t[2] += d; t[3] += wn;
                for (int c = 0; c < L; c++) if (cons[c] >= 0) { want_c[(size_t)c * 25 + cons[c] * 5 + code[g][c]]++; beyond += c >= kLcWindow && code[g][c] != cons[c]; }
            }
            want_l[5] += undec; want_l[6] += undec * prof;
        }
        for (int t = 0; t < T; t++) for (int f = 0; f < 4; f++) want_l[1 + f] += want_t[(size_t)t * 4 + f];
        // the scratch: cleared as far as the host call clears it, a pattern beyond
        const LcLayout lay = lc_layout_of(T, N, L);
        Buf<uint8_t> sc(lay.bytes);
        const unsigned gx = (unsigned)((N + kLaneRun - 1) / kLaneRun), groups = lc_vote_groups(W);
        long points = 0;
        for (int s = 0; s < kSchedules; s++) {
            sc.fill(s % 2 ? 0x5A : 0xA5);
            memset(sc.p, 0, lay.cleared);
            memcpy(sc.p + lay.tidx, tiles, sizeof(tiles));
            A = Args{(const int *)(sc.p + lay.tidx), N, label.data(), members.data(), rows.data(), words, L, max_d, max_family, (uint32_t)W, (int)groups,
                     (unsigned long long *)(sc.p + lay.cursor), (unsigned long long *)(sc.p + lay.cnt_t), (unsigned long long *)(sc.p + lay.cnt_l),
                     (unsigned long long *)(sc.p + lay.calls), (uint32_t *)(sc.p + lay.slot), (uint32_t *)(sc.p + lay.region)};
            const bool permute = set_schedule(s, (unsigned)trial);
            run_grid(gx, 2, reserve, permute);
            run_grid(gx, 2, scatter, permute);
            // the list and the table: permutations, whatever the schedule
            if ((long)(*A.cursor >> 32) != voted_roots) return fail_("families in the cursor", trial, s, 0, (long)(*A.cursor >> 32), voted_roots);
            std::vector<uint32_t> table(A.region + W - voted_roots, A.region + W), roots;
            for (const auto &m : fam) {
                const int n = (int)m.size();
                if (n < 3 || n > max_family) continue;
                roots.push_back((uint32_t)m[0]);
                const uint32_t start = A.slot[m[0]];
                if ((size_t)start + n - 1 > W - voted_roots) return fail_("a range ends in the table, family", trial, s, (long)m[0], start, 0);
                std::vector<uint32_t> got(A.region + start, A.region + start + n - 1), copies(m.begin() + 1, m.end());
                std::sort(got.begin(), got.end());
                if (got != copies) return fail_("the range is no permutation of the copies of family", trial, s, (long)m[0], got[0], copies[0]);
            }
            std::sort(table.begin(), table.end()); std::sort(roots.begin(), roots.end());
            if (table != roots) return fail_("the table is no permutation of the voted roots", trial, s, 0, (long)table.size(), (long)roots.size());
            run_grid(groups, 1, vote, permute);
            points += emu_counts.points;
            unsigned long long c[kLcLaneCnt];
            std::vector<long long> got_l(20, 0);
            for (int t = 0; t < T; t++) for (int f = 0; f < 4; f++) {
                unsigned long long v = 0; for (int r = 0; r < kSpread; r++) v += A.cnt_t[((size_t)t * kSpread + r) * 4 + f];
                if ((long long)v != want_t[(size_t)t * 4 + f]) return fail_("tile counter", trial, s, t * 4 + f, (long)v, (long)want_t[(size_t)t * 4 + f]);
                got_l[1 + f] += (long long)v;
            }
            for (int f = 0; f < kLcLaneCnt; f++) { c[f] = 0; for (int r = 0; r < kSpread; r++) c[f] += A.cnt_l[(size_t)r * kLcLaneCnt + f]; }
            got_l[0] = (long long)c[kLcFamilies]; got_l[5] = (long long)c[kLcUndecided]; got_l[6] = (long long)c[kLcUndecidedCalls]; got_l[7] = (long long)c[kLcFirstOff];
            got_l[8] = (long long)c[kLcPairs]; got_l[9] = (long long)c[kLcLarge]; got_l[10] = (long long)c[kLcLargeWells];
            for (int b = 0; b < kLcBins; b++) got_l[11 + b] = (long long)c[kLcDist + b];
            for (int f = 0; f < 20; f++) if (got_l[f] != want_l[f]) return fail_("lane row column", trial, s, f, (long)got_l[f], (long)want_l[f]);
            for (size_t e = 0; e < n_calls; e++) if ((long long)A.calls[e] != want_c[e]) return fail_("calls entry", trial, s, (long)e, (long)A.calls[e], (long)want_c[e]);
        }
        printf("case %d ok: L %d words %d N %ld max_d %d max_family %d schedules %d families %lld wells %lld profiled %lld mismatches %lld "
               "with_n %lld undecided %lld first_off %lld pairs %lld large %lld dist8 %lld beyond %ld points %ld\n",
               trial, L, words, (long)N, max_d, max_family, kSchedules, want_l[0], want_l[1], want_l[2], want_l[3], want_l[4], want_l[5], want_l[7],
               want_l[8], want_l[9], want_l[19], beyond, points);
    }
    return 0;
}
