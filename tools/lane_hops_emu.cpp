// lane_hops_emu.cpp - k_lh_tally (csrc/lane_hops.inc) run on the CPU: the kernel's source is compiled as it stands,
// the 256 lanes of a workgroup are fibers (tools/wave_emu.h) that meet at every __syncthreads, __ballot and __shfl, and
// LDS is the kernel's static storage.  Pooled lanes with index errors and swaps planted on the copies, a lane of one
// key, a lane whose keys are all unlisted and a lane with more distinct (root, copy) cells in a run than the LDS table
// has entries; tiles of less than a run and of a run and a bit; index reads of 8, 16 and 20 cycles split inside the
// first word, at the word boundary, inside the second word and not at all; every max_e and M = 0, 3 and 1024: the
// counters and the matrix are compared with the definitions of include/welldup_lanehops.h computed directly.  Every
// trial runs under the eleven schedules of emu_reads.h - a lane may hand over at every atomic: never, lanes in reverse,
// always, with probability 1/3 under eight seeds; workgroups permuted in all but the first - and each must give the
// definitions: the claims of the LDS table (a plain atomicCAS) then meet on free entries, and those that lose are
// counted (lost_lds, over the schedules at 1/3).  Prints MISMATCH and exits 1 on a difference.
// tests/test_lanehops_emu.py builds and runs it, and once more with -DWAVE_EMU_TORN_CAS=3 (the LDS claim torn), which
// must end in MISMATCH; no GPU is involved, and nothing here says anything about time.
//
//   g++ -O1 -g -std=c++17 -fsanitize=undefined -Iinclude tools/lane_hops_emu.cpp -o lane_hops_emu
#include "wave_emu.h"
#include "emu_reads.h"
#include <set>
#define WD_LANE_MISMATCH_EMU                        // lm_fold is lane_mismatch.inc's
#include "../well_duplicates_amd/csrc/lane_mismatch.inc"
#define WD_LANE_HOPS_EMU
#include "../well_duplicates_amd/csrc/lane_hops.inc"

struct Args { const int *tile_idx; int64_t N; const uint32_t *label; const uint2 *key; unsigned long long m1, m2; int max_e, M;
              const unsigned long long *listed; const uint16_t *rank; unsigned long long *cnt_t, *cnt_l, *matrix; };
static Args A;
static void entry() { k_lh_tally(A.tile_idx, A.N, A.label, A.key, A.m1, A.m2, A.max_e, A.M, A.listed, A.rank, A.cnt_t, A.cnt_l, A.matrix); }
typedef std::vector<int> Codes;
static unsigned long long key_of(const Codes &c) { unsigned long long k = 0; for (size_t i = 0; i < c.size(); i++) k |= (unsigned long long)c[i] << (32 * (i / 10) + 3 * (i % 10)); return k; }
struct Trial { int I, split, E; int64_t N; int mode, M; };   // mode 0: a pool, sparse copies; 1: one key; 2: every key unlisted; 3: many cells
int main() {
    srand(5);
    const Trial trials[12] = {{8, 8, 0, 700, 0, 3},     {16, 8, 1, 9000, 0, 1024}, {16, 16, 3, 700, 0, 0},  {20, 10, 0, 9000, 3, 1024},
                              {20, 13, 1, 700, 1, 3},   {8, 8, 3, 9000, 1, 0},     {16, 8, 0, 700, 2, 3},   {16, 16, 1, 9000, 2, 1024},
                              {20, 10, 3, 700, 0, 1024}, {20, 13, 0, 9000, 0, 3},  {16, 8, 3, 9000, 3, 1024}, {20, 13, 1, 9000, 0, 0}};
    for (int trial = 0; trial < 12; trial++) {
        const Trial &t = trials[trial];
        const int I = t.I, split = t.split, E = t.E, M = t.M, mode = t.mode, T = 3;
        const int64_t N = t.N;
        int tiles[2] = {2, 0};                              // tile index 1 never added
        const size_t W = (size_t)N * T;
        const int top = mode == 2 ? 4 : 5;                  // mode 2: no N in the lane; every listed key begins with one
        // the libraries: distinct keys; the listing is the first M of them (mode 2: M keys of their own)
        const int n_lib = M == 1024 ? 1100 : 12;
        std::vector<Codes> lib; std::set<unsigned long long> have;
        while ((int)lib.size() < n_lib) { Codes c(I); for (int i = 0; i < I; i++) c[i] = rand() % 40 ? rand() % 4 : rand() % top; if (have.insert(key_of(c)).second) lib.push_back(c); }
        std::vector<unsigned long long> listed;
        if (mode == 2) { std::set<unsigned long long> own; while ((int)listed.size() < M) { Codes c(I); c[0] = 4; for (int i = 1; i < I; i++) c[i] = rand() % 4; if (own.insert(key_of(c)).second) listed.push_back(key_of(c)); } }
        else for (int i = 0; i < M && i < n_lib; i++) listed.push_back(key_of(lib[(size_t)(mode == 0 ? (i * 7) % n_lib : i)]));
        if (mode == 0 && M > 0) { std::set<unsigned long long> u(listed.begin(), listed.end()); if ((int)u.size() != M) { listed.clear(); for (int i = 0; i < M; i++) listed.push_back(key_of(lib[(size_t)i])); } }
        if ((int)listed.size() != M) { printf("MISMATCH trial %d: %zu keys to list, not %d\n", trial, listed.size(), M); return 1; }
        std::vector<Codes> code(W); std::vector<uint32_t> label(W, kInvalid);
        for (int ti : tiles) for (int64_t w = 0; w < N; w++) {
            size_t g = (size_t)ti * N + w; code[g] = lib[(size_t)(mode == 1 ? 0 : rand() % n_lib)];
            if (mode != 1 && rand() % 10 == 0) code[g][rand() % I] = rand() % top;           // an index read error
            if (rand() % 10) label[g] = (uint32_t)g;        // PF, its own root for now
        }
        size_t root0 = (size_t)0 * N + 3; label[root0] = (uint32_t)root0;
        for (int ti : tiles) for (int64_t w = 0; w < N; w++) {
            size_t g = (size_t)ti * N + w; if (label[g] == kInvalid || g == root0) continue;
            size_t r = root0;
            if (mode == 0 || mode == 2) {                   // a copy of a well before it, on tile 0 or on its own tile
                if (rand() % 4) continue;
                r = (rand() % 2 ? (size_t)0 : (size_t)ti * N) + rand() % 3000 % N; if (r >= g || label[r] != r) continue;
                code[g] = code[r];
                const Codes &o = lib[(size_t)(rand() % n_lib)];
                switch (rand() % 8) {
                case 0: code[g][rand() % I] = rand() % top; break;                                          // a read error
                case 1: for (int c = 0; c < split; c++) code[g][c] = o[c]; break;                           // part 1 another library's
                case 2: for (int c = split; c < I; c++) code[g][c] = o[c]; break;                           // part 2
                case 3: code[g] = o; break;                                                                 // both
                case 4: for (int i = 0; i <= E; i++) code[g][rand() % 2 ? rand() % I : (rand() % 2 ? I - 1 : 0)] = rand() % top; break;
                case 5: code[g][rand() % 2 ? split - 1 : std::min(split, I - 1)] = rand() % top; break;     // at the edge of the parts
                default: break;
                }
            } else if (mode == 3) {                         // every other well a copy of one of a few roots, whatever its key
                if (w % 64 == 0 && ti == 0) continue;
                r = (size_t)(rand() % (int)((N + 63) / 64)) * 64; if (label[r] != r) continue;
            }
            label[g] = (uint32_t)r;
        }
        // (a root is its own root: a well whose root has meanwhile become a member goes back to being single)
        for (size_t g = 0; g < W; g++) if (label[g] != kInvalid && label[g] != g && label[label[g]] != label[g]) label[g] = (uint32_t)g;
        std::vector<uint2> key(W, uint2{0, 0});
        for (size_t g = 0; g < W; g++) if (!code[g].empty()) { unsigned long long k = key_of(code[g]); key[g] = uint2{(uint32_t)k, (uint32_t)(k >> 32)}; }
        // the listing as the host half hands it over: sorted, each key with its place in the caller's list
        std::vector<std::pair<unsigned long long, uint16_t>> order; std::map<unsigned long long, int> rank_of;
        for (int i = 0; i < M; i++) { order.push_back({listed[(size_t)i], (uint16_t)i}); rank_of[listed[(size_t)i]] = i; }
        std::sort(order.begin(), order.end());
        std::vector<unsigned long long> s_keys(M + 1, 0); std::vector<uint16_t> s_rank(M + 1, 0);
        for (int i = 0; i < M; i++) { s_keys[(size_t)i] = order[(size_t)i].first; s_rank[(size_t)i] = order[(size_t)i].second; }
        const size_t cells = (size_t)(M + 1) * (M + 1);
        std::vector<unsigned long long> cnt_t((size_t)T * kSpread * kLhTileCnt, 0), cnt_l(kSpread * kLhLaneCnt, 0), matrix(cells, 0);
        A = Args{tiles, N, label.data(), key.data(), lh_mask(0, split), lh_mask(split, I), E, M, s_keys.data(), s_rank.data(), cnt_t.data(), cnt_l.data(), matrix.data()};
        // the definitions, directly
        std::vector<long long> wt((size_t)T * 4, 0), wst(9, 0), wm(cells, 0); size_t most_cells = 0;
        for (int ti : tiles) { std::set<size_t> in_run;
            for (int64_t w = 0; w < N; w++) {
                if (w % kLaneRun == 0) in_run.clear();
                size_t g = (size_t)ti * N + w; if (label[g] == kInvalid || label[g] == g) continue;
                size_t r = label[g]; int d1 = 0, d2 = 0;
                for (int c = 0; c < I; c++) (c < split ? d1 : d2) += code[r][c] != code[g][c];
                int s1 = d1 == 0 ? 0 : d1 <= E ? 1 : 2, s2 = d2 == 0 ? 0 : d2 <= E ? 1 : 2;
                wst[3 * s1 + s2]++; wt[ti * 4]++; wt[ti * 4 + 1] += r / (size_t)N == (size_t)ti;
                wt[ti * 4 + 2] += (s1 == 2) != (s2 == 2); wt[ti * 4 + 3] += s1 == 2 && s2 == 2;
                auto a = rank_of.find(key_of(code[r])), b = rank_of.find(key_of(code[g]));
                size_t cell = (size_t)(a == rank_of.end() ? M : a->second) * (M + 1) + (b == rank_of.end() ? M : b->second);
                wm[cell]++; in_run.insert(cell); most_cells = std::max(most_cells, in_run.size());
            } }
        long long pairs = 0, points = 0, never_lost = 0, lost_lds = 0;
        for (int sch = 0; sch < kSchedules; sch++) {
            const bool permute = set_schedule(sch, 1000u * trial + 17);      // (the seed: one under which every trial loses a claim at 1/3)
            std::fill(cnt_t.begin(), cnt_t.end(), 0ull); std::fill(cnt_l.begin(), cnt_l.end(), 0ull); std::fill(matrix.begin(), matrix.end(), 0ull);      // the host's memset of the scratch
            run_grid((unsigned)((N + kLaneRun - 1) / kLaneRun), 2, entry, permute);
            points += emu_counts.points;
            if (sch == 0) never_lost = emu_counts.lost[kEmuTable] + emu_counts.lost[kEmuUnion] + emu_counts.lost[kEmuLds];
            if (sch >= 3) lost_lds += emu_counts.lost[kEmuLds];
            pairs = 0;
            for (int tt = 0; tt < T; tt++) for (int f = 0; f < 4; f++) { unsigned long long s = 0; for (int r = 0; r < kSpread; r++) s += cnt_t[((size_t)tt * kSpread + r) * 4 + f];
                if ((long long)s != wt[tt * 4 + f]) { printf("MISMATCH trial %d tile %d col %d: %llu want %lld\n", trial, tt, f, s, wt[tt * 4 + f]); printf("  (schedule %d %s)\n", sch, schedule_name(sch)); return 1; } if (f == 0) pairs += s; }
            for (int b = 0; b < 9; b++) { unsigned long long s = 0; for (int r = 0; r < kSpread; r++) s += cnt_l[r * kLhLaneCnt + b];
                if ((long long)s != wst[b]) { printf("MISMATCH trial %d state %d: %llu want %lld\n", trial, b, s, wst[b]); printf("  (schedule %d %s)\n", sch, schedule_name(sch)); return 1; } }
            for (size_t e = 0; e < cells; e++) if ((long long)matrix[e] != wm[e]) { printf("MISMATCH trial %d cell %zu: %llu want %lld\n", trial, e, matrix[e], wm[e]); printf("  (schedule %d %s)\n", sch, schedule_name(sch)); return 1; }
            if (mode == 1 && (wm[0] != pairs || wst[0] != pairs)) { printf("MISMATCH trial %d: one key, but %lld of %lld pairs in cell 0\n", trial, wm[0], pairs); printf("  (schedule %d %s)\n", sch, schedule_name(sch)); return 1; }
            if (mode == 2 && wm[cells - 1] != pairs) { printf("MISMATCH trial %d: unlisted keys, but %lld of %lld pairs in Other\n", trial, wm[cells - 1], pairs); printf("  (schedule %d %s)\n", sch, schedule_name(sch)); return 1; }
        }
        printf("trial %d ok: I %d split %d E %d N %ld M %d mode %d pairs %lld cells %zu slots %d state", trial, I, split, E, (long)N, M, mode, pairs, most_cells, kLhSlots);
        for (int b = 0; b < 9; b++) printf(" %lld", wst[b]);
        printf(" schedules %d points %lld never_lost %lld lost_lds %lld\n", kSchedules, points, never_lost, lost_lds);
    }
    return 0;
}
