// lane_mismatch_emu.cpp - k_lm_tally (csrc/lane_mismatch.inc) run on the CPU: the kernel's source is compiled as it
// stands, the 256 lanes of a workgroup are fibers (ucontext) that a round-robin scheduler switches at the collectives -
// __syncthreads is a rendezvous of the workgroup, __ballot and __shfl of a wave - and LDS is the kernel's static
// storage.  Lanes of sparse pairs, of copies that all differ from one root at one cycle and of equal reads, tiles of
// less than a run and of a run and a bit, reads inside the LDS window and beyond it, every max_d: the counters and
// Sub are compared with the definitions of include/welldup_lanemismatch.h computed directly.  Prints MISMATCH and
// exits 1 on a difference.  tests/test_lanemismatch_emu.py builds and runs it; no GPU is involved, and nothing here
// says anything about time.
//
//   g++ -O1 -g -std=c++17 -fsanitize=undefined -Iinclude tools/lane_mismatch_emu.cpp -o lane_mismatch_emu
#include "wave_emu.h"
#define WD_LANE_MISMATCH_EMU
#include "../well_duplicates_amd/csrc/lane_mismatch.inc"

struct Args { const int *tile_idx; int64_t N; const uint32_t *label, *rows; int words, L, max_d; unsigned long long *cnt_t, *cnt_l, *sub; };
static Args A;
static void entry() { k_lm_tally(A.tile_idx, A.N, A.label, A.rows, A.words, A.L, A.max_d, A.cnt_t, A.cnt_l, A.sub); }
int main() {
    srand(3);
    for (int trial = 0; trial < 12; trial++) {
        const int Ls[] = {37, 83, 151, 165, 400, 40};
        int L = Ls[trial % 6], words = (L + 9) / 10, T = 3, max_d = trial % 8;
        int64_t N = trial % 2 ? 9000 : 700;                 // two runs per tile, the second partial; or a partial one
        int tiles[2] = {2, 0};                              // tile index 1 never added
        size_t W = (size_t)N * T;
        std::vector<uint32_t> rows(W * words, 0), label(W, kInvalid);
        std::vector<std::vector<int>> code(W);
        int mode = trial % 3;                               // 0: sparse pairs, 1: every well a copy of one root at one cycle, 2: equal reads
        for (int ti : tiles) for (int64_t w = 0; w < N; w++) {
            size_t g = (size_t)ti * N + w; code[g].resize(L);
            for (int c = 0; c < L; c++) code[g][c] = rand() % 5;
            if (rand() % 10) label[g] = (uint32_t)g;        // PF, its own root for now
        }
        size_t root0 = (size_t)0 * N + 3; label[root0] = (uint32_t)root0;
        for (int ti : tiles) for (int64_t w = 0; w < N; w++) {
            size_t g = (size_t)ti * N + w; if (label[g] == kInvalid || g == root0) continue;
            size_t r = root0; int nd = 0;
            if (mode == 0) { if (rand() % 20) continue; r = (size_t)0 * N + rand() % 3000 % N; if (r >= g || label[r] != r) continue; nd = rand() % 11; }
            else if (mode == 1) nd = -1;
            code[g] = code[r]; label[g] = (uint32_t)r;
            if (nd == -1) code[g][L / 2] = (code[r][L / 2] + 1) % 5;
            for (int i = 0; i < nd; i++) { int c = rand() % 3 ? rand() % L : (rand() % 2 ? L - 1 : 0); code[g][c] = rand() % 5; }
        }
        // (a root is its own root: a well whose root has meanwhile become a member goes back to being single)
        for (size_t g = 0; g < W; g++) if (label[g] != kInvalid && label[g] != g && label[label[g]] != label[g]) { label[g] = (uint32_t)g; }
        for (size_t g = 0; g < W; g++) if (!code[g].empty()) for (int c = 0; c < L; c++) rows[g * words + c / 10] |= (uint32_t)code[g][c] << (3 * (c % 10));
        std::vector<unsigned long long> cnt_t((size_t)T * kSpread * kLmTileCnt, 0), cnt_l(kSpread * kLmLaneCnt, 0), sub((size_t)L * 25, 0);
        A = Args{tiles, N, label.data(), rows.data(), words, L, max_d, cnt_t.data(), cnt_l.data(), sub.data()};
        for (unsigned by = 0; by < 2; by++) for (unsigned bx = 0; bx < (unsigned)((N + kLaneRun - 1) / kLaneRun); bx++) run_block(bx, by, entry);
        // the definitions, directly
        std::vector<long long> wt((size_t)T * 4, 0), wd(9, 0), wsub((size_t)L * 25, 0);
        for (int ti : tiles) for (int64_t w = 0; w < N; w++) {
            size_t g = (size_t)ti * N + w; if (label[g] == kInvalid || label[g] == g) continue;
            size_t r = label[g]; int d = 0; for (int c = 0; c < L; c++) d += code[r][c] != code[g][c];
            wd[std::min(d, 8)]++; wt[ti * 4]++;
            if (d <= max_d) { wt[ti * 4 + 1]++; wt[ti * 4 + 2] += d;
                for (int c = 0; c < L; c++) if (code[r][c] != code[g][c]) { wsub[c * 25 + code[r][c] * 5 + code[g][c]]++; wt[ti * 4 + 3] += code[r][c] == 4 || code[g][c] == 4; } }
        }
        long long pairs = 0;
        for (int t = 0; t < T; t++) for (int f = 0; f < 4; f++) { unsigned long long s = 0; for (int r = 0; r < kSpread; r++) s += cnt_t[((size_t)t * kSpread + r) * 4 + f];
            if ((long long)s != wt[t * 4 + f]) { printf("MISMATCH trial %d tile %d col %d: %llu want %lld\n", trial, t, f, s, wt[t * 4 + f]); return 1; } if (f == 0) pairs += s; }
        for (int b = 0; b < 9; b++) { unsigned long long s = 0; for (int r = 0; r < kSpread; r++) s += cnt_l[r * kLmLaneCnt + b];
            if ((long long)s != wd[b]) { printf("MISMATCH trial %d dist %d: %llu want %lld\n", trial, b, s, wd[b]); return 1; } }
        for (size_t e = 0; e < sub.size(); e++) if ((long long)sub[e] != wsub[e]) { printf("MISMATCH trial %d sub %zu: %llu want %lld\n", trial, e, sub[e], wsub[e]); return 1; }
        printf("trial %d ok: L %d N %ld max_d %d mode %d pairs %lld dist", trial, L, (long)N, max_d, mode, pairs); for (int b = 0; b < 9; b++) printf(" %lld", wd[b]); printf("\n");
    }
    return 0;
}
