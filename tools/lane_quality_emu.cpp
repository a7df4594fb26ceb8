// lane_quality_emu.cpp - k_lq_tally (csrc/lane_quality.inc) run on the CPU: the kernel's source is compiled as it
// stands on tools/wave_emu.h (a fiber per lane, switched at the collectives; LDS is the kernel's static storage).
// Lanes of sparse pairs, of equal reads with one quality value, of equal reads with random qualities, and a single
// pair whose cycles visit the 64 cells in turn (at L = 64 every cell holds one observation); L = 37 and 151 (16-byte
// pieces, the first with a partial last word), 40 (a full last word), 83 (nine words) and 1024 (103 words); tiles of
// less than a run and of a run and a bit; every max_d.  The counters, Obs and Mis are compared with the definitions
// of include/welldup_lanequality.h computed directly.  Prints MISMATCH and exits 1 on a difference.
// tests/test_lanequality_emu.py builds and runs it; no GPU is involved, and nothing here says anything about time.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -Iinclude tools/lane_quality_emu.cpp -o lane_quality_emu
#include "wave_emu.h"
#define WD_LANE_MISMATCH_EMU
#define WD_LANE_QUALITY_EMU
#include "../well_duplicates_amd/csrc/lane_mismatch.inc"
#include "../well_duplicates_amd/csrc/lane_quality.inc"

struct Args { const int *tile_idx; int64_t N; const uint32_t *label, *rows, *qrows; int words, L, max_d; unsigned long long *cnt_t, *cells; };
static Args A;
static void entry() { k_lq_tally(A.tile_idx, A.N, A.label, A.rows, A.qrows, A.words, A.L, A.max_d, A.cnt_t, A.cells); }
struct Trial { int mode, L; int64_t N; int max_d; };   // mode 0: sparse pairs, 1: equal reads one quality, 2: equal reads random qualities, 3: one pair, every cell
int main() {
    srand(5);
    const Trial trials[] = {{0, 37, 700, 3}, {0, 83, 9000, 7}, {0, 1024, 700, 5}, {0, 151, 9000, 6}, {0, 40, 700, 1},
                            {1, 37, 9000, 0}, {1, 83, 700, 2}, {1, 1024, 700, 0}, {2, 37, 700, 1}, {2, 83, 9000, 0},
                            {2, 1024, 700, 4}, {3, 64, 700, 7}, {3, 37, 700, 7}, {3, 1024, 700, 7}};
    int trial = 0;
    for (const Trial &tr : trials) {
        const int L = tr.L, words = (L + 9) / 10, T = 3, max_d = tr.max_d, mode = tr.mode;
        const int64_t N = tr.N;
        int tiles[2] = {2, 0};                              // tile index 1 never added
        size_t W = (size_t)N * T;
        std::vector<uint32_t> rows(W * words, 0), qrows(W * words, 0), label(W, kInvalid);
        std::vector<std::vector<uint8_t>> code(W), qbin(W);
        for (int ti : tiles) for (int64_t w = 0; w < N; w++) {
            size_t g = (size_t)ti * N + w; code[g].resize(L); qbin[g].resize(L);
            for (int c = 0; c < L; c++) { code[g][c] = rand() % 5; qbin[g][c] = mode == 1 ? 5 : rand() % 3 ? 7 : rand() % 8; }
            if (rand() % 10) label[g] = (uint32_t)g;        // PF, its own root for now
        }
        size_t root0 = (size_t)0 * N + 3; label[root0] = (uint32_t)root0;
        if (mode == 3) {                                    // one pair: cycle c visits cell c % 64, the member differs at every 9th of the first 55
            size_t g = (size_t)2 * N + 77; label[g] = (uint32_t)root0; code[g] = code[root0];
            for (int c = 0; c < L; c++) { qbin[root0][c] = (c % 64) / 8; qbin[g][c] = c % 8; }
            for (int c = 0; c < L && c < 55; c += 9) code[g][c] = (code[root0][c] + 1) % 5;
        } else for (int ti : tiles) for (int64_t w = 0; w < N; w++) {
            size_t g = (size_t)ti * N + w; if (label[g] == kInvalid || g == root0) continue;
            size_t r = root0; int nd = 0;
            if (mode == 0) { if (rand() % 20) continue; r = (size_t)0 * N + rand() % 3000 % N; if (r >= g || label[r] != r) continue; nd = rand() % 11; }
            code[g] = code[r]; label[g] = (uint32_t)r;
            for (int i = 0; i < nd; i++) { int c = rand() % 3 ? rand() % L : (rand() % 2 ? L - 1 : 0); code[g][c] = rand() % 5; }
        }
        // (a root is its own root: a well whose root has meanwhile become a member goes back to being single)
        for (size_t g = 0; g < W; g++) if (label[g] != kInvalid && label[g] != g && label[label[g]] != label[g]) { label[g] = (uint32_t)g; }
        for (size_t g = 0; g < W; g++) if (!code[g].empty()) for (int c = 0; c < L; c++) {
            rows[g * words + c / 10] |= (uint32_t)code[g][c] << (3 * (c % 10)); qrows[g * words + c / 10] |= (uint32_t)qbin[g][c] << (3 * (c % 10)); }
        std::vector<unsigned long long> cnt_t((size_t)T * kSpread * kLqTileCnt, 0), cells((size_t)kSpread * 2 * kLqCells, 0);
        A = Args{tiles, N, label.data(), rows.data(), qrows.data(), words, L, max_d, cnt_t.data(), cells.data()};
        for (unsigned by = 0; by < 2; by++) for (unsigned bx = 0; bx < (unsigned)((N + kLaneRun - 1) / kLaneRun); bx++) run_block(bx, by, entry);
        // the definitions, directly
        std::vector<long long> wt((size_t)T * 4, 0), wobs(64, 0), wmis(64, 0);
        for (int ti : tiles) for (int64_t w = 0; w < N; w++) {
            size_t g = (size_t)ti * N + w; if (label[g] == kInvalid || label[g] == g) continue;
            size_t r = label[g]; int d = 0; for (int c = 0; c < L; c++) d += code[r][c] != code[g][c];
            wt[ti * 4]++;
            if (d <= max_d) { wt[ti * 4 + 1]++; wt[ti * 4 + 2] += L; wt[ti * 4 + 3] += d;
                for (int c = 0; c < L; c++) { int cell = qbin[r][c] * 8 + qbin[g][c]; wobs[cell]++; wmis[cell] += code[r][c] != code[g][c]; } }
        }
        long long pairs = 0, prof = 0, occupied = 0, most = 0;
        for (int t = 0; t < T; t++) for (int f = 0; f < 4; f++) { unsigned long long s = 0; for (int r = 0; r < kSpread; r++) s += cnt_t[((size_t)t * kSpread + r) * 4 + f];
            if ((long long)s != wt[t * 4 + f]) { printf("MISMATCH trial %d tile %d col %d: %llu want %lld\n", trial, t, f, s, wt[t * 4 + f]); return 1; } if (f == 0) pairs += s; if (f == 1) prof += s; }
        for (int e = 0; e < 128; e++) { unsigned long long s = 0; for (int r = 0; r < kSpread; r++) s += cells[(size_t)r * 128 + e];
            long long want = e < 64 ? wobs[e] : wmis[e - 64];
            if ((long long)s != want) { printf("MISMATCH trial %d %s cell %d: %llu want %lld\n", trial, e < 64 ? "obs" : "mis", e % 64, s, want); return 1; }
            if (e < 64) { occupied += s > 0; most = std::max(most, (long long)s); } }
        printf("trial %d ok: L %d N %ld max_d %d mode %d pairs %lld profiled %lld cells %lld most %lld\n", trial, L, (long)N, max_d, mode, pairs, prof, occupied, most);
        trial++;
    }
    return 0;
}
