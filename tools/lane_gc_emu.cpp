// lane_gc_emu.cpp - k_lgc_tally (csrc/lane_gc.inc) run on the CPU: the kernel's source is compiled as it stands, the
// 256 lanes of a workgroup are fibers (tools/wave_emu.h) that meet at every barrier, ballot and shuffle, and LDS is the
// kernel's static storage.  Tiles of less than a run and of a run and a bit; rows of 1, 3, 4, 6, 16 and 103 words (9 to
// 1024 cycles: g beyond the LDS window among them); a rows' base that lies 0 to 3 words past a 16-byte boundary, so
// that the pieces of the contiguous loading begin before, at and after a row's first word; random reads with planted
// groups whose copies carry their own reads, equal reads (one root, every well of a wave on one bin) and pairs only;
// max_n of 0, 1 and L: the tile counters and the histogram are compared with the definitions of
// include/welldup_lanegc.h computed directly.  Prints MISMATCH and exits 1 on a difference.
// tests/test_lanegc_emu.py builds and runs it; no GPU is involved, and nothing here says anything about time.
//
//   g++ -O1 -g -std=c++17 -fsanitize=undefined -Iinclude tools/lane_gc_emu.cpp -o lane_gc_emu
#include "wave_emu.h"
constexpr uint32_t kLmLow = 0x09249249u;            // (lane_mismatch.inc's: the lowest bit of each of a word's ten codes)
#define WD_LANE_GC_EMU
#include "../well_duplicates_amd/csrc/lane_gc.inc"

struct Args { const int *tile_idx; int64_t N; const uint32_t *label, *members, *rows; int words, L, max_n; unsigned long long *cnt_t, *hist; };
static Args A;
static void entry() { k_lgc_tally(A.tile_idx, A.N, A.label, A.members, A.rows, A.words, A.L, A.max_n, A.cnt_t, A.hist); }
int main() {
    srand(5);
    const int Ls[] = {9, 25, 40, 51, 151, 1024};            // rows of 1, 3, 4, 6, 16 and 103 words
    for (int trial = 0; trial < 18; trial++) {
        const int i = trial % 6, round = trial / 6;         // every L with every max_n, every mode and both N
        const int L = Ls[i], words = (L + 9) / 10, T = 3, mode = (i + 2 * round) % 3, mis = (i + round) % 4;
        const int max_n = (i + round) % 3 == 0 ? 0 : (i + round) % 3 == 1 ? 1 : L;
        const int64_t N = (i + round) % 2 ? 9000 : 700;     // two runs per tile, the second partial; or a partial one
        int tiles[2] = {2, 0};                              // tile index 1 never added
        const size_t W = (size_t)N * T;
        std::vector<uint32_t> store(W * words + 8, 0xFFFFFFFFu), label(W, kInvalid), members(W, 0);
        uint32_t *rows = store.data();
        while ((int)(((uintptr_t)rows >> 2) & 3) != mis) rows++;        // the base, `mis` words past a 16-byte boundary
        std::vector<std::vector<uint8_t>> code(W);
        // mode 0: random reads, planted groups of 2 to 40 wells with reads of their own; 1: equal reads; 2: pairs only
        std::vector<uint8_t> one(L); for (int c = 0; c < L; c++) one[c] = rand() % 4;
        for (int ti : tiles) for (int64_t w = 0; w < N; w++) {
            size_t g = (size_t)ti * N + w; code[g].resize(L);
            const int kind = rand() % 16;                   // mostly random codes; some reads all G, all N, all A, one N
            for (int c = 0; c < L; c++) code[g][c] = kind == 0 ? 2 : kind == 1 ? 4 : kind == 2 ? 0 : rand() % 50 ? rand() % 4 : 4;
            if (kind == 3) { for (int c = 0; c < L; c++) if (code[g][c] == 4) code[g][c] = 1; code[g][rand() % L] = 4; }
            if (mode == 1) code[g] = one;
            if (rand() % 10) label[g] = (uint32_t)g;        // PF, its own root for now
        }
        if (mode == 0) for (int grp = 0; grp < 60; grp++) {
            size_t r = (size_t)tiles[rand() % 2] * N + rand() % N; if (label[r] != r || members[r]) continue;
            int want = 1 + rand() % 39;
            for (int i = 0; i < want; i++) { size_t g = (size_t)tiles[rand() % 2] * N + rand() % N;
                if (g <= r || label[g] != g || members[g]) continue; label[g] = (uint32_t)r; members[r]++; if (rand() % 2) code[g] = code[r]; }
        } else {
            size_t root = W;
            for (size_t g = 0; g < W; g++) if (label[g] != kInvalid) {
                if (mode == 1) { if (root == W) root = g; else { label[g] = (uint32_t)root; members[root]++; } }
                else if (root == W) root = g; else { label[g] = (uint32_t)root; members[root]++; code[g] = code[root]; root = W; }
            }
        }
        for (size_t g = 0; g < W; g++) if (!code[g].empty()) { for (int k = 0; k < words; k++) rows[g * words + k] = 0;
            for (int c = 0; c < L; c++) rows[g * words + c / 10] |= (uint32_t)code[g][c] << (3 * (c % 10)); }
        std::vector<unsigned long long> cnt_t((size_t)T * kSpread * kLgcTileCnt, 0), hist((size_t)(L + 1) * kSpread * kLgcCols, 0);
        A = Args{tiles, N, label.data(), members.data(), rows, words, L, max_n, cnt_t.data(), hist.data()};
        for (unsigned by = 0; by < 2; by++) for (unsigned bx = 0; bx < (unsigned)((N + kLaneRun - 1) / kLaneRun); bx++) run_block(bx, by, entry);
        // the definitions, directly (the group sizes counted from the labels, not taken from members)
        std::vector<long long> size(W, 0), wt((size_t)T * kLgcTileCnt, 0), wh((size_t)(L + 1) * 4, 0);
        for (size_t g = 0; g < W; g++) if (label[g] != kInvalid) size[label[g]]++;
        long long counted = 0, skipped = 0, top = 0;
        for (int ti : tiles) for (int64_t w = 0; w < N; w++) {
            size_t g = (size_t)ti * N + w; if (label[g] == kInvalid) continue;
            int gc = 0, nn = 0; for (int c = 0; c < L; c++) { gc += code[g][c] == 1 || code[g][c] == 2; nn += code[g][c] == 4; }
            const int pop = label[g] != g ? 2 : size[g] > 1 ? 1 : 0;
            long long *t = &wt[(size_t)ti * kLgcTileCnt];
            t[0]++; t[1 + pop]++;
            if (nn > max_n) { t[4 + pop]++; if (pop == 1) t[7] += size[g]; skipped++; continue; }
            counted++; top += gc >= kLgcWindow;
            wh[(size_t)gc * 4 + pop]++; if (pop == 1) wh[(size_t)gc * 4 + 3] += size[g];
            t[8] += gc; if (pop == 2) t[9] += gc;
        }
        for (int t = 0; t < T; t++) for (int f = 0; f < kLgcTileCnt; f++) { unsigned long long s = 0; for (int r = 0; r < kSpread; r++) s += cnt_t[((size_t)t * kSpread + r) * kLgcTileCnt + f];
            if ((long long)s != wt[(size_t)t * kLgcTileCnt + f]) { printf("MISMATCH trial %d tile %d col %d: %llu want %lld\n", trial, t, f, s, wt[(size_t)t * kLgcTileCnt + f]); return 1; } }
        for (int g = 0; g <= L; g++) for (int f = 0; f < 4; f++) { unsigned long long s = 0; for (int r = 0; r < kSpread; r++) s += hist[((size_t)g * kSpread + r) * 4 + f];
            if ((long long)s != wh[(size_t)g * 4 + f]) { printf("MISMATCH trial %d g %d col %d: %llu want %lld\n", trial, g, f, s, wh[(size_t)g * 4 + f]); return 1; } }
        printf("trial %d ok: L %d words %d N %ld max_n %d mode %d mis %d counted %lld skipped %lld beyond %lld\n", trial, L, words, (long)N, max_n, mode, mis,
               counted, skipped, top);
    }
    return 0;
}
