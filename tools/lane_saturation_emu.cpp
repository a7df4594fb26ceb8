// lane_saturation_emu.cpp - k_ls_min and k_ls_tally (csrc/lane_saturation.inc) run on the CPU: the kernels' source is
// compiled as it stands on the shims of tools/wave_emu.h (a fiber per lane, switched at the collectives).  Lanes of
// sparse pairs, of equal reads (every pair on one root) and of copies that all sit beside their originals, tiles of
// less than a run and of a run and a bit, 1, 20 and 64 steps, radii 0, 2500 and 2^25 and the form without
// coordinates: the head row, NewReads and NewDistinct are compared with the definitions of
// include/welldup_lanesaturation.h computed directly (the step in 64-bit arithmetic, the class minima by a loop over
// the wells).  Prints MISMATCH and exits 1 on a difference.  tests/test_lanesaturation_emu.py builds and runs it; no
// GPU is involved, and nothing here says anything about time.
//
//   g++ -O1 -g -std=c++17 -fsanitize=undefined -Iinclude tools/lane_saturation_emu.cpp -o lane_saturation_emu
#include "wave_emu.h"
#define WD_LANE_SATURATION_EMU
#include "../well_duplicates_amd/csrc/lane_saturation.inc"

struct Args { const int *tile_idx; int64_t N; const uint32_t *label; const int2 *xy; unsigned long long radius2; uint32_t steps, salt; uint32_t *cls; unsigned long long *cnt, *head; };
static Args A;
static void entry_min() { k_ls_min(A.tile_idx, A.N, A.label, A.xy, A.radius2, A.steps, A.salt, A.cls); }
static void entry_tally() { k_ls_tally(A.tile_idx, A.N, A.label, A.xy, A.radius2, A.steps, A.salt, A.cls, A.cnt, A.head); }
static int want_step(uint64_t g, uint64_t seed, uint64_t S) {
    const uint64_t M = 0xFFFFFFFFull;
    uint64_t h = (g + seed * 0x9E3779B9ull) & M;
    h ^= h >> 16; h = h * 0x85EBCA6Bull & M; h ^= h >> 13; h = h * 0xC2B2AE35ull & M; h ^= h >> 16;
    return (int)(h * S >> 32);
}
int main() {
    srand(7);
    const int64_t radii[] = {0, 2500, 1 << 25, -1};         // -1: without coordinates
    const int step_counts[] = {1, 20, 64};
    for (int trial = 0; trial < 72; trial++) {
        const int T = 3, mode = trial / 2 % 3;              // 0: sparse pairs, 1: equal reads, 2: every odd well a copy of the well before it
        const int64_t N = trial % 2 ? 9000 : 700, radius = radii[trial / 6 % 4];  // two runs per tile, the second partial; or a partial one
        const int S = step_counts[trial / 24];
        const uint32_t seed = (uint32_t)trial * 2654435761u + (trial % 5 == 0 ? 0 : 1);
        int tiles[2] = {2, 0};                              // tile index 1 never added
        const size_t W = (size_t)N * T;
        std::vector<uint32_t> label(W, kInvalid);
        std::vector<int2> xy(N);
        for (int64_t w = 0; w < N; w++)                     // most wells in a corner of 3000 x 3000, the rest anywhere
            xy[w] = rand() % 4 ? int2{rand() % 3000, rand() % 3000} : int2{rand() % (1 << 24), rand() % (1 << 24)};
        xy[3] = int2{0, 0};
        xy[N - 1] = int2{(1 << 24) - 1, (1 << 24) - 1};     // (q = 2^49 - 2^26 + 2 from well 3: what 32 bits cannot hold)
        if (mode == 2) for (int64_t w = 1; w < N - 1; w += 2) xy[w] = int2{std::min(xy[w - 1].x + rand() % 20, (1 << 24) - 1), std::min(xy[w - 1].y + rand() % 20, (1 << 24) - 1)};
        for (int ti : tiles) for (int64_t w = 0; w < N; w++) if (rand() % 10 || mode == 2) label[(size_t)ti * N + w] = (uint32_t)((size_t)ti * N + w);
        const size_t root0 = 3; label[root0] = (uint32_t)root0;
        for (int ti : tiles) for (int64_t w = 0; w < N; w++) {
            const size_t g = (size_t)ti * N + w; if (label[g] == kInvalid || g == root0) continue;
            size_t r = root0;
            if (mode == 0) { if (rand() % 6) continue; r = (size_t)(rand() % 2 ? ti : 0) * N + rand() % N; if (r >= g || label[r] != r) continue; }
            if (mode == 2) { if (w % 2 == 0 || w == N - 1) continue; r = g - 1; }
            label[g] = (uint32_t)r;
        }
        // (a root is its own root: a well whose root has meanwhile become a member goes back to being single)
        for (size_t g = 0; g < W; g++) if (label[g] != kInvalid && label[g] != g && label[label[g]] != label[g]) label[g] = (uint32_t)g;
        const unsigned long long radius2 = radius > 0 ? (unsigned long long)radius * (unsigned long long)radius : 0;
        std::vector<uint32_t> cls(W, 0xFFFFFFFFu);
        std::vector<unsigned long long> cnt((size_t)kSpread * 2 * kLsSteps, 0), head((size_t)kSpread * kLsHead, 0);
        A = Args{tiles, N, label.data(), radius2 ? xy.data() : nullptr, radius2, (uint32_t)S, seed * 0x9E3779B9u, cls.data(), cnt.data(), head.data()};
        const unsigned nbx = (unsigned)((N + kLaneRun - 1) / kLaneRun);
        for (unsigned by = 0; by < 2; by++) for (unsigned bx = 0; bx < nbx; bx++) run_block(bx, by, entry_min);
        for (unsigned by = 0; by < 2; by++) for (unsigned bx = 0; bx < nbx; bx++) run_block(bx, by, entry_tally);
        // the definitions, directly
        std::vector<long long> wr(S, 0), wdi(S, 0); long long pf = 0, dropped = 0;
        std::vector<int> cmin(W, 1 << 30);
        std::vector<char> is_dropped(W, 0);
        for (int ti : tiles) for (int64_t w = 0; w < N; w++) {
            const size_t g = (size_t)ti * N + w; if (label[g] == kInvalid) continue;
            pf++;
            const size_t r = label[g];
            if (r != g && radius > 0 && (int)(r / N) == ti) {
                const long long dx = (long long)xy[w].x - xy[r % N].x, dy = (long long)xy[w].y - xy[r % N].y;
                if ((unsigned long long)(dx * dx + dy * dy) < (unsigned long long)radius * (unsigned long long)radius) { is_dropped[g] = 1; dropped++; continue; }
            }
            const int s = want_step(g, seed, S);
            wr[s]++; cmin[r] = std::min(cmin[r], s);
        }
        for (int ti : tiles) for (int64_t w = 0; w < N; w++) { const size_t g = (size_t)ti * N + w; if (label[g] == g) wdi[cmin[g]]++; }
        unsigned long long got_h[2] = {0, 0}; long long sr = 0, sd = 0;
        for (int r = 0; r < kSpread; r++) for (int f = 0; f < 2; f++) got_h[f] += head[r * kLsHead + f];
        if ((long long)got_h[0] != pf || (long long)got_h[1] != dropped) { printf("MISMATCH trial %d head: %llu %llu want %lld %lld\n", trial, got_h[0], got_h[1], pf, dropped); return 1; }
        for (int j = 0; j < kLsSteps; j++) { unsigned long long a = 0, b = 0; for (int r = 0; r < kSpread; r++) { a += cnt[(size_t)r * 2 * kLsSteps + j]; b += cnt[(size_t)r * 2 * kLsSteps + kLsSteps + j]; }
            const long long wa = j < S ? wr[j] : 0, wb = j < S ? wdi[j] : 0;
            if ((long long)a != wa || (long long)b != wb) { printf("MISMATCH trial %d step %d: %llu %llu want %lld %lld\n", trial, j, a, b, wa, wb); return 1; } sr += a; sd += b; }
        printf("trial %d ok: N %ld mode %d steps %d radius %ld pf %lld dropped %lld reads %lld distinct %lld\n", trial, (long)N, mode, S, (long)radius, pf, dropped, sr, sd);
    }
    return 0;
}
