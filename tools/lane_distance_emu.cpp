// lane_distance_emu.cpp - k_lg_tally (csrc/lane_distance.inc) run on the CPU: the kernel's source is compiled as it
// stands on the shims of tools/wave_emu.h (a fiber per lane, switched at the collectives).  Lanes of sparse pairs, of
// equal reads (every pair on one root) and of copies that all sit beside their originals, tiles of less than a run
// and of a run and a bit, radii 0, 32, 2500 and 2^25, with the matrix and without: the counters, Dist and TilePairs
// are compared with the definitions of include/welldup_lanedistance.h computed directly (the bins by compares, not
// by the highest bit).  Prints MISMATCH and exits 1 on a difference.  tests/test_lanedistance_emu.py builds and runs
// it; no GPU is involved, and nothing here says anything about time.
//
//   g++ -O1 -g -std=c++17 -fsanitize=undefined -Iinclude tools/lane_distance_emu.cpp -o lane_distance_emu
#include "wave_emu.h"
#define WD_LANE_DISTANCE_EMU
#include "../well_duplicates_amd/csrc/lane_distance.inc"

struct Args { const int *tile_idx; int64_t N; const uint32_t *label; const int2 *xy; unsigned long long radius2; int n_hist; unsigned long long *cnt_t, *cnt_l, *pairs; };
static Args A;
static void entry() { k_lg_tally(A.tile_idx, A.N, A.label, A.xy, A.radius2, A.n_hist, A.cnt_t, A.cnt_l, A.pairs); }
static int want_bin(unsigned long long q) { int b = 0; while (b < 10 && q >= (1ull << (10 + 2 * b))) b++; return b; }
int main() {
    srand(5);
    const int64_t radii[] = {0, 32, 2500, 1 << 25};
    for (int trial = 0; trial < 24; trial++) {
        const int T = 3, mode = trial / 2 % 3;              // 0: sparse pairs, 1: equal reads, 2: every odd well a copy of the well before it
        const int64_t N = trial % 2 ? 9000 : 700, radius = radii[trial / 6];     // two runs per tile, the second partial; or a partial one
        const int matrix = (trial + trial / 6) % 2;
        int tiles[2] = {2, 0};                              // tile index 1 never added
        const size_t W = (size_t)N * T;
        std::vector<uint32_t> label(W, kInvalid);
        std::vector<int2> xy(N);
        for (int64_t w = 0; w < N; w++)                     // most wells in a corner of 3000 x 3000, the rest anywhere: every bin
            xy[w] = rand() % 4 ? int2{rand() % 3000, rand() % 3000} : int2{rand() % (1 << 24), rand() % (1 << 24)};
        xy[3] = int2{0, 0};
        xy[N - 1] = int2{(1 << 24) - 1, (1 << 24) - 1};     // (q = 2^49 - 2^26 + 2 from well 3: what 32 bits cannot hold)
        if (mode == 2) for (int64_t w = 1; w < N - 1; w += 2) xy[w] = int2{std::min(xy[w - 1].x + rand() % 20, (1 << 24) - 1), std::min(xy[w - 1].y + rand() % 20, (1 << 24) - 1)};
        for (int ti : tiles) for (int64_t w = 0; w < N; w++) if (rand() % 10 || mode == 2) label[(size_t)ti * N + w] = (uint32_t)((size_t)ti * N + w);
        const size_t root0 = 3; label[root0] = (uint32_t)root0;
        for (int ti : tiles) for (int64_t w = 0; w < N; w++) {
            const size_t g = (size_t)ti * N + w; if (label[g] == kInvalid || g == root0) continue;
            size_t r = root0;
            if (mode == 0) { if (rand() % 12) continue; r = (size_t)(rand() % 2 ? ti : 0) * N + rand() % N; if (r >= g || label[r] != r) continue; }
            if (mode == 2) { if (w % 2 == 0 || w == N - 1) continue; r = g - 1; }
            label[g] = (uint32_t)r;
        }
        // (a root is its own root: a well whose root has meanwhile become a member goes back to being single)
        for (size_t g = 0; g < W; g++) if (label[g] != kInvalid && label[g] != g && label[label[g]] != label[g]) label[g] = (uint32_t)g;
        std::vector<unsigned long long> cnt_t((size_t)T * kSpread * kLgTileCnt, 0), cnt_l(kSpread * kLgLaneCnt, 0), pairs((size_t)T * T, 0);
        A = Args{tiles, N, label.data(), xy.data(), (unsigned long long)radius * (unsigned long long)radius, matrix ? T : 0, cnt_t.data(), cnt_l.data(), pairs.data()};
        for (unsigned by = 0; by < 2; by++) for (unsigned bx = 0; bx < (unsigned)((N + kLaneRun - 1) / kLaneRun); bx++) run_block(bx, by, entry);
        // the definitions, directly
        std::vector<long long> wt((size_t)T * 3, 0), wd(11, 0), wp((size_t)T * T, 0);
        for (int ti : tiles) for (int64_t w = 0; w < N; w++) {
            const size_t g = (size_t)ti * N + w; if (label[g] == kInvalid || label[g] == g) continue;
            const size_t r = label[g]; const int rt = (int)(r / N);
            wt[ti * 3]++; if (matrix) wp[(size_t)rt * T + ti]++;
            if (rt != ti) continue;
            const long long dx = (long long)xy[w].x - xy[r % N].x, dy = (long long)xy[w].y - xy[r % N].y;
            const unsigned long long q = (unsigned long long)(dx * dx + dy * dy);
            wt[ti * 3 + 1]++; wd[want_bin(q)]++;
            if (q < (unsigned long long)radius * (unsigned long long)radius) wt[ti * 3 + 2]++;
        }
        long long sum[3] = {0, 0, 0};
        for (int t = 0; t < T; t++) for (int f = 0; f < 3; f++) { unsigned long long s = 0; for (int r = 0; r < kSpread; r++) s += cnt_t[((size_t)t * kSpread + r) * 3 + f];
            if ((long long)s != wt[t * 3 + f]) { printf("MISMATCH trial %d tile %d col %d: %llu want %lld\n", trial, t, f, s, wt[t * 3 + f]); return 1; } sum[f] += s; }
        for (int b = 0; b < 11; b++) { unsigned long long s = 0; for (int r = 0; r < kSpread; r++) s += cnt_l[r * kLgLaneCnt + b];
            if ((long long)s != wd[b]) { printf("MISMATCH trial %d dist %d: %llu want %lld\n", trial, b, s, wd[b]); return 1; } }
        for (size_t e = 0; e < pairs.size(); e++) if ((long long)pairs[e] != wp[e]) { printf("MISMATCH trial %d pairs %zu: %llu want %lld\n", trial, e, pairs[e], wp[e]); return 1; }
        printf("trial %d ok: N %ld mode %d radius %ld matrix %d pairs %lld same %lld local %lld dist", trial, (long)N, mode, (long)radius, matrix, sum[0], sum[1], sum[2]);
        for (int b = 0; b < 11; b++) printf(" %lld", wd[b]); printf("\n");
    }
    return 0;
}
