// lane_keep_emu.cpp - k_lk_score and k_lk_mark (csrc/lane_keep.inc, with lgc_piece of csrc/lane_gc.inc) run on the CPU
// under shuffled schedules: the kernels' source is compiled as it stands, the 256 lanes of a workgroup are fibers
// (tools/wave_emu.h) that meet at every barrier, ballot and shuffle, LDS is the kernels' static storage, and the two
// launches follow each other on LaneRun's grid as wd_lane_keep launches them, on a scratch that is cleared as far as the
// host call clears it - best all ones, the counters zero - and holds a pattern beyond (the scores, the masks).  Which
// lane's atomicMin reaches a family's word first depends on the schedule, so every case runs under the eleven
// schedules of tools/emu_reads.h: under each, every score, every family's word, every mask byte and every counter
// must be what the definitions of include/welldup_lanekeep.h give, computed directly - so every schedule gives the same.
// Cases: families of 2, 3, 63, 64, 65 and 600 wells (400 on a tile of less than a run) laid over two tiles, the wells
// of one family side by side so that they share waves, and across a run's boundary (N = 8193 and 9000: kLaneRun is
// 8192); a family all of one score (the root must win), the best well last, first and on the other tile, two wells
// sharing the top score; equal reads with one quality and with random ones (one label for every wave); rows of 1, 3,
// 4, 6, 16 and 103 words with the rows' base 0 to 3 words past a 16-byte boundary; N % 4 = 1, 2 and 3; min_q 0, 15
// and 64 (every weight zero); no mask for some tiles.  On the lanes of equal reads the atomicMin calls are counted and
// held to one per wave and trip.
// Prints MISMATCH and exits 1 on a difference.  With -DWAVE_EMU_TORN_MIN (the minimum torn: another fiber may lower the
// word between its load and its store) it must do so: tests/test_lanekeep_emu.py builds and runs both.  No GPU is
// involved, and nothing here says anything about time.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -Iinclude tools/lane_keep_emu.cpp -o lane_keep_emu
#include "wave_emu.h"
#include "emu_reads.h"
constexpr uint32_t kLmLow = 0x09249249u;            // (lane_mismatch.inc's: the lowest bit of each of a word's ten codes)
#define WD_LANE_GC_EMU
#include "../well_duplicates_amd/csrc/lane_gc.inc"
#define WD_LANE_KEEP_EMU
#include "../well_duplicates_amd/csrc/lane_keep.inc"

struct Args {
    const int *tile_idx; int64_t N; const uint32_t *label, *members, *qrows; int words; LkWeights wts;
    uint16_t *score; unsigned long long *best; uint8_t *const *maskp; unsigned long long *cnt_t, *cnt_l;
};
static Args A;
static void score_() { k_lk_score(A.tile_idx, A.N, A.label, A.members, A.qrows, A.words, A.wts, A.score, A.best); }
static void mark_() { k_lk_mark(A.tile_idx, A.N, A.label, A.members, A.score, A.best, A.maskp, A.cnt_t, A.cnt_l); }

static int fail_(const char *what, int trial, int s, long at, long long got, long long want)
{
    printf("MISMATCH case %d schedule %d (%s): %s %ld: %lld want %lld\n", trial, s, schedule_name(s), what, at, got, want);
    return 1;
}

static int gain_bin(long g) { return g == 0 ? 0 : g < 10 ? 1 : g < 20 ? 2 : g < 50 ? 3 : g < 100 ? 4 : g < 200 ? 5 : g < 500 ? 6 : 7; }

int main()
{
    std::mt19937 rng(29);
    const int edges[8] = {0, 2, 8, 14, 20, 26, 32, 38};
    const int Ls[] = {9, 25, 40, 51, 151, 1024};            // rows of 1, 3, 4, 6, 16 and 103 words
    const int64_t Ns[] = {701, 8193, 702, 9000, 703};       // N % 4 = 1, 1, 2, 0, 3; a run and a bit twice
    const int min_qs[] = {0, 15, 64};
    constexpr int T = 3, kCases = 18;
    for (int trial = 0; trial < kCases; trial++) {
        const int L = Ls[trial % 6], words = (L + 9) / 10, mode = trial < 12 ? 0 : 1 + trial % 2;      // 0: families, 1: equal reads of one quality, 2: of random ones
        const int mis = (trial + trial / 6) % 4, min_q = mode == 2 ? min_qs[trial / 2 % 2] : min_qs[(trial + trial / 3) % 3];      // (random qualities mean nothing at 64)
        const int64_t N = L == 1024 ? (trial < 12 ? Ns[(trial / 6) * 2] : 8193) : Ns[(trial + trial / 6) % 5];
        int tiles[2] = {2, 0};                              // tile index 1 never added
        const size_t W = (size_t)N * T;
        int w8[8];
        for (int b = 0; b < 8; b++) w8[b] = edges[b] >= min_q ? edges[b] : 0;
        const LkWeights wts = lk_weights_of(w8);                         // (the host's own arithmetic: the kernel's form of the weights)
        std::vector<uint32_t> store(W * words + 8, 0xFFFFFFFFu), label(W, kInvalid), members(W, 0);
        uint32_t *qrows = store.data();
        while ((int)(((uintptr_t)qrows >> 2) & 3) != mis) qrows++;      // the base, `mis` words past a 16-byte boundary
        std::vector<std::vector<uint8_t>> code(W);          // the bin of every cycle, per well of an added tile
        const uint8_t one_q = (uint8_t)(1 + rng() % 7);
        for (int ti : tiles) for (int64_t w = 0; w < N; w++) {
            const size_t g = (size_t)ti * N + w; code[g].resize(L);
            const int kind = mode == 2 ? 2 : rng() % 8;     // mostly random bins; some wells all of the top bin, all of bin 0 (not among the equal reads: the top score would come at once)
            for (int c = 0; c < L; c++) code[g][c] = mode == 1 ? one_q : kind == 0 ? 7 : kind == 1 ? 0 : (uint8_t)(rng() % 8);
            if (rng() % 10) label[g] = (uint32_t)g;         // PF, its own root for now
        }
        long planted = 0;
        auto family = [&](const std::vector<size_t> &ids) { // ascending ids, all made PF: the first is the root
            for (size_t i = 0; i < ids.size(); i++) { label[ids[i]] = (uint32_t)ids[0]; if (i) members[ids[0]]++; }
            planted++;
        };
        auto fill = [&](size_t g, uint8_t bin) { std::fill(code[g].begin(), code[g].end(), bin); };
        if (mode == 0) {
            // a family of `size` wells from well `at`: member j on tile 2 if j % 3 == 2, else on tile 0 - side by side
            // on both, the root on tile 0
            int64_t at = 7;
            auto block = [&](int size, int64_t from) {
                std::vector<size_t> lo, hi;
                for (int j = 0; j < size; j++) (j % 3 == 2 ? hi : lo).push_back((size_t)(j % 3 == 2 ? 2 * N : 0) + (size_t)(from + j));
                lo.insert(lo.end(), hi.begin(), hi.end());
                family(lo);
                return lo;
            };
            for (int size : {2, 3, 63, 64, 65}) { block(size, at); at += size + 1; }
            if (N > kLaneRun) block(600, std::min<int64_t>(kLaneRun - 300, N - 600)); else { block(400, at); at += 401; }      // (over the run's boundary on both tiles)
            if (N > kLaneRun) at = 300;
            // five wells each, f[0] .. f[3] on tile 0 and f[4] on tile 2: one score throughout; the best last (on the
            // other tile), first, and in the middle with the runner-up on the other tile; two sharing the top
            std::vector<size_t> f = block(5, at); at += 6; for (size_t g : f) fill(g, 5);
            f = block(5, at); at += 6; for (size_t g : f) fill(g, 1); fill(f[4], 7);
            f = block(5, at); at += 6; for (size_t g : f) fill(g, 2); fill(f[0], 7);
            f = block(5, at); at += 6; for (size_t g : f) fill(g, 3); fill(f[3], 7); fill(f[4], 5);
            f = block(5, at); at += 6; for (size_t g : f) fill(g, 1); fill(f[1], 6); fill(f[2], 6);
            // and sparse pairs and triples anywhere
            for (int grp = 0; grp < 80; grp++) {
                std::vector<size_t> ids;
                for (int j = 0, want = 2 + rng() % 2; j < want; j++) {
                    const size_t g = (size_t)tiles[rng() % 2] * N + rng() % N;
                    if (label[g] == g && !members[g] && std::find(ids.begin(), ids.end(), g) == ids.end()) ids.push_back(g);
                }
                std::sort(ids.begin(), ids.end());
                if (ids.size() >= 2) family(ids);
            }
        } else {
            std::vector<size_t> ids;
            for (size_t g = 0; g < W; g++) if (label[g] != kInvalid) ids.push_back(g);
            family(ids);
        }
        for (size_t g = 0; g < W; g++) if (!code[g].empty()) {
            for (int k = 0; k < words; k++) qrows[g * words + k] = 0;
            for (int c = 0; c < L; c++) qrows[g * words + c / 10] |= (uint32_t)code[g][c] << (3 * (c % 10));
        }
        // the definitions, directly
        std::vector<long long> sc(W, 0), want_t((size_t)T * kLkTileCnt, 0), want_l(kLkLaneCnt, 0);
        std::vector<unsigned long long> want_best(W, ~0ull);
        std::vector<uint8_t> want_mask(W, 0);
        std::map<uint32_t, std::vector<size_t>> fam;
        for (size_t g = 0; g < W; g++) if (!code[g].empty()) {
            for (int c = 0; c < L; c++) sc[g] += w8[code[g][c]];
            if (label[g] != kInvalid) fam[label[g]].push_back(g);
        }
        long families = 0, moved = 0;
        for (const auto &[root, wells] : fam) {
            size_t best = wells[0];
            for (size_t g : wells) if (sc[g] > sc[best]) best = g;      // (ascending: the first of the largest is the smallest id)
            if (wells.size() > 1) {
                want_best[root] = (unsigned long long)(0xFFFF - sc[best]) << 32 | best;
                want_l[kLkFamilies]++; want_l[kLkMoved] += best != root; want_l[kLkSumRoots] += sc[root];
                want_l[kLkGain + gain_bin((long)(sc[best] - sc[root]))]++;
                families++; moved += best != root;
            }
            for (size_t g : wells) {
                long long *t = &want_t[(g / N) * kLkTileCnt];
                const bool kept = g == best;
                t[0]++; t[kept ? 1 : 2]++; t[3] += kept && g != root; t[kept ? 4 : 5] += sc[g];
                want_mask[g] = kept;
            }
        }
        long bound = 0;                                     // waves x trips over the launch
        for (int64_t r0 = 0; r0 < N; r0 += kLaneRun) bound += 2 * (kTdBlock / kWave) * ((std::min<int64_t>(N, r0 + kLaneRun) - r0 + kTdBlock - 1) / kTdBlock);
        long mins_most = 0, points = 0;
        const unsigned nbx = (unsigned)((N + kLaneRun - 1) / kLaneRun);
        for (int s = 0; s < kSchedules; s++) {
            const bool permute = set_schedule(s, (unsigned)trial);
            Buf<uint16_t> score(W);                         // (0xA5: dirty)
            Buf<unsigned long long> best(W), cnt_t((size_t)T * kSpread * kLkTileCnt), cnt_l((size_t)kSpread * kLkLaneCnt);
            Buf<uint8_t> mask(W);
            best.fill(0xFF); cnt_t.fill(0); cnt_l.fill(0);
            uint8_t *maskp[T] = {trial % 2 ? nullptr : mask.p, nullptr, mask.p + 2 * N};      // (tile 0 has no mask in the odd cases)
            A = Args{tiles, N, label.data(), members.data(), qrows, words, wts, score.p, best.p, maskp, cnt_t.p, cnt_l.p};
            emu_mins = 0;
            points += run_grid(nbx, 2, score_, permute).points;
            const long mins = emu_mins;
            points += run_grid(nbx, 2, mark_, permute).points;
            mins_most = std::max(mins_most, mins);
            if (mode != 0 && mins > bound) return fail_("atomicMin calls on a lane of equal reads, bound", trial, s, 0, mins, bound);
            for (size_t g = 0; g < W; g++) {
                const bool added = !code[g].empty();
                if (score[g] != (added ? (uint16_t)sc[g] : (uint16_t)0xA5A5)) return fail_("score of well", trial, s, (long)g, score[g], sc[g]);
                if (best[g] != want_best[g]) return fail_("best of well", trial, s, (long)g, (long long)best[g], (long long)want_best[g]);
                const uint8_t *m = maskp[g / N];
                const uint8_t want = !added || !m ? 0xA5 : want_mask[g];
                if (mask[g] != want) return fail_("mask of well", trial, s, (long)g, mask[g], want);
            }
            for (int t = 0; t < T; t++) for (int f = 0; f < kLkTileCnt; f++) {
                unsigned long long v = 0; for (int r = 0; r < kSpread; r++) v += cnt_t[((size_t)t * kSpread + r) * kLkTileCnt + f];
                if ((long long)v != want_t[(size_t)t * kLkTileCnt + f]) return fail_("tile counter", trial, s, t * 100 + f, (long long)v, want_t[(size_t)t * kLkTileCnt + f]);
            }
            for (int f = 0; f < kLkLaneCnt; f++) {
                unsigned long long v = 0; for (int r = 0; r < kSpread; r++) v += cnt_l[(size_t)r * kLkLaneCnt + f];
                if ((long long)v != want_l[f]) return fail_("lane counter", trial, s, f, (long long)v, want_l[f]);
            }
        }
        printf("case %d ok: N %ld L %d words %d mis %d min_q %d mode %d schedules %d families %ld moved %ld planted %ld mins %ld bound %ld points %ld\n",
               trial, (long)N, L, words, mis, min_q, mode, kSchedules, families, moved, planted, mins_most, bound, points);
    }
    return 0;
}
