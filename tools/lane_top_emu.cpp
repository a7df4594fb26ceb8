// lane_top_emu.cpp - k_lt_hist, k_lt_collect and k_lt_spread (csrc/lane_top.inc) run on the CPU: the kernels' source
// is compiled as it stands on the shims of tools/wave_emu.h (a fiber per lane, switched at the collectives).  Lanes of
// scattered groups of sizes 2 .. 600, of equal reads (one group holds the lane) and of pairs only, tiles of less than
// a run and of a run and a bit, a tile index never added: the first pass's bins and the 16 levels, a linear pass over
// a range of keys (bins and the roots above it), the candidates at a threshold, and tile_count and exact of a list
// are compared with the definitions of include/welldup_lanetop.h computed directly.  Prints MISMATCH and exits 1 on
// a difference.  tests/test_lanetop_emu.py builds and runs it; no GPU is involved, and nothing here says anything
// about time.
//
//   g++ -O1 -g -std=c++17 -fsanitize=undefined -Iinclude tools/lane_top_emu.cpp -o lane_top_emu
#include "wave_emu.h"
#include <map>
#include <set>
constexpr int kLaneTopMaxPasses = 8;
#define WD_LANE_TOP_EMU
#include "../well_duplicates_amd/csrc/lane_top.inc"

struct Args { const int *tile_idx; int64_t N; int T; const uint32_t *label, *members, *rows; int words; int first; unsigned long long lo; int shift; uint32_t nb; unsigned long long *hist;
              unsigned long long thr; uint2 *cand; uint32_t cap; uint32_t *count; const uint2 *tab; int n; uint32_t *tcnt, *exact; };
static Args A;
static void entry_hist() { k_lt_hist(A.tile_idx, A.N, A.label, A.members, A.first, A.lo, A.shift, A.nb, A.hist); }
static void entry_collect() { k_lt_collect(A.tile_idx, A.N, A.label, A.members, A.thr, A.cand, A.cap, A.count); }
static void entry_spread() { k_lt_spread(A.tile_idx, A.N, A.T, A.label, A.rows, A.words, A.tab, A.n, A.tcnt, A.exact); }
static const unsigned kEdges[16] = WD_LANETOP_EDGES;
static int want_level(unsigned s) { int l = 0; while (l + 1 < 16 && s >= kEdges[l + 1]) l++; return l; }
static int fail_(int trial, const char *what, long long got, long long want) { printf("MISMATCH trial %d %s: %lld want %lld\n", trial, what, got, want); return 1; }
int main() {
    srand(11);
    for (int trial = 0; trial < 18; trial++) {
        const int T = 3, mode = trial % 3, words = 1 + trial % 4;   // 0: scattered groups, 1: equal reads, 2: pairs only
        const int64_t N = trial / 3 % 2 ? 9000 : 700;               // two runs per tile, the second partial; or a partial one
        int tiles[2] = {2, 0};                                      // tile index 1 never added
        const size_t W = (size_t)N * T;
        std::vector<uint32_t> label(W, kInvalid), members(W, 0), rows(W * words);
        for (auto &r : rows) r = (uint32_t)rand() & 0x3FFFFFFFu;
        std::vector<size_t> pf;
        for (int ti : tiles) for (int64_t w = 0; w < N; w++) if (rand() % 10 || mode == 2) pf.push_back((size_t)ti * N + w);
        std::sort(pf.begin(), pf.end());
        if (mode == 1) for (size_t g : pf) label[g] = (uint32_t)pf[0];
        else if (mode == 2) { for (size_t i = 0; i + 1 < pf.size(); i += 2) label[pf[i]] = label[pf[i + 1]] = (uint32_t)pf[i]; if (pf.size() % 2) label[pf.back()] = (uint32_t)pf.back(); }
        else {
            std::vector<size_t> sh(pf); for (size_t i = sh.size(); i > 1; i--) std::swap(sh[i - 1], sh[(size_t)rand() % i]);
            const int sizes[] = {600, 101, 100, 99, 65, 64, 63, 50, 49, 24, 23, 12, 11, 10, 9, 8, 7, 3, 3, 2, 2, 2, 2, 2};
            size_t at = 0;
            for (int s : sizes) { if (at + s > sh.size()) break; size_t r = *std::min_element(sh.begin() + at, sh.begin() + at + s); for (int j = 0; j < s; j++) label[sh[at + j]] = (uint32_t)r; at += s; }
            for (; at < sh.size(); at++) label[sh[at]] = (uint32_t)sh[at];
        }
        std::map<uint32_t, std::vector<size_t>> groups;
        for (size_t g : pf) { if (label[g] != g) members[label[g]]++; groups[label[g]].push_back(g); }
        for (size_t g : pf) if (label[g] != g && rand() % 3) memcpy(&rows[g * words], &rows[(size_t)label[g] * words], 4 * words);   // two of three copies exact
        // ---- the first pass
        std::vector<unsigned long long> hist((size_t)kSpread * kLtRow, 0);
        const unsigned nbx = (unsigned)((N + kLaneRun - 1) / kLaneRun);
        A = Args{}; A.tile_idx = tiles; A.N = N; A.T = T; A.label = label.data(); A.members = members.data(); A.rows = rows.data(); A.words = words;
        A.first = 1; A.nb = kLtFirstBins; A.hist = hist.data();
        for (unsigned by = 0; by < 2; by++) for (unsigned bx = 0; bx < nbx; bx++) run_block(bx, by, entry_hist);
        std::vector<long long> want(kLtRow, 0);
        std::vector<unsigned long long> keys;
        for (auto &kv : groups) { const unsigned s = (unsigned)kv.second.size(); const int l = want_level(s); want[kLtLev + l]++; want[kLtLev + kLtLevels + l] += s;
            if (s >= 2) { int b = 0; while (b + 1 < kLtFirstBins && lt_first_lo(b + 1) <= s) b++; want[b]++; keys.push_back(((unsigned long long)s << 32) | (uint32_t)~kv.first); } }
        for (int i = 0; i < kLtRow; i++) { unsigned long long a = 0; for (int r = 0; r < kSpread; r++) a += hist[(size_t)r * kLtRow + i]; if ((long long)a != want[i]) return fail_(trial, "first pass word", (long long)a, want[i]) + 0 * printf("  word %d\n", i); }
        std::sort(keys.begin(), keys.end());
        // ---- a linear pass over the keys from the median up to the 9/10 quantile, and the candidates from there
        long long n_cand = 0;
        if (!keys.empty()) {
            const unsigned long long lo = keys[keys.size() / 2], hi = keys[keys.size() * 9 / 10] + 1, width = hi - lo;
            int shift = 0; while (((width - 1) >> shift) + 1 > (unsigned long long)kLtBins) shift++;
            const uint32_t nb = (uint32_t)(((width - 1) >> shift) + 1);
            std::fill(hist.begin(), hist.end(), 0); A.first = 0; A.lo = lo; A.shift = shift; A.nb = nb;
            for (unsigned by = 0; by < 2; by++) for (unsigned bx = 0; bx < nbx; bx++) run_block(bx, by, entry_hist);
            std::fill(want.begin(), want.end(), 0);
            for (unsigned long long k : keys) if (k >= lo) { const unsigned long long b = (k - lo) >> shift; want[b < nb ? b : kLtAbove]++; }
            for (int i = 0; i < kLtRow; i++) { unsigned long long a = 0; for (int r = 0; r < kSpread; r++) a += hist[(size_t)r * kLtRow + i]; if ((long long)a != want[i]) return fail_(trial, "linear pass word", (long long)a, want[i]); }
            std::vector<uint2> cand(keys.size() + 1, uint2{0, 0}); uint32_t count = 0;
            A.thr = lo; A.cand = cand.data(); A.cap = (uint32_t)(trial % 2 ? keys.size() : keys.size() / 4); A.count = &count;   // (a short buffer is not written past)
            for (unsigned by = 0; by < 2; by++) for (unsigned bx = 0; bx < nbx; bx++) run_block(bx, by, entry_collect);
            std::set<unsigned long long> got, wantk;
            for (unsigned long long k : keys) if (k >= lo) wantk.insert(k);
            if (count != wantk.size()) return fail_(trial, "candidates", count, (long long)wantk.size());
            for (uint32_t i = 0; i < std::min(count, A.cap); i++) got.insert(((unsigned long long)cand[i].y << 32) | (uint32_t)~cand[i].x);
            for (size_t i = A.cap; i < cand.size(); i++) if (cand[i].x || cand[i].y) return fail_(trial, "written past the capacity at", (long long)i, 0);
            if (got.size() != std::min<size_t>(count, A.cap)) return fail_(trial, "distinct candidates", (long long)got.size(), count);
            for (unsigned long long k : got) if (!wantk.count(k)) return fail_(trial, "a candidate below the threshold", (long long)k, 0);
            n_cand = count;
        }
        // ---- the spread of the (up to) 1024 largest
        const int n = (int)std::min<size_t>(keys.size(), trial % 2 ? WD_LANETOP_MAX : 5);
        std::vector<uint2> tab(kLtSlots, uint2{kInvalid, 0});
        std::vector<uint32_t> list(n), tcnt((size_t)WD_LANETOP_MAX * T, 0), exact(WD_LANETOP_MAX, 0);
        for (int r = 0; r < n; r++) { list[r] = ~(uint32_t)keys[keys.size() - 1 - r]; uint32_t s = lt_slot(list[r]); while (tab[s].x != kInvalid) s = (s + 1) & (kLtSlots - 1); tab[s] = uint2{list[r], (uint32_t)r}; }
        A.tab = tab.data(); A.n = n; A.tcnt = tcnt.data(); A.exact = exact.data();
        for (unsigned by = 0; by < 2; by++) for (unsigned bx = 0; bx < nbx; bx++) run_block(bx, by, entry_spread);
        for (int r = 0; r < WD_LANETOP_MAX; r++) {
            std::vector<long long> wt(T, 0); long long we = 0;
            if (r < n) for (size_t g : groups[list[r]]) { wt[g / N]++; we += !memcmp(&rows[g * words], &rows[(size_t)list[r] * words], 4 * words); }
            for (int t = 0; t < T; t++) if (tcnt[(size_t)r * T + t] != wt[t]) return fail_(trial, "tile_count", tcnt[(size_t)r * T + t], wt[t]);
            if (exact[r] != we) return fail_(trial, "exact", exact[r], we);
        }
        printf("trial %d ok: N %ld mode %d words %d pf %zu groups %zu candidates %lld listed %d\n", trial, (long)N, mode, words, pf.size(), keys.size(), n_cand, n);
    }
    return 0;
}
