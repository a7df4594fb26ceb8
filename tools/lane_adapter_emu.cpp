// lane_adapter_emu.cpp - k_lad_tally (csrc/lane_adapter.inc, with lgc_piece of csrc/lane_gc.inc) run on the CPU under
// shuffled schedules: the kernel's source is compiled as it stands, twice - the bit-parallel search and the
// code-by-code one of -DWD_LAD_NAIVE -, the 256 lanes of a workgroup are fibers (tools/wave_emu.h) that meet at every
// barrier, ballot and shuffle, and every case runs under the eleven schedules of tools/emu_reads.h.  The rows, the
// search's table and the LDS staging block are heap blocks of exactly their size (the staging block: the wells of a
// sub-trip x the row stride), so a load or a store outside them is the address sanitizer's to report.
// Two parts, each compared with the definitions of include/welldup_laneadapter.h computed directly, char by char:
//   the search alone: lad_search of both forms on single rows, for every L of 9, 10, 37, 63, 64, 65, 83, 151, 1024 with
//     every m of 8, 13, 19, 32, every E of 0 .. 3 and every O of 3, 8, m (where O <= L); the host's table (lad_table)
//     against allowed(p) bit by bit.  The reads: the adapter planted at every p in 0 .. L - O; 0, 1, E and E + 1
//     substitutions that include the adapter's first base, its last (of those that fit) and a middle one; an N inside
//     the match; overlaps of O - 1, O, m - 1 and m at the read's end with allowed(p) and allowed(p) + 1 mismatches; two
//     matches in one read; for every adapter base j the plant that puts it on cycle 9, 10, 19, 20, 63, 64, 127 and 128
//     - both sides of the first boundaries of the ten-code row words and of the 64-bit position words - with that base
//     substituted alone and with E more; random reads;
//   the kernel: the same reads (or equal reads that carry the adapter, or pairs only) as the rows of two tiles of three
//     with families of 2 to 600 wells, N % 4 = 1, 2, 3 and a run and a bit, a rows' base 0 to 3 words past a 16-byte
//     boundary, counters that start at zero inside blocks that hold a pattern beyond.
// Prints MISMATCH and exits 1 on a difference.  -DWD_LAD_DROP_CARRY (the shift of the mismatch vector does not carry
// across the position words) must end so; -DLANE_ADAPTER_EMU_SHORT_LDS (the staging block one row short) must end in a
// sanitizer report: tests/test_laneadapter_emu.py builds and runs the three.  No GPU is involved, and nothing here says
// anything about time.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -Iinclude tools/lane_adapter_emu.cpp -o lane_adapter_emu
#include "wave_emu.h"
#include "emu_reads.h"
#include "welldup_laneadapter.h"
constexpr uint32_t kLmLow = 0x09249249u;            // (lane_mismatch.inc's: the lowest bit of each of a word's ten codes)
#define WD_LANE_GC_EMU
#include "../well_duplicates_amd/csrc/lane_gc.inc"
#define WD_LANE_ADAPTER_EMU
static uint32_t *lad_emu_stage;
namespace bitpar {
#include "../well_duplicates_amd/csrc/lane_adapter.inc"
}
#define WD_LAD_NAIVE 1
namespace naive {
#include "../well_duplicates_amd/csrc/lane_adapter.inc"
}
using bitpar::kLadCols; using bitpar::kLadTileCnt; using bitpar::kLadParWords; using bitpar::kLadParGe; using bitpar::kLadWindow;

struct Args { const int *tile_idx; int64_t N; const uint32_t *label, *members, *rows; int words, L, m, E, O; const unsigned long long *par; unsigned long long *cnt_t, *hist; };
static Args A;
static void entry_bitpar() { bitpar::k_lad_tally(A.tile_idx, A.N, A.label, A.members, A.rows, A.words, A.L, A.m, A.E, A.O, A.par, A.cnt_t, A.hist); }
static void entry_naive() { naive::k_lad_tally(A.tile_idx, A.N, A.label, A.members, A.rows, A.words, A.L, A.m, A.E, A.O, A.par, A.cnt_t, A.hist); }

// a heap block of exactly n elements (Buf rounds up to 256 bytes and more: not for what the sanitizer is to guard)
template <class T> struct Exact {
    T *p; size_t n;
    explicit Exact(size_t count) : p((T *)malloc(count * sizeof(T))), n(count) { memset((void *)p, 0xA5, n * sizeof(T)); }
    ~Exact() { free((void *)p); }
    Exact(const Exact &) = delete;
    void fill(int byte) { memset((void *)p, byte, n * sizeof(T)); }
    T &operator[](size_t i) { return p[i]; }
};

typedef std::vector<uint8_t> Read;
static std::mt19937 rng(41);

// the header's a(w), char by char; mism of the first match
static int def_a(const Read &r, const uint8_t *ad, int L, int m, int E, int O, int *mism)
{
    for (int p = 0; p + O <= L; p++) {
        const int o = std::min(m, L - p), allowed = o == m ? E : E * o / m;
        int mm = 0;
        for (int j = 0; j < o; j++) mm += r[p + j] != ad[j];
        if (mm <= allowed) { *mism = mm; return p; }
    }
    *mism = 0;
    return L;
}

// the adapter written over r from p, as much as fits; the bases of `subs` substituted, that of n_at an N
static void plant(Read &r, const uint8_t *ad, int L, int m, int p, uint32_t subs, int n_at = -1)
{
    for (int j = 0; j < m && p + j < L; j++)
        r[p + j] = j == n_at ? 4 : (subs >> j) & 1 ? (uint8_t)((ad[j] + 1 + rng() % 3) % 4) : ad[j];
}

// `count` bases of 0 .. o - 1 that include `must`
static uint32_t subs_with(int o, int must, int count)
{
    uint32_t s = 0;
    if (count > 0) s |= 1u << must;
    for (int j = (must + 1) % o, left = count - 1; left > 0 && j != must; j = (j + 1) % o) { s |= 1u << j; left--; }
    return s;
}

// the scripted reads of one (L, m, E, O); want_p: the p an exact plant was made at (-1: whatever comes)
static void scripted(std::vector<Read> &out, std::vector<int> &want_p, const uint8_t *ad, int L, int m, int E, int O)
{
    auto add = [&](int p, uint32_t subs, int n_at, int want) {
        if (p < 0 || p >= L) return;
        Read r;
        int mm;
        for (int tries = 0; tries < 200; tries++) {          // (a background that does not match before the plant)
            r = random_read(rng, L, 0);
            plant(r, ad, L, m, p, subs, n_at);
            if (want < 0) break;
            for (int a; (a = def_a(r, ad, L, m, E, O, &mm)) < want;) {      // a match before the plant: an N into it
                int j = 0;
                while (a + j < p && r[a + j] == 4) j++;
                if (a + j >= p) break;
                r[a + j] = 4;
            }
            if (def_a(r, ad, L, m, E, O, &mm) == want) break;
        }
        out.push_back(r); want_p.push_back(want);
    };
    for (int p = 0; p + O <= L; p++) add(p, 0, -1, p);
    const int ps[] = {0, (L - m) / 2, L - m, L - (m + O) / 2};
    for (int p : ps) if (p >= 0 && p + O <= L) {
        const int o = std::min(m, L - p);
        for (int must : {0, o - 1, o / 2}) for (int count : {0, 1, E, E + 1}) add(p, subs_with(o, must, std::min(count, o)), -1, -1);
        add(p, 0, o / 2, -1);                               // an N inside the match
        add(p, subs_with(o, 0, E), o - 1, -1);
    }
    for (int o : {O - 1, O, m - 1, m}) if (o >= 1 && o <= L) {
        const int p = L - o, allowed = o == m ? E : E * o / m;
        for (int count : {allowed, allowed + 1, 0}) if (count <= o) for (int must : {0, o - 1}) add(p, subs_with(o, must, count), -1, -1);
    }
    if (L >= 2 * m + 4) { Read r = random_read(rng, L, 0); plant(r, ad, L, m, 1, 0); plant(r, ad, L, m, m + 3, 0); out.push_back(r); want_p.push_back(-1);
        r = random_read(rng, L, 0); plant(r, ad, L, m, 2, subs_with(m, 1, E + 1)); plant(r, ad, L, m, m + 3, 0); out.push_back(r); want_p.push_back(-1); }
    for (int edge : {9, 10, 19, 20, 63, 64, 127, 128}) for (int j = 0; j < m; j++) {
        const int p = edge - j;
        if (p < 0 || p + O > L || edge >= L) continue;
        const int o = std::min(m, L - p);
        uint32_t more = 1u << j;                            // E more, after j where they fit, else before it
        for (int i = 1, left = E; left > 0 && i < o; i++) { const int at = j + i < o ? j + i : j + i - o; if (!((more >> at) & 1)) { more |= 1u << at; left--; } }
        add(p, 1u << j, -1, -1);
        add(p, more, -1, -1);
    }
    for (int i = 0; i < 40; i++) { out.push_back(random_read(rng, L, 30)); want_p.push_back(-1); }
}

static void pack(const Read &r, int L, int words, uint32_t *row)
{
    for (int k = 0; k < words; k++) row[k] = 0;
    for (int c = 0; c < L; c++) row[c / 10] |= (uint32_t)r[c] << (3 * (c % 10));
}

static const int kLs[] = {9, 10, 37, 63, 64, 65, 83, 151, 1024}, kMs[] = {8, 13, 19, 32};

// ---- part 1: the search alone
static int search_part()
{
    long rows = 0, combos = 0;
    for (int L : kLs) for (int m : kMs) for (int E = 0; E <= 3; E++) for (int oi = 0; oi < 3; oi++) {
        const int O = oi == 0 ? 3 : oi == 1 ? 8 : m;
        if (O > L || (oi == 2 && m == 8)) continue;
        uint8_t ad[32];
        for (int j = 0; j < m; j++) ad[j] = rng() % 4;
        Exact<unsigned long long> par(kLadParWords);
        bitpar::lad_table(ad, L, m, E, O, par.p);
        for (int p = 0; p < 64 * ((1024 + 63) / 64); p++) {    // the host's table against allowed(p)
            const int o = std::min(m, L - p), allowed = p + O > L ? -1 : o == m ? E : E * o / m;
            for (int e = 0; e < 4; e++)
                if ((int)((par[kLadParGe + 4 * (p / 64) + e] >> (p % 64)) & 1) != (e <= allowed)) {
                    printf("MISMATCH table L %d m %d E %d O %d: position %d e %d\n", L, m, E, O, p, e); return 1; }
        }
        std::vector<Read> reads; std::vector<int> want_p;
        scripted(reads, want_p, ad, L, m, E, O);
        const int words = (L + 9) / 10;
        std::vector<bool> hit(L + 1, false);
        for (size_t i = 0; i < reads.size(); i++) {
            Exact<uint32_t> row(words);
            pack(reads[i], L, words, row.p);
            int mm;
            const int a = def_a(reads[i], ad, L, m, E, O, &mm);
            const uint32_t want = (uint32_t)a | (uint32_t)mm << 16;
            const uint32_t got_b = bitpar::lad_search(row.p, words, L, m, E, O, par.p), got_n = naive::lad_search(row.p, words, L, m, E, O, par.p);
            if (got_b != want || got_n != want) {
                printf("MISMATCH search L %d m %d E %d O %d read %zu: bit-parallel %u/%u naive %u/%u want %d/%d\n", L, m, E, O, i,
                       got_b & 0xFFFF, got_b >> 16, got_n & 0xFFFF, got_n >> 16, a, mm); return 1; }
            if (want_p[i] >= 0 && a != want_p[i]) { printf("MISMATCH plant L %d m %d E %d O %d: p %d found at %d\n", L, m, E, O, want_p[i], a); return 1; }
            hit[a] = true; rows++;
        }
        for (int p = 0; p + O <= L; p++) if (!hit[p]) { printf("MISMATCH cover L %d m %d E %d O %d: no read with a = %d\n", L, m, E, O, p); return 1; }
        combos++;
    }
    printf("search ok: combos %ld rows %ld\n", combos, rows);
    return 0;
}

// ---- part 2: the kernel
int main()
{
    if (search_part()) return 1;
    constexpr int T = 3, kCases = 18;
    const int64_t Ns[] = {701, 702, 703, 8449};
    for (int trial = 0; trial < kCases; trial++) {
        const int L = kLs[trial % 9], m = kMs[(trial + trial / 9) % 4], E = (trial + trial / 4) % 4, words = (L + 9) / 10;
        const int O = std::min(L, trial % 3 == 0 ? 3 : trial % 3 == 1 ? std::min(8, m) : m);
        const int mode = trial < 12 ? 0 : 1 + trial % 2, mis = (trial + trial / 9) % 4;      // 0: scripted and random reads with families; 1: equal reads; 2: pairs only
        uint8_t ad[32];
        for (int j = 0; j < m; j++) ad[j] = rng() % 4;
        std::vector<Read> script; std::vector<int> want_p;
        scripted(script, want_p, ad, L, m, E, O);
        const int64_t N = L == 1024 ? 8449 : (trial % 9 == 7 ? 8449 : Ns[trial % 3]);
        int tiles[2] = {2, 0};                              // tile index 1 never added
        const size_t W = (size_t)N * T;
        Exact<uint32_t> store(W * words + mis);
        std::vector<uint32_t> label(W, kInvalid), members(W, 0);
        uint32_t *rows = store.p + mis;                     // the base, `mis` words past a 16-byte boundary
        std::vector<Read> code(W);
        Read one = random_read(rng, L, 0);
        plant(one, ad, L, m, std::min(L - O, 5 + trial), 0);
        size_t next = 0;
        for (int64_t w = 0; w < N; w++) for (int ti : tiles) {      // the scripted reads side by side on both tiles
            const size_t g = (size_t)ti * N + w;
            const bool planted = mode != 1 && next < script.size();
            code[g] = mode == 1 ? one : planted ? script[next++] : random_read(rng, L, 30);
            if (rng() % 10 || mode == 1 || planted) label[g] = (uint32_t)g;      // PF, its own root for now
        }
        long families = 0;
        auto family = [&](std::vector<size_t> ids) {
            std::sort(ids.begin(), ids.end());
            for (size_t i = 0; i < ids.size(); i++) { label[ids[i]] = (uint32_t)ids[0]; if (i) members[ids[0]]++; }
            families++;
        };
        if (mode == 0) {
            int64_t at = 3;
            for (int size : {2, 3, 63, 64, 65, 600}) {      // member j on tile 2 if j % 3 == 2, else on tile 0
                if (at + size > N) break;
                std::vector<size_t> ids;
                for (int j = 0; j < size; j++) ids.push_back((size_t)(j % 3 == 2 ? 2 * N : 0) + (size_t)(at + j));
                family(ids); at += size + 1;
            }
            for (int grp = 0; grp < 40; grp++) {
                std::vector<size_t> ids;
                for (int j = 0, want = 2 + rng() % 2; j < want; j++) {
                    const size_t g = (size_t)tiles[rng() % 2] * N + rng() % N;
                    if (label[g] == g && !members[g] && std::find(ids.begin(), ids.end(), g) == ids.end()) ids.push_back(g);
                }
                if (ids.size() >= 2) family(ids);
            }
        } else {
            std::vector<size_t> ids;
            for (size_t g = 0; g < W; g++) if (label[g] != kInvalid) {
                ids.push_back(g);
                if (mode == 2 && ids.size() == 2) { family(ids); ids.clear(); }
            }
            if (mode == 1) family(ids);
        }
        for (size_t g = 0; g < W; g++) if (!code[g].empty()) pack(code[g], L, words, rows + g * words);
        // the definitions, directly (the group sizes counted from the labels, not taken from members)
        std::vector<long long> size(W, 0), wt((size_t)T * kLadTileCnt, 0), wh((size_t)(L + 1) * 4, 0);
        for (size_t g = 0; g < W; g++) if (label[g] != kInvalid) size[label[g]]++;
        long with = 0, inexact = 0, partial = 0, beyond = 0, distinct_a = 0;
        for (int ti : tiles) for (int64_t w = 0; w < N; w++) {
            const size_t g = (size_t)ti * N + w; if (label[g] == kInvalid) continue;
            int mm;
            const int a = def_a(code[g], ad, L, m, E, O, &mm);
            const int pop = label[g] != g ? 2 : size[g] > 1 ? 1 : 0;
            long long *t = &wt[(size_t)ti * kLadTileCnt];
            t[0]++; t[1 + pop]++;
            distinct_a += wh[(size_t)a * 4] + wh[(size_t)a * 4 + 1] + wh[(size_t)a * 4 + 2] == 0;
            wh[(size_t)a * 4 + pop]++; if (pop == 1) wh[(size_t)a * 4 + 3] += size[g];
            beyond += a >= kLadWindow;
            if (a == L) continue;
            t[4 + pop]++; if (pop == 1) t[7] += size[g];
            t[8] += mm > 0; t[9] += a + m > L; t[10] += a;
            with++; inexact += mm > 0; partial += a + m > L;
        }
        Exact<unsigned long long> par(kLadParWords);
        bitpar::lad_table(ad, L, m, E, O, par.p);
        size_t stage_words = (size_t)bitpar::lad_sub_wells(words) * bitpar::lad_stride(words);
#ifdef LANE_ADAPTER_EMU_SHORT_LDS
        stage_words -= bitpar::lad_stride(words);           // (the bug the sanitizer must report)
#endif
        Exact<uint32_t> stage(stage_words);
        lad_emu_stage = stage.p;
        const unsigned nbx = (unsigned)((N + kLaneRun - 1) / kLaneRun);
        long points = 0;
        for (int form = 0; form < 2; form++) for (int s = 0; s < kSchedules; s++) {
            const bool permute = set_schedule(s, (unsigned)trial);
            Buf<unsigned long long> cnt_t((size_t)T * kSpread * kLadTileCnt), hist((size_t)(L + 1) * kSpread * kLadCols);
            cnt_t.fill(0); hist.fill(0); stage.fill(0xA5);
            A = Args{tiles, N, label.data(), members.data(), rows, words, L, m, E, O, par.p, cnt_t.p, hist.p};
            points += run_grid(nbx, 2, form ? entry_naive : entry_bitpar, permute).points;
            for (int t = 0; t < T; t++) for (int f = 0; f < kLadTileCnt; f++) { unsigned long long v = 0; for (int r = 0; r < kSpread; r++) v += cnt_t[((size_t)t * kSpread + r) * kLadTileCnt + f];
                if ((long long)v != wt[(size_t)t * kLadTileCnt + f]) { printf("MISMATCH case %d form %d schedule %d tile %d col %d: %llu want %lld\n", trial, form, s, t, f, v, wt[(size_t)t * kLadTileCnt + f]); return 1; } }
            for (int a = 0; a <= L; a++) for (int f = 0; f < 4; f++) { unsigned long long v = 0; for (int r = 0; r < kSpread; r++) v += hist[((size_t)a * kSpread + r) * 4 + f];
                if ((long long)v != wh[(size_t)a * 4 + f]) { printf("MISMATCH case %d form %d schedule %d a %d col %d: %llu want %lld\n", trial, form, s, a, f, v, wh[(size_t)a * 4 + f]); return 1; } }
        }
        printf("case %d ok: N %ld L %d words %d mis %d m %d E %d O %d mode %d schedules %d families %ld with %ld inexact %ld partial %ld beyond %ld distinct %ld sub %d points %ld\n",
               trial, (long)N, L, words, mis, m, E, O, mode, kSchedules, families, with, inexact, partial, beyond, distinct_a,
               bitpar::lad_sub_wells(words), points);
    }
    return 0;
}
