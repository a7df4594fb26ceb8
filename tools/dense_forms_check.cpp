// CPU check of csrc/dense_forms.inc (the dense path's bit-level forms, with csrc/lev2_stream.inc under row_lev2)
// against the textbook edit distance:
//   g++ -O1 -std=c++17 -fsanitize=address,undefined tools/dense_forms_check.cpp -o check && ./check [seed] [scale]
// Reads are held as symbols (0..3 = A, C, G, T; 4 = N, a no-call).  The signature word, the screen word and the
// 16-dword packed row are built from them here, by the format the comment above k_dense_pack (scan_dense.inc)
// states; then, each against min(textbook distance, 3):
//   * lev2_window on the signature words, L <= 10;
//   * row_lev2 on signature words and rows; sig_mismatches + row_mismatches against the Hamming distance;
//   * lev2_masks on the three diagonals' mismatch masks, built as lev2_gather builds them;
//   * lev2_window16 on the screen words, against the distance of the 16-cycle prefixes with N read as A
//     (and screen_mismatches against their Hamming distance);
//   * lev2_screen <= 1 whenever the whole reads are within distance 2.
// Every pair is run in both orders.  fold10x4 (with codes4) and the pack kernel's arithmetic - fold8's three lines
// restated, then transpose4x4 - are driven dword by dword on four wells' raw bytes with random quality bits and
// must give the very words built from the symbols.
// -DDENSE_FORMS_BAD_CLZ breaks this program's own __clz shim so that the last mismatch t lands one field too low:
// such a build must exit non-zero (tests/test_dense_forms.py).  The shim errs by one signature field, three bits:
// by one BIT no result can change - the range masks keep bit 0 of every field only, and (1 << (3t - 1)) - (1 << 3p)
// covers the same field bits as (1 << 3t) - (1 << 3p).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <vector>

// ---- shims for what the forms take from HIP ----
static inline int __popc(uint32_t x) { return __builtin_popcount(x); }
static inline int __popcll(uint64_t x) { return __builtin_popcountll(x); }
static inline int __ffs(int x) { return __builtin_ffs(x); }
static inline int __clz(int x)
{
    const int n = x ? __builtin_clz((unsigned)x) : 32;
#ifdef DENSE_FORMS_BAD_CLZ
    return n + 3;
#else
    return n;
#endif
}
using std::max;
using std::min;
// v_perm_b32: byte i of the result is byte sel.byte[i] of the eight source bytes {s0, s1}, s1 the low four
static inline uint32_t perm_b32(uint32_t s0, uint32_t s1, uint32_t sel)
{
    const uint64_t src = ((uint64_t)s0 << 32) | s1;
    uint32_t out = 0;
    for (int i = 0; i < 4; i++) {
        const uint32_t s = (sel >> (8 * i)) & 0xFFu;
        if (s > 7u) {
            fprintf(stderr, "perm selector %u: only 0..7 are modelled\n", s);
            exit(2);
        }
        out |= (uint32_t)((src >> (8 * s)) & 0xFFu) << (8 * i);
    }
    return out;
}
#define __builtin_amdgcn_perm perm_b32

#define WD_HD
constexpr int kSigCycles = 10;          // wd_shared.h (dense_forms.inc asserts the value)
#include "../well_duplicates_amd/csrc/lev2_stream.inc"
#include "../well_duplicates_amd/csrc/dense_forms.inc"

typedef std::vector<uint8_t> Read;
static const int kLengths[] = {1, 2, 5, 8, 9, 10, 11, 15, 16, 17, 18, 26, 42, 43, 74, 75, 129, 159, 160};

static int textbook(const uint8_t *a, const uint8_t *b, int n)
{
    int row[256];                                  // row[j]: distance of a[0, i) and b[0, j)
    for (int j = 0; j <= n; j++)
        row[j] = j;
    for (int i = 1; i <= n; i++) {
        int diag = row[0], left = i;               // (i - 1, j - 1) and (i, j - 1)
        row[0] = i;
        const uint8_t ai = a[i - 1];
        for (int j = 1; j <= n; j++) {
            const int up = row[j];
            int v = diag + (ai != b[j - 1] ? 1 : 0);
            v = up + 1 < v ? up + 1 : v;
            v = left + 1 < v ? left + 1 : v;
            diag = up;
            row[j] = left = v;
        }
    }
    return row[n];
}

// ---- the words of a read, from its symbols ----
struct Words {
    uint32_t sig, scr, row[kRowDw];
};

static Words words_of(const Read &s, std::mt19937 &rng)
{
    const int L = (int)s.size();
    Words w;
    w.sig = w.scr = 0;
    for (int j = 0; j < L && j < kSigCycles; j++)
        w.sig |= (uint32_t)s[(size_t)j] << (3 * j);                           // 0..3, 4 = no-call
    for (int j = 0; j < L && j < kScreenCycles; j++)
        w.scr |= (uint32_t)(s[(size_t)j] & 3u) << (2 * j);                    // a no-call reads as A
    for (int i = 0; i < kRowDw; i++)
        w.row[i] = 0;
    for (int j = kSigCycles; j < L; j++) {
        const int r = j - kSigCycles, k = r / 32, q = r % 32;
        if (s[(size_t)j] != 4) {
            w.row[3 * k + (q >> 4)] |= (uint32_t)s[(size_t)j] << (2 * (q & 15));
            w.row[3 * k + 2] |= 1u << q;
        }
    }
    // groups the pack kernel never writes (and the last dword): whatever was there before
    for (int k = 0; k < kRowCycles / 32; k++)
        if (kSigCycles + 32 * k >= L)
            for (int i = 0; i < 3; i++)
                w.row[3 * k + i] = (uint32_t)rng();
    w.row[kRowDw - 1] = (uint32_t)rng();
    return w;
}

static long g_bad = 0, g_pairs = 0, g_at2 = 0;

static void fail(const char *what, const char *kind, int L, int p, int t, int want, int got)
{
    static std::map<std::string, int> seen;          // a few lines per form
    g_bad++;
    if (seen[what]++ < 4)
        fprintf(stderr, "MISMATCH %s: %s L %d p %d t %d want %d got %d\n", what, kind, L, p, t, want, got);
}

// one ordered pair through every form
static void check_ordered(const Read &a, const Read &b, const Words &wa, const Words &wb, int want, int ham, int want16,
                          int ham16, const char *kind, int p, int t)
{
    const int L = (int)a.size();
    if (L <= kSigCycles) {
        const int d = lev2_window(wa.sig, wb.sig);
        if (d != want)
            fail("lev2_window", kind, L, p, t, want, d);
    }
    {
        const int d = row_lev2(wa.sig, wb.sig, wa.row, wb.row, L);
        if (d != want)
            fail("row_lev2", kind, L, p, t, want, d);
        const int h = sig_mismatches(wa.sig, wb.sig) + row_mismatches(wa.row, wb.row, L);
        if (h != ham)
            fail("sig_mismatches + row_mismatches", kind, L, p, t, ham, h);
    }
    {
        uint64_t m0[3] = {0, 0, 0}, mp[3] = {0, 0, 0}, mm[3] = {0, 0, 0};
        for (int j = 0; j < L; j++) {
            const uint8_t a0 = a[(size_t)j], b0 = b[(size_t)j];
            const uint8_t a_next = a[(size_t)min(j + 1, L - 1)], a_prev = a[(size_t)max(j - 1, 0)];
            m0[j / 64] |= (uint64_t)(a0 != b0) << (j % 64);
            mp[j / 64] |= (uint64_t)(a_next != b0) << (j % 64);
            mm[j / 64] |= (uint64_t)(a_prev != b0) << (j % 64);
        }
        const int d = lev2_masks(m0, mp, mm);
        if (d != want)
            fail("lev2_masks", kind, L, p, t, want, d);
    }
    {
        const int d = lev2_window16(wa.scr, wb.scr);
        if (d != want16)
            fail("lev2_window16", kind, L, p, t, want16, d);
        const int h = (int)screen_mismatches(wa.scr, wb.scr);
        if (h != ham16)
            fail("screen_mismatches", kind, L, p, t, ham16, h);
        const uint32_t s = lev2_screen(wa.scr, wa.scr >> 2, wa.scr << 2, wb.scr);
        if (want <= 2 && s > 1u)
            fail("lev2_screen rejects a pair within 2", kind, L, p, t, 1, (int)s);
        if (want16 <= 2 && s > 1u)
            fail("lev2_screen rejects prefixes within 2", kind, L, p, t, 1, (int)s);
    }
}

static void check_pair(const Read &a, const Read &b, std::mt19937 &rng, const char *kind, int p = -1, int t = -1)
{
    const int L = (int)a.size(), P = min(L, kScreenCycles);
    const int dist = textbook(a.data(), b.data(), L), want = min(dist, 3);
    int ham = 0, ham16 = 0;
    uint8_t pa[kScreenCycles], pb[kScreenCycles];
    for (int j = 0; j < L; j++)
        ham += a[(size_t)j] != b[(size_t)j];
    for (int j = 0; j < P; j++) {
        pa[j] = a[(size_t)j] & 3u;
        pb[j] = b[(size_t)j] & 3u;
        ham16 += pa[j] != pb[j];
    }
    const int want16 = min(textbook(pa, pb, P), 3);
    const Words wa = words_of(a, rng), wb = words_of(b, rng);
    check_ordered(a, b, wa, wb, want, ham, want16, ham16, kind, p, t);
    check_ordered(b, a, wb, wa, want, ham, want16, ham16, kind, p, t);
    g_pairs += 2;
    g_at2 += 2 * (dist == 2);
}

// raw BCL byte of a symbol: base in the low two bits, some quality above; a no-call is 0
static uint8_t raw_byte(int sym, std::mt19937 &rng) { return sym == 4 ? 0 : (uint8_t)(sym | ((1 + rng() % 40) << 2)); }

// fold10x4 and the pack kernel's arithmetic on four wells' raw bytes against the words built from the symbols
static void check_quad(const Read *const (&s)[4], std::mt19937 &rng)
{
    const int L = (int)s[0]->size();
    std::vector<uint8_t> raw[4];
    Words w[4];
    for (int b = 0; b < 4; b++) {
        for (int j = 0; j < L; j++)
            raw[b].push_back(raw_byte((*s[b])[(size_t)j], rng));
        w[b] = words_of(*s[b], rng);
    }
    auto dword = [&](int j) -> uint32_t {         // one cycle of four wells, as a plane holds them
        return raw[0][(size_t)j] | ((uint32_t)raw[1][(size_t)j] << 8) | ((uint32_t)raw[2][(size_t)j] << 16) |
               ((uint32_t)raw[3][(size_t)j] << 24);
    };
    if (L >= kSigCycles) {
        uint32_t v[10], out[4];
        for (int f = 0; f < 10; f++)
            v[f] = dword(f);
        fold10x4(v, out);
        for (int b = 0; b < 4; b++)
            if (out[b] != w[b].sig)
                fail("fold10x4", "quad", L, b, -1, (int)w[b].sig, (int)out[b]);
    }
    for (int k = 0; k < kRowCycles / 32; k++) {
        const int jg = kSigCycles + 32 * k;
        if (jg >= L)
            break;
        uint32_t Q[8] = {0, 0, 0, 0, 0, 0, 0, 0}, Z[4] = {0, 0, 0, 0};
        for (int c = 0; c < 4; c++) {
            const int j0 = jg + 8 * c;
            if (j0 + 8 <= L) {                    // k_dense_pack's fold8
                uint32_t nz = 0;
                for (int f = 0; f < 8; f++) {
                    const uint32_t v = dword(j0 + f);
                    Q[2 * c + (f >> 2)] |= (v & 0x03030303u) << (2 * (f & 3));
                    const uint32_t x = ((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v;
                    nz = (x & 0x80808080u) | ((nz >> 1) & 0x7F7F7F7Fu);
                }
                Z[c] = nz;
            } else {                              // ... and its byte path for the read's last cycles
                for (int f = 0; f < 8 && j0 + f < L; f++)
                    for (int b = 0; b < 4; b++) {
                        const uint32_t byte = raw[b][(size_t)(j0 + f)];
                        Q[2 * c + (f >> 2)] |= (byte & 3u) << (8 * b + 2 * (f & 3));
                        Z[c] |= (byte ? 1u : 0u) << (8 * b + f);
                    }
            }
        }
        uint32_t lo[4], hi[4], nzw[4];
        transpose4x4(Q[0], Q[1], Q[2], Q[3], lo);
        transpose4x4(Q[4], Q[5], Q[6], Q[7], hi);
        transpose4x4(Z[0], Z[1], Z[2], Z[3], nzw);
        for (int b = 0; b < 4; b++)
            if (lo[b] != w[b].row[3 * k] || hi[b] != w[b].row[3 * k + 1] || nzw[b] != w[b].row[3 * k + 2])
                fail("pack arithmetic", "quad", L, b, k, (int)w[b].row[3 * k], (int)lo[b]);
    }
}

// ---- inputs ----
static Read random_read(int L, int alpha, std::mt19937 &rng)
{
    Read a((size_t)L);
    for (auto &v : a)
        v = (uint8_t)(rng() % alpha == 4 ? 4 : rng() % std::min(alpha, 4));
    return a;
}

// as tools/lev2_stream_check.cpp draws them
static void random_pairs(int L, long cases, std::mt19937 &rng)
{
    for (long c = 0; c < cases; c++) {
        const int alpha = (rng() % 4 == 0) ? 2 : 5;
        const Read a = random_read(L, alpha, rng);
        Read b = a;
        const char *kind = "substitutions";
        switch (rng() % 4) {
        case 0:
            for (int q = (int)(rng() % 4); q > 0; q--)
                b[rng() % L] = (uint8_t)(rng() % 5);
            break;
        case 1:
            kind = "one deletion, one insertion";
            if (L >= 2) {
                b.erase(b.begin() + (long)(rng() % L));
                b.insert(b.begin() + (long)(rng() % L), (uint8_t)(rng() % 5));
                if (rng() & 1)
                    b[rng() % L] = (uint8_t)(rng() % 5);
            }
            break;
        case 2:
            kind = "unrelated";
            b = random_read(L, alpha, rng);
            break;
        default:
            kind = "two shifted stretches";
            if (L >= 6) {
                b.erase(b.begin() + 1);
                b.insert(b.begin() + L / 2, (uint8_t)(rng() % 5));
                b.erase(b.begin() + L / 2 + 1);
                b.push_back((uint8_t)(rng() % 5));
            }
        }
        check_pair(a, b, rng, kind);
        if (c % 8 == 0) {
            const Read c2 = random_read(L, alpha, rng), d2 = random_read(L, 5, rng);
            const Read *const quad[4] = {&a, &b, &c2, &d2};
            check_quad(quad, rng);
        }
    }
}

static std::vector<int> boundary_set(int L)
{
    const int all[] = {0, 1, 7, 8, 9, 10, 11, 15, 16, 17, 18, 41, 42, 63, 64, 73, 74, 127, 128, L - 9, L - 8, L - 2, L - 1};
    std::vector<int> out;
    for (int v : all)
        if (v >= 0 && v < L)
            out.push_back(v);
    std::sort(out.begin(), out.end());
    out.erase(std::unique(out.begin(), out.end()), out.end());
    return out;
}

static Read shifted(const Read &a, int p, int t, bool up, uint8_t drawn)
{
    Read b = a;
    if (up) {
        for (int i = p; i < t; i++)
            b[(size_t)i] = a[(size_t)i + 1];
        b[(size_t)t] = drawn;
    } else {
        for (int i = p + 1; i <= t; i++)
            b[(size_t)i] = a[(size_t)i - 1];
        b[(size_t)p] = drawn;
    }
    return b;
}

static void substitute(Read &b, int at, std::mt19937 &rng) { b[(size_t)at] = (uint8_t)((b[(size_t)at] + 1 + rng() % 4) % 5); }

// the scripted kinds of tests/lev2_scripts.py, first mismatch p and last mismatch t as planned
static void scripted_pairs(int L, std::mt19937 &rng)
{
    const std::vector<int> B = boundary_set(L);
    for (int p : B)
        for (int t : B) {
            if (p >= t)
                continue;
            for (int dir = 0; dir < 2; dir++) {
                const bool up = dir == 0;
                const Read a = random_read(L, 5, rng);
                const Read b = shifted(a, p, t, up, (uint8_t)(rng() % 5));
                check_pair(a, b, rng, up ? "up" : "down", p, t);
                for (int at : {0, p - 1, t + 1, L - 1})
                    if (at >= 0 && at < L && (at < p || at > t)) {
                        Read c = b;
                        substitute(c, at, rng);
                        check_pair(a, c, rng, up ? "up + substitution outside" : "down + substitution outside", p, t);
                    }
                if (t - p >= 2) {
                    Read c = b;
                    substitute(c, p + 1 + (int)(rng() % (t - p - 1)), rng);
                    check_pair(a, c, rng, up ? "up + substitution inside" : "down + substitution inside", p, t);
                }
                {   // a no-call inside the shifted stretch of a; then read as A in b only
                    Read a2 = a;
                    const int m = up ? p + 1 + (int)(rng() % (t - p)) : p + (int)(rng() % (t - p));
                    a2[(size_t)m] = 4;
                    Read c = shifted(a2, p, t, up, (uint8_t)(rng() % 5));
                    check_pair(a2, c, rng, up ? "up over a no-call" : "down over a no-call", p, t);
                    c[(size_t)(up ? m - 1 : m + 1)] = 0;
                    check_pair(a2, c, rng, up ? "up, the no-call read as A" : "down, the no-call read as A", p, t);
                }
                {   // a stretch of two letters: fewer cycles mismatch in place than the shift spans
                    Read a2 = a;
                    const uint8_t x = (uint8_t)(rng() % 4), y = (uint8_t)((x + 1 + rng() % 3) % 4);
                    for (int i = p; i <= t; i++)
                        a2[(size_t)i] = (rng() & 1) ? x : y;
                    check_pair(a2, shifted(a2, p, t, up, (rng() & 1) ? x : y), rng, up ? "up, two letters" : "down, two letters", p, t);
                }
                if (t - p >= 2) {   // two separate stretches [p, m] and [m + 2, t]
                    const int m = p + (int)(rng() % (t - p - 1));
                    Read c = shifted(a, p, m, up, (uint8_t)(rng() % 5));
                    c = shifted(c, m + 2, t, (rng() & 1) != 0, (uint8_t)(rng() % 5));      // (disjoint: it reads a's cycles)
                    check_pair(a, c, rng, "two shifted stretches", p, t);
                }
            }
            {
                const Read a = random_read(L, 5, rng);
                Read c = a;
                substitute(c, p, rng);
                substitute(c, t, rng);
                check_pair(a, c, rng, "two substitutions", p, t);
                if (t - p >= 2) {
                    substitute(c, p + 1 + (int)(rng() % (t - p - 1)), rng);
                    check_pair(a, c, rng, "three substitutions", p, t);
                }
            }
        }
}

// every pair of reads over {A, C, N}
static void exhaustive(int L, std::mt19937 &rng)
{
    const uint8_t sym[3] = {0, 1, 4};
    int n = 1;
    for (int i = 0; i < L; i++)
        n *= 3;
    std::vector<Read> all((size_t)n, Read((size_t)L));
    for (int v = 0; v < n; v++)
        for (int i = 0, r = v; i < L; i++, r /= 3)
            all[(size_t)v][(size_t)i] = sym[r % 3];
    for (int x = 0; x < n; x++)
        for (int y = x; y < n; y++)               // (check_pair runs both orders)
            check_pair(all[(size_t)x], all[(size_t)y], rng, "exhaustive");
}

int main(int argc, char **argv)
{
    const unsigned seed = argc > 1 ? (unsigned)atoi(argv[1]) : 1u;
    const double scale = argc > 2 ? atof(argv[2]) : 1.0;
    std::mt19937 rng(seed);
    for (int L = 1; L <= 6; L++)
        exhaustive(L, rng);
    for (int L : kLengths) {
        if (g_bad)
            break;                                // (the first failing stage says enough)
        scripted_pairs(L, rng);
        // (the textbook distance costs L * L: fewer random pairs of the long reads)
        random_pairs(L, (long)(scale * std::min(30000.0, 1.5e8 / ((double)L * L))), rng);
    }
    printf("%ld pairs (%ld at distance exactly 2), %ld disagreements\n", g_pairs, g_at2, g_bad);
    return g_bad ? 1 : 0;
}
