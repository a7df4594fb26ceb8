// dense_forms.inc - the pure bit-level forms of the dense path (scan_dense.inc): folding plane dwords into
// signature words, the readers of a packed row, and the closed forms of Levenshtein <= 2 on signature words,
// screen words, packed rows and ballot masks.  Functions of their arguments only - no memory, no lane
// exchange - so that tools/dense_forms_check.cpp compiles this very file for the CPU (with shims for the few
// intrinsics) and runs every form against the textbook distance (tests/test_dense_forms.py).
// Included by scan_dense.inc after lev2_stream.inc; needs kSigCycles (wd_shared.h).
#ifndef WD_HD
#define WD_HD __host__ __device__
#endif
// keeps a value in a vector register and the compiler from looking through it (nothing on the host)
#if defined(__HIP_DEVICE_COMPILE__)
#define WD_OPAQUE_VGPR(x) asm volatile("" : "+v"(x))
#else
#define WD_OPAQUE_VGPR(x)
#endif

constexpr uint32_t kSigLow = 0x09249249u;                   // bit 0 of each 3-bit field
constexpr int kScreenCycles = 16;      // Levenshtein screen word: cycles 0..15, 2 bits each
constexpr int kRowCycles = 160;                       // cycles a row holds
constexpr int kRowDw = 16;                            // dwords per row (15 used)
static_assert(kSigCycles == 10 && 3 * kSigCycles <= 32, "the signature word: ten 3-bit fields, an 8 + 2 split in row_lev2");

// Four wells at a time: the base codes of the 4 bytes of a dword, each in its own byte lane
// (0..3 = byte & 3, 4 = the byte was 0, a no-call).
WD_HD inline uint32_t codes4(uint32_t v)
{
    const uint32_t zero = ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v) & 0x80808080u;     // bit 7 where byte == 0
    return (v & 0x03030303u) | (zero >> 5);
}

// Ten cycles of wells i .. i+3, one dword per plane (4 wells) -> one 30-bit word per well.
// Cycles are first paired inside the byte lanes (6 bits per lane), so the per-well unpacking
// happens 5 times instead of 10.
WD_HD inline void fold10x4(const uint32_t (&v)[10], uint32_t (&out)[4])
{
    out[0] = out[1] = out[2] = out[3] = 0;
#pragma unroll
    for (int m = 0; m < 5; m++) {
        const uint32_t pr = codes4(v[2 * m]) | (codes4(v[2 * m + 1]) << 3);
#pragma unroll
        for (int b = 0; b < 4; b++)
            out[b] |= ((pr >> (8 * b)) & 0x3Fu) << (6 * m);
    }
}

// mismatching cycles among those folded into two signatures
WD_HD inline int sig_mismatches(uint32_t x, uint32_t y)
{
    const uint32_t d = x ^ y;
    return __popc((d | (d >> 1) | (d >> 2)) & kSigLow);
}

// Levenshtein distance <= 2 between strings of EQUAL length is one of two things: at most two
// substitutions, or one deletion plus one insertion with exact matches everywhere else - the
// strings agree up to the first mismatch p and after the last mismatch t, and in between one is
// the other shifted by one position (b[i] == a[i+1] on [p, t), or b[i] == a[i-1] on (p, t]).
// On a prefix the same test is a necessary condition.  (tests/test_properties.py checks this
// characterisation against the textbook DP.)  Returns the distance if it is <= 2, else 3.
// a, b: up to 10 cycles, 3 bits each (unused high fields equal in both).
WD_HD inline int lev2_window(uint32_t a, uint32_t b)
{
    const uint32_t x = a ^ b;
    const uint32_t m0 = (x | (x >> 1) | (x >> 2)) & kSigLow;
    const int h = __popc(m0);
    if (h <= 2)
        return h;
    const int pb = __ffs((int)m0) - 1;                               // 3 * first mismatching field
    const int tb = 31 - __clz((int)m0);                              // 3 * last mismatching field
    const uint32_t rng = ((1u << tb) - (1u << pb)) & kSigLow;        // fields [p, t)
    const uint32_t xp = (a >> 3) ^ b;                                // b[i] against a[i+1]
    if ((((xp | (xp >> 1) | (xp >> 2)) & kSigLow) & rng) == 0)
        return 2;
    const uint32_t xm = (a << 3) ^ b;                                // b[i] against a[i-1]
    if ((((xm | (xm >> 1) | (xm >> 2)) & kSigLow) & (rng << 3)) == 0)
        return 2;
    return 3;
}

WD_HD inline void transpose4x4(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t (&r)[4])
{
    // r[b] = {a0.byte b, a1.byte b, a2.byte b, a3.byte b}
    const uint32_t p0 = __builtin_amdgcn_perm(a1, a0, 0x05010400u), p1 = __builtin_amdgcn_perm(a1, a0, 0x07030602u);
    const uint32_t q0 = __builtin_amdgcn_perm(a3, a2, 0x05010400u), q1 = __builtin_amdgcn_perm(a3, a2, 0x07030602u);
    r[0] = __builtin_amdgcn_perm(q0, p0, 0x05040100u);
    r[1] = __builtin_amdgcn_perm(q0, p0, 0x07060302u);
    r[2] = __builtin_amdgcn_perm(q1, p1, 0x05040100u);
    r[3] = __builtin_amdgcn_perm(q1, p1, 0x07060302u);
}

// ---- readers of a packed row (k_dense_verify) ----
// bit r of a 16-bit value -> bit 2r
WD_HD inline uint32_t spread16(uint32_t x)
{
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    return (x | (x << 1)) & 0x55555555u;
}

// mismatching cycles among cycles kSigCycles .. L-1 of two rows (no-call = a fifth symbol)
WD_HD inline int row_mismatches(const uint32_t *ra, const uint32_t *rb, int L)
{
    int mm = 0;
    // (unrolled with the bound as a predicate: as a loop over a run-time count the rows are indexed through
    // s_set_gpr_idx and copied into place first)
#pragma unroll
    for (int k = 0; k < kRowCycles / 32; k++) {
        const uint32_t xl = ra[3 * k] ^ rb[3 * k], xh = ra[3 * k + 1] ^ rb[3 * k + 1], nd = ra[3 * k + 2] ^ rb[3 * k + 2];
        const int m = __popc(((xl | (xl >> 1)) & 0x55555555u) | spread16(nd & 0xFFFFu)) +
                      __popc(((xh | (xh >> 1)) & 0x55555555u) | spread16(nd >> 16));
        mm += kSigCycles + 32 * k < L ? m : 0;
    }
    return mm;
}

// eight cycles (chunk c of group k) of a row as the 4-bit codes of lev2_stream.inc
WD_HD inline uint32_t row_codes8(const uint32_t *r, int k, int c)
{
    uint32_t x = (r[3 * k + (c >> 1)] >> (16 * (c & 1))) & 0xFFFFu;          // bases: two bits per cycle
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;                                         // ... in the low half of every nibble
    uint32_t y = (r[3 * k + 2] >> (8 * c)) & 0xFFu;                           // not a no-call: one bit per cycle
    y = (y | (y << 12)) & 0x000F000Fu;
    y = (y | (y << 6)) & 0x03030303u;
    y = (y | (y << 3)) & 0x11111111u;                                         // ... in bit 0 of every nibble
    return x | (y << 2);
}

// the first cycles of a read as the exact signature word holds them (3 bits each, no-call = 4) -> those codes
WD_HD inline uint32_t sig_codes(uint32_t sig, int first, int n)
{
    uint32_t w = 0;
    for (int f = 0; f < n; f++) {
        const uint32_t sgn = (sig >> (3 * (first + f))) & 7u;
        w |= (sgn < 4u ? (4u | sgn) : 0u) << (4 * f);
    }
    return w;
}

// Levenshtein distance of two whole reads if it is <= 2, else 3: the signature words for the first
// kSigCycles cycles, the rows for the rest, through the streaming closed form (lev2_stream.inc)
WD_HD inline int row_lev2(uint32_t sig_a, uint32_t sig_b, const uint32_t *ra, const uint32_t *rb, int L)
{
    uint32_t st = lev2_init();
    const int n0 = min(L, kSigCycles);
    st = lev2_step(st, sig_codes(sig_a, 0, min(n0, 8)), sig_codes(sig_b, 0, min(n0, 8)), min(n0, 8));
    if (n0 > 8)
        st = lev2_step(st, sig_codes(sig_a, 8, n0 - 8), sig_codes(sig_b, 8, n0 - 8), n0 - 8);
    for (int k = 0; k < kRowCycles / 32 && lev2_alive(st); k++)
        for (int c = 0; c < 4; c++) {
            const int n = min(8, L - (kSigCycles + 32 * k + 8 * c));
            if (n <= 0)
                break;
            st = lev2_step(st, row_codes8(ra, k, c), row_codes8(rb, k, c), n);
        }
    return lev2_alive(st) ? lev2_dist(st) : 3;
}

// The Levenshtein <= 2 screen of the compare stage, on screen words (16 cycles, 2 bits each; ah =
// a >> 2, al = a << 2), without branches.  Equal-length reads within distance 2 differ by at most
// two substitutions, or one is the other shifted by one cycle between the first mismatch p and
// the last one t (lev2_window) - then a cycle that mismatches both in place and against the
// shifted copy can only be t (b[i] = a[i+1] on [p, t)) or p (b[i] = a[i-1] on (p, t]).  Returns
// <= 1 if the pair may be within distance 2 on these cycles, which is necessary for being within
// distance 2 on the whole read.  Random reads pass with probability ~1e-4, so the survivors are
// the duplicates; k_dense_verify decides them exactly.  (tests/test_properties.py checks the screen
// against the textbook distance.)
WD_HD inline uint32_t lev2_screen(uint32_t a, uint32_t ah, uint32_t al, uint32_t b)
{
    const uint32_t x0 = a ^ b, xp = ah ^ b, xm = al ^ b;
    uint32_t m0 = (x0 | (x0 >> 1)) & 0x55555555u;
    // (opaque: otherwise the compiler distributes the two ANDs below over the ORs and spends six
    // three-input logic instructions per pair instead of three)
    WD_OPAQUE_VGPR(m0);
    const uint32_t up = (xp | (xp >> 1)) & m0;
    const uint32_t dn = (xm | (xm >> 1)) & m0;
    // popc(m0) - 1 <= 1 for one or two mismatches; identical words have up = dn = 0
    return min(min((uint32_t)__popc(m0) - 1u, (uint32_t)__popc(up)), (uint32_t)__popc(dn));
}

// lev2_window on screen words (up to 16 cycles, 2 bits each): the exact distance of the two
// 16-cycle prefixes as the screen sees them (a no-call reads as A) if it is <= 2, else 3 - what
// lev2_screen only bounds.  k_dense_mark runs it on the screen's survivors.
WD_HD inline int lev2_window16(uint32_t a, uint32_t b)
{
    const uint32_t x = a ^ b;
    const uint32_t m0 = (x | (x >> 1)) & 0x55555555u;
    const int h = __popc(m0);
    if (h <= 2)
        return h;
    const int pb = __ffs((int)m0) - 1;                               // 2 * first mismatching field
    const int tb = 31 - __clz((int)m0);                              // 2 * last mismatching field
    const uint32_t rng = ((1u << tb) - (1u << pb)) & 0x55555555u;    // fields [p, t)
    const uint32_t xp = (a >> 2) ^ b;                                // b[i] against a[i+1]
    if ((((xp | (xp >> 1)) & 0x55555555u) & rng) == 0)
        return 2;
    const uint32_t xm = (a << 2) ^ b;                                // b[i] against a[i-1]
    if ((((xm | (xm >> 1)) & 0x55555555u) & (rng << 2)) == 0)
        return 2;
    return 3;
}

// mismatching cycles among the (up to 16) folded into two screen words: a lower bound of the
// reads' Hamming distance (a no-call reads as A)
WD_HD inline uint32_t screen_mismatches(uint32_t x, uint32_t y)
{
    const uint32_t d = x ^ y;
    return (uint32_t)__popc((d | (d >> 1)) & 0x55555555u);
}

// The closed form (lev2_window) on the mismatch masks of the three diagonals, one bit per cycle in three
// 64-bit words (lev2_gather's ballots): m0 - b[j] against a[j], mp - against a[j+1], mm - against a[j-1].
// The distance if it is <= 2, else 3.
WD_HD inline int lev2_masks(const uint64_t (&m0)[3], const uint64_t (&mp)[3], const uint64_t (&mm)[3])
{
    const int h = __popcll(m0[0]) + __popcll(m0[1]) + __popcll(m0[2]);
    if (h <= 2)
        return h;
    const int first = m0[0] ? __builtin_ctzll(m0[0]) : m0[1] ? 64 + __builtin_ctzll(m0[1]) : 128 + __builtin_ctzll(m0[2]);
    const int last = m0[2] ? 191 - __builtin_clzll(m0[2]) : m0[1] ? 127 - __builtin_clzll(m0[1]) : 63 - __builtin_clzll(m0[0]);
    bool up = true, down = true;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        auto below = [](int n) -> uint64_t { return n >= 64 ? ~0ull : n <= 0 ? 0ull : ((1ull << n) - 1); };
        const uint64_t rng = below(last - 64 * ch) & ~below(first - 64 * ch);              // [first, last)
        const uint64_t rng2 = below(last + 1 - 64 * ch) & ~below(first + 1 - 64 * ch);     // (first, last]
        up = up && (mp[ch] & rng) == 0;
        down = down && (mm[ch] & rng2) == 0;
    }
    return (up || down) ? 2 : 3;
}
