// lev2_stream.inc - Levenshtein distance <= 2 between EQUAL-LENGTH reads as a streaming closed form.
//
// The reference's production default is `-e 2` with the Levenshtein metric
// (count_well_duplicates.py:200, :252, :258, :282-283).  For reads of equal length, distance <= 2
// is one of two things (dense_forms.inc: lev2_window; tests/test_properties.py checks it against the
// textbook DP): at most two substitutions, or one deletion plus one insertion with exact matches
// everywhere else - the reads agree before the first mismatching cycle p and after the last one t,
// and in between one is the other shifted by one cycle:
//     up:    b[i] == a[i+1] for i in [p, t)          (a loses a[p], gains a symbol at t)
//     down:  b[i] == a[i-1] for i in (p, t]
// On a prefix the same test is a necessary condition, and it is the exact prefix criterion (a
// prefix pair that fails it cannot be completed to a pair within distance 2), so it prunes as well
// as the banded row DP does - for a dozen bit operations per ROUND of up to 8 cycles instead of
// some 50 per cycle.
//
// The state after any number of cycles is 12 bits, so a survivor's queue entry stays 8 bytes:
//     h      [0,2)   in-place mismatches so far, saturating at 3
//     up_run [2]     the up-shift has matched at every cycle since p   (meaningless while h == 0)
//     dn_run [3]     the down-shift has matched at every cycle since p
//     up_t   [4]     up_run as it stood at the last mismatch t: b[p..t) == a[p+1..t]
//     dn_t   [5]     the same for the down-shift: b(p..t] == a[p..t)
//     pa     [6,9)   the centre's code of the last cycle seen
//     pb     [9,12)  the neighbour's code of the last cycle seen
// A cycle's code is 3 bits in a 4-bit field: byte & 3, plus 4 if the byte is not 0 - so a no-call
// (byte 0, 'N' in the reference: bcl_direct_reader.py:352-361) is 0 and A, C, G, T are 4..7; N
// matches N and nothing else, as the reference's string compare has it.
//
// Plain C++ (no HIP intrinsics): tools/lev2_stream_check.cpp compiles this file for the CPU and runs
// it against the textbook distance (tests/test_lev2_stream.py).
#ifndef WD_HD
#define WD_HD __host__ __device__
#endif

constexpr uint32_t kLev2Nib = 0x11111111u;          // bit 0 of every 4-bit field

// code of one BCL byte, as above
WD_HD inline uint32_t lev2_code(uint32_t byte)
{
    return (byte & 3u) | ((byte < 1u ? byte : 1u) << 2);
}

// Four cycles of a well held as the bytes of one dword (the interleaved layout: byte q = cycle q)
// -> their codes in bits [0,16).
WD_HD inline uint32_t lev2_codes4(uint32_t w)
{
    // bit 7 of every byte that is not zero (exact: no carry crosses a byte)
    const uint32_t nz = (((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u;
    const uint32_t c = (w & 0x03030303u) | (nz >> 5);         // the code in bits [0,3) of every byte
    const uint32_t u = c | (c >> 4);                          // byte q's code also at 8q - 4
    return (u & 0xFFu) | ((u >> 8) & 0xFF00u);
}

WD_HD inline uint32_t lev2_init() { return 0u; }

// State after n more cycles (1 <= n <= 8).  a / b: the centre's / the neighbour's codes of those
// cycles, first cycle in bits [0,4); fields at and above 4n are ignored.
WD_HD inline uint32_t lev2_step(uint32_t st, uint32_t a, uint32_t b, int n)
{
    const uint32_t keep = n >= 8 ? kLev2Nib : (((1u << (4 * n)) - 1u) & kLev2Nib);
    const uint32_t pa = (st >> 6) & 7u, pb = (st >> 9) & 7u;
    const uint32_t x0 = a ^ b;
    const uint32_t xu = ((b << 4) | pb) ^ a;                  // field i: b[i-1] against a[i]
    const uint32_t xd = ((a << 4) | pa) ^ b;                  // field i: a[i-1] against b[i]
    const uint32_t m0 = (x0 | (x0 >> 1) | (x0 >> 2)) & keep;  // in-place mismatches of this round
    uint32_t mu = (xu | (xu >> 1) | (xu >> 2)) & keep;
    uint32_t md = (xd | (xd >> 1) | (xd >> 2)) & keep;
    const uint32_t h = st & 3u;
    const bool started = h != 0u;
    // the shift tests count from the cycle after the first mismatch p on: every cycle of this round
    // if p lies behind, else those above this round's first mismatch (none if there is none)
    const uint32_t first = m0 & (0u - m0);
    const uint32_t valid = started ? ~0u : ~(first | (first - 1u));
    mu &= valid;
    md &= valid;
    // cycles up to this round's last mismatch t
    const uint32_t le_t = m0 ? ((2u << (31 - __builtin_clz(m0))) - 1u) : 0u;
    const bool up_in = !started || ((st >> 2) & 1u), dn_in = !started || ((st >> 3) & 1u);
    const bool up_t = m0 ? (up_in && (mu & le_t) == 0u) : (((st >> 4) & 1u) != 0u);
    const bool dn_t = m0 ? (dn_in && (md & le_t) == 0u) : (((st >> 5) & 1u) != 0u);
    const bool up_run = up_in && mu == 0u, dn_run = dn_in && md == 0u;
    const uint32_t hn = h + (uint32_t)__builtin_popcount(m0);
    const int top = 4 * (n - 1);
    return (hn < 3u ? hn : 3u) | ((uint32_t)up_run << 2) | ((uint32_t)dn_run << 3) | ((uint32_t)up_t << 4) |
           ((uint32_t)dn_t << 5) | (((a >> top) & 7u) << 6) | (((b >> top) & 7u) << 9);
}

// Can the pair still end within distance 2?  After the last cycle: is it within distance 2?
WD_HD inline bool lev2_alive(uint32_t st) { return (st & 3u) < 3u || (st & 0x30u) != 0u; }

// The distance of a pair that is within 2 (one length-preserving edit is a substitution, so a pair
// with more than two mismatching cycles that passes is at distance exactly 2).
WD_HD inline int lev2_dist(uint32_t st) { return (st & 3u) < 3u ? (int)(st & 3u) : 2; }
