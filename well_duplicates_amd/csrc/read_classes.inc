// read_classes.inc - what the three parts of the tiledups unit (welldup_tiledups.hip, tile_near.inc,
// lane_dups.inc) build read classes from, each once: the alphabet and the fingerprint, the pass over the
// planes, the lock-free table, the compare loop on the planes, the wave-grouped add and the spread counters.
// Included by welldup_tiledups.hip before anything else of the unit, and by nothing outside it.  Everything
// here is inlined into the kernels that use it.

namespace {

using namespace wd;

constexpr unsigned long long kEmpty = ~0ull;       // a free slot (no entry looks like it: an id is < 2^32 - 1)
constexpr int kFpCycles = 10;                      // cycles folded per 30-bit word, and planes in flight per lane

// the reference's alphabet: byte 0 is N (4), any other byte its low two bits (bcl_direct_reader.py:352-361)
__device__ inline uint32_t code_of(uint32_t byte) { return byte ? (byte & 3u) : 4u; }

// ---- fingerprint ------------------------------------------------------------------------------
// Ten cycles, three bits each, make a 30-bit word; the words of a read go through two 32-bit
// multiplicative hashes (a 64-bit multiply per word and well would make the pass compute bound).
// Whatever this hash cannot tell apart is told apart on the reads by the insert (claim_or_join).
struct Fp {
    uint32_t a = 0x811C9DC5u, b = 0x01000193u;
    __device__ inline void fold(uint32_t w)
    {
        a = (a ^ w) * 0x9E3779B1u;
        a ^= a >> 15;
        b = (b + w) * 0x85EBCA6Bu;
        b ^= b >> 13;
    }
    __device__ inline unsigned long long value() const { return ((unsigned long long)a << 32) | b; }
};

__device__ inline unsigned long long mix64(unsigned long long x)      // (the murmur3 finaliser)
{
    x ^= x >> 33;
    x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33;
    x *= 0xC4CEB9FE1A85EC53ull;
    x ^= x >> 33;
    return x;
}

// ---- the plane pass -----------------------------------------------------------------------------
// One 30-bit word of wells w .. w + 3 from dword loads: planes c .. c1 - 1 (FULL: c .. c + kFpCycles - 1, all ten
// in flight).  Every plane is 4-byte aligned.  The plane pointers are the same for every lane: they come through
// the scalar cache.
template <bool FULL>
__device__ inline void plane_word4(const uint8_t *const *pl, int c, int c1, int64_t w, uint32_t (&acc)[4])
{
    if constexpr (FULL) {
        uint32_t v[kFpCycles];
#pragma unroll
        for (int j = 0; j < kFpCycles; j++)                 // (non-temporal: the planes are streamed)
            v[j] = __builtin_nontemporal_load((const uint32_t *)(pl[c + j] + w));
#pragma unroll
        for (int q = 0; q < 4; q++)
            acc[q] = 0;
#pragma unroll
        for (int j = 0; j < kFpCycles; j++)
#pragma unroll
            for (int q = 0; q < 4; q++)
                acc[q] |= code_of((v[j] >> (8 * q)) & 0xFFu) << (3 * j);
    } else {
#pragma unroll
        for (int q = 0; q < 4; q++)
            acc[q] = 0;
        for (int j = 0; c + j < c1; j++) {
            const uint32_t v = __builtin_nontemporal_load((const uint32_t *)(pl[c + j] + w));
#pragma unroll
            for (int q = 0; q < 4; q++)
                acc[q] |= code_of((v >> (8 * q)) & 0xFFu) << (3 * j);
        }
    }
}

// Cycles [c0, c1) of wells w .. w + 3 (QUAD: plane_word4) or of well w (byte loads: unaligned planes, and the
// last N % 4 wells of a tile), as 30-bit words of ten codes; the last word holds what is left.  word(k, acc)
// gets the k-th word of the pass, acc[q] that of well w + q.
template <bool QUAD, class Word>
__device__ inline void plane_pass(const uint8_t *const *pl, int c0, int c1, int64_t w, Word word)
{
    int c = c0, k = 0;
    if constexpr (QUAD) {
        for (; c + kFpCycles <= c1; c += kFpCycles, k++) {
            uint32_t acc[4];
            plane_word4<true>(pl, c, c1, w, acc);
            word(k, acc);
        }
        if (c < c1) {
            uint32_t acc[4];
            plane_word4<false>(pl, c, c1, w, acc);
            word(k, acc);
        }
    } else {
        for (; c < c1; c += kFpCycles, k++) {
            uint32_t acc[1] = {0};
            for (int j = 0; j < kFpCycles && c + j < c1; j++)
                acc[0] |= code_of(pl[c + j][w]) << (3 * j);
            word(k, acc);
        }
    }
}

// ---- the table ----------------------------------------------------------------------------------
// A slot is one 64-bit word (tag << 32) | id, all ones = free; the id it holds is the representative of a
// class (a well index in a tile's table, a global id in the lane's).  Memory model as for the parent
// pointers of welldup_sets.hip (per-XCD L2s, L1s that other CUs' stores never refresh): inside a kernel a
// slot is only touched by agent-scope atomics - a relaxed load, a CAS that claims a free slot with tag and
// own id at once, an atomic min that lowers the representative.  Why the outcome does not depend on the
// order of execution:
//   - a slot is claimed once and never freed, and every id that joins it has been compared with its
//     representative by same_class and found equal: all ids a slot ever names belong to one class, so a
//     stale representative is still a member of that class and decides a comparison the same way;
//   - a load that sees a free slot is followed by the CAS, which fails on a slot claimed meanwhile and
//     returns what it holds: the lane then treats the same slot as it would have, had it seen that value;
//   - every id of a class therefore passes the same slots (those of other classes on its probe path,
//     which never change class) and stops at the first that is free or its own class's: a class has
//     exactly one slot, and the min leaves its smallest id there, whichever lane came first.
// Equality is decided by same_class(cur) - exactly, on the reads or on the word itself - never by the tag: a
// tag only saves comparisons.  The caller sees to it that the table has a free slot left.
// tag has its low 32 bits clear, hash picks the first slot; returns the slot of id's class.
template <class Slot, class Same>
__device__ inline Slot claim_or_join(unsigned long long *table, Slot slot_mask, unsigned long long hash,
                                     unsigned long long tag, uint32_t id, Same same_class)
{
    const unsigned long long mine = tag | id;
    Slot s = (Slot)hash & slot_mask;
    for (;;) {
        // (a load first: a CAS straight away saved 6 % of k_td_insert on a tile of mostly unique reads, and
        // on a tile of equal reads put 4.3 M of them on one word - 49 ms instead of 3)
        unsigned long long cur = __hip_atomic_load(table + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kEmpty &&
            __hip_atomic_compare_exchange_strong(table + s, &cur, mine, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
            break;                                                     // claimed (else cur = what the slot holds now)
        if (same_class(cur)) {
            if (id < (uint32_t)cur)                                    // (the word only ever goes down)
                __hip_atomic_fetch_min(table + s, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            break;
        }
        s = (s + 1) & slot_mask;
    }
    return s;
}

// ---- comparing two wells on the planes --------------------------------------------------------------
// acc = step(acc, code of a, code of b) over the L cycles; settled(acc) is asked after every kCmpCycles
// cycles - with TAIL also after each of the last L % kCmpCycles - and ends the walk.
// (kCmpCycles cycles of both wells are loaded before the first is looked at: a lane that compared cycle by
// cycle waited for two dependent loads 150 times over, and its wave with it)
constexpr int kCmpCycles = 16;

template <bool TAIL, class T, class Step, class Settled>
__device__ inline T compare_wells(const uint8_t *const *pl, int L, uint32_t a, uint32_t b, T acc, Step step,
                                  Settled settled)
{
    int c = 0;
    for (; c + kCmpCycles <= L; c += kCmpCycles) {
        uint32_t x[kCmpCycles], y[kCmpCycles];
#pragma unroll
        for (int j = 0; j < kCmpCycles; j++) {
            const uint8_t *p = pl[c + j];
            x[j] = p[a];
            y[j] = p[b];
        }
#pragma unroll
        for (int j = 0; j < kCmpCycles; j++)
            acc = step(acc, code_of(x[j]), code_of(y[j]));
        if (settled(acc))
            return acc;
    }
    for (; c < L; c++) {
        const uint8_t *p = pl[c];
        acc = step(acc, code_of(p[a]), code_of(p[b]));
        if (TAIL && settled(acc))
            return acc;
    }
    return acc;
}

__device__ inline bool reads_equal(const uint8_t *const *pl, int L, uint32_t a, uint32_t b)
{
    return !compare_wells<true>(pl, L, a, b, 0u, [](uint32_t diff, uint32_t x, uint32_t y) { return diff | (x ^ y); },
                          [](uint32_t diff) { return diff != 0; });
}

// mismatching cycles of wells a and b, counted no further than the block in which they pass k
__device__ inline int hamming_upto(const uint8_t *const *pl, int L, uint32_t a, uint32_t b, int k)
{
    return compare_wells<false>(pl, L, a, b, 0, [](int d, uint32_t x, uint32_t y) { return d + (x != y); },
                         [k](int d) { return d > k; });
}

// ---- the wave-grouped add -----------------------------------------------------------------------
// The lanes of a wave that name the same word as the first active one add once, the others one each: what
// this lane has to add (wells of one class lie side by side when a tile's reads are all equal: 4.3 M adds
// to one word took 49 ms).  Every lane of the wave must call it.
__device__ inline uint32_t wave_grouped(bool active, uint32_t key)
{
    const unsigned long long act = __ballot(active);
    if (!act)
        return 0;
    const int lane = threadIdx.x & (kWave - 1), leader = __ffsll((long long)act) - 1;
    const uint32_t key0 = (uint32_t)__shfl((int)key, leader);
    const bool same = active && key == key0;
    const unsigned long long group = __ballot(same);
    if (lane == leader)
        return (uint32_t)__popcll(group);
    return active && !same ? 1u : 0u;
}

// ---- spread counters ----------------------------------------------------------------------------
// Counter rows in a workspace are [rows][kSpread][width] uint64: a workgroup adds its sums to copy
// blockIdx.x % kSpread and the host adds the copies up (one copy per row serialises the ~17 000
// workgroups of a 4.3 M-well tile on a few addresses: welldup_sets.hip)
constexpr int kSpread = 64;

__device__ inline unsigned long long *spread_row(unsigned long long *cnt, size_t row, int width)
{
    return cnt + (row * kSpread + blockIdx.x % kSpread) * width;
}

// out[0 .. width) = the sum of the kSpread copies of a row of the downloaded counters
void sum_spread(const unsigned long long *h_cnt, size_t row, int width, unsigned long long *out)
{
    std::fill(out, out + width, 0ull);
    for (int r = 0; r < kSpread; r++)
        for (int f = 0; f < width; f++)
            out[f] += h_cnt[(row * kSpread + r) * width + f];
}

}  // namespace
