// scan_queue.inc - survivor queue helpers and k_scan_q, the default equality / Hamming kernel.
// Included by welldup.hip after scan_sequential.inc.
// -------------------------------------------------------------------------------------
// Queue kernel (Hamming family with early exit): the default for equality / Hamming <= k
// -------------------------------------------------------------------------------------
// k_scan above pays one dependent HBM round trip per target per round, so reading fewer cycles
// in the first round (less traffic) only adds rounds (more latency).  This kernel makes the
// round, not the target, the unit of latency:
//   phase 0  the block stages its targets' metadata in LDS, reads all their filter bytes in
//            one go and builds the list of (valid target, pass) work items;
//   phase 1  each wave streams over its items with a 4-stage software pipeline (neighbour
//            indices two items ahead, plane bytes one item ahead, all loads unconditional so
//            the compiler's counted vmcnt keeps two gathers in flight).  Only B1 cycles are
//            read; neighbours still within k mismatches ("survivors", ~1/4^B1 of them) are
//            compacted into a small per-wave LDS queue {well index, target, slot, mismatches};
//   phase 2  the wave drains its queue in rounds of 1, 2, 4, 8 ... further cycles, one lane
//            per survivor (dense), re-compacting after each round; late survivors are finished
//            with one lane per cycle; whoever survives all L cycles is a duplicate and bumps
//            its target's per-level counter in LDS;
//   phase 3  per-target tallies -> block histogram (LDS atomics) -> one global atomic each.
// A pass holds 127 slots: lane 63 of the second slot always shadows the centre well, so the
// centre's byte comes out of the same load as the neighbours'.
constexpr int kFinishAllMax = 64;   // late survivors are read to their last cycle all at once (q_finish_all) while this few
#ifndef WD_QCAP
#define WD_QCAP 128
#endif
#ifndef WD_Q_OCC_IL
#define WD_Q_OCC_IL 8
#endif
constexpr int kQCap = WD_QCAP;      // >= kPass: after a drain one pass always fits (256 until round 4: 16 KB of queues per
                                    // workgroup, seven workgroups per CU; with 128 eight fit, and the interleaved kernels -
                                    // 60 registers - take them: equality 0.0791 -> 0.0747 ms, the others unchanged)
#ifndef WD_Q_DEPTH
#define WD_Q_DEPTH 1
#endif
constexpr int kQDepth = WD_Q_DEPTH; // steps between the issue of an item's plane-byte gather and its use (k_scan_q, phase 1)
constexpr int kFinishInPlace = 40;  // survivors of a pass's first round from which the pass is finished where it stands
                                    // (low-diversity reads: amplicons, failed cycles), not through the queue
static_assert(kQCap >= kPass && kQCap >= kFinishAllMax,
              "after a drain one pass must fit the queue, and q_finish_all adds up its pieces in the idle queue buffer");

// WD_Q_CHECK(event, value, bound): nothing on the device.  The CPU emulation (tools/scan_queue_emu.cpp) defines it to
// count the event, to note the value it came with (the queue's occupancy) and to assert the bound - what the comments
// here promise, checked where it is relied on.
#ifndef WD_Q_CHECK
#define WD_Q_CHECK(event, value, bound)
#endif

// A field of k_scan_q's kernel argument (ScanArgs is its only one), loaded WHERE IT IS USED.  Left to
// the compiler every field is fetched at the top of the kernel and then occupies scalar registers to
// its last use - the arguments of the tally phase and of the once-in-a-thousand duplicate path across
// the whole streaming loop, where the scalar file is what spills.
// (CPU emulation, WD_EMU: the same offset read from a host copy of the ScanArgs the launch was given, a heap block of
// sizeof(ScanArgs) bytes - the offsetof arithmetic of WD_LATE_ARG is then what a wrong offset shows in.)
template <typename T>
__device__ inline T late_arg(int offset)
{
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "one or two dwords");
#ifdef WD_EMU
    T v;
    memcpy(&v, emu_kernarg + offset, sizeof(T));
    return v;
#else
    const __attribute__((address_space(4))) char *kp =
        (const __attribute__((address_space(4))) char *)__builtin_amdgcn_kernarg_segment_ptr();
    T v;
    if constexpr (sizeof(T) == 8)
        asm volatile("s_load_dwordx2 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(kp), "s"(offset) : "memory");
    else
        asm volatile("s_load_dword %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(kp), "s"(offset) : "memory");
    return v;
#endif
}
#define WD_LATE_ARG(field) late_arg<decltype(ScanArgs::field)>((int)offsetof(ScanArgs, field))

// ---- survivor queue of k_scan_q -------------------------------------------------------
// A queue entry is {well index, tag}: tag = target-in-block << 24 | mismatches << 16 | slot.
struct QEnv {
    const int32_t *s_centre;      // LDS: centre index of each target of the block
    const int32_t *s_off;         // LDS: ring offsets, levels + 1 per target
    uint32_t *s_d;                // LDS: per-target per-level duplicate counters
    const uint32_t *s_tid;        // LDS, nullable: the targets' indices in the file (bits 0..30), where they are not
                                  // t_first + position (k_scan_lines: a block's targets are no run of the list)
    gbytes base0;                 // strided layout: cycle 0 plane of this tile
    const uint8_t *const *ptab;   // pointer-table layout: this tile's L plane pointers
    int64_t stride;
    int levels, L, k, tile, t_first;
};

// WS = bytes between consecutive wells of one cycle: 1 = a plane per cycle (the BCL files'
// layout); 4 = cycles interleaved in groups of four ([group][well][4]), where base0 is group 0
// of the tile and `stride` the bytes between groups, so that the 4 cycles of a well are one dword.
template <bool STRIDED, int WS = 1>
__device__ inline gbytes q_plane(const QEnv &v, int j)
{
    if (WS == 4)
        return v.base0 + (int64_t)(j >> 2) * v.stride + (j & 3);
    return STRIDED ? v.base0 + (int64_t)j * v.stride : as_global(v.ptab[j]);
}

// a duplicate found: bump its target's per-level counter (and the optional hit log)
__device__ inline void q_record_dup(const QEnv &v, int tl, int e, int dist)
{
    const int32_t *o = v.s_off + tl * (v.levels + 1);
    const int rel0 = o[0];
    int lev = 0;
    for (int l = 1; l < v.levels; l++)
        lev += (e >= o[l] - rel0) ? 1 : 0;
    atomicAdd(&v.s_d[tl * v.levels + lev], 1u);
    if (WD_LATE_ARG(log_hits)) {
        // (global address space throughout: see as_gptr, device_common.inc)
        gptr<const ScanRare> rp = as_gptr(WD_LATE_ARG(rare));
        gptr<const int32_t> perm = as_gptr(WD_LATE_ARG(perm));      // nullable: index in the targets file of the t-th target of the (sorted) view
        wd_hit *const hits = rp->hits;
        const long long hit_cap = rp->hit_cap;
        const unsigned long long h = g_atomic_add(rp->hit_count, 1ull);
        if ((long long)h < hit_cap) {
            const int t = v.s_tid ? (int)(v.s_tid[tl] & 0x7FFFFFFFu) : perm ? perm[v.t_first + tl] : v.t_first + tl;
            gptr<int32_t> rec = (gptr<int32_t>)as_gptr(hits + h);     // wd_hit: four int32 {tile, target, slot, dist}
            rec[0] = v.tile;
            rec[1] = t;
            rec[2] = rel0 + e;
            rec[3] = dist;
        }
    }
}

__device__ inline void q_wave_sync()
{
    // LDS traffic of one wave is processed in order; this only stops the compiler from
    // moving queue reads above the pushes of other lanes
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Drain a wave's queue: every entry has seen cycles [0, j0); rounds of 1, 2, 4, 8 ... more
// cycles, one lane per survivor, re-compacting after each round.  Whoever is still alive
// after 8 + 4k cycles is almost certainly a true duplicate (a random neighbour gets there
// with probability ~1e-5 or less): those are finished one entry at a time with one LANE PER
// CYCLE - a single ballot + popcount adds up 64 cycles' mismatches, so a duplicate costs
// ceil((L - 8) / 64) round trips instead of (L - 8) / 8.  (Entry-at-a-time is only cheap when
// entries are few: with k = 3 some 3 % of random neighbours are still alive at cycle 8.)
// qn is reset to 0.
// (finish_from: device_common.inc)
// Mismatching cycles among cycles j .. j + nc - 1 (all < L) between well idx and centre c: a whole round
// of NBT cycles issues its 2 NBT loads back to back with plane addresses that are plain arithmetic (no
// per-cycle clamps or conditions: those cost a scalar register pair each, times eight, live across the
// kernel's hot loop); a short last round goes cycle by cycle.
template <bool STRIDED, int WS, int NBT>
__device__ inline int q_round_mm(const QEnv &v, int j, int nc, uint32_t idx, uint32_t c)
{
    int mm = 0;
    if (nc == NBT) {
        uint32_t w[NBT], cb[NBT];
#pragma unroll
        for (int q = 0; q < NBT; q++) {
            gbytes p = q_plane<STRIDED, WS>(v, j + q);
            w[q] = ldb(p, idx * WS);
            cb[q] = ldb(p, c * WS);
        }
#pragma unroll
        for (int q = 0; q < NBT; q++)
            mm += code_of(w[q]) != code_of(cb[q]) ? 1 : 0;
    } else {
        for (int q = 0; q < nc; q++) {
            gbytes p = q_plane<STRIDED, WS>(v, j + q);
            mm += code_of(ldb(p, idx * WS)) != code_of(ldb(p, c * WS)) ? 1 : 0;
        }
    }
    return mm;
}

// The end of a drain: whoever is still queued after finish_from(k) cycles is read to the last cycle in ONE
// go - every lane takes a piece of 4 cycles of one entry, 8 loads issued back to back, the pieces' mismatch
// counts added up in LDS (the idle queue buffer) - so that all the duplicates of a wave cost one or two round
// trips to memory between them.  (Rounds 1 to 3 finished them one entry at a time, a lane per cycle: a round
// trip per duplicate at the end of every wave's life, a third of a workgroup's 25 us on the bench workload.)
constexpr int kFinishPiece = 4;      // (8 would spill registers in the line walk, whose pipeline registers are live across a drain)
template <bool STRIDED, int WS>
__device__ inline void q_finish_all(const QEnv &v, const uint2 *qa, uint2 *qb, int n, int j, int lane)
{
    const int L = v.L, k = v.k;
    const int pieces = (L - j + kFinishPiece - 1) / kFinishPiece;       // per entry, >= 1 (j < L)
    WD_Q_CHECK(finish_all, n, n >= 1 && n <= kFinishAllMax && n <= kQCap && j < L);     // (qb, a queue buffer, takes n sums)
    for (int i = lane; i < n; i += kWave)
        qb[i].x = 0u;
    q_wave_sync();
    const int units = n * pieces;
    for (int u0 = 0; u0 < units; u0 += kWave) {
        const int u = u0 + lane;
        if (u < units) {
            const int i = u / pieces, pc = u - i * pieces;
            const uint2 ent = qa[i];
            const uint32_t idx = ent.x, c = (uint32_t)v.s_centre[ent.y >> 24];
            const int jf = j + pc * kFinishPiece;
            uint32_t w[kFinishPiece], cb[kFinishPiece];
#pragma unroll
            for (int q = 0; q < kFinishPiece; q++) {
                gbytes p = q_plane<STRIDED, WS>(v, min(jf + q, L - 1));
                w[q] = ldb(p, idx * WS);
                cb[q] = ldb(p, c * WS);
            }
            uint32_t mm = 0;
#pragma unroll
            for (int q = 0; q < kFinishPiece; q++)
                mm += (jf + q < L && code_of(w[q]) != code_of(cb[q])) ? 1u : 0u;
            if (mm)
                atomicAdd(&qb[i].x, mm);
        }
    }
    q_wave_sync();
    for (int i = lane; i < n; i += kWave) {
        const uint2 ent = qa[i];
        const int mm = (int)((ent.y >> 16) & 0xFFu) + (int)qb[i].x;
        if (mm <= k)
            q_record_dup(v, (int)(ent.y >> 24), (int)(ent.y & 0xFFFFu), mm);
    }
}

template <bool STRIDED, int MAXB = 8, int WS = 1>
__device__ inline void q_drain(const QEnv &v, uint2 *q_a, uint2 *q_b, int &qn, int j0, int lane)
{
    q_wave_sync();
    WD_Q_CHECK(drain, qn, qn >= 0 && qn <= kQCap);
    const int L = v.L, k = v.k;
    int j = min(j0, L);
    // cycles of the first drain round (then 2, 4, .. MAXB; measured).  Interleaved: the rest of the group the
    // first round's dword did not cover costs no line of its own - a whole group at once
    int nb = (WS == 4 && (j & 3) == 0) ? 4 : 1;
    uint2 *qa = q_a, *qb = q_b;
    int n = qn;
    while (n > 0 && j < L) {
        // (all at once pays while entries are few - the survivors of 8 + 4k cycles are the duplicates; on
        // low-diversity input - amplicons, failed cycles - every neighbour gets here, and those are taken on 64 at a time,
        // 8 cycles a round: pieces of 8 cycles x 256 entries would be six rounds of loads for nothing)
        if (j >= finish_from(k) && n <= kFinishAllMax) {
            q_finish_all<STRIDED, WS>(v, qa, qb, n, j, lane);
            break;
        }
        const bool last = j + nb >= L;
        const int nc = min(nb, L - j);                 // cycles of this round that exist
        int n2 = 0;
        for (int p0 = 0; p0 < n; p0 += kWave) {
            const bool have = p0 + lane < n;
            uint2 ent = make_uint2(0u, 0u);
            if (have)
                ent = qa[p0 + lane];
            const uint32_t idx = ent.x;
            const int tl = (int)(ent.y >> 24);
            const int e = (int)(ent.y & 0xFFFFu);
            int mm = (int)((ent.y >> 16) & 0xFFu);
            if (have) {
                const uint32_t c = (uint32_t)v.s_centre[tl];
                static_assert(MAXB == 8, "rounds of 1, 2, 4, 8 cycles");
                switch (nb) {
                case 1: mm += q_round_mm<STRIDED, WS, 1>(v, j, nc, idx, c); break;
                case 2: mm += q_round_mm<STRIDED, WS, 2>(v, j, nc, idx, c); break;
                case 4: mm += q_round_mm<STRIDED, WS, 4>(v, j, nc, idx, c); break;
                default: mm += q_round_mm<STRIDED, WS, 8>(v, j, nc, idx, c); break;
                }
            }
            const bool alive = have && mm <= k;
            if (last) {
                if (alive)
                    q_record_dup(v, tl, e, mm);
            } else {
                const uint64_t m = __ballot(alive);
                if (alive) {
                    const int pos = n2 + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                             __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                    qb[pos] = make_uint2(idx, (ent.y & 0xFF00FFFFu) | ((uint32_t)min(mm, 255) << 16));
                }
                n2 += __popcll(m);
                WD_Q_CHECK(compact, n2, n2 <= n);
            }
        }
        q_wave_sync();
        uint2 *t = qa; qa = qb; qb = t;
        n = last ? 0 : n2;
        j += nb;
        nb = min(MAXB, nb * 2);
    }
    qn = 0;
}

// Push the lanes flagged `alive` (ballot m) behind the qn entries already queued.
__device__ inline void q_push(uint2 *q_a, int qn, uint64_t m, bool alive, uint32_t idx, uint32_t tag)
{
    if (alive) {
        const int pos = qn + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                 __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        q_a[pos] = make_uint2(idx, tag);
    }
}

__host__ __device__ inline int scan_q_lds_dwords(int levels, int tpb, int entry_dwords = 2)
{
    int n = (1 + 5 * levels) + tpb + tpb * (levels + 1) + tpb * levels + tpb + kMaxPasses * tpb + 4;
    n = (n + 3) & ~3;               // queue entries are 8- or 16-byte records
    return n + kWaves * 2 * kQCap * entry_dwords;
}

// ---- Levenshtein survivors: the banded-DP state travels with the queue entry ------------
// Entry = {well index, target << 24 | slot, state lo, state hi}.  State of LevState<H>, H <= 3
// (k <= 7, values <= 8): W = 2H+1 band cells of 4 bits, the last W well codes (3 bits each)
// and the last H+1 centre codes - 28 + 21 + 12 = 61 bits.
#ifndef WD_LEV_CELL_MASK
#define WD_LEV_CELL_MASK 15         // (a control build of tools/scan_lev_emu.cpp keeps three bits, to show that its test notices)
#endif
template <int H>
__device__ inline uint64_t lev_pack(const LevState<H> &s, uint64_t ch)
{
    constexpr int W = 2 * H + 1;
    uint64_t pk = 0;
#pragma unroll
    for (int d = 0; d < W; d++)
        pk |= (uint64_t)(s.r[d] & WD_LEV_CELL_MASK) << (4 * d);
    pk |= (s.wh & ((1ull << (3 * W)) - 1)) << 28;
    pk |= (ch & ((1ull << (3 * (H + 1))) - 1)) << 49;
    return pk;
}

template <int H>
__device__ inline void lev_unpack(uint64_t pk, LevState<H> &s, uint64_t &ch)
{
    constexpr int W = 2 * H + 1;
#pragma unroll
    for (int d = 0; d < W; d++)
        s.r[d] = (int)((pk >> (4 * d)) & 15);
    s.wh = (pk >> 28) & ((1ull << (3 * W)) - 1);
    ch = (pk >> 49) & ((1ull << (3 * (H + 1))) - 1);
}

// Drain for the Levenshtein family: rounds of 8 more cycles, one lane per survivor, state
// unpacked / advanced / re-packed; at L the remaining rows are finished and r[H] <= k decides.
template <bool STRIDED, int H, int WS = 1>
__device__ inline void q_drain_lev(const QEnv &v, uint4 *q_a, uint4 *q_b, int &qn, int j0, int lane)
{
    q_wave_sync();
    WD_Q_CHECK(drain, qn, qn >= 0 && qn <= kQCap);
    const int L = v.L, k = v.k, cap = v.k + 1;
    constexpr int NB = 8;
    int nb = WS == 4 ? 4 : 1;                          // cycles of the first drain round (then 2, 4, 8, 8 ...): most survivors of
                                                       // the first round die within two more cycles, and every cycle read is a line
    int j = min(j0, L);
    uint4 *qa = q_a, *qb = q_b;
    int n = qn;
    while (n > 0 && j < L) {
        const bool last = j + nb >= L;
        int n2 = 0;
        for (int p0 = 0; p0 < n; p0 += kWave) {
            const bool have = p0 + lane < n;
            uint4 ent = make_uint4(0u, 0u, 0u, 0u);
            if (have)
                ent = qa[p0 + lane];
            const uint32_t idx = ent.x;
            const int tl = (int)(ent.y >> 24);
            const int e = (int)(ent.y & 0xFFFFu);
            LevState<H> st;
            uint64_t ch;
            lev_unpack<H>(((uint64_t)ent.w << 32) | ent.z, st, ch);
            bool alive = false;
            if (have) {
                const uint32_t c = (uint32_t)v.s_centre[tl];
                uint32_t w[NB], cb[NB];
#pragma unroll
                for (int q = 0; q < NB; q++) {
                    if (q < nb) {
                        gbytes p = q_plane<STRIDED, WS>(v, min(j + q, L - 1));
                        w[q] = ldb(p, idx * WS);
                        cb[q] = ldb(p, c * WS);
                    }
                }
#pragma unroll
                for (int q = 0; q < NB; q++) {
                    if (q < nb && j + q < L) {
                        const uint32_t cc = code_of(cb[q]);
                        ch = (ch << 3) | cc;
                        st.push(j + q + 1, ch, cc, code_of(w[q]), L, cap);
                    }
                }
                if (last) {
                    st.finish(L, ch, cap, k);
                    if (st.dup(k))
                        q_record_dup(v, tl, e, st.dist());
                } else {
                    alive = st.alive(k, j + nb, ch, L, cap);
                }
            }
            if (!last) {
                const uint64_t m = __ballot(alive);
                if (alive) {
                    const int pos = n2 + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                             __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                    const uint64_t pk = lev_pack<H>(st, ch);
                    qb[pos] = make_uint4(idx, ent.y, (uint32_t)pk, (uint32_t)(pk >> 32));
                }
                n2 += __popcll(m);
                WD_Q_CHECK(compact, n2, n2 <= n);
            }
        }
        q_wave_sync();
        uint4 *t = qa; qa = qb; qb = t;
        n = last ? 0 : n2;
        j += nb;
        nb = min(NB, nb * 2);
    }
    qn = 0;
}

// ---- Levenshtein <= 2, closed form (lev2_stream.inc): the 12-bit state travels in the tag ----
// Entry = {well index, target << 24 | state << 12 | slot}: 8 bytes, as in the Hamming family.
// One lane per survivor; a round costs a dozen bit operations per 8 cycles.  Rounds of 1, 2, 4 more cycles while
// most survivors are random neighbours about to die (every cycle read is a line), then 8 at a time.  Interleaved
// layout: the rest of the group first (4 cycles, one dword), then 6 groups at a time - whoever is left is a
// duplicate and is read to its end anyway, and every round is a round trip at the end of the wave's life.
template <bool STRIDED, int WS = 1>
__device__ inline void q_drain_lev2(const QEnv &v, uint2 *q_a, uint2 *q_b, int &qn, int j0, int lane)
{
    q_wave_sync();
    WD_Q_CHECK(drain, qn, qn >= 0 && qn <= kQCap);
    const int L = v.L;
    constexpr int NB = WS == 4 ? 24 : 8;                                 // cycles of the longest round (planes: 16 would
                                                                         // spill registers in every kernel that drains)
    int nb = WS == 4 ? 4 : 1;
    int j = min(j0, L);
    uint2 *qa = q_a, *qb = q_b;
    int n = qn;
    while (n > 0 && j < L) {
        const bool last = j + nb >= L;
        int n2 = 0;
        for (int p0 = 0; p0 < n; p0 += kWave) {
            const bool have = p0 + lane < n;
            uint2 ent = make_uint2(0u, 0u);
            if (have)
                ent = qa[p0 + lane];
            const uint32_t idx = ent.x;
            const int tl = (int)(ent.y >> 24);
            uint32_t st = (ent.y >> 12) & 0xFFFu;
            bool alive = false;
            if (have) {
                const uint32_t c = (uint32_t)v.s_centre[tl];
                if constexpr (WS == 4) {
                    // j is a multiple of 4 here: whole dwords of four cycles (a short last group is cut by nc)
                    uint32_t da[NB / 4], db[NB / 4];
#pragma unroll
                    for (int g = 0; g < NB / 4; g++) {
                        if (4 * g < nb) {
                            const int64_t go = (int64_t)min((j >> 2) + g, max((L + 3) / 4 - 1, 0)) * v.stride;
                            db[g] = *(const __attribute__((address_space(1))) uint32_t *)(v.base0 + go + (size_t)idx * 4);
                            da[g] = *(const __attribute__((address_space(1))) uint32_t *)(v.base0 + go + (size_t)c * 4);
                        }
                    }
#pragma unroll
                    for (int h = 0; h < NB / 8; h++) {                   // 8 cycles (two groups) per step of the closed form
                        const int nc = min(min(nb, L - j) - 8 * h, 8);
                        if (nc > 0) {
                            const uint32_t wa = lev2_codes4(da[2 * h]) | (4 * (2 * h + 1) < nb ? lev2_codes4(da[2 * h + 1]) << 16 : 0u);
                            const uint32_t wb = lev2_codes4(db[2 * h]) | (4 * (2 * h + 1) < nb ? lev2_codes4(db[2 * h + 1]) << 16 : 0u);
                            st = lev2_step(st, wa, wb, nc);
                        }
                    }
                } else {
                    uint32_t w[NB], cb[NB];
#pragma unroll
                    for (int q = 0; q < NB; q++) {
                        if (q < nb) {
                            gbytes p = q_plane<STRIDED, WS>(v, min(j + q, L - 1));
                            w[q] = ldb(p, idx);
                            cb[q] = ldb(p, c);
                        }
                    }
#pragma unroll
                    for (int h = 0; h < NB / 8; h++) {
                        const int nc = min(min(nb, L - j) - 8 * h, 8);
                        if (nc > 0) {
                            uint32_t wa = 0, wb = 0;
#pragma unroll
                            for (int q = 0; q < 8; q++) {
                                if (8 * h + q < nb) {
                                    wa |= lev2_code(cb[8 * h + q]) << (4 * q);
                                    wb |= lev2_code(w[8 * h + q]) << (4 * q);
                                }
                            }
                            st = lev2_step(st, wa, wb, nc);
                        }
                    }
                }
                alive = lev2_alive(st);
                if (last && alive)
                    q_record_dup(v, tl, (int)(ent.y & 0xFFFu), lev2_dist(st));
            }
            if (!last) {
                const uint64_t m = __ballot(alive);
                if (alive) {
                    const int pos = n2 + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                             __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                    qb[pos] = make_uint2(idx, (ent.y & 0xFF000FFFu) | (st << 12));
                }
                n2 += __popcll(m);
                WD_Q_CHECK(compact, n2, n2 <= n);
            }
        }
        q_wave_sync();
        uint2 *t = qa; qa = qb; qb = t;
        n = last ? 0 : n2;
        j += nb;
        nb = WS == 4 ? NB : (nb < 4 ? nb * 2 : NB);
    }
    qn = 0;
}

// LEVH = 0: equality / Hamming (mismatch count in the entry's tag).  LEVH = 1..3: Levenshtein
// <= k with band half-width LEVH, banded-DP state in the entry (k = 3 .. 7, and k = 2 on request).
// LEVH = kLev2Closed: Levenshtein <= 2 - the reference's default `-e 2` - by the streaming closed
// form of lev2_stream.inc: no DP anywhere, 12 bits of state in the tag.
constexpr int kLev2Closed = -1;
template <bool STRIDED, int B1, int LEVH = 0, int WS = 1>
__global__ __launch_bounds__(kBlock, LEVH > 0 ? 4 : (WS == 4 ? WD_Q_OCC_IL : 6)) void k_scan_q(ScanArgs a)
{
    static_assert(WS == 1 || (WS == 4 && STRIDED && ((B1 == 4 && LEVH == 0) || (B1 == 8 && (LEVH == 1 || LEVH == kLev2Closed)))),
                  "the interleaved layout is read a dword (4 cycles) at a time: one for equality / Hamming, "
                  "two for the first round of Levenshtein <= 2 / <= 3");
    using Entry = typename std::conditional<LEVH <= 0, uint2, uint4>::type;
    using LevS = LevState<(LEVH > 0 ? LEVH : 1)>;
    WD_DYNAMIC_LDS(smem);
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int levels = a.levels;
    const int L = a.L;
    const int k = a.k;
    const int tpb = a.tpb;
    const int ncnt = 1 + 5 * levels;
    const int chunks = (a.T + tpb - 1) / tpb;
    // Workgroup b runs on XCD b % 8.  The (tile, chunk) pairs are dealt out so that every XCD walks a
    // contiguous stretch of them: the chunks of a tile - neighbouring bands of wells once the targets are
    // sorted by centre - then follow each other through ONE L2, and a line two of them touch is fetched
    // from HBM once.  (Round-robin, chunk c and chunk c + 1 sat on different dies.)
    const int nb = (int)gridDim.x, per_xcd = (nb + kXcds - 1) / kXcds;
    int vb = (int)(blockIdx.x % kXcds) * per_xcd + (int)(blockIdx.x / kXcds);
    if (nb % kXcds) {                // a ragged grid: the dies that come first take one block more
        const int big = nb % kXcds, x = (int)(blockIdx.x % kXcds), small = nb / kXcds;
        vb = (x < big ? x * (small + 1) : big * (small + 1) + (x - big) * small) + (int)(blockIdx.x / kXcds);
    }
    const int tile = vb / chunks;
    const int chunk = vb - tile * chunks;
    const int t_first = chunk * tpb;
    const int n_t = min(tpb, a.T - t_first);

    uint32_t *s_cnt = smem;
    int32_t *s_centre = (int32_t *)(s_cnt + ncnt);
    int32_t *s_off = s_centre + tpb;
    uint32_t *s_d = (uint32_t *)(s_off + tpb * (levels + 1));
    uint32_t *s_valid = s_d + tpb * levels;
    uint32_t *s_items = s_valid + tpb;
    uint32_t *s_misc = s_items + kMaxPasses * tpb;
    const int q_base = (int)((((s_misc + 4) - smem) + 3) & ~3);
    Entry *q_a = (Entry *)(smem + q_base) + wave * 2 * kQCap;
    Entry *q_b = q_a + kQCap;

    gbytes filt = as_global(a.filter[tile]);
    const uint8_t *const *ptab = STRIDED ? nullptr : a.planes + (size_t)tile * L;
    gbytes base0 = STRIDED ? as_global(a.planes[tile]) : nullptr;
    const int64_t stride = a.stride;
    auto plane_ptr = [&](int j) -> gbytes {
        if (WS == 4)
            return base0 + (int64_t)(j >> 2) * stride + (j & 3);
        return STRIDED ? base0 + (int64_t)j * stride : as_global(ptab[j]);
    };
    const int cap = k + 1;

    // ---------------- phase 0: metadata, filter bytes, work items ----------------
    for (int i = threadIdx.x; i < ncnt; i += kBlock)
        s_cnt[i] = 0;
    for (int i = threadIdx.x; i < n_t * levels; i += kBlock)
        s_d[i] = 0;
    for (int i = threadIdx.x; i < n_t; i += kBlock)
        s_centre[i] = a.centre[t_first + i];
    for (int i = threadIdx.x; i < n_t * (levels + 1); i += kBlock)
        s_off[i] = a.lvl_off[(size_t)t_first * (levels + 1) + i];
    __syncthreads();
    if (wave == 0) {
        const bool in = lane < n_t;
        const int32_t *o = s_off + (in ? lane : 0) * (levels + 1);
        const uint32_t c = in ? (uint32_t)s_centre[lane] : 0u;
        const uint32_t fb = in ? (uint32_t)filt[c] : 0u;
        bool valid = in && (fb & 1u);                          // :236-237
        if (a.check_empty && valid) {                           // :249
            bool empty = false;
            for (int l = 0; l < levels; l++)
                empty = empty || (o[l + 1] <= o[l]);
            if (empty) {
                g_atomic_or(as_gptr(WD_LATE_ARG(rare))->status, kStatusEmptyLevel);
                valid = false;
            }
        }
        const int K = in ? o[levels] - o[0] : 0;
        const int np = valid ? (K + kPass - 1) / kPass : 0;
        int incl = np;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int v = __shfl_up(incl, d);
            if (lane >= d)
                incl += v;
        }
        if (in)
            s_valid[lane] = valid ? 1u : 0u;
        for (int p = 0; p < np; p++)
            s_items[incl - np + p] = ((uint32_t)lane << 8) | (uint32_t)p;
        if (lane == kWave - 1)
            s_misc[0] = (uint32_t)incl;
    }
    __syncthreads();

    QEnv env;
    env.s_centre = s_centre;
    env.s_off = s_off;
    env.s_d = s_d;
    env.s_tid = nullptr;
    env.base0 = base0;
    env.ptab = ptab;
    env.stride = stride;
    env.levels = levels;
    env.L = L;
    env.k = k;
    env.tile = tile;
    env.t_first = t_first;
    int qn = 0;

    // ---------------- phase 1: pipelined first round over this wave's items -----------------
    const int nitems = (int)s_misc[0];
    const int n_my = nitems > wave ? (nitems - wave + kWaves - 1) / kWaves : 0;
    if (n_my > 0) {
        // plane pointers of the first round (clamped: cycles >= L are masked out below)
        gbytes pp[B1];
#pragma unroll
        for (int q = 0; q < B1; q++)
            pp[q] = plane_ptr(min(q, max(L - 1, 0)));

        // item registers by age: 0 = indices being loaded, 2 = plane bytes being asked for, AGE = being consumed
        // (kQDepth steps between the issue of an item's gather and its use.  Measured in round 4: neither a
        // deeper pipeline nor a static ring of register sets - the loop unrolled AGE + 1 times so that no value
        // moves between registers while its load is in flight - makes a lane faster: a step costs 0.75 us
        // whatever the depth, and a workgroup's life is as much its prologue and its last drain as its steps)
        constexpr int AGE = 2 + kQDepth;
        constexpr int NW = WS == 4 ? B1 / 4 : B1;               // registers of one slot's first round
        constexpr int SB = 2;
        uint32_t it[AGE + 1], i0[AGE + 1], i1[AGE + 1];
        uint32_t w0[AGE + 1][NW], w1[AGE + 1][NW];
#pragma unroll
        for (int g = 0; g <= AGE; g++) {
            it[g] = i0[g] = i1[g] = 0;
#pragma unroll
            for (int q = 0; q < NW; q++)
                w0[g][q] = w1[g][q] = 0;
        }
        uint32_t &it3 = it[AGE], &i0_3 = i0[AGE], &i1_3 = i1[AGE];
        uint32_t (&w0_3)[NW] = w0[AGE], (&w1_3)[NW] = w1[AGE];
        uint32_t &i0_2 = i0[2], &i1_2 = i1[2], &it0 = it[0], &i0_0 = i0[0], &i1_0 = i1[0];
        uint32_t (&w0_2)[NW] = w0[2], (&w1_2)[NW] = w1[2];

        for (int s = 0; s < n_my + AGE; s++) {
            // rotate ages
#pragma unroll
            for (int g = AGE; g > 0; g--) {
                it[g] = it[g - 1];
                i0[g] = i0[g - 1];
                i1[g] = i1[g - 1];
            }
#pragma unroll
            for (int g = AGE; g > 2; g--) {
#pragma unroll
                for (int q = 0; q < NW; q++) {
                    w0[g][q] = w0[g - 1][q];
                    w1[g][q] = w1[g - 1][q];
                }
            }

            // stage A: neighbour indices of item s (clamped to the wave's last item).  FIRST in program order:
            // loads come back in the order they were issued, and stage B waits for the indices of item s-2 -
            // issued before that step's gather, so the wait leaves the gathers of the last steps in flight
            // (with the gather ahead of the index loads every step waited for the gather of the step before)
            {
                it0 = s_items[wave + kWaves * min(s, n_my - 1)];
                const int tl = (int)(it0 >> 8);
                const int base = (int)(it0 & 0xFFu) * kPass;
                const int off0 = __builtin_amdgcn_readfirstlane(s_off[tl * (levels + 1)]);
                const int K = __builtin_amdgcn_readfirstlane(s_off[tl * (levels + 1) + levels]) - off0;
                const int e0 = base + lane, e1 = e0 + kWave;
                // (loads are unconditional - clamped slot - so that the number of loads per step is static, and
                // NOTHING reads their results in this step: a select between the loaded index and the centre
                // here made the wave wait for the load it had just issued, and for every gather before it.
                // Idle lanes read the target's last neighbour once more - masked out at the compare - and lane
                // 63 of the second slot becomes the centre well where the index is used, in stage B)
                i0_0 = (uint32_t)a.nbr[off0 + min(e0, K - 1)];
                i1_0 = (uint32_t)a.nbr[off0 + min(e1, K - 1)];
            }
            // stage B: plane bytes of item s-2 (its indices were requested two steps ago)
            // lane 63 of the second slot shadows the centre well: its byte comes out of the same load as the
            // neighbours' (the queue and the in-place finish take the slot's index from here, too)
            if (lane == kWave - 1)
                i1_2 = (uint32_t)s_centre[it[SB] >> 8];
            if (WS == 4) {
                // interleaved layout: the first four cycles of a well are one aligned dword
                // (kept whole until stage C: taking the bytes apart here would wait for the load)
#pragma unroll
                for (int g = 0; g < B1 / 4; g++) {
                    const int64_t go = (int64_t)min(g, max((L + 3) / 4 - 1, 0)) * stride;      // (short reads have fewer groups)
                    w0_2[g] = *(const __attribute__((address_space(1))) uint32_t *)(base0 + go + (size_t)i0_2 * 4);
                    w1_2[g] = *(const __attribute__((address_space(1))) uint32_t *)(base0 + go + (size_t)i1_2 * 4);
                }
            } else if (L > 0) {
#pragma unroll
                for (int q = 0; q < B1; q++) {
                    w0_2[q] = ldb(pp[q], i0_2);
                    w1_2[q] = ldb(pp[q], i1_2);
                }
            }
            // stage C: consume the item of age AGE
            if (s >= AGE) {
                const int tl = (int)(it3 >> 8);
                const int base = (int)(it3 & 0xFFu) * kPass;
                const int off0 = __builtin_amdgcn_readfirstlane(s_off[tl * (levels + 1)]);
                const int K = __builtin_amdgcn_readfirstlane(s_off[tl * (levels + 1) + levels]) - off0;
                const int e0 = base + lane, e1 = e0 + kWave;
                const bool a0 = e0 < K, a1 = lane < kWave - 1 && e1 < K;
                if constexpr (LEVH == 0) {
                    int mm0 = 0, mm1 = 0;
                    if constexpr (WS == 4) {
                        // the dword at once: the four cycles' codes side by side (lev2_codes4: six operations), the
                        // centre's on the scalar side - byte by byte this compare was sixty vector instructions of a
                        // step's hundred and seventy, on a machine that takes four clocks per vector instruction
                        static_assert(B1 == 4, "one dword is the first round");
                        const uint32_t cw = lev2_codes4((uint32_t)__builtin_amdgcn_readlane((int)w1_3[0], kWave - 1));
                        const uint32_t keep = L >= 4 ? (kLev2Nib & 0xFFFFu) : (((1u << (4 * L)) - 1u) & kLev2Nib);
                        const uint32_t y0 = lev2_codes4(w0_3[0]) ^ cw, y1 = lev2_codes4(w1_3[0]) ^ cw;
                        mm0 = __popc((y0 | (y0 >> 1) | (y0 >> 2)) & keep);
                        mm1 = __popc((y1 | (y1 >> 1) | (y1 >> 2)) & keep);
                    } else {
#pragma unroll
                        for (int q = 0; q < B1; q++) {
                            if (q < L) {
                                const uint32_t cc = code_of((uint32_t)__builtin_amdgcn_readlane((int)w1_3[q], kWave - 1));
                                mm0 += code_of(w0_3[q]) != cc ? 1 : 0;
                                mm1 += code_of(w1_3[q]) != cc ? 1 : 0;
                            }
                        }
                    }
                    const bool al0 = a0 && mm0 <= k, al1 = a1 && mm1 <= k;
                    const uint64_t m0 = __ballot(al0), m1 = __ballot(al1);
                    if (m0 | m1) {
                        if (B1 >= L) {
                            if (al0)
                                q_record_dup(env, tl, e0, mm0);
                            if (al1)
                                q_record_dup(env, tl, e1, mm1);
                        } else {
                            const int n0 = __popcll(m0), n1 = __popcll(m1);
                            if (n0 + n1 >= kFinishInPlace) {
                                WD_Q_CHECK(in_place, n0 + n1, n0 + n1 <= kPass);
                                // A third of the pass still alive after the first round: reads of low diversity.
                                // Through the queue every survivor would fetch its centre's byte beside its own,
                                // cycle after cycle (twice the loads of the first round's scheme, where the centre
                                // rides in lane 63 of the second slot) - this pass is finished where it stands.
                                bool x0 = al0, x1 = al1;
                                if constexpr (WS == 4) {
                                    // (interleaved layout: a dword = four cycles of a well; B1 is a multiple of 4)
                                    for (int j = B1; j < L && (__ballot(x0) | __ballot(x1)); j += 4) {
                                        const int64_t go = (int64_t)(j >> 2) * stride;
                                        const uint32_t d0 = *(const __attribute__((address_space(1))) uint32_t *)(base0 + go + (size_t)i0_3 * 4);
                                        const uint32_t d1 = *(const __attribute__((address_space(1))) uint32_t *)(base0 + go + (size_t)i1_3 * 4);
                                        const uint32_t c0w = lev2_codes4(d0), c1w = lev2_codes4(d1);
                                        const uint32_t caw = (uint32_t)__builtin_amdgcn_readlane((int)c1w, kWave - 1);
                                        const int ncy = min(4, L - j);
                                        const uint32_t keep = ((1u << (4 * ncy)) - 1u) & kLev2Nib;
                                        const uint32_t y0 = caw ^ c0w, y1 = caw ^ c1w;
                                        mm0 += __popc((y0 | (y0 >> 1) | (y0 >> 2)) & keep);
                                        mm1 += __popc((y1 | (y1 >> 1) | (y1 >> 2)) & keep);
                                        x0 = x0 && mm0 <= k;
                                        x1 = x1 && mm1 <= k;
                                    }
                                }
                                for (int j = B1; WS == 1 && j < L && (__ballot(x0) | __ballot(x1)); j += 4) {
                                    uint32_t u0[4], u1[4];
#pragma unroll
                                    for (int q = 0; q < 4; q++) {
                                        gbytes p = plane_ptr(min(j + q, L - 1));
                                        u0[q] = ldb(p, i0_3);
                                        u1[q] = ldb(p, i1_3);
                                    }
#pragma unroll
                                    for (int q = 0; q < 4; q++) {
                                        if (j + q < L) {
                                            const uint32_t cc = code_of((uint32_t)__builtin_amdgcn_readlane((int)u1[q], kWave - 1));
                                            mm0 += code_of(u0[q]) != cc ? 1 : 0;
                                            mm1 += code_of(u1[q]) != cc ? 1 : 0;
                                        }
                                    }
                                    x0 = x0 && mm0 <= k;
                                    x1 = x1 && mm1 <= k;
                                }
                                if (x0)
                                    q_record_dup(env, tl, e0, mm0);
                                if (x1)
                                    q_record_dup(env, tl, e1, mm1);
                                continue;
                            }
                            if (qn + n0 + n1 > kQCap) {
                                WD_Q_CHECK(drain_mid, qn, qn <= kQCap);
                                q_drain<STRIDED, 8, WS>(env, (uint2 *)q_a, (uint2 *)q_b, qn, B1, lane);
                            }
                            WD_Q_CHECK(push, qn + n0 + n1, qn + n0 + n1 <= kQCap);
                            q_push((uint2 *)q_a, qn, m0, al0, i0_3,
                                   ((uint32_t)tl << 24) | ((uint32_t)min(mm0, 255) << 16) | (uint32_t)e0);
                            q_push((uint2 *)q_a, qn + n0, m1, al1, i1_3,
                                   ((uint32_t)tl << 24) | ((uint32_t)min(mm1, 255) << 16) | (uint32_t)e1);
                            qn += n0 + n1;
                        }
                    }
                } else if constexpr (LEVH == kLev2Closed) {
                    // codes of the round's cycles, 4 bits each; lane 63 of the second slot holds the centre
                    uint32_t wb0 = 0, wb1 = 0;
                    if constexpr (WS == 4) {
                        wb0 = lev2_codes4(w0_3[0]) | (lev2_codes4(w0_3[1]) << 16);
                        wb1 = lev2_codes4(w1_3[0]) | (lev2_codes4(w1_3[1]) << 16);
                    } else {
#pragma unroll
                        for (int q = 0; q < B1; q++) {
                            wb0 |= lev2_code(w0_3[q]) << (4 * q);
                            wb1 |= lev2_code(w1_3[q]) << (4 * q);
                        }
                    }
                    const uint32_t wa = (uint32_t)__builtin_amdgcn_readlane((int)wb1, kWave - 1);
                    const int nc = min(B1, L);
                    const uint32_t st0 = lev2_step(lev2_init(), wa, wb0, nc), st1 = lev2_step(lev2_init(), wa, wb1, nc);
                    const bool al0 = a0 && lev2_alive(st0), al1 = a1 && lev2_alive(st1);
                    const uint64_t m0 = __ballot(al0), m1 = __ballot(al1);
                    if (m0 | m1) {
                        if (B1 >= L) {
                            if (al0)
                                q_record_dup(env, tl, e0, lev2_dist(st0));
                            if (al1)
                                q_record_dup(env, tl, e1, lev2_dist(st1));
                        } else {
                            const int n0 = __popcll(m0), n1 = __popcll(m1);
                            if (WS == 1 && n0 + n1 >= kFinishInPlace) {
                                WD_Q_CHECK(in_place, n0 + n1, n0 + n1 <= kPass);
                                // (low diversity: the pass is finished where it stands, as in the Hamming family.
                                // Not in the interleaved layout: there the queue's rounds of two dwords per entry
                                // are the better deal - measured, every read equal: 19.5 us per tile through the
                                // queue, 24.6 in place)
                                uint32_t s0 = st0, s1 = st1;
                                bool x0 = al0, x1 = al1;
                                for (int j = B1; j < L && (__ballot(x0) | __ballot(x1)); j += 4) {
                                    uint32_t u0[4], u1[4];
#pragma unroll
                                    for (int q = 0; q < 4; q++) {
                                        gbytes p = plane_ptr(min(j + q, L - 1));
                                        u0[q] = ldb(p, i0_3);
                                        u1[q] = ldb(p, i1_3);
                                    }
                                    uint32_t c0w = 0, c1w = 0;
#pragma unroll
                                    for (int q = 0; q < 4; q++) {
                                        c0w |= lev2_code(u0[q]) << (4 * q);
                                        c1w |= lev2_code(u1[q]) << (4 * q);
                                    }
                                    const uint32_t caw = (uint32_t)__builtin_amdgcn_readlane((int)c1w, kWave - 1);
                                    const int ncy = min(4, L - j);
                                    s0 = lev2_step(s0, caw, c0w, ncy);
                                    s1 = lev2_step(s1, caw, c1w, ncy);
                                    x0 = x0 && lev2_alive(s0);
                                    x1 = x1 && lev2_alive(s1);
                                }
                                if (x0)
                                    q_record_dup(env, tl, e0, lev2_dist(s0));
                                if (x1)
                                    q_record_dup(env, tl, e1, lev2_dist(s1));
                                continue;
                            }
                            if (qn + n0 + n1 > kQCap) {
                                WD_Q_CHECK(drain_mid, qn, qn <= kQCap);
                                q_drain_lev2<STRIDED, WS>(env, (uint2 *)q_a, (uint2 *)q_b, qn, B1, lane);
                            }
                            WD_Q_CHECK(push, qn + n0 + n1, qn + n0 + n1 <= kQCap);
                            q_push((uint2 *)q_a, qn, m0, al0, i0_3, ((uint32_t)tl << 24) | (st0 << 12) | (uint32_t)e0);
                            q_push((uint2 *)q_a, qn + n0, m1, al1, i1_3, ((uint32_t)tl << 24) | (st1 << 12) | (uint32_t)e1);
                            qn += n0 + n1;
                        }
                    }
                } else {
                    LevS s0, s1;
                    s0.init(cap);
                    s1.init(cap);
                    uint64_t ch = ~0ull;
#pragma unroll
                    for (int q = 0; q < B1; q++) {
                        if (q < L) {
                            // interleaved: cycle q of a well is byte q % 4 of its dword q / 4
                            const uint32_t cb = WS == 4 ? ((uint32_t)__builtin_amdgcn_readlane((int)w1_3[WS == 4 ? q >> 2 : 0], kWave - 1) >> (8 * (q & 3))) & 0xFFu
                                                        : (uint32_t)__builtin_amdgcn_readlane((int)w1_3[WS == 4 ? 0 : q], kWave - 1);
                            const uint32_t b0 = WS == 4 ? (w0_3[WS == 4 ? q >> 2 : 0] >> (8 * (q & 3))) & 0xFFu : w0_3[WS == 4 ? 0 : q];
                            const uint32_t b1 = WS == 4 ? (w1_3[WS == 4 ? q >> 2 : 0] >> (8 * (q & 3))) & 0xFFu : w1_3[WS == 4 ? 0 : q];
                            const uint32_t cc = code_of(cb);
                            ch = (ch << 3) | cc;
                            s0.push(q + 1, ch, cc, code_of(b0), L, cap);
                            s1.push(q + 1, ch, cc, code_of(b1), L, cap);
                        }
                    }
                    if (B1 >= L) {                      // whole read seen: finish the last rows
                        s0.finish(L, ch, cap, k);
                        s1.finish(L, ch, cap, k);
                        if (a0 && s0.dup(k))
                            q_record_dup(env, tl, e0, s0.dist());
                        if (a1 && s1.dup(k))
                            q_record_dup(env, tl, e1, s1.dist());
                    } else {
                        const bool al0 = a0 && s0.alive(k, B1, ch, L, cap);
                        const bool al1 = a1 && s1.alive(k, B1, ch, L, cap);
                        const uint64_t m0 = __ballot(al0), m1 = __ballot(al1);
                        if (m0 | m1) {
                            const int n0 = __popcll(m0), n1 = __popcll(m1);
                            if (qn + n0 + n1 > kQCap) {
                                WD_Q_CHECK(drain_mid, qn, qn <= kQCap);
                                q_drain_lev<STRIDED, (LEVH > 0 ? LEVH : 1), WS>(env, (uint4 *)q_a, (uint4 *)q_b, qn, B1, lane);
                            }
                            WD_Q_CHECK(push, qn + n0 + n1, qn + n0 + n1 <= kQCap);
                            if (al0) {
                                const int pos = qn + __builtin_amdgcn_mbcnt_hi((uint32_t)(m0 >> 32),
                                                         __builtin_amdgcn_mbcnt_lo((uint32_t)m0, 0u));
                                const uint64_t pk = lev_pack(s0, ch);
                                ((uint4 *)q_a)[pos] = make_uint4(i0_3, ((uint32_t)tl << 24) | (uint32_t)e0,
                                                                 (uint32_t)pk, (uint32_t)(pk >> 32));
                            }
                            if (al1) {
                                const int pos = qn + n0 + __builtin_amdgcn_mbcnt_hi((uint32_t)(m1 >> 32),
                                                              __builtin_amdgcn_mbcnt_lo((uint32_t)m1, 0u));
                                const uint64_t pk = lev_pack(s1, ch);
                                ((uint4 *)q_a)[pos] = make_uint4(i1_3, ((uint32_t)tl << 24) | (uint32_t)e1,
                                                                 (uint32_t)pk, (uint32_t)(pk >> 32));
                            }
                            qn += n0 + n1;
                        }
                    }
                }
            }
        }
        if (qn > 0) {
            if constexpr (LEVH == 0)
                q_drain<STRIDED, 8, WS>(env, (uint2 *)q_a, (uint2 *)q_b, qn, B1, lane);
            else if constexpr (LEVH == kLev2Closed)
                q_drain_lev2<STRIDED, WS>(env, (uint2 *)q_a, (uint2 *)q_b, qn, B1, lane);
            else
                q_drain_lev<STRIDED, LEVH, WS>(env, (uint4 *)q_a, (uint4 *)q_b, qn, B1, lane);
        }
    }
    __syncthreads();

    // ---------------- phase 3: tallies (count_well_duplicates.py:80-95 as histograms) -------
    uint32_t acc_wells = 0, acc_dups = 0, acc_hit = 0, acc_first = 0, acc_last = 0, acc_valid = 0;
    gptr<uint32_t> const out_pt = as_gptr(WD_LATE_ARG(out_per_target));
    gptr<const int32_t> const perm = out_pt ? as_gptr(WD_LATE_ARG(perm)) : nullptr;
    const size_t T_all = (size_t)WD_LATE_ARG(T);
    for (int tl = wave; tl < n_t; tl += kWaves) {
        const bool valid = __builtin_amdgcn_readfirstlane(s_valid[tl]) != 0;
        gptr<uint32_t> opt = out_pt ? out_pt + ((size_t)tile * T_all + (perm ? perm[t_first + tl] : t_first + tl)) * levels
                                    : nullptr;
        if (!valid) {
            if (opt && lane < levels)
                opt[lane] = WD_INVALID_TARGET;
            continue;
        }
        uint32_t my_d = 0, my_w = 0;
        if (lane < levels) {
            my_d = s_d[tl * levels + lane];
            my_w = (uint32_t)(s_off[tl * (levels + 1) + lane + 1] - s_off[tl * (levels + 1) + lane]);
        }
        const uint64_t hm = __ballot(lane < levels && my_d > 0);
        acc_valid += 1;
        acc_wells += my_w;
        acc_dups += my_d;
        acc_hit += my_d ? 1u : 0u;
        if (hm) {
            acc_first += (lane == __ffsll((long long)hm) - 1) ? 1u : 0u;
            acc_last += (lane == 63 - __clzll((long long)hm)) ? 1u : 0u;
        }
        if (opt && lane < levels)
            opt[lane] = my_d;
    }
    if (lane < levels) {
        if (acc_wells) atomicAdd(&s_cnt[1 + lane], acc_wells);
        if (acc_dups) atomicAdd(&s_cnt[1 + levels + lane], acc_dups);
        if (acc_hit) atomicAdd(&s_cnt[1 + 2 * levels + lane], acc_hit);
        if (acc_first) atomicAdd(&s_cnt[1 + 3 * levels + lane], acc_first);
        if (acc_last) atomicAdd(&s_cnt[1 + 4 * levels + lane], acc_last);
    }
    if (lane == 0 && acc_valid)
        atomicAdd(&s_cnt[0], acc_valid);
    __syncthreads();
    unsigned long long *const out_tile = WD_LATE_ARG(out_tile);
    for (int i = threadIdx.x; i < ncnt; i += kBlock) {
        const uint32_t v = s_cnt[i];
        if (v)
            g_atomic_add(&out_tile[(size_t)tile * ncnt + i], (unsigned long long)v);
    }
}

