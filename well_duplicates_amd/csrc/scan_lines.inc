// scan_lines.inc - the line walk: the (target, slot) pairs of a sampled targets set, taken in the order
// of their NEIGHBOUR wells.  Included by welldup.hip after scan_queue.inc (it reuses the survivor queue).
// -------------------------------------------------------------------------------------
// k_scan_q walks target by target: a wave loads the ~86 neighbours of one target, and a cache line two
// targets' neighbourhoods share is asked for twice - the sorted walk (install_sorted_view) makes the
// second request an L2 hit when it comes soon enough.  On a dense sampled set (BASELINE configs[3]:
// 10 000 targets x 163 neighbours on 4.09 M wells) every line is wanted by three or four targets and
// half of those repeats still go to the fabric.
// Here the unit of work is the pair, and the pairs are sorted by neighbour well (a tile-independent
// index: build_line_tables, once per targets set).  Consecutive lanes read consecutive wells, so a line is
// asked for by ONE wave-load per cycle however many targets want it, and a pair costs a fraction of the
// instructions (no per-target item pipeline: two index loads and B1 byte loads per 128 pairs).
//   phase 0  a block (a run of <= kLwPairs pairs that involve <= kLwTargets targets) stages what it needs
//            of its targets in LDS: centre well, ring offsets, filter bit, and the centre's codes of the
//            first B1 cycles as one word of 4-bit fields (lev2_code);
//   phase 1  each wave streams over its share of the pairs, two per lane and step, software-pipelined
//            (indices two steps ahead, plane bytes one step ahead, every load unconditional: pairs of
//            targets whose centre fails the filter read the block's first well instead); survivors of
//            the first B1 cycles go to the wave's LDS queue in k_scan_q's entry format;
//   phase 2  q_drain / q_drain_lev2 as in k_scan_q (the queue does not care where its entries came from);
//   phase 3  a target's pairs lie in several blocks, so its per-level duplicate counts are partial here:
//            Dups are added as they are; Hit / first / last follow from the target's hit-level mask in
//            global memory, each transition of which is applied once (as in the dense path:
//            dense_record) - the block whose pairs include a target's first pair also counts it as a
//            valid target and adds its ring sizes to Wells.
constexpr int kLwTargets = 256;       // targets per block at most: the queue entry's tag holds 8 bits
constexpr int kLwPairs = 12288;       // pairs per block, by default (the first round has to amortise the prologue and the last
                                      // drain; measured on the configs[3] shape: 8192 .. 16384 within 3 %, 4096 and 32768 worse)
constexpr int kLwStep = 2 * kWave;    // pairs per wave and step
constexpr int kLwQCap = 128;          // survivor queue entries per wave (>= kLwStep: after a drain one step's survivors always fit)
constexpr int kLwInPlace = 43;        // survivors of a step's first round (of its 128 pairs) from which the step is finished where it stands
static_assert(kLwQCap >= kLwStep && kLwQCap >= kFinishAllMax,
              "after a drain one step must fit the queue, and q_finish_all adds up its pieces in the idle queue buffer");

// (ScanArgs first: the survivor queue's rare paths fetch `rare`, `perm` and `log_hits` from the kernel
// argument segment at ScanArgs' offsets - late_arg, scan_queue.inc)
struct LineArgs {
    ScanArgs s;                     // planes, filter, stride, centre / lvl_off (file order), out_tile, out_per_target
                                    // (zeroed by the launcher), rare, perm = null, T, levels, L, k, log_hits
    const int32_t *pw;              // [P] neighbour well of every (target, slot) pair, ascending
    const uint32_t *pm;             // [P] target within the block << 16 | slot
    const int4 *blk;                // [n_blk] {first pair, pairs, first entry of btgt, targets}
    const uint32_t *btgt;           // the blocks' targets: index in the file | (this block holds its first pair) << 31
    const int32_t *bcen;            // ... and their centre wells (one dependent load less in the prologue)
    const int32_t *boff;            // ... and their ring offsets, levels + 1 per entry (rows of lvl_off, block by block)
    uint32_t *mask;                 // [n_tiles][mask_stride]: hit-level mask, 8 bits per target (zeroed by the launcher)
    long long mask_stride;
    int n_blk;
    int tmax;                       // most targets of any block (a multiple of 4): what the LDS tables are sized for
};
static_assert(offsetof(LineArgs, s) == 0, "the queue's late arguments are read at ScanArgs' offsets");

__host__ __device__ inline int scan_lines_lds_dwords(int levels, int tmax)
{
    int n = (1 + 5 * levels) + tmax * (1 + (levels + 1) + levels + 1 + 1 + 1) + 4;
    n = (n + 3) & ~3;
    return n + kWaves * 2 * kLwQCap * 2;
}

// sum over the wave's lanes, wave-uniform (an inclusive scan inside each row of 16 lanes by DPP shifts, then
// the row sums handed on with row_bcast)
__device__ inline uint32_t lw_wave_sum(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);     // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);     // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);     // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);     // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);    // row_bcast:15 into rows 1 and 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);    // row_bcast:31 into rows 2 and 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, kWave - 1);
}

// LEVH = 0: equality / Hamming <= k; kLev2Closed: Levenshtein <= 2 (lev2_stream.inc).  B1 <= 8.
// WS = 4: the interleaved layout ([group of 4 cycles][well][4 bytes], scan_queue.inc: q_plane) - a pair's
// first round is one dword (B1 = 4) or two (B1 = 8), and a line of 32 wells x 4 cycles is asked for once per
// GROUP instead of a line of 128 wells once per cycle.
template <bool STRIDED, int B1, int LEVH, int WS = 1>
// (waves per SIMD the register budget is cut for: interleaved equality / Hamming - 67 registers - gains 6 % at seven,
// the closed form loses 7 % there; measured on the configs[3] shape)
__global__ __launch_bounds__(kBlock, (WS == 4 && LEVH == 0) ? 7 :
                                     LEVH == 0 && B1 <= 6 && STRIDED ? 6 : (LEVH == 0 && B1 == 8 && WS == 1 ? 4 : 5))
void k_scan_lines(LineArgs a)
{
    static_assert(B1 >= 1 && B1 <= 8, "the centre's first-round codes are one word of 4-bit fields");
    static_assert(LEVH == 0 || LEVH == kLev2Closed, "equality / Hamming, or Levenshtein <= 2 by the closed form");
    static_assert(WS == 1 || (WS == 4 && STRIDED && (B1 == 4 || B1 == 8)), "interleaved: whole dwords of four cycles");
    constexpr int NLD = WS == 4 ? B1 / 4 : B1;               // loads per pair of the first round
    WD_DYNAMIC_LDS(smem);                                    // (device_common.inc: a heap block of the launch's bytes in the CPU emulation)
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int levels = a.s.levels, L = a.s.L, k = a.s.k;
    const int ncnt = 1 + 5 * levels;
    // workgroup b runs on XCD b % 8: every XCD walks a contiguous stretch of (block, tile) pairs
    const int nb = (int)gridDim.x, per_xcd = (nb + kXcds - 1) / kXcds;
    int vb = (int)(blockIdx.x % kXcds) * per_xcd + (int)(blockIdx.x / kXcds);
    if (nb % kXcds) {
        const int big = nb % kXcds, x = (int)(blockIdx.x % kXcds), small = nb / kXcds;
        vb = (x < big ? x * (small + 1) : big * (small + 1) + (x - big) * small) + (int)(blockIdx.x / kXcds);
    }
    // tile fastest: a block's slice of the pair tables (8 bytes per pair) is read for every tile - walked
    // tile by tile the whole table, 13 MB on the configs[3] shape, came out of HBM again for each of them
    // (a third of the kernel's line fetches); walked block by block the slice stays in the XCD's L2
    const int n_tiles = nb / a.n_blk;
    const int bi = vb / n_tiles;
    const int tile = vb - bi * n_tiles;
    const int4 bd = a.blk[bi];
    const int p0 = bd.x, np = bd.y, n_t = bd.w;

    uint32_t *s_cnt = smem;
    int32_t *s_centre = (int32_t *)(s_cnt + ncnt);
    const int tmax = a.tmax;
    int32_t *s_off = s_centre + tmax;
    uint32_t *s_d = (uint32_t *)(s_off + tmax * (levels + 1));
    uint32_t *s_tid = s_d + tmax * levels;
    uint32_t *s_valid = s_tid + tmax;
    uint32_t *s_cw = s_valid + tmax;                        // the centre's codes of cycles 0 .. B1-1
    const int q_base = (int)((((s_cw + tmax + 4) - smem) + 3) & ~3);
    uint2 *q_a = (uint2 *)(smem + q_base) + wave * 2 * kLwQCap;
    uint2 *q_b = q_a + kLwQCap;

    gbytes filt = as_global(a.s.filter[tile]);
    const uint8_t *const *ptab = STRIDED ? nullptr : a.s.planes + (size_t)tile * L;
    gbytes base0 = STRIDED ? as_global(a.s.planes[tile]) : nullptr;
    const int64_t stride = a.s.stride;
    auto plane_ptr = [&](int j) -> gbytes {
        if (WS == 4)
            return base0 + (int64_t)(j >> 2) * stride + (j & 3);
        return STRIDED ? base0 + (int64_t)j * stride : as_global(ptab[j]);
    };
    // interleaved: group g of well w as a dword (short reads have fewer groups: clamped, the excess masked by nc)
    auto group_dword = [&](int g, uint32_t w) -> uint32_t {
        const int64_t go = (int64_t)min(g, max((L + 3) / 4 - 1, 0)) * stride;
        return *(const __attribute__((address_space(1))) uint32_t *)(base0 + go + (size_t)w * 4);
    };

    // ---------------- phase 0: the block's targets ----------------
    for (int i = threadIdx.x; i < ncnt; i += kBlock)
        s_cnt[i] = 0;
    for (int i = threadIdx.x; i < n_t * levels; i += kBlock)
        s_d[i] = 0;
    for (int lt = threadIdx.x; lt < n_t; lt += kBlock) {
        const uint32_t e = a.btgt[bd.z + lt];
        const uint32_t c = (uint32_t)a.bcen[bd.z + lt];
        s_tid[lt] = e;
        s_centre[lt] = (int32_t)c;
        s_valid[lt] = (uint32_t)filt[c] & 1u;               // :236-237
        uint32_t cw = 0;
        if constexpr (WS == 4) {
#pragma unroll
            for (int g = 0; g < NLD; g++)
                cw |= lev2_codes4(L > 0 ? group_dword(g, c) : 0u) << (16 * g);
        } else {
#pragma unroll
            for (int q = 0; q < B1; q++)
                if (q < L)
                    cw |= lev2_code(ldb(plane_ptr(q), c)) << (4 * q);
        }
        s_cw[lt] = cw;
    }
    // the ring offsets of the block's targets: a copy of the block's slice of `boff` (build_line_tables lays the
    // rows out per block, so this is one coalesced pass with nothing depending on the target's index - as a
    // gather from lvl_off it was up to nine dependent round trips per target, or a private array in scratch)
    for (int i = threadIdx.x; i < n_t * (levels + 1); i += kBlock)
        s_off[i] = a.boff[(size_t)bd.z * (levels + 1) + i];
    __syncthreads();

    QEnv env;
    env.s_centre = s_centre;
    env.s_off = s_off;
    env.s_d = s_d;
    env.s_tid = s_tid;
    env.base0 = base0;
    env.ptab = ptab;
    env.stride = stride;
    env.levels = levels;
    env.L = L;
    env.k = k;
    env.tile = tile;
    env.t_first = 0;
    int qn = 0;

    // ---------------- phase 1: the pairs, two per lane and step ----------------
    const int n_steps = (np + kWaves * kLwStep - 1) / (kWaves * kLwStep);      // steps of this wave (the waves take steps in turn)
    {
        gbytes pp[NLD];
#pragma unroll
        for (int q = 0; q < NLD; q++)
            pp[q] = WS == 4 ? base0 + (int64_t)min(q, max((L + 3) / 4 - 1, 0)) * stride        // group q of the tile
                            : plane_ptr(min(q, max(L - 1, 0)));
        const uint32_t idle_well = (uint32_t)a.pw[p0];      // what a pair of a filtered-out target reads instead
        // registers by age: 0 = indices being loaded, 1 = their bytes being asked for, 2 = bytes in flight,
        // 3 = being consumed.  Program order in a step: the index loads of step s, then the byte loads of
        // step s-1 (its indices were asked for a step ago, BEFORE that step's bytes: waiting for them leaves
        // those bytes in flight), then the compares of step s-3 - two steps' bytes are on their way at any time
        uint32_t w0_0 = 0, w1_0 = 0, m0_0 = 0, m1_0 = 0, w0_1 = 0, w1_1 = 0, m0_1 = 0, m1_1 = 0;
        uint32_t w0_2 = 0, w1_2 = 0, m0_2 = 0, m1_2 = 0, w0_3 = 0, w1_3 = 0, m0_3 = 0, m1_3 = 0;
        bool h0_0 = false, h1_0 = false, h0_1 = false, h1_1 = false, h0_2 = false, h1_2 = false, h0_3 = false, h1_3 = false;
        uint32_t b0_1[NLD], b1_1[NLD], b0_2[NLD], b1_2[NLD], b0_3[NLD], b1_3[NLD];
#pragma unroll
        for (int q = 0; q < NLD; q++)
            b0_1[q] = b1_1[q] = b0_2[q] = b1_2[q] = b0_3[q] = b1_3[q] = 0;
        for (int s = 0; s < n_steps + 3; s++) {
            // rotate ages
            w0_3 = w0_2; w1_3 = w1_2; m0_3 = m0_2; m1_3 = m1_2; h0_3 = h0_2; h1_3 = h1_2;
#pragma unroll
            for (int q = 0; q < NLD; q++) {
                b0_3[q] = b0_2[q];
                b1_3[q] = b1_2[q];
                b0_2[q] = b0_1[q];
                b1_2[q] = b1_1[q];
            }
            w0_2 = w0_1; w1_2 = w1_1; m0_2 = m0_1; m1_2 = m1_1; h0_2 = h0_1; h1_2 = h1_1;
            w0_1 = w0_0; w1_1 = w1_0; m0_1 = m0_0; m1_1 = m1_0; h0_1 = h0_0; h1_1 = h1_0;
            // stage A: indices of step s (clamped to the block's last pair)
            {
                const int r0 = (min(s, n_steps - 1) * kWaves + wave) * kLwStep + lane, r1 = r0 + kWave;
                h0_0 = s < n_steps && r0 < np;
                h1_0 = s < n_steps && r1 < np;
                const int i0 = p0 + min(r0, np - 1), i1 = p0 + min(r1, np - 1);
                w0_0 = (uint32_t)a.pw[i0];
                w1_0 = (uint32_t)a.pw[i1];
                m0_0 = a.pm[i0];
                m1_0 = a.pm[i1];
            }
            // stage B: plane bytes of step s-1
            {
                const bool v0 = h0_1 && s_valid[m0_1 >> 16] != 0u, v1 = h1_1 && s_valid[m1_1 >> 16] != 0u;
                h0_1 = v0;
                h1_1 = v1;
                const uint32_t x0 = v0 ? w0_1 : idle_well, x1 = v1 ? w1_1 : idle_well;
                if (L > 0) {
#pragma unroll
                    for (int q = 0; q < NLD; q++) {
                        if constexpr (WS == 4) {             // a dword: four cycles of the well
                            b0_1[q] = *(const __attribute__((address_space(1))) uint32_t *)(pp[q] + (size_t)x0 * 4);
                            b1_1[q] = *(const __attribute__((address_space(1))) uint32_t *)(pp[q] + (size_t)x1 * 4);
                        } else {
                            b0_1[q] = ldb(pp[q], x0);
                            b1_1[q] = ldb(pp[q], x1);
                        }
                    }
                }
            }
            // stage C: consume step s-3
            if (s >= 3) {
                const uint32_t lt0 = m0_3 >> 16, lt1 = m1_3 >> 16;
                const uint32_t ca0 = s_cw[lt0], ca1 = s_cw[lt1];
                uint32_t wb0 = 0, wb1 = 0;
#pragma unroll
                for (int q = 0; q < NLD; q++) {
                    if constexpr (WS == 4) {
                        wb0 |= lev2_codes4(b0_3[q]) << (16 * q);
                        wb1 |= lev2_codes4(b1_3[q]) << (16 * q);
                    } else {
                        wb0 |= lev2_code(b0_3[q]) << (4 * q);
                        wb1 |= lev2_code(b1_3[q]) << (4 * q);
                    }
                }
                const int nc = min(B1, L);
                bool al0, al1;
                uint32_t t0, t1;                             // what travels in the entry's tag besides target and slot
                if constexpr (LEVH == 0) {
                    const uint32_t keep = nc >= 8 ? kLev2Nib : (((1u << (4 * nc)) - 1u) & kLev2Nib);
                    const uint32_t x0 = ca0 ^ wb0, x1 = ca1 ^ wb1;
                    const int mm0 = __popc((x0 | (x0 >> 1) | (x0 >> 2)) & keep), mm1 = __popc((x1 | (x1 >> 1) | (x1 >> 2)) & keep);
                    al0 = h0_3 && mm0 <= k;
                    al1 = h1_3 && mm1 <= k;
                    t0 = (uint32_t)min(mm0, 255) << 16;
                    t1 = (uint32_t)min(mm1, 255) << 16;
                } else {
                    const uint32_t st0 = lev2_step(lev2_init(), ca0, wb0, nc), st1 = lev2_step(lev2_init(), ca1, wb1, nc);
                    al0 = h0_3 && lev2_alive(st0);
                    al1 = h1_3 && lev2_alive(st1);
                    t0 = st0 << 12;
                    t1 = st1 << 12;
                }
                const uint64_t ma = __ballot(al0), mb = __ballot(al1);
                if (ma | mb) {
                    const uint32_t e0 = m0_3 & 0xFFFFu, e1 = m1_3 & 0xFFFFu;
                    if (B1 >= L) {                           // the whole read has been seen
                        if (al0)
                            q_record_dup(env, (int)lt0, (int)e0, LEVH == 0 ? (int)(t0 >> 16) : lev2_dist(t0 >> 12));
                        if (al1)
                            q_record_dup(env, (int)lt1, (int)e1, LEVH == 0 ? (int)(t1 >> 16) : lev2_dist(t1 >> 12));
                    } else {
                        const int n0 = __popcll(ma), n1 = __popcll(mb);
                        if (n0 + n1 >= kLwInPlace) {
                            WD_Q_CHECK(in_place, n0 + n1, n0 + n1 <= kLwStep);
                            // A third of the step's pairs still alive after the first round: reads of low diversity
                            // (amplicons, failed cycles).  Through the queue every one of them would be written,
                            // read back and compacted round after round - this step is finished where it stands,
                            // every lane on its own two pairs (as k_scan_q does with a pass: kFinishInPlace).
                            const uint32_t c0 = (uint32_t)s_centre[lt0], c1 = (uint32_t)s_centre[lt1];
                            bool x0 = al0, x1 = al1;
                            uint32_t r0 = LEVH == 0 ? (t0 >> 16) : (t0 >> 12), r1 = LEVH == 0 ? (t1 >> 16) : (t1 >> 12);
                            for (int j = B1; j < L && (__ballot(x0) | __ballot(x1)); j += 4) {
                                uint32_t wa0, wa1, wb0, wb1;             // codes of 4 cycles: centres (a) and wells (b)
                                if constexpr (WS == 4) {
                                    const uint32_t g = (uint32_t)(j >> 2);   // (B1 is a multiple of 4: whole groups)
                                    wb0 = lev2_codes4(group_dword((int)g, w0_3));
                                    wb1 = lev2_codes4(group_dword((int)g, w1_3));
                                    wa0 = lev2_codes4(group_dword((int)g, c0));
                                    wa1 = lev2_codes4(group_dword((int)g, c1));
                                } else {
                                    uint32_t ub0[4], ub1[4], ua0[4], ua1[4];
#pragma unroll
                                    for (int q = 0; q < 4; q++) {
                                        gbytes p = plane_ptr(min(j + q, L - 1));
                                        ub0[q] = ldb(p, w0_3);
                                        ub1[q] = ldb(p, w1_3);
                                        ua0[q] = ldb(p, c0);
                                        ua1[q] = ldb(p, c1);
                                    }
                                    wa0 = wa1 = wb0 = wb1 = 0;
#pragma unroll
                                    for (int q = 0; q < 4; q++) {
                                        wb0 |= lev2_code(ub0[q]) << (4 * q);
                                        wb1 |= lev2_code(ub1[q]) << (4 * q);
                                        wa0 |= lev2_code(ua0[q]) << (4 * q);
                                        wa1 |= lev2_code(ua1[q]) << (4 * q);
                                    }
                                }
                                const int ncy = min(4, L - j);
                                if constexpr (LEVH == 0) {
                                    const uint32_t keep4 = ((1u << (4 * ncy)) - 1u) & kLev2Nib;
                                    const uint32_t y0 = wa0 ^ wb0, y1 = wa1 ^ wb1;
                                    r0 += (uint32_t)__popc((y0 | (y0 >> 1) | (y0 >> 2)) & keep4);
                                    r1 += (uint32_t)__popc((y1 | (y1 >> 1) | (y1 >> 2)) & keep4);
                                    x0 = x0 && (int)r0 <= k;
                                    x1 = x1 && (int)r1 <= k;
                                } else {
                                    r0 = lev2_step(r0, wa0, wb0, ncy);
                                    r1 = lev2_step(r1, wa1, wb1, ncy);
                                    x0 = x0 && lev2_alive(r0);
                                    x1 = x1 && lev2_alive(r1);
                                }
                            }
                            if (x0)
                                q_record_dup(env, (int)lt0, (int)e0, LEVH == 0 ? (int)r0 : lev2_dist(r0));
                            if (x1)
                                q_record_dup(env, (int)lt1, (int)e1, LEVH == 0 ? (int)r1 : lev2_dist(r1));
                            continue;
                        }
                        if (qn + n0 + n1 > kLwQCap) {
                            WD_Q_CHECK(drain_mid, qn, qn <= kLwQCap);
                            if constexpr (LEVH == 0)
                                q_drain<STRIDED, 8, WS>(env, q_a, q_b, qn, B1, lane);
                            else
                                q_drain_lev2<STRIDED, WS>(env, q_a, q_b, qn, B1, lane);
                        }
                        WD_Q_CHECK(push, qn + n0 + n1, qn + n0 + n1 <= kLwQCap);
                        q_push(q_a, qn, ma, al0, w0_3, (lt0 << 24) | t0 | e0);
                        q_push(q_a, qn + n0, mb, al1, w1_3, (lt1 << 24) | t1 | e1);
                        qn += n0 + n1;
                    }
                }
            }
        }
        if (qn > 0) {
            if constexpr (LEVH == 0)
                q_drain<STRIDED, 8, WS>(env, q_a, q_b, qn, B1, lane);
            else
                q_drain_lev2<STRIDED, WS>(env, q_a, q_b, qn, B1, lane);
        }
    }
    __syncthreads();

    // ---------------- phase 3: tallies ----------------
    // (count_well_duplicates.py:80-95 as histograms; Hit / first / last through the targets' hit masks:
    // another block may hold the rest of a target's pairs.)  One LANE per target: Targets and Wells - every
    // target has them - are wave sums; duplicates are rare and go lane by lane.  (The counters are 32-bit
    // and wrap: a later block may move a first / last hit, so a block's delta may be negative.)
    uint32_t acc_valid = 0;
    for (int base = wave * kWave; base < n_t; base += kWaves * kWave) {
        const int lt = base + lane;
        const bool in = lt < n_t;
        const uint32_t e = in ? s_tid[lt] : 0u;
        const int t = (int)(e & 0x7FFFFFFFu);
        const bool owner = in && (e >> 31) != 0u, valid = in && s_valid[lt] != 0u;
        uint32_t *opt = a.s.out_per_target ? a.s.out_per_target + ((size_t)tile * a.s.T + t) * levels : nullptr;
        if (owner && !valid && opt)
            for (int l = 0; l < levels; l++)
                opt[l] = WD_INVALID_TARGET;
        const bool counts = owner && valid;                  // the block with a target's first pair counts it
        acc_valid += lw_wave_sum(counts ? 1u : 0u);
        for (int l = 0; l < levels; l++) {
            const uint32_t sz = counts ? (uint32_t)(s_off[lt * (levels + 1) + l + 1] - s_off[lt * (levels + 1) + l]) : 0u;
            const uint32_t sum = lw_wave_sum(sz);
            if (lane == 0 && sum)
                atomicAdd(&s_cnt[1 + l], sum);
        }
        uint32_t bits = 0;
        if (valid)
            for (int l = 0; l < levels; l++)
                bits |= (s_d[lt * levels + l] > 0u ? 1u : 0u) << l;
        if (bits) {
            for (int l = 0; l < levels; l++) {
                const uint32_t d = s_d[lt * levels + l];
                if (d) {
                    atomicAdd(&s_cnt[1 + levels + l], d);
                    if (opt)
                        atomicAdd(&opt[l], d);
                }
            }
            const int sh = (t & 3) * 8;
            const uint32_t old = (atomicOr(a.mask + (size_t)tile * a.mask_stride + (t >> 2), bits << sh) >> sh) & 0xFFu;
            const uint32_t now = old | bits, fresh = bits & ~old;
            for (int l = 0; l < levels; l++)
                if ((fresh >> l) & 1u)
                    atomicAdd(&s_cnt[1 + 2 * levels + l], 1u);
            if (now != old) {
                const int f_old = old ? __ffs((int)old) - 1 : -1, f_new = __ffs((int)now) - 1;
                const int l_old = old ? 31 - __clz((int)old) : -1, l_new = 31 - __clz((int)now);
                if (f_new != f_old) {
                    atomicAdd(&s_cnt[1 + 3 * levels + f_new], 1u);
                    if (f_old >= 0)
                        atomicAdd(&s_cnt[1 + 3 * levels + f_old], ~0u);          // -1 (mod 2^32)
                }
                if (l_new != l_old) {
                    atomicAdd(&s_cnt[1 + 4 * levels + l_new], 1u);
                    if (l_old >= 0)
                        atomicAdd(&s_cnt[1 + 4 * levels + l_old], ~0u);
                }
            }
        }
    }
    if (lane == 0 && acc_valid)
        atomicAdd(&s_cnt[0], acc_valid);
    __syncthreads();
    for (int i = threadIdx.x; i < ncnt; i += kBlock) {
        const int32_t v = (int32_t)s_cnt[i];                 // (first / last deltas may be negative)
        if (v)
            atomicAdd(&a.s.out_tile[(size_t)tile * ncnt + i], (unsigned long long)(long long)v);
    }
}
