// scan_dense.inc - the dense path: one LANE per target, for "every well is a centre" scans.
// Included by welldup.hip after scan_queue.inc.
// -------------------------------------------------------------------------------------
// With millions of targets of ~36 neighbours each (BASELINE config 5) a wave per target wastes
// most lanes and pays hundreds of instructions per target, and every well is visited ~36 times
// as somebody's neighbour.  The dense path is five small kernels per scan:
//   k_dense_sig     folds the first 10 cycles of every well into a 32-bit signature (3 bits per
//                   cycle: base code 0..3, 4 = no-call): 10 planes read once, 4 bytes per well out;
//   k_dense_pairs   one lane per target, consecutive lanes = consecutive centres.  For the q-th
//                   neighbour the 64 lanes read 64 entries of the transposed neighbour table (one
//                   contiguous run: int16 offsets from the centre, or int32 indices) and 64 mostly
//                   consecutive signatures: one load and one compare per (target, neighbour).
//                   Only 36/4^10 = 3e-5 random neighbours per target outlive it - the survivors
//                   are the duplicates.  They are queued in LDS and leave for the block's own
//                   region of a survivor queue in global memory (an LDS counter per block: one
//                   shared global counter would serialise ~1 atomic per wave in L2 and cost 10x
//                   the kernel).  Also counts Targets and Wells;
//   k_dense_pack    only when the batch holds many survivors: folds ALL cycles of every well
//                   into 16-byte pieces of 40 cycles.  Checking one pair byte by byte touches
//                   2 x (L - 10) cache lines, one per plane; beyond ~0.7 % duplicate wells that
//                   costs more HBM lines than streaming every plane exactly once;
//   k_dense_verify  settles the survivors: the two wells' packed pieces when the batch was
//                   packed, otherwise one lane per CYCLE over the planes.  A duplicate bumps Dups
//                   and, through an atomic per-target hit mask, moves Hit / first-hit / last-hit
//                   counters (each mask transition is applied once, so the histograms come out
//                   exact whatever the order);
//   k_dense_reduce  folds the per-tile counter slots into out_tile.
// Levenshtein <= 2 (the reference's default) rides the same kernels: see lev2_window (dense_forms.inc).
// Since round 2 most groups of 64 consecutive centres compare from LDS windows (k_dense_windows,
// k_dense_pairs_win); since round 3, where the neighbour relation is symmetric (every well a centre:
// k_dense_symcheck), every pair is compared once, from its lower well, and recorded at both ends
// (DenseArgs::sym, dense_record_pair), and the windows arrive by inline-assembly LDS-DMA with counted
// waits (lds_dma_dword: the builtin makes the compiler wait for the DMA before every LDS read).
// The pairs kernel is bound by gather latency x occupancy and L1/TA issue, not by HBM
// (profiles/r01_f_*): hence the signature (one load per compare instead of one per cycle), the
// branch-free survivor test, the register-rotated software pipeline, and nothing but loads and
// LDS traffic inside its loop.
// (kDenseChainVersion, kSigCycles, kRowGroups, kDenseMaxK: wd_shared.h - the dispatch needs them too)
// (kDenseSlots, kMaxSeg, kWinMaxK, kWinGap, kWinDwords, kMarkBlock, kWinBufs, kWinBufsSym, kRankBlock and the arithmetic
// of a launch - strides, LDS dwords per wave, window counts, grids: dense_launch.inc, free of HIP, which the CPU
// emulation of this chain shares)
#include "dense_launch.inc"

// ---- the seams of this file for the CPU emulation (tools/scan_dense_emu.cpp, which defines WD_EMU) ----
// What a host compiler cannot take - inline assembly and LDS addresses - stands behind these; on the device each
// expands to exactly the text that stood in its place, in the style of WD_DYNAMIC_LDS (device_common.inc).
//   WD_PIN(constraints)     the empty asm that makes values opaque to the optimiser; nothing on the CPU
//   WD_WAIT_VM0 / _N(n)     s_waitcnt vmcnt(0) / vmcnt(immediate); on the CPU a rendezvous of the wave that lands
//                           the wave's oldest LDS-DMA pieces until n remain (emu_dma_wait)
//   WD_LDS_ADDR(p)          the LDS byte address of p; on the CPU its byte offset in the launch's LDS block
//   WD_DENSE_NOTE(event)    nothing on the device; the CPU emulation counts the regions that overflowed
//   WD_LOCKSTEP()           nothing on the device, where the lanes of a wave run in lockstep: the places where a lane
//                           reads LDS words another lane of its wave wrote just before, with no collective between.
//                           The emulation's fibers are not in lockstep, so this is a rendezvous of the wave there.
//   WD_DENSE_CONTROL(name, statement)  nothing on the device; the emulation runs the statement when its control
//                           `name` is on - a bug planted on purpose, to show that the emulation's checks can fail
// wait_vmcnt and lds_dma_dword (below) have a CPU body each; the address-space casts are empty attributes there
// (tools/wave_emu.h), so the scalar-cache pointer loads ((address_space(4)) of a.filter) compile as they stand.
#ifdef WD_EMU
#define WD_PIN(...) ((void)0)
#define WD_WAIT_VM0() emu_dma_wait(0)
#define WD_WAIT_VM_N(n) emu_dma_wait(n)
#define WD_LDS_ADDR(p) emu_lds_addr(p)
#define WD_DENSE_NOTE(event) emu_dense_note(kNote_##event)
#define WD_LOCKSTEP() ((void)__ballot(false))
#define WD_DENSE_CONTROL(name, statement) do { if (emu_dense_control(kControl_##name)) { statement; } } while (0)
#else
#define WD_DENSE_NOTE(event) ((void)0)
#define WD_LOCKSTEP() ((void)0)
#define WD_DENSE_CONTROL(name, statement) ((void)0)
#define WD_PIN(...) asm volatile("" : __VA_ARGS__)
#define WD_WAIT_VM0() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#define WD_WAIT_VM_N(n) asm volatile("s_waitcnt vmcnt(%0)" : : "n"(n) : "memory")
#define WD_LDS_ADDR(p) ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)(p))
#endif
using gsig = const __attribute__((address_space(1))) uint32_t *;
using gidx = const __attribute__((address_space(1))) int32_t *;

struct DenseArgs {
    const uint8_t *const *planes;   // device table: [n_tiles*L], or [n_tiles] bases if strided
    const uint8_t *const *filter;   // device table [n_tiles]
    int64_t stride;                 // bytes between consecutive cycle planes of a tile
    const int32_t *centre;
    const int32_t *lvl_off;
    const int32_t *nbr;             // CSR neighbour list (only the Levenshtein overflow path reads it)
    const void *nbr_t;              // neighbour lists transposed per 64-target group: int32 well indices,
                                    // or (idx16) int16 offsets from the target's centre
    const long long *gbase;         // start of each group's block in nbr_t
    const int32_t *rel_t;           // [levels][T]: slot where ring l+1 ends, counted from the target's first slot
    const void *udelta;             // [gbase/64 + q]: the q-th neighbour's offset from the centre where a group shares it (type of nbr_t)
    const uint8_t *guni;            // [groups]: 1 = 64 consecutive centres whose q-th neighbours all sit at centre + udelta
    // window groups (k_dense_windows): consecutive centres whose neighbours' signatures are staged in LDS
    const int32_t *ginfo;           // nullable [groups]: elements of the group's union of neighbour offsets | runs << 9 | window dwords << 14; 0 = gather
    const uint16_t *uoff;           // [groups][kpad]: where union element u of lane 0 sits in the window (bytes)
    const int2 *useg;               // [groups][kMaxSeg]: the window's runs {offset of the first signature from lane 0's centre, first dword in the window | length << 16}
    const int32_t *wdelta;          // [groups][kpad]: the union's offsets from the centre, in (ring, offset) order
    const uint8_t *wlev;            // [groups][kpad]: ... and their rings (0-based)
    const uint32_t *wmask;          // [groups][kpad / 32][64]: which union elements each lane's target has (whole union, (ring, offset) order)
    const uint8_t *wfull;           // [groups][kpad]: place in the whole union of the element the compare stage lists at this position
                                    // (the identity, or - pairs seen from one end - the elements above the centre only)
    int sym;                        // every pair is seen from its lower well only and recorded at both (dense_record_pair)
    int32_t centre0;                // ... target t's centre is centre0 + t then
    int kpad, win_dwords;           // row length of uoff / wdelta (multiple of 32, <= kWinMaxK); LDS dwords of one window
    int win_bufs;                   // LDS windows per wave (kWinBufs, or kWinBufsSym for the one-ended compare)
    uint32_t *sig;                  // [n_tiles][sig_stride] signatures
    long long sig_stride;
    uint32_t *sig2;                 // nullable [n_tiles][sig_stride]: cycles 10..19 (second look for Levenshtein)
    unsigned long long *partial;    // [n_tiles][kDenseSlots][partial_stride] counter slots (out_tile row layout)
    uint32_t *mask;                 // [n_tiles][mask_stride]: hit-level mask, 8 bits per target
    long long mask_stride;
    uint2 *queue;                   // [regions][q_per] survivors {well index, target-in-group << 24 | mismatches << 20 | level << 17 | slot}
    uint32_t *q_cnt;                // [regions] entries used; region = tile * groups + group of 64 targets
    int q_per;
    uint32_t *cand;                 // two flags of the batch: [0] there are survivors, [kDenseSlots] a Levenshtein queue overflowed
                                    // (plain stores of 1: counting them with atomics on a few lines serialised the compare stage)
    uint4 *rows;                    // nullable [n_tiles][N][kRowGroups], filled from the front: cycles 10.. of the MARKED wells only
                                    // (k_dense_pack's format), a well's row at its rank among the tile's marked wells
    uint32_t *mark;                 // [n_tiles][mw_stride]: one bit per well, set for both wells of every survivor pair
    uint32_t *wprefix;              // [n_tiles][mw_stride]: marked wells in earlier words of the same kMarkBlock-word block
    uint32_t *bprefix;              // [n_tiles][mw_stride / kMarkBlock]: marked wells in earlier blocks of the tile
    long long mw_stride;            // mark words per tile, a multiple of kMarkBlock
    int pack_mode;                  // -1 = by threshold, 0 = never, 1 = always
    uint32_t *out_per_target;       // nullable [n_tiles][T][levels]
    const ScanRare *rare;
    long long N;
    int T, levels, L, k, n_tiles, tile_chunk, sig_cycles, partial_stride, strided, check_empty, log_hits, idx16;
    int lev2;                       // Levenshtein <= 2 instead of Hamming <= k (needs rows)
    const int32_t *pblocks;         // nullable [n_pblocks]: the target blocks k_dense_pairs is launched over (the rest are window groups)
    int n_pblocks;
    int tile0;                      // index of this part's first tile in the scan (hit records carry scan-wide tile numbers)
};

__device__ inline gbytes dense_plane(const DenseArgs &a, int tile, int j)
{
    return a.strided ? as_global(a.planes[tile]) + (int64_t)j * a.stride
                     : as_global(a.planes[(size_t)tile * a.L + j]);
}

// The planes of one tile, resolved once per kernel.  STRIDED: a scalar base and a stride, so a
// plane address is pure arithmetic; otherwise one pointer load per plane.  (Deciding this at run
// time inside the load loops puts a pointer load and a full wait in front of every data load.)
template <bool STRIDED>
struct TilePlanes {
    gbytes base;
    int64_t stride;
    const uint8_t *const *tbl;
    __device__ inline TilePlanes(const DenseArgs &a, int tile)
    {
        stride = a.stride;
        tbl = STRIDED ? nullptr : a.planes + (size_t)tile * a.L;
        base = nullptr;
        if (STRIDED) {
            const uint64_t b = (uint64_t)a.planes[tile];
            base = (gbytes)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(b >> 32)) << 32) |
                            (uint32_t)__builtin_amdgcn_readfirstlane((int)b));
        }
    }
    __device__ inline gbytes at(int j) const { return STRIDED ? base + (int64_t)j * stride : as_global(tbl[j]); }
};

// The pure forms - codes4, fold10x4, sig_mismatches, lev2_window, transpose4x4, the readers of a packed row,
// row_lev2, lev2_screen, lev2_window16, screen_mismatches, lev2_masks - and kSigLow, kScreenCycles, kRowCycles,
// kRowDw: a file of their own, which tools/dense_forms_check.cpp compiles for the CPU.
#include "dense_forms.inc"

// Ten cycles (planes j0 .. j0+9, all present) of wells i .. i+3 -> one 30-bit word per well.
// NT: non-temporal loads, for kernels that stream the planes once.
template <bool STRIDED, bool NT = false>
__device__ inline void pack10x4(const TilePlanes<STRIDED> &pl, int j0, long long i, uint32_t (&out)[4])
{
    gbytes p[10];
#pragma unroll
    for (int f = 0; f < 10; f++)
        p[f] = pl.at(j0 + f);
    uint32_t v[10];
#pragma unroll
    for (int f = 0; f < 10; f++)
        v[f] = NT ? __builtin_nontemporal_load((const __attribute__((address_space(1))) uint32_t *)(p[f] + i))
                  : *(const __attribute__((address_space(1))) uint32_t *)(p[f] + i);
    fold10x4(v, out);
}

// Sixteen cycles (planes 0..15, all present) of wells i .. i+3 -> the signature word (cycles 0..9,
// exact) and the screen word per well: byte & 3 per cycle, so a no-call (byte 0) reads as A - fine
// for a screen, which may only err towards "maybe" (merging two symbols can only lower an edit
// distance).  Every plane is loaded once.
template <bool STRIDED>
__device__ inline void sig_screen16x4(const TilePlanes<STRIDED> &pl, long long i, uint32_t (&sig)[4], uint32_t (&scr)[4])
{
    uint32_t v[kScreenCycles];
#pragma unroll
    for (int f = 0; f < kScreenCycles; f++)
        v[f] = __builtin_nontemporal_load((const __attribute__((address_space(1))) uint32_t *)(pl.at(f) + i));
    uint32_t first[10];
#pragma unroll
    for (int f = 0; f < 10; f++)
        first[f] = v[f];
    fold10x4(first, sig);
    scr[0] = scr[1] = scr[2] = scr[3] = 0;
#pragma unroll
    for (int m = 0; m < 4; m++) {                      // four cycles per byte lane, then one byte per well
        const uint32_t q = (v[4 * m] & 0x03030303u) | ((v[4 * m + 1] & 0x03030303u) << 2) |
                           ((v[4 * m + 2] & 0x03030303u) << 4) | ((v[4 * m + 3] & 0x03030303u) << 6);
#pragma unroll
        for (int b = 0; b < 4; b++)
            scr[b] |= ((q >> (8 * b)) & 0xFFu) << (8 * m);
    }
}

// The scratch the rest of the chain expects zeroed - hit masks, mark words and counter slots of this
// tile, the batch's two flags - cleared by the first kernel of the chain (four memset launches and the
// gaps around them were 30 us of a part's 1.3 ms).
__device__ inline void dense_clear_scratch(const DenseArgs &a, int tile)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x, G = (long long)gridDim.x * blockDim.x;
    uint4 *mask = (uint4 *)(a.mask + (size_t)tile * a.mask_stride);            // (strides: multiples of 32 words)
    for (long long w = g; w < a.mask_stride / 4; w += G)
        mask[w] = make_uint4(0u, 0u, 0u, 0u);
    if (a.rows) {
        uint4 *mark = (uint4 *)(a.mark + (size_t)tile * a.mw_stride);
        for (long long w = g; w < a.mw_stride / 4; w += G)
            mark[w] = make_uint4(0u, 0u, 0u, 0u);
    }
    unsigned long long *partial = a.partial + (size_t)tile * kDenseSlots * a.partial_stride;
    for (long long w = g; w < (long long)kDenseSlots * a.partial_stride; w += G)
        partial[w] = 0ull;
    if (tile == 0)
        for (long long w = g; w < kDenseSlots + 1; w += G)
            a.cand[w] = 0u;
}

// VEC4: every plane is 4-byte aligned, so a thread folds 4 consecutive wells from dword loads
template <bool VEC4, bool STRIDED>
__global__ __launch_bounds__(kBlock) void k_dense_sig(DenseArgs a)
{
    const int tile = blockIdx.y;
    dense_clear_scratch(a, tile);
    const TilePlanes<STRIDED> pl(a, tile);
    constexpr int V = VEC4 ? 4 : 1;
    const long long i = ((long long)blockIdx.x * kBlock + threadIdx.x) * V;
    if (i >= a.N)
        return;
    uint32_t *out = a.sig + (size_t)tile * a.sig_stride;
    uint32_t *out2 = a.sig2 ? a.sig2 + (size_t)tile * a.sig_stride : nullptr;
    if (VEC4 && i + 4 <= a.N && out2 && a.L >= kScreenCycles) {
        // Levenshtein: cycles 0..9, 3 bits each, exact -> sig; cycles 0..15, 2 bits each -> the
        // screen word the compare stage reads
        uint32_t o[4], o2[4];
        sig_screen16x4(pl, i, o, o2);
        *(uint4 *)(out + i) = make_uint4(o[0], o[1], o[2], o[3]);
        *(uint4 *)(out2 + i) = make_uint4(o2[0], o2[1], o2[2], o2[3]);
        return;
    }
    {   // cycles 0..9, 3 bits each, exact (no-call = 4) -> sig
        const int S = min(kSigCycles, a.L);
        if (VEC4 && i + 4 <= a.N && S == kSigCycles) {
            uint32_t o[4];
            pack10x4<STRIDED, true>(pl, 0, i, o);             // (non-temporal: the planes are streamed)
            *(uint4 *)(out + i) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
            for (long long w = i; w < a.N && w < i + V; w++) {
                uint32_t sgn = 0;
                for (int j = 0; j < S; j++)
                    sgn |= code_of(pl.at(j)[w]) << (3 * j);
                out[w] = sgn;
            }
        }
    }
    if (out2) {   // short reads or unaligned planes: the screen word, well by well
        const int S = min(kScreenCycles, a.L);
        for (long long w = i; w < a.N && w < i + V; w++) {
            uint32_t sgn = 0;
            for (int j = 0; j < S; j++)
                sgn |= ((uint32_t)pl.at(j)[w] & 3u) << (2 * j);
            out2[w] = sgn;
        }
    }
}

// Was (will) this batch be packed?  Every wave of k_dense_pack and k_dense_verify asks the same
// device-side question, so the host never has to wait for the survivor count.
__device__ inline bool dense_packed(const DenseArgs &a)
{
    if (!a.rows)
        return false;
    if (a.cand[kDenseSlots])                      // a Levenshtein group overflowed: rows are needed
        return true;
    if (a.pack_mode == 0)
        return false;
    return a.pack_mode > 0 || a.cand[0] != 0;     // rows whenever there is a survivor (launch_dense)
}

// ---- marked wells and their rows --------------------------------------------------------
// k_dense_pairs sets one bit per well that takes part in a survivor pair (usually a few percent
// of the tile).  Only those wells get a packed row, at their rank among the tile's marked wells:
// rank = marked wells in earlier blocks (bprefix) + in earlier words of the block (wprefix) +
// lower bits of the well's own word.  So the pack kernel writes 64 bytes per MARKED well instead
// of per well, its loads skip every cache line without a marked well, and the verify kernel finds
// a well's whole row in one 64-byte piece.
struct MarkIndex {
    const uint32_t *mark, *wprefix, *bprefix;
    __device__ inline MarkIndex(const DenseArgs &a, int tile)
        : mark(a.mark + (size_t)tile * a.mw_stride), wprefix(a.wprefix + (size_t)tile * a.mw_stride),
          bprefix(a.bprefix + (size_t)tile * (a.mw_stride / kMarkBlock)) {}
    __device__ inline uint32_t rank(uint32_t well) const
    {
        const uint32_t w = well >> 5;
        return bprefix[w / kMarkBlock] + wprefix[w] + (uint32_t)__popc(mark[w] & ((1u << (well & 31u)) - 1u));
    }
};

__device__ inline void dense_mark(const DenseArgs &a, int tile, uint32_t well)
{
    atomicOr(a.mark + (size_t)tile * a.mw_stride + (well >> 5), 1u << (well & 31u));
}

// exclusive prefix sum over the block's threads (blockDim.x = 64 * NW); total in *sum
template <int NW>
__device__ inline uint32_t block_exclusive_scan(uint32_t v, uint32_t *s_w, uint32_t *sum)
{
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        inc += lane >= d ? o : 0u;
    }
    if (lane == kWave - 1)
        s_w[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < NW; i++) {
        before += i < wave ? s_w[i] : 0u;
        all += s_w[i];
    }
    __syncthreads();
    *sum = all;
    return before + inc - v;
}

// per block of kMarkBlock mark words: marked wells before each word (wprefix) and in the block
// (left in bprefix for k_dense_rank_blocks)
__global__ __launch_bounds__(kMarkBlock) void k_dense_rank_words(DenseArgs a)
{
    __shared__ uint32_t s_w[kMarkBlock / kWave];
    if (!dense_packed(a))
        return;
    const int tile = blockIdx.y;
    const size_t w = (size_t)blockIdx.x * kMarkBlock + threadIdx.x;
    uint32_t total;
    const uint32_t ex = block_exclusive_scan<kMarkBlock / kWave>(
        (uint32_t)__popc(a.mark[(size_t)tile * a.mw_stride + w]), s_w, &total);
    a.wprefix[(size_t)tile * a.mw_stride + w] = ex;
    if (threadIdx.x == 0)
        a.bprefix[(size_t)tile * (a.mw_stride / kMarkBlock) + blockIdx.x] = total;
}

// per tile: block totals -> marked wells before each block
__global__ __launch_bounds__(kRankBlock) void k_dense_rank_blocks(DenseArgs a)
{
    __shared__ uint32_t s_w[kRankBlock / kWave];
    if (!dense_packed(a))
        return;
    uint32_t *bp = a.bprefix + (size_t)blockIdx.x * (a.mw_stride / kMarkBlock);
    const long long nb = a.mw_stride / kMarkBlock;
    uint32_t carry = 0;
    for (long long b0 = 0; b0 < nb; b0 += kRankBlock) {
        const long long b = b0 + threadIdx.x;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan<kRankBlock / kWave>(b < nb ? bp[b] : 0u, s_w, &total);
        if (b < nb)
            bp[b] = carry + ex;
        carry += total;
    }
}

// Cycles sig_cycles.. of every MARKED well -> its row (the first word of a read is its signature).
// VEC wells per thread (4 needs every plane 4-byte aligned and reads dwords).  Threads without a
// marked well leave at once, so only cache lines that hold a marked well are fetched.
// ---- packed rows, round 3's format ---------------------------------------------------------
// A marked well's row (64 bytes) holds cycles kSigCycles.. in five groups of 32 cycles, three dwords each:
//   [3k], [3k+1]  the bases, two bits per cycle (byte q = cycles 4q .. 4q+3 of the group; a no-call's bits
//                 are 0, as its byte's are)
//   [3k+2]        one bit per cycle: the byte was NOT a no-call
// Round 2's rows held 3-bit codes, ten cycles to a word; turning a loaded dword (one cycle of four wells)
// into those cost 15 vector instructions, and the pack kernel - which streams 140 planes and should be
// nothing but an HBM stream - spent 55 % of the chip's vector issue slots on it (DESIGN.md 5.4).  Here
// the four wells of a dword stay side by side in its byte lanes until the end: the bases of four cycles
// are two instructions per cycle ((v & 0x03030303) << 2f, or-ed), the no-call bits five (exact non-zero
// test per byte, rotated into a byte of flags), and a 4 x 4 byte transpose (8 v_perm) per 16 cycles
// hands every well its own dwords: about 8 instructions per dword loaded.
// The grid may hold fewer workgroups than the tile has blocks of kBlock * VEC wells (gridDim.x of them
// per tile): each then walks the tile with a stride - a bounded footprint, so that the compare stage of
// the next part finds wave slots beside it (launch_dense).
constexpr int kPackChunks = 4;        // chunks of eight cycles whose loads a thread has in flight together (1, 2, 4)
template <int VEC, bool STRIDED, bool NT = false>
__global__ __launch_bounds__(kBlock) void k_dense_pack(DenseArgs a)
{
    if (!dense_packed(a))
        return;
    const int tile = blockIdx.y;
    const MarkIndex mi(a, tile);
    const TilePlanes<STRIDED> pl(a, tile);
    const int L = a.L;
    uint32_t *rows = (uint32_t *)(a.rows + (size_t)tile * a.N * kRowGroups);
    const long long n_vb = (a.N + (long long)kBlock * VEC - 1) / ((long long)kBlock * VEC);
    for (long long vb = blockIdx.x; vb < n_vb; vb += gridDim.x) {
        const long long i = (vb * kBlock + threadIdx.x) * VEC;
        if (i >= a.N)
            continue;
        const uint32_t mword = mi.mark[i >> 5];
        const uint32_t bits = (mword >> (i & 31)) & ((1u << VEC) - 1u);      // VEC divides 32: one word
        if (!bits)
            continue;
        const uint32_t r0 = mi.rank((uint32_t)i);
        const bool whole = i + VEC <= a.N;
        for (int k = 0; k < kRowCycles / 32; k++) {
            const int jg = kSigCycles + 32 * k;
            if (jg >= L)
                break;                                      // k_dense_verify never reads these
            constexpr int PC = STRIDED ? kPackChunks : 1;   // (a table of plane pointers: 32 of them at once spill)
            uint32_t Q[8], Z[4];                            // byte lane b = well i + b
#pragma unroll
            for (int c = 0; c < 4; c++)
                Q[2 * c] = Q[2 * c + 1] = Z[c] = 0;
            auto plane_dword = [&](int j) -> uint32_t {
                return NT ? __builtin_nontemporal_load((const __attribute__((address_space(1))) uint32_t *)(pl.at(j) + i))
                          : *(const __attribute__((address_space(1))) uint32_t *)(pl.at(j) + i);
            };
            auto fold8 = [&](const uint32_t *v, int c) {     // eight cycles of four wells into chunk c of Q, Z
                uint32_t nz = 0;
#pragma unroll
                for (int f = 0; f < 8; f++) {
                    Q[2 * c + (f >> 2)] |= (v[f] & 0x03030303u) << (2 * (f & 3));
                    const uint32_t x = ((v[f] & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v[f];         // bit 7: the byte is not 0
                    nz = (x & 0x80808080u) | ((nz >> 1) & 0x7F7F7F7Fu);                    // cycle f ends at bit f
                }
                Z[c] = nz;
            };
#pragma unroll
            for (int cb = 0; cb < 4; cb += PC) {
                if (VEC == 4 && jg + 8 * (cb + PC) <= L && whole) {
                    // 8 x PC loads back to back, no branch between them: the loads in flight per wave
                    // are what keeps the stream going (8 at a time: 5.6 TB/s; 32: 6.2, same box)
                    uint32_t v[8 * PC];
#pragma unroll
                    for (int f = 0; f < 8 * PC; f++)
                        v[f] = plane_dword(jg + 8 * cb + f);
#pragma unroll
                    for (int cc = 0; cc < PC; cc++)
                        fold8(v + 8 * cc, cb + cc);
                    continue;
                }
#pragma unroll
                for (int cc = 0; cc < PC; cc++) {  // the read's last cycles, the tile's last wells
                    const int c = cb + cc, j0 = jg + 8 * c;
                    if (VEC == 4 && j0 + 8 <= L && whole) {
                        uint32_t v[8];
#pragma unroll
                        for (int f = 0; f < 8; f++)
                            v[f] = plane_dword(j0 + f);
                        fold8(v, c);
                    } else {
                        for (int f = 0; f < 8 && j0 + f < L; f++) {
#pragma unroll
                            for (int b = 0; b < VEC; b++)
                                if (i + b < a.N) {
                                    const uint32_t byte = pl.at(j0 + f)[i + b];
                                    Q[2 * c + (f >> 2)] |= (byte & 3u) << (8 * b + 2 * (f & 3));
                                    Z[c] |= (byte ? 1u : 0u) << (8 * b + f);
                                }
                        }
                    }
                }
            }
            uint32_t lo[4], hi[4], nzw[4];
            transpose4x4(Q[0], Q[1], Q[2], Q[3], lo);
            transpose4x4(Q[4], Q[5], Q[6], Q[7], hi);
            transpose4x4(Z[0], Z[1], Z[2], Z[3], nzw);
#pragma unroll
            for (int b = 0; b < VEC; b++)
                if ((bits >> b) & 1u) {
                    uint32_t *row = rows + (size_t)(r0 + (uint32_t)__popc(bits & ((1u << b) - 1u))) * kRowDw + 3 * k;
                    row[0] = lo[b];
                    row[1] = hi[b];
                    row[2] = nzw[b];
                }
        }
    }
}

// Neighbour lists regrouped for the lane-per-target kernel: for each group of 64 consecutive
// targets, nbr_t[gbase + q*64 + lane] is the q-th neighbour of target 64*group + lane (the
// target's own centre where q >= K), so that one wave-load reads 256 contiguous bytes - or 128
// when every neighbour lies within +-32767 wells of its centre (the reference's generator looks
// at +-20000 records, prepare_cluster_indexes.py:19) and the table holds int16 offsets instead.
// OUT = int16_t: sets *wide if some offset does not fit (the caller then builds the int32 table).
// On a regular grid the 64 consecutive centres of a group nearly always see their q-th neighbour at
// the same offset (all but the groups that straddle a row end): such groups are flagged in guni
// and their offsets listed in udelta, so the scan needs 4 bytes per (group, q) instead of a
// 128-256 byte index load per (wave, q).
template <typename OUT>
__global__ __launch_bounds__(kWave) void k_transpose_nbr(const int32_t *centre, const int32_t *lvl_off,
                                                         const int32_t *nbr, const long long *gbase,
                                                         OUT *nbr_t, int T, int levels, uint32_t *wide,
                                                         OUT *udelta, uint8_t *guni)
{
    const int g = blockIdx.x;
    const int lane = threadIdx.x;
    const int t = g * kWave + lane;
    const bool in = t < T;
    const int off0 = in ? lvl_off[(size_t)t * (levels + 1)] : 0;
    const int K = in ? lvl_off[(size_t)t * (levels + 1) + levels] - off0 : 0;
    const int c = in ? centre[t] : 0;
    const long long b0 = gbase[g], b1 = gbase[g + 1];
    const int kmax = (int)((b1 - b0) / kWave);
    bool too_far = false;
    const int c_prev = __shfl_up(c, 1);
    bool uniform = __all(in && (lane == 0 || c == c_prev + 1)) != 0;
    for (int q = 0; q < kmax; q++) {
        const int w = q < K ? nbr[off0 + q] : c;
        const int d0 = __builtin_amdgcn_readfirstlane(w - c);
        const bool same = __all(q < K && w - c == d0) != 0;
        uniform = uniform && same;
        if (lane == 0)
            udelta[b0 / kWave + q] = same ? (OUT)d0 : (OUT)0;
        if (sizeof(OUT) == 2) {
            const long long d = (long long)w - c;
            too_far = too_far || d < -32767 || d > 32767;
            nbr_t[b0 + (long long)q * kWave + lane] = (OUT)d;
        } else {
            nbr_t[b0 + (long long)q * kWave + lane] = (OUT)w;
        }
    }
    if (too_far)
        atomicOr(wide, 1u);
    if (lane == 0)
        guni[g] = uniform ? 1 : 0;
}

// Ring ends per target, level-major, so that the lane-per-target kernel reads them coalesced
// (the CSR rows of lvl_off are levels + 1 ints apart).
__global__ __launch_bounds__(kBlock) void k_transpose_off(const int32_t *lvl_off, int32_t *rel_t, int T, int levels)
{
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= T)
        return;
    const int32_t *o = lvl_off + (size_t)t * (levels + 1);
    for (int l = 0; l < levels; l++)
        rel_t[(size_t)l * T + t] = o[l + 1] - o[0];
}

// Is the neighbour relation symmetric?  True when every well is a centre (target t's centre is centre[0] + t),
// every ring lists its wells in strictly ascending order (what the generators write) and b is in ring r of a
// exactly when a is in ring r of b - what rings cut out of distances give.  The dense path then compares
// every pair once, from its lower well, and records a duplicate at both ends (DenseArgs::sym); anything
// else keeps the two-ended compare.  No ring may be empty either (:249 - such a target is not valid, and
// the one-ended compare does not look).  One thread per target: its own rings in order, then a binary
// search for its centre in the matching ring of every neighbour.
__global__ __launch_bounds__(kBlock) void k_dense_symcheck(const int32_t *centre, const int32_t *lvl_off, const int32_t *nbr,
                                                           int T, int levels, uint32_t *bad)
{
    const int t = blockIdx.x * kBlock + threadIdx.x;
    if (t >= T)
        return;
    const int c0 = centre[0], c = centre[t];
    bool ok = c == c0 + t;
    const int32_t *o = lvl_off + (size_t)t * (levels + 1);
    for (int l = 0; l < levels && ok; l++) {
        const int first = o[l], end = o[l + 1];
        ok = end > first;
        for (int i = first; i < end && ok; i++) {
            const int w = nbr[i];
            const long long t2 = (long long)w - c0;
            ok = w != c && t2 >= 0 && t2 < T && (i == first || nbr[i - 1] < w);
            if (!ok)
                break;
            // c in ring l of w (ascending: that ring is checked by w's own thread)
            const int32_t *o2 = lvl_off + (size_t)t2 * (levels + 1);
            int lo = o2[l], hi = o2[l + 1];              // [lo, hi)
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                const int v = nbr[mid];
                if (v < c)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            ok = lo < o2[l + 1] && nbr[lo] == c;
        }
    }
    if (!ok)
        *bad = 1u;
}

// Window groups.  On a grid the 64 consecutive centres of a group see nearly the same pattern of
// neighbours: the q-th neighbour of centre c sits at c + d for a small set of offsets d (one run
// of offsets per row of the ring pattern), though not every centre has every offset (pixel
// rounding moves wells in and out of the outermost ring from one column to the next, and groups
// straddle row ends).  For such a group this kernel builds, once per targets set:
//   - the UNION of the lanes' (ring, offset) pairs in (ring, offset) order - also the order of
//     every lane's own list, so lane i's slot of union element u is the number of its members
//     below u - and one membership bit per (lane, element).  (The same offset may sit in two
//     rings: the two row parities of a honeycomb see it at different distances.)
//                                                                              -> wdelta, wlev, wmask
//   - the runs of the union's offsets: for run [lo, hi] the wave needs the signatures of wells
//     c0 + lo .. c0 + 63 + hi, one contiguous stretch; the window is the runs one after the
//     other                                                                    -> useg
//   - where element u of lane 0 sits in that window (byte offset); lane i reads the dword at
//     uoff[u] + 4 i: an LDS read in place of a gather through L1               -> uoff
// One wave per group.  A group stays with the global gathers (ginfo = 0) when its centres are
// not consecutive or the union does
// not fit (more than kpad <= kWinMaxK elements, kMaxSeg runs or kWinDwords signatures).
__global__ __launch_bounds__(kWave) void k_dense_windows(const int32_t *centre, const int32_t *lvl_off,
                                                         const int32_t *nbr, int T, int levels, int kpad,
                                                         int32_t *ginfo, int2 *useg, uint16_t *uoff,
                                                         int32_t *wdelta, uint8_t *wlev, uint32_t *wmask, uint32_t *win_max,
                                                         int half, uint8_t *wfull)
{
    __shared__ int s_d[kWinMaxK];         // union, in order of discovery: offset
    __shared__ int s_lev[kWinMaxK];       // ... and ring
    __shared__ int s_rank[kWinMaxK];      // ... and position in (ring, offset) order
    __shared__ int s_sd[kWinMaxK];        // offsets in (ring, offset) order
    __shared__ int s_slev[kWinMaxK];      // ... and their rings
    __shared__ int s_lo[kWinMaxK];        // first offset of the run the element belongs to
    __shared__ int s_len[kWinMaxK];       // != 0 where the element opens a run: the run's length in dwords
    __shared__ int s_base[kWinMaxK];      // ... and where it starts in the window
    __shared__ uint32_t s_mask[(kWinMaxK / 32) * kWave];
    const int g = blockIdx.x, lane = threadIdx.x;
    const int t = g * kWave + lane;
    const bool in = t < T;                             // (a partial last group: the lanes past the last target have no neighbours)
    const int c0 = centre[g * kWave];
    const int c = in ? centre[t] : c0 + lane;
    if (!__all(c == c0 + lane))
        return;
    const int32_t *o = lvl_off + (size_t)(in ? t : T - 1) * (levels + 1);
    const int off0 = o[0];
    const int K = in ? o[levels] - off0 : 0;
    int kmax = K;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1)
        kmax = max(kmax, __shfl_xor(kmax, d));
    auto ring_of = [&](int q) {                        // 0-based ring of the lane's slot q
        int lev = 0;
        for (int l = 1; l < levels; l++)
            lev += (off0 + q >= o[l]) ? 1 : 0;
        return lev;
    };
    // ---- the union, one slot index at a time over all lanes ----
    int n = 0;
    for (int q = 0; q < kmax; q++) {
        const bool have = q < K;
        const int d = have ? nbr[off0 + q] - c : 0;
        const int lev = have ? ring_of(q) : 0;
        bool isnew = have;
        for (int e = 0; e < min(n, kpad); e++)
            if (have && s_d[e] == d && s_lev[e] == lev)
                isnew = false;
        uint64_t m = __ballot(isnew);
        while (m) {
            const int leader = __builtin_ctzll(m);
            const int dl = __shfl(d, leader), ll = __shfl(lev, leader);
            if (lane == 0 && n < kpad) {
                s_d[n] = dl;
                s_lev[n] = ll;
            }
            n++;
            isnew = isnew && !(d == dl && lev == ll);
            m = __ballot(isnew);
        }
        __syncthreads();
    }
    if (n > kpad || n == 0)
        return;
    // ---- (ring, offset) order ----
    for (int e = lane; e < n; e += kWave) {
        int r = 0;
        for (int f = 0; f < n; f++)
            r += (s_lev[f] < s_lev[e] || (s_lev[f] == s_lev[e] && s_d[f] < s_d[e])) ? 1 : 0;
        s_rank[e] = r;
        s_sd[r] = s_d[e];
        s_slev[r] = s_lev[e];
    }
    for (int w = 0; w < kpad / 32; w++)
        s_mask[w * kWave + lane] = 0;
    __syncthreads();
    // ---- membership: which union elements does this lane have ----
    bool in_order = true;                              // the lane's own list runs through the union upwards
    int u_prev = -1;
    for (int q = 0; q < K; q++) {
        const int d = nbr[off0 + q] - c, lev = ring_of(q);
        int u = 0;
        for (int e = 0; e < n; e++)
            u = (s_d[e] == d && s_lev[e] == lev) ? s_rank[e] : u;
        s_mask[(u >> 5) * kWave + lane] |= 1u << (u & 31);
        in_order = in_order && u > u_prev;
        u_prev = u;
    }
    // a ring that is not listed in ascending order of wells, or lists a well twice: the lane's slot
    // of an element is then not the number of its members below it - such a group keeps the gathers
    if (__any(!in_order))
        return;
    // ---- the elements the compare stage walks: all of them, or (half: every pair is seen from its lower
    // well) those above the centre, still in (ring, offset) order; s_full = their place in the whole union
    // (the membership words and a lane's slot numbers stay those of the whole union) ----
    __syncthreads();
    int *const s_hd = s_d, *const s_hlev = s_lev, *const s_full = s_rank;       // (the discovery-order tables are done with)
    const int n_all = n;
    {
        int keep_below[(kWinMaxK + kWave - 1) / kWave], keep[(kWinMaxK + kWave - 1) / kWave];
        int i = 0, mine = 0;
        for (int p = lane; p < n_all; p += kWave, i++) {
            keep[i] = (!half || s_sd[p] > 0) ? 1 : 0;
            int b = 0;
            for (int f = 0; f < p; f++)
                b += (!half || s_sd[f] > 0) ? 1 : 0;
            keep_below[i] = b;
            mine += keep[i];
        }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1)
            mine += __shfl_xor(mine, d);
        __syncthreads();                               // (s_rank was read by the membership loop above)
        i = 0;
        for (int p = lane; p < n_all; p += kWave, i++)
            if (keep[i]) {
                s_hd[keep_below[i]] = s_sd[p];
                s_hlev[keep_below[i]] = s_slev[p];
                s_full[keep_below[i]] = p;
            }
        n = mine;
    }
    __syncthreads();
    if (n == 0 || (half && n >= kpad))
        return;                                        // nothing above these centres: the gather kernel finds that out quickly
    for (int p = lane; p < n; p += kWave) {            // from here on s_sd / s_slev are the walked elements
        s_sd[p] = s_hd[p];
        s_slev[p] = s_hlev[p];
    }
    // half: the window also holds the centres' own signatures (offset 0, position n of the tables: the
    // compare stage then needs nothing from memory but its window)
    const int n_el = n;
    if (half) {
        if (lane == 0) {
            s_sd[n] = 0;
            s_slev[n] = 0;
            s_full[n] = 0;
        }
        n = n + 1;
    }
    __syncthreads();
    // ---- runs of the union's offsets (ring order no longer matters: positions p, f are arbitrary labels) ----
    for (int p = lane; p < n; p += kWave) {           // p opens a run: nothing within kWinGap below it
        const int d = s_sd[p];
        bool start = true;
        for (int f = 0; f < n; f++) {
            const int v = s_sd[f];
            if ((v < d && d - v <= kWinGap) || (v == d && f < p))
                start = false;
        }
        s_len[p] = start ? 1 : 0;
    }
    __syncthreads();
    for (int p = lane; p < n; p += kWave) {           // the run of p: the highest start not above it
        const int d = s_sd[p];
        int lo = INT32_MIN;
        for (int f = 0; f < n; f++)
            if (s_len[f] && s_sd[f] <= d && s_sd[f] > lo)
                lo = s_sd[f];
        s_lo[p] = lo;
    }
    __syncthreads();
    for (int p = lane; p < n; p += kWave) {           // its length: lane 0's first .. lane 63's last
        if (!s_len[p])
            continue;
        const int d = s_sd[p];
        int hi = d;
        for (int f = 0; f < n; f++)
            if (s_lo[f] == d)
                hi = max(hi, s_sd[f]);
        s_len[p] = kWave + hi - d;
    }
    __syncthreads();
    int nseg = 0, total = 0;
    for (int p = lane; p < n; p += kWave) {           // runs in ascending order of their first offset
        if (!s_len[p])
            continue;
        int base = 0, rank = 0;
        for (int f = 0; f < n; f++)
            if (s_len[f] && s_sd[f] < s_sd[p]) {
                base += s_len[f];
                rank++;
            }
        s_base[p] = base;
        nseg++;
        total += s_len[p];
        if (rank < kMaxSeg)
            useg[(size_t)g * kMaxSeg + rank] = make_int2(s_sd[p], (int)((uint32_t)base | ((uint32_t)s_len[p] << 16)));
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        nseg += __shfl_xor(nseg, d);
        total += __shfl_xor(total, d);
    }
    __syncthreads();
    if (nseg > kMaxSeg || total > kWinDwords)
        return;
    for (int p = lane; p < kpad; p += kWave) {
        int off = 0;
        if (p < n) {
            const int lo = s_lo[p];
            for (int f = 0; f < n; f++)
                if (s_len[f] && s_sd[f] == lo)
                    off = s_base[f] + s_sd[p] - lo;
        }
        uoff[(size_t)g * kpad + p] = (uint16_t)(off * 4);            // in bytes
        wdelta[(size_t)g * kpad + p] = p < n ? s_sd[p] : 0;
        wlev[(size_t)g * kpad + p] = (uint8_t)(p < n ? s_slev[p] : 0);
        wfull[(size_t)g * kpad + p] = (uint8_t)(p < n ? s_full[p] : 0);
    }
    for (int w = 0; w < kpad / 32; w++)
        wmask[((size_t)g * (kpad / 32) + w) * kWave + lane] = s_mask[w * kWave + lane];
    if (lane == 0) {
        ginfo[g] = n_el | (nseg << 9) | (total << 14);
        atomicMax(win_max, (uint32_t)total);
    }
}

// A duplicate found at level `lev` (0-based): Dups, the target's hit mask and what follows from
// its change, the optional per-target matrix and hit log.  Counter layout = out_tile row:
// [valid, wells[levels], dups[levels], hit[levels], first[levels], last[levels]].
// TALLY is either a global counter slot (64-bit adds) or a block's LDS copy of the last four
// groups (32-bit, signed deltas), flushed by the caller.
// ... in two steps, so that a caller with two targets to record for (dense_record_pair) has both mask
// atomics in flight before it looks at either answer: dense_mask_set returns the target's hit mask as it
// was, dense_record_with the rest.
__device__ inline uint32_t dense_mask_set(const DenseArgs &a, int tile, int t, int lev)
{
    const int sh = (t & 3) * 8;
    return (atomicOr(a.mask + (size_t)tile * a.mask_stride + (t >> 2), (1u << lev) << sh) >> sh) & 0xFFu;
}

template <typename TALLY>
__device__ inline void dense_record_with(const DenseArgs &a, TALLY *tally, int tile, int t, int q, int lev, int dist, uint32_t old)
{
    const int levels = a.levels;
    using V = TALLY;
    atomicAdd(&tally[lev], (V)1);
    if (!((old >> lev) & 1u)) {
        const uint32_t now = old | (1u << lev);
        atomicAdd(&tally[levels + lev], (V)1);
        const int f_old = old ? __ffs((int)old) - 1 : -1, f_new = __ffs((int)now) - 1;
        if (f_new != f_old) {
            atomicAdd(&tally[2 * levels + f_new], (V)1);
            if (f_old >= 0)
                atomicAdd(&tally[2 * levels + f_old], (V)~(V)0);           // -1 (mod 2^n)
        }
        const int l_old = old ? 31 - __clz((int)old) : -1, l_new = 31 - __clz((int)now);
        if (l_new != l_old) {
            atomicAdd(&tally[3 * levels + l_new], (V)1);
            if (l_old >= 0)
                atomicAdd(&tally[3 * levels + l_old], (V)~(V)0);
        }
    }
    if (a.out_per_target)
        atomicAdd(&a.out_per_target[((size_t)tile * a.T + t) * levels + lev], 1u);
    if (a.log_hits) {
        // (global address space throughout: the pointers inside ScanRare come out of memory, and one flat
        // access anywhere in a kernel turns every wait on a load into vmcnt(0) - as_gptr, device_common.inc)
        gptr<const ScanRare> rp = as_gptr(a.rare);
        wd_hit *const hits = rp->hits;
        const long long hit_cap = rp->hit_cap;
        const unsigned long long h = g_atomic_add(rp->hit_count, 1ull);
        if ((long long)h < hit_cap) {
            gptr<int32_t> rec = (gptr<int32_t>)as_gptr(hits + h);     // wd_hit: {tile, target, slot, dist}
            rec[0] = a.tile0 + tile;
            rec[1] = t;
            rec[2] = a.lvl_off[(size_t)t * (levels + 1)] + q;
            rec[3] = dist;
        }
    }
}

template <typename TALLY>
__device__ inline void dense_record(const DenseArgs &a, TALLY *tally, int tile, int t, int q, int lev, int dist)
{
    dense_record_with(a, tally, tile, t, q, lev, dist, dense_mask_set(a, tile, t, lev));
}

// the Dups.. part of target t's global counter slot
__device__ inline unsigned long long *dense_slot(const DenseArgs &a, int tile, int t)
{
    return a.partial + ((size_t)tile * kDenseSlots + (t & (kDenseSlots - 1))) * a.partial_stride + 1 + a.levels;
}

// Pairs seen from one end (DenseArgs::sym): the pair (centre c of target t, well w > c in t's ring `lev`,
// slot q) is a duplicate at distance `dist`.  It counts for t if t's centre passes the filter, and for the
// target whose centre is w - which lists c in the same ring of ITS (the host checked that the neighbour
// relation is symmetric: k_dense_symcheck) - if w passes, instead of being compared for a second time from
// the other end.
template <typename TALLY_T, typename TALLY_W>
__device__ inline void dense_record_pair(const DenseArgs &a, TALLY_T *tally_t, TALLY_W tally_w, int tile, int t, uint32_t c,
                                         int q, int lev, uint32_t w, int dist)
{
    gbytes filt = as_global(a.filter[tile]);
    const uint32_t fc = filt[c], fw = filt[w];                                 // (both in flight)
    const bool rec_t = fc & 1u, rec_w = fw & 1u;                               // :236-237
    const int t2 = (int)w - a.centre0;
    // both targets' mask atomics go out before either answer is looked at
    const uint32_t old_t = rec_t ? dense_mask_set(a, tile, t, lev) : 0u;
    const uint32_t old_w = rec_w ? dense_mask_set(a, tile, t2, lev) : 0u;
    if (rec_t)
        dense_record_with(a, tally_t, tile, t, q, lev, dist, old_t);
    if (rec_w) {
        // (c sits in the same ring of w as w in c's: k_dense_symcheck; its slot there is only the hit log's business)
        int q2 = 0;
        if (a.log_hits) {
            const int32_t *o = a.lvl_off + (size_t)t2 * (a.levels + 1);
            const int first = o[lev], end = o[lev + 1];
            for (int i = first; i < end; i++)
                q2 = (uint32_t)a.nbr[i] == c ? i - o[0] : q2;
        }
        dense_record_with(a, tally_w(t2), tile, t2, q2, lev, dist, old_w);
    }
}

// s_waitcnt vmcnt(n) for a wave-uniform n known at run time (the instruction takes an immediate).
__device__ inline void wait_vmcnt(int n)
{
#ifdef WD_EMU
    emu_dma_wait(n < 48 ? n : 48);
#else
#define WD_VM(N) case N: asm volatile("s_waitcnt vmcnt(" #N ")" ::: "memory"); break;
#define WD_VM8(B) WD_VM(B) WD_VM(B + 1) WD_VM(B + 2) WD_VM(B + 3) WD_VM(B + 4) WD_VM(B + 5) WD_VM(B + 6) WD_VM(B + 7)
    switch (n) {
    WD_VM(0) WD_VM(1) WD_VM(2) WD_VM(3) WD_VM(4) WD_VM(5) WD_VM(6) WD_VM(7)
    WD_VM(8) WD_VM(9) WD_VM(10) WD_VM(11) WD_VM(12) WD_VM(13) WD_VM(14) WD_VM(15)
    WD_VM(16) WD_VM(17) WD_VM(18) WD_VM(19) WD_VM(20) WD_VM(21) WD_VM(22) WD_VM(23)
    WD_VM(24) WD_VM(25) WD_VM(26) WD_VM(27) WD_VM(28) WD_VM(29) WD_VM(30) WD_VM(31)
    WD_VM(32) WD_VM(33) WD_VM(34) WD_VM(35) WD_VM(36) WD_VM(37) WD_VM(38) WD_VM(39)
    WD_VM(40) WD_VM(41) WD_VM(42) WD_VM(43) WD_VM(44) WD_VM(45) WD_VM(46) WD_VM(47)
    WD_VM(48)
    default: asm volatile("s_waitcnt vmcnt(48)" ::: "memory"); break;     // (waits for more than asked: never wrong)
    }
#undef WD_VM8
#undef WD_VM
#endif
}

// 64 dwords from global memory straight into LDS (LDS-DMA): lane i's dword at base + voff goes to LDS byte
// address lds + 4 i.  Through inline assembly on purpose: the compiler makes every LDS read that follows a
// __builtin_amdgcn_global_load_lds wait for it (vmcnt(0)) - it cannot tell the windows apart - and that
// turned the compare stage's "loads two tiles ahead" into a full round trip per tile.  The waits are the
// caller's (wait_vmcnt); `base` must be wave-uniform.
__device__ inline void lds_dma_dword(const void *base, uint32_t voff, uint32_t lds)
{
#ifdef WD_EMU
    emu_dma_issue(base, voff, lds);
#else
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2" : : "s"(lds), "v"(voff), "s"(base) : "memory");
#endif
}

// sum over the wave's lanes (wave-uniform result): an inclusive scan inside each row of 16 lanes
// by DPP shifts (lanes without a source add 0), then row sums handed on with row_bcast
__device__ inline uint32_t wave_sum(uint32_t v)
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);     // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);     // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);     // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);     // row_shr:8: lane 15 of a row = its sum
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);    // row_bcast:15 into rows 1 and 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);    // row_bcast:31 into rows 2 and 3
    return (uint32_t)__builtin_amdgcn_readlane((int)v, kWave - 1);
}

// Targets, Wells and the per-target output's initial state: what a tile's report needs of a target
// besides its duplicates depends only on the centre's filter byte (count_well_duplicates.py:236-237)
// and the ring sizes.  One thread takes 4 targets through `tile_chunk` tiles (ring sizes stay in
// registers, eight tiles' filter bytes are in flight together); the sums travel as 16-bit fields,
// two to a word.  Also raises the empty-ring assertion (:249); the compare kernels only skip
// such targets.
__global__ __launch_bounds__(kBlock) void k_dense_counts(DenseArgs a)
{
    const int levels = a.levels;
    const int lane = threadIdx.x & (kWave - 1);
    const int tile0 = blockIdx.y * a.tile_chunk;
    const int n_tl = min(a.tile_chunk, a.n_tiles - tile0);
    uint32_t c[4], pk[4][4];                           // centre; ring sizes, two 16-bit fields per word
    bool in[4], empty[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int t = (blockIdx.x * 4 + j) * kBlock + threadIdx.x;
        in[j] = t < a.T;
        c[j] = in[j] ? (uint32_t)a.centre[t] : 0u;
        empty[j] = false;
        int prev = 0;
#pragma unroll
        for (int h = 0; h < 4; h++)
            pk[j][h] = 0;
        // (every ring end asked for before the first is looked at: as a loop over `levels` each load was
        // waited for in turn, a dozen round trips one after the other for a thread's four targets)
        int endv[8];
#pragma unroll
        for (int l = 0; l < 8; l++)
            endv[l] = (in[j] && l < levels) ? a.rel_t[(size_t)l * a.T + t] : 0;
#pragma unroll
        for (int l = 0; l < 8; l++) {
            if (l < levels) {
                const int end = endv[l];
                pk[j][l >> 1] |= (uint32_t)(end - prev) << (16 * (l & 1));
                empty[j] = empty[j] || (in[j] && end <= prev);
                prev = end;
            }
        }
        empty[j] = empty[j] && a.check_empty;
    }
    constexpr int TB = 8;                              // tiles whose filter bytes are in flight together
    for (int tb = 0; tb < n_tl; tb += TB) {
        uint32_t f[TB][4];
#pragma unroll
        for (int i = 0; i < TB; i++) {
            gbytes filt = (gbytes)((const __attribute__((address_space(4))) unsigned long long *)a.filter)[tile0 + min(tb + i, n_tl - 1)];
#pragma unroll
            for (int j = 0; j < 4; j++)
                f[i][j] = filt[c[j]];
        }
#pragma unroll
        for (int i = 0; i < TB; i++) {
            if (tb + i >= n_tl)
                break;
            const int tile = tile0 + tb + i;
            uint32_t n_valid = 0, sum[4] = {0, 0, 0, 0};   // 4 targets x <= 128 wells x 64 lanes < 2^16 per field
#pragma unroll
            for (int j = 0; j < 4; j++) {
                bool valid = in[j] && (f[i][j] & 1u);
                if (valid && empty[j]) {
                    g_atomic_or(as_gptr(a.rare)->status, kStatusEmptyLevel);
                    valid = false;
                }
                if (a.out_per_target && in[j]) {
                    const int t = (blockIdx.x * 4 + j) * kBlock + threadIdx.x;
                    uint32_t *opt = a.out_per_target + ((size_t)tile * a.T + t) * levels;
                    for (int l = 0; l < levels; l++)
                        opt[l] = valid ? 0u : WD_INVALID_TARGET;
                }
                n_valid += valid ? 1u : 0u;
#pragma unroll
                for (int h = 0; h < 4; h++)
                    sum[h] += valid ? pk[j][h] : 0u;
            }
            // the wave's sums, straight to the tile's counter slot (one lane per counter)
            n_valid = wave_sum(n_valid);
            uint32_t mine = n_valid;
#pragma unroll
            for (int h = 0; h < 4; h++)
                if (2 * h < levels) {
                    const uint32_t s2 = wave_sum(sum[h]);
                    mine = lane == 1 + 2 * h ? (s2 & 0xFFFFu) : lane == 2 + 2 * h ? (s2 >> 16) : mine;
                }
            if (lane <= levels && mine) {
                unsigned long long *slot = a.partial + ((size_t)tile * kDenseSlots + ((blockIdx.x * kWaves + (threadIdx.x >> 6)) & (kDenseSlots - 1))) * a.partial_stride;
                atomicAdd(&slot[lane], (unsigned long long)mine);
            }
        }
    }
}

// The compare stage of the dense path for window groups (k_dense_windows).  One wave = one group
// of 64 consecutive centres, taken through `tile_chunk` tiles: the group's tables are read once,
// and everything a tile needs from memory - the centres' filter bytes and signatures and the
// window of neighbouring signatures, copied into LDS by LDS-DMA in pieces of 64 - is requested two
// tiles ahead.  Per tile the wave then does nothing but LDS reads and compares: lane i finds union
// element u at window[uoff[u] + 4 i].  Waves are independent (own windows, own survivor queue in
// LDS, own queue region in global memory): no barrier anywhere.
// Written for few instructions per (target, element): the first version spent 600 scalar and 400
// vector instructions per wave and tile and was bound by instruction issue (the scalar unit is
// shared by the CU's four SIMDs), not by LDS or memory.  Hence: the tile-invariant source offsets
// of the window pieces stay in registers (a piece costs three instructions), the compare loop
// is unrolled so that every lane select is an immediate, passes are found with vector min
// instead of scalar mask logic, nothing on the way of a survivor loads from memory, and the
// per-tile counts are left to k_dense_counts.
// MODE 0: equality, 1: Hamming <= k, 2: Levenshtein <= 2
// SYM: pairs are seen from their lower well only - the tables list the union's elements above the
// centre (half the compares, half the window), a lane compares whatever its own filter byte says (the
// pair may count for the other well), and k_dense_verify records a duplicate at both ends.
// NPC > 0 (SYM only): every wave asks for exactly NPC pieces of 64 signatures per tile (the launch's window
// size: a group with a smaller window reads its centres' signatures again) into one of kWinBufsSym windows -
// the counted waits are immediates then and the issue loop has no scalar test per piece.
template <int MODE, bool SYM, int NPC = 0>
__global__ __launch_bounds__(kBlock) void k_dense_pairs_win(DenseArgs a)
{
    static_assert(NPC == 0 || SYM, "fixed piece counts belong to the one-ended compare");
    WD_DYNAMIC_LDS(s_dyn);                               // per wave: kWinBufs windows, then the survivor queue
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int levels = a.levels;
    const int k = a.k;
    // per wave: kWinBufs windows, one survivor queue per tile of the chunk, their entry counts
    // (dense_per_wave_dwords, dense_launch.inc, written out: through the function the compiler adds the three terms in
    // another order.  The CPU emulation's LDS block has the host's bytes exactly, so a difference is a sanitizer report.)
    const int per_wave = a.win_bufs * a.win_dwords + a.tile_chunk * (2 * a.q_per + 1) + (a.tile_chunk & 1);
    uint32_t *s_win = s_dyn + wave * per_wave;
    uint2 *s_q_all = (uint2 *)(s_win + a.win_bufs * a.win_dwords);
    uint32_t *s_nq = (uint32_t *)(s_q_all + a.tile_chunk * a.q_per);
    // Block -> (block of 256 targets, chunk of tiles), XCD x owning a contiguous range of target
    // blocks (workgroups are dealt round-robin to the 8 XCDs): blocks a few rows apart share
    // signature lines and run on the same L2 close in time.
    const int bpt = (a.T + kBlock - 1) / kBlock;
    const int gpx = (bpt + kXcds - 1) / kXcds;
    const int seq = blockIdx.x / kXcds;
    const int tblock = (int)(blockIdx.x % kXcds) * gpx + seq % gpx;
    const int tile0 = (seq / gpx) * a.tile_chunk;
    if (tile0 >= a.n_tiles || tblock >= bpt)
        return;
    const int n_tl = min(a.tile_chunk, a.n_tiles - tile0);
    const int groups = (a.T + kWave - 1) / kWave;
    const int grp = tblock * kWaves + wave;
    if (grp >= groups)
        return;                                          // (no barriers below: a wave may leave alone)
    const int gi = __builtin_amdgcn_readfirstlane(a.ginfo[grp]);
    if (gi == 0)
        return;                                          // a gather group: k_dense_pairs has it
    int Ku = gi & 0x1FF;
    const int nrun = (gi >> 9) & 31, total = gi >> 14;
    const int t = grp * kWave + lane;
    const bool in = t < a.T;                             // (the last group may be partial: its spare lanes compare nothing)
    const uint32_t c_ld = (uint32_t)a.centre[in ? t : grp * kWave];
    const uint32_t c0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)c_ld);       // lane i's centre is c0 + i
    const uint32_t c = in ? c_ld : c0;                   // (a spare lane loads what lane 0 loads)

    // ---- the group's tables, in registers for every tile ----
    // lane u holds what is known of union elements u and 64 + u: window offset (bytes), offset
    // from the centre, ring; every lane holds its own membership bits.  The loops below pick them
    // with v_readlane: no memory access and almost no scalar instruction between a compare and
    // the next, and none at all on the way of a survivor into the queue.
    uint32_t off_b0 = 0, off_b1 = 0, lev_v = 0, mk[kWinMaxK / 32] = {0, 0, 0, 0};
    int dl_0 = 0, dl_1 = 0;
    static_assert(kWinMaxK == 128, "four membership words, two registers per element table");
    {
        const size_t row = (size_t)grp * a.kpad;
        if (lane < a.kpad) {
            off_b0 = a.uoff[row + lane];
            dl_0 = a.wdelta[row + lane];
            lev_v = a.wlev[row + lane];
            if (SYM)                                     // (bits 16..: the element's place in the whole union)
                lev_v |= (uint32_t)a.wfull[row + lane] << 16;
        }
        if (kWave + lane < a.kpad) {
            off_b1 = a.uoff[row + kWave + lane];
            dl_1 = a.wdelta[row + kWave + lane];
            lev_v |= (uint32_t)a.wlev[row + kWave + lane] << 8;
            if (SYM)
                lev_v |= (uint32_t)a.wfull[row + kWave + lane] << 24;
        }
#pragma unroll
        for (int w = 0; w < kWinMaxK / 32; w++)
            if (w < a.kpad / 32)
                mk[w] = a.wmask[((size_t)grp * (a.kpad / 32) + w) * kWave + lane];
    }
    bool empty = !in;                                    // a ring of this target is empty (:249): k_dense_counts reports it
    if (a.check_empty && in) {
        int prev = 0;
        for (int l = 0; l < levels; l++) {
            const int end = a.rel_t[(size_t)l * a.T + t];
            empty = empty || end <= prev;
            prev = end;
        }
    }
    // source of window dword 64 j + lane, as a byte offset into the tile's signatures: the runs one
    // after the other; dwords past the window's end, and wells outside the tile (a union element of
    // another lane may point there for this one), read the centre's own signature instead
    constexpr int NJ = NPC > 0 ? NPC : kWinDwords / kWave;
    int n_pc = NPC > 0 ? NPC : (total + kWave - 1) / kWave;            // pieces of 64 dwords
    uint32_t src_b[NJ];
    {
        // (the runs are in ascending order of their place in the window: dword i belongs to the
        // last run that starts at or before it)
        const int2 run_v = lane < nrun ? a.useg[(size_t)grp * kMaxSeg + lane] : make_int2(0, 0);
        int shift[NJ];                                 // source offset of dword i = i + shift
#pragma unroll
        for (int j = 0; j < NJ; j++)
            shift[j] = 0;
        for (int r = 0; r < nrun; r++) {
            const int lo = __builtin_amdgcn_readlane(run_v.x, r);
            const int base = (int)((uint32_t)__builtin_amdgcn_readlane(run_v.y, r) & 0xFFFFu);
#pragma unroll
            for (int j = 0; j < NJ; j++)
                if (j < n_pc)
                    shift[j] = j * kWave + lane >= base ? lo - base : shift[j];
        }
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const int i = j * kWave + lane;
            const uint32_t w = c0 + (uint32_t)(i + shift[j]);
            src_b[j] = ((i < total && w < (uint32_t)a.N) ? w : c) << 2;
        }
    }

    // ---- per tile: loads issued two tiles ahead ----
    // Order inside the loop: compare tile i (registers and LDS only) -> wait for everything in
    // flight (the loads of tile i + 1, issued a whole compare phase ago, and the stores of tile
    // i - 1) -> issue the loads of tile i + 2 into the window tile i has just finished with ->
    // write out tile i's results.  The memory counter retires in order, so the one wait per tile
    // never waits for anything issued less than a compare phase ago.  (The filter pointers come
    // through the scalar cache: a vector load of the pointer would be one more wait.)
    using cptr = const __attribute__((address_space(4))) unsigned long long *;
    uint32_t f_ld = 0, sig_ld = 0;                     // destinations of the loads in flight
    auto issue = [&](int tile, int buf) {              // everything tile `tile` needs from memory
        gbytes filt = (gbytes)((cptr)a.filter)[tile];
        gsig sg = (gsig)((MODE != 0 ? a.sig2 : a.sig) + (size_t)tile * a.sig_stride);    // distances > 0: the screen words
        f_ld = SYM ? 1u : (uint32_t)filt[c];            // (SYM: the filter bytes of both ends are k_dense_verify's business)
        sig_ld = sg[c];
        const uint32_t dst = WD_LDS_ADDR(s_win + buf * a.win_dwords);
        // (opaque: or the compiler evaluates the 16 comparisons once, before the tile loop, and
        // keeps them in spilled registers)
        WD_PIN("+s"(n_pc));
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            if (j >= n_pc)
                break;
            // (not the builtin: the compiler would make the next tile's first LDS read wait for these)
            lds_dma_dword((const void *)sg, src_b[j], dst + (uint32_t)j * (kWave * 4u));
        }
    };
    // SYM: the centre's own signature is in the window too (table position Ku), so a tile costs n_pc LDS-DMA
    // loads and nothing else; they go out through inline assembly (lds_dma_dword) with counted waits, the
    // windows of the next `ahead` tiles in flight while this one is compared
    const int n_bufs = NPC > 0 ? kWinBufsSym : a.win_bufs, ahead_max = n_bufs - 1;
    const uint32_t lds0 = WD_LDS_ADDR(s_win);
    const uint32_t own_off = SYM ? (uint32_t)__builtin_amdgcn_readlane((int)(Ku < kWave ? off_b0 : off_b1), Ku & 63) : 0u;
    auto issue_sym = [&](int tile, int buf) {
        const char *sgb = (const char *)((MODE != 0 ? a.sig2 : a.sig) + (size_t)tile * a.sig_stride);
        const uint32_t dst = lds0 + (uint32_t)(buf * a.win_dwords) * 4u;
        if (NPC == 0)
            WD_PIN("+s"(n_pc));
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            if (NPC == 0 && j >= n_pc)
                break;
            lds_dma_dword(sgb, src_b[j], dst + (uint32_t)j * (kWave * 4u));
        }
    };
    uint32_t f_cur = 1u, csig = 0u;
    int buf = 0;                                         // SYM: the window of the tile being compared
    if constexpr (SYM) {
        for (int d = 0; d < ahead_max && d < n_tl; d++)
            issue_sym(tile0 + d, d);
    } else {
        issue(tile0, 0);
        WD_WAIT_VM0();
        f_cur = f_ld;
        csig = sig_ld;
        if (n_tl > 1)
            issue(tile0 + 1, 1);
    }
    for (int ti = 0; ti < n_tl; ti++) {
        const int tile = tile0 + ti;
        if constexpr (SYM) {
            // tiles ti .. min(ti + ahead_max, n_tl) - 1 have been asked for; this one must have landed
            if constexpr (NPC > 0) {
                // (kWinBufsSym - 2 tiles' windows stay in flight behind the one waited for)
                constexpr int A = kWinBufsSym - 2;
                static_assert(A == 1 || A == 2, "one or two tiles behind");
                const int rem = n_tl - ti - 1;
                if (rem >= A)
                    WD_WAIT_VM_N(A * NPC);
                else if (A == 2 && rem == 1)
                    WD_WAIT_VM_N(NPC);
                else
                    WD_WAIT_VM0();
            } else {
                wait_vmcnt((min(ti + ahead_max, n_tl) - ti - 1) * n_pc);
            }
            // (the control: tile ti + ahead_max asked for one window early - into the window this tile is about to be compared in)
            WD_DENSE_CONTROL(early_issue, if (ti + ahead_max < n_tl) issue_sym(tile + ahead_max, buf));
            csig = *(const uint32_t *)((const char *)(s_win + buf * a.win_dwords + lane) + own_off);
        }
        const bool valid = (f_cur & 1u) != 0 && !empty;                    // :236-237
        uint32_t n_q = 0;                                // survivors of this wave and tile (wave-uniform)
        uint2 *s_q = s_q_all + ti * a.q_per;             // they stay in LDS until the wave has done all its tiles
        const uint32_t csig_h = csig >> 2, csig_l = csig << 2;             // (Levenshtein screen)
        auto mismatches = [&](uint32_t w) -> uint32_t {      // Levenshtein: 0 = may be a duplicate (k_dense_verify decides)
            return MODE == 0 ? w ^ csig : MODE == 1 ? screen_mismatches(w, csig) : lev2_screen(csig, csig_h, csig_l, w);
        };
        if (__ballot(valid) != 0) {
            const char *win_l = (const char *)(s_win + (SYM ? buf : ti % kWinBufs) * a.win_dwords + lane);    // this lane's column
            // (the tables are the same for every tile: opaque, or the compiler reads all lanes out
            // once, before the tile loop, and keeps them in spilled scalar registers)
            WD_PIN("+v"(off_b0), "+v"(off_b1), "+s"(Ku));
            WD_PIN("+v"(dl_0), "+v"(dl_1), "+v"(lev_v), "+v"(mk[0]), "+v"(mk[1]), "+v"(mk[2]), "+v"(mk[3]));
            // fully unrolled over chunks of 8 elements, so that every lane select below is an
            // immediate: per element one v_readlane, one v_add, one ds_read_b32 and the compare.
            // (Elements past the union's end read the window's first dwords, and membership is only
            // looked at when some lane of the chunk passes: a pass there costs a look, never a count.)
#pragma unroll
            for (int ch = 0; ch < kWinMaxK / 8; ch++) {
                if (ch * 8 >= Ku)
                    break;
                const uint32_t ov = ch < 8 ? off_b0 : off_b1;
                uint32_t sc[8];
#pragma unroll
                for (int u = 0; u < 8; u++)
                    sc[u] = mismatches(*(const uint32_t *)(win_l + (uint32_t)__builtin_amdgcn_readlane((int)ov, (ch * 8 + u) & 63)));
                uint32_t best = ~0u;                  // vector min instead of scalar mask logic
#pragma unroll
                for (int u = 0; u < 8; u++)
                    best = min(best, sc[u]);
                const uint32_t thr = MODE == 1 ? (uint32_t)k : MODE == 2 ? 1u : 0u;
                if (__ballot(valid && best <= thr) == 0)
                    continue;
                // ---- a survivor in this chunk (rare): its elements one by one, now with membership ----
                if constexpr (SYM) {
                    // (the membership words are those of the whole union: an element's place there comes
                    // with its ring, wave-uniform)
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        constexpr uint32_t one = 1u;
                        const int el = ch * 8 + u;
                        if (el >= Ku)
                            break;
                        if (__ballot(sc[u] <= thr) == 0)     // (at 2 % duplicates every other chunk comes here: look
                            continue;                        // at an element's tables only if some lane passes on it)
                        const uint32_t lv = (uint32_t)__builtin_amdgcn_readlane((int)lev_v, el & 63);
                        const uint32_t lev = (lv >> (el < kWave ? 0 : 8)) & 0xFFu;
                        const int uf = (int)((lv >> (el < kWave ? 16 : 24)) & 0xFFu);
                        const int word = uf >> 5, bit = uf & 31;
                        const uint32_t mkw = word == 0 ? mk[0] : word == 1 ? mk[1] : word == 2 ? mk[2] : mk[3];
                        const bool alive = valid && ((mkw >> bit) & one) && sc[u] <= thr;
                        const uint64_t m = __ballot(alive);
                        if (m == 0)
                            continue;
                        const int before = (word > 0 ? __popc(mk[0]) : 0) + (word > 1 ? __popc(mk[1]) : 0) +
                                           (word > 2 ? __popc(mk[2]) : 0);
                        const int dlt = __builtin_amdgcn_readlane(el < kWave ? dl_0 : dl_1, el & 63);
                        if (alive) {
                            const uint32_t p = n_q + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                         __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                            if (p < (uint32_t)a.q_per)
                                s_q[p] = make_uint2(c + (uint32_t)dlt,
                                                    ((uint32_t)lane << 24) | ((MODE == 1 ? sc[u] : 0u) << 20) | (lev << 17) |
                                                        (uint32_t)(before + __popc(mkw & ((one << bit) - one))));
                        }
                        n_q += (uint32_t)__popcll(m);
                    }
                    continue;
                }
                const uint32_t mkw = mk[ch / 4];
                const int before = (ch / 4 > 0 ? __popc(mk[0]) : 0) + (ch / 4 > 1 ? __popc(mk[1]) : 0) +
                                   (ch / 4 > 2 ? __popc(mk[2]) : 0);         // the lane's members in earlier words
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    constexpr uint32_t one = 1u;
                    const int el = ch * 8 + u, bit = el & 31;
                    const bool alive = valid && ((mkw >> bit) & one) && sc[u] <= thr && el < Ku;
                    const uint64_t m = __ballot(alive);
                    if (m == 0)
                        continue;
                    const int dlt = __builtin_amdgcn_readlane(el < kWave ? dl_0 : dl_1, el & 63);
                    const uint32_t lev = ((uint32_t)__builtin_amdgcn_readlane((int)lev_v, el & 63) >> (el < kWave ? 0 : 8)) & 0xFFu;
                    if (alive) {
                        const uint32_t p = n_q + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                     __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                        if (p < (uint32_t)a.q_per)
                            s_q[p] = make_uint2(c + (uint32_t)dlt,       // slot: the lane's members before this one
                                                ((uint32_t)lane << 24) | ((MODE == 1 ? sc[u] : 0u) << 20) | (lev << 17) |
                                                    (uint32_t)(before + __popc(mkw & ((one << bit) - one))));
                    }
                    n_q += (uint32_t)__popcll(m);
                }
            }
        }

        // ---- the next tile's inputs have landed; start the loads of the one after ----
        uint32_t f_nxt = 1u, sig_nxt = 0u;
        if constexpr (SYM) {
            // the window the tile before this one was compared in is free: tile ti + ahead_max goes there
            if (ti + ahead_max < n_tl)
                issue_sym(tile + ahead_max, buf + ahead_max >= n_bufs ? buf + ahead_max - n_bufs : buf + ahead_max);
        } else {
            WD_WAIT_VM0();
            f_nxt = f_ld;
            sig_nxt = sig_ld;
            // (the copies happen HERE: left alone the compiler moves them to the top of the next iteration,
            // behind the loads issued below, and waits for those before the compare)
            WD_PIN("+v"(f_nxt), "+v"(sig_nxt));
            if (ti + 2 < n_tl)
                issue(tile + 2, ti % kWinBufs);
        }

        // ---- survivors: nothing leaves the wave here.  A store or an atomic issued now would sit
        // in front of the next tile's wait (atomics stay in flight for ~3000 cycles on a busy chip:
        // marking in place made this kernel six times slower); the queues of all tiles go out after
        // the last one ----
        const size_t region = (size_t)tile * groups + grp;
        if (lane == 0)
            s_nq[ti] = n_q <= (uint32_t)a.q_per ? n_q : 0xFFFFFFFFu;
        if (n_q > (uint32_t)a.q_per) {
            WD_DENSE_NOTE(overflow_win);
            // More survivors than the region holds (low-diversity reads).  Levenshtein: leave the
            // whole group to k_dense_verify, which then needs the packed rows of all its wells;
            // otherwise finish every pair of this group here, one lane per target, cycle by cycle.
            if (lane == 0) {
                a.q_cnt[region] = MODE == 2 ? 0xFFFFFFFFu : 0u;
                if (MODE == 2 && a.L > a.sig_cycles)
                    a.cand[kDenseSlots] = 1u;
            }
            if (MODE == 2 && a.rows != nullptr && a.L > a.sig_cycles && valid)
                dense_mark(a, tile, c);
            gsig sg = (gsig)(a.sig + (size_t)tile * a.sig_stride);              // the exact signatures
            const uint32_t csig_x = MODE == 2 ? 0u : sg[c];
            int q = 0;
            for (int u = 0; u < Ku; u++) {
                const int uf = SYM ? (int)a.wfull[(size_t)grp * a.kpad + u] : u;  // the element's place in the whole union
                const uint32_t mkw = (uf >> 5) == 0 ? mk[0] : (uf >> 5) == 1 ? mk[1] : (uf >> 5) == 2 ? mk[2] : mk[3];
                if (!(valid && ((mkw >> (uf & 31)) & 1u)))
                    continue;
                if (SYM)                                 // the slot: the lane's members below it in the whole union
                    q = ((uf >> 5) > 0 ? __popc(mk[0]) : 0) + ((uf >> 5) > 1 ? __popc(mk[1]) : 0) +
                        ((uf >> 5) > 2 ? __popc(mk[2]) : 0) + __popc(mkw & ((1u << (uf & 31)) - 1u));
                const uint32_t w_i = c + (uint32_t)a.wdelta[(size_t)grp * a.kpad + u];
                if (MODE == 2) {
                    if (a.rows != nullptr && a.L > a.sig_cycles)
                        dense_mark(a, tile, w_i);
                } else {
                    int mm = sig_mismatches(sg[w_i], csig_x);
                    for (int j = a.sig_cycles; j < a.L && mm <= k; j++) {
                        gbytes p_j = dense_plane(a, tile, j);
                        mm += code_of(p_j[w_i]) != code_of(p_j[c]) ? 1 : 0;
                    }
                    if (mm <= k) {
                        const int lev = (int)a.wlev[(size_t)grp * a.kpad + u];
                        if (SYM)
                            dense_record_pair(a, dense_slot(a, tile, t), [&](int t2) { return dense_slot(a, tile, t2); },
                                              tile, t, c, q, lev, w_i, mm);
                        else
                            dense_record(a, dense_slot(a, tile, t), tile, t, q, lev, mm);
                    }
                }
                q++;
            }
        }
        if constexpr (SYM) {
            buf = buf + 1 == n_bufs ? 0 : buf + 1;
        } else {
            f_cur = f_nxt;
            csig = sig_nxt;
        }
    }
    // ---- every tile's survivors -> this group's regions of the global queue.  The Hamming family
    // marks the survivors' wells (they get packed rows) right here; Levenshtein survivors first pass
    // k_dense_mark's exact test ----
    WD_LOCKSTEP();
    for (int ti = 0; ti < n_tl; ti++) {
        const uint32_t n_q = s_nq[ti];
        if (n_q == 0xFFFFFFFFu)
            continue;                                    // overflowed: settled above
        const int tile = tile0 + ti;
        const size_t region = (size_t)tile * groups + grp;
        if ((uint32_t)lane < n_q) {
            const uint2 e = s_q_all[ti * a.q_per + lane];
            a.queue[region * a.q_per + lane] = e;
            if (MODE != 2 && a.rows != nullptr && a.L > a.sig_cycles) {
                dense_mark(a, tile, e.x);
                dense_mark(a, tile, c0 + (e.y >> 24));
            }
        }
        if (lane == 0) {
            a.q_cnt[region] = n_q;
            if (MODE != 2 && n_q)
                a.cand[0] = 1u;
        }
    }
}

constexpr int kDenseU = 4;            // neighbours per step of the gather pipeline (measured: 2 and 8 are slower)
// The compare stage of the dense path for gather groups (whatever k_dense_windows could not turn
// into a window group): one wave = one group of 64 targets, taken through `tile_chunk` tiles, the
// neighbours' signatures gathered through L1 (one index load and one signature load per target
// and neighbour, software-pipelined).  Same outputs and the same queue regions as
// k_dense_pairs_win; waves are independent, no barrier.
// MODE 0: equality, 1: Hamming <= k, 2: Levenshtein <= 2
// SYM: as in k_dense_pairs_win - only neighbours above the centre are taken up, whatever the filter says.
template <int MODE, bool IDX16, bool SYM>
__global__ __launch_bounds__(kBlock) void k_dense_pairs(DenseArgs a)
{
    WD_DYNAMIC_LDS(s_dyn);                               // per wave: kWinBufs windows, then the survivor queue
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int levels = a.levels;
    const int L = a.L;
    const int k = a.k;
    uint2 *s_q = (uint2 *)(s_dyn + wave * (a.win_bufs * a.win_dwords + a.tile_chunk * (2 * a.q_per + 1) + (a.tile_chunk & 1)) +
                           a.win_bufs * a.win_dwords);                     // (k_dense_pairs_win's LDS layout: its first queue)
    // Block -> (block of 256 targets, chunk of tiles).  Workgroups are dealt round-robin to the 8
    // XCDs, each with its own L2: XCD x owns a contiguous range of target blocks, so that blocks a
    // few rows apart - which share signature lines - run on the same XCD close in time.
    const int bpt = (a.T + kBlock - 1) / kBlock;
    const int gpx = (bpt + kXcds - 1) / kXcds;               // target blocks per XCD
    const int xcd = blockIdx.x % kXcds;
    const int seq = blockIdx.x / kXcds;
    const int tc = a.tile_chunk;
    // (launched over a list of target blocks when the window kernel has the others: launch_dense)
    const int tblock = a.n_pblocks > 0 ? a.pblocks[blockIdx.x % (unsigned)a.n_pblocks] : xcd * gpx + seq % gpx;
    const int tile0 = (a.n_pblocks > 0 ? (int)(blockIdx.x / (unsigned)a.n_pblocks) : seq / gpx) * tc;
    if (tile0 >= a.n_tiles || tblock >= bpt)
        return;
    const int n_tl = min(tc, a.n_tiles - tile0);
    const int groups = (a.T + kWave - 1) / kWave;
    const int grp_raw = tblock * kWaves + wave;
    if (grp_raw >= groups)
        return;                                          // (no barriers below: a wave may leave alone)
    const int grp = grp_raw;
    if (a.ginfo && __builtin_amdgcn_readfirstlane(a.ginfo[grp]) != 0)
        return;                                          // a window group: k_dense_pairs_win has it
    const int t = grp * kWave + lane;
    const bool in = t < a.T;

    // ---- this lane's target (the same for every tile) ----
    const uint32_t c = in ? (uint32_t)a.centre[t] : 0u;
    int rel[8];                                        // ring l+1 ends at slot rel[l] (levels <= 8)
#pragma unroll
    for (int l = 0; l < 8; l++)
        rel[l] = (in && l < levels) ? a.rel_t[(size_t)l * a.T + t] : 0x7FFFFFFF;
    bool empty = false;                                // :249
    if (a.check_empty) {
#pragma unroll
        for (int l = 0; l < 8; l++)
            empty = empty || (l < levels && rel[l] <= (l ? rel[l - 1] : 0));
    }
    int K_all = 0;
#pragma unroll
    for (int l = 0; l < 8; l++)
        K_all = (in && l == levels - 1) ? rel[l] : K_all;
    const int S = a.sig_cycles;

    // ---- the group's tables ----
    const long long gb_v = a.gbase[grp];
    const long long gb = ((long long)__builtin_amdgcn_readfirstlane((int)(gb_v >> 32)) << 32) |
                         (uint32_t)__builtin_amdgcn_readfirstlane((int)gb_v);
    const int gk = __builtin_amdgcn_readfirstlane((int)((a.gbase[grp + 1] - gb_v) >> 6));   // >= every K, >= 1
    using gidx16 = const __attribute__((address_space(1))) int16_t *;
    gidx nt = (gidx)((const int32_t *)a.nbr_t + (IDX16 ? 0 : gb));
    gidx16 nt16 = (gidx16)((const int16_t *)a.nbr_t + (IDX16 ? gb : 0));
    constexpr int U = kDenseU;                         // neighbours per step
    // gather path, uniform group: the q-th neighbour is centre + udelta[q] for every lane, so the
    // index stream of the group shrinks from 128-256 bytes per neighbour to one element
    const bool uni = __builtin_amdgcn_readfirstlane((int)a.guni[grp]) != 0;
    const long long ub = gb / kWave;
    gidx p32 = uni ? (gidx)((const int32_t *)a.udelta + (IDX16 ? 0 : ub)) : nt;
    gidx16 p16 = uni ? (gidx16)((const int16_t *)a.udelta + (IDX16 ? ub : 0)) : nt16;
    const int e_stride = uni ? 1 : kWave, e_lane = uni ? 0 : lane;
    const uint32_t c_add = (IDX16 || uni) ? c : 0u;
    auto ld_idx = [&](int q) -> uint32_t {             // own centre where q >= K
        const int e = min(q, gk - 1) * e_stride + e_lane;
        // streamed once: keep L1 for signatures
        return c_add + (IDX16 ? (uint32_t)(int)__builtin_nontemporal_load(p16 + e)
                              : (uint32_t)__builtin_nontemporal_load(p32 + e));
    };
    // ---- per tile: loads issued two tiles ahead ----
    // Order inside the loop: compare tile i (registers and LDS only) -> wait for everything in
    // flight (the loads of tile i + 1, issued a whole compare phase ago, and the stores of tile
    // i - 1) -> issue the loads of tile i + 2 into the window tile i has just finished with ->
    // write out tile i's results.  The memory counter retires in order, so the one wait per tile
    // never waits for anything issued less than a compare phase ago.
    uint32_t f_ld = 0, sig_ld = 0;                     // destinations of the loads in flight
    auto issue = [&](int tile, int buf) {              // everything tile `tile` needs from memory
        gbytes filt = (gbytes)((const __attribute__((address_space(4))) unsigned long long *)a.filter)[tile];   // (scalar cache)
        gsig sg = (gsig)((MODE != 0 ? a.sig2 : a.sig) + (size_t)tile * a.sig_stride);    // distances > 0: the screen words
        f_ld = (in && !SYM) ? (uint32_t)filt[c] : 0u;
        sig_ld = sg[c];
    };
    issue(tile0, 0);
    WD_WAIT_VM0();
    uint32_t f_cur = f_ld, csig = sig_ld;
    if (n_tl > 1)
        issue(tile0 + 1, 1);
    for (int ti = 0; ti < n_tl; ti++) {
        const int tile = tile0 + ti;
        const bool valid = in && (SYM || (f_cur & 1u)) && !empty;          // :236-237, :249 (k_dense_counts reports it)
        const int K = valid ? K_all : 0;
        gsig sg = (gsig)((MODE != 0 ? a.sig2 : a.sig) + (size_t)tile * a.sig_stride);
        int kmax = K;                                     // wave-wide trip count
#pragma unroll
        for (int d = 32; d > 0; d >>= 1)
            kmax = max(kmax, __shfl_xor(kmax, d));
        kmax = __builtin_amdgcn_readfirstlane(kmax);
        uint32_t n_q = 0;                                // survivors of this wave and tile (wave-uniform)
        // A survivor of the signature goes to the wave's LDS queue: nothing but loads and LDS
        // traffic inside the compare loops, so the compiler's counted waits stay exact (a global
        // store or atomic on a rare path makes it wait for everything on every trip).
        auto push = [&](bool alive, uint32_t idx, int q, int mm) {
            const uint64_t m = __ballot(alive);
            if (m == 0)
                return;
            if (alive) {
                const uint32_t p = n_q + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                             __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                if (p < (uint32_t)a.q_per) {
                    uint32_t lev = 0;
#pragma unroll
                    for (int l = 0; l < 7; l++)
                        lev += (l < levels - 1 && q >= rel[l]) ? 1u : 0u;
                    s_q[p] = make_uint2(idx, ((uint32_t)lane << 24) | ((uint32_t)mm << 20) | (lev << 17) | (uint32_t)q);
                }
            }
            n_q += (uint32_t)__popcll(m);
        };
        const uint32_t csig_h = csig >> 2, csig_l = csig << 2;             // (Levenshtein screen)
        auto passes = [&](uint32_t w) -> bool {
            return MODE == 0 ? w == csig : MODE == 1 ? screen_mismatches(w, csig) <= (uint32_t)k : lev2_screen(csig, csig_h, csig_l, w) <= 1u;
        };
        auto mismatches = [&](uint32_t w) -> int {           // Levenshtein: 0 = may be a duplicate (k_dense_verify decides)
            return MODE == 2 ? (passes(w) ? 0 : 3) : MODE == 1 ? (int)screen_mismatches(w, csig) : sig_mismatches(w, csig);
        };

        {
            // ---- gather: index and signature loads through L1, software-pipelined ----
            // (the vector memory counter retires in order, so what a step may wait for is decided by
            // the order in which loads are issued)
            // one step, in program order: the signature loads of the NEXT step (its indices arrived two
            // steps ago), the index loads of three steps ahead, then the compares of this step, whose
            // signatures were requested one step ago - two steps' gathers are in flight at any time
            auto step = [&](int q0, uint32_t (&w)[U], uint32_t (&cur)[U], uint32_t (&w_next)[U], uint32_t (&nxt)[U],
                            uint32_t (&far)[U]) {
#pragma unroll
                for (int u = 0; u < U; u++)
                    w_next[u] = sg[nxt[u]];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < U; u++)
                    far[u] = ld_idx(q0 + 3 * U + u);
                __builtin_amdgcn_sched_barrier(0);
                // common case: nobody in the wave outlives the signature - one test per step
                uint32_t some = 0;                             // (bitwise on purpose: no branches here)
#pragma unroll
                for (int u = 0; u < U; u++)
                    some |= (uint32_t)passes(w[u]) & (uint32_t)(q0 + u < K);
                if (__ballot(some != 0) == 0)
                    return;
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const int mm = mismatches(w[u]);
                    push(q0 + u < K && mm <= k && (!SYM || cur[u] > c), cur[u], q0 + u, mm);
                }
            };
            // four index sets and two signature sets rotate by name, not by moves (a move would wait
            // for its load)
            uint32_t i0[U], i1[U], i2[U], i3[U], s0[U], s1[U];
            if (kmax > 0) {
#pragma unroll
                for (int u = 0; u < U; u++) {
                    i0[u] = ld_idx(u);
                    i1[u] = ld_idx(U + u);
                    i2[u] = ld_idx(2 * U + u);
                }
                // everything loaded so far is consumed here, so that no wait for it lands inside the loop
                WD_PIN("+v"(csig));
#pragma unroll
                for (int u = 0; u < U; u++)
                    s0[u] = sg[i0[u]];
            }
            for (int q0 = 0; q0 < kmax; q0 += 4 * U) {
                step(q0, s0, i0, s1, i1, i3);
                if (q0 + U >= kmax)
                    break;
                step(q0 + U, s1, i1, s0, i2, i0);
                if (q0 + 2 * U >= kmax)
                    break;
                step(q0 + 2 * U, s0, i2, s1, i3, i1);
                if (q0 + 3 * U >= kmax)
                    break;
                step(q0 + 3 * U, s1, i3, s0, i0, i2);
            }
        }

        // ---- the next tile's inputs have landed; start the loads of the one after ----
        WD_WAIT_VM0();
        const uint32_t f_nxt = f_ld, sig_nxt = sig_ld;
        if (ti + 2 < n_tl)
            issue(tile + 2, ti % kWinBufs);

        // ---- survivors -> this group's region of the global queue (k_dense_mark takes over) ----
        const size_t region = (size_t)tile * groups + grp;
        if (n_q <= (uint32_t)a.q_per) {
            uint2 *qreg = a.queue + region * a.q_per;
            const bool mark_here = MODE != 2 && a.rows != nullptr && L > a.sig_cycles;     // (as in k_dense_pairs_win)
            for (uint32_t i0 = 0; i0 < n_q; i0 += kWave) {
                const uint32_t i = i0 + lane;
                const uint2 e = i < n_q ? s_q[i] : make_uint2(0u, 0u);
                const uint32_t cc = (uint32_t)__shfl((int)c, (int)(e.y >> 24));
                if (i < n_q) {
                    qreg[i] = e;
                    if (mark_here) {
                        dense_mark(a, tile, e.x);
                        dense_mark(a, tile, cc);
                    }
                }
            }
            if (lane == 0) {
                a.q_cnt[region] = n_q;
                if (MODE != 2 && n_q)
                    a.cand[0] = 1u;
            }
        } else if (MODE == 2) {
            WD_DENSE_NOTE(overflow_gather);
            // More survivors than the region holds (low-diversity reads): leave the whole group to
            // k_dense_verify, which then needs the packed rows of all its wells
            if (lane == 0) {
                a.q_cnt[region] = 0xFFFFFFFFu;
                if (L > a.sig_cycles)
                    a.cand[kDenseSlots] = 1u;
            }
            if (a.rows != nullptr && L > a.sig_cycles && valid) {
                dense_mark(a, tile, c);
                for (int q = 0; q < K; q++)
                    dense_mark(a, tile, ld_idx(q));
            }
        } else {
            // ... or drop the queue and finish every pair of this group here, one lane per target,
            // cycle by cycle
            WD_DENSE_NOTE(overflow_gather);
            if (lane == 0)
                a.q_cnt[region] = 0;
            gsig sgx = (gsig)(a.sig + (size_t)tile * a.sig_stride);             // the exact signatures
            const uint32_t csig_x = sgx[c];
            for (int q = 0; q < K; q++) {
                const uint32_t w_i = ld_idx(q);
                if (SYM && w_i <= c)
                    continue;
                int mm = sig_mismatches(sgx[w_i], csig_x);
                for (int j = S; j < L && mm <= k; j++) {
                    gbytes p_j = dense_plane(a, tile, j);
                    mm += code_of(p_j[w_i]) != code_of(p_j[c]) ? 1 : 0;
                }
                if (mm <= k) {
                    int lev = 0;
#pragma unroll
                    for (int l = 0; l < 7; l++)
                        lev += (l < levels - 1 && q >= rel[l]) ? 1 : 0;
                    if (SYM)
                        dense_record_pair(a, dense_slot(a, tile, t), [&](int t2) { return dense_slot(a, tile, t2); },
                                          tile, t, c, q, lev, w_i, mm);
                    else
                        dense_record(a, dense_slot(a, tile, t), tile, t, q, lev, mm);
                }
            }
        }
        f_cur = f_nxt;
        csig = sig_nxt;
    }
}

// 64 consecutive group regions of one tile, walked by one wave with their entries flattened:
// lane r holds region g0 + r's count; entry e of the flattened list lives in the region r with
// before[r] <= e < before[r + 1].  (A region holds a handful of entries: one wave per region
// would leave most lanes idle.)
struct RegionWalk {
    uint32_t raw;        // this lane's region: q_cnt as k_dense_pairs left it (0xFFFFFFFF: overflowed)
    uint32_t before;     // entries in the regions of lower lanes
    uint32_t total;      // entries of all 64 regions
    uint32_t *s_pre;     // this wave's 64 words of LDS
    __device__ inline RegionWalk(const DenseArgs &a, int tile, int g0, int groups, uint32_t *lds)
    {
        const int lane = threadIdx.x & (kWave - 1);
        s_pre = lds;
        raw = g0 + lane < groups ? a.q_cnt[(size_t)tile * groups + g0 + lane] : 0u;
        const uint32_t cnt = raw == 0xFFFFFFFFu ? 0u : raw;
        uint32_t inc = cnt;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const uint32_t o = __shfl_up(inc, d);
            inc += lane >= d ? o : 0u;
        }
        before = inc - cnt;
        total = (uint32_t)__shfl((int)inc, kWave - 1);
        s_pre[lane] = before;
        WD_LOCKSTEP();
    }
    // region (0..63) and index within it of flattened entry e < total
    __device__ inline void locate(uint32_t e, int &r, uint32_t &j) const
    {
        int lo = 0;                                   // the last lane with before <= e (empty regions share a value)
#pragma unroll
        for (int step = 32; step > 0; step >>= 1)
            lo += (lo + step < kWave && s_pre[lo + step] <= e) ? step : 0;
        r = lo;
        j = e - s_pre[lo];
    }
};

// Levenshtein only, between the compare stage and the rank scan: every queued survivor that passes
// the exact test on the screen's cycles marks its two wells (they get packed rows), and the
// batch's survivors are counted for dense_packed().  (The Hamming family's screen is exact on its
// cycles: k_dense_pairs* mark and count in place.)
__global__ __launch_bounds__(kBlock) void k_dense_mark(DenseArgs a)
{
    __shared__ uint32_t s_pre[kWaves][kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.y;
    const int groups = (a.T + kWave - 1) / kWave;
    const int g0 = (blockIdx.x * kWaves + wave) * kWave;
    if (g0 >= groups)
        return;
    const RegionWalk rw(a, tile, g0, groups, s_pre[wave]);
    const bool want_rows = a.rows != nullptr && a.L > a.sig_cycles;
    // Levenshtein: the compare stage's screen lets ~1e-4 of the random pairs through (it only bounds
    // the distance); the exact test on the same 16 cycles strikes nearly all of them here
    // (mismatch field 15), before they cost two marks and two packed rows each
    const uint32_t *scr = a.lev2 ? a.sig2 + (size_t)tile * a.sig_stride : nullptr;
    uint32_t kept = 0;
    for (uint32_t base = 0; (want_rows || scr) && base < rw.total; base += kWave) {
        const uint32_t e = base + lane;
        bool keep = e < rw.total;
        int r = 0;
        uint32_t j = 0;
        if (keep)
            rw.locate(e, r, j);
        uint2 *slot = a.queue + ((size_t)tile * groups + g0 + r) * a.q_per + j;
        const uint2 ent = keep ? *slot : make_uint2(0u, 0u);
        const size_t tt = (size_t)(g0 + r) * kWave + (ent.y >> 24);
        const uint32_t cc = !keep ? 0u : a.sym ? (uint32_t)(a.centre0 + (int)tt) : (uint32_t)a.centre[tt];
        if (scr && keep && lev2_window16(scr[cc], scr[ent.x]) > 2) {
            keep = false;
            slot->y = ent.y | (0xFu << 20);
        }
        if (keep && want_rows) {
            dense_mark(a, tile, ent.x);
            dense_mark(a, tile, cc);
        }
        kept += (uint32_t)__popcll(__ballot(keep));
    }
    if (!(want_rows || scr))
        kept = rw.total;
    if (lane == 0 && kept)
        a.cand[0] = 1u;
}

// Levenshtein <= 2 of one pair straight from the planes, the whole wave on it: lane j of a chunk
// holds cycle j of both reads and the centre's cycles j+1 and j-1; three ballots per chunk give
// the mismatch masks of the three diagonals, and the closed form (lev2_window) is evaluated on
// those bit masks.  L <= 192.  The result is wave-uniform.
template <bool STRIDED>
__device__ inline int lev2_gather(const TilePlanes<STRIDED> &pl, int L, uint32_t idx, uint32_t c, int lane)
{
    uint64_t m0[3] = {0, 0, 0}, mp[3] = {0, 0, 0}, mm[3] = {0, 0, 0};
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        if (ch * kWave < L) {
            const int j = ch * kWave + lane;
            const bool in = j < L;
            gbytes p = pl.at(min(j, L - 1));
            const uint32_t a0 = code_of(p[c]), b0 = code_of(p[idx]);
            const uint32_t a_next = code_of(pl.at(min(j + 1, L - 1))[c]);
            const uint32_t a_prev = code_of(pl.at(max(min(j, L - 1) - 1, 0))[c]);
            m0[ch] = __ballot(in && a0 != b0);
            mp[ch] = __ballot(in && a_next != b0);          // b[j] against a[j+1]
            mm[ch] = __ballot(in && a_prev != b0);          // b[j] against a[j-1]
        }
    }
    return lev2_masks(m0, mp, mm);
}

// Survivors of the signature, one wave per 64 group regions of a tile (blockIdx.y = tile), their
// entries flattened: one lane per entry up to cycle 8 + 4k, then one lane per CYCLE for whoever is
// left - all remaining cycles of an entry in one round trip (up to 256 at a time), and two entries
// in flight.  Tallies gather in LDS and reach the global counter slots once per block.
template <bool STRIDED>
__global__ __launch_bounds__(kBlock) void k_dense_verify(DenseArgs a)
{
    __shared__ uint32_t s_tally[4 * 8];                  // dups, hit, first, last deltas (levels <= 8)
    __shared__ uint32_t s_pre[kWaves][kWave];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int levels = a.levels;
    const int groups = (a.T + kWave - 1) / kWave;
    const int tile = blockIdx.y;
    const TilePlanes<STRIDED> pl(a, tile);
    // XCD x takes a contiguous range of targets (as in k_dense_pairs): a duplicate pair is
    // usually seen from both ends, a few target blocks apart, and the second visit then finds
    // the pair's lines in that XCD's L2
    const int nvb = (groups + kWave * kWaves - 1) / (kWave * kWaves);           // blocks of 4 x 64 regions
    const int vpx = (nvb + kXcds - 1) / kXcds;
    const int vb = (int)(blockIdx.x % kXcds) * vpx + (int)(blockIdx.x / kXcds);
    const int g0 = vb < nvb ? (vb * kWaves + wave) * kWave : groups;
    if ((int)threadIdx.x < 4 * levels)
        s_tally[threadIdx.x] = 0;
    __syncthreads();
    const int L = a.L, k = a.k;
    const int jf = min(L, finish_from(k));
    const bool packed = dense_packed(a);
    const RegionWalk rw(a, tile, g0, groups, s_pre[wave]);
    const bool whole_in_sig = a.L <= a.sig_cycles;       // short reads: the signature filter was exact
    // a marked well's row: cycles sig_cycles.., 10 per word (the first word of a read is its signature)
    const MarkIndex mi(a, tile);
    const uint4 *rows_t = a.rows + (size_t)tile * a.N * kRowGroups;
    const uint32_t *sig_t = a.sig + (size_t)tile * a.sig_stride;
    // Levenshtein <= 2 on a packed batch: two rows per pair
    auto load_row = [&](uint32_t well, uint32_t (&r)[kRowDw]) {
        const uint4 *p = rows_t + (size_t)mi.rank(well) * kRowGroups;
#pragma unroll
        for (int g = 0; g < kRowGroups; g++) {
            const uint4 x = p[g];
            r[4 * g] = x.x; r[4 * g + 1] = x.y; r[4 * g + 2] = x.z; r[4 * g + 3] = x.w;
        }
    };
    // a duplicate: for its target - or (sym: the pair is queued once, from its lower well) for both wells' targets
    auto record = [&](int t, uint32_t c, int q, int lev, uint32_t idx, int d) {
        if (a.sym)
            dense_record_pair(a, s_tally, [&](int) { return s_tally; }, tile, t, c, q, lev, idx, d);
        else
            dense_record(a, s_tally, tile, t, q, lev, d);
    };
    auto lev2_pair = [&](uint32_t idx, uint32_t c) -> int {
        uint32_t ra[kRowDw], rb[kRowDw];
        load_row(c, ra);
        load_row(idx, rb);
        return row_lev2(sig_t[c], sig_t[idx], ra, rb, a.L);
    };
    // groups whose survivor queue overflowed in k_dense_pairs (which then made the batch a packed
    // one): every pair of the group's 64 targets, one lane per target
    for (uint64_t over = a.lev2 ? __ballot(rw.raw == 0xFFFFFFFFu) : 0ull; over; over &= over - 1) {
        const int t = (g0 + __builtin_ctzll(over)) * kWave + lane;
        const bool in = t < a.T;
        const uint32_t c = in ? (uint32_t)a.centre[t] : 0u;
        const bool valid = in && (a.sym || (as_global(a.filter[tile])[c] & 1u));
        const int32_t *o = a.lvl_off + (size_t)(in ? t : 0) * (levels + 1);
        const int K = valid ? o[levels] - o[0] : 0;
        for (int q = 0; q < K; q++) {
            int lev = 0;
            for (int l = 1; l < levels; l++)
                lev += (o[0] + q >= o[l]) ? 1 : 0;
            const uint32_t idx = (uint32_t)a.nbr[o[0] + q];
            if (a.sym && idx <= c)
                continue;                                // (seen from the other well)
            const int d = whole_in_sig ? lev2_window(sig_t[c], sig_t[idx]) : lev2_pair(idx, c);
            if (d <= 2)
                record(t, c, q, lev, idx, d);
        }
    }
    for (uint32_t base = 0; base < rw.total; base += kWave) {
        bool have = base + lane < rw.total;
        int r = 0;
        uint32_t slot_j = 0;
        if (have)
            rw.locate(base + lane, r, slot_j);
        uint2 ent = make_uint2(0u, 0u);
        if (have)
            ent = a.queue[((size_t)tile * groups + g0 + r) * a.q_per + slot_j];
        const uint32_t idx = ent.x;
        const int t = (g0 + r) * kWave + (int)(ent.y >> 24);
        const int q = (int)(ent.y & 0x1FFFFu);
        const int lev = (int)((ent.y >> 17) & 7u);
        // mismatches within the exact signature word (the entry's field holds the screen's count)
        have = have && ((ent.y >> 20) & 0xFu) != 15u;       // struck by k_dense_mark
        // (one-ended compare: centres are consecutive, no load)
        const uint32_t c = !have ? 0u : a.sym ? (uint32_t)(a.centre0 + t) : (uint32_t)a.centre[t];
        // (equality: the compare stage queued the pair because the signatures were equal)
        int mm = (have && !a.lev2 && k > 0) ? sig_mismatches(sig_t[ent.x], sig_t[c]) : 0;
        if (a.lev2 && whole_in_sig) {
            // the whole read is in the (exact) signature word
            if (have) {
                const int d = lev2_window(sig_t[c], sig_t[idx]);
                if (d <= 2)
                    record(t, c, q, lev, idx, d);
            }
            continue;
        }
        if (a.lev2 && packed) {
            if (have) {
                const int d = lev2_pair(idx, c);
                if (d <= 2)
                    record(t, c, q, lev, idx, d);
            }
            continue;
        }
        if (a.lev2) {
            // rows not in use (dense_pack = 0): each survivor is checked against the planes by the whole wave
            const bool alive = have;
            uint64_t todo = __ballot(alive);
            while (todo) {
                const int i = __builtin_ctzll(todo);
                todo &= todo - 1;
                const int d = lev2_gather(pl, L, (uint32_t)__shfl((int)idx, i), (uint32_t)__shfl((int)c, i), lane);
                if (lane == i && d <= 2)
                    record(t, c, q, lev, idx, d);
            }
            continue;
        }
        if (packed) {
            // one lane per entry: the two wells' rows, one 64-byte piece each (mm: the signature's share)
            if (have) {
                uint32_t ra[kRowDw], rb[kRowDw];
                load_row(c, ra);
                load_row(idx, rb);
                const int d = mm + row_mismatches(ra, rb, L);
                if (d <= k)
                    record(t, c, q, lev, idx, d);
            }
            continue;
        }
        bool alive = have;
        int j = a.sig_cycles;
        // lane per entry: rounds of up to 4 cycles, both wells' bytes in flight together
        while (j < jf && __ballot(alive)) {
            const int nb = min(4, jf - j);
            if (alive) {
                uint32_t w[4], cb[4];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    gbytes p = pl.at(min(j + i, L - 1));
                    w[i] = p[idx];
                    cb[i] = p[c];
                }
#pragma unroll
                for (int i = 0; i < 4; i++)
                    mm += (i < nb && code_of(w[i]) != code_of(cb[i])) ? 1 : 0;
                alive = mm <= k;
            }
            j += nb;
        }
        // lane per cycle
        if (j < L) {
            uint64_t todo = __ballot(alive);
            while (todo) {
                const int i0 = __builtin_ctzll(todo);
                todo &= todo - 1;
                const bool two = todo != 0;
                const int i1 = two ? __builtin_ctzll(todo) : i0;
                if (two)
                    todo &= todo - 1;
                const uint32_t bi0 = (uint32_t)__shfl((int)idx, i0), bc0 = (uint32_t)__shfl((int)c, i0);
                const uint32_t bi1 = (uint32_t)__shfl((int)idx, i1), bc1 = (uint32_t)__shfl((int)c, i1);
                int bm0 = __shfl(mm, i0), bm1 = __shfl(mm, i1);
                for (int jc = j; jc < L && (bm0 <= k || bm1 <= k); jc += 4 * kWave) {
                    uint32_t x0[4], y0[4], x1[4], y1[4];
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        gbytes p = pl.at(min(jc + r * kWave + lane, L - 1));
                        x0[r] = p[bi0];
                        y0[r] = p[bc0];
                        x1[r] = p[bi1];
                        y1[r] = p[bc1];
                    }
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const bool in = jc + r * kWave + lane < L;
                        bm0 += __popcll(__ballot(in && code_of(x0[r]) != code_of(y0[r])));
                        bm1 += __popcll(__ballot(in && code_of(x1[r]) != code_of(y1[r])));
                    }
                }
                if (lane == i0)
                    mm = bm0;
                if (two && lane == i1)
                    mm = bm1;
            }
        }
        if (alive && mm <= k)
            record(t, c, q, lev, idx, mm);
    }
    __syncthreads();
    if ((int)threadIdx.x < 4 * levels) {
        const int32_t v = (int32_t)s_tally[threadIdx.x];
        if (v) {
            unsigned long long *slot = a.partial + ((size_t)tile * kDenseSlots + (blockIdx.x & (kDenseSlots - 1))) * a.partial_stride;
            atomicAdd(&slot[1 + levels + threadIdx.x], (unsigned long long)(long long)v);
        }
    }
}

__global__ __launch_bounds__(kWave) void k_dense_reduce(const unsigned long long *partial, int stride,
                                                        int ncnt, unsigned long long *out_tile)
{
    const int tile = blockIdx.x;
    for (int i = threadIdx.x; i < ncnt; i += kWave) {
        unsigned long long s = 0;
        for (int sl = 0; sl < kDenseSlots; sl++)
            s += partial[((size_t)tile * kDenseSlots + sl) * stride + i];
        out_tile[(size_t)tile * ncnt + i] += s;
    }
}
