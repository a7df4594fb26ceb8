// wave_emu.h - what a kernel's source needs to run on the CPU as it stands (tools/lane_mismatch_emu.cpp,
// tools/lane_distance_emu.cpp, tools/lane_quality_emu.cpp, tools/lane_saturation_emu.cpp, tools/lane_top_emu.cpp, tools/lane_hops_emu.cpp, tools/lane_gc_emu.cpp): the 256 lanes of a
// workgroup are fibers (ucontext) that a round-robin scheduler switches at the collectives - __syncthreads is a
// rendezvous of the workgroup, __ballot and __shfl of a wave -, LDS is the kernel's static storage, an atomic add or
// minimum or a compare-and-swap is a plain one (one fiber runs at a time), and the qualifiers are empty.  Include it, then the kernel's
// .inc file, then call run_block(block x, block y, kernel call) per workgroup.  The device half of csrc/lane_pass.inc -
// the run (kLaneRun, LaneRun) and wave_by_key - comes with it, included at the end: the kernels' own, not a copy.
// Nothing here says anything about time.
#pragma once
#include <ucontext.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <algorithm>
using std::min; using std::max;
struct uint4 { uint32_t x, y, z, w; };
static uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }
struct int2 { int x, y; };
struct uint2 { uint32_t x, y; };
static uint2 make_uint2(uint32_t x, uint32_t y) { return uint2{x, y}; }
struct D3 { unsigned x, y, z; };
constexpr int kTdBlock = 256, kWave = 64, kSpread = 64, kFpCycles = 10, kLdCmpWords = 8;
constexpr uint32_t kInvalid = 0xFFFFFFFFu;
constexpr int kMaxCycles = 1024;
static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
// ---- fibers: one per lane of a workgroup, switched at collectives
struct Fiber { ucontext_t ctx; bool done; char *stack; };
static Fiber fib[kTdBlock]; static ucontext_t sched; static int cur;
static D3 g_block;
#define threadIdx (D3{(unsigned)cur, 0, 0})
#define blockIdx g_block
static void yield_() { swapcontext(&fib[cur].ctx, &sched); }
static int bar_count = 0; static long bar_gen = 0;
static void __syncthreads() { long g = bar_gen; if (++bar_count == kTdBlock) { bar_count = 0; bar_gen++; } else while (bar_gen == g) yield_(); }
struct WaveSync { int count = 0; long gen = 0; unsigned long long pred[2] = {0, 0}; int val[2][kWave]; };
static WaveSync ws[kTdBlock / kWave];
static unsigned long long __ballot(bool p) {
    WaveSync &w = ws[cur / kWave]; long g = w.gen; int par = g & 1, lane = cur % kWave;
    if (w.count == 0) w.pred[par] = 0;
    if (p) w.pred[par] |= 1ull << lane;
    if (++w.count == kWave) { w.count = 0; w.gen++; } else while (w.gen == g) yield_();
    return w.pred[par];
}
static int __shfl(int v, int src) {
    WaveSync &w = ws[cur / kWave]; long g = w.gen; int par = g & 1, lane = cur % kWave;
    w.val[par][lane] = v;
    if (++w.count == kWave) { w.count = 0; w.gen++; } else while (w.gen == g) yield_();
    return w.val[par][src];
}
#define __popcll __builtin_popcountll
#define __ffsll __builtin_ffsll
#define __clzll __builtin_clzll
#define __popc __builtin_popcount
#define __ffs __builtin_ffs
template <class T, class U> static T atomicAdd(T *p, U v) { T o = *p; *p += (T)v; return o; }
template <class T> static T atomicCAS(T *p, T expect, T v) { T o = *p; if (o == expect) *p = v; return o; }
template <class T, class U> static T atomicMin(T *p, U v) { T o = *p; if ((T)v < o) *p = (T)v; return o; }
static unsigned long long *spread_row(unsigned long long *cnt, size_t row, int width) { return cnt + (row * kSpread + blockIdx.x % kSpread) * width; }
// the lanes of the wave below this one whose bit is set in the mask's low (high) half, added to a
#define __builtin_amdgcn_mbcnt_lo(m, a) ((a) + (uint32_t)__builtin_popcount((uint32_t)(m) & (uint32_t)((1ull << std::min(cur % kWave, 32)) - 1)))
#define __builtin_amdgcn_mbcnt_hi(m, a) ((a) + (uint32_t)__builtin_popcount((uint32_t)(m) & (uint32_t)((1ull << std::max(cur % kWave - 32, 0)) - 1)))
#define __device__
#define __host__
#define __global__
#define __shared__ static
#define __launch_bounds__(x)
#define __restrict__
// ---- a workgroup: every fiber runs `kernel` (the emulator's call of its kernel with its arguments) to the end
static void (*g_kernel)();
static void entry_() { g_kernel(); fib[cur].done = true; swapcontext(&fib[cur].ctx, &sched); }
static void run_block(unsigned bx, unsigned by, void (*kernel)()) {
    g_block = D3{bx, by, 0};
    g_kernel = kernel;
    for (int t = 0; t < kTdBlock; t++) {
        if (!fib[t].stack) fib[t].stack = (char *)malloc(1 << 16);
        getcontext(&fib[t].ctx); fib[t].ctx.uc_stack.ss_sp = fib[t].stack; fib[t].ctx.uc_stack.ss_size = 1 << 16; fib[t].ctx.uc_link = &sched;
        fib[t].done = false; makecontext(&fib[t].ctx, entry_, 0);
    }
    int left = kTdBlock;
    while (left) for (int t = 0; t < kTdBlock; t++) if (!fib[t].done) { cur = t; swapcontext(&sched, &fib[t].ctx); if (fib[t].done) left--; }
}
#define WD_LANE_PASS_EMU
#include "../well_duplicates_amd/csrc/lane_pass.inc"
