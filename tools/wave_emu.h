// wave_emu.h - what a kernel's source needs to run on the CPU as it stands (tools/lane_mismatch_emu.cpp,
// tools/lane_distance_emu.cpp, tools/lane_quality_emu.cpp, tools/lane_saturation_emu.cpp, tools/lane_top_emu.cpp, tools/lane_hops_emu.cpp, tools/lane_gc_emu.cpp, tools/lane_adapter_emu.cpp, tools/lane_consensus_emu.cpp, tools/lane_umi_emu.cpp, tools/lane_keep_emu.cpp,
// tools/lane_molecules_emu.cpp, tools/read_classes_emu.cpp, tools/near_emu.cpp, tools/dup_sets_emu.cpp, tools/lane_index_emu.cpp, tools/gen_rings_emu.cpp,
// tools/scan_queue_emu.cpp, tools/scan_lines_emu.cpp, tools/scan_dense_emu.cpp, tools/scan_lev_emu.cpp): the 256 lanes of a
// workgroup are fibers (ucontext) that a round-robin scheduler switches at the collectives - __syncthreads is a
// rendezvous of the workgroup, __ballot and __shfl of a wave -, LDS is the kernel's static storage, an atomic add or
// minimum or a compare-and-swap is a plain one (one fiber runs at a time), and the qualifiers are empty.  Include it, then the kernel's
// .inc file, then call run_block(block x, block y, kernel call) per workgroup.  The device half of csrc/lane_pass.inc -
// the run (kLaneRun, LaneRun) and wave_by_key - comes with it, included at the end: the kernels' own, not a copy.
// Nothing here says anything about time.
//
// Schedules.  Every atomic - the atomicAdd family and the __hip_atomic_* builtins - is a scheduling point followed by
// the plain operation: at a point the fiber may hand over to the next one, so that other lanes run between a lane's
// load and its compare-and-swap, or between the two finds of a union.  emu_schedule(policy, seed) decides: never (the
// default: fibers switch at the collectives alone, as they always did here), with probability 1/3, always; reverse
// starts the fibers of a workgroup from lane 255 down; run_grid runs the workgroups of a launch one after the other
// (a workgroup still runs to its end before the next begins), in a seeded permutation of (x, y) if asked.  emu_counts
// holds the scheduling points passed and the compare-and-swaps that lost - found another value than expected - since
// emu_counts_clear() (run_grid returns those of its launch), the latter by emu_cas_tag, which the emulator sets before a launch (kEmuTable, kEmuUnion).
// The plain atomicCAS counts under kEmuLds, whatever the tag: the kernels use it on their tables in LDS alone
// (k_li_tally, k_lh_tally), and there without a load before it - a lane that meets an entry another key took long ago
// finds "another value" too, under every schedule.  So it counts as lost when the word held `expect` as the lane
// arrived at the scheduling point and no longer did after it: another lane took the free entry in between, which is
// what a lost claim is, and what the schedule that never hands over cannot produce.  The
// emulation is sequentially consistent: every fiber sees every store at once.  With -DWAVE_EMU_TORN_CAS the
// compare-and-swap is broken on purpose - a scheduling point between its load and its store - for the emulators' tests
// to show that they notice (without a value: in the __hip_atomic compare-and-swaps, whatever their tag; =2: in those
// tagged kEmuUnion alone; =3: in the plain atomicCAS alone, so that each build of an emulator that has both kinds
// shows one of them); nothing else builds that way.
// -DWAVE_EMU_TORN_MIN breaks atomicMin the same way - a scheduling point between its load and its store, so that a
// lane writes over a smaller value another lane stored in between (tools/lane_keep_emu.cpp); off by default.
// -DWAVE_EMU_TORN_ADD breaks atomicAdd the same way, for an emulator whose kernels take their places by adds
// (tools/lane_consensus_emu.cpp; tools/gen_rings_emu.cpp, which clears emu_torn_add for its count pass so that the
// fill pass's claim of an LDS slot alone is broken).
// -DWAVE_EMU_TORN_OR breaks atomicOr the same way (tools/scan_lines_emu.cpp: the hit-level masks four targets share a
// word of; tools/scan_dense_emu.cpp, which builds with both flags and clears emu_torn_or or emu_torn_add at run time).
// Workgroups have kEmuBlock = 256 lanes unless a unit defines WAVE_EMU_MAX_BLOCK before this header and sets emu_block
// (a multiple of kWave) before a launch: tools/scan_dense_emu.cpp runs kernels of 64, 256 and 1024 lanes.
// -DWAVE_EMU_UNIT_DEFS: the emulator includes csrc/read_classes.inc and csrc/tile_classes.inc (the head of the tiledups unit),
// which define kTdBlock, kSpread, kFpCycles, kLdCmpWords, kInvalid, kMaxCycles, align256 and spread_row themselves:
// this header then leaves them, and lane_pass.inc, out.  tools/dup_sets_emu.cpp defines it too: csrc/dup_sets.inc
// brings kSpread, kInvalid and align256 of its own.
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
struct int4 { int x, y, z, w; };
static int4 make_int4(int x, int y, int z, int w) { return int4{x, y, z, w}; }
struct uint2 { uint32_t x, y; };
static uint2 make_uint2(uint32_t x, uint32_t y) { return uint2{x, y}; }
struct D3 { unsigned x, y, z; };
constexpr int kEmuBlock = 256;
// A unit whose kernels have other workgroup sizes (tools/scan_dense_emu.cpp: 64, 256 and 1024 lanes) defines
// WAVE_EMU_MAX_BLOCK before this header and sets emu_block before a launch; everyone else gets 256 lanes, as ever.
#ifndef WAVE_EMU_MAX_BLOCK
#define WAVE_EMU_MAX_BLOCK 256
#endif
constexpr int kEmuMaxBlock = WAVE_EMU_MAX_BLOCK;
static int emu_block = kEmuBlock;                  // lanes of the workgroups being run: a multiple of kWave, <= kEmuMaxBlock
#ifndef WD_SHARED_H                                // (an emulator that included csrc/wd_shared.h before this header has the library's kWave)
constexpr int kWave = 64;
#endif
#ifndef WAVE_EMU_UNIT_DEFS
constexpr int kTdBlock = kEmuBlock, kSpread = 64, kFpCycles = 10, kLdCmpWords = 8;
constexpr uint32_t kInvalid = 0xFFFFFFFFu;
constexpr int kMaxCycles = 1024;
static size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
#endif
// ---- fibers: one per lane of a workgroup, switched at collectives - and at atomics, if the schedule says so
struct Fiber { ucontext_t ctx; void *sp; bool done; char *stack; const long *wait; long wait_at; };      // wait: the generation of the rendezvous it stands at
static Fiber emu_fib[kEmuMaxBlock]; static ucontext_t emu_sched; static void *emu_sched_sp; static int emu_lane;
// A switch saves the registers a call preserves on the fiber's own stack and changes stacks: swapcontext does the same
// and a system call for the signal mask on top, which at a switch per atomic was most of an emulator's run time (near_emu: 47 s against 6).
// Elsewhere than on x86-64, or with -DWAVE_EMU_UCONTEXT, it is swapcontext.
#if defined(__x86_64__) && !defined(WAVE_EMU_UCONTEXT)
#define WAVE_EMU_FAST 1
extern "C" void emu_switch(void **from_sp, void *to_sp);
asm(".text\n.globl emu_switch\n.type emu_switch,@function\nemu_switch:\n"
    "pushq %rbp\npushq %rbx\npushq %r12\npushq %r13\npushq %r14\npushq %r15\n"
    "movq %rsp, (%rdi)\nmovq %rsi, %rsp\n"
    "popq %r15\npopq %r14\npopq %r13\npopq %r12\npopq %rbx\npopq %rbp\nret\n");
#endif
static D3 g_block, g_grid;
#define threadIdx (D3{(unsigned)emu_lane, 0, 0})
#define blockIdx g_block
#define gridDim g_grid                             // (run_grid sets it: the launch's workgroups)
#ifdef WAVE_EMU_FAST
static void yield_() { emu_switch(&emu_fib[emu_lane].sp, emu_sched_sp); }
#else
static void yield_() { swapcontext(&emu_fib[emu_lane].ctx, &emu_sched); }
#endif
// at a rendezvous whose generation is g: not run again before the last lane has come (the scheduler passes it over)
static void await_(const long &gen, long g) { Fiber &f = emu_fib[emu_lane]; f.wait = &gen; f.wait_at = g; while (gen == g) yield_(); f.wait = nullptr; }
// A ballot or a shuffle under a condition (if (w < N) { .. __ballot(pf) .. }) is one of the wave's lanes that take the
// branch: it is complete when every lane of the wave stands at it, waits at the workgroup's barrier (away) or has ended
// (gone) - the lanes that went round it - and a lane that is not there sets no bit.
struct WaveSync { int count = 0, away = 0, gone = 0; long gen = 0; unsigned long long pred[2] = {0, 0}; int val[2][kWave]; };
static WaveSync emu_ws[kEmuMaxBlock / kWave];
static bool wave_complete_(WaveSync &w) { if (w.count + w.away + w.gone < kWave) return false; w.count = 0; w.gen++; return true; }
static int bar_count = 0; static long bar_gen = 0;
static void __syncthreads() {
    long g = bar_gen;
    if (++bar_count == emu_block) { bar_count = 0; bar_gen++; for (WaveSync &w : emu_ws) w.away = 0; return; }
    WaveSync &w = emu_ws[emu_lane / kWave]; w.away++; if (w.count) wave_complete_(w);
    await_(bar_gen, g);
}
static unsigned long long __ballot(bool p) {
    WaveSync &w = emu_ws[emu_lane / kWave]; long g = w.gen; int par = g & 1, lane = emu_lane % kWave;
    if (w.count == 0) w.pred[par] = 0;
    if (p) w.pred[par] |= 1ull << lane;
    w.count++; if (!wave_complete_(w)) await_(w.gen, g);
    return w.pred[par];
}
static int __shfl(int v, int src) {
    WaveSync &w = emu_ws[emu_lane / kWave]; long g = w.gen; int par = g & 1, lane = emu_lane % kWave;
    w.val[par][lane] = v;
    w.count++; if (!wave_complete_(w)) await_(w.gen, g);
    return w.val[par][src];
}
// the wave's other rendezvous (csrc/scan_queue.inc): a lane takes the value of the lane `d` below it (its own, where there
// is none), of lane `src`, or of the first lane that stands at the call; the barrier of a wave is a rendezvous without a
// value, and the fence that goes with it says nothing here - the emulation is sequentially consistent.
static int __shfl_up(int v, int d) { const int lane = emu_lane % kWave; const int o = __shfl(v, lane >= d ? lane - d : lane); return o; }
static int emu_readfirstlane(int v) {
    WaveSync &w = emu_ws[emu_lane / kWave]; long g = w.gen; int par = g & 1, lane = emu_lane % kWave;
    if (w.count == 0) w.pred[par] = 0;
    w.pred[par] |= 1ull << lane; w.val[par][lane] = v;
    w.count++; if (!wave_complete_(w)) await_(w.gen, g);
    return w.val[par][__builtin_ctzll(w.pred[par])];
}
// DPP (csrc/scan_lines.inc: lw_wave_sum), by the ISA's account of it and not by what its caller needs: the wave is four
// rows of 16 lanes, a row four banks of 4.  row_shr:n (0x111 .. 0x11F) reads the lane n below in the same row,
// row_bcast:15 (0x142) lane 15 of the row before, row_bcast:31 (0x143) lane 31 in rows 2 and 3.  A lane whose row or
// bank the masks switch off keeps `old`; one whose source lies outside its row (or, for the broadcasts, does not
// exist) gets 0 with bound_ctrl and keeps `old` without.  Any other control word is not emulated: abort.
static int emu_update_dpp(int old, int src, int ctrl, int row_mask, int bank_mask, bool bound_ctrl) {
    WaveSync &w = emu_ws[emu_lane / kWave]; long g = w.gen; int par = g & 1, lane = emu_lane % kWave;
    w.val[par][lane] = src;
    w.count++; if (!wave_complete_(w)) await_(w.gen, g);
    const int row = lane / 16, in_row = lane % 16;
    int from = -1;
    if (ctrl >= 0x111 && ctrl <= 0x11F) from = in_row >= (ctrl & 0xF) ? lane - (ctrl & 0xF) : -1;
    else if (ctrl == 0x142) from = row >= 1 ? row * 16 - 1 : -1;
    else if (ctrl == 0x143) from = row >= 2 ? 31 : -1;
    else { fprintf(stderr, "wave_emu.h: DPP control word 0x%X is not emulated\n", ctrl); abort(); }
    if (!((row_mask >> row) & 1) || !((bank_mask >> (in_row / 4)) & 1)) return old;
    if (from < 0) return bound_ctrl ? 0 : old;
    return w.val[par][from];
}
#define __builtin_amdgcn_update_dpp(old, src, ctrl, row_mask, bank_mask, bound_ctrl) \
    emu_update_dpp((int)(old), (int)(src), (ctrl), (row_mask), (bank_mask), (bound_ctrl))
#define __builtin_amdgcn_readlane(v, src) __shfl((int)(v), (src))
#define __builtin_amdgcn_readfirstlane(v) emu_readfirstlane((int)(v))
#define __builtin_amdgcn_wave_barrier() ((void)__ballot(false))
#define __builtin_amdgcn_fence(order, scope) ((void)0)
// __attribute__((address_space(1))) of the kernels' global pointers: an empty attribute on the host
#define address_space(n)
#define __popcll __builtin_popcountll
#define __ffsll __builtin_ffsll
#define __clzll __builtin_clzll
#define __popc __builtin_popcount
#define __ffs __builtin_ffs
// ---- the schedule: what happens at a scheduling point
enum EmuPolicy { kEmuNever, kEmuThird, kEmuAlways };
enum { kEmuTable = 0, kEmuUnion = 1, kEmuLds = 2 };
struct EmuCounts { long points, lost[3]; };
static EmuCounts emu_counts;
static int emu_cas_tag = kEmuTable;
static EmuPolicy emu_policy = kEmuNever; static bool emu_reverse = false; static uint64_t emu_rng = 1;
static uint64_t emu_next() { emu_rng ^= emu_rng << 13; emu_rng ^= emu_rng >> 7; emu_rng ^= emu_rng << 17; return emu_rng; }      // (xorshift64: the inputs keep rand())
static void emu_schedule(EmuPolicy policy, bool reverse, uint64_t seed) { emu_policy = policy; emu_reverse = reverse; emu_rng = seed * 0x9E3779B97F4A7C15ull | 1; }
static void emu_counts_clear() { emu_counts = EmuCounts{0, {0, 0, 0}}; }
static void emu_point() {
    emu_counts.points++;
    if (emu_policy == kEmuAlways || (emu_policy == kEmuThird && emu_next() % 3 == 0)) yield_();
}
// emu_add_hook, if set, sees every atomicAdd as it takes effect - the word, what it held, the lane (emu_lane): an
// emulator that wants to know in which order the lanes took their places (tools/gen_rings_emu.cpp).
static void (*emu_add_hook)(const void *p, long long old) = nullptr;
#ifdef WAVE_EMU_TORN_ADD                           // (the deliberate bug of an add: another fiber may add between its load and its store)
static bool emu_torn_add = true;                   // (an emulator may confine the bug to some of its launches)
template <class T, class U> static T atomicAdd(T *p, U v) { emu_point(); T o = *p; if (emu_torn_add) emu_point(); *p = o + (T)v; if (emu_add_hook) emu_add_hook(p, (long long)o); return o; }
#else
template <class T, class U> static T atomicAdd(T *p, U v) { emu_point(); T o = *p; *p += (T)v; if (emu_add_hook) emu_add_hook(p, (long long)o); return o; }
#endif
template <class T> static T atomicCAS(T *p, T expect, T v) {
    const bool was_free = *p == expect;
    emu_point();
    const T o = *p;
    if (o != expect) { emu_counts.lost[kEmuLds] += was_free; return o; }
#ifdef WAVE_EMU_TORN_CAS
    if (WAVE_EMU_TORN_CAS == 3) emu_point();       // (the deliberate bug, as below)
#endif
    *p = v;
    return o;
}
// emu_mins counts the atomicMin calls since an emulator last cleared it (tools/lane_keep_emu.cpp holds a kernel to a bound on them).
static long emu_mins = 0;
#ifdef WAVE_EMU_TORN_MIN                           // (the deliberate bug of a minimum: another fiber may lower the word between its load and its store)
template <class T, class U> static T atomicMin(T *p, U v) { emu_point(); emu_mins++; T o = *p; emu_point(); if ((T)v < o) *p = (T)v; return o; }
#else
template <class T, class U> static T atomicMin(T *p, U v) { emu_point(); emu_mins++; T o = *p; if ((T)v < o) *p = (T)v; return o; }
#endif
#ifdef WAVE_EMU_TORN_OR                            // (the deliberate bug of an or: another fiber may set bits of the word between its load and its store)
static bool emu_torn_or = true;                    // (an emulator may switch the bug off: one build for its torn or and its torn add)
template <class T, class U> static T atomicOr(T *p, U v) { emu_point(); T o = *p; if (emu_torn_or) emu_point(); *p = o | (T)v; return o; }
#else
template <class T, class U> static T atomicOr(T *p, U v) { emu_point(); T o = *p; *p |= (T)v; return o; }
#endif
// the clang builtins of the kernels that say their memory order and scope: the order and the scope mean nothing here
#define __HIP_MEMORY_SCOPE_AGENT 4
template <class T> static T __hip_atomic_load(const T *p, int, int) { emu_point(); return *p; }
template <class T, class U> static void __hip_atomic_store(T *p, U v, int, int) { emu_point(); *p = (T)v; }
template <class T, class U> static bool __hip_atomic_compare_exchange_strong(T *p, T *expect, U v, int, int, int) {
    emu_point();
    const T o = *p;
    if (o != *expect) { emu_counts.lost[emu_cas_tag]++; *expect = o; return false; }
#ifdef WAVE_EMU_TORN_CAS
    if (WAVE_EMU_TORN_CAS == 1 || (WAVE_EMU_TORN_CAS == 2 && emu_cas_tag == kEmuUnion)) emu_point();      // (the deliberate bug: another fiber may store between the load and the store)
#endif
    *p = (T)v;
    return true;
}
template <class T, class U> static T __hip_atomic_fetch_min(T *p, U v, int, int) { emu_point(); T o = *p; if ((T)v < o) *p = (T)v; return o; }
template <class T, class U> static T __hip_atomic_fetch_add(T *p, U v, int, int) { return atomicAdd(p, v); }      // (a scheduling point, torn with -DWAVE_EMU_TORN_ADD, seen by emu_add_hook)
template <class T, class U> static T __hip_atomic_fetch_or(T *p, U v, int, int) { return atomicOr(p, v); }
template <class T, class U> static T __hip_atomic_fetch_sub(T *p, U v, int, int) { emu_point(); T o = *p; *p -= (T)v; return o; }
template <class T, class U> static T __hip_atomic_exchange(T *p, U v, int, int) { emu_point(); T o = *p; *p = (T)v; return o; }
#define __builtin_nontemporal_load(p) (*(p))
#ifndef WAVE_EMU_UNIT_DEFS
static unsigned long long *spread_row(unsigned long long *cnt, size_t row, int width) { return cnt + (row * kSpread + blockIdx.x % kSpread) * width; }
#endif
// the lanes of the wave below this one whose bit is set in the mask's low (high) half, added to a
#define __builtin_amdgcn_mbcnt_lo(m, a) ((a) + (uint32_t)__builtin_popcount((uint32_t)(m) & (uint32_t)((1ull << std::min(emu_lane % kWave, 32)) - 1)))
#define __builtin_amdgcn_mbcnt_hi(m, a) ((a) + (uint32_t)__builtin_popcount((uint32_t)(m) & (uint32_t)((1ull << std::max(emu_lane % kWave - 32, 0)) - 1)))
#define __device__
#define __host__
#define __global__
#define __shared__ static
#define __launch_bounds__(...)
#define __restrict__
// ---- a workgroup: every fiber runs `kernel` (the emulator's call of its kernel with its arguments) to the end
static void (*g_kernel)();
static void entry_() { g_kernel(); emu_fib[emu_lane].done = true; WaveSync &w = emu_ws[emu_lane / kWave]; w.gone++; if (w.count) wave_complete_(w); yield_(); }
static void run_block(unsigned bx, unsigned by, void (*kernel)()) {
    g_block = D3{bx, by, 0};
    g_kernel = kernel;
    for (WaveSync &w : emu_ws) w.away = w.gone = 0;
    for (int t = 0; t < emu_block; t++) {
        Fiber &f = emu_fib[t];
        if (!f.stack) f.stack = (char *)malloc(1 << 16);
        f.done = false; f.wait = nullptr;
#ifdef WAVE_EMU_FAST
        void **sp = (void **)(f.stack + (1 << 16));
        *--sp = nullptr; *--sp = (void *)entry_;
        for (int r = 0; r < 6; r++) *--sp = nullptr;
        f.sp = sp;
#else
        getcontext(&f.ctx); f.ctx.uc_stack.ss_sp = f.stack; f.ctx.uc_stack.ss_size = 1 << 16; f.ctx.uc_link = &emu_sched;
        makecontext(&f.ctx, entry_, 0);
#endif
    }
    int left = emu_block;
    while (left) for (int i = 0; i < emu_block; i++) {
        const int t = emu_reverse ? emu_block - 1 - i : i;
        if (!emu_fib[t].done && !(emu_fib[t].wait && *emu_fib[t].wait == emu_fib[t].wait_at)) { emu_lane = t;
#ifdef WAVE_EMU_FAST
            emu_switch(&emu_sched_sp, emu_fib[t].sp);
#else
            swapcontext(&emu_sched, &emu_fib[t].ctx);
#endif
            if (emu_fib[t].done) left--; }
    }
}
// a launch of gx * gy workgroups: in the order x fastest, or (permute) in a permutation drawn from the schedule's seed.
// Returns the launch's own counts (emu_counts goes on adding up).  emu_after_block, if set, is called after every
// workgroup of a launch with its (x, y): an emulator that wants to see what one workgroup changed.
static void (*emu_after_block)(unsigned bx, unsigned by) = nullptr;
static EmuCounts run_grid(unsigned gx, unsigned gy, void (*kernel)(), bool permute = false) {
    const EmuCounts before = emu_counts;
    g_grid = D3{gx, gy, 1};
    std::vector<unsigned> order((size_t)gx * gy);
    for (size_t i = 0; i < order.size(); i++) order[i] = (unsigned)i;
    if (permute) for (size_t i = order.size(); i > 1; i--) std::swap(order[i - 1], order[emu_next() % i]);
    for (unsigned b : order) { run_block(b % gx, b / gx, kernel); if (emu_after_block) emu_after_block(b % gx, b / gx); }
    return EmuCounts{emu_counts.points - before.points, {emu_counts.lost[0] - before.lost[0], emu_counts.lost[1] - before.lost[1], emu_counts.lost[2] - before.lost[2]}};
}
#ifndef WAVE_EMU_UNIT_DEFS
#define WD_LANE_PASS_EMU
#include "../well_duplicates_amd/csrc/lane_pass.inc"
#endif
