// device_common.inc - what every scan kernel shares: global-address-space byte loads of the plane tables,
// the symbol code of a BCL byte, lane-range masks.  Included by welldup_scan.hip and welldup_dense.hip.
// Plane / filter pointers reach the kernels through pointer tables in memory, so the compiler
// only knows them as generic ("flat") addresses: flat loads need a VGPR address pair each and
// force vmcnt(0)+lgkmcnt(0) waits.  They are device-global by contract (include/welldup.h), so
// say so: global_load_ubyte with a scalar base, a 32-bit lane offset and counted vmcnt.
using gbytes = const __attribute__((address_space(1))) uint8_t *;
__device__ inline gbytes as_global(const uint8_t *p) { return (gbytes)p; }

// Cache policy of the plane-byte loads.  On a pure one-byte-per-line gather non-temporal loads
// (`global_load_ubyte ... nt`) reach 52.0 vs 47.1 G lines/s (tools/microbench_modes.hip; sc0 /
// sc1 change nothing and no policy fetches less than the full 128-byte line) - but the scan
// re-reads lines through L1/L2 (both slots of a pass, the centre's line, the drain rounds), and
// with nt it ran 0.163 ms instead of 0.137 ms.  So: default policy; -DWD_NT_LOADS=1 to retry.
#ifndef WD_NT_LOADS
#define WD_NT_LOADS 0
#endif
__device__ inline uint32_t ldb(gbytes p, uint32_t i)
{
#if WD_NT_LOADS
    return __builtin_nontemporal_load(p + i);
#else
    return p[i];
#endif
}

// The dynamic LDS block of a kernel, sized at the launch.  In the CPU emulation (tools/scan_queue_emu.cpp, which
// defines WD_EMU) it is a heap block of exactly the launch's bytes, so that a carve-up which is longer than the
// host's figure (scan_q_lds_dwords) is an access the address sanitizer reports.
#ifdef WD_EMU
#define WD_DYNAMIC_LDS(name) uint32_t *const name = emu_dynamic_lds
#else
#define WD_DYNAMIC_LDS(name) extern __shared__ uint32_t name[]
#endif

// Symbol code of a BCL byte: 0 -> 4 ('N'), else byte & 3 (bcl_direct_reader.py:352-361).
__device__ inline uint32_t code_of(uint32_t b)
{
    return (b & 3u) | (((b - 1u) >> 29) & 4u);
}

// Bits [lo, hi) of a 64-bit mask, lo/hi clamped to [0, 64].
__device__ inline uint64_t range_mask(int lo, int hi)
{
    lo = lo < 0 ? 0 : (lo > 64 ? 64 : lo);
    hi = hi < 0 ? 0 : (hi > 64 ? 64 : hi);
    uint64_t mh = hi >= 64 ? ~0ull : ((1ull << hi) - 1ull);
    uint64_t ml = lo >= 64 ? ~0ull : ((1ull << lo) - 1ull);
    return mh & ~ml;
}

// Cycles after which a survivor is almost certainly a true duplicate and is finished with one lane per
// cycle (scan_queue.inc: drain; scan_dense.inc: k_dense_verify).
__device__ inline int finish_from(int k) { return 8 + 4 * max(k, 0); }

// Pointers that reach a kernel through memory (the ScanRare block, a late-loaded kernel argument) are generic
// ("flat") addresses to the compiler, and ONE flat access anywhere in a kernel - even on a once-in-a-thousand
// path - makes every later wait on a load a full `s_waitcnt vmcnt(0)`: flat operations may return out of
// order, so the wait-count pass stops counting (SIInsertWaitcnts: pending flat).  They are device-global by
// contract (include/welldup.h), so the rare paths say so too.
template <class T>
using gptr = __attribute__((address_space(1))) T *;
template <class T>
__device__ inline gptr<T> as_gptr(T *p) { return (gptr<T>)p; }
__device__ inline unsigned long long g_atomic_add(unsigned long long *p, unsigned long long v)
{
    return __hip_atomic_fetch_add(as_gptr(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline uint32_t g_atomic_add(uint32_t *p, uint32_t v)
{
    return __hip_atomic_fetch_add(as_gptr(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ inline uint32_t g_atomic_or(uint32_t *p, uint32_t v)
{
    return __hip_atomic_fetch_or(as_gptr(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
