// scan_dense_emu.cpp - the dense chain (csrc/scan_dense.inc) run on the CPU under shuffled schedules: the sibling of
// tools/scan_queue_emu.cpp and tools/scan_lines_emu.cpp, whose heads say what the emulation is (fibers for the lanes
// of a workgroup, rendezvous for the wave's collectives, a scheduling point at every atomic) and what it is not
// (lockstep, caches, time, the memory model).  The kernels' source is compiled as it stands.
//
// A case is launched as ensure_dense_tables and launch_dense (csrc/welldup_dense.hip) launch it, in their order and
// with their grids: k_transpose_off, k_transpose_nbr<int16_t> (and <int32_t> when the flag asks for it),
// k_dense_symcheck, k_dense_windows; then per part k_dense_sig, k_dense_counts, k_dense_pairs_win and / or
// k_dense_pairs, k_dense_mark (Levenshtein), k_dense_rank_words, k_dense_rank_blocks, k_dense_pack, k_dense_verify,
// k_dense_reduce.  The arithmetic of a launch - strides, the clamp of q_per, win_bufs and npc, the LDS bytes, the
// grids, kpad, the group bases, the list of gather blocks, the parts - is the library's own (csrc/dense_launch.inc),
// and between kernels the decisions are taken from the words the host reads: tblflags, ginfo, guni, centre[0].
// Parts run one after the other on two alternating scratch sets, which start dirty (0xA5) and stay dirty.
// Workgroups have 64, 256 (kMarkBlock too) and 1024 lanes here (WAVE_EMU_MAX_BLOCK, emu_block of tools/wave_emu.h).
//
// Every buffer is a heap block of exactly its size (Exact<>): the inputs, every table (nbr_t and udelta at their int16
// or int32 size), sig and sig2 (the last tile's row N words long, not sig_stride: no kernel writes the padding),
// partial, mask and mark at the strides the chain declares (dense_clear_scratch writes them as uint4), queue, q_cnt,
// cand (kDenseSlots + 1 words), wprefix, bprefix, rows (tiles x N x kRowGroups), the outputs, the hit array, the
// ScanRare block and the dynamic LDS block of each compare launch, which is poisoned between workgroups.  (The static
// __shared__ arrays of the other kernels are the program's static storage: neither exact nor poisoned.)
//
// THE LDS-DMA MODEL.  On the device a DMA piece (lds_dma_dword) is one instruction of the wave, and so is a wait.  The
// fibers of a wave are not in lockstep, so both are rendezvous of the wave here - for the reason scan_queue_emu.cpp
// gives for its push hook, and at the same price: this program cannot see an ordering between a wave's own LDS reads
// and its next issue that only lockstep provides, nor one the rendezvous itself supplies.  A lane's source dword is
// read at issue, under the sanitizer.  It reaches LDS in one of two modes, and every case runs under both:
//   late   a piece lands only when a wait requires it - a wait for vmcnt(n) retires the wave's oldest pieces until n
//          remain - and between issue and landing its destination dwords hold poison: a wait that is too lenient;
//   early  a piece lands at issue: an issue into a window that is still being compared.
// Pieces alone are counted: in the one-ended (SYM) kernels nothing else is in flight in the tile loop but what the
// overflow path issues behind them, which can only make the device wait for more; every other wait is vmcnt(0).
// Pieces still in flight when a workgroup ends are a MISMATCH.
//
// Before any scan the tables are checked element by element against the numpy reference of tests/dense_cases.py
// (the case file's `extra`), window tables of the window groups only - a gather group's rows are nobody's.  The table
// kernels and the scan run under the eleven schedules of tools/emu_reads.h (workgroups permuted in all but the
// first), the scan in both DMA modes, and under each out_tile, out_per_target
// (WD_INVALID_TARGET rows included), the status word, the hit count and the hit records (scan-wide tile numbers; a set)
// must be the file's.  Prints a line per case; MISMATCH and exit 1 on a difference.
// Controls (tests/test_dense_emu.py), chosen by a first argument --control=NAME so that they cost no build each:
// lenient_wait, every wait one piece too lenient; early_issue, the one-ended kernel asks for tile ti + ahead_max one
// window early, into the window tile ti is about to be compared in (early sees the other tile's signatures, late the poison); short_lds, the LDS block without the last wave's last queue;
// short_nbrt, nbr_t one entry short; short_rows, rows one row short; skip_clear, the first counter slot and the first
// mask word of a part dirty again after the clear; and, in a build with -DWAVE_EMU_TORN_OR -DWAVE_EMU_TORN_ADD
// (tools/wave_emu.h), torn_or and torn_add: an or / an add that another fiber may cut in two.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude tools/scan_dense_emu.cpp -o scan_dense_emu
#define WD_EMU 1
#include "../well_duplicates_amd/csrc/wd_shared.h"
#define WAVE_EMU_UNIT_DEFS
#define WAVE_EMU_MAX_BLOCK 1024
#include "wave_emu.h"
#include "emu_reads.h"
#include "scan_emu_common.h"
#include <climits>
#include <cstddef>
#include <memory>

// ---- what wave_emu.h does not have and these kernels use
#define blockDim (D3{(unsigned)emu_block, 1, 1})
#define __clz __builtin_clz
#define __builtin_amdgcn_sched_barrier(x) ((void)0)
static int2 make_int2(int x, int y) { return int2{x, y}; }
static int __shfl_xor(int v, int d) { return __shfl(v, (emu_lane % kWave) ^ d); }
static int __all(bool p) { return __ballot(!p) == 0; }                  // (of the lanes that stand there)
static int __any(bool p) { return __ballot(p) != 0; }
// v_perm_b32 (dense_forms.inc: transpose4x4), as tools/dense_forms_check.cpp models it: byte i of the result is byte
// sel.byte[i] of the eight source bytes {s0, s1}, s1 the low four
static uint32_t perm_b32(uint32_t s0, uint32_t s1, uint32_t sel)
{
    const uint64_t src = ((uint64_t)s0 << 32) | s1;
    uint32_t out = 0;
    for (int i = 0; i < 4; i++) {
        const uint32_t b = (sel >> (8 * i)) & 0xFFu;
        if (b > 7u) { fprintf(stderr, "perm selector %u: only 0..7 are modelled\n", b); exit(2); }
        out |= (uint32_t)((src >> (8 * b)) & 0xFFu) << (8 * i);
    }
    return out;
}
#define __builtin_amdgcn_perm perm_b32
#define WD_HD
template <class T, class U> static T atomicMax(T *p, U v) { emu_point(); T o = *p; if ((T)v > o) *p = (T)v; return o; }

// ---- the seams of csrc/scan_dense.inc
enum Control { kNoControl, kLenientWait, kShortLds, kShortNbrt, kShortRows, kSkipClear, kControl_early_issue, kTornOr, kTornAdd };
static const char *const kControlName[] = {"", "lenient_wait", "short_lds", "short_nbrt", "short_rows", "skip_clear", "early_issue", "torn_or", "torn_add"};
static int g_control = kNoControl;
static bool emu_dense_control(int c) { return g_control == c; }
static uint32_t *emu_dynamic_lds = nullptr;         // the launch's LDS block (WD_DYNAMIC_LDS)
static size_t g_lds_bytes = 0;
static int g_dma_early = 0;                         // the mode: 0 late, 1 early
static long g_pieces = 0, g_dma_left = 0;
constexpr uint32_t kDmaPoison = 0xDEADD0A5u;
struct DmaPiece { uint32_t *dst; uint32_t val; };
static std::vector<DmaPiece> emu_dma_q[kEmuMaxBlock];     // per lane: its dwords of the wave's pieces in flight, oldest first
static size_t emu_dma_head[kEmuMaxBlock];
static uint32_t emu_lds_addr(const void *p) { return (uint32_t)((const char *)p - (const char *)emu_dynamic_lds); }
static void emu_dma_issue(const void *base, uint32_t voff, uint32_t lds)
{
    (void)__ballot(false);                          // one instruction of the wave: every lane is done with what came before
    const uint32_t v = *(const uint32_t *)((const char *)base + voff);
    uint32_t *dst = (uint32_t *)((char *)emu_dynamic_lds + lds) + emu_lane % kWave;
    if (emu_lane % kWave == 0) g_pieces++;
    if (g_dma_early) { *dst = v; return; }
    // (a different word in every dword: under one poison word a window and the centres' own signatures in it would all
    // be "equal", every queue would overflow, and the in-place finish would put the counts right again)
    *dst = kDmaPoison ^ ((uint32_t)(uintptr_t)dst * 2654435761u);
    emu_dma_q[emu_lane].push_back(DmaPiece{dst, v});
}
static void emu_dma_wait(int n)
{
    if (g_control == kLenientWait) n++;
    std::vector<DmaPiece> &q = emu_dma_q[emu_lane];
    size_t &h = emu_dma_head[emu_lane];
    while (q.size() - h > (size_t)n) { *q[h].dst = q[h].val; h++; }
    (void)__ballot(false);                          // the wave goes on when every lane's dwords have landed
}
enum { kNote_overflow_win, kNote_overflow_gather, kNotes };
static long g_notes[kNotes];
static void emu_dense_note(int e) { if (emu_lane % kWave == 0) g_notes[e]++; }

#include "../well_duplicates_amd/csrc/device_common.inc"
#include "../well_duplicates_amd/csrc/lev2_stream.inc"
#include "../well_duplicates_amd/csrc/scan_dense.inc"

static void after_block(unsigned, unsigned)
{
    if (emu_dynamic_lds) memset(emu_dynamic_lds, 0xA5, g_lds_bytes);     // (LDS is nobody's between workgroups)
    for (int t = 0; t < kEmuMaxBlock; t++) {
        g_dma_left += (long)(emu_dma_q[t].size() - emu_dma_head[t]);
        emu_dma_q[t].clear(); emu_dma_head[t] = 0;
    }
}

// ---- launches: the kernel's arguments in statics, the kernel behind a plain function
static DenseArgs D;
template <void (*K)(DenseArgs)> static void call_d() { K(D); }
static std::set<std::string> g_ran;                 // the instantiations of this case
static long g_launches = 0;
static long launch(const char *name, void (*k)(), unsigned gx, unsigned gy, int block, bool permute)
{
    g_ran.insert(name); g_launches++;
    emu_block = block;
    return run_grid(gx, gy, k, permute).points;
}

// ---- the options and expectations of a case: the file's `extra` (tests/dense_cases.py: write_case)
enum { X_MAGIC, X_SYM, X_WINDOWS, X_PACK, X_QCAP, X_CHUNK, X_NT, X_OVERLAP, X_PART, X_PACKBLOCKS, X_MISALIGN,
       X_CONST0, X_IDX16 = X_CONST0 + 8, X_SYM_ON, X_KPAD, X_WINMAX, X_GROUPS, X_TOTAL, X_HEAD };
static int tables_fail(const CaseFile &c, const char *what, long at, long long got, long long want)
{
    printf("MISMATCH case %s tables: %s %ld: %lld want %lld\n", c.name.c_str(), what, at, got, want);
    return 1;
}

struct Tables {
    std::unique_ptr<Exact<long long>> gbase;
    std::unique_ptr<Exact<int32_t>> rel_t, ginfo, wdelta, pblocks, nbr32, ud32;
    std::unique_ptr<Exact<int16_t>> nbr16, ud16;
    std::unique_ptr<Exact<uint8_t>> guni, wlev, wfull;
    std::unique_ptr<Exact<uint16_t>> uoff;
    std::unique_ptr<Exact<int2>> useg;
    std::unique_ptr<Exact<uint32_t>> wmask;
    Exact<uint32_t> flags{3};
    bool idx16 = true, sym_on = false;
    int groups = 0, kpad = 0, win_dwords = 0, n_pblocks = 0, n_window = 0, n_uniform = 0, centre0 = 0;
    long long total = 0;
    int64_t k_max = 0;
    const void *nbr_t() const { return idx16 ? (const void *)nbr16->p : (const void *)nbr32->p; }
    const void *udelta() const { return idx16 ? (const void *)ud16->p : (const void *)ud32->p; }
};

// arguments of the table kernels
static struct { const int32_t *centre, *off, *nbr; const long long *gbase; void *nbr_t, *udelta; uint8_t *guni; int T, levels, kpad, half;
                uint32_t *flags; int32_t *rel_t, *ginfo, *wdelta; int2 *useg; uint16_t *uoff; uint8_t *wlev, *wfull; uint32_t *wmask; } TA;
static void call_transpose_off() { k_transpose_off(TA.off, TA.rel_t, TA.T, TA.levels); }
static void call_transpose16() { k_transpose_nbr<int16_t>(TA.centre, TA.off, TA.nbr, TA.gbase, (int16_t *)TA.nbr_t, TA.T, TA.levels, TA.flags, (int16_t *)TA.udelta, TA.guni); }
static void call_transpose32() { k_transpose_nbr<int32_t>(TA.centre, TA.off, TA.nbr, TA.gbase, (int32_t *)TA.nbr_t, TA.T, TA.levels, TA.flags, (int32_t *)TA.udelta, TA.guni); }
static void call_symcheck() { k_dense_symcheck(TA.centre, TA.off, TA.nbr, TA.T, TA.levels, TA.flags + 2); }
static void call_windows() { k_dense_windows(TA.centre, TA.off, TA.nbr, TA.T, TA.levels, TA.kpad, TA.ginfo, TA.useg, TA.uoff, TA.wdelta, TA.wlev, TA.wmask, TA.flags + 1, TA.half, TA.wfull); }

// arguments of k_dense_reduce(partial, stride, ncnt, out_tile + t0 * ncnt)
static struct { const unsigned long long *partial; int stride, ncnt; unsigned long long *out; } RA;
static void call_reduce() { k_dense_reduce(RA.partial, RA.stride, RA.ncnt, RA.out); }

// ensure_dense_tables
static void build_tables(const CaseFile &c, Inputs &in, const std::vector<int32_t> &x, Tables &tb, bool permute)
{
    const int T = c.T, levels = c.levels;
    const size_t row = (size_t)levels + 1;
    for (int t = 0; t < T; t++) tb.k_max = std::max<int64_t>(tb.k_max, (int64_t)c.off[(size_t)t * row + levels] - c.off[(size_t)t * row]);
    std::vector<long long> gbase;
    dense_group_bases(c.off.data(), T, levels, gbase);
    tb.groups = (T + kWave - 1) / kWave;
    tb.total = gbase.back();
    tb.gbase.reset(new Exact<long long>(gbase.size()));
    std::copy(gbase.begin(), gbase.end(), tb.gbase->p);
    tb.rel_t.reset(new Exact<int32_t>((size_t)T * levels));
    tb.guni.reset(new Exact<uint8_t>((size_t)tb.groups));
    TA = {};
    TA.centre = in.centre.p; TA.off = in.off.p; TA.nbr = in.nbr.p; TA.gbase = tb.gbase->p; TA.guni = tb.guni->p; TA.T = T; TA.levels = levels;
    TA.flags = tb.flags.p; TA.rel_t = tb.rel_t->p;
    launch("k_transpose_off", call_transpose_off, (unsigned)((T + kBlock - 1) / kBlock), 1, kBlock, permute);
    const size_t n_el = (size_t)tb.total - (g_control == kShortNbrt ? 1 : 0);      // (the control: the last entry is nobody's)
    tb.nbr16.reset(new Exact<int16_t>(n_el));
    tb.ud16.reset(new Exact<int16_t>((size_t)(tb.total / kWave)));
    tb.flags[0] = tb.flags[1] = 0;
    TA.nbr_t = tb.nbr16->p; TA.udelta = tb.ud16->p;
    launch("k_transpose_nbr<int16_t>", call_transpose16, (unsigned)tb.groups, 1, kWave, permute);
    if (tb.flags[0]) {
        tb.idx16 = false;
        tb.nbr16.reset(); tb.ud16.reset();
        tb.nbr32.reset(new Exact<int32_t>(n_el));
        tb.ud32.reset(new Exact<int32_t>((size_t)(tb.total / kWave)));
        TA.nbr_t = tb.nbr32->p; TA.udelta = tb.ud32->p;
        launch("k_transpose_nbr<int32_t>", call_transpose32, (unsigned)tb.groups, 1, kWave, permute);
    }
    if (x[X_SYM] && T >= 2) {
        tb.flags[2] = 0;
        launch("k_dense_symcheck", call_symcheck, (unsigned)((T + kBlock - 1) / kBlock), 1, kBlock, permute);
        tb.sym_on = tb.flags[2] == 0;
        tb.centre0 = in.centre[0];
    }
    tb.kpad = dense_kpad(tb.k_max);
    std::vector<int32_t> ginfo((size_t)tb.groups, 0);
    if (tb.kpad > 0) {
        const size_t g = (size_t)tb.groups, kp = (size_t)tb.kpad;
        tb.ginfo.reset(new Exact<int32_t>(g)); tb.uoff.reset(new Exact<uint16_t>(g * kp)); tb.useg.reset(new Exact<int2>(g * kMaxSeg));
        tb.wdelta.reset(new Exact<int32_t>(g * kp)); tb.wlev.reset(new Exact<uint8_t>(g * kp)); tb.wfull.reset(new Exact<uint8_t>(g * kp));
        tb.wmask.reset(new Exact<uint32_t>(g * (kp / 32) * kWave));
        memset(tb.ginfo->p, 0, g * sizeof(int32_t));
        TA.kpad = tb.kpad; TA.half = tb.sym_on ? 1 : 0; TA.ginfo = tb.ginfo->p; TA.useg = tb.useg->p; TA.uoff = tb.uoff->p; TA.wdelta = tb.wdelta->p;
        TA.wlev = tb.wlev->p; TA.wfull = tb.wfull->p; TA.wmask = tb.wmask->p;
        launch("k_dense_windows", call_windows, (unsigned)tb.groups, 1, kWave, permute);
        tb.win_dwords = dense_win_dwords_of(tb.flags[1]);
        std::copy(tb.ginfo->p, tb.ginfo->p + g, ginfo.begin());
    }
    for (int g = 0; g < tb.groups; g++) { tb.n_uniform += (*tb.guni)[(size_t)g] != 0; tb.n_window += ginfo[(size_t)g] != 0; }
    std::vector<int32_t> pb;
    dense_pblocks(ginfo.data(), tb.groups, pb);
    tb.n_pblocks = (int)pb.size();
    tb.pblocks.reset(new Exact<int32_t>(pb.size()));
    std::copy(pb.begin(), pb.end(), tb.pblocks->p);
}

// every table element against the numpy reference
static int check_tables(const CaseFile &c, const std::vector<int32_t> &x, const Tables &tb)
{
    const int T = c.T, levels = c.levels;
    if (x[X_GROUPS] != tb.groups) return tables_fail(c, "groups", 0, tb.groups, x[X_GROUPS]);
    if (x[X_TOTAL] != tb.total) return tables_fail(c, "entries of nbr_t", 0, tb.total, x[X_TOTAL]);
    if (x[X_IDX16] != (int)tb.idx16) return tables_fail(c, "int16 table", 0, tb.idx16, x[X_IDX16]);
    if (x[X_SYM_ON] != (int)tb.sym_on) return tables_fail(c, "symmetric verdict", 0, tb.sym_on, x[X_SYM_ON]);
    if (x[X_KPAD] != tb.kpad) return tables_fail(c, "kpad", 0, tb.kpad, x[X_KPAD]);
    if (tb.kpad && (uint32_t)x[X_WINMAX] != tb.flags.p[1]) return tables_fail(c, "win_max", 0, tb.flags.p[1], x[X_WINMAX]);
    const size_t G = (size_t)tb.groups, total = (size_t)tb.total, kp = (size_t)tb.kpad;
    size_t need = X_HEAD + (G + 1) + 2 * G + total + total / kWave + (size_t)T * levels;
    if (x.size() < need) return tables_fail(c, "words of the expectation", 0, (long long)x.size(), (long long)need);
    const int32_t *e = x.data() + X_HEAD;
    for (size_t i = 0; i <= G; i++) if ((*tb.gbase)[i] != e[i]) return tables_fail(c, "gbase", (long)i, (*tb.gbase)[i], e[i]);
    e += G + 1;
    for (size_t i = 0; i < G; i++) if ((*tb.guni)[i] != e[i]) return tables_fail(c, "guni", (long)i, (*tb.guni)[i], e[i]);
    e += G;
    const int32_t *eg = e;
    for (size_t i = 0; i < G; i++) { const int32_t got = tb.kpad ? (*tb.ginfo)[i] : 0; if (got != e[i]) return tables_fail(c, "ginfo", (long)i, got, e[i]); }
    e += G;
    for (size_t i = 0; i < total; i++) { const int32_t got = tb.idx16 ? (*tb.nbr16)[i] : (*tb.nbr32)[i]; if (got != e[i]) return tables_fail(c, "nbr_t", (long)i, got, e[i]); }
    e += total;
    for (size_t i = 0; i < total / kWave; i++) { const int32_t got = tb.idx16 ? (*tb.ud16)[i] : (*tb.ud32)[i]; if (got != e[i]) return tables_fail(c, "udelta", (long)i, got, e[i]); }
    e += total / kWave;
    for (size_t i = 0; i < (size_t)T * levels; i++) if ((*tb.rel_t)[i] != e[i]) return tables_fail(c, "rel_t", (long)i, (*tb.rel_t)[i], e[i]);
    e += (size_t)T * levels;
    for (size_t g = 0; g < G; g++) {
        if (!eg[g]) continue;
        const size_t nrun = (size_t)((eg[g] >> 9) & 31);
        need += 2 * nrun + 4 * kp + (kp / 32) * kWave;
        if (x.size() < need) return tables_fail(c, "words of the expectation (window tables)", (long)g, (long long)x.size(), (long long)need);
        for (size_t r = 0; r < nrun; r++) {
            const int2 u = (*tb.useg)[g * kMaxSeg + r];
            if (u.x != e[2 * r] || u.y != e[2 * r + 1]) return tables_fail(c, "useg", (long)(g * kMaxSeg + r), u.x, e[2 * r]);
        }
        e += 2 * nrun;
        for (size_t p = 0; p < kp; p++) if ((*tb.uoff)[g * kp + p] != e[p]) return tables_fail(c, "uoff", (long)(g * kp + p), (*tb.uoff)[g * kp + p], e[p]);
        e += kp;
        for (size_t p = 0; p < kp; p++) if ((*tb.wdelta)[g * kp + p] != e[p]) return tables_fail(c, "wdelta", (long)(g * kp + p), (*tb.wdelta)[g * kp + p], e[p]);
        e += kp;
        for (size_t p = 0; p < kp; p++) if ((*tb.wlev)[g * kp + p] != e[p]) return tables_fail(c, "wlev", (long)(g * kp + p), (*tb.wlev)[g * kp + p], e[p]);
        e += kp;
        for (size_t p = 0; p < kp; p++) if ((*tb.wfull)[g * kp + p] != e[p]) return tables_fail(c, "wfull", (long)(g * kp + p), (*tb.wfull)[g * kp + p], e[p]);
        e += kp;
        for (size_t p = 0; p < (kp / 32) * kWave; p++) {
            const uint32_t got = (*tb.wmask)[g * (kp / 32) * kWave + p];
            if (got != (uint32_t)e[p]) return tables_fail(c, "wmask", (long)(g * (kp / 32) * kWave + p), got, (uint32_t)e[p]);
        }
        e += (kp / 32) * kWave;
    }
    if (x.size() != need) return tables_fail(c, "words of the expectation (behind the tables)", 0, (long long)x.size(), (long long)need);
    return 0;
}

// one scratch set of a scan, every block exact; dirty from its birth
struct Scratch {
    Exact<uint32_t> sig, sig2, mask, q_cnt, cand, mark, wprefix, bprefix;
    Exact<unsigned long long> partial;
    Exact<uint2> queue;
    Exact<uint4> rows;
    Scratch(const DenseShape &s, int part, long long N, bool two_sigs, bool want_rows)
        : sig((size_t)(part - 1) * s.sig_stride + N), sig2(two_sigs ? (size_t)(part - 1) * s.sig_stride + N : 0),
          mask((size_t)part * s.mask_stride), q_cnt((size_t)part * s.n_groups), cand(kDenseSlots + 1), mark((size_t)part * s.mw_stride),
          wprefix((size_t)part * s.mw_stride), bprefix((size_t)part * (s.mw_stride / kMarkBlock)),
          partial((size_t)part * kDenseSlots * s.partial_stride), queue((size_t)part * s.n_groups * s.q_per),
          rows(want_rows ? (size_t)part * N * kRowGroups - (g_control == kShortRows ? kRowGroups : 0) : 0) {}     // (the control: the last row is nobody's)
};

struct RunStats { long points = 0, queued = 0, over_regions = 0, packed_parts = 0, parts = 0; int npc = 0, win_bufs = 0, tc_last = 0; };

#define DK(...) #__VA_ARGS__, call_d<__VA_ARGS__>
// launch_dense: one scan under one schedule and one DMA mode.  Returns 0 if everything is the file's.
static int run_scan(const CaseFile &c, Inputs &in, const std::vector<int32_t> &x, const Tables &tb, int s, unsigned seed, RunStats &st, uint64_t &order_hash)
{
    const bool permute = set_schedule(s, seed);
    const int T = c.T, levels = c.levels, ncnt = 1 + 5 * levels, n_tiles = c.tiles;
    const long long N = c.n;
    const bool strided = c.layout != 0, lev2 = c.fam == 1 && c.k == 2 && c.L <= 40 * kRowGroups;
    Exact<unsigned long long> out_tile((size_t)n_tiles * ncnt);
    Exact<uint32_t> out_pt(c.has_pt ? (size_t)n_tiles * T * levels : 0);
    Exact<uint32_t> status(1);
    Exact<unsigned long long> hit_count(1);
    Exact<wd_hit> hits(c.hit_cap > 0 ? (size_t)c.hit_cap : 0);
    Exact<ScanRare> rare(1);
    memset(out_tile.p, 0, out_tile.n * sizeof(unsigned long long));     // (wd_scan_async clears the tile counters and the hit count)
    status[0] = 0; hit_count[0] = 0;
    rare[0] = ScanRare{status.p, hits.p, hit_count.p, (long long)std::max(c.hit_cap, 0)};

    const int tile_chunk = dense_tile_chunk_of(x[X_CHUNK], n_tiles);
    const int part = dense_part_tiles_of(x[X_OVERLAP] != 0, x[X_PART], n_tiles, tile_chunk);
    const int n_parts = (n_tiles + part - 1) / part, n_sets = n_parts > 1 ? 2 : 1;
    DenseArgs d = {};
    d.stride = in.stride; d.centre = in.centre.p; d.lvl_off = in.off.p; d.nbr_t = tb.nbr_t(); d.idx16 = tb.idx16 ? 1 : 0;
    d.rel_t = tb.rel_t->p; d.udelta = tb.udelta(); d.guni = tb.guni->p;
    d.ginfo = (x[X_WINDOWS] && tb.ginfo) ? tb.ginfo->p : nullptr;
    if (tb.kpad) { d.uoff = tb.uoff->p; d.useg = tb.useg->p; d.wdelta = tb.wdelta->p; d.wlev = tb.wlev->p; d.wmask = tb.wmask->p; d.wfull = tb.wfull->p; }
    d.sym = tb.sym_on ? 1 : 0; d.centre0 = tb.centre0; d.kpad = tb.kpad; d.gbase = tb.gbase->p; d.rare = rare.p;
    d.N = N; d.T = T; d.levels = levels; d.L = c.L; d.k = c.k; d.sig_cycles = std::min(kSigCycles, c.L); d.strided = strided ? 1 : 0;
    d.check_empty = c.check_empty; d.log_hits = c.hit_cap > 0 ? 1 : 0;
    const DenseShape shp = dense_shape(N, T, levels, tile_chunk, x[X_QCAP], lev2, d.sym != 0, d.ginfo != nullptr, tb.win_dwords);
    d.sig_stride = shp.sig_stride; d.partial_stride = shp.partial_stride; d.mask_stride = shp.mask_stride; d.q_per = shp.q_per;
    d.win_bufs = shp.win_bufs; d.win_dwords = shp.win_dwords; d.mw_stride = shp.mw_stride;
    st.npc = shp.npc; st.win_bufs = shp.win_bufs;
    d.pack_mode = x[X_PACK]; d.lev2 = lev2 ? 1 : 0; d.nbr = in.nbr.p;
    const bool want_rows = (d.pack_mode != 0 || lev2) && c.L > d.sig_cycles && c.L <= 40 * kRowGroups;
    const bool two_sigs = lev2 || c.k > 0;
    std::unique_ptr<Scratch> sets[2];
    for (int i = 0; i < n_sets; i++) sets[i].reset(new Scratch(shp, part, N, two_sigs, want_rows));
    bool aligned4 = (in.stride & 3) == 0;
    for (size_t i = 0; i < in.planes.n && aligned4; i++) aligned4 = ((uintptr_t)in.planes[i] & 3u) == 0;
    const int pmode = lev2 ? 2 : (c.k == 0 ? 0 : 1);
    const long long n_groups = shp.n_groups;
    for (int cpart = 0; cpart < n_parts; cpart++) {
        const int t0 = cpart * part, nt = std::min(part, n_tiles - t0);
        Scratch &sc = *sets[cpart & 1];
        d.pblocks = d.ginfo ? tb.pblocks->p : nullptr;
        d.n_pblocks = d.ginfo ? tb.n_pblocks : 0;
        const DensePart prt = dense_part(shp, N, T, nt, tile_chunk, d.n_pblocks);
        d.planes = in.planes.p + (strided ? (size_t)t0 : (size_t)t0 * c.L);
        d.filter = in.filter.p + t0;
        d.out_per_target = out_pt.p ? out_pt.p + (size_t)t0 * T * levels : nullptr;
        d.tile0 = t0; d.n_tiles = nt; d.tile_chunk = prt.tc; st.tc_last = prt.tc;
        d.sig = sc.sig.p; d.sig2 = two_sigs ? sc.sig2.p : nullptr;
        d.partial = sc.partial.p; d.mask = sc.mask.p; d.queue = sc.queue.p; d.q_cnt = sc.q_cnt.p;
        d.mark = sc.mark.p; d.wprefix = sc.wprefix.p; d.bprefix = sc.bprefix.p; d.cand = sc.cand.p;
        d.rows = want_rows ? sc.rows.p : nullptr;
        D = d;
        if (aligned4 && strided) st.points += launch(DK(k_dense_sig<true, true>), prt.wells4, (unsigned)nt, kBlock, permute);
        else if (aligned4) st.points += launch(DK(k_dense_sig<true, false>), prt.wells4, (unsigned)nt, kBlock, permute);
        else if (strided) st.points += launch(DK(k_dense_sig<false, true>), prt.wells1, (unsigned)nt, kBlock, permute);
        else st.points += launch(DK(k_dense_sig<false, false>), prt.wells1, (unsigned)nt, kBlock, permute);
        if (g_control == kSkipClear) { memset(sc.partial.p, 0xA5, sizeof(unsigned long long)); memset(sc.mask.p, 0xA5, sizeof(uint32_t)); }
        st.points += launch(DK(k_dense_counts), prt.counts_x, prt.chunks, kBlock, permute);
        // the compare stage: its LDS block, exactly the host's bytes
        g_lds_bytes = prt.q_lds - (g_control == kShortLds ? (size_t)2 * d.q_per * sizeof(uint32_t) : 0);      // (the control: without the last wave's last queue)
        Exact<uint32_t> lds_block(g_lds_bytes / sizeof(uint32_t));
        emu_dynamic_lds = lds_block.p;
        const bool gather = tb.n_window < n_groups || !d.ginfo;
#define PAIRS(MODE, SYM)                                                                                                           \
        do {                                                                                                                       \
            if (d.ginfo) st.points += launch(DK(k_dense_pairs_win<MODE, SYM, 0>), prt.pairs, 1, kBlock, permute);                  \
            if (gather) {                                                                                                          \
                if (tb.idx16) st.points += launch(DK(k_dense_pairs<MODE, true, SYM>), prt.pairs_listed, 1, kBlock, permute);       \
                else st.points += launch(DK(k_dense_pairs<MODE, false, SYM>), prt.pairs_listed, 1, kBlock, permute);               \
            }                                                                                                                      \
        } while (0)
#define PAIRS_N(MODE, NPC)                                                                                                         \
        do {                                                                                                                       \
            st.points += launch(DK(k_dense_pairs_win<MODE, true, NPC>), prt.pairs, 1, kBlock, permute);                            \
            if (tb.n_window < n_groups) {                                                                                          \
                if (tb.idx16) st.points += launch(DK(k_dense_pairs<MODE, true, true>), prt.pairs_listed, 1, kBlock, permute);      \
                else st.points += launch(DK(k_dense_pairs<MODE, false, true>), prt.pairs_listed, 1, kBlock, permute);              \
            }                                                                                                                      \
        } while (0)
#define PAIRS_SYM(MODE)                                                                                                            \
        do {                                                                                                                       \
            switch (shp.npc) {                                                                                                     \
            case 4: PAIRS_N(MODE, 4); break;                                                                                       \
            case 5: PAIRS_N(MODE, 5); break;                                                                                       \
            case 6: PAIRS_N(MODE, 6); break;                                                                                       \
            case 8: PAIRS_N(MODE, 8); break;                                                                                       \
            default: PAIRS(MODE, true); break;                                                                                     \
            }                                                                                                                      \
        } while (0)
        if (pmode == 0 && d.sym) PAIRS_SYM(0);
        else if (pmode == 0) PAIRS(0, false);
        else if (pmode == 1 && d.sym) PAIRS_SYM(1);
        else if (pmode == 1) PAIRS(1, false);
        else if (d.sym) PAIRS_SYM(2);
        else PAIRS(2, false);
#undef PAIRS_SYM
#undef PAIRS_N
#undef PAIRS
        emu_dynamic_lds = nullptr;
        for (size_t r = 0; r < (size_t)nt * n_groups; r++) { const uint32_t q = sc.q_cnt[r]; if (q == 0xFFFFFFFFu) st.over_regions++; else st.queued += q; }
        if (lev2) st.points += launch(DK(k_dense_mark), shp.mark_blocks, (unsigned)nt, kBlock, permute);
        if (d.rows) {
            st.points += launch(DK(k_dense_rank_words), prt.rank_words, (unsigned)nt, kMarkBlock, permute);
            st.points += launch(DK(k_dense_rank_blocks), (unsigned)nt, 1, kRankBlock, permute);
            const unsigned pg4 = dense_pack_grid_x(prt.wells4, n_parts > 1, x[X_PACKBLOCKS], nt), pg1 = dense_pack_grid_x(prt.wells1, n_parts > 1, x[X_PACKBLOCKS], nt);
            if (aligned4 && strided && x[X_NT]) st.points += launch(DK(k_dense_pack<4, true, true>), pg4, (unsigned)nt, kBlock, permute);
            else if (aligned4 && strided) st.points += launch(DK(k_dense_pack<4, true>), pg4, (unsigned)nt, kBlock, permute);
            else if (aligned4) st.points += launch(DK(k_dense_pack<4, false>), pg4, (unsigned)nt, kBlock, permute);
            else if (strided) st.points += launch(DK(k_dense_pack<1, true>), pg1, (unsigned)nt, kBlock, permute);
            else st.points += launch(DK(k_dense_pack<1, false>), pg1, (unsigned)nt, kBlock, permute);
        }
        if (strided) st.points += launch(DK(k_dense_verify<true>), prt.verify_x, (unsigned)nt, kBlock, permute);
        else st.points += launch(DK(k_dense_verify<false>), prt.verify_x, (unsigned)nt, kBlock, permute);
        st.parts++;
        st.packed_parts += d.rows && (sc.cand[kDenseSlots] || d.pack_mode > 0 || (d.pack_mode != 0 && sc.cand[0]));      // (dense_packed)
        // k_dense_reduce(partial, stride, ncnt, out_tile + t0 * ncnt)
        RA = {d.partial, d.partial_stride, ncnt, out_tile.p + (size_t)t0 * ncnt};
        st.points += launch("k_dense_reduce", call_reduce, (unsigned)nt, 1, kWave, permute);
    }
    emu_block = kEmuBlock;

    int bad = 0;
    if (g_dma_left) { bad |= fail_(c, s, "LDS-DMA pieces in flight at the end of a workgroup", 0, g_dma_left, 0); g_dma_left = 0; }
    if (status[0] != (uint32_t)c.status) bad |= fail_(c, s, "status", 0, status[0], c.status);
    for (size_t i = 0; i < out_tile.n; i++)
        if ((long long)out_tile[i] != c.want_tile[i]) { bad |= fail_(c, s, "out_tile", (long)i, (long long)out_tile[i], c.want_tile[i]); break; }
    for (size_t i = 0; i < out_pt.n; i++)
        if (out_pt[i] != c.want_pt[i]) { bad |= fail_(c, s, "out_per_target", (long)i, out_pt[i], c.want_pt[i]); break; }
    if (c.hit_cap > 0) bad |= check_hits(c, s, hit_count[0], hits, order_hash);
    return bad;
}

int main(int argc, char **argv)
{
    int first = 1;
    if (argc > 1 && !strncmp(argv[1], "--control=", 10)) {
        for (int i = 1; i <= kTornAdd; i++) if (!strcmp(argv[1] + 10, kControlName[i])) g_control = i;
        if (!g_control) { fprintf(stderr, "%s: no such control\n", argv[1]); return 2; }
        first = 2;
    }
#if defined(WAVE_EMU_TORN_OR) && defined(WAVE_EMU_TORN_ADD)
    emu_torn_or = g_control == kTornOr; emu_torn_add = g_control == kTornAdd;
#else
    if (g_control >= kTornOr) { fprintf(stderr, "%s: not built with -DWAVE_EMU_TORN_OR -DWAVE_EMU_TORN_ADD\n", argv[1]); return 2; }
#endif
    if (argc <= first) { fprintf(stderr, "usage: scan_dense_emu [--control=NAME] CASE_FILE...\n"); return 2; }
    emu_after_block = after_block;
    int bad = 0;
    for (int a = first; a < argc; a++) {
        CaseFile c;
        if (!read_case(argv[a], c, kDenseMaxK) || c.levels > 8 || c.layout > 1 || c.extra.size() < X_HEAD || c.extra[X_MAGIC] != 0x31534E44) {
            fprintf(stderr, "%s: not a case file of the dense chain\n", argv[a]); return 2;
        }
        const std::vector<int32_t> &x = c.extra;
        const int consts[8] = {kSigCycles, kMaxSeg, kWinMaxK, kWinGap, kWinDwords, kMarkBlock, kWinBufs, kWinBufsSym};
        for (int i = 0; i < 8; i++) if (x[X_CONST0 + i] != consts[i]) { fprintf(stderr, "%s: constant %d is %d here, the case assumes %d\n", argv[a], i, consts[i], x[X_CONST0 + i]); return 2; }
        Inputs in(c);
        // a pointer table whose planes lie 1 to 3 bytes off alignment (each still ends where its block ends)
        std::vector<std::unique_ptr<Exact<uint8_t>>> odd;
        if (x[X_MISALIGN] && c.layout == 0)
            for (size_t i = 0; i < in.planes.n; i++) {
                const size_t by = 1 + i % 3;
                odd.emplace_back(new Exact<uint8_t>((size_t)c.n + by));
                memcpy(odd.back()->p + by, in.planes[i], (size_t)c.n);
                in.planes[i] = odd.back()->p + by;
            }
        g_ran.clear(); g_launches = 0; g_pieces = 0; g_dma_left = 0;
        for (long &n : g_notes) n = 0;
        // the tables: built and checked under every schedule (their atomics: the wide flag's or, win_max's maximum); the
        // scans read those of the last
        std::unique_ptr<Tables> tbp;
        int tables_bad = 0;
        for (int s = 0; s < kSchedules && !tables_bad; s++) {
            const bool permute = set_schedule(s, (unsigned)a);
            tbp.reset(new Tables);
            build_tables(c, in, x, *tbp, permute);
            tables_bad = check_tables(c, x, *tbp);
        }
        if (tables_bad) { bad++; fflush(stdout); continue; }
        Tables &tb = *tbp;
        RunStats st;
        std::set<uint64_t> orders;
        int failed = 0, runs = 0;
        for (int mode = 0; mode < 2; mode++) {
            g_dma_early = mode;
            int failed_mode = 0;
            for (int s = 0; s < kSchedules && !failed_mode; s++) {
                uint64_t order_hash = 0;
                const long before = g_pieces;
                failed_mode = run_scan(c, in, x, tb, s, (unsigned)a, st, order_hash);
                if (failed_mode) printf("MISMATCH case %s under dma %s (pieces %ld)\n", c.name.c_str(), mode ? "early" : "late", g_pieces - before);
                orders.insert(order_hash); runs++;
            }
            failed |= failed_mode;
        }
        bad += failed;
        std::string ran;
        for (const std::string &k : g_ran) ran += (ran.empty() ? "" : "; ") + k;
        if (!failed)
            printf("case %s ok: n %d tiles %d T %d levels %d L %d k %d groups %d window %d uniform %d idx16 %d sym %d kpad %d win_dwords %d win_bufs %d npc %d "
                   "tc %d parts %ld runs %d launches %ld points %ld pieces %ld queued %ld overflow_win %ld overflow_gather %ld over_regions %ld packed %ld "
                   "hits %d orders %zu kernels [%s]\n",
                   c.name.c_str(), c.n, c.tiles, c.T, c.levels, c.L, c.k, tb.groups, tb.n_window, tb.n_uniform, (int)tb.idx16, (int)tb.sym_on, tb.kpad,
                   tb.win_dwords, st.win_bufs, st.npc, st.tc_last, st.parts / std::max(runs, 1), runs, g_launches, st.points, g_pieces, st.queued,
                   g_notes[kNote_overflow_win], g_notes[kNote_overflow_gather], st.over_regions, st.packed_parts, c.hit_cap > 0 ? c.hits : -1,
                   orders.size(), ran.c_str());
        fflush(stdout);
    }
    return bad ? 1 : 0;
}
