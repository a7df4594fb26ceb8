// scan_lev_emu.cpp - the three kernels that run Levenshtein <= k by the banded DP, k >= 2, on the CPU under shuffled
// schedules, as tools/scan_queue_emu.cpp runs the two default families of k_scan_q: the kernels' source is compiled as it
// stands, the lanes of a workgroup are fibers (tools/wave_emu.h), a ballot, a readlane, a readfirstlane and the wave's
// barrier are rendezvous of the wave, and every atomic is a point at which the schedule may hand over to another lane.
//
//   k_scan_q<S, B1, LEVH, WS>, LEVH = 1 .. 3 (csrc/scan_queue.inc): launched as launch_queue_lev_t (csrc/welldup_queue.hip)
//       launches it - tiles x chunks workgroups of kBlock lanes, the dynamic LDS block of scan_q_lds_dwords(levels, tpb, 4)
//       dwords, the host's own figure (the queue entries are 16 bytes: lev_pack / lev_unpack, q_drain_lev).  WD_Q_CHECK
//       counts the drains, the pushes and the compactions and asserts the occupancies; the push hook is the rendezvous
//       of the wave that tools/scan_queue_emu.cpp documents, with the price it names.
//   k_scan<LevState<H>, S, lev_first(H), 8>, H in {1, 2, 3, 4, 6, 8} (csrc/scan_sequential.inc): launch_lev's grid
//       (csrc/welldup_scan.hip), static LDS, ScanArgs.early 1 or 0 as the case says.
//   k_scan_lev_generic<S> (csrc/scan_lev_generic.inc): T x tiles workgroups of one wave; its LDS block - WD_DYNAMIC_LDS,
//       csrc/device_common.inc - is a heap block of exactly lev_generic_lds_bytes(L, H) bytes, so that the carve-up (row,
//       wcode, ccode) is checked by the address sanitizer at every case.
//
// Every buffer is a heap allocation of its own with no slack (tools/scan_emu_common.h: Exact<>, Inputs), the kernel
// argument block of k_scan_q included (late_arg).  The cases are tests/levk_cases.py's, written by tests/test_levk_emu.py
// (family word 2; behind the hit records {kind 0 queue / 1 k_scan / 2 generic, band half-width, early}).  Every case runs
// under the eleven schedules of tools/emu_reads.h, the workgroups permuted in all but the first; under each one out_tile,
// out_per_target (WD_INVALID_TARGET rows included), the status word, hit_count and the hit records with their distances
// must be the file's.  Prints a line per case; MISMATCH and exit 1 on a difference.
//
// --state FILE...: no kernel, LevState<H> alone (and lev_pack / lev_unpack for H <= 3) against the textbook distance,
// driven as the kernels drive it - push per cycle, alive() behind every round of the schedule (k_scan_q's 1, 2, 4, 8, 8 ..
// behind its first round, 4, 8, 8 .. interleaved, k_scan's batches of 8), for H <= 3 a pack / unpack round trip there,
// finish(), dup(), dist().  For every H and k = 2 H, 2 H + 1: every pair of reads over {A, C, N} of 1 .. 6 cycles (both orders:
// all ordered pairs); then every pair of the files, both orders, with the file's band and threshold.
//
// Control builds (tests/test_levk_emu.py): -DLEVK_EMU_NARROW, the band one diagonal short - the kernels are handed k / 2 - 1
// where the launchers hand k / 2 (the templated ones are instantiated with H - 1); -DWD_LEV_CELL_MASK=7, lev_pack keeps
// three bits of a band cell; -DLEVK_EMU_SHORT_LDS, the generic kernel's LDS block kWave bytes short; -DSCANQ_EMU_SHORT_NBR,
// nbr one entry short.  -DLEVK_EMU_KINDS=mask compiles some of the three kinds only (a control build's time is its compiler's).
// No GPU is involved; the emulation is sequentially consistent and says nothing about caches, time, the memory model or
// what the device compiler makes of the same source.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude tools/scan_lev_emu.cpp -o scan_lev_emu
#define WD_EMU 1                                    // (csrc/wd_shared.h without HIP; the seams of the kernel source)
#include "../well_duplicates_amd/csrc/wd_shared.h"  // kWave .. kMaxPasses, lev_first, ScanArgs, ScanRare: the library's own
#define WAVE_EMU_UNIT_DEFS                          // (none of wave_emu.h's tiledups constants, nor lane_pass.inc)
#include "wave_emu.h"
#include "emu_reads.h"
#include "scan_emu_common.h"                        // Exact<>, the case file, Inputs, the hit records' check
#include <cstddef>
#include <type_traits>

static uint32_t *emu_dynamic_lds = nullptr;         // the launch's LDS block (WD_DYNAMIC_LDS)
static const char *emu_kernarg = nullptr;           // the launch's ScanArgs, as the kernarg segment holds it (late_arg)
enum { kEv_drain, kEv_drain_mid, kEv_in_place, kEv_finish_all, kEv_push, kEv_compact, kEvents };
static long g_events[kEvents];
static void emu_q_check(int event, int value, bool bound, const char *name, const char *text)
{
    if (!bound) { printf("MISMATCH bound at %s: %s does not hold, value %d (lane %d)\n", name, text, value, emu_lane); fflush(stdout); abort(); }
    if (emu_lane % kWave == 0) g_events[event]++;   // (every lane of the wave passes: counted once)
    if (event == kEv_push) (void)__ballot(false);   // (tools/scan_queue_emu.cpp: the lanes run in lockstep, the fibers do not)
}
#define WD_Q_CHECK(event, value, bound) emu_q_check(kEv_##event, (value), (bound), #event, #bound)

#include "../well_duplicates_amd/csrc/device_common.inc"
#include "../well_duplicates_amd/csrc/scan_sequential.inc"
#include "../well_duplicates_amd/csrc/lev2_stream.inc"
#include "../well_duplicates_amd/csrc/scan_queue.inc"
#include "../well_duplicates_amd/csrc/scan_lev_generic.inc"

constexpr int kEmuLevB2 = 8;                        // kLevB2 (csrc/welldup_scan.hip; tests/test_levk_emu.py holds it to the source)
#ifdef LEVK_EMU_NARROW
constexpr int kNarrow = 1;                          // (the control build: the band one diagonal short)
#else
constexpr int kNarrow = 0;
#endif
enum { kKindQueue, kKindSeq, kKindGeneric };
#ifndef LEVK_EMU_KINDS                              // (a control build compiles the kinds it concerns: 1 k_scan_q, 2 k_scan, 4 the generic kernel)
#define LEVK_EMU_KINDS 7
#endif

static ScanArgs A;
static int g_generic_h = 0;
template <bool S, int B1, int H, int WS> static void call_q() { k_scan_q<S, B1, H - kNarrow, WS>(A); }
template <int H, bool S> static void call_seq() { k_scan<LevState<H - kNarrow>, S, lev_first(H), kEmuLevB2>(A); }
template <bool S> static void call_generic() { k_scan_lev_generic<S>(A, g_generic_h - kNarrow); }
typedef void (*Kernel)();
static Kernel pick(int kind, bool strided, int B1, int h, int ws)
{
#if LEVK_EMU_KINDS & 4
    if (kind == kKindGeneric) return strided ? call_generic<true> : call_generic<false>;
#endif
#if LEVK_EMU_KINDS & 1
#define Q(S, B, H, W) if (kind == kKindQueue && strided == S && B1 == B && h == H && ws == W) return call_q<S, B, H, W>;
#else
#define Q(S, B, H, W)
#endif
#if LEVK_EMU_KINDS & 2
#define K(H) if (kind == kKindSeq && h == H && B1 == lev_first(H)) return strided ? call_seq<H, true> : call_seq<H, false>;
#else
#define K(H)
#endif
#ifndef LEVK_EMU_NARROW                             // (a band of no diagonal but the main one is another family's kernel)
    Q(false, 5, 1, 1) Q(true, 5, 1, 1) Q(false, 6, 1, 1) Q(true, 6, 1, 1) Q(true, 8, 1, 4)
    K(1)
#endif
    Q(false, 8, 2, 1) Q(true, 8, 2, 1) Q(false, 11, 2, 1) Q(true, 11, 2, 1)
    Q(false, 13, 3, 1) Q(true, 13, 3, 1) Q(false, 14, 3, 1) Q(true, 14, 3, 1)
    K(2) K(3) K(4) K(6) K(8)
#undef Q
#undef K
    return nullptr;
}

static size_t g_lds_bytes = 0;
static void after_block(unsigned, unsigned) { if (emu_dynamic_lds) memset(emu_dynamic_lds, 0xA5, g_lds_bytes); }      // (LDS is nobody's between workgroups)

// one schedule of one case: one launch.  Returns 0 if everything is the file's.
static int run_schedule(const CaseFile &c, Inputs &in, Kernel kernel, int kind, int h, int early, int s, unsigned seed, long &points, uint64_t &order_hash)
{
    const bool permute = set_schedule(s, seed);
    const int T = c.T, levels = c.levels, ncnt = 1 + 5 * levels;
    Exact<unsigned long long> out_tile((size_t)c.tiles * ncnt);
    Exact<uint32_t> out_pt(c.has_pt ? (size_t)c.tiles * T * levels : 0);
    Exact<uint32_t> status(1);
    Exact<unsigned long long> hit_count(1);
    Exact<wd_hit> hits(c.hit_cap > 0 ? (size_t)c.hit_cap : 0);
    Exact<ScanRare> rare(1);
    memset(out_tile.p, 0, out_tile.n * sizeof(unsigned long long));     // (wd_scan_async clears the tile counters and the hit count)
    status[0] = 0; hit_count[0] = 0;
    rare[0] = ScanRare{status.p, hits.p, hit_count.p, (long long)std::max(c.hit_cap, 0)};
    A = ScanArgs{};
    A.planes = in.planes.p; A.filter = in.filter.p; A.stride = in.stride;
    A.centre = in.centre.p; A.lvl_off = in.off.p; A.nbr = in.nbr.p;
    A.out_tile = out_tile.p; A.out_per_target = out_pt.p; A.rare = rare.p; A.perm = in.perm.p;
    A.T = T; A.levels = levels; A.L = c.L; A.k = c.k; A.tpb = c.tpb; A.early = early; A.check_empty = c.check_empty; A.log_hits = c.hit_cap >= 0;
    Exact<char> kernarg(sizeof(ScanArgs));
    memcpy(kernarg.p, &A, sizeof(ScanArgs));
    emu_kernarg = kernarg.p;
    // the launches of launch_queue_lev_t, launch_lev and wd_scan_async's generic branch: the grid, the lanes, the LDS bytes
    size_t lds = 0;
    unsigned grid = (unsigned)(((T + c.tpb - 1) / c.tpb) * c.tiles);
    emu_block = kBlock;
    if (kind == kKindQueue) lds = (size_t)scan_q_lds_dwords(levels, c.tpb, 4) * sizeof(uint32_t);
    if (kind == kKindGeneric) { lds = lev_generic_lds_bytes(c.L, h); grid = (unsigned)(T * c.tiles); emu_block = kWave; g_generic_h = h; }
#ifdef LEVK_EMU_SHORT_LDS
    if (kind == kKindGeneric) lds -= kWave;                                  // (the control build)
#endif
    g_lds_bytes = lds;
    Exact<uint8_t> lds_block(lds);
    emu_dynamic_lds = (uint32_t *)lds_block.p;
    points += run_grid(grid, 1, kernel, permute).points;
    emu_dynamic_lds = nullptr; emu_kernarg = nullptr; emu_block = kBlock;

    int bad = 0;
    if (status[0] != (uint32_t)c.status) bad |= fail_(c, s, "status", 0, status[0], c.status);
    for (size_t i = 0; i < out_tile.n; i++)
        if ((long long)out_tile[i] != c.want_tile[i]) { bad |= fail_(c, s, "out_tile", (long)i, (long long)out_tile[i], c.want_tile[i]); break; }
    for (size_t i = 0; i < out_pt.n; i++)
        if (out_pt[i] != c.want_pt[i]) { bad |= fail_(c, s, "out_per_target", (long)i, out_pt[i], c.want_pt[i]); break; }
    if (c.hit_cap >= 0)
        bad |= check_hits(c, s, hit_count[0], hits, order_hash);
    return bad;
}

static std::string kernel_name(int kind, bool strided, int B1, int h, int ws)
{
    char b[96];
    const char *S = strided ? "true" : "false";
    if (kind == kKindQueue) snprintf(b, sizeof(b), "k_scan_q<%s, %d, %d, %d>", S, B1, h, ws);
    else if (kind == kKindSeq) snprintf(b, sizeof(b), "k_scan<LevState<%d>, %s, %d, %d>", h, S, lev_first(h), kEmuLevB2);
    else snprintf(b, sizeof(b), "k_scan_lev_generic<%s>", S);
    return b;
}

// ---- the state alone -------------------------------------------------------------------------------------------------
static int textbook(const uint8_t *a, const uint8_t *b, int L)
{
    std::vector<int> prev(L + 1), cur(L + 1);
    for (int j = 0; j <= L; j++) prev[j] = j;
    for (int i = 1; i <= L; i++) {
        cur[0] = i;
        for (int j = 1; j <= L; j++) cur[j] = std::min(std::min(prev[j] + 1, cur[j - 1] + 1), prev[j - 1] + (a[i - 1] != b[j - 1]));
        prev.swap(cur);
    }
    return prev[L];
}

// the cycles behind which alive() is asked: sched 0 k_scan_q on planes (first round B1, then 1, 2, 4, 8, 8 ..), 1 interleaved
// (8, then 4, 8, 8 ..), 2 k_scan (lev_first(H), then 8, 8 ..)
static std::vector<int> rounds_of(int sched, int H, int k, int L)
{
    const int first_even = lev_first(H) - (H <= 2 ? 2 : 0), first_odd = lev_first(H) + 1 - (H == 1 ? 2 : 0);      // launch_queue_lev_t
    int j = sched == 0 ? ((k & 1) ? first_odd : first_even) : sched == 1 ? 8 : lev_first(H);
    int nb = sched == 0 ? 1 : sched == 1 ? 4 : kEmuLevB2;
    std::vector<int> out;
    while (j < L) { out.push_back(j); j += nb; nb = sched == 2 ? kEmuLevB2 : std::min(8, nb * 2); }
    return out;
}

static long g_state_runs = 0;
// c: the centre's codes, w: the well's (0 .. 3 bases, 4 the no-call: code_of's).  Returns 0 if the state says what the textbook says.
template <int H>
static int state_pair(const uint8_t *c, const uint8_t *w, int L, int k, int sched, const char *what)
{
    const int cap = k + 1, want = textbook(c, w, L);
    const std::vector<int> rounds = rounds_of(sched, H, k, L);
    LevState<H> st;
    st.init(cap);
    uint64_t ch = ~0ull;
    size_t r = 0;
    g_state_runs++;
    for (int p = 1; p <= L; p++) {
        ch = (ch << 3) | c[p - 1];
        st.push(p, ch, c[p - 1], w[p - 1], L, cap);
        if (r < rounds.size() && rounds[r] == p) {
            r++;
            if (!st.alive(k, p, ch, L, cap) && want <= k) {
                printf("MISMATCH state %s: LevState<%d> k %d L %d schedule %d: alive() false behind cycle %d, distance %d\n", what, H, k, L, sched, p, want);
                return 1;
            }
            if constexpr (H <= 3) {
                if (sched != 2) {                   // the queue entry between two rounds
                    LevState<H> back;
                    uint64_t ch2;
                    lev_unpack<H>(lev_pack<H>(st, ch), back, ch2);
                    st = back; ch = ch2;
                }
            }
        }
    }
    st.finish(L, ch, cap, k);
    if (st.dup(k) != (want <= k) || (want <= k && st.dist() != want)) {
        printf("MISMATCH state %s: LevState<%d> k %d L %d schedule %d: dup %d dist %d, distance %d\n", what, H, k, L, sched, (int)st.dup(k), st.dist(), want);
        return 1;
    }
    return 0;
}

template <int H>
static int state_exhaustive()
{
    int bad = 0;
    const uint8_t letters[3] = {0, 1, 4};
    for (int k = 2 * H; k <= 2 * H + 1; k++)
        for (int sched = H <= 3 ? 0 : 2; sched <= 2 && !bad; sched++) {
            if (sched == 1 && H != 1) continue;     // (the interleaved layout: band half-width 1 alone)
            for (int L = 1; L <= 6 && !bad; L++) {
                int n = 1;
                for (int i = 0; i < L; i++) n *= 3;
                std::vector<uint8_t> reads((size_t)n * L);
                for (int v = 0; v < n; v++) for (int i = 0, q = v; i < L; i++, q /= 3) reads[(size_t)v * L + i] = letters[q % 3];
                for (int x = 0; x < n && !bad; x++) for (int y = 0; y < n && !bad; y++)
                    bad |= state_pair<H>(&reads[(size_t)x * L], &reads[(size_t)y * L], L, k, sched, "exhaustive");
            }
        }
    return bad;
}

static int state_file(const CaseFile &c, int kind, int h)
{
    const int sched = kind == kKindQueue ? (c.layout == 2 ? 1 : 0) : 2;
    int bad = 0;
    std::vector<uint8_t> cen(c.L), nb(c.L);
    for (int tile = 0; tile < c.tiles && !bad; tile++)
        for (int t = 0; t < c.T && !bad; t++) {
            const int32_t *o = &c.off[(size_t)t * (c.levels + 1)];
            for (int j = 0; j < c.L; j++) cen[j] = (uint8_t)code_of(c.plane(tile, j)[c.centre[t]]);
            for (int p = o[0]; p < o[c.levels] && !bad; p++) {
                for (int j = 0; j < c.L; j++) nb[j] = (uint8_t)code_of(c.plane(tile, j)[c.nbr[p]]);
                for (int order = 0; order < 2 && !bad; order++) {
                    const uint8_t *a = order ? nb.data() : cen.data(), *b = order ? cen.data() : nb.data();
                    switch (h) {
                    case 1: bad |= state_pair<1>(a, b, c.L, c.k, sched, c.name.c_str()); break;
                    case 2: bad |= state_pair<2>(a, b, c.L, c.k, sched, c.name.c_str()); break;
                    case 3: bad |= state_pair<3>(a, b, c.L, c.k, sched, c.name.c_str()); break;
                    case 4: bad |= state_pair<4>(a, b, c.L, c.k, sched, c.name.c_str()); break;
                    case 6: bad |= state_pair<6>(a, b, c.L, c.k, sched, c.name.c_str()); break;
                    case 8: bad |= state_pair<8>(a, b, c.L, c.k, sched, c.name.c_str()); break;
                    default: break;                 // (the generic kernel keeps no LevState)
                    }
                }
            }
        }
    return bad;
}

int main(int argc, char **argv)
{
    const bool state = argc >= 2 && !strcmp(argv[1], "--state");
    if (argc < 2) { fprintf(stderr, "usage: scan_lev_emu [--state] CASE_FILE...\n"); return 2; }
    emu_after_block = after_block;
    int bad = 0;
    if (state) {
        bad |= state_exhaustive<1>() | state_exhaustive<2>() | state_exhaustive<3>() | state_exhaustive<4>() | state_exhaustive<6>() | state_exhaustive<8>();
        printf("state exhaustive %s: pairs over {A, C, N} of 1 .. 6 cycles, runs %ld\n", bad ? "MISMATCH" : "ok", g_state_runs);
    }
    for (int a = state ? 2 : 1; a < argc; a++) {
        CaseFile c;
        if (!read_case(argv[a], c, 1 << 20) || c.fam != 2 || c.extra.size() != 3) { fprintf(stderr, "%s: not a case file of the banded DP\n", argv[a]); return 2; }
        const int kind = c.extra[0], h = c.extra[1], early = c.extra[2];
        const bool strided = c.layout != 0;
        const int ws = c.layout == 2 ? 4 : 1;
        if (state) {
            const long before = g_state_runs;
            const int failed = state_file(c, kind, h);
            bad += failed;
            if (!failed) printf("state %s ok: band %d k %d L %d runs %ld\n", c.name.c_str(), h, c.k, c.L, g_state_runs - before);
            continue;
        }
        const Kernel kernel = pick(kind, strided, c.B1, h, ws);
        if (!kernel) { fprintf(stderr, "%s: no such instantiation\n", argv[a]); return 2; }
        Inputs in(c);
        for (long &e : g_events) e = 0;
        long points = 0, launches = 0;
        std::set<uint64_t> orders;
        int failed = 0, schedules = 0;
        for (int s = 0; s < kSchedules && !failed; s++) {
            uint64_t order_hash = 0;
            failed = run_schedule(c, in, kernel, kind, h, early, s, (unsigned)a, points, order_hash);
            orders.insert(order_hash); launches++; schedules++;
        }
        bad += failed;
        if (!failed)
            printf("case %s ok: kernel %s n %d tiles %d T %d levels %d L %d k %d tpb %d early %d schedules %d launches %ld points %ld "
                   "mid_drains %ld drains %ld compactions %ld pushes %ld hits %d orders %zu\n",
                   c.name.c_str(), kernel_name(kind, strided, c.B1, h, ws).c_str(), c.n, c.tiles, c.T, c.levels, c.L, c.k, c.tpb, early, schedules,
                   launches, points, g_events[kEv_drain_mid], g_events[kEv_drain], g_events[kEv_compact], g_events[kEv_push],
                   c.hit_cap >= 0 ? c.hits : -1, orders.size());
        fflush(stdout);
    }
    return bad ? 1 : 0;
}
