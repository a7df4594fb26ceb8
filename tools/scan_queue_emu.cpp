// scan_queue_emu.cpp - k_scan_q (csrc/scan_queue.inc) run on the CPU under shuffled schedules: the kernel's source is
// compiled as it stands, the 256 lanes of a workgroup are fibers (tools/wave_emu.h), a ballot, a shuffle, a readlane
// and the wave's barrier are rendezvous of the wave, and every atomic - the LDS adds of q_record_dup and q_finish_all,
// the hit log's place claim, the tallies - is a point at which the schedule may hand over to another lane.
//
// A case is launched as launch_queue_t / launch_queue_lev_t (csrc/welldup_queue.hip) launch it: a grid of tiles x
// chunks workgroups of kBlock lanes, which the kernel walks through its own XCD mapping, tpb targets per workgroup and
// the dynamic LDS block of scan_q_lds_dwords(levels, tpb, 2) dwords - the host's own figure, not one of this file's.
// The two seams of the kernel source: WD_DYNAMIC_LDS (csrc/device_common.inc) is here a heap block of exactly the
// launch's bytes, and late_arg reads its offset from a heap copy of the ScanArgs, sizeof(ScanArgs) bytes long.
// WD_Q_CHECK, empty on the device, counts here the drains entered with items still to come (and notes the queue's
// occupancy at each), the passes finished in place, the q_finish_all calls and the pushes, and asserts the occupancy the
// kernel's comments promise.
// TO WHOEVER REWRITES THE KERNEL: the lanes of a wave run in lockstep, these fibers do not, so the push hook
// (WD_Q_CHECK(push, ..)) is here a rendezvous of the wave that the kernel does not have - without it a fiber that is
// through q_finish_all would push over queue entries another fiber has not read yet.  The price: this program cannot
// see a q_wave_sync that is missing between the end of a drain and the next push.  A rewrite that lets one wave's
// push race another wave's read there, or moves the hook, has to be judged by reading; the GPU tests are the check.
//
// Every buffer is a heap allocation of its own with no slack - nbr exactly lvl_off[T][levels] entries, centre, lvl_off,
// perm, the filters, the hit array (hit_cap records), out_per_target and out_tile as the ABI says, a pointer-table
// plane n bytes, a strided tile L * n, an interleaved tile ceil(L / 4) groups of 4 n bytes - so that the address
// sanitizer is the check on every clamp of the kernel's unconditional loads.
//
// Instantiated: what the launchers can launch for the two default families - k_scan_q<false|true, 1..8, 0, 1>,
// <true, 4, 0, 4> (equality / Hamming), <false|true, 4|5|6, kLev2Closed, 1> and <true, 8, kLev2Closed, 4> (Levenshtein
// <= 2 by the closed form).  The banded DP (LEVH 1..3, 16-byte queue entries) runs in tools/scan_lev_emu.cpp, with the two
// other kernels of Levenshtein <= k.
//
// The cases are not made here: tests/test_scanq_emu.py writes each case of tests/scanq_cases.py into a file, and this
// program takes the files as its arguments (tools/scan_emu_common.h says what a file holds; the sibling,
// tools/scan_lines_emu.cpp, reads the same format).
// Every case runs under the eleven schedules of tools/emu_reads.h, the workgroups permuted in all but the first; under
// each one out_tile, out_per_target (WD_INVALID_TARGET rows included), the status word and hit_count must be the
// file's, and the records below hit_cap distinct records of the file's set (all of it, where the cap is not reached) -
// their order is the schedule's, and `orders` counts the different ones.  Prints a line per case; MISMATCH and exit 1
// on a difference.  Control builds (tests/test_scanq_emu.py): -DWAVE_EMU_TORN_ADD, an add that another fiber may cut
// in two; -DSCANQ_EMU_SHORT_LDS, the LDS block without the last wave's second queue buffer; -DSCANQ_EMU_SHORT_NBR, nbr
// one entry short.
// No GPU is involved; the emulation is sequentially consistent and says nothing about caches, time or the memory model.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude tools/scan_queue_emu.cpp -o scan_queue_emu
#define WD_EMU 1                                    // (csrc/wd_shared.h without HIP; the two seams of the kernel source)
#include "../well_duplicates_amd/csrc/wd_shared.h"  // kWave .. kMaxPasses, ScanArgs, ScanRare: the library's own
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
static std::set<int> g_mid_qn;                      // the queue's occupancy at every drain entered with items still to come
static void emu_q_check(int event, int value, bool bound, const char *name, const char *text)
{
    if (!bound) { printf("MISMATCH bound at %s: %s does not hold, value %d (lane %d)\n", name, text, value, emu_lane); fflush(stdout); abort(); }
    if (emu_lane % kWave == 0) g_events[event]++;   // (every lane of the wave passes: counted once)
    if (event == kEv_drain_mid) g_mid_qn.insert(value);
    // The lanes of a wave run in lockstep, the fibers do not: a drain that ends in q_finish_all ends with every lane
    // reading its queue entries, and the pushes that follow it in the program follow it in every lane.  Here a fiber
    // that is through would push over entries another has not read yet - so the push is a rendezvous of the wave.
    if (event == kEv_push) (void)__ballot(false);
}
#define WD_Q_CHECK(event, value, bound) emu_q_check(kEv_##event, (value), (bound), #event, #bound)

#include "../well_duplicates_amd/csrc/device_common.inc"
#include "../well_duplicates_amd/csrc/scan_sequential.inc"
#include "../well_duplicates_amd/csrc/lev2_stream.inc"
#include "../well_duplicates_amd/csrc/scan_queue.inc"

static ScanArgs A;
template <bool S, int B1, int H, int WS> static void call_() { k_scan_q<S, B1, H, WS>(A); }
typedef void (*Kernel)();
static Kernel pick(bool strided, int B1, int levh, int ws)
{
#define Q(S, B, H, W) if (strided == S && B1 == B && levh == H && ws == W) return call_<S, B, H, W>;
    Q(false, 1, 0, 1) Q(false, 2, 0, 1) Q(false, 3, 0, 1) Q(false, 4, 0, 1) Q(false, 5, 0, 1) Q(false, 6, 0, 1) Q(false, 7, 0, 1) Q(false, 8, 0, 1)
    Q(true, 1, 0, 1) Q(true, 2, 0, 1) Q(true, 3, 0, 1) Q(true, 4, 0, 1) Q(true, 5, 0, 1) Q(true, 6, 0, 1) Q(true, 7, 0, 1) Q(true, 8, 0, 1)
    Q(true, 4, 0, 4)
    Q(false, 4, kLev2Closed, 1) Q(false, 5, kLev2Closed, 1) Q(false, 6, kLev2Closed, 1)
    Q(true, 4, kLev2Closed, 1) Q(true, 5, kLev2Closed, 1) Q(true, 6, kLev2Closed, 1)
    Q(true, 8, kLev2Closed, 4)
#undef Q
    return nullptr;
}

static size_t g_lds_bytes = 0;
static void after_block(unsigned, unsigned) { memset(emu_dynamic_lds, 0xA5, g_lds_bytes); }        // (LDS is nobody's between workgroups)

// one schedule of one case: one launch.  Returns 0 if everything is the file's.
static int run_schedule(const CaseFile &c, Inputs &in, Kernel kernel, int s, unsigned seed, long &points, uint64_t &order_hash)
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
    A.T = T; A.levels = levels; A.L = c.L; A.k = c.k; A.tpb = c.tpb; A.early = 1; A.check_empty = c.check_empty; A.log_hits = c.hit_cap >= 0;
    Exact<char> kernarg(sizeof(ScanArgs));
    memcpy(kernarg.p, &A, sizeof(ScanArgs));
    emu_kernarg = kernarg.p;
    // the launch of launch_queue_t / launch_queue_lev_t: tiles x chunks workgroups, the LDS bytes of the host's own figure
    const size_t lds = (size_t)scan_q_lds_dwords(levels, c.tpb, 2) * sizeof(uint32_t);
#ifdef SCANQ_EMU_SHORT_LDS
    g_lds_bytes = lds - (size_t)kQCap * sizeof(uint2);                   // (the control build: without the last wave's second queue buffer)
#else
    g_lds_bytes = lds;
#endif
    Exact<uint32_t> lds_block(g_lds_bytes / sizeof(uint32_t));
    emu_dynamic_lds = lds_block.p;
    const int chunks = (T + c.tpb - 1) / c.tpb;
    points += run_grid((unsigned)(chunks * c.tiles), 1, kernel, permute).points;
    emu_dynamic_lds = nullptr; emu_kernarg = nullptr;

    int bad = 0;
    if (status[0] != (uint32_t)c.status) bad |= fail_(c, s, "status", 0, status[0], c.status);
    for (size_t i = 0; i < out_tile.n; i++)
        if ((long long)out_tile[i] != c.want_tile[i]) { bad |= fail_(c, s, "out_tile", (long)i, (long long)out_tile[i], c.want_tile[i]); break; }
    for (size_t i = 0; i < out_pt.n; i++)
        if (out_pt[i] != c.want_pt[i]) { bad |= fail_(c, s, "out_per_target", (long)i, out_pt[i], c.want_pt[i]); break; }
    if (c.hit_cap >= 0) {
        bad |= check_hits(c, s, hit_count[0], hits, order_hash);
    }
    return bad;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: scan_queue_emu CASE_FILE...\n"); return 2; }
    emu_after_block = after_block;
    int bad = 0;
    for (int a = 1; a < argc; a++) {
        CaseFile c;
        if (!read_case(argv[a], c, kMaxPasses * kPass)) { fprintf(stderr, "%s: not a case file\n", argv[a]); return 2; }
        const bool strided = c.layout != 0;
        const int levh = c.fam ? kLev2Closed : 0, ws = c.layout == 2 ? 4 : 1;
        const Kernel kernel = pick(strided, c.B1, levh, ws);
        if (!kernel) { fprintf(stderr, "%s: no such instantiation\n", argv[a]); return 2; }
        Inputs in(c);
        for (long &e : g_events) e = 0;
        g_mid_qn.clear();
        long points = 0, launches = 0;
        std::set<uint64_t> orders;
        int failed = 0, schedules = 0;
        for (int s = 0; s < kSchedules && !failed; s++) {
            uint64_t order_hash = 0;
            failed = run_schedule(c, in, kernel, s, (unsigned)a, points, order_hash);
            orders.insert(order_hash); launches++; schedules++;
        }
        bad += failed;
        std::string mid_qn;
        for (int v : g_mid_qn) mid_qn += (mid_qn.empty() ? "" : ",") + std::to_string(v);
        if (!failed)
            printf("case %s ok: kernel k_scan_q<%s, %d, %d, %d> n %d tiles %d T %d levels %d L %d k %d tpb %d schedules %d launches %ld points %ld "
                   "mid_drains %ld drains %ld in_place %ld finish_all %ld pushes %ld hits %d orders %zu mid_qn %s\n",
                   c.name.c_str(), strided ? "true" : "false", c.B1, levh, ws, c.n, c.tiles, c.T, c.levels, c.L, c.k, c.tpb, schedules, launches,
                   points, g_events[kEv_drain_mid], g_events[kEv_drain], g_events[kEv_in_place], g_events[kEv_finish_all], g_events[kEv_push],
                   c.hit_cap >= 0 ? c.hits : -1, orders.size(), mid_qn.empty() ? "-" : mid_qn.c_str());
        fflush(stdout);
    }
    return bad ? 1 : 0;
}
