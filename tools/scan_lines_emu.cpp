// scan_lines_emu.cpp - k_scan_lines (csrc/scan_lines.inc) run on the CPU under shuffled schedules, on the tables the
// library's own make_line_tables (csrc/line_tables.inc) builds: the sibling of tools/scan_queue_emu.cpp, whose head says
// what the emulation is (fibers for the 256 lanes, rendezvous for the wave's collectives - here lw_wave_sum's DPP too -,
// a scheduling point at every atomic) and what it is not (lockstep, caches, time, the memory model).
//
// A case is launched as launch_lines_t (csrc/welldup_lines.hip) launches it: the tables of make_line_tables, called with
// the case's CSR and its line_pairs; mask_stride as the launcher computes it; mask and out_per_target zeroed; perm
// null; lw_blocks x tiles workgroups, which the kernel walks through its own XCD mapping (the workgroups of a launch run
// one after the other here, in a permuted order in all schedules but the first: a target's blocks apply their
// transitions of its hit-level byte in an order the hardware would be free to pick); the dynamic LDS block of
// scan_lines_lds_dwords(levels, tmax) dwords, the host's own figure; the argument block behind late_arg a heap copy of
// the LineArgs, sizeof(LineArgs) bytes.  Every buffer is a heap allocation of its own with no slack - pw, pm, blk, btgt,
// bcen, boff, mask (tiles x mask_stride words), the filters and planes (tools/scan_emu_common.h: Inputs), out_tile,
// out_per_target, the hit array, the LDS block - so that the address sanitizer is the check on min(r, np - 1), on
// idle_well = pw[p0], on the clamps of pp[q] and group_dword and on the LDS carve-up.
//
// Before any kernel runs the tables are checked: element by element against the tables tests/linewalk_cases.py expects
// (a numpy stable argsort by well and a greedy cut; the case file's `extra`: n_blk, tmax, entries of btgt, then pw, pm,
// blk, btgt, bcen, boff - or a single 0 where the walk does not apply, and then the function must say so), and directly:
// pw ascending, the (target, slot) pairs a permutation of the CSR's, equal wells in target-then-slot order, every block
// within both limits, every target's owner bit set exactly once and in the first block that holds one of its pairs,
// tmax a multiple of 4 and the maximum.
//
// Under each of the eleven schedules of tools/emu_reads.h the tile counters, the per-target counts (WD_INVALID_TARGET
// rows included), the status word, the hit count and the hit records (a set) must be the file's, and every byte of
// mask the OR of 1 << level over the levels at which the file's hit records give that target a duplicate on that tile.
// Prints a line per case: the instantiation as the launcher names it, blocks, tmax, the drains entered with items
// still to come (mid_drains; their occupancies: mid_qn), the steps finished in place, the pushes, the targets whose
// pairs lie in more than one block (split), the negative first / last deltas applied (neg_deltas, all schedules), the
// distinct orders of the hit records.  First of all lw_wave_sum is run alone on all ones, the lane's index, one lane
// set (lanes 0, 15, 16, 31, 32, 47, 48, 63), 0xFFFFFFFF everywhere and random words: the plain sum mod 2^32 in every lane.
// MISMATCH and exit 1 on a difference.  Control builds (tests/test_linewalk_emu.py): -DWAVE_EMU_TORN_ADD,
// -DWAVE_EMU_TORN_OR (tools/wave_emu.h); -DSCANL_EMU_SHORT_LDS, the LDS block without the last wave's second queue
// buffer; -DSCANL_EMU_SHORT_PW, pw and pm one entry short; -DSCANL_EMU_SHORT_MASK, mask one word short.
//
// Instantiated: the fourteen the launcher can launch - k_scan_lines<false|true, 2|3|5|6|8, 0, 1>, <true, 4, 0, 4>,
// <false|true, 5, kLev2Closed, 1>, <true, 8, kLev2Closed, 4>.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude tools/scan_lines_emu.cpp -o scan_lines_emu
#define WD_EMU 1                                    // (csrc/wd_shared.h without HIP; the seams of the kernel source)
#include "../well_duplicates_amd/csrc/wd_shared.h"
#define WAVE_EMU_UNIT_DEFS
#include "wave_emu.h"
#include "emu_reads.h"
#include "scan_emu_common.h"
#include <cstddef>
#include <map>
#define __clz __builtin_clz

static uint32_t *emu_dynamic_lds = nullptr;         // the launch's LDS block (WD_DYNAMIC_LDS)
static const char *emu_kernarg = nullptr;           // the launch's LineArgs, as the kernarg segment holds it (late_arg)
static size_t g_lds_bytes = 0;
enum { kEv_drain, kEv_drain_mid, kEv_in_place, kEv_finish_all, kEv_push, kEv_compact, kEvents };
static long g_events[kEvents], g_neg_deltas;
static std::set<int> g_mid_qn;
static void emu_q_check(int event, int value, bool bound, const char *name, const char *text)
{
    if (!bound) { printf("MISMATCH bound at %s: %s does not hold, value %d (lane %d)\n", name, text, value, emu_lane); fflush(stdout); abort(); }
    if (emu_lane % kWave == 0) g_events[event]++;   // (every lane of the wave passes: counted once)
    if (event == kEv_drain_mid) g_mid_qn.insert(value);
    // (the push is a rendezvous of the wave here, as in the sibling and for its reason: fibers are not in lockstep)
    if (event == kEv_push) (void)__ballot(false);
}
#define WD_Q_CHECK(event, value, bound) emu_q_check(kEv_##event, (value), (bound), #event, #bound)
// an add of -1 (mod 2^32) on a word of the LDS block: a first / last hit that moved
static void add_hook(const void *p, long long old)
{
    const char *q = (const char *)p, *lds = (const char *)emu_dynamic_lds;
    if (lds && q >= lds && q < lds + g_lds_bytes && (uint32_t)(*(const uint32_t *)p - (uint32_t)old) == ~0u) g_neg_deltas++;
}

#include "../well_duplicates_amd/csrc/device_common.inc"
#include "../well_duplicates_amd/csrc/scan_sequential.inc"
#include "../well_duplicates_amd/csrc/lev2_stream.inc"
#include "../well_duplicates_amd/csrc/scan_queue.inc"
#include "../well_duplicates_amd/csrc/scan_lines.inc"
#include "../well_duplicates_amd/csrc/line_tables.inc"

static LineArgs A;
template <bool S, int B1, int H, int WS> static void call_() { k_scan_lines<S, B1, H, WS>(A); }
typedef void (*Kernel)();
static Kernel pick(bool strided, int B1, int levh, int ws)
{
#define Q(S, B, H, W) if (strided == S && B1 == B && levh == H && ws == W) return call_<S, B, H, W>;
    Q(false, 2, 0, 1) Q(false, 3, 0, 1) Q(false, 5, 0, 1) Q(false, 6, 0, 1) Q(false, 8, 0, 1)
    Q(true, 2, 0, 1) Q(true, 3, 0, 1) Q(true, 5, 0, 1) Q(true, 6, 0, 1) Q(true, 8, 0, 1)
    Q(true, 4, 0, 4)
    Q(false, 5, kLev2Closed, 1) Q(true, 5, kLev2Closed, 1)
    Q(true, 8, kLev2Closed, 4)
#undef Q
    return nullptr;
}

// ---- lw_wave_sum alone: one workgroup, every wave on its own 64 words
static uint32_t g_sum_in[kBlock], g_sum_out[kBlock];
static void sum_kernel() { g_sum_out[threadIdx.x] = lw_wave_sum(g_sum_in[threadIdx.x]); }
static int selftest_wave_sum()
{
    std::mt19937 rng(12345);
    std::vector<std::vector<uint32_t>> inputs;
    inputs.push_back(std::vector<uint32_t>(kBlock, 1u));
    { std::vector<uint32_t> v(kBlock); for (int i = 0; i < kBlock; i++) v[i] = (uint32_t)(i % kWave); inputs.push_back(v); }
    for (int at : {0, 15, 16, 31, 32, 47, 48, 63}) {
        std::vector<uint32_t> v(kBlock, 0u);
        for (int w = 0; w < kWaves; w++) v[w * kWave + at] = 0x80000001u + (uint32_t)w;
        inputs.push_back(v);
    }
    inputs.push_back(std::vector<uint32_t>(kBlock, 0xFFFFFFFFu));
    for (int r = 0; r < 8; r++) { std::vector<uint32_t> v(kBlock); for (uint32_t &x : v) x = (uint32_t)rng(); inputs.push_back(v); }
    int bad = 0;
    for (int s = 0; s < 3; s++) {                   // never, reverse, always: the rendezvous must not care
        set_schedule(s, 7);
        for (size_t i = 0; i < inputs.size(); i++) {
            std::copy(inputs[i].begin(), inputs[i].end(), g_sum_in);
            memset(g_sum_out, 0xA5, sizeof(g_sum_out));
            g_grid = D3{1, 1, 1};
            run_block(0, 0, sum_kernel);
            for (int l = 0; l < kBlock && !bad; l++) {
                uint32_t want = 0;
                for (int j = 0; j < kWave; j++) want += inputs[i][(size_t)(l / kWave * kWave + j)];
                if (g_sum_out[l] != want) { printf("MISMATCH lw_wave_sum input %zu schedule %d lane %d: %u want %u\n", i, s, l, g_sum_out[l], want); bad = 1; }
            }
        }
    }
    if (!bad) printf("selftest lw_wave_sum passed: inputs %zu\n", inputs.size());
    return bad;
}

// ---- the tables: the library's function against the case file's expectation, and against their own definition
static int tables_fail(const CaseFile &c, const char *what, long at, long long got, long long want)
{
    printf("MISMATCH case %s tables: %s %ld: %lld want %lld\n", c.name.c_str(), what, at, got, want);
    return 1;
}
static int check_tables(const CaseFile &c, bool applies, const LineTables &lt, size_t per_block, int &split)
{
    const std::vector<int32_t> &x = c.extra;
    if (x.empty()) return tables_fail(c, "no expectation in the file", 0, 0, 1);
    if (!applies) return x[0] == 0 ? 0 : tables_fail(c, "the function says: does not apply; blocks", 0, 0, x[0]);
    const size_t P = lt.well.size(), nb = lt.blk.size(), nt = lt.btgt.size(), row = (size_t)c.levels + 1;
    if (x[0] != (int32_t)nb) return tables_fail(c, "blocks", 0, (long long)nb, x[0]);
    if (x.size() < 3 || x[1] != lt.tmax) return tables_fail(c, "tmax", 0, lt.tmax, x.size() < 3 ? -1 : x[1]);
    if (x[2] != (int32_t)nt) return tables_fail(c, "entries of btgt", 0, (long long)nt, x[2]);
    if (x.size() != 3 + 2 * P + 4 * nb + 2 * nt + nt * row) return tables_fail(c, "words of the expectation", 0, (long long)x.size(), (long long)(3 + 2 * P + 4 * nb + 2 * nt + nt * row));
    const int32_t *e = x.data() + 3;
    for (size_t i = 0; i < P; i++) if (lt.well[i] != e[i]) return tables_fail(c, "pw", (long)i, lt.well[i], e[i]);
    e += P;
    for (size_t i = 0; i < P; i++) if (lt.meta[i] != (uint32_t)e[i]) return tables_fail(c, "pm", (long)i, lt.meta[i], (uint32_t)e[i]);
    e += P;
    for (size_t i = 0; i < nb; i++) {
        const int got[4] = {lt.blk[i].x, lt.blk[i].y, lt.blk[i].z, lt.blk[i].w};
        for (int j = 0; j < 4; j++) if (got[j] != e[4 * i + j]) return tables_fail(c, "blk", (long)(4 * i + j), got[j], e[4 * i + j]);
    }
    e += 4 * nb;
    for (size_t i = 0; i < nt; i++) if (lt.btgt[i] != (uint32_t)e[i]) return tables_fail(c, "btgt", (long)i, lt.btgt[i], (uint32_t)e[i]);
    e += nt;
    for (size_t i = 0; i < nt; i++) if (lt.bcen[i] != e[i]) return tables_fail(c, "bcen", (long)i, lt.bcen[i], e[i]);
    e += nt;
    for (size_t i = 0; i < nt * row; i++) if (lt.boff[i] != e[i]) return tables_fail(c, "boff", (long)i, lt.boff[i], e[i]);
    // ... and what the tables are by definition, whatever the reference thinks
    std::vector<char> seen((size_t)c.P, 0);
    std::vector<int> first_block((size_t)c.T, -1), owner_block((size_t)c.T, -1), owners((size_t)c.T, 0), blocks_of((size_t)c.T, 0);
    long prev_well = -1, prev_t = -1, prev_slot = -1;
    int tmax = 0;
    size_t next_pair = 0, next_tgt = 0;
    for (size_t b = 0; b < nb; b++) {
        const int4 d = lt.blk[b];
        if ((size_t)d.x != next_pair || (size_t)d.z != next_tgt) return tables_fail(c, "a block's first pair / first target", (long)b, d.x, (long long)next_pair);
        if (d.y < 1 || (size_t)d.y > per_block || d.w < 1 || d.w > kLwTargets) return tables_fail(c, "a block's limits (pairs)", (long)b, d.y, (long long)per_block);
        next_pair += (size_t)d.y; next_tgt += (size_t)d.w;
        if (next_pair > P || next_tgt > nt) return tables_fail(c, "a block's end", (long)b, (long long)next_pair, (long long)P);
        tmax = std::max(tmax, d.w);
        std::vector<char> used((size_t)d.w, 0);
        for (int i = 0; i < d.w; i++) {
            const uint32_t en = lt.btgt[(size_t)d.z + i];
            const int t = (int)(en & 0x7FFFFFFFu);
            if (t >= c.T) return tables_fail(c, "btgt: target", d.z + i, t, c.T);
            blocks_of[(size_t)t]++;
            if (en >> 31) { owners[(size_t)t]++; owner_block[(size_t)t] = (int)b; }
            if (lt.bcen[(size_t)d.z + i] != c.centre[(size_t)t]) return tables_fail(c, "bcen by definition", d.z + i, lt.bcen[(size_t)d.z + i], c.centre[(size_t)t]);
            for (size_t l = 0; l < row; l++)
                if (lt.boff[((size_t)d.z + i) * row + l] != c.off[(size_t)t * row + l]) return tables_fail(c, "boff by definition", d.z + i, lt.boff[((size_t)d.z + i) * row + l], c.off[(size_t)t * row + l]);
        }
        for (int i = 0; i < d.y; i++) {
            const size_t p = (size_t)d.x + i;
            const uint32_t ltg = lt.meta[p] >> 16, slot = lt.meta[p] & 0xFFFFu;
            if ((int)ltg >= d.w) return tables_fail(c, "pm: local target", (long)p, ltg, d.w);
            used[ltg] = 1;
            const int t = (int)(lt.btgt[(size_t)d.z + ltg] & 0x7FFFFFFFu);
            const int32_t *o = &c.off[(size_t)t * row];
            if ((int32_t)slot >= o[c.levels] - o[0]) return tables_fail(c, "pm: slot", (long)p, slot, o[c.levels] - o[0]);
            const size_t at = (size_t)o[0] + slot;
            if (seen[at]) return tables_fail(c, "a (target, slot) pair twice", (long)p, (long long)at, -1);
            seen[at] = 1;
            if (lt.well[p] != c.nbr[at]) return tables_fail(c, "pw: not the pair's neighbour", (long)p, lt.well[p], c.nbr[at]);
            if (lt.well[p] < prev_well) return tables_fail(c, "pw: not ascending", (long)p, lt.well[p], prev_well);
            if (lt.well[p] == prev_well && (t < prev_t || (t == prev_t && (long)slot <= prev_slot)))
                return tables_fail(c, "equal wells: not in target-then-slot order", (long)p, t, prev_t);
            prev_well = lt.well[p]; prev_t = t; prev_slot = (long)slot;
            if (first_block[(size_t)t] < 0) first_block[(size_t)t] = (int)b;
        }
        for (int i = 0; i < d.w; i++) if (!used[(size_t)i]) return tables_fail(c, "a target of a block without a pair in it", d.z + i, 0, 1);
    }
    if (next_pair != P || next_tgt != nt) return tables_fail(c, "the blocks' pairs", 0, (long long)next_pair, (long long)P);
    size_t csr_pairs = 0;
    for (int t = 0; t < c.T; t++) csr_pairs += (size_t)(c.off[(size_t)t * row + c.levels] - c.off[(size_t)t * row]);
    if (csr_pairs != P) return tables_fail(c, "pairs (the CSR's)", 0, (long long)P, (long long)csr_pairs);
    split = 0;
    for (int t = 0; t < c.T; t++) {
        if (owners[(size_t)t] != 1 || owner_block[(size_t)t] != first_block[(size_t)t])
            return tables_fail(c, "owner bit: once, in the first block of the target", t, owner_block[(size_t)t], first_block[(size_t)t]);
        split += blocks_of[(size_t)t] > 1;
    }
    if (lt.tmax % 4 || lt.tmax != ((tmax + 3) & ~3)) return tables_fail(c, "tmax by definition", 0, lt.tmax, (tmax + 3) & ~3);
    return 0;
}

static void after_block(unsigned, unsigned) { memset(emu_dynamic_lds, 0xA5, g_lds_bytes); }        // (LDS is nobody's between workgroups)

// the tables on the heap, each block exact: made once, read by every schedule
struct Tables {
    Exact<int32_t> pw; Exact<uint32_t> pm; Exact<int4> blk; Exact<uint32_t> btgt; Exact<int32_t> bcen, boff;
#ifdef SCANL_EMU_SHORT_PW
    static constexpr size_t kShort = 1;             // (the control build: the last pair's entries are nobody's)
#else
    static constexpr size_t kShort = 0;
#endif
    explicit Tables(const LineTables &lt)
        : pw(lt.well.size() - kShort), pm(lt.meta.size() - kShort), blk(lt.blk.size()), btgt(lt.btgt.size()), bcen(lt.bcen.size()), boff(lt.boff.size())
    {
        std::copy(lt.well.begin(), lt.well.begin() + pw.n, pw.p);
        std::copy(lt.meta.begin(), lt.meta.begin() + pm.n, pm.p);
        std::copy(lt.blk.begin(), lt.blk.end(), blk.p);
        std::copy(lt.btgt.begin(), lt.btgt.end(), btgt.p);
        std::copy(lt.bcen.begin(), lt.bcen.end(), bcen.p);
        std::copy(lt.boff.begin(), lt.boff.end(), boff.p);
    }
};

// one schedule of one case: one launch.  Returns 0 if everything is the file's.
static int run_schedule(const CaseFile &c, Inputs &in, Tables &tb, const LineTables &lt, Kernel kernel, int s, unsigned seed, long &points, uint64_t &order_hash)
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
    // launch_lines_t
    A = LineArgs{};
    A.s.planes = in.planes.p; A.s.filter = in.filter.p; A.s.stride = in.stride;
    A.s.centre = in.centre.p; A.s.lvl_off = in.off.p; A.s.nbr = in.nbr.p;
    A.s.out_tile = out_tile.p; A.s.out_per_target = out_pt.p; A.s.rare = rare.p; A.s.perm = nullptr;
    A.s.T = T; A.s.levels = levels; A.s.L = c.L; A.s.k = c.k; A.s.tpb = c.tpb; A.s.early = 1; A.s.check_empty = 0; A.s.log_hits = c.hit_cap >= 0;
    A.pw = tb.pw.p; A.pm = tb.pm.p; A.blk = tb.blk.p; A.btgt = tb.btgt.p; A.bcen = tb.bcen.p; A.boff = tb.boff.p;
    A.n_blk = (int)lt.blk.size(); A.tmax = lt.tmax;
    A.mask_stride = (((long long)T + 3) / 4 + 31) & ~31ll;
#ifdef SCANL_EMU_SHORT_MASK
    Exact<uint32_t> mask((size_t)c.tiles * (size_t)A.mask_stride - 1);  // (the control build: the last word is nobody's)
#else
    Exact<uint32_t> mask((size_t)c.tiles * (size_t)A.mask_stride);
#endif
    memset(mask.p, 0, mask.n * sizeof(uint32_t));
    if (out_pt.n) memset(out_pt.p, 0, out_pt.n * sizeof(uint32_t));
    A.mask = mask.p;
    Exact<char> kernarg(sizeof(LineArgs));
    memcpy(kernarg.p, &A, sizeof(LineArgs));
    emu_kernarg = kernarg.p;
    const size_t lds = (size_t)scan_lines_lds_dwords(levels, lt.tmax) * sizeof(uint32_t);
#ifdef SCANL_EMU_SHORT_LDS
    g_lds_bytes = lds - (size_t)kLwQCap * sizeof(uint2);                 // (the control build: without the last wave's second queue buffer)
#else
    g_lds_bytes = lds;
#endif
    Exact<uint32_t> lds_block(g_lds_bytes / sizeof(uint32_t));
    emu_dynamic_lds = lds_block.p;
    points += run_grid((unsigned)(A.n_blk * c.tiles), 1, kernel, permute).points;
    emu_dynamic_lds = nullptr; emu_kernarg = nullptr;

    int bad = 0;
    if (status[0] != (uint32_t)c.status) bad |= fail_(c, s, "status", 0, status[0], c.status);
    for (size_t i = 0; i < out_tile.n; i++)
        if ((long long)out_tile[i] != c.want_tile[i]) { bad |= fail_(c, s, "out_tile", (long)i, (long long)out_tile[i], c.want_tile[i]); break; }
    for (size_t i = 0; i < out_pt.n; i++)
        if (out_pt[i] != c.want_pt[i]) { bad |= fail_(c, s, "out_per_target", (long)i, out_pt[i], c.want_pt[i]); break; }
    if (c.hit_cap >= 0) bad |= check_hits(c, s, hit_count[0], hits, order_hash);
    // the hit-level masks: per (tile, target) the levels at which the oracle's records give it a duplicate
    std::vector<uint8_t> want_mask((size_t)c.tiles * T, 0);
    for (int i = 0; i < c.hits; i++) {
        const int32_t *r = &c.want_hits[(size_t)4 * i];
        const int32_t *o = &c.off[(size_t)r[1] * (levels + 1)];
        int lev = 0;
        while (lev + 1 < levels && r[2] >= o[lev + 1]) lev++;
        want_mask[(size_t)r[0] * T + r[1]] |= (uint8_t)(1u << lev);
    }
    for (size_t i = 0; i < mask.n; i++) {
        const size_t tile = i / (size_t)A.mask_stride, word = i % (size_t)A.mask_stride;
        uint32_t want = 0;
        for (int b = 0; b < 4; b++) if ((long long)word * 4 + b < T) want |= (uint32_t)want_mask[tile * T + word * 4 + b] << (8 * b);
        if (mask[i] != want) { bad |= fail_(c, s, "mask", (long)i, mask[i], want); break; }
    }
    return bad;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: scan_lines_emu CASE_FILE...\n"); return 2; }
    emu_after_block = after_block;
    int bad = selftest_wave_sum();
    fflush(stdout);
    emu_add_hook = add_hook;
    for (int a = 1; a < argc; a++) {
        CaseFile c;
        if (!read_case(argv[a], c, 1 << 20) || c.line_pairs < 1 || c.levels > 8) { fprintf(stderr, "%s: not a case file of the line walk\n", argv[a]); return 2; }
        const bool strided = c.layout != 0;
        const int levh = c.fam ? kLev2Closed : 0, ws = c.layout == 2 ? 4 : 1;
        const Kernel kernel = pick(strided, c.B1, levh, ws);
        if (!kernel) { fprintf(stderr, "%s: no such instantiation\n", argv[a]); return 2; }
        // what wd_set_targets notes of a targets file
        const size_t row = (size_t)c.levels + 1;
        int64_t k_max = 0; bool has_empty = false;
        for (int t = 0; t < c.T; t++) {
            k_max = std::max<int64_t>(k_max, (int64_t)c.off[(size_t)t * row + c.levels] - c.off[(size_t)t * row]);
            for (int l = 0; l < c.levels; l++) has_empty = has_empty || c.off[(size_t)t * row + l + 1] <= c.off[(size_t)t * row + l];
        }
        LineTables lt;
        const bool applies = make_line_tables(c.centre.data(), c.off.data(), c.nbr.data(), c.T, c.levels, c.P, (size_t)c.line_pairs, k_max, has_empty, lt);
        int split = 0;
        if (check_tables(c, applies, lt, (size_t)c.line_pairs, split)) { bad++; fflush(stdout); continue; }
        if (!applies) { printf("case %s ok: does not apply\n", c.name.c_str()); fflush(stdout); continue; }
        char kname[64];
        if (ws == 4) snprintf(kname, sizeof(kname), "k_scan_lines<true, %d, %d, 4>", c.B1, levh);
        else snprintf(kname, sizeof(kname), "k_scan_lines<%s, %d, %d>", strided ? "true" : "false", c.B1, levh);
        Inputs in(c);
        Tables tb(lt);
        for (long &e : g_events) e = 0;
        g_neg_deltas = 0;
        g_mid_qn.clear();
        long points = 0, launches = 0;
        std::set<uint64_t> orders;
        int failed = 0, schedules = 0;
        for (int s = 0; s < kSchedules && !failed; s++) {
            uint64_t order_hash = 0;
            failed = run_schedule(c, in, tb, lt, kernel, s, (unsigned)a, points, order_hash);
            orders.insert(order_hash); launches++; schedules++;
        }
        bad += failed;
        std::string mid_qn;
        for (int v : g_mid_qn) mid_qn += (mid_qn.empty() ? "" : ",") + std::to_string(v);
        if (!failed)
            printf("case %s ok: kernel %s n %d tiles %d T %d levels %d L %d k %d line_pairs %d blocks %zu tmax %d schedules %d launches %ld points %ld "
                   "mid_drains %ld drains %ld in_place %ld finish_all %ld pushes %ld split %d neg_deltas %ld hits %d orders %zu mid_qn %s\n",
                   c.name.c_str(), kname, c.n, c.tiles, c.T, c.levels, c.L, c.k, c.line_pairs, lt.blk.size(), lt.tmax, schedules, launches,
                   points, g_events[kEv_drain_mid], g_events[kEv_drain], g_events[kEv_in_place], g_events[kEv_finish_all], g_events[kEv_push],
                   split, g_neg_deltas, c.hit_cap >= 0 ? c.hits : -1, orders.size(), mid_qn.empty() ? "-" : mid_qn.c_str());
        fflush(stdout);
    }
    return bad ? 1 : 0;
}
