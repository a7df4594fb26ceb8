// gen_rings_emu.cpp - k_gen_rings<false> and k_gen_rings<true> (csrc/gen_rings.inc) run on the CPU under shuffled
// schedules: the kernel's source is compiled as it stands, the 256 lanes of a workgroup are fibers (tools/wave_emu.h),
// LDS is the kernel's static storage and every atomic is a point at which the schedule may hand over to another lane.
// The two launches follow each other as in wd_targets_from_coords (csrc/welldup_scan.hip): the status word cleared, the
// count pass on one workgroup per centre, refusal if a ring is empty (status bit 2), the host's prefix sum over
// (centre, ring), the fill pass, refusal if a centre has more than kGenMaxMatches matches (bit 4).
// The cases are not made here: tests/test_genrings_emu.py writes each case of tests/genrings_cases.py - coordinates,
// centres, radii, the status and the CSR its plain reference expects - into a file, and this program takes the files
// as its arguments:
//   int32  'GRC1', n, T, centres given (0: every well a centre), levels, status (0, 2 or 4), P
//   int32  radii[levels + 1], x[n], y[n], centre[T]; unless status == 2: lvl_off[T * (levels + 1)], nbr[P]
// Every case runs under the eleven schedules of tools/emu_reads.h, the workgroups of a launch permuted in all but the
// first, and under each one the status, P, lvl_off and nbr must be the file's and the words behind nbr[P - 1] untouched.
// In which slot of LDS a match lands depends on the schedule, and the ranking that follows exists to undo that: so the
// order in which the lanes took their slots in the fill pass is recorded (emu_add_hook), turned into the sequence of
// record indices slot by slot - lane l holds the matches j with (j - lo) % 256 == l, in ascending order - and counted:
// `descents` is the number of slots that hold a smaller index than the slot before, summed over the ten shuffled
// schedules (`never_descents`: under the first), `orders` the number of different sequences among the eleven.
// Prints a line per case; MISMATCH and exit 1 on a difference.  With -DWAVE_EMU_TORN_ADD (an add that another fiber
// may cut in two, in the fill pass alone: two matches in one slot) it must do so at the cases with many matches:
// tests/test_genrings_emu.py builds and runs both.
// No GPU is involved; the emulation is sequentially consistent and says nothing about caches or time.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -Iinclude tools/gen_rings_emu.cpp -o gen_rings_emu
#include "wave_emu.h"
#include "emu_reads.h"
#include <set>
#include "welldup.h"
constexpr int kBlock = kEmuBlock;
constexpr int kMaxLevels = WD_MAX_LEVELS;
#include "../well_duplicates_amd/csrc/gen_rings.inc"

static GenArgs A;
static void count_pass() { k_gen_rings<false>(A); }
static void fill_pass() { k_gen_rings<true>(A); }

constexpr int kGuard = 2 * kGenMaxMatches;          // words behind nbr[P - 1] that must stay as they were
constexpr int32_t kPattern = (int32_t)0xA5A5A5A5;

struct CaseFile {
    std::string name;
    int n = 0, T = 0, given = 0, levels = 0, status = 0, P = 0;
    std::vector<int32_t> md, x, y, centre, off, nbr;
};

static bool read_case(const char *path, CaseFile &c)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    int32_t head[7];
    auto get = [&](std::vector<int32_t> &v, size_t count) { v.resize(count); return count == 0 || fread(v.data(), 4, count, f) == count; };
    bool ok = fread(head, 4, 7, f) == 7 && head[0] == 0x31435247 && head[1] > 0 && head[2] >= 0 && head[4] >= 1 && head[4] <= kMaxLevels && head[6] >= 0;
    if (ok) {
        c.n = head[1]; c.T = head[2]; c.given = head[3]; c.levels = head[4]; c.status = head[5]; c.P = head[6];
        ok = get(c.md, (size_t)c.levels + 1) && get(c.x, (size_t)c.n) && get(c.y, (size_t)c.n) && get(c.centre, (size_t)c.T);
        if (ok && c.status != 2) ok = get(c.off, (size_t)c.T * (c.levels + 1)) && get(c.nbr, (size_t)c.P);
        for (int32_t t : c.centre) ok = ok && t >= 0 && t < c.n;        // (as wd_targets_from_coords refuses them)
        ok = ok && fgetc(f) == EOF;
    }
    fclose(f);
    const std::string p(path);
    const size_t slash = p.find_last_of('/'), dot = p.find_last_of('.');
    c.name = p.substr(slash == std::string::npos ? 0 : slash + 1, dot == std::string::npos ? std::string::npos : dot - (slash == std::string::npos ? 0 : slash + 1));
    return ok;
}

// ---- the order in which the fill pass's lanes took their slots
static const CaseFile *g_case = nullptr;
static bool g_fill = false;
static std::vector<int> g_claims;                   // the lane of every add of the running workgroup, in the order of the adds
static long g_descents, g_unplaced;
static uint64_t g_order_hash;
static void add_hook(const void *, long long) { if (g_fill) g_claims.push_back(emu_lane); }
static void after_block(unsigned bx, unsigned)
{
    if (!g_fill) return;
    const CaseFile &c = *g_case;
    std::vector<int> claims; claims.swap(g_claims);
    if (c.status == 2) return;
    const int64_t centre = c.centre[bx], lo = centre > kGenWindow ? centre - kGenWindow : 0;
    const int32_t *off = &c.off[(size_t)bx * (c.levels + 1)];
    std::vector<int32_t> all(c.nbr.begin() + off[0], c.nbr.begin() + off[c.levels]);
    std::sort(all.begin(), all.end());
    std::vector<std::vector<int32_t>> of_lane(kEmuBlock);
    for (int32_t j : all) of_lane[(j - lo) % kEmuBlock].push_back(j);
    std::vector<size_t> next(kEmuBlock, 0);
    uint64_t h = 1469598103934665603ull ^ bx;
    int32_t before = -1;
    for (int lane : claims) {
        if (next[lane] == of_lane[lane].size()) { g_unplaced++; continue; }     // (a match the file does not know: nbr will differ)
        const int32_t j = of_lane[lane][next[lane]++];
        g_descents += j < before; before = j;
        h = (h ^ (uint64_t)j) * 1099511628211ull;
    }
    g_order_hash += h;                              // (a sum: the workgroups come in the schedule's order)
}

static int fail_(const CaseFile &c, int s, const char *what, long at, long got, long want)
{
    printf("MISMATCH case %s schedule %d (%s): %s %ld: %ld want %ld\n", c.name.c_str(), s, schedule_name(s), what, at, got, want);
    return 1;
}

// one schedule of one case: wd_targets_from_coords' launches.  Returns 0 if everything is the file's.
static int run_schedule(const CaseFile &c, int s, unsigned seed, Buf<int32_t> &x, Buf<int32_t> &y, Buf<int32_t> &centre, long &points)
{
    const bool permute = set_schedule(s, seed);
    const int T = c.T, levels = c.levels;
    Buf<int32_t> counts(std::max<size_t>(1, (size_t)T * levels));
    Buf<uint32_t> status(1);
    status[0] = 0;
    A = GenArgs{};
    A.x = x.p; A.y = y.p; A.centres = c.given ? centre.p : nullptr;
    A.n = c.n; A.n_centres = T; A.levels = levels;
    for (int r = 0; r <= levels; r++) A.md2[r] = c.md[r] * c.md[r];
    A.counts = counts.p; A.lvl_off = nullptr; A.nbr = nullptr; A.status = status.p;
    g_fill = false;
#ifdef WAVE_EMU_TORN_ADD
    emu_torn_add = false;                           // the count pass whole: what that build breaks is the claim of a slot
#endif
    points += run_grid((unsigned)T, 1, count_pass, permute).points;
#ifdef WAVE_EMU_TORN_ADD
    emu_torn_add = true;
#endif
    if (status[0] & 2u)
        return c.status == 2 ? 0 : fail_(c, s, "status after the count pass", 0, status[0], c.status);
    if (c.status == 2) return fail_(c, s, "status after the count pass", 0, status[0], 2);
    Buf<int32_t> off(std::max<size_t>(1, (size_t)T * (levels + 1)));
    int64_t P = 0;
    for (int t = 0; t < T; t++) {
        for (int l = 0; l < levels; l++) { off[(size_t)t * (levels + 1) + l] = (int32_t)P; P += counts[(size_t)t * levels + l]; }
        off[(size_t)t * (levels + 1) + levels] = (int32_t)P;
    }
    for (size_t i = 0; i < (size_t)T * (levels + 1); i++)
        if (off[i] != c.off[i]) return fail_(c, s, "lvl_off", (long)i, off[i], c.off[i]);
    if (P != c.P) return fail_(c, s, "P", 0, (long)P, c.P);
    Buf<int32_t> nbr((size_t)P + kGuard);
    for (size_t i = 0; i < nbr.n; i++) nbr[i] = kPattern;
    A.lvl_off = off.p; A.nbr = nbr.p;
    g_fill = true; g_claims.clear();
    points += run_grid((unsigned)T, 1, fill_pass, permute).points;
    g_fill = false;
    for (size_t i = 0; i < (size_t)kGuard; i++)
        if (nbr[(size_t)P + i] != kPattern) return fail_(c, s, "a word behind nbr", (long)i, nbr[(size_t)P + i], kPattern);
    if (status[0] & 4u)
        return c.status == 4 ? 0 : fail_(c, s, "status after the fill pass", 0, status[0], c.status);
    if (status[0] != (uint32_t)c.status) return fail_(c, s, "status after the fill pass", 0, status[0], c.status);
    for (int64_t i = 0; i < P; i++)
        if (nbr[(size_t)i] != c.nbr[(size_t)i]) return fail_(c, s, "nbr", (long)i, nbr[(size_t)i], c.nbr[(size_t)i]);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 2) { fprintf(stderr, "usage: gen_rings_emu CASE_FILE...\n"); return 2; }
    emu_add_hook = add_hook;
    emu_after_block = after_block;
    int bad = 0;
    for (int k = 1; k < argc; k++) {
        CaseFile c;
        if (!read_case(argv[k], c)) { fprintf(stderr, "%s: not a case file\n", argv[k]); return 2; }
        g_case = &c;
        Buf<int32_t> x((size_t)c.n), y((size_t)c.n), centre(std::max<size_t>(1, (size_t)c.T));
        std::copy(c.x.begin(), c.x.end(), x.p); std::copy(c.y.begin(), c.y.end(), y.p); std::copy(c.centre.begin(), c.centre.end(), centre.p);
        long points = 0, descents = 0, never_descents = 0, unplaced = 0;
        std::set<uint64_t> orders;
        int failed = 0;
        for (int s = 0; s < kSchedules && !failed; s++) {
            g_descents = g_unplaced = 0; g_order_hash = 0;
            failed = run_schedule(c, s, (unsigned)k, x, y, centre, points);
            (s ? descents : never_descents) += g_descents; unplaced += g_unplaced;
            orders.insert(g_order_hash);
        }
        bad += failed;
        if (!failed)
            printf("case %s ok: n %d T %d levels %d P %d status %d schedules %d never_descents %ld descents %ld orders %zu unplaced %ld points %ld\n",
                   c.name.c_str(), c.n, c.T, c.levels, c.P, c.status, kSchedules, never_descents, descents, orders.size(), unplaced, points);
    }
    return bad ? 1 : 0;
}
