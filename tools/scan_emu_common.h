// scan_emu_common.h - what tools/scan_queue_emu.cpp (k_scan_q) and tools/scan_lines_emu.cpp (k_scan_lines) share: a heap
// block of exactly its size, the case file and its reader, the inputs of a case as the kernels read them, and the check
// of the hit records.  Include after csrc/wd_shared.h (WD_EMU), wave_emu.h and emu_reads.h.
//
// A case file (tests/scanq_cases.py: write_case; tests/linewalk_cases.py adds the last two fields of the head and `extra`):
//   int32  'SQC1', family (0 Hamming, 1 Levenshtein <= 2), layout (0 pointer table, 1 strided planes, 2 interleaved),
//          B1, n, tiles, T, levels, L, k, tpb, perm given, out_per_target given, check_empty,
//          hit_cap (-1: no log), hits, P, status, line_pairs (0: a case of k_scan_q), words of `extra`
//   int32  centre[T], lvl_off[T * (levels + 1)], nbr[P], perm[T] if given  (the view the kernel reads)
//   uint8  per tile: filter[n], planes[L][n]
//   int64  out_tile[tiles * (1 + 5 * levels)];  uint32 out_per_target[tiles * T * levels] if given;
//   int32  hit records {tile, target, slot, dist}[hits];  int32 extra[] (the line walk's expected tables)
#pragma once
#include <set>
#include <string>

// a heap block of exactly `count` elements (nullptr if none): what lies behind it is the sanitizer's
template <class T> struct Exact {
    T *p = nullptr; size_t n = 0;
    explicit Exact(size_t count) : n(count) { if (n) { p = (T *)malloc(n * sizeof(T)); memset((void *)p, 0xA5, n * sizeof(T)); } }
    ~Exact() { free((void *)p); }
    Exact(const Exact &) = delete;
    T &operator[](size_t i) { return p[i]; }
};

struct CaseFile {
    std::string name;
    int fam = 0, layout = 0, B1 = 0, n = 0, tiles = 0, T = 0, levels = 0, L = 0, k = 0, tpb = 0, has_perm = 0, has_pt = 0,
        check_empty = 0, hit_cap = -1, hits = 0, P = 0, status = 0, line_pairs = 0;
    std::vector<int32_t> centre, off, nbr, perm, want_hits, extra;
    std::vector<uint8_t> bytes;                     // per tile: filter[n], planes[L][n]
    std::vector<int64_t> want_tile;
    std::vector<uint32_t> want_pt;
    const uint8_t *filt(int tile) const { return bytes.data() + (size_t)tile * (L + 1) * n; }
    const uint8_t *plane(int tile, int c) const { return filt(tile) + (size_t)(c + 1) * n; }
};

// max_slots: the most slots of a target the kernel's launcher takes (what wd_set_targets or the dispatch refuses is no case)
static bool read_case(const char *path, CaseFile &c, int max_slots)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    int32_t h[20];
    auto get = [&](auto &v, size_t count) { v.resize(count); return count == 0 || fread(v.data(), sizeof(v[0]), count, f) == count; };
    bool ok = fread(h, 4, 20, f) == 20 && h[0] == 0x31435153;
    if (ok) {
        c.fam = h[1]; c.layout = h[2]; c.B1 = h[3]; c.n = h[4]; c.tiles = h[5]; c.T = h[6]; c.levels = h[7]; c.L = h[8]; c.k = h[9];
        c.tpb = h[10]; c.has_perm = h[11]; c.has_pt = h[12]; c.check_empty = h[13]; c.hit_cap = h[14]; c.hits = h[15]; c.P = h[16]; c.status = h[17];
        c.line_pairs = h[18];
        ok = c.n > 0 && c.tiles > 0 && c.T > 0 && c.levels >= 1 && c.levels <= kMaxLevels && c.L >= 1 && c.tpb >= 1 && c.tpb <= kMaxTpb &&
             c.P >= 0 && c.hits >= 0 && c.hit_cap >= -1 && c.line_pairs >= 0 && h[19] >= 0;
    }
    if (ok) {
        const size_t ncnt = 1 + 5 * (size_t)c.levels;
        ok = get(c.centre, (size_t)c.T) && get(c.off, (size_t)c.T * (c.levels + 1)) && get(c.nbr, (size_t)c.P) &&
             get(c.perm, c.has_perm ? (size_t)c.T : 0) && get(c.bytes, (size_t)c.tiles * (c.L + 1) * c.n) &&
             get(c.want_tile, (size_t)c.tiles * ncnt) && get(c.want_pt, c.has_pt ? (size_t)c.tiles * c.T * c.levels : 0) &&
             get(c.want_hits, (size_t)c.hits * 4) && get(c.extra, (size_t)h[19]) && fgetc(f) == EOF;
        // what wd_set_targets refuses: a centre or a neighbour outside the tile, offsets that are no CSR, more slots than the kernel takes
        for (int32_t v : c.centre) ok = ok && v >= 0 && v < c.n;
        for (int32_t v : c.nbr) ok = ok && v >= 0 && v < c.n;
        for (int t = 0; ok && t < c.T; t++) {
            const int32_t *o = &c.off[(size_t)t * (c.levels + 1)];
            for (int l = 0; l < c.levels; l++) ok = ok && o[l] <= o[l + 1];
            ok = ok && o[0] >= 0 && o[c.levels] <= c.P && o[c.levels] - o[0] <= max_slots;
        }
    }
    fclose(f);
    const std::string p(path);
    const size_t slash = p.find_last_of('/'), dot = p.find_last_of('.');
    const size_t from = slash == std::string::npos ? 0 : slash + 1;
    c.name = p.substr(from, dot == std::string::npos ? std::string::npos : dot - from);
    return ok;
}

static int fail_(const CaseFile &c, int s, const char *what, long at, long long got, long long want)
{
    printf("MISMATCH case %s schedule %d (%s): %s %ld: %lld want %lld\n", c.name.c_str(), s, schedule_name(s), what, at, got, want);
    return 1;
}
// (every kind that differs under a schedule is printed, the first place of each: a control build shows what it broke)

// the inputs of a case on the heap, each block exact: made once, read by every schedule
struct Inputs {
    Exact<int32_t> centre, off, nbr, perm;
    std::vector<Exact<uint8_t> *> blocks;           // filters, then planes: a plane, a strided tile or an interleaved tile each
    Exact<const uint8_t *> planes, filter;
    int64_t stride = 0;
    explicit Inputs(const CaseFile &c)
        : centre((size_t)c.T), off((size_t)c.T * (c.levels + 1)),
#ifdef SCANQ_EMU_SHORT_NBR
          nbr((size_t)c.P - 1),                     // (the control build: the last entry is nobody's)
#else
          nbr((size_t)c.P),
#endif
          perm(c.has_perm ? (size_t)c.T : 0), planes(c.layout == 0 ? (size_t)c.tiles * c.L : (size_t)c.tiles), filter((size_t)c.tiles)
    {
        std::copy(c.centre.begin(), c.centre.end(), centre.p);
        std::copy(c.off.begin(), c.off.end(), off.p);
        std::copy(c.nbr.begin(), c.nbr.begin() + nbr.n, nbr.p);
        if (c.has_perm) std::copy(c.perm.begin(), c.perm.end(), perm.p);
        const size_t n = (size_t)c.n;
        auto block = [&](size_t bytes) { blocks.push_back(new Exact<uint8_t>(bytes)); return blocks.back()->p; };
        for (int i = 0; i < c.tiles; i++) {
            uint8_t *fb = block(n);
            memcpy(fb, c.filt(i), n);
            filter[(size_t)i] = fb;
            if (c.layout == 0) {                    // a pointer per cycle, an allocation per cycle
                for (int j = 0; j < c.L; j++) { uint8_t *pb = block(n); memcpy(pb, c.plane(i, j), n); planes[(size_t)i * c.L + j] = pb; }
            } else if (c.layout == 1) {             // the tile's planes back to back
                uint8_t *pb = block(n * c.L);
                for (int j = 0; j < c.L; j++) memcpy(pb + n * j, c.plane(i, j), n);
                planes[(size_t)i] = pb; stride = (int64_t)n;
            } else {                                // [group][well][4]; the cycles behind L of the last group stay 0xA5
                uint8_t *pb = block(n * 4 * (size_t)((c.L + 3) / 4));
                for (int j = 0; j < c.L; j++) for (size_t w = 0; w < n; w++) pb[(size_t)(j >> 2) * 4 * n + w * 4 + (j & 3)] = c.plane(i, j)[w];
                planes[(size_t)i] = pb; stride = (int64_t)(4 * n);
            }
        }
    }
    ~Inputs() { for (Exact<uint8_t> *b : blocks) delete b; }
};

// the hit count and the records below hit_cap: distinct records of the file's set (all of it, where the cap is not
// reached); their order is the schedule's, hashed into order_hash.  Returns 0 if they are.
static int check_hits(const CaseFile &c, int s, unsigned long long hit_count, Exact<wd_hit> &hits, uint64_t &order_hash)
{
    int bad = 0;
    if ((long long)hit_count != c.hits) bad |= fail_(c, s, "hit_count", 0, (long long)hit_count, c.hits);
    std::set<std::vector<int32_t>> want, got;
    for (int i = 0; i < c.hits; i++) want.insert(std::vector<int32_t>(c.want_hits.begin() + 4 * i, c.want_hits.begin() + 4 * i + 4));
    const long written = std::min<long>(c.hit_cap, std::min<long>(c.hits, (long)hit_count));
    uint64_t hsh = 1469598103934665603ull;
    for (long i = 0; i < written; i++) {
        const std::vector<int32_t> r{hits[(size_t)i].tile, hits[(size_t)i].target, hits[(size_t)i].slot, hits[(size_t)i].dist};
        if (!want.count(r)) { bad |= fail_(c, s, "hit record (not one of the oracle's)", i, r[2], -1); break; }
        if (!got.insert(r).second) { bad |= fail_(c, s, "hit record (written twice)", i, r[2], -1); break; }
        for (int32_t v : r) hsh = (hsh ^ (uint64_t)(uint32_t)v) * 1099511628211ull;
    }
    // (a log with room for every record holds the oracle's set, whatever the count says)
    if (c.hit_cap >= c.hits && got.size() < want.size())
        bad |= fail_(c, s, "hit record (missing)", (long)got.size(), (long long)got.size(), (long long)want.size());
    order_hash = hsh;
    return bad;
}
