// emu_reads.h - what tools/read_classes_emu.cpp and tools/near_emu.cpp share besides wave_emu.h: the reads they feed
// the kernels, the definitions computed directly, the eleven schedules of a case and aligned memory.
// tests/contention_inputs.py builds the same kinds of reads in numpy for the GPU (tests/test_gpu_contention.py).
#pragma once
#include <map>
#include <random>
#include <string>

// 256-byte aligned (as every array of a workspace is), filled with a pattern no kernel may depend on
template <class T> struct Buf {
    T *p = nullptr; size_t n = 0;
    explicit Buf(size_t count) : n(count) { p = (T *)aligned_alloc(256, (n * sizeof(T) + 255) / 256 * 256 + 256); memset((void *)p, 0xA5, n * sizeof(T)); }
    ~Buf() { free((void *)p); }
    Buf(const Buf &) = delete;
    void fill(int byte) { memset((void *)p, byte, n * sizeof(T)); }
    T &operator[](size_t i) { return p[i]; }
};

// ---- the reads: codes 0..3 = A C G T, 4 = N, per well of one id space (a tile, or the tiles added to a lane)
enum ReadKind { kFamilies, kChainPermuted, kChainDescending, kSlots, kEqual, kNoPf, kReadKinds };
static const char *const kReadKindName[] = {"families", "chain_permuted", "chain_descending", "slots", "equal", "no_pf"};
struct Reads {
    int L = 0;
    std::map<size_t, std::vector<uint8_t>> code;   // by id
    std::map<size_t, bool> pf;
};

static std::vector<uint8_t> random_read(std::mt19937 &rng, int L, int n_in)      // one cycle in n_in is N
{
    std::vector<uint8_t> r(L);
    for (int c = 0; c < L; c++) r[c] = n_in && rng() % n_in == 0 ? 4 : rng() % 4;
    return r;
}

// `ids`: the wells of the space, ascending.  seg0: the cycles of the first segment (kSlots: what its groups share).
static Reads make_reads(ReadKind kind, unsigned seed, const std::vector<size_t> &ids, int L, int seg0)
{
    std::mt19937 rng(seed);
    Reads R; R.L = L;
    const size_t n = ids.size();
    for (size_t g : ids) { R.code[g] = random_read(rng, L, 40); R.pf[g] = rng() % 10 != 0; }
    if (kind == kFamilies) {
        // about 12 centres, a well 0 to 3 substitutions (N among them) from its centre: hundreds of equal reads and
        // of near ones on a few roots
        std::vector<std::vector<uint8_t>> centre;
        for (int i = 0; i < 12; i++) centre.push_back(random_read(rng, L, 20));
        for (size_t g : ids) {
            std::vector<uint8_t> r = centre[rng() % centre.size()];
            for (int s = rng() % 4; s > 0; s--) r[rng() % L] = rng() % 5;
            R.code[g] = r;
        }
    } else if (kind == kChainPermuted || kind == kChainDescending) {
        // 100 reads, each one cycle from the last (and, at L >= 13, two or more from those before): every union meets
        // a fresh root.  Descending ids along the chain hook every root under the next: the deepest forest there is.
        const size_t len = std::min<size_t>(100, n);
        std::vector<size_t> at(ids);
        std::shuffle(at.begin(), at.end(), rng);
        at.resize(len);
        if (kind == kChainDescending) std::sort(at.begin(), at.end(), [](size_t a, size_t b) { return a > b; });
        std::vector<uint8_t> r = random_read(rng, L, 0);
        for (size_t i = 0; i < len; i++) {
            if (i) { const int c = (int)(i % L); r[c] = (uint8_t)((r[c] + 1 + rng() % 3) % 4); }      // (cycle i % L: no step undoes another before L steps)
            R.code[at[i]] = r; R.pf[at[i]] = true;
        }
    } else if (kind == kSlots) {
        // 32 and 33 distinct reads that share their first segment: a slot of exactly kTnLong vertices and one of one
        // more, if no other read's fingerprint falls into them (the emulator looks, and draws again if one does); about
        // half of a group's reads lie one substitution from an earlier one
        std::vector<size_t> at(ids);
        std::shuffle(at.begin(), at.end(), rng);
        size_t used = 0;
        std::vector<std::vector<uint8_t>> heads;
        for (int want : {32, 33}) {
            std::vector<std::vector<uint8_t>> grp;
            const std::vector<uint8_t> head = random_read(rng, L, 0);
            heads.push_back(std::vector<uint8_t>(head.begin(), head.begin() + seg0));
            while ((int)grp.size() < want && used < n) {
                std::vector<uint8_t> r = random_read(rng, L, 0);
                if (!grp.empty() && rng() % 2) { r = grp[rng() % grp.size()]; const int c = seg0 + (int)(rng() % (L - seg0)); r[c] = (uint8_t)((r[c] + 1 + rng() % 3) % 4); }
                std::copy(head.begin(), head.begin() + seg0, r.begin());
                if (std::find(grp.begin(), grp.end(), r) != grp.end()) continue;
                grp.push_back(r);
                R.code[at[used]] = r; R.pf[at[used]] = true; used++;
            }
        }
        for (; used < n; used++)                    // the others: another first segment
            for (const auto &h : heads)
                while (std::equal(h.begin(), h.end(), R.code[at[used]].begin())) R.code[at[used]] = random_read(rng, L, 40);
    } else if (kind == kEqual) {
        const std::vector<uint8_t> r = random_read(rng, L, 20);
        for (size_t g : ids) R.code[g] = r;
    } else if (kind == kNoPf) {
        for (size_t g : ids) R.pf[g] = false;
    }
    return R;
}

// a plane's byte of a code: N is byte 0, a base its code under a quality that is not 0
static uint8_t byte_of(uint8_t code, std::mt19937 &rng) { return code == 4 ? 0 : (uint8_t)(code | (1 + rng() % 63) << 2); }

// ---- the definitions, directly
constexpr uint32_t kNoLabel = 0xFFFFFFFFu;
struct Truth {
    std::map<size_t, uint32_t> class_label, cluster_label;      // by id: the smallest id with the same read / of the cluster; kNoLabel for a non-PF well
    std::map<size_t, uint32_t> class_members, cluster_members;  // by id: the others of its class / cluster at the smallest id, 0 elsewhere
    long classes = 0, near_pairs = 0, unions = 0;               // distinct reads; unordered pairs of them within k; clusters merged (reads - clusters)
};

static Truth truth_of(const Reads &R, int k)
{
    Truth t;
    std::map<std::vector<uint8_t>, uint32_t> rep;
    for (const auto &[g, r] : R.code) {
        t.class_label[g] = t.cluster_label[g] = kNoLabel; t.class_members[g] = t.cluster_members[g] = 0;
        if (R.pf.at(g) && !rep.count(r)) rep[r] = (uint32_t)g;          // (ids ascend: the first is the smallest)
    }
    t.classes = (long)rep.size();
    std::vector<const std::vector<uint8_t> *> reads; std::vector<uint32_t> id, root;
    for (const auto &[r, g] : rep) { reads.push_back(&r); id.push_back(g); root.push_back((uint32_t)root.size()); }
    auto find = [&](uint32_t x) { while (root[x] != x) x = root[x] = root[root[x]]; return x; };
    for (size_t i = 0; i < reads.size(); i++) for (size_t j = 0; j < i; j++) {
        int d = 0;
        for (int c = 0; c < R.L && d <= k; c++) d += (*reads[i])[c] != (*reads[j])[c];
        if (d > k) continue;
        t.near_pairs++;
        const uint32_t a = find((uint32_t)i), b = find((uint32_t)j);
        if (a != b) { root[a] = b; t.unions++; }
    }
    std::vector<uint32_t> smallest(reads.size(), kNoLabel);
    for (size_t i = 0; i < reads.size(); i++) { const uint32_t r = find((uint32_t)i); smallest[r] = std::min(smallest[r], id[i]); }
    std::map<uint32_t, uint32_t> cluster_of;       // representative -> cluster label
    for (size_t i = 0; i < reads.size(); i++) cluster_of[id[i]] = smallest[find((uint32_t)i)];
    for (const auto &[g, r] : R.code) if (R.pf.at(g)) {
        const uint32_t c = rep[r], cl = cluster_of[c];
        t.class_label[g] = c; t.cluster_label[g] = cl;
        if (c != g) t.class_members[c]++;
        if (cl != g) t.cluster_members[cl]++;
    }
    return t;
}

// ---- the schedules of a case: never, reverse, always, then eight seeds at probability 1/3; the workgroups of a
// launch in a permuted order in all but the first
constexpr int kSchedules = 11;
static const char *schedule_name(int s) { return s == 0 ? "never" : s == 1 ? "reverse" : s == 2 ? "always" : "third"; }
static bool set_schedule(int s, unsigned seed)     // returns: permute the workgroups
{
    emu_schedule(s == 2 ? kEmuAlways : s >= 3 ? kEmuThird : kEmuNever, s == 1, seed * 16 + s);
    emu_counts_clear();
    return s != 0;
}
