// line_tables.inc - the line walk's tables (scan_lines.inc) as plain C++: no HIP, no context.  Included by
// welldup_lines.hip after scan_lines.inc (kLwTargets), whose build_line_tables downloads the targets, calls
// make_line_tables and uploads what it made; and by the CPU emulation (tools/scan_lines_emu.cpp, WD_EMU), which
// launches k_scan_lines on the very tables the library would build.
// -------------------------------------------------------------------------------------
// Every (target, slot) pair of the targets, sorted by neighbour well (stable: equal wells stay in target-then-slot
// order), cut into blocks of at most `per_block` pairs that involve at most kLwTargets targets.
// (Needs <algorithm>, <vector>, <string.h> and int4 / make_int4 of whoever includes it: wd_shared.h there, wave_emu.h here.)

struct LineTables {
    std::vector<int32_t> well;      // [P] neighbour well of every pair, ascending (LineArgs::pw)
    std::vector<uint32_t> meta;     // [P] target within the block << 16 | slot (pm)
    std::vector<int4> blk;          // {first pair, pairs, first entry of btgt, targets} per block
    std::vector<uint32_t> btgt;     // the blocks' targets: index in the file | (the first block to see it) << 31
    std::vector<int32_t> bcen;      // ... their centre wells
    std::vector<int32_t> boff;      // ... their ring offsets, levels + 1 per entry
    int tmax = 0;                   // most targets of any block, rounded up to a multiple of 4
};

// false: the walk does not apply (an empty ring, more than 4095 slots in a target, no pairs, too many of them,
// offsets that are no CSR) - `out` is then not to be used.
inline bool make_line_tables(const int32_t *cen, const int32_t *off, const int32_t *nbr, int T, int levels, int64_t P,
                             size_t per_block, int64_t k_max, bool has_empty_level, LineTables &out)
{
    if (T < 1 || levels < 1 || P < 1 || P > (1ll << 26) || has_empty_level || k_max > 4095)
        return false;
    const size_t row = (size_t)levels + 1;
    // (well, target, slot) of every pair; a target's slots are [off[t][0], off[t][levels]) of nbr
    struct Pair { int32_t well, t; uint32_t slot; };
    std::vector<Pair> pairs;
    pairs.reserve((size_t)P);
    for (int t = 0; t < T; t++) {
        const int32_t b = off[(size_t)t * row], e = off[(size_t)t * row + levels];
        if (b < 0 || e > P || e < b)
            return false;
        for (int32_t i = b; i < e; i++)
            pairs.push_back(Pair{nbr[(size_t)i], t, (uint32_t)(i - b)});
    }
    if (pairs.empty())
        return false;
    {
        // by well, stable (equal wells stay in target order): three counting passes of 11 bits - a comparison
        // sort of a few million pairs would be a tenth of a second of every run's start-up
        std::vector<Pair> tmp(pairs.size());
        int32_t lo_well = pairs[0].well;
        for (const Pair &q : pairs)
            lo_well = std::min(lo_well, q.well);
        for (int pass = 0; pass < 3; pass++) {
            std::vector<size_t> cnt(2049, 0);
            const int sh = 11 * pass;
            auto digit = [&](const Pair &q) { return (size_t)(((uint32_t)(q.well - lo_well) >> sh) & 2047u); };
            for (const Pair &q : pairs)
                cnt[digit(q) + 1]++;
            for (int d = 0; d < 2048; d++)
                cnt[(size_t)d + 1] += cnt[(size_t)d];
            for (const Pair &q : pairs)
                tmp[cnt[digit(q)]++] = q;
            pairs.swap(tmp);
        }
        // (33 bits of spread would need a fourth pass: wells are int32 and tiles hold a few million)
        if ((uint32_t)(pairs.back().well - lo_well) >> 31)
            return false;
        for (size_t i = 1; i < pairs.size(); i++)
            if (pairs[i - 1].well > pairs[i].well) {                 // (spread above 2^33 cannot happen; belt and braces)
                std::stable_sort(pairs.begin(), pairs.end(), [](const Pair &x, const Pair &y) { return x.well < y.well; });
                break;
            }
    }
    const size_t n = pairs.size();
    std::vector<int32_t> &well = out.well;
    std::vector<uint32_t> &meta = out.meta, &btgt = out.btgt;
    std::vector<int4> &blk = out.blk;
    well.assign(n, 0);
    meta.assign(n, 0u);
    btgt.clear();
    blk.clear();
    std::vector<int> local((size_t)T, -1), seen_in((size_t)T, -1);
    std::vector<char> counted((size_t)T, 0);
    size_t first = 0;
    int tmax = 0;
    while (first < n) {
        const int b = (int)blk.size();
        const size_t tgt0 = btgt.size();
        size_t i = first;
        for (; i < n && i - first < per_block; i++) {
            const int t = pairs[i].t;
            if (seen_in[(size_t)t] != b) {
                if (btgt.size() - tgt0 == (size_t)kLwTargets)
                    break;                                       // the block's target table is full
                seen_in[(size_t)t] = b;
                local[(size_t)t] = (int)(btgt.size() - tgt0);
                btgt.push_back((uint32_t)t | (counted[(size_t)t] ? 0u : 0x80000000u));   // the first block to see it owns it
                counted[(size_t)t] = 1;
            }
            well[i] = pairs[i].well;
            meta[i] = ((uint32_t)local[(size_t)t] << 16) | pairs[i].slot;
        }
        blk.push_back(make_int4((int)first, (int)(i - first), (int)tgt0, (int)(btgt.size() - tgt0)));
        tmax = std::max(tmax, (int)(btgt.size() - tgt0));
        first = i;
    }
    out.tmax = (tmax + 3) & ~3;
    // (a target without a single pair would never be counted: has_empty_level excludes it)
    out.bcen.assign(btgt.size(), 0);
    out.boff.assign(btgt.size() * row, 0);
    for (size_t i = 0; i < btgt.size(); i++) {
        const size_t t = (size_t)(btgt[i] & 0x7FFFFFFFu);
        out.bcen[i] = cen[t];
        memcpy(&out.boff[i * row], &off[t * row], row * sizeof(int32_t));
    }
    return true;
}
