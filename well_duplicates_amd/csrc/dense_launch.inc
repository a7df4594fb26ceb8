// dense_launch.inc - the arithmetic of a dense scan's launches, free of HIP: the constants of the chain, the
// strides of its scratch, the clamp of q_per, the choice of win_bufs and npc, the LDS bytes of the compare
// stage, the grids, kpad from k_max, the group bases and the list of gather blocks.  ensure_dense_tables and
// launch_dense (welldup_dense.hip), wd_scan_async (welldup_scan.hip: the tile chunk) and the CPU emulation of
// the chain (tools/scan_dense_emu.cpp) all take them from here - the precedents are scan_q_lds_dwords
// (scan_queue.inc) and line_tables.inc - so that a buffer of exactly these sizes under the address sanitizer
// checks the figures the library itself launches with, not a copy of them.
// Needs wd_shared.h (kWave, kBlock, kWaves, kXcds, kSigCycles, kRowGroups) and <vector>, <algorithm>.
#ifndef WD_DENSE_LAUNCH_INC
#define WD_DENSE_LAUNCH_INC

constexpr int kDenseSlots = 64;       // counter slots per tile (power of two): same-line atomics serialise
constexpr int kMaxSeg = 16;           // window groups: runs of consecutive signatures staged in LDS per wave
constexpr int kWinMaxK = 128;         // ... for groups whose targets have at most this many different neighbour offsets
constexpr int kWinGap = 24;           // ... offsets this close share a run
constexpr int kWinDwords = 1024;      // ... and at most this many signatures per window (4 KB): 16 loads of 64
constexpr int kMarkBlock = 256;       // mark words per block of the rank scan (8192 wells)
constexpr int kWinBufs = 2;           // LDS windows per wave: the next tile's loads land while this tile is compared
constexpr int kWinBufsSym = 3;        // ... of the one-ended compare (half the window each): two tiles' windows in flight
constexpr int kDenseMaxChunk = 16;    // tiles a wave of the compare stage walks at most (LDS: one survivor queue per tile)
constexpr int kRankBlock = 1024;      // lanes of k_dense_rank_blocks
constexpr size_t kDenseLdsBound = 32 * 1024;   // LDS of a compare-stage workgroup at which five of them still share a CU

// LDS dwords of one wave of the compare stage (k_dense_pairs_win, k_dense_pairs): its windows, one survivor queue
// (uint2 entries) per tile of the chunk, their entry counts, and one word that keeps the next wave's windows
// 8-byte aligned when the chunk is odd.  launch_dense sizes the block by this figure; the kernels carve by the
// same sum, written out in place (scan_dense.inc says why).
inline int dense_per_wave_dwords(int win_bufs, int win_dwords, int tile_chunk, int q_per)
{
    return win_bufs * win_dwords + tile_chunk * (2 * q_per + 1) + (tile_chunk & 1);
}

// tiles a wave of the compare stage walks (wd_scan_async), and tiles per part of a dense scan: two halves of a
// small scan, else as many tiles as one compare-stage wave walks; the whole scan when the overlap is off
inline int dense_tile_chunk_of(int option, int n_tiles) { return std::max(1, std::min({option, n_tiles, kDenseMaxChunk})); }
inline int dense_part_tiles_of(bool overlap, int part_tiles_option, int n_tiles, int tile_chunk)
{
    if (!overlap || n_tiles < 2)
        return std::max(1, n_tiles);
    if (part_tiles_option > 0)
        return std::min(part_tiles_option, n_tiles);
    return n_tiles >= 2 * tile_chunk ? tile_chunk : (n_tiles + 1) / 2;
}

// ---- the tables (ensure_dense_tables) ----
// Group bases of the transposed neighbour table from host-side ring offsets (row = levels + 1): [groups + 1]
inline void dense_group_bases(const int32_t *lvl_off, int T, int levels, std::vector<long long> &gbase)
{
    const size_t row = (size_t)levels + 1;
    const int groups = (T + kWave - 1) / kWave;
    gbase.assign((size_t)groups + 1, 0);
    long long pos = 0;
    for (int g = 0; g < groups; g++) {
        int kmax = 1;                                  // at least one row so min(q, gk-1) is valid
        for (int t = g * kWave; t < std::min(T, (g + 1) * kWave); t++)
            kmax = std::max(kmax, lvl_off[(size_t)t * row + levels] - lvl_off[(size_t)t * row]);
        gbase[g] = pos;
        pos += (long long)kmax * kWave;
    }
    gbase[groups] = pos;
}
// row length of the window tables (a multiple of 32, <= kWinMaxK: the union of a group's offsets may be a little
// larger than any one target's list, and a group that straddles the end of a grid row sees two patterns), or 0:
// no window tables for these targets
inline int dense_kpad(int64_t k_max)
{
    const int64_t kpad = std::min<int64_t>(kWinMaxK, (2 * k_max + 8 + 31) & ~(int64_t)31);
    return (k_max >= 1 && k_max <= kpad) ? (int)kpad : 0;
}
// LDS dwords of one window from the largest window of any group (k_dense_windows: win_max): whole pieces of 64
inline int dense_win_dwords_of(uint32_t win_max) { return (int)((win_max + kWave - 1) / kWave * kWave); }
// The target blocks (kWaves groups each) that hold a group the window kernel leaves to the gather kernel:
// k_dense_pairs is launched over this list, not over every block of the tile (with every well a centre that is
// ONE block - the last, partial group - and the launch over all 16 834 cost 29 us per 8 tiles to find it)
inline void dense_pblocks(const int32_t *ginfo, int groups, std::vector<int32_t> &pb)
{
    pb.clear();
    for (int b = 0; b * kWaves < groups; b++) {
        bool any = false;
        for (int w = 0; w < kWaves && b * kWaves + w < groups; w++)
            any = any || ginfo[(size_t)(b * kWaves + w)] == 0;
        if (any)
            pb.push_back(b);
    }
}

// ---- a scan (launch_dense) ----
struct DenseShape {
    long long sig_stride;       // signature words per tile
    long long mask_stride;      // hit-mask words per tile (8 bits per target), a multiple of 32: cleared as uint4
    long long mw_stride;        // mark words per tile, a multiple of kMarkBlock
    int partial_stride;         // counters per slot: whole 128-byte lines
    long long n_groups, bpt;    // groups of 64 targets, blocks of kBlock targets
    int q_per;                  // survivor-queue entries per group and tile
    int win_bufs, npc;          // LDS windows per wave; pieces of 64 signatures per window if the kernel is built for that many (else 0)
    int win_dwords;             // LDS dwords of one window
    size_t cand_words;          // words of one set of the batch's flags
    unsigned mark_blocks;       // workgroups per tile of k_dense_mark (and, rounded up to the XCDs, k_dense_verify)
};

// The LDS bound behind the choice of win_bufs and npc.  It is taken once per scan, with the scan's tile chunk -
// the largest any part runs with (a part's own chunk is min(tile_chunk, its tiles)) - and with the alignment word
// counted whether that chunk is odd or not: an upper bound on dense_per_wave_dwords of every part.  Deliberately
// NOT the parts' own `+ (tc & 1)`: every part of a scan then runs the same instantiation with the same window
// count, whatever the parity of its last, shorter part, and the figure can only err towards fewer windows.
inline size_t dense_lds_bound_bytes(int win_bufs, int win_dwords, int tile_chunk, long long q_per)
{
    return (size_t)kWaves * ((size_t)win_bufs * win_dwords * 4 + 4 * ((size_t)tile_chunk * (2 * q_per + 1) + 1));
}

// table_win_dwords: dense_win_dwords_of(win_max) of the tables; windows: the window tables are in use (DenseArgs::ginfo)
inline DenseShape dense_shape(long long N, int T, int levels, int tile_chunk, long long queue_cap, bool lev2, bool sym,
                              bool windows, int table_win_dwords)
{
    DenseShape s;
    s.sig_stride = (N + 127) & ~(long long)127;
    s.partial_stride = ((1 + 5 * levels) + 15) & ~15;              // whole 128-byte lines per slot
    s.mask_stride = (((long long)T + 3) / 4 + 31) & ~31ll;
    s.mw_stride = (((N + 31) / 32) + kMarkBlock - 1) / kMarkBlock * kMarkBlock;
    s.n_groups = (T + kWave - 1) / kWave;
    s.bpt = (T + kBlock - 1) / kBlock;
    // survivors per group of 64 targets: on diverse reads almost nobody passes 10 cycles (36 x
    // P(<= 2 mismatches in 10) = 0.015 per target; ~2 per group for Levenshtein <= 2), so the
    // region holds mostly duplicate pairs; what does not fit is finished inside k_dense_pairs (or,
    // for Levenshtein, by k_dense_verify): a speed knob, not a limit
    long long q_per = queue_cap > 0 ? queue_cap : (lev2 ? 32 : 16);
    q_per = std::max<long long>(1, std::min<long long>(q_per, kWave));      // one queue entry per lane at most
    s.q_per = (int)q_per;
    // (the one-ended compare keeps the windows of three tiles in flight while LDS lets five workgroups share a CU)
    s.win_bufs = kWinBufs;
    s.win_dwords = table_win_dwords;
    s.npc = 0;
    if (sym) {
        for (s.win_bufs = kWinBufsSym; s.win_bufs > kWinBufs; s.win_bufs--)
            if (dense_lds_bound_bytes(s.win_bufs, s.win_dwords, tile_chunk, q_per) <= kDenseLdsBound)
                break;
        if (s.win_bufs == kWinBufsSym && windows)
            for (int cand : {4, 5, 6, 8})
                if (!s.npc && s.win_dwords <= cand * kWave &&
                    dense_lds_bound_bytes(s.win_bufs, cand * kWave, tile_chunk, q_per) <= kDenseLdsBound)
                    s.npc = cand;
        if (s.npc)
            s.win_dwords = s.npc * kWave;
    }
    s.cand_words = (kDenseSlots + 1 + 31) & ~(size_t)31;
    s.mark_blocks = (unsigned)((s.n_groups + kWave * kWaves - 1) / (kWave * kWaves));
    return s;
}

// one part of nt tiles
struct DensePart {
    int tc;                     // tiles a wave walks in this part
    size_t q_lds;               // LDS bytes of a compare-stage workgroup
    unsigned pairs;             // workgroups of k_dense_pairs_win (and of k_dense_pairs without a list)
    unsigned pairs_listed;      // ... of k_dense_pairs over n_pblocks listed blocks (`pairs` where there is no list)
    unsigned wells4, wells1;    // x of k_dense_sig / k_dense_pack: blocks of 4 kBlock / kBlock wells (y = nt)
    unsigned counts_x, chunks;  // k_dense_counts: x, y
    unsigned rank_words;        // k_dense_rank_words: x (y = nt); k_dense_rank_blocks: nt workgroups of kRankBlock lanes
    unsigned verify_x;          // k_dense_verify: x (y = nt); k_dense_mark: mark_blocks x nt; k_dense_reduce: nt
};
inline DensePart dense_part(const DenseShape &s, long long N, int T, int nt, int tile_chunk, int n_pblocks)
{
    DensePart p;
    p.tc = std::max(1, std::min(tile_chunk, nt));
    p.chunks = (unsigned)((nt + p.tc - 1) / p.tc);
    // LDS of a compare-stage wave: its windows, one queue per tile of the chunk, their counts
    p.q_lds = (size_t)kWaves * 4 * (size_t)dense_per_wave_dwords(s.win_bufs, s.win_dwords, p.tc, s.q_per);
    p.pairs = (unsigned)((long long)kXcds * ((s.bpt + kXcds - 1) / kXcds) * p.chunks);
    // the gather kernel: over the listed target blocks only, when the window kernel takes the rest
    p.pairs_listed = n_pblocks > 0 ? (unsigned)((long long)n_pblocks * p.chunks) : p.pairs;
    p.wells4 = (unsigned)((N + 4ll * kBlock - 1) / (4ll * kBlock));
    p.wells1 = (unsigned)((N + kBlock - 1) / kBlock);
    p.counts_x = (unsigned)((T + 4 * kBlock - 1) / (4 * kBlock));
    p.rank_words = (unsigned)(s.mw_stride / kMarkBlock);
    p.verify_x = kXcds * ((s.mark_blocks + kXcds - 1) / kXcds);
    return p;
}
// with a compare stage beside it the pack kernel gets a bounded footprint: pack_blocks workgroups in all (they
// walk their tiles with a stride), not one per kBlock * VEC wells
inline unsigned dense_pack_grid_x(unsigned full, bool parts, int pack_blocks, int nt)
{
    if (parts && pack_blocks > 0)
        return std::min(full, (unsigned)std::max(1, pack_blocks / nt));
    return full;
}

#endif
