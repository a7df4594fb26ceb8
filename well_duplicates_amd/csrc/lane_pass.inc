// lane_pass.inc - what the passes that run after a lane's finish share: lane_index.inc's tally, lane_mismatch.inc,
// lane_distance.inc, lane_quality.inc, lane_saturation.inc and lane_top.inc.  Each reads the labels the finish left
// (and what else of the accumulator it needs) over the tiles that were added and writes the caller's scratch.
// Included once from welldup_tiledups.hip, after lane_near.inc and before lane_index.inc.  The device half needs
// kTdBlock, kWave and the collectives only, so the emulators (tools/wave_emu.h) take it alone, with
// WD_LANE_PASS_EMU; the host half uses read_classes.inc (sum_spread) and lane_dups.inc (the accumulator,
// ld_tiles_added).

namespace {

// ---- device: the walk over a run, the grouping of a wave by key ------------------------------------------
constexpr int kLaneRun = 8192;                     // consecutive wells of a tile a workgroup takes
static_assert(kLaneRun % kTdBlock == 0, "a run is whole trips of the workgroup");

// The run of a workgroup: grid (ceil(N / kLaneRun), tiles added), tile_idx = their tile indices.  Workgroup (x, y)
// takes wells x * kLaneRun .. of tile ti = tile_idx[y], whose wells have the global ids base + w; a lane takes one
// well per trip.  walk calls body(has, w, g) once per trip in every lane of the workgroup: has = this lane has a well
// (the last run of a tile ends inside a trip), w its number in the tile, g its global id - neither is to be used
// without `has`.  body contains collectives (the ballots of a pass, wave_by_key below), so every lane must reach it
// on every trip: the trips depend on the run alone, never on the lane, and a body never leaves the walk early.
struct LaneRun {
    int ti;
    size_t base;
    int64_t run0, run1;
    __device__ LaneRun(const int *__restrict__ tile_idx, int64_t N)
        : ti(tile_idx[blockIdx.y]), base((size_t)ti * (size_t)N), run0((int64_t)blockIdx.x * kLaneRun),
          run1(min(run0 + kLaneRun, N))
    {
    }
    template <class Body>
    __device__ inline void walk(Body &&body) const
    {
        for (int64_t w0 = run0; w0 < run1; w0 += kTdBlock) {
            const int64_t w = w0 + threadIdx.x;
            body(w < run1, w, base + (size_t)w);
        }
    }
};

// The active lanes of a wave grouped by key: f(key, group, first) runs once per distinct key among them, in every
// lane of the wave - group = the ballot of the lanes that hold the key, first = this lane is the lowest of them.
// Why the passes add through it: a lane of equal reads gives every lane of a wave the same key - one bin, one root,
// one rank -, and an add per lane would queue the 64 of them, and millions over the lane, on one word; here the
// group's first lane adds the group's size once.  A wave without an active lane pays one ballot.  Every lane of the
// wave must call it (it is made of collectives); the trips are the same for the whole wave, so f may itself use
// __ballot and __shfl (the group's first lane is lane __ffsll(group) - 1).
template <class F>
__device__ inline void wave_by_key(bool active, uint32_t key, F &&f)
{
    const int lane = threadIdx.x & (kWave - 1);
    unsigned long long rest = __ballot(active);
    while (rest) {
        const int leader = __ffsll((long long)rest) - 1;
        const uint32_t k0 = (uint32_t)__shfl((int)key, leader);
        const unsigned long long group = __ballot(active && key == k0);
        f(k0, group, lane == leader);
        rest &= ~group;
    }
}

}  // namespace

#ifndef WD_LANE_PASS_EMU                           // (tools/wave_emu.h: the device half on the CPU)
#include "welldup_lanedistance.h"                  // the limits of a radius and of a coordinate

namespace {

// ---- host: the start of a pass -------------------------------------------------------------------------
// The steps every pass after a finish begins with.  A pass calls them in this order with its own checks and the
// zeroing of its results between them, where they have always been - a call wrong in two ways fails on the same one -,
// and hands over its phrases whole: their wording differs from pass to pass and nothing here composes them.
struct LanePass {
    wd_lane_dups *ld;
    std::vector<int> tiles;                        // the tile indices that were added
    dim3 grid;                                     // LaneRun's
    int rc = WD_OK;                                // what the pass returns when start() says false
    explicit LanePass(wd_lane_dups *l) : ld(l) {}
    int finished(const char *say) const { return ld->finished ? WD_OK : fail(ld->ctx, WD_ERR_ARG, say); }
    // `need` bytes of device memory; small names the pass's size function
    int scratch(const void *dev, size_t bytes, size_t need, const char *small, const char *host) const
    {
        if (!dev || bytes < need)
            return fail(ld->ctx, WD_ERR_ARG, small);
        return on_device(dev) ? WD_OK : fail(ld->ctx, WD_ERR_ARG, host);
    }
    // The tiles, and with any the device bound and the grid.  false: nothing to launch, the pass returns rc - WD_OK
    // for a lane without wells or tiles, whose results stay zero, or the error.
    bool start()
    {
        if (ld->N > 0)
            tiles = ld_tiles_added(ld);
        if (tiles.empty())
            return false;
        grid = dim3((unsigned)((ld->N + kLaneRun - 1) / kLaneRun), (unsigned)tiles.size());
        rc = bind_device(ld->ctx) ? WD_ERR_HIP : WD_OK;
        return rc == WD_OK;
    }
    // the tile indices into the scratch: queued after the pass has cleared it, their place included
    int upload(int *d_tidx) const
    {
        wd_ctx *ctx = ld->ctx;
        WD_HIP(ctx, hipMemcpyAsync(d_tidx, tiles.data(), tiles.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        return WD_OK;
    }
};

// ---- host: a radius and the coordinates of a tile's wells (distances, saturation) -------------------------
// what = "lane distances" or "lane saturation", the head of the message
int lane_pass_radius(wd_ctx *ctx, const char *what, int64_t radius)
{
    if (radius < 0 || radius > WD_LANEDISTANCE_MAX_RADIUS)
        return fail(ctx, WD_ERR_ARG, std::string(what) + ": the radius is 0.." + std::to_string(WD_LANEDISTANCE_MAX_RADIUS) +
                                         ", not " + std::to_string(radius));
    return WD_OK;
}

// x and y of the N wells, each 0 .. WD_LANEDISTANCE_MAX_COORD, side by side as the kernels load them
int lane_pass_coords(wd_ctx *ctx, const char *what, const int32_t *x, const int32_t *y, int64_t N, std::vector<int2> &h_xy)
{
    h_xy.resize((size_t)N);
    for (int64_t w = 0; w < N; w++) {
        if (((uint32_t)x[w] | (uint32_t)y[w]) > (uint32_t)WD_LANEDISTANCE_MAX_COORD)
            return fail(ctx, WD_ERR_ARG, std::string(what) + ": well " + std::to_string(w) + " lies at (" +
                                             std::to_string(x[w]) + ", " + std::to_string(y[w]) + "), outside 0.." +
                                             std::to_string(WD_LANEDISTANCE_MAX_COORD));
        h_xy[(size_t)w] = make_int2(x[w], y[w]);
    }
    return WD_OK;
}

// ---- host: the spread counters on their way back --------------------------------------------------------
// [rows][kSpread][width] copies of counters in device memory (spread_row).  spread_fetch queues the download of
// every one it is given behind whatever else the pass has queued, synchronises the stream - the one time a pass (or a
// histogram pass of lane top) does - and sum() then adds up a row's copies.
struct SpreadFetch {
    const void *dev;
    size_t rows;
    int width;
    std::vector<unsigned long long> h;
    SpreadFetch(const void *d, size_t r, int w) : dev(d), rows(r), width(w) {}
    void sum(size_t row, unsigned long long *out) const { sum_spread(h.data(), row, width, out); }
};

int spread_fetch(wd_ctx *ctx, std::initializer_list<SpreadFetch *> fetches)
{
    for (SpreadFetch *f : fetches) {
        f->h.resize(f->rows * kSpread * (size_t)f->width);
        WD_HIP(ctx, hipMemcpyAsync(f->h.data(), f->dev, f->h.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    WD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return WD_OK;
}

// The rows of mismatches, distances and qualities: a tile's counters are its row and add up to the first columns of
// the lane's; with `lane`, the first n_lane of its counters follow them in the lane's row.
void lane_pass_rows(const SpreadFetch &tile, int T, int64_t *tile_rows, int64_t *lane_row, const SpreadFetch *lane = nullptr,
                    int n_lane = 0)
{
    std::vector<unsigned long long> c((size_t)std::max(tile.width, lane ? lane->width : 0));
    for (int t = 0; t < T; t++) {
        tile.sum((size_t)t, c.data());
        for (int f = 0; f < tile.width; f++) {
            tile_rows[(size_t)t * tile.width + f] = (int64_t)c[f];
            lane_row[f] += (int64_t)c[f];
        }
    }
    if (lane) {
        lane->sum(0, c.data());
        for (int b = 0; b < n_lane; b++)
            lane_row[tile.width + b] = (int64_t)c[b];
    }
}

}  // namespace
#endif
