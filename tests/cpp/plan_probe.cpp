// plan_probe.cpp -- prints what sf_plan.h decides, for tests/test_plan_host.py (no GPU, no library: the header alone).
//
//   plan_probe                  one line per schedule case below: a context's renders in a row, its order state
//                               carried from one to the next as launch() / sf_render_frames carry it
//   plan_probe share H B N      one line per member i of N: "i tile_rows rows" of band_share(H, B, N, i)
//
// The machine of every case: 256 CUs, 8 XCD queue groups with 4 queues each, occupancy 32 / 32 / 28 blocks per CU of
// the general, lean and pair kernels.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "sf_plan.h"

using namespace sfplan;

static const Grids kGrids = { 32u * 256u, 32u * 256u, 28u * 256u };
static const char* const kKernelNames[] = { "sf_trace_queue1",  "sf_trace_queue1c", "sf_trace_queue1s",   // (by Kernel)
                                            "sf_trace_queue1t", "sf_trace_queue1g", "sf_trace_queue2",
                                            "sf_trace_queue2c", "sf_trace_queue4",  "sf_trace_frames1" };

struct Case {
    const char* name;
    uint32_t W, H;
    uint32_t band_rows, band_count, band_index;
    const char* renders;   // one character per render: '0' a launch of its own, 'n' n frames in one launch
    void (*knobs)(Knobs&);
};

static std::string runs(const std::string* v, size_t n)   // "a*2,b*1": run lengths of equal neighbours
{
    std::string out;
    for (size_t i = 0; i < n;) {
        size_t j = i;
        while (j < n && v[j] == v[i]) ++j;
        out += (out.empty() ? "" : ",") + v[i] + "*" + std::to_string(j - i);
        i = j;
    }
    return out;
}

static void run(const Case& c)
{
    Knobs k;
    if (c.knobs) c.knobs(k);
    const BandShare sh = band_share(c.H, c.band_rows, c.band_count, c.band_index);
    OrderState o = { 0u, false, 0u };
    const size_t n = std::strlen(c.renders);
    std::string* launches = new std::string[n];
    std::string* orders = new std::string[n];
    std::string rebuilds, counts;
    uint32_t lean = 0, pair = 0;
    for (size_t r = 0; r < n; ++r) {
        const Launch l = { (c.W + 7u) / 8u, sh.tile_rows, sh.band_count, false, false, false, false, 0u,
                           (uint32_t)(c.renders[r] - '0') };
        const RenderPlan p = render_plan(l, k, kGrids, o);
        if (!p.ok) {
            launches[r] = "refused";
            orders[r] = "-";
            continue;
        }
        char buf[256];
        // order: "no" row-major, "none" the schedule's but none of these units exists yet, "read"; splits: -1 auto
        std::snprintf(buf, sizeof buf, "%s:%u%s:grid=%u:%u/%u:order=%s:costs=%d:splits=%d:flags=%#x",
                      kKernelNames[p.kernel], p.units, p.pair ? "pairs" : "tiles", p.grid, p.xcds, p.queues,
                      !p.use_order ? "no" : p.have_order ? "read" : "none", (int)p.costs,
                      p.split_buckets == SF_SPLIT_AUTO ? -1 : (int)p.split_buckets, p.flags_add);
        launches[r] = buf;
        lean += p.lean;
        pair += p.pair;
        o.phase = p.order_phase;
        if (p.rebuild) {   // (order_rebuild)
            o.n = p.units;
            o.pair = p.pair;
            rebuilds += (rebuilds.empty() ? "" : ",") + std::to_string(r + 1);
        }
        orders[r] = std::to_string(o.n) + (o.pair ? "p" : "t");
    }
    std::printf("%s | %s | rebuild=%s | orders=%s | lean=%u pair=%u\n", c.name, runs(launches, n).c_str(),
                rebuilds.empty() ? "-" : rebuilds.c_str(), runs(orders, n).c_str(), lean, pair);
    delete[] launches;
    delete[] orders;
}

static const char kFive[] = "00000";
// 66 renders: the large frames' 64-render rebuild period shows
static const char kLong[] = "000000000000000000000000000000000000000000000000000000000000000000";
static const char kLong4[] = "444444444444444444444444444444444444444444444444444444444444444444";

static const Case kCases[] = {
    // the frame sizes
    { "1920x1080", 1920, 1080, 0, 0, 0, kLong, nullptr },
    { "1280x720", 1280, 720, 0, 0, 0, kLong, nullptr },
    { "640x360", 640, 360, 0, 0, 0, "0000000", nullptr },
    { "1080p share 0/8", 1920, 1080, 8, 8, 0, kLong, nullptr },
    { "96x64", 96, 64, 0, 0, 0, kFive, nullptr },
    { "16x8 SF_ORDER=0", 16, 8, 0, 0, 0, kFive, [](Knobs& k) { k.order_mode = 0; } },
    { "1920x1080 x4", 1920, 1080, 0, 0, 0, kLong4, nullptr },
    // the knobs, at the two smallest sizes
    { "96x64 SF_PAIR=1", 96, 64, 0, 0, 0, kFive, [](Knobs& k) { k.pair = 1; } },
    { "16x8 SF_PAIR=1", 16, 8, 0, 0, 0, kFive, [](Knobs& k) { k.pair = 1; } },
    { "16x8 SF_PAIR=1 SF_ORDER=0", 16, 8, 0, 0, 0, kFive, [](Knobs& k) { k.pair = 1; k.order_mode = 0; } },
    { "96x64 SF_PAIR=0", 96, 64, 0, 0, 0, kFive, [](Knobs& k) { k.pair = 0; } },
    { "16x8 SF_PAIR=0", 16, 8, 0, 0, 0, kFive, [](Knobs& k) { k.pair = 0; } },
    { "96x64 SF_LEAN=0", 96, 64, 0, 0, 0, kFive, [](Knobs& k) { k.lean = false; } },
    { "16x8 SF_LEAN=0 SF_ORDER=0", 16, 8, 0, 0, 0, kFive, [](Knobs& k) { k.lean = false; k.order_mode = 0; } },
    { "96x64 SF_ORDER=1 SF_SPLIT_BUCKETS=0 SF_ORDER_RECORD=0", 96, 64, 0, 0, 0, kFive,
      [](Knobs& k) { k.order_mode = 1; k.split_buckets = 0; k.split_env = true; k.order_record = 0; } },
    { "16x8 SF_ORDER=1 SF_SPLIT_BUCKETS=0 SF_ORDER_RECORD=0", 16, 8, 0, 0, 0, kFive,
      [](Knobs& k) { k.order_mode = 1; k.split_buckets = 0; k.split_env = true; k.order_record = 0; } },
    { "96x64 SF_HALVES=1", 96, 64, 0, 0, 0, kFive, [](Knobs& k) { k.halves = 1; } },
    { "96x64 SF_HALVES=1 SF_ORDER=0", 96, 64, 0, 0, 0, kFive, [](Knobs& k) { k.halves = 1; k.order_mode = 0; } },
    { "16x8 SF_HALVES=1 SF_ORDER=0", 16, 8, 0, 0, 0, kFive, [](Knobs& k) { k.halves = 1; k.order_mode = 0; } },
    { "96x64 SF_MAX_BLOCKS=3", 96, 64, 0, 0, 0, kFive, [](Knobs& k) { k.max_blocks = 3; } },
    { "16x8 SF_MAX_BLOCKS=1", 16, 8, 0, 0, 0, kFive, [](Knobs& k) { k.max_blocks = 1; } },
    { "96x64 SF_TRACE_WAVES=2", 96, 64, 0, 0, 0, kFive, [](Knobs& k) { k.waves_per_block = 2; } },
    { "16x8 SF_TRACE_WAVES=2", 16, 8, 0, 0, 0, kFive, [](Knobs& k) { k.waves_per_block = 2; } },
    // an order of pair units met by a multi-frame launch, and the other way round: as many pairs as tiles (one tile
    // column), so only the kind of the order's units tells them apart
    { "8x16 SF_PAIR=1 SF_ORDER=1 SF_ORDER_EVERY=64", 8, 16, 0, 0, 0, "02200",
      [](Knobs& k) { k.pair = 1; k.order_mode = 1; k.order_every = 64; } },
    // tests/test_gpu_frames.py: the two paths alternating on one context under pair units
    { "40x16 SF_PAIR=1 SF_ORDER=1 SF_ORDER_EVERY=1", 40, 16, 0, 0, 0, "020",
      [](Knobs& k) { k.pair = 1; k.order_mode = 1; k.order_every = 1; } },
    // 2^27 tiles: 3 frames stay below 2^29 unit positions, 4 do not
    { "131072x65536 x3 x4", 131072, 65536, 0, 0, 0, "34", nullptr },
};

int main(int argc, char** argv)
{
    if (argc == 5 && std::strcmp(argv[1], "share") == 0) {
        const uint32_t H = (uint32_t)std::atol(argv[2]), B = (uint32_t)std::atol(argv[3]), N = (uint32_t)std::atol(argv[4]);
        for (uint32_t i = 0; i < (N ? N : 1u); ++i) {   // (N = 0: the default, one member)
            const BandShare s = band_share(H, B, N, i);
            std::printf("%u %u %u\n", i, s.tile_rows, s.rows);
        }
        return 0;
    }
    for (const Case& c : kCases) run(c);
    return 0;
}
