// sf_plan.h -- the render schedule, decided once: which units a persistent trace launch works through, which kernel
// takes them, on what grid and queues, and what it does to the heavy-first order. Plain integer arithmetic on a
// handful of inputs, for launch() (sf_render, sf_render_to) and sf_render_frames alike (sf_capi.hip); no HIP, no
// allocation, no environment: it runs on every frame's enqueue path. Results never depend on any of it -- only time
// does, so each rule carries the measurement it came from. (tests/test_plan_host.py works the rules by hand.)
#pragma once

#include <stdint.h>

#include "sf_internal.h"   // SF_FLAG_*, SF_SPLIT_*

namespace sfplan {

// ---- a member's band share of the frame ----
// The frame's rows are cut into bands of band_rows (a multiple of 8 wherever tiles are counted), dealt round-robin
// to band_count members. 0 for band_rows: one band of the whole frame; 0 for band_count: one member.
struct BandShare {
    uint32_t band_rows, band_count;   // with the defaults filled in
    uint32_t tiles_per_band;          // band_rows / 8
    uint32_t tile_rows;               // owned tile rows: full bands for all but possibly the frame's last band
    uint32_t rows;                    // owned pixel rows
};

inline BandShare band_share(uint32_t H, uint32_t band_rows, uint32_t band_count, uint32_t band_index)
{
    BandShare s{};
    s.band_rows = band_rows ? band_rows : ((H + 7u) / 8u) * 8u;
    s.band_count = band_count ? band_count : 1u;
    s.tiles_per_band = s.band_rows / 8u;
    const uint32_t bands = (H + s.band_rows - 1u) / s.band_rows;
    for (uint32_t b = band_index; b < bands; b += s.band_count) {
        const uint32_t y0 = b * s.band_rows, y1 = y0 + s.band_rows < H ? y0 + s.band_rows : H;
        s.rows += y1 - y0;
        s.tile_rows += (y1 + 7u) / 8u - y0 / 8u;
    }
    return s;
}

// ---- the queue split of a persistent grid ----
struct QueueSplit {
    uint32_t xcds;     // XCD queue groups in use (power of 2): a block's group is blockIdx mod xcds
    uint32_t queues;   // tile queues in use: xcds x queues per XCD
};

inline QueueSplit queue_split(uint32_t blocks, uint32_t waves_per_block, uint32_t xcd_groups, uint32_t queues_per_xcd)
{
    // every queue group needs blocks of its own: fewer groups for a grid of fewer blocks than groups
    uint32_t xcds = xcd_groups;
    while (xcds > 1u && xcds > blocks) xcds >>= 1;
    // several queues per XCD split each XCD's tickets over as many counters (less contention on each); every queue
    // needs waves of its own, so only with a full grid (>= 64 waves per queue)
    uint32_t queues = xcds;
    if (queues_per_xcd > 1u && blocks * waves_per_block >= 64u * xcds * queues_per_xcd) queues = xcds * queues_per_xcd;
    return { xcds, queues };
}

// ---- the render plan ----

// The context's schedule knobs, as sf_create reads them from the environment.
struct Knobs {
    uint32_t waves_per_block = SF_TRACE_WAVES;   // env SF_TRACE_WAVES = 1 | 2 | 4
    bool compact = false;              // env SF_COMPACT=1: the trace kernel with active-ray compaction of sparse nodes
    uint32_t xcd_groups = 8;           // XCD queue groups, one per XCD (power of 2; env SF_NQUEUES)
    uint32_t queues_per_xcd = 4;       // env SF_QUEUES_PER_XCD = 1 | 2 | 4: tile queues per XCD (full grids)
    bool lean = true;                  // env SF_LEAN=0: the general tile loop (sf_trace_queue1g) everywhere
    int pair = -1;                     // pair units (env SF_PAIR): 0 never, 1 wherever the lean loop may run,
                                       // -1 where the frame has at least as many pairs as the grid has waves
    uint32_t max_blocks = 0;           // diagnostics: env SF_MAX_BLOCKS caps the persistent grid
    // Heavy-first unit order: -1 (default) by frame size, see render_plan; env SF_ORDER=0 never, SF_ORDER=1 always
    int order_mode = -1;
    uint32_t order_every = 0;          // env SF_ORDER_EVERY = k: rebuild the order after every k-th render only
                                       // (0 = auto: 3 for small frames, 64 for frames over twice the grid, else 1)
    int order_record = -1;             // env SF_ORDER_RECORD=0|1: unit costs recorded only by the render a rebuild
                                       // reads / by every render (default: only on frames over twice the grid)
    uint32_t split_buckets = SF_SPLIT_AUTO;   // env SF_SPLIT_BUCKETS = k: top k buckets (0: never split)
    bool split_env = false;            // SF_SPLIT_BUCKETS given
    uint32_t split_parts = 4;          // env SF_SPLIT_PARTS = 2 (halves) | 4 (quarters); 640x360: 0.122 -> 0.097 ms with quarters
    bool subtree = false;              // env SF_SPLIT_PARTS=subtree: split tiles traced as 4 subtree parts (SF_FLAG_SUBTREE)
    int halves = -1;                   // env SF_HALVES: row-major units as tile halves (SF_FLAG_HALVES); -1 = by policy
};

// What one launch is and asks for.
struct Launch {
    uint32_t tiles_x, tile_rows;       // the share's tiles: per row, owned rows
    uint32_t band_count;               // members the frame is shared among (1: a whole frame)
    bool compact, packed, aux, tile_trace;   // sf_render_params' compact / packed / emit_aux; the tile trace is on
    uint32_t flags;                    // SF_FLAG_* the launch carries so far
    uint32_t frames;                   // 0: one context's own launch (sf_render, sf_render_to); n: the multi-frame
                                       // kernel with n frames on this context's queues and order (sf_render_frames)
};

// Resident blocks of a full grid (blocks per CU x CUs) of the kernel each loop would take: the general one (the kernel
// of the knobs' waves per block, or sf_trace_frames1), the lean tile loop's, the pair-unit loop's.
struct Grids {
    uint32_t general, lean, pair;
};

// The context's heavy-first order as the last rebuild left it.
struct OrderState {
    uint32_t n;       // unit count the order is a permutation of (0: none)
    bool pair;        // its units are pair units, not tiles
    uint32_t phase;   // renders since the last rebuild
};

// sf_trace_queue1 ... sf_trace_queue4: the persistent trace kernels of one frame; sf_trace_frames1: of several
enum Kernel : uint32_t { kQueue1, kQueue1c, kQueue1s, kQueue1t, kQueue1g, kQueue2, kQueue2c, kQueue4, kFrames1 };

struct RenderPlan {
    bool ok;                  // false: the launch is refused (SF_EINVAL), nothing else holds
    bool pair;                // units are pair units (counts as a pair launch, sf_pair_launches)
    uint32_t units;           // tiles or pairs of one frame: what the order and the costs are indexed by
    Kernel kernel;
    uint32_t grid;            // blocks
    uint32_t xcds, queues;
    bool use_order;           // the launch runs on the context's order state (reads an order, or builds the first)
    bool have_order;          // ... and an order of its units exists: the launch reads it
    bool rebuild;             // the order is rebuilt after the launch, from the costs it records
    bool record;              // unit costs are recorded by every render, not only by a rebuilding one
    bool costs;               // this launch records unit costs (rebuild || record)
    uint32_t split_buckets;   // effective: what the rebuild splits
    uint32_t order_waves;     // resident waves the rebuild plans for
    bool halves, subtree;
    uint32_t flags_add;       // SF_FLAG_HALVES, SF_FLAG_SUBTREE
    uint32_t px_magic;        // pair units: floor((2^32 - 1) / ceil(tiles_x / 2)), else 0
    uint32_t order_phase;     // the context's next order_phase
    bool lean;                // counts as a lean launch (sf_lean_launches): the lean tile loop or the pair loop
};

inline RenderPlan render_plan(const Launch& l, const Knobs& k, const Grids& g, const OrderState& o)
{
    RenderPlan p{};
    const uint32_t wpb = k.waves_per_block;
    // The multi-frame launch has one kernel and one loop: it never pairs, has no lean form and no halves.
    const bool batch = l.frames != 0u;
    // The lean tile loop (sf_trace_queue1t) serves a launch that asks for nothing it leaves out: whole-tile units
    // of one plain frame. What the launch itself says is known here; what the schedule adds (part units, unit
    // costs) below -- the grid is sized by the occupancy of the kernel the launch takes.
    const uint32_t lean_off = SF_FLAG_DIAG_HALF | SF_FLAG_DIAG_HALF_SEL | SF_FLAG_DIAG_UNITS |
                              SF_FLAG_DIAG_FORCE_RETRACE | SF_FLAG_PRIO_FLAT;
    const bool plain = !batch && k.lean && wpb == 1u && l.band_count == 1u && !l.compact && !l.packed && !l.aux &&
                       !l.tile_trace;
    const bool lean_ok = plain && (l.flags & lean_off) == 0u;
    uint32_t units = l.tiles_x * l.tile_rows;
    // Pair units (sf_trace_queue1: two adjacent tiles per wave, the traversal's upper levels walked once): a
    // launch the lean loop could serve -- the pair loop also serves the forced re-trace itself -- of a frame
    // with more tiles than twice the persistent grid, the pair kernel's and the single-tile lean loop's: there
    // are then at least as many pairs as waves, and the frame is one the schedule below calls `large` (1080p and
    // up; 1280x720, 14 400 tiles against 2 x 7 168 and 2 x 8 192 waves, keeps its single-tile path: with one
    // pair per wave it measured 0.028 -> 0.040 ms). Every schedule quantity below then counts pair units, and
    // the render that rebuilds the order records unit costs in the pair loop (sf_trace_queue1c): a context
    // never mixes tile and pair orders.
    const uint32_t pair_off = lean_off & ~SF_FLAG_DIAG_FORCE_RETRACE;
    const uint32_t pair_grid = g.pair > g.lean ? g.pair : g.lean;
    // (a context told to split tiles, SF_SPLIT_BUCKETS, keeps tile units by default: pair units have no parts)
    p.pair = plain && (l.flags & pair_off) == 0u && k.halves <= 0 && k.pair != 0 &&
             (k.pair > 0 || (units > 2u * pair_grid && !(k.split_env && k.split_buckets != 0u)));
    if (p.pair) {
        const uint32_t pairs_x = (l.tiles_x + 1u) / 2u;
        units = pairs_x * l.tile_rows;
        p.px_magic = 0xffffffffu / pairs_x;
    }
    p.units = units;
    uint32_t blocks = p.pair ? g.pair : lean_ok ? g.lean : g.general;
    const bool small = units <= 2u * blocks * wpb;   // units fill the full persistent grid at most twice
    // The heavy-first order (and the splits it carries) only where the frame's tiles fill at most half
    // the grid's waves: there idle slots take the split heaviest tiles and shorten the frame. With 3
    // frames in flight, frames of more tiles are throughput-bound and the order costs more than it
    // gains: 1280x720 0.039 -> 0.036 ms, a 1080p member's share over 2 / 4 GPUs 0.045 -> 0.042 /
    // 0.028 -> 0.026 ms without it, while 640x360 keeps it (0.0203 vs 0.0232 ms on a fixed view).
    // A member's share of a multi-GPU frame (band_count > 1) stays row-major too: its tiles are every N-th
    // band row of the frame, and with frames in flight the order measured slower there at every N (1080p
    // over 8 GPUs: 0.0212 vs 0.0204 ms per frame, `profiles/r3/share2/r3aw.txt`).
    const bool tiny = 2u * units <= blocks * wpb && l.band_count == 1u;
    // Round 4: whole frames of more than twice the grid's waves (1080p and up) take the order too, in a form
    // that costs the steady state nothing: rebuilt after every 16th render (64th since round 5, below) from that
    // render's unit costs alone (the renders between record nothing), heavy tiles split by the makespan model.
    // With 3 frames in flight the steady frame period is unchanged (1080p 0.0787 vs 0.0792 ms, 4K 0.373 vs 0.373),
    // but a frame whose successors are not yet queued -- the last of a timed loop, a lone frame -- no longer ends
    // on its heaviest tiles' serial traversal: one frame alone 0.175 -> 0.151-0.164 ms at 1080p, and the
    // driver's 20-step loop 0.0871 -> 0.0846 ms per frame (mean of 4 interleaved runs a side,
    // profiles/r4/order_ab.txt). Frames between half and twice the grid (1280x720) measured slower with it
    // (0.0358 -> 0.0388 ms) and keep the row-major order. End of round 4, with the faster kernel: large
    // frames take the order WITHOUT splits -- the split parts re-traverse their tile's shared upper levels,
    // and with frames in flight only the loop's last frame gains from them: the 20-step loop 0.0759-0.0782
    // -> 0.0748-0.0766 ms, one frame alone 0.133-0.136 -> 0.129-0.139, steady period unchanged (5
    // interleaved runs a side, profiles/r4/split0_ab.txt).
    const bool large = !small && l.band_count == 1u;
    p.use_order = k.order_mode > 0 || (k.order_mode < 0 && (tiny || large));
    p.split_buckets = (p.pair || (large && !k.split_env)) ? 0u : k.split_buckets;   // (pairs: no parts)
    // row-major halves (SF_FLAG_HALVES): every tile as two units of its pixel rows 0-3 / 4-7
    p.halves = !batch && !p.use_order && k.halves > 0;
    // work units: tiles, or up to `split_parts` per tile when the schedule may split tiles
    const bool parts = p.use_order && p.split_buckets != 0u;
    const uint32_t units_max = parts ? k.split_parts * units : p.halves ? 2u * units : units;
    // the grid: no more waves than units -- of all its frames, for the multi-frame launch, whose kernel finds a
    // unit's frame by a reciprocal that is exact for positions below 2^29 (FrameBatch.magic)
    if (batch && (uint64_t)l.frames * units_max >= 0x20000000ull) return p;
    const uint32_t need = batch ? l.frames * units_max : (units_max + wpb - 1u) / wpb;
    if (blocks > need) blocks = need;
    if (k.max_blocks && blocks > k.max_blocks) blocks = k.max_blocks;
    // the order is rebuilt after every order_every-th render (and whenever none exists for this launch's
    // units); the renders in between keep the last order and record their unit costs only.
    // Small frames (tiles fill the persistent grid less than twice) are latency-bound: there the stale
    // order costs the trace nothing measurable while the two order kernels are ~5 us of a ~80 us
    // frame, so by default they are rebuilt after every 3rd render (640x360 -6 %, 1280x720 -4 %);
    // full grids are throughput-bound and a stale order costs more than the kernels (1080p).
    // (large frames: every 64th since round 5 -- the rebuild's scan is one 16-wave workgroup, which waits for
    // wave slots behind the frames in flight, 64 us median and up to 1.6 ms in the bench, with its slot's next
    // frame queued behind it: the driver's 20-step loop 0.0727-0.0743 -> 0.0721-0.0722 ms in two 5-run A/Bs;
    // a one-wave scan, or the rebuild on a stream of its own, measured slower, profiles/r5/order/)
    const uint32_t every = k.order_every ? k.order_every : (small ? 3u : large ? 64u : 1u);
    // (an order of this launch's units: the multi-frame launch's are tiles, so an order of pair units that
    // sf_render_to left on the context makes it rebuild, and the other way round)
    p.have_order = o.n == units && o.pair == p.pair;
    p.rebuild = p.use_order && (!p.have_order || o.phase + 1u >= every);
    p.order_phase = !p.use_order ? o.phase : p.rebuild ? 0u : o.phase + 1u;
    // unit costs: recorded by every render, or only by the render whose costs the rebuild reads
    p.record = p.use_order && (k.order_record >= 0 ? k.order_record != 0 : !large);
    p.costs = p.use_order && (p.rebuild || p.record);
    // split tiles are traced as subtree parts
    p.subtree = !batch && p.use_order && k.subtree && p.split_buckets != 0u && wpb == 1u;
    p.flags_add = (p.halves ? SF_FLAG_HALVES : 0u) | (p.subtree ? SF_FLAG_SUBTREE : 0u);
    const uint32_t flags = l.flags | p.flags_add;
    // lean: no part units in what the launch reads (the order's splits, row-major halves) and no unit costs
    // recorded (the render a rebuild of the order reads takes the general loop)
    p.lean = p.pair || (lean_ok && !parts && !p.halves && !p.costs && !(flags & (SF_FLAG_SUBTREE | SF_FLAG_HALVES)));
    p.order_waves = blocks * wpb;   // (as sized above: the rebuild plans for the grid before the cap below)
    // a launch that qualified for the lean loop takes the general one after all: its own occupancy caps the grid
    if (lean_ok && !p.lean && g.general < g.lean && blocks > g.general) blocks = g.general;
    p.grid = blocks;
    const QueueSplit q = queue_split(blocks, wpb, k.xcd_groups, k.queues_per_xcd);
    p.xcds = q.xcds;
    p.queues = q.queues;
    p.kernel = batch ? kFrames1
             : p.pair ? (p.costs ? kQueue1c : kQueue1)
             : wpb == 1u ? ((flags & SF_FLAG_SUBTREE) ? kQueue1s : p.lean ? kQueue1t : kQueue1g)
             : wpb == 2u ? (k.compact ? kQueue2c : kQueue2) : kQueue4;
    p.ok = true;
    return p;
}

}  // namespace sfplan
