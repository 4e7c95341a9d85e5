// sf_capi.hip -- host side of the C ABI declared in include/sphereflake/sf.h.
//
// Owns the per-device context: device G-buffer (positions, normals as float4, reference layout
// Sphereflake.h:7-11), optional aux channels (minT, hit index), the read-only constants block
// (child frames, per-depth tables, rsqrtps table), stats words and the overflow tile list.
// Launches are stream-ordered; nothing here synchronises except sf_download / sf_get_stats /
// sf_synchronize.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "sf_build_id.h"   // SF_SOURCE_HASH (generated: build/, scripts/source_hash.py)
#include "sf_internal.h"
#include "sf_plan.h"       // the render schedule: band shares, the queue split, the render plan
#include "sphereflake/sf.h"

extern "C" __global__ void sf_trace_wave1(FrameArgs a, uint32_t* overflow_list, uint32_t* overflow_count);
extern "C" __global__ void sf_trace_wave2(FrameArgs a, uint32_t* overflow_list, uint32_t* overflow_count);
extern "C" __global__ void sf_trace_wave4(FrameArgs a, uint32_t* overflow_list, uint32_t* overflow_count);
extern "C" __global__ void sf_trace_queue1(FrameArgs a);
extern "C" __global__ void sf_trace_queue1c(FrameArgs a);
extern "C" __global__ void sf_trace_queue1t(FrameArgs a);
extern "C" __global__ void sf_trace_frames1(FrameBatch b);
extern "C" __global__ void sf_trace_queue1g(FrameArgs a);
extern "C" __global__ void sf_trace_queue1s(FrameArgs a);
extern "C" __global__ void sf_trace_queue2(FrameArgs a);
extern "C" __global__ void sf_trace_queue4(FrameArgs a);
extern "C" __global__ void sf_trace_queue2c(FrameArgs a);
extern "C" __global__ void sf_order_scan(uint32_t* chunk_cnt, uint32_t nc, uint32_t n_tiles,
                                         uint32_t split_buckets, uint32_t parts, uint32_t spare, uint32_t waves,
                                         uint32_t prio_buckets,
                                         uint32_t* chunk_off, uint32_t* order_meta, const uint32_t* fuse_cost,
                                         uint32_t* fuse_order, uint32_t split_cap);
extern "C" __global__ void sf_order_bucket_scan(const uint32_t* chunk_cnt, uint32_t nc, uint32_t* chunk_rel, uint32_t* tot);
extern "C" __global__ void sf_order_scatter_plan(const uint32_t* cost, uint32_t n, uint32_t* chunk_cnt,
                                                 const uint32_t* chunk_rel, const uint32_t* tot, uint32_t split_buckets,
                                                 uint32_t parts, uint32_t spare, uint32_t waves, uint32_t prio_buckets,
                                                 uint32_t split_cap, uint32_t* order_meta, uint32_t* order);
extern "C" __global__ void sf_order_scatter(const uint32_t* cost, uint32_t n, uint32_t* chunk_cnt,
                                            const uint32_t* chunk_off, const uint32_t* order_meta, uint32_t* order,
                                            uint32_t* rank_out);
extern "C" __global__ void sf_fixup_wave(FrameArgs a, const uint32_t* overflow_list, uint32_t* counters,
                                         uint32_t parity);
extern "C" __global__ void sf_trace_ray(FrameArgs a);
extern "C" __global__ void sf_trace_dirs_wave(FrameArgs a, const float* dirs, uint32_t stride, uint32_t groups,
                                              uint32_t* overflow_list, uint32_t* overflow_count);
extern "C" __global__ void sf_trace_dirs_fixup(FrameArgs a, const float* dirs, uint32_t stride,
                                               const uint32_t* overflow_list, uint32_t* counters, uint32_t parity);
extern "C" __global__ void sf_trace_rays_wave(FrameArgs a, const float* origins, const float* dirs, uint32_t ostride,
                                              uint32_t dstride, uint32_t rpo, uint32_t mixed_ok, uint32_t groups,
                                              uint32_t* overflow_list, uint32_t* overflow_count);
extern "C" __global__ void sf_trace_rays_one(FrameArgs a, const float* origins, const float* dirs, uint32_t ostride,
                                             uint32_t dstride, uint32_t rpo, uint32_t groups, uint32_t* overflow_list,
                                             uint32_t* overflow_count);
extern "C" __global__ void sf_trace_rays_fixup(FrameArgs a, const float* origins, const float* dirs, uint32_t ostride,
                                               uint32_t dstride, uint32_t rpo, const uint32_t* overflow_list,
                                               uint32_t* counters, uint32_t parity);
extern "C" __global__ void sf_trace_shadow_wave(FrameArgs a, const float* pos4, ShadowArgs sa, uint8_t* vis,
                                                uint32_t groups, uint32_t* overflow_list, uint32_t* overflow_count);
extern "C" __global__ void sf_trace_shadow_fixup(FrameArgs a, const float* pos4, ShadowArgs sa, uint8_t* vis,
                                                 const uint32_t* overflow_list, uint32_t* counters, uint32_t parity);
extern "C" __global__ void sf_light_image_px(uint32_t W, uint32_t H, const float* pos4, const float* nrm4,
                                          const uint8_t* vis, ShadowArgs sa, float ambient, uint8_t* rgba);
extern "C" __global__ void sf_trace_shadows_wave(FrameArgs a, const float* pos4, ShadowLights sl, uint64_t* mask,
                                                 uint32_t groups, uint32_t* overflow_list, uint32_t* overflow_count);
extern "C" __global__ void sf_trace_shadows_fixup(FrameArgs a, const float* pos4, ShadowLights sl, uint64_t* mask,
                                                  const uint32_t* overflow_list, uint32_t* counters, uint32_t parity);
extern "C" __global__ void sf_light_image_many_px(uint32_t W, uint32_t H, const float* pos4, const float* nrm4,
                                                  const uint64_t* mask, ShadowLights sl, float ambient, uint8_t* rgba);
extern "C" __global__ void sf_trace_sun_wave(FrameArgs a, const float* pos4, SunArgs sa, uint8_t* vis, uint32_t groups,
                                             uint32_t* overflow_list, uint32_t* overflow_count);
extern "C" __global__ void sf_trace_sun_fixup(FrameArgs a, const float* pos4, SunArgs sa, uint8_t* vis,
                                              const uint32_t* overflow_list, uint32_t* counters, uint32_t parity);
extern "C" __global__ void sf_light_image_sun_px(uint32_t W, uint32_t H, const float* pos4, const float* nrm4,
                                                 const uint8_t* vis, float sx, float sy, float sz, float ambient,
                                                 uint8_t* rgba);
extern "C" __global__ void sf_trace_suns_wave(FrameArgs a, const float* pos4, SunDirs sd, uint64_t* mask,
                                              uint32_t groups, uint32_t* overflow_list, uint32_t* overflow_count);
extern "C" __global__ void sf_trace_suns_fixup(FrameArgs a, const float* pos4, SunDirs sd, uint64_t* mask,
                                               const uint32_t* overflow_list, uint32_t* counters, uint32_t parity);
extern "C" __global__ void sf_light_image_suns_px(uint32_t W, uint32_t H, const float* pos4, const float* nrm4,
                                                  const uint64_t* mask, SunDirs sd, float ambient, uint8_t* rgba);
extern "C" __global__ void sf_trace_shafts_wave(FrameArgs a, const float* pos4, ShaftArgs sh, uint64_t* mask,
                                                uint32_t groups, uint32_t* overflow_list, uint32_t* overflow_count);
extern "C" __global__ void sf_trace_shafts_fixup(FrameArgs a, const float* pos4, ShaftArgs sh, uint64_t* mask,
                                                 const uint32_t* overflow_list, uint32_t* counters, uint32_t parity);
extern "C" __global__ void sf_light_image_shafts_px(uint32_t W, uint32_t H, const float* pos4, const uint64_t* mask,
                                                    ShaftArgs sh, float gain, float cr, float cg, float cb,
                                                    uint8_t* rgba);
extern "C" __global__ void sf_trace_suns_sum_wave(FrameArgs a, const float* pos4, const float* nrm4, SunSum ss,
                                                  float* out, uint32_t groups, uint32_t* overflow_list,
                                                  uint32_t* overflow_count);
extern "C" __global__ void sf_trace_suns_sum_fixup(FrameArgs a, const float* pos4, const float* nrm4, SunSum ss,
                                                   float* out, const uint32_t* overflow_list, uint32_t* counters,
                                                   uint32_t parity);
extern "C" __global__ void sf_trace_shadows_sum_wave(FrameArgs a, const float* pos4, const float* nrm4, ShadowSum ss,
                                                     float* out, uint32_t groups, uint32_t* overflow_list,
                                                     uint32_t* overflow_count);
extern "C" __global__ void sf_trace_shadows_sum_fixup(FrameArgs a, const float* pos4, const float* nrm4, ShadowSum ss,
                                                      float* out, const uint32_t* overflow_list, uint32_t* counters,
                                                      uint32_t parity);
extern "C" __global__ void sf_trace_ao_wave(FrameArgs a, const float* pos4, const float* nrm4, AoArgs ao, uint64_t* mask,
                                            uint32_t groups, uint32_t* overflow_list, uint32_t* overflow_count);
extern "C" __global__ void sf_trace_ao_fixup(FrameArgs a, const float* pos4, const float* nrm4, AoArgs ao,
                                             uint64_t* mask, const uint32_t* overflow_list, uint32_t* counters,
                                             uint32_t parity);
extern "C" __global__ void sf_trace_ao_sum_wave(FrameArgs a, const float* pos4, const float* nrm4, AoSum ao, float* out,
                                                uint32_t groups, uint32_t* overflow_list, uint32_t* overflow_count);
extern "C" __global__ void sf_trace_ao_sum_fixup(FrameArgs a, const float* pos4, const float* nrm4, AoSum ao,
                                                 float* out, const uint32_t* overflow_list, uint32_t* counters,
                                                 uint32_t parity);
extern "C" __global__ void sf_trace_ao_spin_wave(FrameArgs a, const float* pos4, const float* nrm4, AoArgs ao, AoSpin sp,
                                                 uint64_t* mask, uint32_t groups, uint32_t* overflow_list,
                                                 uint32_t* overflow_count);
extern "C" __global__ void sf_trace_ao_spin_fixup(FrameArgs a, const float* pos4, const float* nrm4, AoArgs ao,
                                                  AoSpin sp, uint64_t* mask, const uint32_t* overflow_list,
                                                  uint32_t* counters, uint32_t parity);
extern "C" __global__ void sf_trace_ao_spin_sum_wave(FrameArgs a, const float* pos4, const float* nrm4, AoSum ao,
                                                     AoSpin sp, float* out, uint32_t groups, uint32_t* overflow_list,
                                                     uint32_t* overflow_count);
extern "C" __global__ void sf_trace_ao_spin_sum_fixup(FrameArgs a, const float* pos4, const float* nrm4, AoSum ao,
                                                      AoSpin sp, float* out, const uint32_t* overflow_list,
                                                      uint32_t* counters, uint32_t parity);
extern "C" __global__ void sf_trace_mirror_wave(FrameArgs a, const float* pos4, const float* nrm4, MirrorArgs mr,
                                                AoSpin sp, uint64_t* mask, uint32_t groups, uint32_t* overflow_list,
                                                uint32_t* overflow_count);
extern "C" __global__ void sf_trace_mirror_fixup(FrameArgs a, const float* pos4, const float* nrm4, MirrorArgs mr,
                                                 AoSpin sp, uint64_t* mask, const uint32_t* overflow_list,
                                                 uint32_t* counters, uint32_t parity);
extern "C" __global__ void sf_trace_mirror_sum_wave(FrameArgs a, const float* pos4, const float* nrm4, MirrorSum mr,
                                                    AoSpin sp, float* out, uint32_t groups, uint32_t* overflow_list,
                                                    uint32_t* overflow_count);
extern "C" __global__ void sf_trace_mirror_sum_fixup(FrameArgs a, const float* pos4, const float* nrm4, MirrorSum mr,
                                                     AoSpin sp, float* out, const uint32_t* overflow_list,
                                                     uint32_t* counters, uint32_t parity);
extern "C" __global__ void sf_light_filter_px(uint32_t W, uint32_t H, const float* pos4, const float* nrm4,
                                              const float* in, float* out, uint32_t R, float normal_min, float k2);
extern "C" __global__ void sf_light_accumulate_px(uint32_t W, uint32_t H, const float* pos4, const float* nrm4,
                                                  const float* in, const float* hpos4, const float* hnrm4,
                                                  const float* hist, float* out, LightAccum a);
extern "C" __global__ void sf_light_fill_px(uint32_t n, float r, float g, float b, float* buf);
extern "C" __global__ void sf_light_image_buffer_px(uint32_t W, uint32_t H, const float* pos4, const float* buf,
                                                    uint8_t* rgba);
extern "C" __global__ void sf_band_unpack(FrameArgs a, const float4* stage, uint32_t stage_rows, uint32_t band_rows,
                                           uint32_t n, uint32_t first, uint32_t members, uint32_t row0);
extern "C" __global__ void sf_node_table(FrameArgs a, float4* table, uint32_t nodes);
extern "C" __global__ void sf_slab_unpack4(FrameArgs a, const uint32_t* stage, const float4* table, uint32_t table_depth,
                                           uint32_t stage_rows, uint32_t band_rows, uint32_t n, uint32_t first,
                                           uint32_t members);
extern "C" __global__ void sf_post_ssao(PostArgs a);
extern "C" __global__ void sf_post_blur(PostArgs a, uint32_t dir);
extern "C" __global__ void sf_post_final(PostArgs a);
extern "C" __global__ void sf_post_fused(PostArgs a);
extern "C" __global__ void sf_mt_draws(uint32_t* state, uint32_t* out, uint32_t n);
extern "C" __global__ void sf_mt_raw(const uint32_t* state, uint32_t* raw, uint32_t blocks);
extern "C" __global__ void sf_mt_jump_partial(const uint32_t* raw, const uint64_t* polys, uint32_t poly_words,
                                              uint32_t* partial);
extern "C" __global__ void sf_mt_segments(const uint32_t* state, const uint32_t* partial, uint32_t L, uint32_t n,
                                          uint32_t* out, uint32_t* state_out);
extern "C" __global__ void sf_progressive_trace(FrameArgs a, const uint32_t* draws, uint64_t counter0, uint32_t packets,
                                                uint64_t ticket0, PacketLane* lanes, unsigned long long* owner,
                                                const uint32_t* perm, uint32_t levels, uint32_t* ovf_list,
                                                uint32_t* ovf_cnt);
extern "C" __global__ void sf_progressive_fixup(FrameArgs a, const uint32_t* draws, uint64_t counter0, uint32_t packets,
                                                uint64_t ticket0, PacketLane* lanes, unsigned long long* owner,
                                                const uint32_t* perm, const uint32_t* ovf_list, uint32_t* counters,
                                                uint32_t parity);
extern "C" __global__ void sf_progressive_fixup_sse(FrameArgs a, const uint32_t* draws, uint64_t counter0,
                                                    uint32_t packets, uint64_t ticket0, PacketLane* lanes,
                                                    unsigned long long* owner, const uint32_t* perm,
                                                    const uint32_t* ovf_list, uint32_t* counters, uint32_t parity);
extern "C" __global__ void sf_packet_bin(FrameArgs a, const uint32_t* draws, uint64_t counter0, uint32_t packets,
                                         uint32_t pw, uint32_t bin_shift, uint32_t bins_x, uint32_t* bin_cnt);
extern "C" __global__ void sf_packet_scan(uint32_t* bin_cnt, uint32_t nbins, const uint32_t* rank);
extern "C" __global__ void sf_bin_hist(const uint32_t* bin_cost, uint32_t nbins, uint32_t* chunk_cnt);
extern "C" __global__ void sf_packet_place(FrameArgs a, const uint32_t* draws, uint64_t counter0, uint32_t packets,
                                           uint32_t pw, uint32_t bin_shift, uint32_t bins_x, uint32_t* bin_cur,
                                           uint32_t* perm);
extern "C" __global__ void sf_progressive_trace_sse(FrameArgs a, const uint32_t* draws, uint64_t counter0,
                                                    uint32_t packets, uint64_t ticket0, PacketLane* lanes,
                                                    unsigned long long* owner, const uint32_t* perm, uint32_t levels,
                                                    uint32_t* ovf_list, uint32_t* ovf_cnt);
extern "C" __global__ void sf_progressive_scatter(FrameArgs a, uint32_t packets, uint64_t ticket0,
                                                  const PacketLane* lanes, const unsigned long long* owner);

static const uint32_t kLut[2048] = {
#include "rsqrtps_lut.inc"
};

namespace {

constexpr uint32_t kRaysFixupBlocks = 1024;   // grid of sf_trace_rays_fixup (grid-stride over the re-trace list)
constexpr uint32_t kDefaultLevels = 12;   // depths 0..11 expand; every BASELINE camera stays <= 10
// sf_shadow_defaults' relative bias: the smallest power of two at which no pixel that faces the light by more than
// 30 degrees is shadowed by its own sphere (scripts/experiments/shadow_bias.py)
constexpr float kShadowBias = 0x1p-10f;
// parallel mt19937 draws (sf_mtjump.cpp, sf_kernels.hip): from this many draws per call, in K <= kMtSegMax
// segments of >= kMtSegMin draws, each jumped to by a convolution split over SF_MT_PARTS workgroups
constexpr uint32_t kMtParMin = 32768, kMtSegMin = 8192, kMtSegMax = 32;
constexpr uint32_t kMtParts = SF_MT_PARTS, kMtRawBlocks = 33;   // raw words x_0..x_20559 (19937 + 623 + 1)

struct DevGuard {
    int prev = -1;
    explicit DevGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DevGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// A context's stream gets a hardware queue of its own (round 6): it is made with a CU mask of every CU, which the
// HIP runtime serves with a queue of that stream's own, not one of the GPU_MAX_HW_QUEUES queues it shares out and
// hands on from destroyed streams. Measured (profiles/r6/multi/queue_reuse/): with shared queues, a dist
// of 8 slots made after a dist of 3 or 4 had run its loops and been destroyed (the bench's legs; any process that
// renders a whole frame before a 1/8 band share) traced the share at 0.0132-0.0141 ms per frame instead of
// 0.0110-0.0113 -- every time, at the same clock, with the same buffers; not after one that made and rendered plain
// contexts, nor after a dist of 8 or 16 slots. Queues of their own: 0.0110-0.0112 in every such sequence.
// (The mask covers every CU: no CU is withheld. Such a stream is not a non-blocking one: work on the legacy default
// stream is ordered with it; the library enqueues nothing there.) SF_STREAM_CUMASK=0: a plain non-blocking stream.
bool stream_cumask_on()
{
    static const bool on = [] {
        const char* ev = std::getenv("SF_STREAM_CUMASK");
        return !ev || std::atoi(ev) != 0;
    }();
    return on;
}
// (the caller has made `device` current)
hipError_t stream_acquire(int device, hipStream_t* out)
{
    if (!stream_cumask_on()) return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
    int cus = 0;
    hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e != hipSuccess) return e;
    std::vector<uint32_t> mask((size_t)(cus + 31) / 32, 0xffffffffu);
    if (cus % 32) mask.back() = (1u << (cus % 32)) - 1u;
    if (hipExtStreamCreateWithCUMask(out, (uint32_t)mask.size(), mask.data()) == hipSuccess) return hipSuccess;
    (void)hipGetLastError();   // (a runtime without CU-masked queues: a plain stream, as with SF_STREAM_CUMASK=0)
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}

}  // namespace

struct sf_ctx {
    uint32_t fast_div = 0;             // ray generation's u = x / W by reciprocal + fma correction (host-verified)
    int device = 0;
    uint32_t W = 0, H = 0;
    hipStream_t stream = nullptr;
    float* pos = nullptr;
    float* nrm = nullptr;
    float* min_t = nullptr;
    uint32_t* hit_index = nullptr;
    int32_t* stats = nullptr;          // [0] max depth, [1] closest key, [2] unrecoverable overflow
    uint32_t* ovf_counters = nullptr;  // [0,1] overflow counts, then the tile queues (SF_QUEUE_WORD); alternating per render
    uint32_t* ovf_list = nullptr;      // 4 x tiles_x * tiles_y entries (one per work unit)
    float4* node_table = nullptr;      // index slab unpack: frames of the nodes of depth <= SF_NODE_TABLE_DEPTH
    float table_root[12];              // the root transform the table was built for
    uint32_t table_gen = 0;            // ... and consts_gen (0: no table yet)
    uint32_t consts_gen = 1;           // bumped by every constant-block upload (children, depth tables)
    struct SlabCacheEntry {            // sf_slab_bytes of recent views (gen 0: empty)
        float root[16];
        uint32_t gen = 0, bytes = 0;
    } slab_cache[64];
    uint32_t slab_cache_next = 0;
    DeviceConsts* consts = nullptr;
    DeviceConsts host_consts;
    // the shadow traces' block (sf_set_shadow_lod): the same but for the depth tables' LOD constant
    DeviceConsts* shadow_consts = nullptr;
    DeviceConsts host_shadow_consts;
    float shadow_lod = 0.0f;           // 0: the variant's own constant
    float child[9][16];
    float root[16];
    float o[3], tl[3], tr[3], bl[3];
    bool has_view = false;
    uint32_t parity = 0;
    int64_t rays = 0;
    int last_hip = 0;
    int fixup_blocks = 256;
    sfplan::Knobs knobs;                         // the schedule's tuning knobs (sf_plan.h), read from the environment
    uint32_t levels_override = 0;                // tuning knob: env SF_LEVELS (LDS levels, 0 = adaptive)
    bool slab_shallow = false;                   // tests only: index slabs as SF_PACKED_INDEX_DIAG (env SF_DIAG_SLAB_SHALLOW)
    int frames_heavy = -1;                       // A/B: sf_render_frames' interleaved head units per frame (env
                                                 // SF_FRAMES_HEAVY; -1: the grid's waves / frames)
    bool frames_one = false;                     // A/B: sf_render_frames takes its kernel for one frame too (env SF_FRAMES_ONE)
    bool persistent = true;                      // tuning knob: env SF_PERSISTENT=0 -> one workgroup per tile group
    uint32_t flags = 0;                          // SF_FLAG_* A/B switches: env SF_FLAGS
    int cus = 256;
    uint32_t prio_buckets = 8;                   // top cost buckets (3 octaves) traced at raised wave priority (env SF_PRIO_BUCKETS)
    int occ_key = -1, occ_blocks = 0;            // cached occupancy (waves per block, levels) -> blocks per CU
    int occ_blocks_lean = 0;                     // the same of sf_trace_queue1t, the lean tile loop (1 wave per block)
    int occ_blocks_pair = 0;                     // the same of sf_trace_queue1 / 1c, the pair-unit loop
    uint32_t pair_launches = 0;                  // trace launches that took the pair-unit loop (sf_pair_launches)
    uint32_t lean_launches = 0;                  // trace launches that took the lean tile loop or the pair loop (sf_lean_launches)
    int variant = SF_VARIANT_AVX;                // reference path reproduced (sf_set_variant)
    // frame-less progressive mode
    uint32_t* mt_state = nullptr;      // 624 words + next index (std::mt19937 layout)
    uint32_t* draws = nullptr;         // 2 per packet
    PacketLane* lanes = nullptr;       // 8 per packet
    uint32_t prog_cap = 0;             // packets the scratch buffers hold
    uint32_t* perm = nullptr;          // binned trace order of a batch (prog_cap)
    uint32_t* bin_cnt = nullptr;       // SF_PROG_MAX_BINS packet-bin counters / cursors
    // frame-less heavy-first trace order (env SF_PROG_ORDER=1; default off: with the packet-mode leaf
    // skip it measured 1-2 % slower, the longest waves no longer set the batch): per bin the cycles of
    // the last wave that started in it, its histogram per 64-bin chunk, and the bins' heavy-first rank
    bool prog_order = false;
    uint32_t* bin_cost = nullptr;
    uint32_t* bin_rank = nullptr;
    uint32_t* bin_order = nullptr;
    uint32_t* bin_chunk_cnt = nullptr;
    uint32_t* bin_chunk_off = nullptr;
    uint32_t* bin_meta = nullptr;
    uint32_t bin_key = 0;              // (shift, bins) of the batches whose costs bin_cost holds; 0 = none
    bool prog_bin = true;              // env SF_PROG_BIN=0: trace packets in draw order
    // Draw prefetch: after a large batch, the next batch's mt19937 draws (same stream, same size) are
    // generated on pf_stream while this batch traces -- the generator is one sequential workgroup.
    // A call that does not continue the stream restores the state saved before the prefetch.
    uint32_t* draws_pf = nullptr;      // the prefetched draws (prog_cap x 2)
    // ... and, where the batch is binned in index order, its binned trace order (the bins depend on the draws,
    // the Sobol index and the frame size only, not on the view): the next batch starts with its trace
    uint32_t* perm_pf = nullptr;       // prog_cap
    uint32_t* bin_cnt_pf = nullptr;    // SF_PROG_MAX_BINS
    uint32_t pf_bin_pl = 0;            // packet lanes the prefetched order was binned for (0: not binned)
    uint32_t* mt_saved = nullptr;      // MT state before the pending prefetch
    hipStream_t pf_stream = nullptr;
    hipEvent_t pf_done = nullptr;      // prefetch written (pf_stream)
    hipEvent_t mt_ready = nullptr;     // this batch's draws generated on the render stream
    hipEvent_t traced = nullptr;       // the last batch's trace done reading its draws
    // parallel draws (env SF_MT_PARALLEL=0: the single-workgroup generator only)
    bool mt_parallel = true;
    uint32_t mt_seg_max = kMtSegMax;   // env SF_MT_SEGMENTS: at most this many segments per call (2..kMtSegMax)
    uint32_t* mt_raw = nullptr;        // kMtRawBlocks x 624 raw words from the state's buffer
    uint32_t* mt_partial = nullptr;    // (kMtSegMax - 1) x kMtParts partial windows
    uint32_t* mt_state2 = nullptr;     // the state after the batch (copied back into mt_state)
    uint64_t* mt_polys = nullptr;      // kMtSegMax jump polynomials t^(j L) mod phi
    uint64_t mt_poly_key = 0;          // (L << 8 | K) of the uploaded polynomials
    bool traced_valid = false;
    uint32_t pf_packets = 0;           // draws pending for a batch of this many packets (0: none)
    bool prog_prefetch = true;         // env SF_PROG_PREFETCH=0: off
    // Adaptive traversal levels: LDS for the deepest level seen so far + 1 (as full frames) instead of
    // SF_PROGRESSIVE_LEVELS (twice the occupancy); a wave that needs more is re-traced by
    // sf_progressive_fixup. env SF_PROG_ADAPT=0: always SF_PROGRESSIVE_LEVELS.
    bool prog_adapt = true;
    int32_t* h_prog_depth = nullptr;   // pinned copy of the max-depth stat after each batch
    uint32_t* prog_ovf = nullptr;      // overflowed wave indices (prog_cap waves)
    uint32_t* prog_ovf_cnt = nullptr;  // [2] list counts, alternating per batch
    uint32_t prog_par = 0;
    unsigned long long* owner = nullptr;   // per pixel: highest ticket written
    // caller-supplied directions (sf_trace_dirs_to): the feature's own re-trace list and counters, so a trace of
    // directions leaves the renders' overflow state, schedule and hints alone
    uint32_t* dirs_ovf = nullptr;      // flagged groups of one trace (dirs_cap entries)
    uint32_t dirs_cap = 0;             // groups the list holds
    uint32_t* dirs_cnt = nullptr;      // [0,1] list counts, alternating per trace; [2] groups re-traced so far
    uint32_t dirs_par = 0;
    float* probe_buf = nullptr;        // sf_probe_dirs: device scratch, 3 + 4 + 4 + 1 + 1 words per ray
    uint32_t probe_cap = 0;            // rays it holds
    float* rprobe_buf = nullptr;       // sf_probe_rays: device scratch, 16 words per ray
    uint32_t rprobe_cap = 0;           // rays it holds
    bool prog_seeded = false;
    uint32_t prog_seed = 0;
    uint64_t prog_next = 0;            // Sobol counter the device MT stream is positioned at
    uint64_t ticket = 1;
    // LDS provisioning hint: max depth seen by a completed render (pinned copy of the device
    // stats word, refreshed asynchronously after every render). Only sizes the traversal stack;
    // a tile that needs more is re-traced by sf_fixup_wave, so a stale hint costs time, never results.
    int32_t* h_depth = nullptr;
    int32_t* h_stats = nullptr;        // pinned: the stats words, copied on the stream by sf_synchronize
    bool stats_dirty = true;           // work was enqueued since the last sf_synchronize checked the stats
    // the stats' unresolved word may have changed since that check: every enqueuing call but a persistent trace
    // with its levels proven and its ties re-traced inline, which adds 0 to it (its max-depth / closest words are
    // read by sf_get_stats, not here) -- after only such traces sf_synchronize needs no stats copy, just the wait
    bool stats_unknown = true;
    int32_t unresolved = 0;            // the stats' unresolved-tile count at the last check
    uint64_t* tile_trace = nullptr;    // diagnostics: per tile {start, end, hw id}
    // Heavy-first tile scheduling: every persistent render records per-tile cycles; sf_tile_order
    // turns them into the next render's tile permutation (heaviest first), so the tail of the
    // persistent kernel drains light tiles. Results never depend on the order.
    uint32_t* tile_cost = nullptr;
    uint32_t* tile_order = nullptr;
    uint32_t* chunk_cnt = nullptr;     // per 64-tile chunk x SF_ORDER_BUCKETS (zeroed by sf_order_scatter)
    uint32_t* chunk_off = nullptr;
    uint32_t* order_meta = nullptr;    // [0] work units in tile_order, [1] first split bucket, [2] parts per split tile, [3] first raised-priority bucket
    uint32_t* order_tot = nullptr;     // per cost bucket: tiles of the rebuilding render (sf_order_bucket_scan)
    uint32_t* part_cost = nullptr;     // per tile: slowest part of a split tile (zeroed, reset by the last part)
    uint32_t* part_done = nullptr;     // per tile: parts finished (zeroed, reset by the last part)
    // env SF_SPLIT_PARTS=subtree: split tiles traced as 4 subtree parts (SF_FLAG_SUBTREE) instead of pixel quarters;
    // part_rec holds their per-pixel results (SF_SPLIT_CAP split slots), split_depth_env the depth they divide
    // (0: the view's deepest LOD-passable depth - 2)
    uint64_t* part_rec = nullptr;
    uint32_t split_depth_env = 0;
    uint32_t order_n = 0;              // unit count the current tile_order is a permutation of (0: none)
    bool order_pair = false;           // its units are pair units (sf_trace_queue1), not tiles
    // Stream ordering across calls: every call that enqueues work on the context's buffers first joins
    // the stream of the previous such call (ctx_join), so renders, frame-less batches, post-processing
    // and downloads issued on different streams of one context run in call order, as on one stream.
    hipStream_t last_stream = nullptr; // stream of the latest enqueued work (nullptr: the context stream)
    hipEvent_t join_ev = nullptr;      // the point later calls order after (see ctx_join / StreamMark)
    // The frame-less prefetch stream at the device's greatest priority (env SF_PF_PRIO=0: normal): HIP deals streams
    // over GPU_MAX_HW_QUEUES (4) hardware queues, and in a process that made other streams first (the bench) the
    // prefetch stream shared the context stream's queue, serialising the next batch's draws behind this batch's
    // trace: SSE 0.440 -> 0.306, AVX 0.607 -> 0.480 ms per 2^18-packet batch in the bench process; a fresh process
    // measured 0.322 / 0.509 with normal priority (profiles/r4/frameless.txt)
    bool pf_prio = true;
    bool tie_inline = true;            // env SF_TIE_INLINE=0: ties under the front-first order go to sf_fixup_wave
    uint32_t order_phase = 0;          // renders since the last rebuild
    // Measurement: HIP events around the main trace kernel of each render (sf_set_kernel_timing)
    static constexpr int kTimed = 64;
    hipEvent_t ev[kTimed][2] = {};
    uint64_t* clock_buf = nullptr;     // per timed render slot: SF_CLOCK_WAVES x {memtime, realtime} at start / end
    bool timing = false;
    uint32_t ev_next = 0, ev_count = 0;
    uint32_t ev_period = 1, ev_phase = 0;   // time every ev_period-th render
    // SSAO post-process (sf_post_process): lazily allocated
    float* noise = nullptr;            // 64x64 float4
    uint8_t* ao = nullptr;             // SSAO target, sized for post_ao_px pixels
    size_t post_ao_px = 0;
    uint8_t* blur_h = nullptr;         // W x H
    uint8_t* blur_v = nullptr;
    uint8_t* image = nullptr;          // W x H RGBA8
    uint8_t* shadow = nullptr;         // W x H visibility bytes (sf_trace_shadow): lazily allocated
    uint64_t* shadow_masks = nullptr;  // W x H visibility masks (sf_trace_shadows): lazily allocated
    float* light = nullptr;            // W x H float4 light buffer (sf_light_fill, sf_trace_suns_sum): lazily allocated
    float* light_filtered = nullptr;   // W x H float4: sf_light_filter's target before the copy back, lazily allocated
    // sf_light_accumulate's history, W x H float4 each, lazily allocated: the last accumulated frame's positions,
    // normals and light, with the origin they are relative to and that view's sf_reproject_matrix
    float* hist_pos = nullptr;
    float* hist_nrm = nullptr;
    float* hist_light = nullptr;
    float hist_o[3] = {};
    float hist_m[9] = {};
    bool hist_valid = false;
    int centre_exact = -1;             // sfhost::post_centre_exact(W) && (H), cached
};

#define SF_HIP(ctx, expr)                                        \
    do {                                                         \
        hipError_t e_ = (expr);                                  \
        if (e_ != hipSuccess) {                                  \
            if (ctx) (ctx)->last_hip = (int)e_;                  \
            return SF_EHIP;                                      \
        }                                                        \
    } while (0)

// Order work about to be enqueued on `s` after everything the context enqueued before, on whatever
// stream (one event wait, only when the stream changes; same-stream calls cost nothing). A call that
// enqueued on a caller's stream records join_ev on it when it returns (StreamMark), so the context never
// touches that stream again afterwards: the caller may destroy it once the work is done.
static int ctx_join(sf_ctx* c, hipStream_t s)
{
    c->stats_dirty = true;   // (every call that enqueues work joins first)
    c->stats_unknown = true;   // (a trace that cannot change the unresolved word restores it, launch())
    hipStream_t last = c->last_stream ? c->last_stream : c->stream;
    if (s == last) return SF_OK;
    if (last == c->stream) SF_HIP(c, hipEventRecord(c->join_ev, c->stream));   // (the context's own stream)
    SF_HIP(c, hipStreamWaitEvent(s, c->join_ev, 0));
    c->last_stream = s == c->stream ? nullptr : s;
    return SF_OK;
}

// End of a call that enqueued on `s`: on a caller's stream, mark the point every later call orders after.
struct StreamMark {
    sf_ctx* c;
    hipStream_t s;
    StreamMark(sf_ctx* c_, hipStream_t s_) : c(c_), s(s_) {}
    ~StreamMark()
    {
        if (s != c->stream) (void)hipEventRecord(c->join_ev, s);
    }
};

// Host-synchronous drain: all work the context enqueued on any stream is done.
static int ctx_drain(sf_ctx* c)
{
    if (int rc = ctx_join(c, c->stream)) return rc;
    SF_HIP(c, hipStreamSynchronize(c->stream));
    return SF_OK;
}

static void free_ctx(sf_ctx* c)
{
    if (!c) return;
    DevGuard g(c->device);
    if (c->last_stream && c->join_ev) (void)hipEventSynchronize(c->join_ev);   // (never the caller's stream)
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->join_ev) (void)hipEventDestroy(c->join_ev);
    (void)hipFree(c->pos);
    (void)hipFree(c->nrm);
    (void)hipFree(c->min_t);
    (void)hipFree(c->hit_index);
    (void)hipFree(c->stats);
    (void)hipFree(c->ovf_counters);
    (void)hipFree(c->ovf_list);
    (void)hipFree(c->node_table);
    (void)hipFree(c->consts);
    (void)hipFree(c->shadow_consts);
    (void)hipFree(c->mt_state);
    (void)hipFree(c->draws);
    (void)hipFree(c->lanes);
    (void)hipFree(c->perm);
    (void)hipFree(c->bin_cnt);
    (void)hipFree(c->bin_cost);
    (void)hipFree(c->bin_rank);
    (void)hipFree(c->bin_order);
    (void)hipFree(c->bin_chunk_cnt);
    (void)hipFree(c->bin_chunk_off);
    (void)hipFree(c->bin_meta);
    if (c->pf_stream) (void)hipStreamSynchronize(c->pf_stream);
    if (c->h_prog_depth) (void)hipHostFree(c->h_prog_depth);
    (void)hipFree(c->prog_ovf);
    (void)hipFree(c->prog_ovf_cnt);
    (void)hipFree(c->draws_pf);
    (void)hipFree(c->perm_pf);
    (void)hipFree(c->bin_cnt_pf);
    (void)hipFree(c->mt_saved);
    (void)hipFree(c->mt_raw);
    (void)hipFree(c->mt_partial);
    (void)hipFree(c->mt_state2);
    (void)hipFree(c->mt_polys);
    if (c->pf_done) (void)hipEventDestroy(c->pf_done);
    if (c->mt_ready) (void)hipEventDestroy(c->mt_ready);
    if (c->traced) (void)hipEventDestroy(c->traced);
    if (c->pf_stream) (void)hipStreamDestroy(c->pf_stream);
    (void)hipFree(c->owner);
    (void)hipFree(c->dirs_ovf);
    (void)hipFree(c->dirs_cnt);
    (void)hipFree(c->probe_buf);
    (void)hipFree(c->rprobe_buf);
    if (c->h_depth) (void)hipHostFree(c->h_depth);
    if (c->h_stats) (void)hipHostFree(c->h_stats);
    (void)hipFree(c->tile_trace);
    (void)hipFree(c->tile_cost);
    (void)hipFree(c->tile_order);
    (void)hipFree(c->chunk_cnt);
    (void)hipFree(c->chunk_off);
    (void)hipFree(c->order_meta);
    (void)hipFree(c->order_tot);
    (void)hipFree(c->part_cost);
    (void)hipFree(c->part_done);
    (void)hipFree(c->part_rec);
    (void)hipFree(c->noise);
    (void)hipFree(c->ao);
    (void)hipFree(c->blur_h);
    (void)hipFree(c->blur_v);
    (void)hipFree(c->image);
    (void)hipFree(c->shadow);
    (void)hipFree(c->shadow_masks);
    (void)hipFree(c->light);
    (void)hipFree(c->light_filtered);
    (void)hipFree(c->hist_pos);
    (void)hipFree(c->hist_nrm);
    (void)hipFree(c->hist_light);
    for (int i = 0; i < sf_ctx::kTimed; ++i)
        for (int j = 0; j < 2; ++j)
            if (c->ev[i][j]) (void)hipEventDestroy(c->ev[i][j]);
    (void)hipFree(c->clock_buf);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

static float variant_lod(const sf_ctx* c) { return c->variant == SF_VARIANT_SSE ? 60.0f : 70.0f; }

// the context's constant block for the LOD constant `lod_constant`, on the host
static void fill_consts(const sf_ctx* c, DeviceConsts* h, float lod_constant)
{
    std::memcpy(h->child, c->child, sizeof c->child);
    sfhost::depth_tables(&h->dt, lod_constant);
    for (int d = 0; d < SF_DEPTH_TABLE; ++d) {
        float* e = h->depth8[d];
        e[0] = h->dt.r2_bound[d];
        e[1] = h->dt.r2_self[d];
        e[2] = h->dt.scale[d];
        e[3] = h->dt.lod[d];
        e[4] = sfhost::leaf_threshold(&h->dt, (uint32_t)d);
        e[5] = std::nextafter((float)(std::sqrt((double)e[0]) * (1.0 + 2.0 * (double)SF_OCCL_MARGIN)), FLT_MAX);
        e[6] = std::nextafter((float)((double)e[3] + std::sqrt((double)e[0]) * (1.0 + 0x1p-18)), FLT_MAX);
        e[7] = 0.0f;
    }
    std::memcpy(h->lut, kLut, sizeof kLut);
    sfhost::sobol_matrices(h->sobol);
    h->rw = 1.0f / (float)c->W;
    h->rh = 1.0f / (float)c->H;
    h->fast_div = c->fast_div ? 1u : 0u;
    h->tx_magic = 0xffffffffu / ((c->W + 7) / 8);
}

// The shadow traces' block alone (sf_set_shadow_lod; the child frames and the variant as they stand).
static int upload_shadow_consts(sf_ctx* c)
{
    fill_consts(c, &c->host_shadow_consts, c->shadow_lod > 0.0f ? c->shadow_lod : variant_lod(c));
    if (int rc_ = ctx_drain(c)) return rc_;   // no kernel of the context may still read the block
    SF_HIP(c, hipMemcpyAsync(c->shadow_consts, &c->host_shadow_consts, sizeof(DeviceConsts), hipMemcpyHostToDevice,
                             c->stream));
    SF_HIP(c, hipStreamSynchronize(c->stream));
    return SF_OK;
}

static int upload_consts(sf_ctx* c)
{
    fill_consts(c, &c->host_consts, variant_lod(c));
    if (int rc_ = ctx_drain(c)) return rc_;   // no kernel of the context may still read the block
    ++c->consts_gen;
    SF_HIP(c, hipMemcpyAsync(c->consts, &c->host_consts, sizeof(DeviceConsts), hipMemcpyHostToDevice, c->stream));
    SF_HIP(c, hipStreamSynchronize(c->stream));
    return upload_shadow_consts(c);   // (the children or the variant changed: the shadow traces' block follows)
}

static int reset_stats_dev(sf_ctx* c, int which)
{
    // which: bit0 max depth, bit1 closest
    int32_t init[2] = { -1, sf_float_key(FLT_MAX) };
    if (int rc_ = ctx_join(c, c->stream)) return rc_;   // after every render that updates the words
    if (which & 1) SF_HIP(c, hipMemcpyAsync(c->stats + 0, &init[0], 4, hipMemcpyHostToDevice, c->stream));
    if (which & 2) SF_HIP(c, hipMemcpyAsync(c->stats + 1, &init[1], 4, hipMemcpyHostToDevice, c->stream));
    SF_HIP(c, hipStreamSynchronize(c->stream));
    return SF_OK;
}

extern "C" {

int sf_abi_version(void) { return SF_ABI_VERSION; }

const char* sf_build_id(void) { return SF_SOURCE_HASH; }

int sf_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* sf_strerror(int s)
{
    switch (s) {
    case SF_OK: return "ok";
    case SF_EINVAL: return "invalid argument";
    case SF_ENOMEM: return "out of memory";
    case SF_EHIP: return "HIP runtime error";
    case SF_ENODEV: return "no such device or not a gfx950 (MI355X) device";
    case SF_ENOVIEW: return "render before SetView";
    case SF_EDEPTH: return "traversal deeper than SF_MAX_DEPTH_LIMIT";
    case SF_ESTATE: return "invalid state";
    case SF_ECOMM: return "RCCL error";
    default: return "unknown error";
    }
}

int sf_last_hip_error(const sf_ctx* ctx) { return ctx ? ctx->last_hip : 0; }

int sf_get_size(const sf_ctx* ctx, uint32_t* width, uint32_t* height)
{
    if (!ctx) return SF_EINVAL;
    if (width) *width = ctx->W;
    if (height) *height = ctx->H;
    return SF_OK;
}

int sf_create(int device, uint32_t width, uint32_t height, sf_ctx** out)
{
    if (!out || width == 0 || height == 0) return SF_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return SF_ENODEV;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return SF_ENODEV;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return SF_ENODEV;

    sf_ctx* c = new (std::nothrow) sf_ctx();
    if (!c) return SF_ENOMEM;
    c->device = device;
    c->W = width;
    c->H = height;
    c->fast_div = sfhost::division_by_reciprocal_exact(width) && sfhost::division_by_reciprocal_exact(height);
    c->fixup_blocks = prop.multiProcessorCount;
    c->cus = prop.multiProcessorCount;
    {   // gfx950: 32 CUs per XCD; a compute partition of the chip exposes fewer XCDs (then fewer queues)
        uint32_t x = c->cus >= 32 ? (uint32_t)c->cus / 32u : 1u, q = 1u;
        while (q * 2u <= x && q * 2u <= 8u) q *= 2u;
        c->knobs.xcd_groups = q;
        if (const char* ev = std::getenv("SF_NQUEUES")) {
            const int v = std::atoi(ev);
            if (v == 1 || v == 2 || v == 4 || v == 8) c->knobs.xcd_groups = (uint32_t)v;
        }
        if (const char* ev = std::getenv("SF_QUEUES_PER_XCD")) {
            const int v = std::atoi(ev);
            if (v == 1 || v == 2 || v == 4) c->knobs.queues_per_xcd = (uint32_t)v;
        }
    }
    if (const char* ev = std::getenv("SF_PERSISTENT")) c->persistent = std::atoi(ev) != 0;
    if (const char* ev = std::getenv("SF_ORDER")) c->knobs.order_mode = std::atoi(ev) != 0 ? 1 : 0;
    if (const char* ev = std::getenv("SF_COMPACT")) c->knobs.compact = std::atoi(ev) != 0;
    if (const char* ev = std::getenv("SF_PF_PRIO")) c->pf_prio = std::atoi(ev) != 0;
    if (const char* ev = std::getenv("SF_TIE_INLINE")) c->tie_inline = std::atoi(ev) != 0;
    if (const char* ev = std::getenv("SF_LEAN")) c->knobs.lean = std::atoi(ev) != 0;
    if (const char* ev = std::getenv("SF_PAIR")) c->knobs.pair = std::atoi(ev) != 0 ? 1 : 0;
    if (const char* ev = std::getenv("SF_ORDER_RECORD")) c->knobs.order_record = std::atoi(ev) != 0 ? 1 : 0;
    if (const char* ev = std::getenv("SF_ORDER_EVERY")) c->knobs.order_every = std::atoi(ev) > 1 ? (uint32_t)std::atoi(ev) : 1u;   // (explicit)
    if (const char* ev = std::getenv("SF_PROG_BIN")) c->prog_bin = std::atoi(ev) != 0;
    if (const char* ev = std::getenv("SF_PROG_PREFETCH")) c->prog_prefetch = std::atoi(ev) != 0;
    if (const char* ev = std::getenv("SF_PROG_ADAPT")) c->prog_adapt = std::atoi(ev) != 0;
    if (const char* ev = std::getenv("SF_PROG_ORDER")) c->prog_order = std::atoi(ev) != 0;
    if (const char* ev = std::getenv("SF_MT_PARALLEL")) c->mt_parallel = std::atoi(ev) != 0;
    if (const char* ev = std::getenv("SF_MT_SEGMENTS")) {
        const int k = std::atoi(ev);
        c->mt_seg_max = k < 2 ? 2u : k > (int)kMtSegMax ? kMtSegMax : (uint32_t)k;
    }
    if (const char* ev = std::getenv("SF_SPLIT_BUCKETS"))
        c->knobs.split_buckets = std::strcmp(ev, "model") == 0 ? SF_SPLIT_MODEL
                         : std::strcmp(ev, "auto") == 0 ? SF_SPLIT_AUTO : (uint32_t)std::atoi(ev);
    if (std::getenv("SF_SPLIT_BUCKETS")) c->knobs.split_env = true;
    if (const char* ev = std::getenv("SF_HALVES")) c->knobs.halves = std::atoi(ev);
    bool subtree = false;
    if (const char* ev = std::getenv("SF_SPLIT_PARTS")) {
        subtree = std::strcmp(ev, "subtree") == 0;
        c->knobs.split_parts = (subtree || std::atoi(ev) == 4) ? 4u : 2u;
        c->knobs.subtree = subtree;   // (part_rec is allocated below)
    }
    if (const char* ev = std::getenv("SF_SPLIT_DEPTH")) c->split_depth_env = (uint32_t)std::atoi(ev);
    if (const char* ev = std::getenv("SF_MAX_BLOCKS")) c->knobs.max_blocks = (uint32_t)std::atoi(ev);
    if (const char* ev = std::getenv("SF_PRIO_BUCKETS")) c->prio_buckets = (uint32_t)std::atoi(ev);
    if (const char* ev = std::getenv("SF_FLAGS")) c->flags = (uint32_t)std::strtoul(ev, nullptr, 0);
    const char* const pipe_env = std::getenv("SF_PIPE");
    if (const char* ev = std::getenv("SF_TRACE_WAVES")) {
        const int w = std::atoi(ev);
        c->knobs.waves_per_block = (w == 1 || w == 2 || w == 4) ? (uint32_t)w : SF_TRACE_WAVES;
    } else if (c->knobs.compact || (pipe_env && std::atoi(pipe_env) != 0)) {
        // the compaction variant is a 2-wave kernel; SF_PIPE=1 once chose a latency variant that was one too, and
        // still means two waves per workgroup (SF_PIPE=0: nothing)
        c->knobs.waves_per_block = 2;
    }
    if (const char* ev = std::getenv("SF_LEVELS")) {
        const int l = std::atoi(ev);
        c->levels_override = (l >= 2 && l <= SF_MAX_DEPTH_LIMIT) ? (uint32_t)l : 0u;
    }
    if (const char* ev = std::getenv("SF_DIAG_SLAB_SHALLOW")) c->slab_shallow = std::atoi(ev) != 0;   // (tests only)
    if (const char* ev = std::getenv("SF_FRAMES_HEAVY")) c->frames_heavy = std::atoi(ev);
    if (const char* ev = std::getenv("SF_FRAMES_ONE")) c->frames_one = std::atoi(ev) != 0;
    DevGuard g(device);
    const size_t npx = (size_t)width * height;
    const size_t ntiles = (size_t)((width + 7) / 8) * ((height + 7) / 8);
    if (ntiles > (size_t)SF_UNIT_TILE_MASK + 1u) {   // a work unit holds the tile index in 27 bits
        delete c;
        return SF_EINVAL;
    }
    auto fail = [&](hipError_t e) {
        c->last_hip = (int)e;
        free_ctx(c);
        return e == hipErrorOutOfMemory ? SF_ENOMEM : SF_EHIP;
    };
    hipError_t e;
    if ((e = stream_acquire(device, &c->stream)) != hipSuccess) return fail(e);
    if ((e = hipEventCreateWithFlags(&c->join_ev, hipEventDisableTiming)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&c->pos, npx * 16)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&c->nrm, npx * 16)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&c->min_t, npx * 4)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&c->hit_index, npx * 4)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&c->stats, 16)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&c->ovf_counters, SF_COUNTER_WORDS * 4)) != hipSuccess) return fail(e);
    // each work unit pushes its tile at most once and a tile has <= 4 units: 4 entries per tile
    if ((e = hipMalloc(&c->ovf_list, 4 * ntiles * 4)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&c->tile_cost, ntiles * 4)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&c->tile_order, 4 * ntiles * 4)) != hipSuccess) return fail(e);   // <= 4 units per tile
    if ((e = hipMalloc(&c->order_meta, 4 * 4)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&c->order_tot, SF_ORDER_BUCKETS * 4)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&c->part_cost, ntiles * 4)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&c->part_done, ntiles * 4)) != hipSuccess) return fail(e);
    if ((e = hipMemsetAsync(c->part_cost, 0, ntiles * 4, c->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemsetAsync(c->part_done, 0, ntiles * 4, c->stream)) != hipSuccess) return fail(e);
    if (subtree && (e = hipMalloc(&c->part_rec, (size_t)SF_SPLIT_CAP * 4u * 192u * 8u)) != hipSuccess) return fail(e);
    const size_t nchunks = (ntiles + 63) / 64;
    if ((e = hipMalloc(&c->chunk_cnt, nchunks * SF_ORDER_BUCKETS * 4)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&c->chunk_off, nchunks * SF_ORDER_BUCKETS * 4)) != hipSuccess) return fail(e);
    if ((e = hipMemsetAsync(c->chunk_cnt, 0, nchunks * SF_ORDER_BUCKETS * 4, c->stream)) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&c->consts, sizeof(DeviceConsts))) != hipSuccess) return fail(e);
    if ((e = hipMalloc(&c->shadow_consts, sizeof(DeviceConsts))) != hipSuccess) return fail(e);
    if ((e = hipHostMalloc(&c->h_depth, 4, hipHostMallocDefault)) != hipSuccess) return fail(e);
    if ((e = hipHostMalloc(&c->h_stats, 16, hipHostMallocDefault)) != hipSuccess) return fail(e);
    *c->h_depth = -1;
    // G-buffer starts as glm vec4() = (0,0,0,0) (Sphereflake.cpp:48-49, type_vec4.inl:59-64)
    if ((e = hipMemsetAsync(c->pos, 0, npx * 16, c->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemsetAsync(c->nrm, 0, npx * 16, c->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemsetAsync(c->min_t, 0, npx * 4, c->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemsetAsync(c->hit_index, 0xff, npx * 4, c->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemsetAsync(c->stats, 0, 16, c->stream)) != hipSuccess) return fail(e);
    if ((e = hipMemsetAsync(c->ovf_counters, 0, SF_COUNTER_WORDS * 4, c->stream)) != hipSuccess) return fail(e);
    sfhost::child_transforms(c->child);
    int rc = upload_consts(c);
    if (rc == SF_OK) rc = reset_stats_dev(c, 3);
    if (rc != SF_OK) {
        free_ctx(c);
        return rc;
    }
    *out = c;
    return SF_OK;
}

void sf_destroy(sf_ctx* ctx) { free_ctx(ctx); }

int sf_set_view(sf_ctx* c, const float origin[3], const float tl[3], const float tr[3], const float bl[3])
{
    if (!c || !origin || !tl || !tr || !bl) return SF_EINVAL;
    std::memcpy(c->o, origin, 12);
    std::memcpy(c->tl, tl, 12);
    std::memcpy(c->tr, tr, 12);
    std::memcpy(c->bl, bl, 12);
    sfhost::root_transform(origin, c->root);
    c->has_view = true;
    return SF_OK;
}

int sf_set_setup(sf_ctx* c, const float child[9][16], const float root[16])
{
    if (!c || !child || !root) return SF_EINVAL;
    // the kernels fuse the 4th term of every child product (SF_AFFINE_FMA, sf_kernels.hip): exact only for affine unit
    // child frames, row 3 = (0, 0, 0, 1) -- what the reference's ComputeChildTransformations makes
    for (int i = 0; i < 9; ++i)
        for (int col = 0; col < 4; ++col)
            if (child[i][4 * col + 3] != (col == 3 ? 1.0f : 0.0f)) return SF_EINVAL;
    DevGuard g(c->device);
    std::memcpy(c->child, child, sizeof c->child);
    std::memcpy(c->root, root, sizeof c->root);
    return upload_consts(c);
}

int sf_get_setup(const sf_ctx* c, float child[9][16], float root[16])
{
    if (!c) return SF_EINVAL;
    if (child) std::memcpy(child, c->child, sizeof c->child);
    if (root) std::memcpy(root, c->root, sizeof c->root);
    return SF_OK;
}

uint32_t sf_slab_rows(uint32_t height, uint32_t band_rows, uint32_t band_count, uint32_t band_index)
{
    return sfplan::band_share(height, band_rows, band_count, band_index).rows;
}

static FrameArgs frame_args(const sf_ctx* c)
{
    FrameArgs a;
    std::memset(&a, 0, sizeof a);
    a.W = c->W;
    a.H = c->H;
    a.fw = (float)c->W;                  // (float)m_Width (Sphereflake.cpp:104-110)
    a.fh = (float)c->H;
    for (int k = 0; k < 3; ++k) {
        a.o[k] = c->o[k];
        a.tl[k] = c->tl[k];
        a.dh[k] = c->tr[k] - c->tl[k];   // m_TopRight - m_TopLeft (Sphereflake.cpp:162)
        a.dv[k] = c->bl[k] - c->tl[k];   // m_BottomLeft - m_TopLeft (Sphereflake.cpp:163)
    }
    for (int col = 0; col < 4; ++col)
        for (int r = 0; r < 3; ++r) a.root[3 * col + r] = c->root[4 * col + r];
    a.tiles_x = (c->W + 7) / 8;
    a.band_count = 1;
    a.consts = c->consts;
    a.stats = c->stats;
    a.flags = c->flags;
    a.xcds = c->knobs.xcd_groups;
    a.queues = c->knobs.xcd_groups;   // (the plan's split once the persistent grid is known, plan_frame_args)
    return a;
}

// The next render's tile order from the tile costs the render just enqueued on `s` recorded (sf_order_scan /
// sf_order_bucket_scan + sf_order_scatter_plan); `waves`: resident waves of its persistent grid.
// (ntiles: the units the costs are indexed by -- tiles, or with `pair` the pair units of sf_trace_queue1c)
static int order_rebuild(sf_ctx* c, hipStream_t s, uint32_t ntiles, uint32_t waves, uint32_t split_buckets, bool pair = false)
{
    const uint32_t nc = (ntiles + 63u) / 64u;
    const uint32_t spare = waves > ntiles ? waves - ntiles : 0u;
    // few chunks: the scan's workgroup also scatters (one launch: ~3 us less host time and one
    // dispatch less on the frame's stream); more: one wave per chunk in a launch of its own
    const bool fuse = nc <= SF_ORDER_FUSE_CHUNKS;
    const uint32_t cap = c->part_rec ? SF_SPLIT_CAP : 0xffffffffu;
    if (fuse) {
        hipLaunchKernelGGL(sf_order_scan, dim3(1), dim3(1024), 0, s, c->chunk_cnt, nc, ntiles, split_buckets,
                           c->knobs.split_parts, spare, waves, c->prio_buckets, c->chunk_off, c->order_meta,
                           (const uint32_t*)c->tile_cost, c->tile_order, cap);
        SF_HIP(c, hipGetLastError());
    } else {   // (round 5: one-wave workgroups only -- see sf_order_bucket_scan)
        hipLaunchKernelGGL(sf_order_bucket_scan, dim3(SF_ORDER_BUCKETS), dim3(64), 0, s, (const uint32_t*)c->chunk_cnt,
                           nc, c->chunk_off, c->order_tot);
        SF_HIP(c, hipGetLastError());
        hipLaunchKernelGGL(sf_order_scatter_plan, dim3(nc), dim3(64), 0, s, (const uint32_t*)c->tile_cost, ntiles,
                           c->chunk_cnt, (const uint32_t*)c->chunk_off, (const uint32_t*)c->order_tot, split_buckets,
                           c->knobs.split_parts, spare, waves, c->prio_buckets, cap, c->order_meta, c->tile_order);
        SF_HIP(c, hipGetLastError());
    }
    c->order_n = ntiles;
    c->order_pair = pair;
    return SF_OK;
}

// LDS traversal levels for the context's view, and whether they are proven sufficient (no tile can overflow).
// Geometric bound: every sphere lies inside the root's bounding sphere (radius 2 around the root centre), so a
// depth-d node can pass the LOD test (t < T_d, Sphereflake.h:146) only if |root centre| - 2 < T_d. The deepest such
// d + 1 levels suffice; a bound that is off only costs a re-trace of the affected tiles (sf_fixup_wave), never results.
// (geometric_levels: the bound alone -- it speaks of the origin and the root ball only, so it holds for rays of any
// direction, sf_trace_dirs_to; frame_levels: narrowed by the deepest depth a finished render of the frame saw)
// (centre: the root centre relative to the rays' origin -- the view's root translation, or 0 - light for sf_trace_shadow_to)
// (dt: the depth tables the trace runs on -- the context's, or the shadow traces' own, sf_set_shadow_lod)
static uint32_t geometric_levels(const DepthTables& dt, const float centre[3], bool* bounded_out)
{
    uint32_t levels = kDefaultLevels;
    const float rc = std::sqrt(centre[0] * centre[0] + centre[1] * centre[1] + centre[2] * centre[2]);
    const float gap = (rc - 2.0f) * (1.0f - 1e-3f);
    bool bounded = false;
    if (gap > 0.0f) {
        uint32_t dmax = 0;
        while (dmax + 1u < SF_DEPTH_TABLE && dt.lod[dmax + 1u] > gap) ++dmax;
        levels = dmax + 1u;
        bounded = levels <= SF_MAX_DEPTH_LIMIT;
    }
    *bounded_out = bounded;
    return levels;
}
static uint32_t geometric_levels(const sf_ctx* c, bool* bounded_out)
{
    return geometric_levels(c->host_consts.dt, c->root + 12, bounded_out);
}

static uint32_t frame_levels(const sf_ctx* c, bool* bounded_out)
{
    bool bounded = false;
    uint32_t levels = geometric_levels(c, &bounded);
    const int32_t seen = *(volatile int32_t*)c->h_depth;   // max depth of a finished render
    if (seen >= 0 && (uint32_t)seen + 1u < levels) {
        levels = (uint32_t)seen + 1u;
        bounded = false;
    }
    if (levels < 4u) levels = 4u;
    if (levels > SF_MAX_DEPTH_LIMIT) levels = SF_MAX_DEPTH_LIMIT;
    if (c->levels_override) {
        levels = c->levels_override;
        bounded = false;
    }
    *bounded_out = bounded;
    return levels;
}

// The persistent trace kernels of one FrameArgs, by sfplan::Kernel (sf_trace_frames1 takes a FrameBatch).
typedef void (*QueueKernel)(FrameArgs);
static const QueueKernel kQueueKernels[sfplan::kFrames1] = { sf_trace_queue1,  sf_trace_queue1c, sf_trace_queue1s,
                                                             sf_trace_queue1t, sf_trace_queue1g, sf_trace_queue2,
                                                             sf_trace_queue2c, sf_trace_queue4 };

// Blocks per CU of the kernels a persistent launch() of these levels may take (occ_blocks: the general loop of the
// knobs' waves per block; occ_blocks_lean, occ_blocks_pair), cached by waves per block, levels and compaction.
static int queue_occupancy(sf_ctx* c, uint32_t levels, size_t lds)
{
    const uint32_t wpb = c->knobs.waves_per_block;
    const int key = (int)(wpb * 64 + levels) | (c->knobs.compact ? 1 << 20 : 0);
    if (c->occ_key == key) return SF_OK;
    const sfplan::Kernel general = wpb == 1 ? sfplan::kQueue1g
                                 : wpb == 2 ? (c->knobs.compact ? sfplan::kQueue2c : sfplan::kQueue2) : sfplan::kQueue4;
    int nb = 0;
    auto query = [&](sfplan::Kernel k) {
        return hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)kQueueKernels[k], (int)(64 * wpb), wpb * lds);
    };
    SF_HIP(c, query(general));
    c->occ_blocks = c->occ_blocks_lean = c->occ_blocks_pair = nb < 1 ? 1 : nb;
    if (wpb == 1) {
        SF_HIP(c, query(sfplan::kQueue1t));
        c->occ_blocks_lean = nb < 1 ? 1 : nb;
        SF_HIP(c, query(sfplan::kQueue1));
        c->occ_blocks_pair = nb < 1 ? 1 : nb;
        SF_HIP(c, query(sfplan::kQueue1c));
        if (nb >= 1 && nb < c->occ_blocks_pair) c->occ_blocks_pair = nb;   // (one grid for both pair kernels)
    }
    c->occ_key = key;
    return SF_OK;
}

// What launch() and sf_render_frames fill alike: the member's band share and, with a plan (the persistent traces),
// its queues, flags and the unit order it runs on -- `oc`'s, the context whose order state the plan was made from;
// `costs`: this frame is the one that records the unit costs the plan asks for.
static void plan_frame_args(FrameArgs& a, const sf_render_params& p, const sfplan::BandShare& sh,
                            const sfplan::RenderPlan* pl, const sf_ctx* oc, bool costs)
{
    a.tile_rows = sh.tile_rows;
    a.tiles_per_band = sh.tiles_per_band;
    a.tpb_magic = 0xffffffffu / sh.tiles_per_band;
    a.band_count = sh.band_count;
    a.band_index = p.band_index;
    a.emit_aux = p.emit_aux ? 1u : 0u;
    if (!pl) return;
    a.xcds = pl->xcds;
    a.queues = pl->queues;
    a.flags |= pl->flags_add;
    a.px_magic = pl->px_magic;
    if (!pl->use_order) return;
    a.tile_order = pl->have_order ? oc->tile_order : nullptr;   // ordered by ctx_join
    a.order_meta = oc->order_meta;
    a.part_cost = oc->part_cost;
    a.part_done = oc->part_done;
    if (costs) {
        a.tile_cost = pl->costs ? oc->tile_cost : nullptr;
        a.chunk_cnt = pl->rebuild ? oc->chunk_cnt : nullptr;
    }
}

extern "C++" {
// A trace launch inside the context's timing ring (sf_set_kernel_timing): every ev_period-th one runs between two
// events of the ring's next slot, and its first waves sample the clocks into that slot (*probe: the launch's
// FrameArgs.clock_probe, set before `enqueue` runs).
template <class Enqueue>
static int timed_launch(sf_ctx* c, hipStream_t s, uint64_t** probe, Enqueue enqueue)
{
    const bool timed = c->timing && c->ev_phase == 0;
    if (c->timing) c->ev_phase = (c->ev_phase + 1u) % c->ev_period;
    if (timed) {
        SF_HIP(c, hipEventRecord(c->ev[c->ev_next][0], s));
        *probe = c->clock_buf + (size_t)c->ev_next * SF_CLOCK_WAVES * 4u;
    }
    enqueue();
    SF_HIP(c, hipGetLastError());
    if (timed) {
        SF_HIP(c, hipEventRecord(c->ev[c->ev_next][1], s));
        c->ev_next = (c->ev_next + 1u) % sf_ctx::kTimed;
        c->ev_count = c->ev_count < (uint32_t)sf_ctx::kTimed ? c->ev_count + 1u : c->ev_count;
    }
    return SF_OK;
}
}   // extern "C++"

// sf_render / sf_render_to: validate; provision the levels (and, for the persistent trace, query the occupancy);
// plan the schedule (sf_plan.h); apply it.
static int launch(sf_ctx* c, const sf_render_params* pp, float* pos, float* nrm, float* min_t, uint32_t* hidx)
{
    if (!c) return SF_EINVAL;
    if (!c->has_view) return SF_ENOVIEW;
    if (!pos || !nrm) return SF_EINVAL;
    sf_render_params p;
    std::memset(&p, 0, sizeof p);
    if (pp) p = *pp;
    const sfplan::BandShare sh = sfplan::band_share(c->H, p.band_rows, p.band_count, p.band_index);
    if (sh.band_rows % 8 != 0 || p.band_index >= sh.band_count) return SF_EINVAL;
    if (p.kernel > SF_KERNEL_PER_RAY || p.max_depth > SF_MAX_DEPTH_LIMIT) return SF_EINVAL;
    hipStream_t s = p.stream ? (hipStream_t)p.stream : c->stream;
    DevGuard g(c->device);
    if (sh.tile_rows == 0) return SF_OK;
    const bool unknown_before = c->stats_unknown;
    if (int rc = ctx_join(c, s)) return rc;
    StreamMark mark_(c, s);

    FrameArgs a = frame_args(c);
    bool unresolved_safe = false;   // this launch adds nothing to the unresolved word (see sf_ctx::stats_unknown)
    a.compact = p.compact ? 1u : 0u;
    if (p.packed > SF_PACKED_INDEX) return SF_EINVAL;
    if (p.packed == SF_PACKED_INDEX && sf_slab_bytes(c) != 4u) return SF_EINVAL;   // (a hit could be too deep)
    a.packed = p.packed;
    if (a.packed == SF_PACKED_INDEX && c->slab_shallow) a.packed = SF_PACKED_INDEX_DIAG;
    if (a.packed && p.kernel == SF_KERNEL_PER_RAY) return SF_EINVAL;   // (the per-ray kernel writes the plain layout)
    a.pos = pos;
    a.nrm = nrm;
    a.min_t = min_t;
    a.hit_index = hidx;
    a.tile_trace = c->tile_trace;
    a.counters = c->ovf_counters;
    a.overflow_list = c->ovf_list;
    a.parity = c->parity;
    if (c->tile_trace) {
        const size_t ntr = (size_t)((c->W + 7) / 8) * ((c->H + 7) / 8);
        a.phase_sums = c->tile_trace + 3 * ntr;
    }

    const uint32_t ntiles = a.tiles_x * sh.tile_rows;
    if (p.kernel == SF_KERNEL_PER_RAY) {
        plan_frame_args(a, p, sh, nullptr, c, false);
        a.max_depth = 31;
        const uint32_t blocks = (ntiles + SF_WAVES_PER_BLOCK - 1) / SF_WAVES_PER_BLOCK;
        hipLaunchKernelGGL(sf_trace_ray, dim3(blocks), dim3(256), 0, s, a);
        SF_HIP(c, hipGetLastError());
    } else {
        const bool autod = p.max_depth == 0;
        bool bounded = false;   // levels proven sufficient: no tile can overflow
        uint32_t levels = frame_levels(c, &bounded);
        if (!autod) bounded = bounded && p.max_depth >= levels;
        a.max_depth = autod ? levels : p.max_depth;
        const size_t lds = (size_t)SF_LDS_WAVE_FLOATS(a.max_depth) * 4;
        uint32_t* cnt = c->ovf_counters + c->parity;
        const uint32_t wpb = c->knobs.waves_per_block;
        const dim3 block(64 * wpb);
        // levels proven sufficient on the persistent kernel: only a tie under the front-first child order can flag
        // a tile, and its own wave re-traces it in index order -- no fixup launch after the trace
        const bool front_first = (c->flags & (SF_FLAG_NO_OCCL_CULL | SF_FLAG_NO_FRONT_FIRST)) == 0u;
        const bool tie_inline = bounded && c->persistent && front_first && c->tie_inline;
        if (tie_inline) a.flags |= SF_FLAG_TIE_INLINE;
        if (c->persistent) {
            if (int rc = queue_occupancy(c, a.max_depth, lds)) return rc;
            const uint32_t cus = (uint32_t)c->cus;
            const sfplan::Launch ask = { a.tiles_x, sh.tile_rows, sh.band_count, a.compact != 0u, a.packed != 0u,
                                         p.emit_aux != 0, a.tile_trace != nullptr, a.flags, 0u };
            const sfplan::Grids full = { (uint32_t)c->occ_blocks * cus, (uint32_t)c->occ_blocks_lean * cus,
                                         (uint32_t)c->occ_blocks_pair * cus };
            const sfplan::RenderPlan pl = sfplan::render_plan(ask, c->knobs, full, { c->order_n, c->order_pair, c->order_phase });
            c->order_phase = pl.order_phase;
            plan_frame_args(a, p, sh, &pl, c, true);
            if (pl.subtree) {
                a.part_rec = c->part_rec;
                a.split_depth = c->split_depth_env ? c->split_depth_env : (levels > 3u ? levels - 3u : 1u);
            }
            if (pl.lean) c->lean_launches += 1u;   // (the pair loop counts as lean too)
            if (pl.pair) c->pair_launches += 1u;
            if (int rc = timed_launch(c, s, &a.clock_probe, [&] {
                    hipLaunchKernelGGL(kQueueKernels[pl.kernel], dim3(pl.grid), block, wpb * lds, s, a);
                }))
                return rc;
            if (pl.rebuild) {   // the next render's unit order, from this render's unit costs
                if (int rc = order_rebuild(c, s, pl.units, pl.order_waves, pl.split_buckets, pl.pair)) return rc;
            }
        } else {   // SF_PERSISTENT=0: one workgroup per tile group, no schedule
            plan_frame_args(a, p, sh, nullptr, c, false);
            const dim3 grid((ntiles + wpb - 1) / wpb);
            if (wpb == 1) hipLaunchKernelGGL(sf_trace_wave1, grid, block, lds, s, a, c->ovf_list, cnt);
            else if (wpb == 2) hipLaunchKernelGGL(sf_trace_wave2, grid, block, 2 * lds, s, a, c->ovf_list, cnt);
            else hipLaunchKernelGGL(sf_trace_wave4, grid, block, 4 * lds, s, a, c->ovf_list, cnt);
            SF_HIP(c, hipGetLastError());
        }
        // Re-trace of overflowed tiles (it also zeroes the next render's overflow counter itself). With the
        // levels proven sufficient (persistent kernel) only an exact tie under the front-first child order can
        // flag a tile -- never seen on the BASELINE views --: its own wave re-traces it (tie_inline), or with
        // SF_TIE_INLINE=0 the fixup's small grid.
        // (no fixup after the trace: nothing is counted as unresolved -- except by an index-slab trace, whose
        // write_pixel counts a hit too deep for the format (SF_SLAB_BAD): that one must leave stats_unknown set so
        // sf_synchronize reads the word and reports SF_EDEPTH (VERDICT/ADVICE r5))
        unresolved_safe = bounded && c->persistent && !(front_first && !tie_inline) && a.packed < SF_PACKED_INDEX;
        if (!(bounded && c->persistent) || (front_first && !tie_inline)) {
            const size_t lds_fix = (size_t)SF_LDS_WAVE_FLOATS(SF_MAX_DEPTH_LIMIT) * 4;
            const uint32_t fb = (bounded && c->persistent) ? 8u : 4u * (uint32_t)c->fixup_blocks;
            hipLaunchKernelGGL(sf_fixup_wave, dim3(fb), dim3(64), lds_fix, s, a,
                               (const uint32_t*)c->ovf_list, c->ovf_counters, c->parity);
            SF_HIP(c, hipGetLastError());
        }
        c->parity ^= 1u;
        // LDS-level hint for later renders: only needed when the geometric bound is unavailable
        if (!bounded) SF_HIP(c, hipMemcpyAsync(c->h_depth, c->stats, 4, hipMemcpyDeviceToHost, s));
    }
    c->rays += (int64_t)sh.rows * c->W;
    if (unresolved_safe) c->stats_unknown = unknown_before;
    return SF_OK;
}

int sf_render(sf_ctx* c, const sf_render_params* p)
{
    if (!c) return SF_EINVAL;
    return launch(c, p, c->pos, c->nrm, c->min_t, c->hit_index);
}

int sf_render_to(sf_ctx* c, const sf_render_params* p, float* pos4, float* nrm4, float* min_t, uint32_t* hidx)
{
    if (p && p->packed && !nrm4) nrm4 = pos4;   // (packed slabs write pos4 only)
    return launch(c, p, pos4, nrm4, min_t, hidx);
}

// ------------------------------------------------------------------------------------------
// The seven list traces (sf.h): sf_trace_dirs_to, sf_trace_rays_to, sf_trace_shadow_to,
// sf_trace_shadows_to, sf_trace_sun_to, sf_trace_suns_to, sf_trace_shafts_to. Each is a one-shot grid, one wave per
// group of 64 rays (an 8x8 tile of an image, or 64 consecutive rays of a list), and a fixup launch behind it that
// re-traces the groups the waves flagged (more levels needed, or a tie under the front-first order). They share one
// re-trace list and its counters (the dirs_* fields; the calls are ordered on the context like any other pair of its
// calls), and read and write none of the renders' state: not the overflow counters' parity, the tile order or costs,
// the depth hint, the timing ring or the frame-less state.
// ------------------------------------------------------------------------------------------

extern "C++" {
// One of list_trace's two launches: the geometry, and the arguments every trace's kernels end in.
struct ListLaunch {
    hipStream_t s;
    uint32_t blocks, groups;
    size_t lds;
    uint32_t* list;       // the re-trace list: the wave kernel appends, the fixup reads
    uint32_t* counters;   // {count of either parity, re-traced groups in all}
    uint32_t parity;      // the wave kernel counts in counters[parity]
    template <class Kernel, class... Args>
    void wave(Kernel kernel, Args... args) const   // kernel(args..., groups, list, count)
    {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64), lds, s, args..., groups, list, counters + parity);
    }
    template <class Kernel, class... Args>
    void fixup(Kernel kernel, Args... args) const   // kernel(args..., list, counters, parity)
    {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64), lds, s, args..., (const uint32_t*)list, counters, parity);
    }
};

// The launch procedure, from validated parameters to SF_OK: order the stream after the context's earlier work, make
// the counters and a list of `groups` entries, launch the wave kernel over `groups` one-wave blocks with `lds` bytes
// and the fixup over at most `fixup_blocks` with `lds_fix`, flip the parity. wave(l) / fixup(l) call l.wave / l.fixup
// with the trace's kernel and its own arguments.
template <class Wave, class Fixup>
static int list_trace(sf_ctx* c, void* stream, uint32_t groups, size_t lds, size_t lds_fix, uint32_t fixup_blocks,
                      Wave wave, Fixup fixup)
{
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    DevGuard g(c->device);
    if (int rc = ctx_join(c, s)) return rc;
    StreamMark mark_(c, s);   // (recorded behind both launches)
    if (!c->dirs_cnt) {
        SF_HIP(c, hipMalloc(&c->dirs_cnt, 3 * 4));
        SF_HIP(c, hipMemsetAsync(c->dirs_cnt, 0, 3 * 4, s));
    }
    if (groups > c->dirs_cap) {   // grown on demand; an earlier trace may still write the old list
        SF_HIP(c, hipStreamSynchronize(s));
        (void)hipFree(c->dirs_ovf);
        c->dirs_ovf = nullptr;
        c->dirs_cap = 0;
        SF_HIP(c, hipMalloc(&c->dirs_ovf, (size_t)groups * 4));
        c->dirs_cap = groups;
    }
    wave(ListLaunch{ s, groups, groups, lds, c->dirs_ovf, c->dirs_cnt, c->dirs_par });
    SF_HIP(c, hipGetLastError());
    fixup(ListLaunch{ s, groups < fixup_blocks ? groups : fixup_blocks, groups, lds_fix, c->dirs_ovf, c->dirs_cnt,
                      c->dirs_par });
    SF_HIP(c, hipGetLastError());
    c->dirs_par ^= 1u;
    return SF_OK;
}
}  // extern "C++"

// The levels a launch provisions: at least 4, at most the LDS limit.
static uint32_t clamp_levels(uint32_t levels)
{
    return levels < 4u ? 4u : levels > SF_MAX_DEPTH_LIMIT ? SF_MAX_DEPTH_LIMIT : levels;
}

// The grouping of width x height caller-supplied rays (sf_trace_dirs_to, sf_trace_rays_to): one row or one column is
// a list of consecutive rays, anything else an image of 8x8 tiles. (groups holds for n < 2^31: the callers check.)
struct RayGroups {
    uint64_t n;
    bool list;
    uint32_t tiles_x, groups;
};
static RayGroups ray_groups(uint32_t width, uint32_t height)
{
    RayGroups r;
    r.n = (uint64_t)width * height;
    r.list = height == 1u || width == 1u;
    r.tiles_x = (width + 7u) / 8u;
    r.groups = r.list ? (uint32_t)((r.n + 63u) / 64u) : r.tiles_x * ((height + 7u) / 8u);
    return r;
}

// The launch's FrameArgs for those rays and output buffers.
static FrameArgs ray_frame_args(const sf_ctx* c, const RayGroups& r, uint32_t width, uint32_t height, uint32_t levels,
                                float* pos4, float* nrm4, float* min_t, uint32_t* hidx)
{
    FrameArgs a = frame_args(c);
    a.W = r.list ? (uint32_t)r.n : width;
    a.H = r.list ? 1u : height;
    a.tiles_x = r.tiles_x;
    a.max_depth = clamp_levels(levels);
    a.emit_aux = 1u;
    a.pos = pos4;
    a.nrm = nrm4;
    a.min_t = min_t;
    a.hit_index = hidx;
    return a;
}

// Caller-supplied directions (kernels sf_trace_dirs_wave / sf_trace_dirs_fixup), at the levels of the geometric bound.
int sf_trace_dirs_to(sf_ctx* c, const sf_dirs_params* p, const float* dirs, float* pos4, float* nrm4, float* min_t,
                     uint32_t* hidx)
{
    if (!c || !p) return SF_EINVAL;
    if (!c->has_view) return SF_ENOVIEW;
    if (p->stride != 3u && p->stride != 4u) return SF_EINVAL;
    if (!dirs || (!pos4 && !nrm4 && !min_t && !hidx)) return SF_EINVAL;
    if (p->max_depth > SF_MAX_DEPTH_LIMIT) return SF_EINVAL;
    const RayGroups r = ray_groups(p->width, p->height);
    if (r.n == 0) return SF_OK;
    if (r.n > 0x7fffffffull) return SF_EINVAL;   // (ray counts are 32-bit in the launch arguments)
    bool bounded = false;
    const uint32_t levels = p->max_depth ? p->max_depth : geometric_levels(c, &bounded);
    const FrameArgs a = ray_frame_args(c, r, p->width, p->height, levels, pos4, nrm4, min_t, hidx);
    const int rc = list_trace(
        c, p->stream, r.groups, (size_t)SF_LDS_WAVE_FLOATS(a.max_depth) * 4,
        (size_t)SF_LDS_WAVE_FLOATS(SF_MAX_DEPTH_LIMIT) * 4, SF_PROG_FIXUP_BLOCKS,
        [&](const ListLaunch& l) { l.wave(sf_trace_dirs_wave, a, dirs, p->stride); },
        [&](const ListLaunch& l) { l.fixup(sf_trace_dirs_fixup, a, dirs, p->stride); });
    if (rc == SF_OK) c->rays += (int64_t)r.n;
    return rc;
}

int sf_trace_dirs(sf_ctx* c, const sf_dirs_params* p, const float* dirs)
{
    if (!c || !p) return SF_EINVAL;
    if (!c->has_view) return SF_ENOVIEW;
    if (p->width != c->W || p->height != c->H) return SF_EINVAL;
    return sf_trace_dirs_to(c, p, dirs, c->pos, c->nrm, c->min_t, c->hit_index);
}

// The probes' device scratch (*buf, *cap rays of `words` floats each, + 3 for alignment), grown on demand.
static int probe_scratch(sf_ctx* c, float** buf, uint32_t* cap, uint32_t n, uint32_t words)
{
    if (n <= *cap) return SF_OK;
    if (int rc = ctx_drain(c)) return rc;   // an earlier probe's trace may still use the old scratch
    (void)hipFree(*buf);
    *buf = nullptr;
    *cap = 0;
    SF_HIP(c, hipMalloc(buf, ((size_t)n * words + 3) * 4));
    *cap = n;
    return SF_OK;
}

// The probes' four output arrays, {pos 4, nrm 4, min_t 1, index 1} words per ray behind `in_words` input words per ray.
struct ProbeOut {
    float *pos, *nrm, *min_t;
    uint32_t* idx;
};
static ProbeOut probe_outputs(float* buf, uint32_t cap, uint32_t in_words)
{
    const size_t in = (size_t)in_words * cap;
    ProbeOut o;
    o.pos = buf + in + (4u - in % 4u) % 4u;   // (16-B aligned)
    o.nrm = o.pos + (size_t)4 * cap;
    o.min_t = o.nrm + (size_t)4 * cap;
    o.idx = reinterpret_cast<uint32_t*>(o.min_t + cap);
    return o;
}

// Wait for the probe's trace and copy out the arrays the caller asked for.
static int probe_download(sf_ctx* c, const ProbeOut& o, uint32_t n, float* min_t, uint32_t* hidx, float* pos4,
                          float* nrm4)
{
    if (int rc = sf_synchronize(c)) return rc;
    if (pos4) SF_HIP(c, hipMemcpy(pos4, o.pos, (size_t)n * 16, hipMemcpyDeviceToHost));
    if (nrm4) SF_HIP(c, hipMemcpy(nrm4, o.nrm, (size_t)n * 16, hipMemcpyDeviceToHost));
    if (min_t) SF_HIP(c, hipMemcpy(min_t, o.min_t, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (hidx) SF_HIP(c, hipMemcpy(hidx, o.idx, (size_t)n * 4, hipMemcpyDeviceToHost));
    return SF_OK;
}

int sf_probe_dirs(sf_ctx* c, const float* dirs3, uint32_t n, float* min_t, uint32_t* hidx, float* pos4, float* nrm4)
{
    if (!c) return SF_EINVAL;
    if (!c->has_view) return SF_ENOVIEW;
    if (!dirs3 || (!pos4 && !nrm4 && !min_t && !hidx)) return SF_EINVAL;
    if (n == 0) return SF_OK;
    if (n > 0x7fffffffu) return SF_EINVAL;
    DevGuard g(c->device);
    if (int rc = probe_scratch(c, &c->probe_buf, &c->probe_cap, n, 13)) return rc;
    float* const d_dirs = c->probe_buf;
    const ProbeOut o = probe_outputs(c->probe_buf, c->probe_cap, 3);
    if (int rc = ctx_join(c, c->stream)) return rc;
    SF_HIP(c, hipMemcpyAsync(d_dirs, dirs3, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    sf_dirs_params p;
    std::memset(&p, 0, sizeof p);
    p.width = n;
    p.height = 1;
    p.stride = 3;
    if (int rc = sf_trace_dirs_to(c, &p, d_dirs, o.pos, o.nrm, o.min_t, o.idx)) return rc;
    return probe_download(c, o, n, min_t, hidx, pos4, nrm4);
}

// Caller-supplied origins and directions (kernels sf_trace_rays_wave / sf_trace_rays_one / sf_trace_rays_fixup). The
// levels are the default, not the view's geometric bound, which speaks of one origin. Where the grouping proves that
// every group of 64 rays has one origin (one origin for all rays, or a list whose rays_per_origin is a multiple of 64)
// the launch leaves out the mixed traversal's per-lane centre stack, which is most of its LDS.
int sf_trace_rays_to(sf_ctx* c, const sf_rays_params* p, const float* origins, const float* dirs, float* pos4,
                     float* nrm4, float* min_t, uint32_t* hidx)
{
    if (!c || !p) return SF_EINVAL;
    if (!c->has_view) return SF_ENOVIEW;
    if (p->dir_stride != 3u && p->dir_stride != 4u) return SF_EINVAL;
    if (p->origin_stride != 3u && p->origin_stride != 4u) return SF_EINVAL;
    if (!origins || !dirs || (!pos4 && !nrm4 && !min_t && !hidx)) return SF_EINVAL;
    if (p->max_depth > SF_MAX_DEPTH_LIMIT) return SF_EINVAL;
    const RayGroups r = ray_groups(p->width, p->height);
    if (r.n == 0) return SF_OK;
    if (r.n > 0x7fffffffull) return SF_EINVAL;   // (ray counts are 32-bit in the launch arguments)
    const uint32_t rpo = p->rays_per_origin ? p->rays_per_origin : 1u;
    const uint32_t levels = p->max_depth ? p->max_depth : kDefaultLevels;
    const FrameArgs a = ray_frame_args(c, r, p->width, p->height, levels, pos4, nrm4, min_t, hidx);
    const bool one_origin_groups = rpo >= r.n || (r.list && rpo % 64u == 0u);
    const uint32_t mixed_ok = (!one_origin_groups || (a.flags & SF_FLAG_FORCE_MIXED)) ? 1u : 0u;
    // (secondary rays go deep: more re-trace blocks than the direction traces', about what the fixup's LDS lets reside)
    const int rc = list_trace(
        c, p->stream, r.groups,
        (size_t)(mixed_ok ? SF_LDS_RAYS_FLOATS(a.max_depth) : SF_LDS_WAVE_FLOATS(a.max_depth)) * 4,
        (size_t)SF_LDS_RAYS_FLOATS(SF_MAX_DEPTH_LIMIT) * 4, kRaysFixupBlocks,
        [&](const ListLaunch& l) {
            if (mixed_ok) l.wave(sf_trace_rays_wave, a, origins, dirs, p->origin_stride, p->dir_stride, rpo, mixed_ok);
            else l.wave(sf_trace_rays_one, a, origins, dirs, p->origin_stride, p->dir_stride, rpo);
        },
        [&](const ListLaunch& l) {
            l.fixup(sf_trace_rays_fixup, a, origins, dirs, p->origin_stride, p->dir_stride, rpo);
        });
    if (rc == SF_OK) c->rays += (int64_t)r.n;
    return rc;
}

int sf_probe_rays(sf_ctx* c, const float* origins3, const float* dirs3, uint32_t n, uint32_t rays_per_origin,
                  float* min_t, uint32_t* hidx, float* pos4, float* nrm4)
{
    if (!c) return SF_EINVAL;
    if (!c->has_view) return SF_ENOVIEW;
    if (!origins3 || !dirs3 || (!pos4 && !nrm4 && !min_t && !hidx)) return SF_EINVAL;
    if (n == 0) return SF_OK;
    if (n > 0x7fffffffu) return SF_EINVAL;
    const uint32_t rpo = rays_per_origin ? rays_per_origin : 1u;
    const uint32_t norig = (n + rpo - 1u) / rpo;
    DevGuard g(c->device);
    // {dirs 3, origins 3 (at most one per ray), pos 4, nrm 4, min_t 1, index 1} words per ray
    if (int rc = probe_scratch(c, &c->rprobe_buf, &c->rprobe_cap, n, 16)) return rc;
    float* const d_dirs = c->rprobe_buf;
    float* const d_org = d_dirs + (size_t)3 * c->rprobe_cap;
    const ProbeOut o = probe_outputs(c->rprobe_buf, c->rprobe_cap, 6);
    if (int rc = ctx_join(c, c->stream)) return rc;
    SF_HIP(c, hipMemcpyAsync(d_dirs, dirs3, (size_t)n * 12, hipMemcpyHostToDevice, c->stream));
    SF_HIP(c, hipMemcpyAsync(d_org, origins3, (size_t)norig * 12, hipMemcpyHostToDevice, c->stream));
    sf_rays_params p;
    std::memset(&p, 0, sizeof p);
    p.width = n;
    p.height = 1;
    p.dir_stride = 3;
    p.origin_stride = 3;
    p.rays_per_origin = rpo;
    if (int rc = sf_trace_rays_to(c, &p, d_org, d_dirs, o.pos, o.nrm, o.min_t, o.idx)) return rc;
    return probe_download(c, o, n, min_t, hidx, pos4, nrm4);
}

// ---- what the light traces share (sf_trace_shadow_to, sf_trace_shadows_to, sf_trace_sun_to, sf_trace_suns_to,
// sf_trace_shafts_to, the summing traces and the AO pair): one wave per 8x8 tile of a position image,
// the shadow traces' own constant block (sf_set_shadow_lod); they touch no statistic (not the stats words, not the ray
// count). The image and its FrameArgs, the checks and fillers of a list of entries, the two launch shapes, the
// context's own buffers and the one-thread-per-pixel pass.

// The position image of a shadow trace: width and height 0 mean the context's size, a null pos4 the context's own
// G-buffer (at its size only). Checks bias and max_depth with them; every failure here is SF_EINVAL.
struct ShadowImage {
    uint32_t W, H, tiles_x, groups;
    const float* pos4;
};
static int shadow_image(const sf_ctx* c, float bias, uint32_t max_depth, uint32_t width, uint32_t height,
                        const float* pos4, ShadowImage* im)
{
    if (!(bias >= 0.0f && bias < 1.0f)) return SF_EINVAL;   // (NaN fails both)
    if (max_depth > SF_MAX_DEPTH_LIMIT) return SF_EINVAL;
    if ((width == 0u) != (height == 0u)) return SF_EINVAL;
    im->W = width ? width : c->W;
    im->H = height ? height : c->H;
    if (!pos4 && (im->W != c->W || im->H != c->H)) return SF_EINVAL;
    if ((uint64_t)im->W * im->H > 0x7fffffffull) return SF_EINVAL;   // (pixel indices are 32-bit in the kernel)
    im->pos4 = pos4 ? pos4 : c->pos;
    im->tiles_x = (im->W + 7u) / 8u;
    im->groups = im->tiles_x * ((im->H + 7u) / 8u);
    return SF_OK;
}

// The launch's FrameArgs for that image; the caller sets the root translation and the levels.
static FrameArgs shadow_frame_args(const sf_ctx* c, const ShadowImage& im)
{
    FrameArgs a = frame_args(c);
    a.W = im.W;
    a.H = im.H;
    a.tiles_x = im.tiles_x;
    a.consts = c->shadow_consts;   // (sf_set_shadow_lod)
    a.stats = nullptr;   // (no statistic is touched)
    return a;
}

// The origin the position image is relative to, and 1 - bias.
static void shadow_origin(const sf_ctx* c, uint32_t use_origin, const float origin[3], float bias, float o[3],
                          float* keep)
{
    for (int k = 0; k < 3; ++k) o[k] = use_origin ? origin[k] : c->o[k];
    *keep = 1.0f - bias;
}

// What every trace checks before anything else: the context and the parameters, the view, and, where the result goes
// to the caller's buffer only, that buffer.
static int trace_preamble(const sf_ctx* c, bool params, bool out = true)
{
    if (!c || !params) return SF_EINVAL;
    if (!c->has_view) return SF_ENOVIEW;
    return out ? SF_OK : SF_EINVAL;
}

// a colour component: finite and not negative (NaN fails the compare)
static bool light_component(float v) { return v >= 0.0f && !std::isinf(v); }

// What every trace of a list of entries (lights, directions, march fractions, samples) checks of the list: n in
// 1..max and the entries' pointer; then the optional `count` values beside them -- colour components, or weights, which
// are not negative (NaN fails the compare) and may be infinite.
static int entries_check(uint32_t n, uint32_t max, const float* entries, const float* values, uint32_t count,
                         bool colours)
{
    if (n == 0u || n > max || !entries) return SF_EINVAL;
    if (values)
        for (uint32_t i = 0; i < count; ++i)
            if (colours ? !light_component(values[i]) : !(values[i] >= 0.0f)) return SF_EINVAL;
    return SF_OK;
}

// An argument block's triples from the caller's host array (read here, before the call returns): as given, and where
// the block has them, times `scale` (one rounding: step 2 of sf_trace_sun_to's definition).
static void entry_triples(uint32_t n, const float* src, float (*given)[3], float (*scaled)[3] = nullptr,
                          float scale = 0.0f)
{
    for (uint32_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) {
            given[i][k] = src[3 * i + k];
            if (scaled) scaled[i][k] = src[3 * i + k] * scale;
        }
}

// Its weights or colour components: the caller's, or `even` each.
static void entry_values(uint32_t count, const float* src, float even, float* dst)
{
    for (uint32_t i = 0; i < count; ++i) dst[i] = src ? src[i] : even;
}

// The levels of a launch over point lights, one value for all of them: max_depth where given, else the largest
// geometric bound over the finite lights (one that is not finite traces nothing).
static uint32_t light_levels(const sf_ctx* c, uint32_t max_depth, const float (*l)[3], uint32_t n)
{
    uint32_t levels = max_depth;
    if (!levels)
        for (uint32_t i = 0; i < n; ++i) {
            const float centre[3] = { 0.0f - l[i][0], 0.0f - l[i][1], 0.0f - l[i][2] };
            if (!std::isfinite(centre[0] + centre[1] + centre[2])) continue;
            bool bounded = false;
            const uint32_t li = geometric_levels(c->host_shadow_consts.dt, centre, &bounded);
            if (li > levels) levels = li;
        }
    return levels;
}

extern "C++" {
// The head of an argument block of entries: zeroed, then the origin, 1 - bias and n.
template <class Args>
static void entry_args(const sf_ctx* c, uint32_t use_origin, const float origin[3], float bias, uint32_t n, Args* x)
{
    std::memset(x, 0, sizeof *x);
    shadow_origin(c, use_origin, origin, bias, x->o, &x->keep);
    x->n = n;
}

// The two launches of the light traces over the tiles of `im`: wave(a, im.pos4, args...) and fixup(a, im.pos4, args...).
// Rays from one point per entry (traverse_ray): the root translation 0 - that point, or 0 where the kernel stages each
// entry's own; the levels are the caller's bound.
template <class Wave, class Fixup, class... Args>
static int fixed_origin_trace(sf_ctx* c, void* stream, const ShadowImage& im, const float centre[3], uint32_t levels,
                              Wave wave, Fixup fixup, Args... args)
{
    FrameArgs a = shadow_frame_args(c, im);
    for (int k = 0; k < 3; ++k) a.root[9 + k] = centre[k];
    a.max_depth = clamp_levels(levels);
    return list_trace(
        c, stream, im.groups, (size_t)SF_LDS_WAVE_FLOATS(a.max_depth) * 4,
        (size_t)SF_LDS_WAVE_FLOATS(SF_MAX_DEPTH_LIMIT) * 4, SF_PROG_FIXUP_BLOCKS,
        [&](const ListLaunch& l) { l.wave(wave, a, im.pos4, args...); },
        [&](const ListLaunch& l) { l.fixup(fixup, a, im.pos4, args...); });
}

// Rays with an origin per lane (traverse_mixed): the context's own root columns, the default levels of
// sf_trace_rays_to, the mixed traversal's LDS and sf_trace_rays_to's fixup grid.
template <class Wave, class Fixup, class... Args>
static int mixed_origin_trace(sf_ctx* c, void* stream, const ShadowImage& im, uint32_t max_depth, Wave wave,
                              Fixup fixup, Args... args)
{
    FrameArgs a = shadow_frame_args(c, im);
    a.max_depth = clamp_levels(max_depth ? max_depth : kDefaultLevels);
    return list_trace(
        c, stream, im.groups, (size_t)SF_LDS_RAYS_FLOATS(a.max_depth) * 4,
        (size_t)SF_LDS_RAYS_FLOATS(SF_MAX_DEPTH_LIMIT) * 4, kRaysFixupBlocks,
        [&](const ListLaunch& l) { l.wave(wave, a, im.pos4, args...); },
        [&](const ListLaunch& l) { l.fixup(fixup, a, im.pos4, args...); });
}

// The calls into the context's own result buffer (*buf, W x H elements, allocated on first use).
template <class T>
static int own_result_buffer(sf_ctx* c, uint32_t width, uint32_t height, T** buf)
{
    if (!c->has_view) return SF_ENOVIEW;
    if ((width || height) && (width != c->W || height != c->H)) return SF_EINVAL;
    if (!*buf) {
        DevGuard g(c->device);
        SF_HIP(c, hipMalloc(buf, (size_t)c->W * c->H * sizeof(T)));
    }
    return SF_OK;
}

// The same for the calls that come with a check of their own (check(): the trace's parameters against the context's
// images): where the buffer (`bytes` per pixel) is yet to be made, the parameters' errors come before the buffer's
// state, and an accumulating call needs it written.
template <class T, class Check>
static int own_buffer_checked(sf_ctx* c, T** buf, size_t bytes, bool accumulate, Check check)
{
    if (*buf) return SF_OK;
    if (int rc = check()) return rc;
    if (accumulate) return SF_ESTATE;
    DevGuard g(c->device);
    SF_HIP(c, hipMalloc(buf, (size_t)c->W * c->H * bytes));
    return SF_OK;
}

// The own-buffer form of a trace whose `_to` form does all its checks: the context's G-buffer into c->*buf.
template <class P, class T>
static int trace_own(sf_ctx* c, const P* p, T* sf_ctx::*buf, int (*to)(sf_ctx*, const P*, const float*, T*))
{
    if (!c || !p) return SF_EINVAL;
    if (int rc = own_result_buffer(c, p->width, p->height, &(c->*buf))) return rc;
    return to(c, p, nullptr, c->*buf);
}

// The context's own buffer c->*buf (`bytes` per pixel) to the host, after everything queued on the context.
template <class T>
static int download_own(sf_ctx* c, T* sf_ctx::*buf, size_t bytes, T* host)
{
    if (!c || !host) return SF_EINVAL;
    if (!(c->*buf)) return SF_ESTATE;
    if (int rc = sf_synchronize(c)) return rc;
    DevGuard g(c->device);
    SF_HIP(c, hipMemcpy(host, c->*buf, (size_t)c->W * c->H * bytes, hipMemcpyDeviceToHost));
    return SF_OK;
}

// Its device pointer: null before the first use, which is SF_ESTATE where the buffer is `required`.
template <class T>
static int own_buffer_pointer(sf_ctx* c, T* sf_ctx::*buf, bool required, T** out)
{
    if (!c || !out) return SF_EINVAL;
    if (required && !(c->*buf)) return SF_ESTATE;
    *out = c->*buf;
    return SF_OK;
}

// One thread per pixel of an image of `pixels` pixels: kernel(args...) on `stream` (null: the context's), ordered after
// the context's earlier work.
template <class Kernel, class... Args>
static int pixel_pass_of(sf_ctx* c, void* stream, size_t pixels, Kernel kernel, Args... args)
{
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    DevGuard g(c->device);
    if (int rc = ctx_join(c, s)) return rc;
    StreamMark mark_(c, s);
    const dim3 grid((unsigned)((pixels + 255u) / 256u));
    if (grid.x == 0u) return SF_OK;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, args...);
    SF_HIP(c, hipGetLastError());
    return SF_OK;
}

// The same for the context's own frame.
template <class Kernel, class... Args>
static int pixel_pass(sf_ctx* c, void* stream, Kernel kernel, Args... args)
{
    return pixel_pass_of(c, stream, (size_t)c->W * c->H, kernel, args...);
}

// The lighting passes that shade by a normal: kernel(W, H, pos4, nrm4, mid..., ambient, rgba), the buffers defaulted to
// the context's. have_vis: there is a visibility buffer to read.
template <class Kernel, class... Mid>
static int light_image_pass(sf_ctx* c, void* stream, float ambient, const float* pos4, const float* nrm4, bool have_vis,
                            uint8_t* rgba, Kernel kernel, Mid... mid)
{
    if (!(ambient >= 0.0f && ambient <= 1.0f)) return SF_EINVAL;
    if (!rgba && !c->image) return SF_ESTATE;
    if (!have_vis) return SF_ESTATE;
    return pixel_pass(c, stream, kernel, c->W, c->H, pos4 ? pos4 : (const float*)c->pos,
                      nrm4 ? nrm4 : (const float*)c->nrm, mid..., ambient, rgba ? rgba : c->image);
}
}  // extern "C++"

// Shadows from a point light (kernels sf_trace_shadow_wave / sf_trace_shadow_fixup), with the root
// transform of the LIGHT (the context's columns, translation 0 - light) and the levels of the light's geometric bound.
int sf_shadow_defaults(const sf_ctx* c, sf_shadow_params* p)
{
    if (!c || !p) return SF_EINVAL;
    std::memset(p, 0, sizeof *p);
    p->bias = kShadowBias;
    return SF_OK;
}

// the launch's ShadowArgs from the parameters (the origin the position image is relative to, the light)
static ShadowArgs shadow_args(const sf_ctx* c, const sf_shadow_params* p)
{
    ShadowArgs sa;
    shadow_origin(c, p->use_origin, p->origin, p->bias, sa.o, &sa.keep);
    for (int k = 0; k < 3; ++k) sa.l[k] = p->light[k];
    return sa;
}

int sf_trace_shadow_to(sf_ctx* c, const sf_shadow_params* p, const float* pos4, uint8_t* vis)
{
    if (int rc = trace_preamble(c, p != nullptr, vis != nullptr)) return rc;
    ShadowImage im;
    if (int rc = shadow_image(c, p->bias, p->max_depth, p->width, p->height, pos4, &im)) return rc;
    const ShadowArgs sa = shadow_args(c, p);
    const float centre[3] = { 0.0f - sa.l[0], 0.0f - sa.l[1], 0.0f - sa.l[2] };   // (Sphereflake.cpp:83 at the light)
    bool bounded = false;
    const uint32_t levels =
        p->max_depth ? p->max_depth : geometric_levels(c->host_shadow_consts.dt, centre, &bounded);
    return fixed_origin_trace(c, p->stream, im, centre, levels, sf_trace_shadow_wave, sf_trace_shadow_fixup, sa, vis);
}

int sf_trace_shadow(sf_ctx* c, const sf_shadow_params* p)
{
    return trace_own(c, p, &sf_ctx::shadow, sf_trace_shadow_to);
}

int sf_download_shadow(sf_ctx* c, uint8_t* vis) { return download_own(c, &sf_ctx::shadow, 1, vis); }

int sf_shadow_buffer(sf_ctx* c, uint8_t** vis) { return own_buffer_pointer(c, &sf_ctx::shadow, false, vis); }

int sf_light_image(sf_ctx* c, const sf_shadow_params* p, float ambient, const float* pos4, const float* nrm4,
                   const uint8_t* vis, uint8_t* rgba)
{
    if (!c || !p) return SF_EINVAL;
    if (!c->has_view && !p->use_origin) return SF_ENOVIEW;
    return light_image_pass(c, p->stream, ambient, pos4, nrm4, vis || c->shadow, rgba, sf_light_image_px,
                            vis ? vis : (const uint8_t*)c->shadow, shadow_args(c, p));
}

// Many lights per pixel in one launch (kernels sf_trace_shadows_wave / sf_trace_shadows_fixup / sf_light_image_many_px,
// DESIGN.md §6.12). The launch of sf_trace_shadow_to with the lights by value in the argument segment; the levels are
// one value for the launch, the largest geometric bound over the lights.
static_assert(SF_SHADOW_LIGHTS == SF_SHADOW_LIGHTS_MAX, "one mask bit per light");
static_assert(sizeof(FrameArgs) + sizeof(ShadowLights) + 64 <= 4096, "kernel argument segment");

int sf_shadows_defaults(const sf_ctx* c, sf_shadows_params* p)
{
    if (!c || !p) return SF_EINVAL;
    std::memset(p, 0, sizeof *p);
    p->bias = kShadowBias;
    return SF_OK;
}

// the launch's ShadowLights from the parameters (the weights: sf_light_image_many's)
static void shadows_args(const sf_ctx* c, const sf_shadows_params* p, ShadowLights* sl)
{
    entry_args(c, p->use_origin, p->origin, p->bias, p->n, sl);
    entry_triples(p->n, p->lights, sl->l);
    entry_values(p->n, p->weights, 1.0f / (float)p->n, sl->w);
}

static const float kNoCentre[3] = { 0.0f, 0.0f, 0.0f };   // (the kernel stages each light's own translation)

int sf_trace_shadows_to(sf_ctx* c, const sf_shadows_params* p, const float* pos4, uint64_t* mask)
{
    if (int rc = trace_preamble(c, p != nullptr, mask != nullptr)) return rc;
    if (int rc = entries_check(p->n, SF_SHADOW_LIGHTS_MAX, p->lights, nullptr, 0u, false)) return rc;
    ShadowImage im;
    if (int rc = shadow_image(c, p->bias, p->max_depth, p->width, p->height, pos4, &im)) return rc;
    ShadowLights sl;
    shadows_args(c, p, &sl);
    return fixed_origin_trace(c, p->stream, im, kNoCentre, light_levels(c, p->max_depth, sl.l, sl.n),
                              sf_trace_shadows_wave, sf_trace_shadows_fixup, sl, mask);
}

int sf_trace_shadows(sf_ctx* c, const sf_shadows_params* p)
{
    return trace_own(c, p, &sf_ctx::shadow_masks, sf_trace_shadows_to);
}

int sf_download_shadow_masks(sf_ctx* c, uint64_t* mask) { return download_own(c, &sf_ctx::shadow_masks, 8, mask); }

int sf_shadow_mask_buffer(sf_ctx* c, uint64_t** mask)
{
    return own_buffer_pointer(c, &sf_ctx::shadow_masks, false, mask);
}

int sf_light_image_many(sf_ctx* c, const sf_shadows_params* p, float ambient, const float* pos4, const float* nrm4,
                        const uint64_t* mask, uint8_t* rgba)
{
    if (!c || !p) return SF_EINVAL;
    if (!c->has_view && !p->use_origin) return SF_ENOVIEW;
    if (int rc = entries_check(p->n, SF_SHADOW_LIGHTS_MAX, p->lights, p->weights, p->n, false)) return rc;
    ShadowLights sl;
    shadows_args(c, p, &sl);
    return light_image_pass(c, p->stream, ambient, pos4, nrm4, mask || c->shadow_masks, rgba, sf_light_image_many_px,
                            mask ? mask : (const uint64_t*)c->shadow_masks, sl);
}

// The LOD constant of the shadow traces (sf.h): a second constant block, the context's own but for the
// depth tables, which sf_trace_shadow_to, sf_trace_shadows_to, sf_trace_sun_to, sf_trace_suns_to and
// sf_trace_shafts_to hand their kernels. No kernel knows.
int sf_set_shadow_lod(sf_ctx* c, float lod_constant)
{
    if (!c || !(lod_constant >= 0.0f) || std::isinf(lod_constant)) return SF_EINVAL;   // (NaN fails the compare)
    if (lod_constant == c->shadow_lod) return SF_OK;
    DevGuard g(c->device);
    const float before = c->shadow_lod;
    c->shadow_lod = lod_constant;
    const int rc = upload_shadow_consts(c);
    if (rc != SF_OK) c->shadow_lod = before;
    return rc;
}

float sf_get_shadow_lod(const sf_ctx* c) { return c ? c->shadow_lod : NAN; }

// Shadows from a directional light (kernels sf_trace_sun_wave / sf_trace_sun_fixup / sf_light_image_sun_px, DESIGN.md
// §6.13), with the context's own root columns (each lane forms its own translation), the default levels of
// sf_trace_rays_to, the mixed traversal's LDS and sf_trace_rays_to's fixup grid.
int sf_sun_defaults(const sf_ctx* c, sf_sun_params* p)
{
    if (!c || !p) return SF_EINVAL;
    std::memset(p, 0, sizeof *p);
    p->dir[2] = 1.0f;
    p->distance = 4.0f;
    p->bias = kShadowBias;
    return SF_OK;
}

int sf_trace_sun_to(sf_ctx* c, const sf_sun_params* p, const float* pos4, uint8_t* vis)
{
    if (int rc = trace_preamble(c, p != nullptr, vis != nullptr)) return rc;
    if (!(p->distance > 0.0f) || std::isinf(p->distance)) return SF_EINVAL;   // (NaN fails the compare)
    ShadowImage im;   // (its checks fail with SF_EINVAL as the distance does: their order cannot be told)
    if (int rc = shadow_image(c, p->bias, p->max_depth, p->width, p->height, pos4, &im)) return rc;
    SunArgs sa;
    shadow_origin(c, p->use_origin, p->origin, p->bias, sa.o, &sa.keep);
    for (int k = 0; k < 3; ++k) sa.f[k] = p->dir[k] * p->distance;   // (one rounding: step 2 of the definition)
    return mixed_origin_trace(c, p->stream, im, p->max_depth, sf_trace_sun_wave, sf_trace_sun_fixup, sa, vis);
}

int sf_trace_sun(sf_ctx* c, const sf_sun_params* p) { return trace_own(c, p, &sf_ctx::shadow, sf_trace_sun_to); }

int sf_light_image_sun(sf_ctx* c, const sf_sun_params* p, float ambient, const float* pos4, const float* nrm4,
                       const uint8_t* vis, uint8_t* rgba)
{
    if (!c || !p) return SF_EINVAL;
    return light_image_pass(c, p->stream, ambient, pos4, nrm4, vis || c->shadow, rgba, sf_light_image_sun_px,
                            vis ? vis : (const uint8_t*)c->shadow, p->dir[0], p->dir[1], p->dir[2]);
}

// Many sun directions per pixel in one launch (kernels sf_trace_suns_wave / sf_trace_suns_fixup /
// sf_light_image_suns_px). The launch of sf_trace_sun_to with the directions by value in the argument
// segment; the mask buffer is sf_trace_shadows'.
static_assert(SF_SUN_DIRS == SF_SUN_DIRS_MAX, "one mask bit per direction");
static_assert(sizeof(FrameArgs) + sizeof(SunDirs) + 64 <= 4096, "kernel argument segment");

int sf_suns_defaults(const sf_ctx* c, sf_suns_params* p)
{
    if (!c || !p) return SF_EINVAL;
    std::memset(p, 0, sizeof *p);
    p->distance = 4.0f;
    p->bias = kShadowBias;
    return SF_OK;
}

// the launch's SunDirs from the parameters (the directions as given and the weights: sf_light_image_suns's)
static void suns_args(const sf_ctx* c, const sf_suns_params* p, SunDirs* sd)
{
    entry_args(c, p->use_origin, p->origin, p->bias, p->n, sd);
    entry_triples(p->n, p->dirs, sd->s, sd->f, p->distance);
    entry_values(p->n, p->weights, 1.0f / (float)p->n, sd->w);
}

int sf_trace_suns_to(sf_ctx* c, const sf_suns_params* p, const float* pos4, uint64_t* mask)
{
    if (int rc = trace_preamble(c, p != nullptr, mask != nullptr)) return rc;
    if (int rc = entries_check(p->n, SF_SUN_DIRS_MAX, p->dirs, nullptr, 0u, false)) return rc;
    if (!(p->distance > 0.0f) || std::isinf(p->distance)) return SF_EINVAL;   // (NaN fails the compare)
    ShadowImage im;
    if (int rc = shadow_image(c, p->bias, p->max_depth, p->width, p->height, pos4, &im)) return rc;
    SunDirs sd;
    suns_args(c, p, &sd);
    return mixed_origin_trace(c, p->stream, im, p->max_depth, sf_trace_suns_wave, sf_trace_suns_fixup, sd, mask);
}

int sf_trace_suns(sf_ctx* c, const sf_suns_params* p)
{
    return trace_own(c, p, &sf_ctx::shadow_masks, sf_trace_suns_to);
}

int sf_light_image_suns(sf_ctx* c, const sf_suns_params* p, float ambient, const float* pos4, const float* nrm4,
                        const uint64_t* mask, uint8_t* rgba)
{
    if (!c || !p) return SF_EINVAL;
    if (int rc = entries_check(p->n, SF_SUN_DIRS_MAX, p->dirs, p->weights, p->n, false)) return rc;
    SunDirs sd;
    suns_args(c, p, &sd);
    return light_image_pass(c, p->stream, ambient, pos4, nrm4, mask || c->shadow_masks, rgba, sf_light_image_suns_px,
                            mask ? mask : (const uint64_t*)c->shadow_masks, sd);
}

// Light shafts: sun visibility along each pixel's view ray in one launch (kernels sf_trace_shafts_wave /
// sf_trace_shafts_fixup / sf_light_image_shafts_px). The launch of sf_trace_suns_to with the march
// fractions by value in the argument segment; the mask buffer is sf_trace_shadows'.
static_assert(SF_SHAFT_SAMPLES == SF_SHAFT_SAMPLES_MAX, "one mask bit per sample");
static_assert(sizeof(FrameArgs) + sizeof(ShaftArgs) + 64 <= 4096, "kernel argument segment");

int sf_shafts_defaults(const sf_ctx* c, sf_shafts_params* p)
{
    if (!c || !p) return SF_EINVAL;
    std::memset(p, 0, sizeof *p);
    p->dir[2] = 1.0f;
    p->distance = 4.0f;
    p->bias = kShadowBias;
    return SF_OK;
}

// n, the fractions, far and the direction image's stride (both calls), the weights (sf_light_image_shafts): the list
// first, as everywhere, then what is shafts' own; every failure is SF_EINVAL, so the order shows in no return code
static int shafts_check(const sf_shafts_params* p, bool weights)
{
    if (int rc = entries_check(p->n, SF_SHAFT_SAMPLES_MAX, p->fractions, weights ? p->weights : nullptr, p->n, false))
        return rc;
    for (uint32_t i = 0; i < p->n; ++i)
        if (!(p->fractions[i] > 0.0f) || std::isinf(p->fractions[i])) return SF_EINVAL;   // (NaN fails the compare)
    if (!(p->far >= 0.0f) || std::isinf(p->far)) return SF_EINVAL;
    if (p->dirs && p->dirs_stride != 3u && p->dirs_stride != 4u) return SF_EINVAL;
    return SF_OK;
}

// the launch's ShaftArgs from the parameters (the weights: sf_light_image_shafts's)
static void shafts_args(const sf_ctx* c, const sf_shafts_params* p, ShaftArgs* sh)
{
    entry_args(c, p->use_origin, p->origin, p->bias, p->n, sh);
    for (int k = 0; k < 3; ++k) sh->f[k] = p->dir[k] * p->distance;   // (one rounding: step 2 of sf_trace_sun_to's)
    if (p->dirs && p->far > 0.0f) {   // (else a miss of the frame is not marched: the kernels never look)
        sh->dirs = p->dirs;
        sh->dirs_stride = p->dirs_stride;
        sh->far = p->far;
    }
    for (uint32_t i = 0; i < p->n; ++i) sh->sigma[i] = p->fractions[i];
    entry_values(p->n, p->weights, 1.0f / (float)p->n, sh->w);
}

int sf_trace_shafts_to(sf_ctx* c, const sf_shafts_params* p, const float* pos4, uint64_t* mask)
{
    if (int rc = trace_preamble(c, p != nullptr, mask != nullptr)) return rc;
    if (int rc = shafts_check(p, false)) return rc;
    if (!(p->distance > 0.0f) || std::isinf(p->distance)) return SF_EINVAL;   // (NaN fails the compare)
    ShadowImage im;
    if (int rc = shadow_image(c, p->bias, p->max_depth, p->width, p->height, pos4, &im)) return rc;
    ShaftArgs sh;
    shafts_args(c, p, &sh);
    return mixed_origin_trace(c, p->stream, im, p->max_depth, sf_trace_shafts_wave, sf_trace_shafts_fixup, sh, mask);
}

int sf_trace_shafts(sf_ctx* c, const sf_shafts_params* p)
{
    return trace_own(c, p, &sf_ctx::shadow_masks, sf_trace_shafts_to);
}

// The buffers defaulted to the context's (as light_image_pass, without a normal image or an ambient term).
int sf_light_image_shafts(sf_ctx* c, const sf_shafts_params* p, float gain, const float colour[3], const float* pos4,
                          const uint64_t* mask, uint8_t* rgba)
{
    if (!c || !p || !colour) return SF_EINVAL;
    if (int rc = shafts_check(p, true)) return rc;
    if (!(gain >= 0.0f) || std::isinf(gain)) return SF_EINVAL;   // (NaN fails the compare)
    for (int k = 0; k < 3; ++k)
        if (!(colour[k] >= 0.0f && colour[k] <= 255.0f)) return SF_EINVAL;
    if (!rgba && !c->image) return SF_ESTATE;
    if (!mask && !c->shadow_masks) return SF_ESTATE;
    ShaftArgs sh;
    shafts_args(c, p, &sh);
    return pixel_pass(c, p->stream, sf_light_image_shafts_px, c->W, c->H, pos4 ? pos4 : (const float*)c->pos,
                      mask ? mask : (const uint64_t*)c->shadow_masks, sh, gain, colour[0], colour[1], colour[2],
                      rgba ? rgba : c->image);
}

// The colour light buffer and the traces that add into it (kernels sf_trace_suns_sum_wave / _fixup,
// sf_trace_shadows_sum_wave / _fixup, sf_light_fill_px, sf_light_image_buffer_px). The launches of
// sf_trace_suns_to / sf_trace_shadows_to, once per chunk of SF_LIGHT_SUM_CHUNK entries: the first chunk with the
// caller's accumulate, the rest accumulating, all on one stream.
static_assert(sizeof(FrameArgs) + sizeof(SunSum) + 64 <= 4096, "kernel argument segment");
static_assert(sizeof(FrameArgs) + sizeof(ShadowSum) + 64 <= 4096, "kernel argument segment");

int sf_light_sum_defaults(const sf_ctx* c, sf_light_sum_params* p)
{
    if (!c || !p) return SF_EINVAL;
    std::memset(p, 0, sizeof *p);
    p->distance = 4.0f;
    p->bias = kShadowBias;
    return SF_OK;
}

// Everything both summing traces check, in one place; the images' sizes come back in `im`.
static int light_sum_check(const sf_ctx* c, const sf_light_sum_params* p, bool suns, const float* pos4,
                           bool ctx_buffer, ShadowImage* im)
{
    if (int rc = entries_check(p->n, SF_LIGHT_SUM_MAX, p->points, p->colours, 3u * p->n, true)) return rc;
    if (suns && (!(p->distance > 0.0f) || std::isinf(p->distance))) return SF_EINVAL;   // (NaN fails the compare)
    if (int rc = shadow_image(c, p->bias, p->max_depth, p->width, p->height, pos4, im)) return rc;
    if (ctx_buffer && (im->W != c->W || im->H != c->H)) return SF_EINVAL;   // (a context buffer, at its size only)
    return SF_OK;
}

static int trace_sum_to(sf_ctx* c, const sf_light_sum_params* p, bool suns, const float* pos4, const float* nrm4,
                        float* out)
{
    if (int rc = trace_preamble(c, p != nullptr)) return rc;
    ShadowImage im;
    if (int rc = light_sum_check(c, p, suns, pos4, !nrm4 || !out, &im)) return rc;
    if (!out && !c->light) return SF_ESTATE;
    float* const dst = out ? out : c->light;
    const float* const nrm = nrm4 ? nrm4 : (const float*)c->nrm;
    const float even = 1.0f / (float)p->n;
    for (uint32_t first = 0; first < p->n; first += SF_LIGHT_SUM_CHUNK) {
        const uint32_t m = p->n - first < SF_LIGHT_SUM_CHUNK ? p->n - first : SF_LIGHT_SUM_CHUNK;
        const uint32_t accumulate = (first || p->accumulate) ? 1u : 0u;
        const float* const pts = p->points + (size_t)3 * first;
        const float* const col = p->colours ? p->colours + (size_t)3 * first : nullptr;
        int rc;
        if (suns) {
            SunSum ss;
            entry_args(c, p->use_origin, p->origin, p->bias, m, &ss);
            ss.accumulate = accumulate;
            entry_triples(m, pts, ss.s, ss.f, p->distance);
            entry_values(3u * m, col, even, &ss.c[0][0]);
            rc = mixed_origin_trace(c, p->stream, im, p->max_depth, sf_trace_suns_sum_wave, sf_trace_suns_sum_fixup,
                                    nrm, ss, dst);
        } else {   // (the levels: the largest geometric bound over the chunk, as sf_trace_shadows_to)
            ShadowSum ss;
            entry_args(c, p->use_origin, p->origin, p->bias, m, &ss);
            ss.accumulate = accumulate;
            entry_triples(m, pts, ss.l);
            entry_values(3u * m, col, even, &ss.c[0][0]);
            rc = fixed_origin_trace(c, p->stream, im, kNoCentre, light_levels(c, p->max_depth, ss.l, m),
                                    sf_trace_shadows_sum_wave, sf_trace_shadows_sum_fixup, nrm, ss, dst);
        }
        if (rc != SF_OK) return rc;
    }
    return SF_OK;
}

// The context's G-buffer into the context's light buffer: an overwriting call makes the buffer, an accumulating one
// needs it written.
static int trace_sum_own(sf_ctx* c, const sf_light_sum_params* p, bool suns)
{
    if (int rc = trace_preamble(c, p != nullptr)) return rc;
    ShadowImage im;
    if (int rc = own_buffer_checked(c, &c->light, 16, p->accumulate != 0u,
                                    [&] { return light_sum_check(c, p, suns, nullptr, true, &im); }))
        return rc;
    return trace_sum_to(c, p, suns, nullptr, nullptr, nullptr);
}

int sf_trace_suns_sum_to(sf_ctx* c, const sf_light_sum_params* p, const float* pos4, const float* nrm4, float* out)
{
    return trace_sum_to(c, p, true, pos4, nrm4, out);
}

int sf_trace_suns_sum(sf_ctx* c, const sf_light_sum_params* p) { return trace_sum_own(c, p, true); }

int sf_trace_shadows_sum_to(sf_ctx* c, const sf_light_sum_params* p, const float* pos4, const float* nrm4, float* out)
{
    return trace_sum_to(c, p, false, pos4, nrm4, out);
}

int sf_trace_shadows_sum(sf_ctx* c, const sf_light_sum_params* p) { return trace_sum_own(c, p, false); }

// The lobe traces: rays about a direction of each pixel's own, laid out from local-frame samples that travel by value in
// the argument segment, with the normal image beside the position image. Ambient
// occlusion about the normal (kernels sf_trace_ao_wave / _fixup, sf_trace_ao_sum_wave / _fixup), the same with a
// per-pixel spin (sf_trace_ao_spin_wave / _fixup, sf_trace_ao_spin_sum_wave / _fixup: the table by value beside the
// samples) and sky reflections about the mirror direction (sf_trace_mirror_wave / _fixup, sf_trace_mirror_sum_wave /
// _fixup: the eye and the sky's gradient beside the samples; a null spin travels as the 1 x 1 table {(1, 0)}, which is
// the unspun definition bit for bit, sf.h). The launches are sf_trace_suns_to's and sf_trace_suns_sum_to's; the mask
// buffer is sf_trace_shadows', the light buffer sf_trace_suns_sum's. Twelve entry points, one host path: lobe_to and
// lobe_own over a LobeCall. The argument blocks stay what the kernels were compiled for, under the 4 KB limit:
static_assert(SF_AO_SAMPLES == SF_AO_SAMPLES_MAX, "one mask bit per sample");
static_assert(SF_AO_SPIN == SF_AO_SPIN_MAX, "the table in the argument block is the ABI's largest");
static_assert(sizeof(AoSpin) <= 520, "the spin table's share of the argument segment");
static_assert(sizeof(FrameArgs) + sizeof(AoArgs) + 64 <= 4096, "kernel argument segment");
static_assert(sizeof(FrameArgs) + sizeof(AoSum) + sizeof(AoSpin) + 64 <= 4096, "kernel argument segment");
static_assert(sizeof(FrameArgs) + sizeof(MirrorArgs) + sizeof(AoSpin) + 64 <= 4096, "kernel argument segment");
static_assert(sizeof(FrameArgs) + sizeof(MirrorSum) + sizeof(AoSpin) + 64 <= 4096, "kernel argument segment");
static_assert(sizeof(AoArgs) == 792 && offsetof(AoArgs, tau) == 16 && offsetof(AoArgs, h) == 24, "AoArgs");
static_assert(sizeof(AoSum) == 1564 && offsetof(AoSum, accumulate) == 24 && offsetof(AoSum, h) == 28 &&
                  offsetof(AoSum, c) == 796, "AoSum");
static_assert(sizeof(AoSpin) == 520 && offsetof(AoSpin, cs) == 8, "AoSpin");
static_assert(sizeof(MirrorArgs) == 808 && offsetof(MirrorArgs, eye) == 24 && offsetof(MirrorArgs, use_eye) == 36 &&
                  offsetof(MirrorArgs, h) == 40, "MirrorArgs");
static_assert(sizeof(MirrorSum) == 1616 && offsetof(MirrorSum, accumulate) == 40 && offsetof(MirrorSum, up) == 44 &&
                  offsetof(MirrorSum, horizon) == 56 && offsetof(MirrorSum, span) == 68 &&
                  offsetof(MirrorSum, h) == 80 && offsetof(MirrorSum, c) == 848, "MirrorSum");

int sf_ao_defaults(const sf_ctx* c, sf_ao_params* p)
{
    if (!c || !p) return SF_EINVAL;
    std::memset(p, 0, sizeof *p);
    p->distance = 4.0f;
    p->bias = kShadowBias;
    return SF_OK;
}

int sf_mirror_defaults(const sf_ctx* c, sf_mirror_params* p)
{
    if (!c || !p) return SF_EINVAL;
    std::memset(p, 0, sizeof *p);
    p->distance = 4.0f;
    p->bias = kShadowBias;
    for (int k = 0; k < 3; ++k) p->zenith[k] = p->horizon[k] = 1.0f;
    p->up[2] = 1.0f;
    return SF_OK;
}

// A call, by what the twelve differ in.
enum SpinRule {
    kNoSpin,           // plain AO: the kernels take no table
    kSpinRequired,     // spun AO: a null table is SF_EINVAL
    kSpinOrIdentity    // the mirror: a null table is the 1 x 1 identity
};
struct LobeCall {
    bool given;                       // the caller's parameters were not null
    sf_ao_params p;                   // the fields all twelve share (the mirror's, copied in)
    const sf_mirror_params* mirror;   // the mirror's own fields, or null
    const sf_ao_spin* spin;
    SpinRule rule;
    bool sum;                         // colours into a light buffer, else one mask bit per sample
};

static LobeCall ao_call(const sf_ao_params* p, const sf_ao_spin* spin, SpinRule rule, bool sum)
{
    LobeCall k;
    std::memset(&k, 0, sizeof k);
    k.given = p != nullptr;
    if (p) k.p = *p;
    k.spin = spin;
    k.rule = rule;
    k.sum = sum;
    return k;
}

static LobeCall mirror_call(const sf_mirror_params* p, const sf_ao_spin* spin, bool sum)
{
    LobeCall k = ao_call(nullptr, spin, kSpinOrIdentity, sum);
    if (!p) return k;
    k.given = true;
    k.mirror = p;
    k.p.samples = p->samples;
    k.p.colours = p->colours;
    k.p.n = p->n;
    k.p.accumulate = p->accumulate;
    k.p.distance = p->distance;
    k.p.bias = p->bias;
    for (int i = 0; i < 3; ++i) k.p.origin[i] = p->origin[i];
    k.p.use_origin = p->use_origin;
    k.p.width = p->width;
    k.p.height = p->height;
    k.p.max_depth = p->max_depth;
    k.p.stream = p->stream;
    return k;
}

// the table: size 1..SF_AO_SPIN_MAX, every value finite; copied into the argument block
static int spin_args(const sf_ao_spin* spin, AoSpin* sp)
{
    if (!spin || !spin->cs || spin->size == 0u || spin->size > SF_AO_SPIN_MAX) return SF_EINVAL;
    std::memset(sp, 0, sizeof *sp);
    sp->size = spin->size;
    for (uint32_t e = 0; e < spin->size * spin->size; ++e)
        for (int k = 0; k < 2; ++k) {
            if (!std::isfinite(spin->cs[2u * e + k])) return SF_EINVAL;
            sp->cs[e][k] = spin->cs[2u * e + k];
        }
    return SF_OK;
}

// Everything a call checks, in this order: the list (the colours: the summing calls only), the distance, the image,
// a context buffer at the context's size only, the eye, the gradient (the summing calls only), then the table, which
// is copied into the argument block. The images' sizes come back in `im`.
static int lobe_check(const sf_ctx* c, const LobeCall& k, const float* pos4, bool ctx_buffer, ShadowImage* im,
                      AoSpin* sp)
{
    const sf_ao_params& p = k.p;
    if (int rc = entries_check(p.n, SF_AO_SAMPLES_MAX, p.samples, k.sum ? p.colours : nullptr, 3u * p.n, true))
        return rc;
    if (!(p.distance > 0.0f) || std::isinf(p.distance)) return SF_EINVAL;   // (NaN fails the compare)
    if (int rc = shadow_image(c, p.bias, p.max_depth, p.width, p.height, pos4, im)) return rc;
    if (ctx_buffer && (im->W != c->W || im->H != c->H)) return SF_EINVAL;
    if (const sf_mirror_params* const m = k.mirror) {
        if (m->use_eye)
            for (int i = 0; i < 3; ++i)
                if (!std::isfinite(m->eye[i])) return SF_EINVAL;
        if (k.sum)
            for (int i = 0; i < 3; ++i)
                if (!light_component(m->zenith[i]) || !light_component(m->horizon[i]) || !std::isfinite(m->up[i]))
                    return SF_EINVAL;
    }
    if (k.rule == kNoSpin) return SF_OK;
    if (k.spin || k.rule == kSpinRequired) return spin_args(k.spin, sp);
    std::memset(sp, 0, sizeof *sp);
    sp->size = 1u;
    sp->cs[0][0] = 1.0f;
    return SF_OK;
}

extern "C++" {
// What the four argument blocks share, what the two summing ones add, and what the mirror's two add.
template <class Args>
static void lobe_args(const sf_ctx* c, const sf_ao_params& p, Args* x)
{
    entry_args(c, p.use_origin, p.origin, p.bias, p.n, x);
    x->tau = p.distance;
    entry_triples(p.n, p.samples, x->h);
}

template <class Sum>
static void lobe_sum_args(const sf_ao_params& p, Sum* x)
{
    x->accumulate = p.accumulate ? 1u : 0u;
    entry_values(3u * p.n, p.colours, 1.0f / (float)p.n, &x->c[0][0]);
}

template <class Mirror>
static void lobe_eye_args(const sf_mirror_params* m, Mirror* x)
{
    x->use_eye = m->use_eye ? 1u : 0u;
    for (int i = 0; i < 3; ++i) x->eye[i] = m->use_eye ? m->eye[i] : 0.0f;
}
}  // extern "C++"

// The `_to` forms: null images are the context's (at its size only), a summing call's null out its light buffer.
static int lobe_to(sf_ctx* c, const LobeCall& k, const float* pos4, const float* nrm4, void* out)
{
    if (int rc = trace_preamble(c, k.given, k.sum || out != nullptr)) return rc;
    ShadowImage im;
    AoSpin sp;
    if (int rc = lobe_check(c, k, pos4, !nrm4 || !out, &im, &sp)) return rc;
    if (!out && !c->light) return SF_ESTATE;
    const sf_ao_params& p = k.p;
    const float* const nrm = nrm4 ? nrm4 : (const float*)c->nrm;
    if (!k.sum) {
        uint64_t* const mask = (uint64_t*)out;
        if (k.mirror) {
            MirrorArgs mr;
            lobe_args(c, p, &mr);
            lobe_eye_args(k.mirror, &mr);
            return mixed_origin_trace(c, p.stream, im, p.max_depth, sf_trace_mirror_wave, sf_trace_mirror_fixup, nrm,
                                      mr, sp, mask);
        }
        AoArgs ao;
        lobe_args(c, p, &ao);
        if (k.rule == kNoSpin)
            return mixed_origin_trace(c, p.stream, im, p.max_depth, sf_trace_ao_wave, sf_trace_ao_fixup, nrm, ao, mask);
        return mixed_origin_trace(c, p.stream, im, p.max_depth, sf_trace_ao_spin_wave, sf_trace_ao_spin_fixup, nrm, ao,
                                  sp, mask);
    }
    float* const dst = out ? (float*)out : c->light;
    if (const sf_mirror_params* const m = k.mirror) {
        MirrorSum mr;
        lobe_args(c, p, &mr);
        lobe_eye_args(m, &mr);
        lobe_sum_args(p, &mr);
        for (int i = 0; i < 3; ++i) {
            mr.up[i] = m->up[i];
            mr.horizon[i] = m->horizon[i];
            mr.span[i] = m->zenith[i] - m->horizon[i];   // (one rounding: zenith.c - horizon.c of the definition)
        }
        return mixed_origin_trace(c, p.stream, im, p.max_depth, sf_trace_mirror_sum_wave, sf_trace_mirror_sum_fixup,
                                  nrm, mr, sp, dst);
    }
    AoSum ao;
    lobe_args(c, p, &ao);
    lobe_sum_args(p, &ao);
    if (k.rule == kNoSpin)
        return mixed_origin_trace(c, p.stream, im, p.max_depth, sf_trace_ao_sum_wave, sf_trace_ao_sum_fixup, nrm, ao,
                                  dst);
    return mixed_origin_trace(c, p.stream, im, p.max_depth, sf_trace_ao_spin_sum_wave, sf_trace_ao_spin_sum_fixup, nrm,
                              ao, sp, dst);
}

// The own-buffer forms: the context's G-buffer into its mask buffer, or into its light buffer, which an overwriting
// call makes and an accumulating one needs written (trace_sum_own).
static int lobe_own(sf_ctx* c, const LobeCall& k)
{
    if (int rc = trace_preamble(c, k.given)) return rc;
    ShadowImage im;
    AoSpin sp;
    const auto check = [&] { return lobe_check(c, k, nullptr, true, &im, &sp); };
    if (k.sum) {
        if (int rc = own_buffer_checked(c, &c->light, 16, k.p.accumulate != 0u, check)) return rc;
        return lobe_to(c, k, nullptr, nullptr, nullptr);
    }
    if (int rc = own_buffer_checked(c, &c->shadow_masks, 8, false, check)) return rc;
    return lobe_to(c, k, nullptr, nullptr, c->shadow_masks);
}

int sf_trace_ao_to(sf_ctx* c, const sf_ao_params* p, const float* pos4, const float* nrm4, uint64_t* mask)
{
    return lobe_to(c, ao_call(p, nullptr, kNoSpin, false), pos4, nrm4, mask);
}

int sf_trace_ao(sf_ctx* c, const sf_ao_params* p) { return lobe_own(c, ao_call(p, nullptr, kNoSpin, false)); }

int sf_trace_ao_sum_to(sf_ctx* c, const sf_ao_params* p, const float* pos4, const float* nrm4, float* out)
{
    return lobe_to(c, ao_call(p, nullptr, kNoSpin, true), pos4, nrm4, out);
}

int sf_trace_ao_sum(sf_ctx* c, const sf_ao_params* p) { return lobe_own(c, ao_call(p, nullptr, kNoSpin, true)); }

int sf_trace_ao_spin_to(sf_ctx* c, const sf_ao_params* p, const sf_ao_spin* spin, const float* pos4, const float* nrm4,
                        uint64_t* mask)
{
    return lobe_to(c, ao_call(p, spin, kSpinRequired, false), pos4, nrm4, mask);
}

int sf_trace_ao_spin(sf_ctx* c, const sf_ao_params* p, const sf_ao_spin* spin)
{
    return lobe_own(c, ao_call(p, spin, kSpinRequired, false));
}

int sf_trace_ao_spin_sum_to(sf_ctx* c, const sf_ao_params* p, const sf_ao_spin* spin, const float* pos4,
                            const float* nrm4, float* out)
{
    return lobe_to(c, ao_call(p, spin, kSpinRequired, true), pos4, nrm4, out);
}

int sf_trace_ao_spin_sum(sf_ctx* c, const sf_ao_params* p, const sf_ao_spin* spin)
{
    return lobe_own(c, ao_call(p, spin, kSpinRequired, true));
}

int sf_trace_mirror_to(sf_ctx* c, const sf_mirror_params* p, const sf_ao_spin* spin, const float* pos4,
                       const float* nrm4, uint64_t* mask)
{
    return lobe_to(c, mirror_call(p, spin, false), pos4, nrm4, mask);
}

int sf_trace_mirror(sf_ctx* c, const sf_mirror_params* p, const sf_ao_spin* spin)
{
    return lobe_own(c, mirror_call(p, spin, false));
}

int sf_trace_mirror_sum_to(sf_ctx* c, const sf_mirror_params* p, const sf_ao_spin* spin, const float* pos4,
                           const float* nrm4, float* out)
{
    return lobe_to(c, mirror_call(p, spin, true), pos4, nrm4, out);
}

int sf_trace_mirror_sum(sf_ctx* c, const sf_mirror_params* p, const sf_ao_spin* spin)
{
    return lobe_own(c, mirror_call(p, spin, true));
}

// The edge-aware box filter of the light buffer (kernel sf_light_filter_px).
int sf_light_filter_defaults(const sf_ctx* c, sf_light_filter_params* p)
{
    if (!c || !p) return SF_EINVAL;
    std::memset(p, 0, sizeof *p);
    p->size = 4u;
    p->normal_min = 0.9f;
    p->plane_max = 0.02f;
    return SF_OK;
}

// The parameters alone: every failure here is SF_EINVAL.
static int filter_check(const sf_ctx* c, const sf_light_filter_params* p, bool ctx_buffer, uint32_t* W, uint32_t* H)
{
    if (p->size == 0u || p->size > SF_AO_SPIN_MAX) return SF_EINVAL;
    if (p->normal_min != p->normal_min) return SF_EINVAL;
    if (!(p->plane_max >= 0.0f) || std::isinf(p->plane_max)) return SF_EINVAL;   // (NaN fails the compare)
    if ((p->width == 0u) != (p->height == 0u)) return SF_EINVAL;
    *W = p->width ? p->width : c->W;
    *H = p->height ? p->height : c->H;
    if (ctx_buffer && (*W != c->W || *H != c->H)) return SF_EINVAL;   // (a context buffer, at its size only)
    if ((uint64_t)*W * *H > 0x7fffffffull) return SF_EINVAL;   // (pixel indices are 32-bit in the kernel)
    return SF_OK;
}

// The launch on the call's stream; `back`: where the result is then copied (the context form), or null.
static int filter_launch(sf_ctx* c, const sf_light_filter_params* p, uint32_t W, uint32_t H, const float* pos4,
                         const float* nrm4, const float* in, float* out, float* back)
{
    const float k2 = p->plane_max * p->plane_max;   // (one rounding: sf.h's k2)
    hipStream_t s = p->stream ? (hipStream_t)p->stream : c->stream;
    DevGuard g(c->device);
    if (int rc = ctx_join(c, s)) return rc;
    StreamMark mark_(c, s);
    const dim3 grid((W + 31u) / 32u, (H + 7u) / 8u);   // (SF_FILTER_BX x SF_FILTER_BY pixels per block, sf_post.hip)
    if (grid.x == 0u || grid.y == 0u) return SF_OK;
    hipLaunchKernelGGL(sf_light_filter_px, grid, dim3(256), 0, s, W, H, pos4, nrm4, in, out, p->size, p->normal_min,
                       k2);
    SF_HIP(c, hipGetLastError());
    if (back) SF_HIP(c, hipMemcpyAsync(back, out, (size_t)W * H * 16, hipMemcpyDeviceToDevice, s));
    return SF_OK;
}

int sf_light_filter_to(sf_ctx* c, const sf_light_filter_params* p, const float* pos4, const float* nrm4,
                       const float* in, float* out)
{
    if (!c || !p || !out) return SF_EINVAL;
    uint32_t W, H;
    if (int rc = filter_check(c, p, !pos4 || !nrm4 || !in, &W, &H)) return rc;
    if (!in && !c->light) return SF_ESTATE;
    const float* const src = in ? in : (const float*)c->light;
    if (src == out) return SF_EINVAL;
    return filter_launch(c, p, W, H, pos4 ? pos4 : (const float*)c->pos, nrm4 ? nrm4 : (const float*)c->nrm, src, out,
                         nullptr);
}

// In place for the caller: into the context's second buffer, then copied back on the same stream.
int sf_light_filter(sf_ctx* c, const sf_light_filter_params* p)
{
    if (!c || !p) return SF_EINVAL;
    uint32_t W, H;
    if (int rc = filter_check(c, p, true, &W, &H)) return rc;
    if (!c->light) return SF_ESTATE;
    if (!c->light_filtered) {
        DevGuard g(c->device);
        SF_HIP(c, hipMalloc(&c->light_filtered, (size_t)W * H * 16));
    }
    return filter_launch(c, p, W, H, c->pos, c->nrm, c->light, c->light_filtered, c->light);
}

// The light buffer over several frames (kernel sf_light_accumulate_px). The inverse of a view's ray
// generation first: host arithmetic in double, every operation rounded on its own (the build's -ffp-contract=off), in
// sf.h's order; sphereflake_amd/lights.py reproject_matrix forms the same bits.
int sf_reproject_matrix(const float view[12], float m[9])
{
    if (!view || !m) return SF_EINVAL;
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(view[k])) return SF_EINVAL;
    const float *o = view, *tl = view + 3, *tr = view + 6, *bl = view + 9;
    double a[3], b[3], cc[3];
    for (int k = 0; k < 3; ++k) {
        const float af = tr[k] - tl[k], bf = bl[k] - tl[k], cf = tl[k] - o[k];   // (binary32, then promoted)
        a[k] = (double)af;
        b[k] = (double)bf;
        cc[k] = (double)cf;
    }
    const double bc[3] = { b[1] * cc[2] - b[2] * cc[1], b[2] * cc[0] - b[0] * cc[2], b[0] * cc[1] - b[1] * cc[0] };
    const double ca[3] = { cc[1] * a[2] - cc[2] * a[1], cc[2] * a[0] - cc[0] * a[2], cc[0] * a[1] - cc[1] * a[0] };
    const double ab[3] = { a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0] };
    const double det = (a[0] * bc[0] + a[1] * bc[1]) + a[2] * bc[2];
    if (det == 0.0 || !std::isfinite(det)) return SF_EINVAL;
    float r[9];
    for (int k = 0; k < 3; ++k) {
        r[k] = (float)(bc[k] / det);
        r[3 + k] = (float)(ca[k] / det);
        r[6 + k] = (float)(ab[k] / det);
    }
    std::memcpy(m, r, sizeof r);
    return SF_OK;
}

int sf_light_accumulate_defaults(const sf_ctx* c, sf_light_accumulate_params* p)
{
    if (!c || !p) return SF_EINVAL;
    std::memset(p, 0, sizeof *p);
    p->max_history = 16u;
    p->normal_min = 0.9f;
    p->plane_max = 0.02f;
    return SF_OK;
}

// The parameters alone (the history's view: the _to form only); every failure here is SF_EINVAL.
static int accumulate_check(const sf_ctx* c, const sf_light_accumulate_params* p, bool ctx_form, uint32_t* W,
                            uint32_t* H)
{
    if (p->max_history == 0u || p->max_history > 65535u) return SF_EINVAL;
    if (p->normal_min != p->normal_min) return SF_EINVAL;
    if (!(p->plane_max >= 0.0f) || std::isinf(p->plane_max)) return SF_EINVAL;   // (NaN fails the compare)
    if (!ctx_form) {
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(p->hist_origin[k])) return SF_EINVAL;
        for (int k = 0; k < 9; ++k)
            if (!std::isfinite(p->hist_m[k])) return SF_EINVAL;
    }
    if ((p->width == 0u) != (p->height == 0u)) return SF_EINVAL;
    *W = p->width ? p->width : c->W;
    *H = p->height ? p->height : c->H;
    if (ctx_form && (*W != c->W || *H != c->H)) return SF_EINVAL;   // (the context's buffers, at its size only)
    if ((uint64_t)*W * *H > 0x7fffffffull) return SF_EINVAL;   // (pixel indices are 32-bit in the kernel)
    return SF_OK;
}

// The kernel's argument block: the thresholds of the params, the two origins and the history view's matrix.
static LightAccum accumulate_args(const sf_light_accumulate_params* p, const float o[3], const float ho[3],
                                  const float m[9])
{
    LightAccum a;
    for (int k = 0; k < 3; ++k) {
        a.o[k] = o[k];
        a.ho[k] = ho[k];
    }
    for (int k = 0; k < 9; ++k) a.m[k] = m[k];
    a.max_history = (float)p->max_history;
    a.normal_min = p->normal_min;
    a.k2 = p->plane_max * p->plane_max;   // (one rounding: sf.h's k2)
    return a;
}

int sf_light_accumulate_to(sf_ctx* c, const sf_light_accumulate_params* p, const float* pos4, const float* nrm4,
                           const float* in, const float* hist_pos4, const float* hist_nrm4, const float* hist,
                           float* out)
{
    if (!c || !p || !pos4 || !nrm4 || !in || !hist_pos4 || !hist_nrm4 || !hist || !out) return SF_EINVAL;
    uint32_t W, H;
    if (int rc = accumulate_check(c, p, false, &W, &H)) return rc;
    for (const float* src : { pos4, nrm4, in, hist_pos4, hist_nrm4, hist })
        if (src == out) return SF_EINVAL;
    if (!c->has_view && !p->use_origin) return SF_ENOVIEW;
    const LightAccum a = accumulate_args(p, p->use_origin ? p->origin : c->o, p->hist_origin, p->hist_m);
    return pixel_pass_of(c, p->stream, (size_t)W * H, sf_light_accumulate_px, W, H, pos4, nrm4, in, hist_pos4,
                         hist_nrm4, hist, out, a);
}

// The context form: into the filter's second buffer, copied back, and the frame kept as the next call's history.
int sf_light_accumulate(sf_ctx* c, const sf_light_accumulate_params* p)
{
    if (!c || !p) return SF_EINVAL;
    uint32_t W, H;
    if (int rc = accumulate_check(c, p, true, &W, &H)) return rc;
    if (!c->has_view) return SF_ENOVIEW;
    if (!c->light) return SF_ESTATE;
    float view[12], m[9];
    std::memcpy(view, c->o, 12);
    std::memcpy(view + 3, c->tl, 12);
    std::memcpy(view + 6, c->tr, 12);
    std::memcpy(view + 9, c->bl, 12);
    if (int rc = sf_reproject_matrix(view, m)) return rc;
    const size_t bytes = (size_t)W * H * 16;
    DevGuard g(c->device);
    for (float** buf : { &c->light_filtered, &c->hist_pos, &c->hist_nrm, &c->hist_light })
        if (!*buf) SF_HIP(c, hipMalloc(buf, bytes));
    hipStream_t s = p->stream ? (hipStream_t)p->stream : c->stream;
    if (!c->hist_valid) {
        // no history: one whose every pixel is a miss with .w = 0, seen through the current view -- every tap is
        // rejected at its first test
        if (int rc = ctx_join(c, s)) return rc;
        StreamMark mark_(c, s);
        SF_HIP(c, hipMemsetAsync(c->hist_pos, 0, bytes, s));
        SF_HIP(c, hipMemsetAsync(c->hist_nrm, 0, bytes, s));
        SF_HIP(c, hipMemsetAsync(c->hist_light, 0, bytes, s));
        std::memcpy(c->hist_o, c->o, sizeof c->hist_o);
        std::memcpy(c->hist_m, m, sizeof c->hist_m);
    }
    const LightAccum a = accumulate_args(p, c->o, c->hist_o, c->hist_m);
    c->hist_valid = false;   // (until the copies below are queued: a failure between leaves no half-made history)
    if (int rc = pixel_pass_of(c, s, (size_t)W * H, sf_light_accumulate_px, W, H, (const float*)c->pos,
                               (const float*)c->nrm, (const float*)c->light, (const float*)c->hist_pos,
                               (const float*)c->hist_nrm, (const float*)c->hist_light, c->light_filtered, a))
        return rc;
    StreamMark mark_(c, s);
    SF_HIP(c, hipMemcpyAsync(c->light, c->light_filtered, bytes, hipMemcpyDeviceToDevice, s));
    SF_HIP(c, hipMemcpyAsync(c->hist_pos, c->pos, bytes, hipMemcpyDeviceToDevice, s));
    SF_HIP(c, hipMemcpyAsync(c->hist_nrm, c->nrm, bytes, hipMemcpyDeviceToDevice, s));
    SF_HIP(c, hipMemcpyAsync(c->hist_light, c->light_filtered, bytes, hipMemcpyDeviceToDevice, s));
    std::memcpy(c->hist_o, c->o, sizeof c->hist_o);
    std::memcpy(c->hist_m, m, sizeof c->hist_m);
    c->hist_valid = true;
    return SF_OK;
}

int sf_light_history_reset(sf_ctx* c)
{
    if (!c) return SF_EINVAL;
    c->hist_valid = false;
    return SF_OK;
}

int sf_light_buffer(sf_ctx* c, float** buf) { return own_buffer_pointer(c, &sf_ctx::light, true, buf); }

int sf_download_light(sf_ctx* c, float* buf4) { return download_own(c, &sf_ctx::light, 16, buf4); }

// One thread per pixel of the context's frame; a null buf is the context's buffer, made here if need be.
int sf_light_fill(sf_ctx* c, const float rgb[3], float* buf, void* stream)
{
    if (!c || !rgb) return SF_EINVAL;
    for (int k = 0; k < 3; ++k)
        if (!light_component(rgb[k])) return SF_EINVAL;
    if (!buf)   // (the traces' path for the buffer; the colour is checked above, so nothing is left for its check)
        if (int rc = own_buffer_checked(c, &c->light, 16, false, [] { return SF_OK; })) return rc;
    return pixel_pass(c, stream, sf_light_fill_px, c->W * c->H, rgb[0], rgb[1], rgb[2], buf ? buf : c->light);
}

// The resolve pass: the buffers defaulted to the context's.
int sf_light_image_buffer(sf_ctx* c, void* stream, const float* pos4, const float* buf, uint8_t* rgba)
{
    if (!c) return SF_EINVAL;
    if (!rgba && !c->image) return SF_ESTATE;
    if (!buf && !c->light) return SF_ESTATE;
    return pixel_pass(c, stream, sf_light_image_buffer_px, c->W, c->H, pos4 ? pos4 : (const float*)c->pos,
                      buf ? buf : (const float*)c->light, rgba ? rgba : c->image);
}

// Multi-frame persistent trace (sf.h; kernel sf_trace_frames1). One launch where every frame's own launch() would be
// a bounded persistent one-wave trace (levels proven for its view, ties re-traced inline, no fixup launch), else one
// launch() per frame. The frames share the first context's tile queues, its unit order (rebuilt from frame 0's costs
// on its schedule) and its kernel timing; each frame writes its own context's G-buffer, aux channels and stats.
int sf_render_frames(sf_ctx* const* cs, uint32_t n, const sf_render_params* pp)
{
    static_assert(SF_RENDER_FRAMES_MAX <= (int)SF_BATCH_MAX, "the batch travels in the kernel argument segment");
    static_assert(sizeof(FrameBatch) <= 4096, "kernel argument segment");
    if (!cs || n == 0 || n > (uint32_t)SF_RENDER_FRAMES_MAX) return SF_EINVAL;
    sf_render_params p;
    std::memset(&p, 0, sizeof p);
    if (pp) p = *pp;
    if (p.compact || p.packed || p.kernel == SF_KERNEL_PER_RAY || p.max_depth) return SF_EINVAL;
    sf_ctx* const c0 = cs[0];
    for (uint32_t k = 0; k < n; ++k) {
        if (!cs[k]) return SF_EINVAL;
        if (!cs[k]->has_view) return SF_ENOVIEW;
        if (cs[k]->device != c0->device || cs[k]->W != c0->W || cs[k]->H != c0->H) return SF_EINVAL;
        for (uint32_t j = 0; j < k; ++j)
            if (cs[j] == cs[k]) return SF_EINVAL;   // (two frames into one G-buffer in one launch would race)
    }
    const sfplan::BandShare sh = sfplan::band_share(c0->H, p.band_rows, p.band_count, p.band_index);
    if (sh.band_rows % 8 != 0 || p.band_index >= sh.band_count || p.kernel > SF_KERNEL_PER_RAY) return SF_EINVAL;
    // one launch only where each frame alone would take the bounded one-wave persistent trace with nothing after it
    uint32_t levels = 0;
    bool one = n > 1 || c0->frames_one;
    for (uint32_t k = 0; k < n && one; ++k) {
        const sf_ctx* c = cs[k];
        bool bounded = false;
        const uint32_t l = frame_levels(c, &bounded);
        const bool front_first = (c->flags & (SF_FLAG_NO_OCCL_CULL | SF_FLAG_NO_FRONT_FIRST)) == 0u;
        one = bounded && c->persistent && c->knobs.waves_per_block == 1u && !c->knobs.compact && !c->part_rec &&
              !c->tile_trace && !(front_first && !c->tie_inline) && c->flags == c0->flags &&
              c->variant == c0->variant && !(c->flags & SF_FLAG_DIAG_HALF);
        levels = l > levels ? l : levels;
    }
    if (!one) {   // one launch per frame: the same frames (launch() orders each context's own calls)
        for (uint32_t k = 0; k < n; ++k)
            if (int rc = launch(cs[k], &p, cs[k]->pos, cs[k]->nrm, cs[k]->min_t, cs[k]->hit_index)) return rc;
        return SF_OK;
    }
    hipStream_t s = p.stream ? (hipStream_t)p.stream : c0->stream;
    DevGuard g(c0->device);
    if (sh.tile_rows == 0) return SF_OK;
    bool unknown_before[SF_BATCH_MAX];
    for (uint32_t k = 0; k < n; ++k) {
        unknown_before[k] = cs[k]->stats_unknown;
        if (int rc = ctx_join(cs[k], s)) return rc;
    }
    const size_t lds = (size_t)SF_LDS_WAVE_FLOATS(levels) * 4;
    const int key = (int)(64 + levels) | (1 << 21);   // (c0's occupancy cache, told apart from launch()'s keys)
    if (c0->occ_key != key) {
        int nb = 0;
        SF_HIP(c0, hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)sf_trace_frames1, 64, lds));
        c0->occ_blocks = nb < 1 ? 1 : nb;
        c0->occ_key = key;
    }
    // the schedule c0's order state gives these frames: launch()'s for one of them, on the one kernel
    const bool front_first = (c0->flags & (SF_FLAG_NO_OCCL_CULL | SF_FLAG_NO_FRONT_FIRST)) == 0u;
    const sfplan::Launch ask = { (c0->W + 7) / 8, sh.tile_rows, sh.band_count, false, false, p.emit_aux != 0, false,
                                 c0->flags | (front_first ? SF_FLAG_TIE_INLINE : 0u), n };
    const sfplan::RenderPlan pl = sfplan::render_plan(ask, c0->knobs, { (uint32_t)c0->occ_blocks * (uint32_t)c0->cus, 0u, 0u },
                                                      { c0->order_n, c0->order_pair, c0->order_phase });
    if (!pl.ok) return SF_EINVAL;
    c0->order_phase = pl.order_phase;
    FrameBatch b;
    std::memset(&b, 0, sizeof b);
    b.nframes = n;
    b.magic = (uint32_t)((0x100000000ull + n - 1u) / n);
    b.units = pl.units;
    b.heavy = c0->frames_heavy >= 0 ? (uint32_t)c0->frames_heavy : pl.grid / n;   // every frame's heaviest units among
                                                                                   // the waves' static first units
    for (uint32_t k = 0; k < n; ++k) {
        sf_ctx* c = cs[k];
        FrameArgs a = frame_args(c);
        if (front_first) a.flags |= SF_FLAG_TIE_INLINE;
        // (only frame 0 records unit costs: the order and its histogram are per unit)
        plan_frame_args(a, p, sh, &pl, c0, k == 0u);
        a.pos = c->pos;
        a.nrm = c->nrm;
        a.min_t = c->min_t;
        a.hit_index = c->hit_index;
        a.max_depth = levels;
        a.counters = c0->ovf_counters;   // the launch's queues: c0's, at c0's parity
        a.overflow_list = c0->ovf_list;
        a.parity = c0->parity;
        b.f[k] = a;
    }
    if (int rc = timed_launch(c0, s, &b.f[0].clock_probe, [&] {
            hipLaunchKernelGGL(sf_trace_frames1, dim3(pl.grid), dim3(64), lds, s, b);
        }))
        return rc;
    if (pl.rebuild)
        if (int rc = order_rebuild(c0, s, pl.units, pl.order_waves, pl.split_buckets)) return rc;
    c0->parity ^= 1u;
    for (uint32_t k = 0; k < n; ++k) {
        sf_ctx* c = cs[k];
        c->rays += (int64_t)sh.rows * c->W;
        c->stats_unknown = unknown_before[k];   // (bounded, unpacked: the launch adds nothing to the unresolved word)
        if (s != c->stream) SF_HIP(c, hipEventRecord(c->join_ev, s));   // (StreamMark)
    }
    return SF_OK;
}

// Depth bound of every hit under the context's view (-1: none provable). Every sphere lies inside the root's
// bounding sphere (radius 2 around the root centre), so a depth-d node can pass the LOD test (t < T_d,
// Sphereflake.h:146) only if |root centre| - 2 < T_d; a node is self-tested only when its parent passed, so hits
// lie at most one level below the deepest such d: the bound launch() provisions its LDS levels from,
// geometric_levels. (That one answers its default, unproven, where the gap is not positive, and d + 1 otherwise --
// proven unless it is more levels than the kernels have: a positive gap shows as one or the other.)
static int hit_depth_bound(const sf_ctx* c)
{
    bool bounded = false;
    const uint32_t levels = geometric_levels(c, &bounded);
    return (bounded || levels > SF_MAX_DEPTH_LIMIT) ? (int)levels : -1;
}

// True when no depth-SF_INDEX_SLAB_DEPTH node can pass the LOD test for any ray of the view, so every hit lies at depth
// <= SF_INDEX_SLAB_DEPTH (heap index below 2^32). Branch and bound over the node tree in double precision: a node's
// whole subtree lies in its bounding ball (centre c, radius 2 r_d: each level's ball is internally tangent to its
// parent's), and a node at depth D can expand only if t < T_D, where its bounding root t >= |c - O| - 2 r_D (O = the
// ray origin, the frame's origin: the root transform maps it to 0). A subtree whose ball stays farther than T_D
// from O is pruned. Slack: the float chain's centres are within ~1e-6 |c| of these, the float t within ~1e-6 of
// the distance; 1e-3 relative and 1e-5 absolute cover both. The search gives up (false) past kMaxNodes nodes.
static bool index_depth_proven(const sf_ctx* c)
{
    const int D = SF_INDEX_SLAB_DEPTH;
    const double TD = (double)c->host_consts.dt.lod[D] * (1.0 + 1e-3) + 1e-5;
    struct Node {
        double m[12];   // columns 0..3, xyz (the child_frame layout)
        int d;
    };
    constexpr int kMaxNodes = 1 << 16;
    std::vector<Node> stack;
    stack.reserve(256);
    Node root;
    for (int col = 0; col < 4; ++col)
        for (int r = 0; r < 3; ++r) root.m[3 * col + r] = (double)c->root[4 * col + r];
    root.d = 0;
    stack.push_back(root);
    int visited = 0;
    while (!stack.empty()) {
        const Node nd = stack.back();
        stack.pop_back();
        if (++visited > kMaxNodes) return false;
        const double* cc = nd.m + 9;
        const double dist = std::sqrt(cc[0] * cc[0] + cc[1] * cc[1] + cc[2] * cc[2]);
        const double R = 2.0 * (double)sfhost::radius((uint32_t)nd.d) * (1.0 + 1e-6) + 1e-5 * (dist + 1.0);
        if (dist - R >= TD) continue;      // no depth-D node of this subtree comes within T_D of the origin
        if (nd.d == D) return false;       // a depth-D node that may expand: a hit could lie at depth D + 1
        const double s = (double)c->host_consts.dt.scale[nd.d];
        for (int i = 0; i < 9; ++i) {
            Node ch;
            ch.d = nd.d + 1;
            for (int col = 0; col < 4; ++col) {
                double b[4];
                for (int k = 0; k < 4; ++k) b[k] = (double)c->child[i][4 * col + k];
                if (col == 3)
                    for (int k = 0; k < 3; ++k) b[k] *= s;
                for (int r = 0; r < 3; ++r)
                    ch.m[3 * col + r] = nd.m[r] * b[0] + nd.m[3 + r] * b[1] + nd.m[6 + r] * b[2] + nd.m[9 + r] * b[3];
            }
            stack.push_back(ch);
        }
    }
    return true;
}

uint32_t sf_slab_bytes(const sf_ctx* cc)
{
    if (!cc || !cc->has_view) return 0;
    const int d = hit_depth_bound(cc);
    if (d >= 0 && d <= SF_INDEX_SLAB_DEPTH) return 4u;   // (the cheap bound: the whole flake is far enough)
    // the search, cached per view (the root transform) and constant block: a camera path revisits its views
    sf_ctx* c = const_cast<sf_ctx*>(cc);   // (the cache only)
    for (const auto& e : c->slab_cache)
        if (e.gen == c->consts_gen && std::memcmp(e.root, c->root, sizeof e.root) == 0) return e.bytes;
    const uint32_t bytes = index_depth_proven(c) ? 4u : 16u;
    auto& e = c->slab_cache[c->slab_cache_next];
    c->slab_cache_next = (c->slab_cache_next + 1u) % (uint32_t)(sizeof c->slab_cache / sizeof c->slab_cache[0]);
    std::memcpy(e.root, c->root, sizeof e.root);
    e.gen = c->consts_gen;
    e.bytes = bytes;
    return bytes;
}

// The unpack of packed band slabs into the G-buffer on stream s. join: order after the context's previous call
// like every public call (sf_unpack_slabs); without it the caller orders the stream itself (sf_dist / sf_group
// run the unpack beside the context's own trace, on a stream of their own, and join it back with an event).
int sfi_unpack_slabs(sf_ctx* c, const void* stage, uint32_t bytes_per_pixel, uint32_t stage_rows, uint32_t band_rows,
                     uint32_t band_count, uint32_t first_member, uint32_t members, hipStream_t s, bool join)
{
    if (!c || !stage || band_rows == 0 || band_rows % 8 != 0 || band_count == 0 || first_member >= band_count ||
        members > band_count - first_member || (bytes_per_pixel != 4u && bytes_per_pixel != 16u))
        return SF_EINVAL;
    if (!c->has_view) return SF_ENOVIEW;
    if (members == 0) return SF_OK;
    // every member's slab must fit its stage_rows rows: a shorter stage would leave its last rows stale
    for (uint32_t k = first_member; k < first_member + members; ++k)
        if (sf_slab_rows(c->H, band_rows, band_count, k) > stage_rows) return SF_EINVAL;
    if (stage_rows == 0) return SF_OK;
    if (bytes_per_pixel == 4u && sf_slab_bytes(c) != 4u) return SF_EINVAL;   // (the view allows no index slab)
    DevGuard g(c->device);
    if (join) {
        if (int rc = ctx_join(c, s)) return rc;
    }
    // work enqueued whatever `join` says: the next sf_synchronize drains and checks (an unpack alone,
    // without the caller's sfi_join / sf_render beside it, must not meet the idle-sync return)
    c->stats_dirty = true;
    c->stats_unknown = true;
    FrameArgs a = frame_args(c);
    a.pos = c->pos;
    a.nrm = c->nrm;
    if (bytes_per_pixel == 4u) {
        if (!c->node_table)
            SF_HIP(c, hipMalloc(&c->node_table, (size_t)SF_NODE_TABLE_NODES * 3 * sizeof(float4)));
        float root12[12];
        for (int col = 0; col < 4; ++col)
            for (int r = 0; r < 3; ++r) root12[3 * col + r] = c->root[4 * col + r];
        if (c->table_gen != c->consts_gen || std::memcmp(root12, c->table_root, sizeof root12) != 0) {
            hipLaunchKernelGGL(sf_node_table, dim3((SF_NODE_TABLE_NODES + 255u) / 256u), dim3(256), 0, s, a,
                               c->node_table, SF_NODE_TABLE_NODES);
            SF_HIP(c, hipGetLastError());
            std::memcpy(c->table_root, root12, sizeof root12);
            c->table_gen = c->consts_gen;
        }
    }
    if (bytes_per_pixel == 4u) {
        // resident workgroups over the 256-pixel segments (each stages the per-lane constants in LDS once): 8 per CU,
        // or fewer when the slabs have fewer segments
        const uint64_t items = (uint64_t)members * stage_rows * ((c->W + 255u) / 256u);
        const uint64_t cap = 8ull * (uint64_t)c->cus;
        const dim3 grid((uint32_t)(items < cap ? items : cap));
        hipLaunchKernelGGL(sf_slab_unpack4, grid, dim3(256), 0, s, a, reinterpret_cast<const uint32_t*>(stage),
                           (const float4*)c->node_table, SF_NODE_TABLE_DEPTH, stage_rows, band_rows, band_count,
                           first_member, members);
        SF_HIP(c, hipGetLastError());
    }
    for (uint32_t r0 = 0; bytes_per_pixel == 16u && r0 < stage_rows; r0 += 65535u) {
        const uint32_t rows = stage_rows - r0 < 65535u ? stage_rows - r0 : 65535u;
        const dim3 grid((c->W + 255u) / 256u, rows, members);
        hipLaunchKernelGGL(sf_band_unpack, grid, dim3(256), 0, s, a, reinterpret_cast<const float4*>(stage),
                           stage_rows, band_rows, band_count, first_member, members, r0);
        SF_HIP(c, hipGetLastError());
    }
    if (join && s != c->stream) SF_HIP(c, hipEventRecord(c->join_ev, s));   // (StreamMark)
    return SF_OK;
}

// Order the context's own stream after everything the context enqueued before, on whatever stream (ctx_join).
// sf_dist / sf_group call it before they record a frame's start event on the context stream: their receive /
// unpack stream waits only for that event, so the event must already follow earlier consumers queued on a
// caller's stream (sf_download_async, sf_post_process on stream X), or the unpack could overwrite rows X is
// still reading.
int sfi_join(sf_ctx* c)
{
    if (!c) return SF_EINVAL;
    DevGuard g(c->device);
    return ctx_join(c, c->stream);
}

int sf_unpack_slabs(sf_ctx* c, const void* stage, uint32_t bytes_per_pixel, uint32_t stage_rows, uint32_t band_rows,
                    uint32_t band_count, uint32_t first_member, uint32_t members, void* stream)
{
    if (!c) return SF_EINVAL;
    return sfi_unpack_slabs(c, stage, bytes_per_pixel, stage_rows, band_rows, band_count, first_member, members,
                            stream ? (hipStream_t)stream : c->stream, true);
}

int sf_unpack_bands(sf_ctx* c, const float* stage4, uint32_t stage_rows, uint32_t band_rows, uint32_t band_count,
                    uint32_t first_member, uint32_t members, void* stream)
{
    return sf_unpack_slabs(c, stage4, 16u, stage_rows, band_rows, band_count, first_member, members, stream);
}

// n draws of the context's mt19937 stream into `out`, on stream s (advances c->mt_state): the single-workgroup
// generator for small counts, else the parallel jump-ahead path (same stream bit for bit).
static int gen_draws(sf_ctx* c, hipStream_t s, uint32_t* out, uint32_t n)
{
    if (!c->mt_parallel || n < kMtParMin) {
        hipLaunchKernelGGL(sf_mt_draws, dim3(1), dim3(256), 0, s, c->mt_state, out, n);
        SF_HIP(c, hipGetLastError());
        return SF_OK;
    }
    uint32_t K = n / kMtSegMin;
    K = K < 2u ? 2u : K > c->mt_seg_max ? c->mt_seg_max : K;
    const uint32_t L = (n + K - 1u) / K;
    const uint32_t pw = (uint32_t)sfhost::mt_poly_words();
    if (!c->mt_raw || !c->mt_partial || !c->mt_state2 || !c->mt_polys) {
        // all four scratch buffers or none: a partial set would let a later call launch on null buffers
        hipError_t e = hipSuccess;
        if (!c->mt_raw) e = hipMalloc(&c->mt_raw, (size_t)kMtRawBlocks * 624 * 4);
        if (e == hipSuccess && !c->mt_partial) e = hipMalloc(&c->mt_partial, (size_t)(kMtSegMax - 1) * kMtParts * 624 * 4);
        if (e == hipSuccess && !c->mt_state2) e = hipMalloc(&c->mt_state2, 625 * 4);
        if (e == hipSuccess && !c->mt_polys) e = hipMalloc(&c->mt_polys, (size_t)kMtSegMax * pw * 8);
        if (e != hipSuccess) {
            (void)hipFree(c->mt_raw);
            (void)hipFree(c->mt_partial);
            (void)hipFree(c->mt_state2);
            (void)hipFree(c->mt_polys);
            c->mt_raw = c->mt_partial = c->mt_state2 = nullptr;
            c->mt_polys = nullptr;
            c->mt_poly_key = 0;
            c->last_hip = (int)e;
            return e == hipErrorOutOfMemory ? SF_ENOMEM : SF_EHIP;
        }
    }
    const uint64_t key = ((uint64_t)L << 8) | K;
    if (c->mt_poly_key != key) {   // (host polynomials cached per (L, K); ~20 ms for a new batch size)
        SF_HIP(c, hipMemcpyAsync(c->mt_polys, sfhost::mt_jump_polys(L, K), (size_t)K * pw * 8, hipMemcpyHostToDevice, s));
        c->mt_poly_key = key;
    }
    hipLaunchKernelGGL(sf_mt_raw, dim3(1), dim3(256), 0, s, (const uint32_t*)c->mt_state, c->mt_raw, kMtRawBlocks);
    hipLaunchKernelGGL(sf_mt_jump_partial, dim3(K - 1u, kMtParts), dim3(256), 0, s, (const uint32_t*)c->mt_raw,
                       (const uint64_t*)c->mt_polys, pw, c->mt_partial);
    hipLaunchKernelGGL(sf_mt_segments, dim3(K), dim3(256), 0, s, (const uint32_t*)c->mt_state,
                       (const uint32_t*)c->mt_partial, L, n, out, c->mt_state2);
    SF_HIP(c, hipGetLastError());
    SF_HIP(c, hipMemcpyAsync(c->mt_state, c->mt_state2, 625 * 4, hipMemcpyDeviceToDevice, s));
    return SF_OK;
}

// Packet bins of a frame-less batch: squares of 2^shift pixels, about 8 packets per bin (a wave's worth of AVX
// packets), at most SF_PROG_MAX_BINS.
static void bin_geometry(const sf_ctx* c, uint32_t packets, uint32_t& shift, uint32_t& bx, uint32_t& by)
{
    for (shift = 2u;; ++shift) {
        bx = (c->W + (1u << shift) - 1u) >> shift;
        by = (c->H + (1u << shift) - 1u) >> shift;
        const uint64_t nb = (uint64_t)bx * by;
        if (nb <= SF_PROG_MAX_BINS && 8ull * nb <= packets) break;
        if (shift == 30u) break;
    }
}

// Binned trace order of `packets` packets (counting sort by bin, index order of the bins) into perm, on stream s.
static int bin_packets(sf_ctx* c, hipStream_t s, const FrameArgs& a, const uint32_t* draws, uint64_t counter0,
                       uint32_t packets, uint32_t pl, uint32_t* cnt, uint32_t* perm)
{
    uint32_t shift, bx, by;
    bin_geometry(c, packets, shift, bx, by);
    const uint32_t nbins = bx * by, pb = (packets + 255u) / 256u;
    SF_HIP(c, hipMemsetAsync(cnt, 0, (size_t)nbins * 4, s));
    hipLaunchKernelGGL(sf_packet_bin, dim3(pb), dim3(256), 0, s, a, draws, counter0, packets, pl, shift, bx, cnt);
    hipLaunchKernelGGL(sf_packet_scan, dim3(1), dim3(1024), 0, s, cnt, nbins, (const uint32_t*)nullptr);
    hipLaunchKernelGGL(sf_packet_place, dim3(pb), dim3(256), 0, s, a, draws, counter0, packets, pl, shift, bx, cnt, perm);
    SF_HIP(c, hipGetLastError());
    return SF_OK;
}

// Frame-less progressive mode (Sphereflake.cpp:67-74, 86-214). The device MT stream is kept in the
// context; a call that does not continue where the previous one stopped (other seed or counter)
// reseeds and jumps ahead by 2 * counter0 draws on the host (sfhost::mt_jump).
int sf_progressive(sf_ctx* c, uint32_t seed, uint64_t counter0, uint32_t packets, void* stream)
{
    if (!c) return SF_EINVAL;
    if (!c->has_view) return SF_ENOVIEW;
    const bool sse = c->variant == SF_VARIANT_SSE;
    const uint32_t pl = sse ? 4u : 8u;             // packet lanes (SIMD_SSE.h / SIMD_AVX.h)
    // the AVX worker samples x0 in [1, W-2], the SSE worker x0 in [0, W-2] (Sphereflake.cpp:117-118, 140-141)
    if (sse ? (c->W < 2 || c->H < 2) : (c->W < 3 || c->H < 3)) return SF_EINVAL;
    if (packets == 0) return SF_OK;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    DevGuard g(c->device);
    if (int rc = ctx_join(c, s)) return rc;
    StreamMark mark_(c, s);
    if (!c->mt_state) {
        SF_HIP(c, hipMalloc(&c->mt_state, 625 * 4));
        SF_HIP(c, hipMalloc(&c->owner, (size_t)c->W * c->H * 8));
        SF_HIP(c, hipMemsetAsync(c->owner, 0, (size_t)c->W * c->H * 8, s));
    }
    // a pending prefetch either is this batch's draws, or is undone (MT state restored)
    bool prefetched = false, prebinned = false;
    const bool binned = c->prog_bin && packets >= SF_PROG_BIN_MIN;
    if (c->pf_packets) {
        SF_HIP(c, hipStreamWaitEvent(s, c->pf_done, 0));
        if (c->pf_packets == packets && c->prog_seeded && seed == c->prog_seed && counter0 == c->prog_next) {
            std::swap(c->draws, c->draws_pf);
            prefetched = true;
            if (binned && !c->prog_order && c->pf_bin_pl == pl) {
                std::swap(c->perm, c->perm_pf);
                prebinned = true;
            }
        } else {
            SF_HIP(c, hipMemcpyAsync(c->mt_state, c->mt_saved, 625 * 4, hipMemcpyDeviceToDevice, s));
        }
        c->pf_packets = 0;
    }
    if (packets > c->prog_cap) {
        (void)hipStreamSynchronize(s);
        (void)hipFree(c->draws);
        (void)hipFree(c->draws_pf);
        (void)hipFree(c->lanes);
        (void)hipFree(c->perm);
        (void)hipFree(c->perm_pf);
        c->perm_pf = nullptr;
        (void)hipFree(c->prog_ovf);
        c->draws = c->draws_pf = nullptr;
        c->lanes = nullptr;
        c->perm = nullptr;
        c->prog_ovf = nullptr;
        c->prog_cap = 0;
        c->traced_valid = false;
        SF_HIP(c, hipMalloc(&c->draws, (size_t)packets * 2 * 4));
        SF_HIP(c, hipMalloc(&c->lanes, (size_t)packets * 8 * sizeof(PacketLane)));
        SF_HIP(c, hipMalloc(&c->perm, (size_t)packets * 4));
        SF_HIP(c, hipMalloc(&c->prog_ovf, ((size_t)packets + 3) / 4 * 4));   // >= one entry per wave
        c->prog_cap = packets;
    }
    if (!c->prog_seeded || seed != c->prog_seed || counter0 != c->prog_next) {
        uint32_t st[625], sj[625];
        sfhost::mt19937_seed(seed, st);
        sfhost::mt_jump(st, 2 * counter0, sj);   // the stream 2 * counter0 draws on (2 per packet)
        SF_HIP(c, hipMemcpyAsync(c->mt_state, sj, sizeof sj, hipMemcpyHostToDevice, s));
        SF_HIP(c, hipStreamSynchronize(s));
        c->prog_seeded = true;
        c->prog_seed = seed;
    }
    FrameArgs a = frame_args(c);
    a.pos = c->pos;
    a.nrm = c->nrm;
    a.min_t = c->min_t;
    a.emit_aux = 1;
    a.packet_lanes = pl;
    if (c->flags & SF_FLAG_DIAG_UNITS) a.tile_trace = c->tile_trace;   // per-wave diagnostics (sf_set_tile_trace)
    if (!prefetched)
        if (int rc = gen_draws(c, s, c->draws, 2 * packets)) return rc;
    // Prefetch the next batch's draws (a continuing stream of the same batch size) on pf_stream, into
    // the buffer the previous batch traced from, overlapped with this batch's trace.
    if (c->prog_prefetch && packets >= SF_PROG_PREFETCH_MIN) {
        if (!c->pf_stream) {
            if (c->pf_prio) {   // (a stream of the device's greatest priority: a hardware queue of its own)
                int least = 0, greatest = 0;
                SF_HIP(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
                SF_HIP(c, hipStreamCreateWithPriority(&c->pf_stream, hipStreamNonBlocking, greatest));
            } else {
                SF_HIP(c, hipStreamCreateWithFlags(&c->pf_stream, hipStreamNonBlocking));
            }
            SF_HIP(c, hipEventCreateWithFlags(&c->pf_done, hipEventDisableTiming));
            SF_HIP(c, hipEventCreateWithFlags(&c->mt_ready, hipEventDisableTiming));
            SF_HIP(c, hipEventCreateWithFlags(&c->traced, hipEventDisableTiming));
            SF_HIP(c, hipMalloc(&c->mt_saved, 625 * 4));
        }
        if (!c->draws_pf) SF_HIP(c, hipMalloc(&c->draws_pf, (size_t)c->prog_cap * 2 * 4));
        SF_HIP(c, hipEventRecord(c->mt_ready, s));                 // MT state advanced past this batch
        SF_HIP(c, hipStreamWaitEvent(c->pf_stream, c->mt_ready, 0));
        if (c->traced_valid) SF_HIP(c, hipStreamWaitEvent(c->pf_stream, c->traced, 0));   // draws_pf free
        SF_HIP(c, hipMemcpyAsync(c->mt_saved, c->mt_state, 625 * 4, hipMemcpyDeviceToDevice, c->pf_stream));
        if (int rc = gen_draws(c, c->pf_stream, c->draws_pf, 2 * packets)) return rc;
        // the next batch's binned order too (index-ordered bins only: a cost-ranked order needs this batch's costs)
        c->pf_bin_pl = 0;
        if (binned && !c->prog_order) {
            if (!c->perm_pf) SF_HIP(c, hipMalloc(&c->perm_pf, (size_t)c->prog_cap * 4));
            if (!c->bin_cnt_pf) SF_HIP(c, hipMalloc(&c->bin_cnt_pf, SF_PROG_MAX_BINS * 4));
            if (int rc = bin_packets(c, c->pf_stream, a, c->draws_pf, counter0 + packets, packets, pl, c->bin_cnt_pf,
                                     c->perm_pf))
                return rc;
            c->pf_bin_pl = pl;
        }
        SF_HIP(c, hipEventRecord(c->pf_done, c->pf_stream));
        c->pf_packets = packets;
    }
    // Trace order: packets binned by a square of 2^shift pixels (about 8 per bin, a wave's worth of
    // AVX packets), so a wave's packets share their traversal. Small batches: draw order.
    const uint32_t* perm = nullptr;
    if (prebinned) {   // (binned on pf_stream with the draws)
        perm = c->perm;
    } else if (binned) {
        if (!c->bin_cnt) SF_HIP(c, hipMalloc(&c->bin_cnt, SF_PROG_MAX_BINS * 4));
        uint32_t shift, bx, by;
        bin_geometry(c, packets, shift, bx, by);
        const uint32_t nbins = bx * by;
        const uint32_t pb = (packets + 255u) / 256u;
        // Heavy-first: bins ranked by the cycles their waves took in the previous batch of the same
        // binning (the view and the bins do not move between batches); the trace grid then starts with
        // the heaviest packets instead of meeting them wherever their screen region falls.
        const uint32_t* rank = nullptr;
        if (c->prog_order) {
            const uint32_t nc = (nbins + 63u) / 64u;
            const uint32_t key = (shift << 24) | nbins;
            if (!c->bin_cost) {
                const size_t nc_max = (SF_PROG_MAX_BINS + 63u) / 64u;
                SF_HIP(c, hipMalloc(&c->bin_cost, SF_PROG_MAX_BINS * 4));
                SF_HIP(c, hipMalloc(&c->bin_rank, SF_PROG_MAX_BINS * 4));
                SF_HIP(c, hipMalloc(&c->bin_order, SF_PROG_MAX_BINS * 4));
                SF_HIP(c, hipMalloc(&c->bin_chunk_cnt, nc_max * SF_ORDER_BUCKETS * 4));
                SF_HIP(c, hipMalloc(&c->bin_chunk_off, nc_max * SF_ORDER_BUCKETS * 4));
                SF_HIP(c, hipMalloc(&c->bin_meta, 4 * 4));
            }
            if (c->bin_key == key) {
                hipLaunchKernelGGL(sf_bin_hist, dim3(nc), dim3(64), 0, s, (const uint32_t*)c->bin_cost, nbins,
                                   c->bin_chunk_cnt);
                hipLaunchKernelGGL(sf_order_scan, dim3(1), dim3(1024), 0, s, c->bin_chunk_cnt, nc, nbins,
                                   0u, 2u, 0u, 0u, 0u, c->bin_chunk_off, c->bin_meta, (const uint32_t*)nullptr,
                                   (uint32_t*)nullptr, 0xffffffffu);
                hipLaunchKernelGGL(sf_order_scatter, dim3(nc), dim3(64), 0, s, (const uint32_t*)c->bin_cost, nbins,
                                   c->bin_chunk_cnt, (const uint32_t*)c->bin_chunk_off, (const uint32_t*)c->bin_meta,
                                   c->bin_order, c->bin_rank);
                SF_HIP(c, hipGetLastError());
                rank = c->bin_rank;
            } else {   // new binning: no costs yet (this batch records them)
                SF_HIP(c, hipMemsetAsync(c->bin_cost, 0, SF_PROG_MAX_BINS * 4, s));
                c->bin_key = key;
            }
            a.bin_cost = c->bin_cost;
            a.bin_shift = shift;
            a.bins_x = bx;
        }
        SF_HIP(c, hipMemsetAsync(c->bin_cnt, 0, (size_t)nbins * 4, s));
        hipLaunchKernelGGL(sf_packet_bin, dim3(pb), dim3(256), 0, s, a, (const uint32_t*)c->draws, counter0, packets,
                           pl, shift, bx, c->bin_cnt);
        hipLaunchKernelGGL(sf_packet_scan, dim3(1), dim3(1024), 0, s, c->bin_cnt, nbins, rank);
        hipLaunchKernelGGL(sf_packet_place, dim3(pb), dim3(256), 0, s, a, (const uint32_t*)c->draws, counter0, packets,
                           pl, shift, bx, c->bin_cnt, c->perm);
        SF_HIP(c, hipGetLastError());
        perm = c->perm;
    }
    const uint32_t ppw = 64u / pl;                   // packets per wave
    const uint32_t waves = (packets + ppw - 1) / ppw;
    uint32_t levels = SF_PROGRESSIVE_LEVELS;
    if (c->prog_adapt) {
        if (!c->h_prog_depth) {
            SF_HIP(c, hipHostMalloc(&c->h_prog_depth, 4, hipHostMallocDefault));
            *c->h_prog_depth = -1;
            SF_HIP(c, hipMalloc(&c->prog_ovf_cnt, 2 * 4));
            SF_HIP(c, hipMemsetAsync(c->prog_ovf_cnt, 0, 2 * 4, s));
        }
        const int32_t seen = *(volatile int32_t*)c->h_prog_depth;   // max depth of a finished batch
        if (seen >= 0 && (uint32_t)seen + 1u < levels) levels = (uint32_t)seen + 1u < 4u ? 4u : (uint32_t)seen + 1u;
    }
    const bool adaptive = levels < SF_PROGRESSIVE_LEVELS;
    uint32_t* ovf_cnt = adaptive ? c->prog_ovf_cnt + c->prog_par : nullptr;
    const size_t lds = (size_t)SF_LDS_WAVE_FLOATS(levels) * 4;
    if (sse)
        hipLaunchKernelGGL(sf_progressive_trace_sse, dim3(waves), dim3(64), lds, s, a, (const uint32_t*)c->draws,
                           counter0, packets, c->ticket, c->lanes, c->owner, perm, levels,
                           adaptive ? c->prog_ovf : nullptr, ovf_cnt);
    else
        hipLaunchKernelGGL(sf_progressive_trace, dim3(waves), dim3(64), lds, s, a, (const uint32_t*)c->draws,
                           counter0, packets, c->ticket, c->lanes, c->owner, perm, levels,
                           adaptive ? c->prog_ovf : nullptr, ovf_cnt);
    SF_HIP(c, hipGetLastError());
    if (adaptive) {   // re-trace the waves that needed more levels (reads this batch's list, zeroes the next)
        const size_t lds_fix = (size_t)SF_LDS_WAVE_FLOATS(SF_PROGRESSIVE_LEVELS) * 4;
        const dim3 fg(SF_PROG_FIXUP_BLOCKS);
        if (sse)
            hipLaunchKernelGGL(sf_progressive_fixup_sse, fg, dim3(64), lds_fix, s, a, (const uint32_t*)c->draws,
                               counter0, packets, c->ticket, c->lanes, c->owner, perm, (const uint32_t*)c->prog_ovf,
                               c->prog_ovf_cnt, c->prog_par);
        else
            hipLaunchKernelGGL(sf_progressive_fixup, fg, dim3(64), lds_fix, s, a, (const uint32_t*)c->draws,
                               counter0, packets, c->ticket, c->lanes, c->owner, perm, (const uint32_t*)c->prog_ovf,
                               c->prog_ovf_cnt, c->prog_par);
        SF_HIP(c, hipGetLastError());
        c->prog_par ^= 1u;
    }
    if (c->pf_stream) {   // the next prefetch may overwrite this batch's draws after this point
        SF_HIP(c, hipEventRecord(c->traced, s));
        c->traced_valid = true;
    }
    hipLaunchKernelGGL(sf_progressive_scatter, dim3((packets * pl + 255) / 256), dim3(256), 0, s, a, packets, c->ticket,
                       (const PacketLane*)c->lanes, (const unsigned long long*)c->owner);
    SF_HIP(c, hipGetLastError());
    if (c->prog_adapt) SF_HIP(c, hipMemcpyAsync(c->h_prog_depth, c->stats, 4, hipMemcpyDeviceToHost, s));
    c->ticket += packets;
    c->prog_next = counter0 + packets;
    c->rays += (int64_t)pl * packets;                // m_RaysPerSecond += 8 / 4 (Sphereflake.cpp:184-186)
    return SF_OK;
}

// The stats words ride the stream in a small copy to pinned memory, queued behind the context's work, so the host
// waits once (a synchronous hipMemcpy after the drain was a second round trip, ~10-20 us per call: per slot of a
// dist, at the end of every timed loop and every lone frame); a context with nothing enqueued since the last call
// only drains, and so does one whose work since then was only persistent traces that cannot add to the unresolved
// word (round 5: the copy was a blit dispatch of ~4 us behind every lone frame's trace, plus its launch gap).
int sf_synchronize(sf_ctx* c)
{
    if (!c) return SF_EINVAL;
    // nothing enqueued since the last check (every call that enqueues work joins first, ctx_join): no runtime
    // call at all -- a multi-slot caller (sf_dist_synchronize) waits only for the slots that have work
    if (!c->stats_dirty) return c->unresolved != 0 ? SF_EDEPTH : SF_OK;
    DevGuard g(c->device);
    // (after only traces that cannot change the unresolved word, the last check's value stands: no copy)
    const bool check = c->stats_dirty && c->stats_unknown;
    if (check) {
        if (int rc_ = ctx_join(c, c->stream)) return rc_;
        SF_HIP(c, hipMemcpyAsync(c->h_stats, c->stats, 12, hipMemcpyDeviceToHost, c->stream));
    }
    if (int rc_ = ctx_drain(c)) return rc_;
    c->stats_dirty = false;
    c->stats_unknown = false;
    if (check) c->unresolved = ((volatile int32_t*)c->h_stats)[2];
    if (c->unresolved != 0) return SF_EDEPTH;
    return SF_OK;
}

int sf_download(sf_ctx* c, float* pos4, float* nrm4, float* min_t, uint32_t* hidx)
{
    if (!c) return SF_EINVAL;
    int rc = sf_synchronize(c);
    if (rc != SF_OK) return rc;
    DevGuard g(c->device);
    const size_t npx = (size_t)c->W * c->H;
    if (pos4) SF_HIP(c, hipMemcpy(pos4, c->pos, npx * 16, hipMemcpyDeviceToHost));
    if (nrm4) SF_HIP(c, hipMemcpy(nrm4, c->nrm, npx * 16, hipMemcpyDeviceToHost));
    if (min_t) SF_HIP(c, hipMemcpy(min_t, c->min_t, npx * 4, hipMemcpyDeviceToHost));
    if (hidx) SF_HIP(c, hipMemcpy(hidx, c->hit_index, npx * 4, hipMemcpyDeviceToHost));
    return SF_OK;
}

// Transfer/interop: stream-ordered D2H into host memory. With page-locked
// destinations (sf_host_register) the copy runs at PCIe DMA rate and overlaps
// whatever the host does until sf_synchronize (context stream) or the caller syncs `stream`.
int sf_download_async(sf_ctx* c, float* pos4, float* nrm4, float* min_t, uint32_t* hidx, void* stream)
{
    if (!c) return SF_EINVAL;
    DevGuard g(c->device);
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const size_t npx = (size_t)c->W * c->H;
    if (int rc = ctx_join(c, s)) return rc;
    StreamMark mark_(c, s);
    if (pos4) SF_HIP(c, hipMemcpyAsync(pos4, c->pos, npx * 16, hipMemcpyDeviceToHost, s));
    if (nrm4) SF_HIP(c, hipMemcpyAsync(nrm4, c->nrm, npx * 16, hipMemcpyDeviceToHost, s));
    if (min_t) SF_HIP(c, hipMemcpyAsync(min_t, c->min_t, npx * 4, hipMemcpyDeviceToHost, s));
    if (hidx) SF_HIP(c, hipMemcpyAsync(hidx, c->hit_index, npx * 4, hipMemcpyDeviceToHost, s));
    return SF_OK;
}

int sf_host_register(void* ptr, size_t bytes)
{
    if (!ptr || !bytes) return SF_EINVAL;
    return hipHostRegister(ptr, bytes, hipHostRegisterDefault) == hipSuccess ? SF_OK : SF_EHIP;
}

int sf_host_unregister(void* ptr)
{
    if (!ptr) return SF_EINVAL;
    return hipHostUnregister(ptr) == hipSuccess ? SF_OK : SF_EHIP;
}

int sf_post_defaults(const sf_ctx* c, sf_post_params* p)
{
    if (!c || !p) return SF_EINVAL;
    std::memset(p, 0, sizeof *p);
    p->sample_radius = -1.0f;
    p->intensity = 0.51f;
    p->scale = 3.28f;
    p->bias = 0.23f;
    p->normal_threshold = 2.47f;
    p->depth_threshold = 0.01f;
    std::memcpy(p->camera_position, c->o, 12);
    p->downscale = 1;
    return SF_OK;
}

int sf_ssao_noise(float* out)
{
    if (!out) return SF_EINVAL;
    sfhost::ssao_noise(out);
    return SF_OK;
}

int sf_post_process(sf_ctx* c, const sf_post_params* prm, const float* pos4, const float* nrm4, uint8_t* rgba,
                    uint8_t* ao)
{
    if (!c || !prm || prm->downscale == 0) return SF_EINVAL;
    const uint32_t aw = c->W / prm->downscale, ah = c->H / prm->downscale;
    if (aw == 0 || ah == 0) return SF_EINVAL;
    DevGuard g(c->device);
    hipStream_t s = prm->stream ? (hipStream_t)prm->stream : c->stream;
    const size_t npx = (size_t)c->W * c->H;
    if (int rc = ctx_join(c, s)) return rc;
    StreamMark mark_(c, s);
    if (!c->noise) {
        static float host_noise[SF_NOISE_SIZE * SF_NOISE_SIZE * 4];
        sfhost::ssao_noise(host_noise);
        SF_HIP(c, hipMalloc(&c->noise, sizeof host_noise));
        SF_HIP(c, hipMemcpy(c->noise, host_noise, sizeof host_noise, hipMemcpyHostToDevice));
    }
    if (!c->image) SF_HIP(c, hipMalloc(&c->image, npx * 4));
    if (c->centre_exact < 0) c->centre_exact = sfhost::post_centre_exact(c->W) && sfhost::post_centre_exact(c->H);
    // Fusion is exact when no blur tap can be accepted: every |n| <= 1.004 (the tracer's normals are
    // rsqrtps-normalised, |n| - 1 < 2^-11) bounds dot(n, n') < 1.01 <= normalThreshold
    const bool own_gbuffer = (!pos4 || pos4 == c->pos) && (!nrm4 || nrm4 == c->nrm);
    const bool fused = !(prm->flags & SF_POST_GENERAL) && prm->downscale == 1 && c->centre_exact &&
                       prm->normal_threshold >= 1.01f && (own_gbuffer || (prm->flags & SF_POST_UNIT_NORMALS));
    if (!fused) {
        if (c->post_ao_px < (size_t)aw * ah) {
            SF_HIP(c, hipFree(c->ao));
            c->ao = nullptr;
            SF_HIP(c, hipMalloc(&c->ao, (size_t)aw * ah));
            c->post_ao_px = (size_t)aw * ah;
        }
        if (!c->blur_h) SF_HIP(c, hipMalloc(&c->blur_h, npx));
        if (!c->blur_v) SF_HIP(c, hipMalloc(&c->blur_v, npx));
    }
    PostArgs a;
    std::memset(&a, 0, sizeof a);
    a.W = c->W;
    a.H = c->H;
    a.aw = aw;
    a.ah = ah;
    a.fw = (float)c->W;
    a.fh = (float)c->H;
    a.faw = (float)aw;
    a.fah = (float)ah;
    // uniform reciprocals, correctly rounded here once instead of per fragment (the same IEEE division)
    a.rfw = 1.0f / a.fw;
    a.rfh = 1.0f / a.fh;
    a.rfaw = 1.0f / a.faw;
    a.rfah = 1.0f / a.fah;
    a.pos = pos4 ? pos4 : c->pos;
    a.nrm = nrm4 ? nrm4 : c->nrm;
    a.noise = c->noise;
    a.stats = c->stats;
    a.radius = prm->sample_radius;
    a.intensity = prm->intensity;
    a.scale = prm->scale;
    a.bias = prm->bias;
    a.normal_thr = prm->normal_threshold;
    a.depth_thr = prm->depth_threshold;
    std::memcpy(a.cam, prm->camera_position, 12);
    a.rgba = rgba ? rgba : c->image;
    const dim3 blk(256);
    const dim3 grid((c->W + 15) / 16, (c->H + 15) / 16);
    if (fused) {
        a.ao = ao;
        hipLaunchKernelGGL(sf_post_fused, grid, blk, 0, s, a);
    } else {
        a.ao = ao ? ao : c->ao;
        a.blur_h = c->blur_h;
        a.blur_v = c->blur_v;
        hipLaunchKernelGGL(sf_post_ssao, dim3((aw + 15) / 16, (ah + 15) / 16), blk, 0, s, a);
        hipLaunchKernelGGL(sf_post_blur, grid, blk, 0, s, a, 0u);
        hipLaunchKernelGGL(sf_post_blur, grid, blk, 0, s, a, 1u);
        hipLaunchKernelGGL(sf_post_final, grid, blk, 0, s, a);
    }
    SF_HIP(c, hipGetLastError());
    return SF_OK;
}

int sf_download_image(sf_ctx* c, uint8_t* rgba)
{
    if (!c || !rgba) return SF_EINVAL;
    if (!c->image) return SF_ESTATE;
    int rc = sf_synchronize(c);
    if (rc != SF_OK) return rc;
    DevGuard g(c->device);
    SF_HIP(c, hipMemcpy(rgba, c->image, (size_t)c->W * c->H * 4, hipMemcpyDeviceToHost));
    return SF_OK;
}

int sf_set_variant(sf_ctx* c, int variant)
{
    if (!c || (variant != SF_VARIANT_AVX && variant != SF_VARIANT_SSE)) return SF_EINVAL;
    if (variant == c->variant) return SF_OK;
    DevGuard g(c->device);
    if (int rc_ = ctx_drain(c)) return rc_;
    c->variant = variant;
    c->order_n = 0;       // tile costs of the other variant's frames: start over
    *c->h_depth = -1;     // level hint likewise
    return upload_consts(c);
}

int sf_get_variant(const sf_ctx* c) { return c ? c->variant : SF_EINVAL; }

int sf_set_tile_trace(sf_ctx* c, int enable)
{
    if (!c) return SF_EINVAL;
    DevGuard g(c->device);
    if (int rc_ = ctx_drain(c)) return rc_;
    if (!enable) {
        (void)hipFree(c->tile_trace);
        c->tile_trace = nullptr;
        return SF_OK;
    }
    if (!c->tile_trace) {
        const size_t ntiles = (size_t)((c->W + 7) / 8) * ((c->H + 7) / 8);
        // per tile {start, end, id}, the diagnostic slots, per work unit {start, end, unit} (<= 4 per tile),
        // per wave {start, end}
        SF_HIP(c, hipMalloc(&c->tile_trace, SF_TRACE_WORDS(ntiles) * 8));
        SF_HIP(c, hipMemset(c->tile_trace, 0, SF_TRACE_WORDS(ntiles) * 8));
    }
    return SF_OK;
}

int sf_get_tile_trace(sf_ctx* c, uint64_t* out, size_t n)
{
    if (!c || !out || !c->tile_trace) return SF_EINVAL;
    DevGuard g(c->device);
    const size_t ntiles = (size_t)((c->W + 7) / 8) * ((c->H + 7) / 8);
    if (n < ntiles * 3) return SF_EINVAL;
    if (int rc_ = ctx_drain(c)) return rc_;
    // n >= 3 * tiles + SF_DIAG_SLOTS also returns the segment sums / event counts of the diagnostic
    // builds (zeros otherwise); n >= SF_TRACE_WORDS(tiles) the per-unit and per-wave records too
    const size_t full = SF_TRACE_WORDS(ntiles);
    SF_HIP(c, hipMemcpy(out, c->tile_trace, (n >= full ? full : n >= ntiles * 3 + SF_DIAG_SLOTS ? ntiles * 3 + SF_DIAG_SLOTS : ntiles * 3) * 8,
                        hipMemcpyDeviceToHost));
    return SF_OK;
}

int sf_get_tile_order(sf_ctx* c, uint32_t* order, uint32_t* cost, size_t n)
{
    if (!c) return SF_EINVAL;
    DevGuard g(c->device);
    const size_t ntiles = (size_t)((c->W + 7) / 8) * ((c->H + 7) / 8);
    if (n < ntiles || (!order && !cost)) return SF_EINVAL;
    if (int rc_ = ctx_drain(c)) return rc_;
    if (c->order_n == 0u) return 0;   // (a band share's order covers its own c->order_n tiles)
    uint32_t meta[2];
    SF_HIP(c, hipMemcpy(meta, c->order_meta, sizeof(meta), hipMemcpyDeviceToHost));
    if (order && n < meta[0]) return SF_EINVAL;
    if (order) SF_HIP(c, hipMemcpy(order, c->tile_order, (size_t)meta[0] * 4, hipMemcpyDeviceToHost));
    if (cost) SF_HIP(c, hipMemcpy(cost, c->tile_cost, (size_t)c->order_n * 4, hipMemcpyDeviceToHost));
    return (int)meta[0];
}

void* sf_context_stream(sf_ctx* c) { return c ? (void*)c->stream : nullptr; }
uint32_t sf_lean_launches(const sf_ctx* c) { return c ? c->lean_launches : 0u; }
uint32_t sf_pair_launches(const sf_ctx* c) { return c ? c->pair_launches : 0u; }
uint32_t sf_order_units(const sf_ctx* c) { return c ? c->order_n : 0u; }

int sf_device_buffers(sf_ctx* c, float** pos4, float** nrm4, float** min_t, uint32_t** hidx)
{
    if (!c) return SF_EINVAL;
    if (pos4) *pos4 = c->pos;
    if (nrm4) *nrm4 = c->nrm;
    if (min_t) *min_t = c->min_t;
    if (hidx) *hidx = c->hit_index;
    return SF_OK;
}

int sf_set_kernel_timing(sf_ctx* c, int enable)
{
    if (!c) return SF_EINVAL;
    DevGuard g(c->device);
    if (enable && !c->ev[0][0]) {
        for (int i = 0; i < sf_ctx::kTimed; ++i)
            for (int j = 0; j < 2; ++j) SF_HIP(c, hipEventCreate(&c->ev[i][j]));
        const size_t cb = (size_t)sf_ctx::kTimed * SF_CLOCK_WAVES * 4u * 8u;
        SF_HIP(c, hipMalloc(&c->clock_buf, cb));
        SF_HIP(c, hipMemset(c->clock_buf, 0, cb));
    }
    if (enable < 0) return SF_EINVAL;
    c->timing = enable != 0;
    c->ev_period = enable > 0 ? (uint32_t)enable : 1u;
    c->ev_next = c->ev_count = c->ev_phase = 0;
    return SF_OK;
}

int sf_kernel_times(sf_ctx* c, float* ms, uint32_t n)
{
    if (!c || !ms) return SF_EINVAL;
    DevGuard g(c->device);
    if (int rc_ = ctx_drain(c)) return rc_;
    const uint32_t k = n < c->ev_count ? n : c->ev_count;
    for (uint32_t i = 0; i < k; ++i) {   // the k most recent, oldest first
        const uint32_t slot = (c->ev_next + sf_ctx::kTimed - k + i) % sf_ctx::kTimed;
        SF_HIP(c, hipEventSynchronize(c->ev[slot][1]));
        SF_HIP(c, hipEventElapsedTime(&ms[i], c->ev[slot][0], c->ev[slot][1]));
    }
    return (int)k;
}

int sf_kernel_clocks(sf_ctx* c, float* mhz, uint32_t n)
{
    if (!c || !mhz) return SF_EINVAL;
    DevGuard g(c->device);
    if (int rc_ = ctx_drain(c)) return rc_;
    const uint32_t k = n < c->ev_count ? n : c->ev_count;
    if (k == 0 || !c->clock_buf) return 0;
    static_assert(SF_CLOCK_WAVES == 8u, "median below assumes 8 records");
    uint64_t rec[SF_CLOCK_WAVES * 4];
    for (uint32_t i = 0; i < k; ++i) {   // the k most recent timed renders, oldest first (as sf_kernel_times)
        const uint32_t slot = (c->ev_next + sf_ctx::kTimed - k + i) % sf_ctx::kTimed;
        SF_HIP(c, hipMemcpy(rec, c->clock_buf + (size_t)slot * SF_CLOCK_WAVES * 4u, sizeof rec, hipMemcpyDeviceToHost));
        float v[SF_CLOCK_WAVES];
        uint32_t m = 0;
        for (uint32_t w = 0; w < SF_CLOCK_WAVES; ++w) {
            const uint64_t* r = rec + 4u * w;
            if (r[3] > r[1] && r[2] > r[0]) v[m++] = (float)((double)(r[2] - r[0]) / (double)(r[3] - r[1]) * 100.0);
        }
        for (uint32_t a = 1; a < m; ++a)   // (insertion sort of <= 8 values)
            for (uint32_t b = a; b > 0 && v[b - 1] > v[b]; --b) std::swap(v[b - 1], v[b]);
        mhz[i] = m ? (m & 1u ? v[m / 2] : 0.5f * (v[m / 2 - 1] + v[m / 2])) : 0.0f;
    }
    return (int)k;
}

int sf_get_stats(sf_ctx* c, sf_stats* out)
{
    if (!c || !out) return SF_EINVAL;
    DevGuard g(c->device);
    if (int rc_ = ctx_drain(c)) return rc_;
    int32_t st[3];
    SF_HIP(c, hipMemcpy(st, c->stats, 12, hipMemcpyDeviceToHost));
    out->max_depth = st[0] < 0 ? 0 : st[0];
    out->closest = sf_key_float(st[1]);
    out->rays = c->rays;
    out->overflow_tiles = st[2];
    if (c->dirs_cnt) {   // plus the groups of direction traces that were re-traced (sf_trace_dirs_to)
        uint32_t re = 0;
        SF_HIP(c, hipMemcpy(&re, c->dirs_cnt + 2, 4, hipMemcpyDeviceToHost));
        out->overflow_tiles += re;
    }
    return SF_OK;
}

int sf_reset_max_depth(sf_ctx* c)
{
    if (!c) return SF_EINVAL;
    DevGuard g(c->device);
    return reset_stats_dev(c, 1);
}

int sf_reset_rays(sf_ctx* c)
{
    if (!c) return SF_EINVAL;
    c->rays = 0;
    return SF_OK;
}

int sf_reset_closest(sf_ctx* c)
{
    if (!c) return SF_EINVAL;
    DevGuard g(c->device);
    return reset_stats_dev(c, 2);
}

int sf_camera_corners(uint32_t W, uint32_t H, const float pos[3], float pitch, float yaw, float roll, float fov,
                      float o[3], float tl[3], float tr[3], float bl[3])
{
    if (!W || !H || !pos || !o || !tl || !tr || !bl) return SF_EINVAL;
    sfhost::camera_corners(W, H, pos, pitch, yaw, roll, fov, o, tl, tr, bl);
    return SF_OK;
}

int sf_child_transforms(float child[9][16])
{
    if (!child) return SF_EINVAL;
    sfhost::child_transforms(child);
    return SF_OK;
}

int sf_root_transform(const float origin[3], float root[16])
{
    if (!origin || !root) return SF_EINVAL;
    sfhost::root_transform(origin, root);
    return SF_OK;
}

int sf_lod_threshold(float r, float lod_constant, float* T)
{
    if (!T || !(r > 0.0f) || !(lod_constant > 0.0f)) return SF_EINVAL;
    *T = sfhost::lod_threshold(r, lod_constant);
    return SF_OK;
}

int sf_division_by_reciprocal_exact(uint32_t n)
{
    return sfhost::division_by_reciprocal_exact(n) ? 1 : 0;
}

int sf_depth_constants(uint32_t depth, float* radius, float* lod)
{
    if (depth >= SF_DEPTH_TABLE) return SF_EINVAL;
    float r = sfhost::radius(depth);
    if (radius) *radius = r;
    if (lod) *lod = sfhost::lod_threshold(r);
    return SF_OK;
}

int sf_mt19937_jump(const uint32_t state_in[625], uint64_t outputs, uint32_t state_out[625])
{
    if (!state_in || !state_out) return SF_EINVAL;
    sfhost::mt_jump(state_in, outputs, state_out);
    return SF_OK;
}

float sf_rsqrtps(float x)
{
    uint32_t b;
    std::memcpy(&b, &x, 4);
    uint32_t E = (b >> 23) & 0xffu;
    uint32_t r;
    if ((b & 0x7fffffffu) > 0x7f800000u) r = b | 0x00400000u;
    else if (E == 0u) r = (b & 0x80000000u) | 0x7f800000u;
    else if (b & 0x80000000u) r = 0xffc00000u;
    else if (E == 0xffu) r = 0u;
    else {
        uint32_t key = ((E & 1u) << 10) | ((b & 0x7fffffu) >> 13);
        int32_t E0 = (E & 1u) ? 127 : 128;
        int32_t k = ((int32_t)E - E0) / 2;
        r = (uint32_t)((int32_t)kLut[key] - k * (1 << 23));
    }
    float f;
    std::memcpy(&f, &r, 4);
    return f;
}

}  // extern "C"
