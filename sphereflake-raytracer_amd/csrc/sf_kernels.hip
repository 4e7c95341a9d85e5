// sf_kernels.hip -- gfx950 (CDNA4) kernels of the Sphereflake primary-ray G-buffer renderer.
//
// Hot path replaced (reference paths relative to /root/reference):
//   ray generation           sphereflake/Sphereflake.cpp:149-150,162-167
//   recursive traversal      sphereflake/Sphereflake.h:86-226 (IntersectSphereflake)
//   packet math              sphereflake/SIMD_AVX.h:59-81 (4x4 product), 163-180 (Dot/Normalize),
//                            236-270 (RaySphereIntersection)
//   G-buffer scatter         sphereflake/Sphereflake.cpp:186-201
//   frame-less sampler       sphereflake/Sphereflake.cpp:86-214, Sobol.cpp:41-55
//
// Numerics: IEEE binary32, the reference's exact operation order, contraction OFF (this file
// and the compile line), correctly rounded division and sqrt (HIP default), denormals kept,
// x86 rsqrtps reproduced from a table. Full frames equal the reference AVX path bit for bit
// under per-ray semantics; the progressive mode reproduces the reference's
// 8-ray packet semantics (packet-wide early-outs, Sphereflake.h:140-153, 207-211,
// SIMD_AVX.h:247-258) bit for bit.
//
// Kernels
//   sf_trace_queue2 -- the product kernel (full frames): a persistent grid of 2-wave workgroups; each wave64
//                      traces one 8x8 pixel tile (or a part of one) per work unit, taken from the previous
//                      render's heavy-first unit order (static first unit, then its block group's atomic
//                      queue). The DFS over the sphereflake is wave-uniform: a node is visited iff at least
//                      one lane of the tile visits it, and each lane keeps exactly its own per-ray visit
//                      semantics through lane masks. When a node expands, 36 lanes build its 9 child
//                      transforms cooperatively (one 4-float column each) into the wave's LDS level,
//                      instead of every ray doing 9 4x4 products per node as the reference packets do.
//                      sf_trace_queue1g/4: 1 / 4 waves per workgroup; sf_trace_queue2c / 1s: the opt-in
//                      active-ray compaction and subtree-split units; sf_trace_queue1t: the lean loop over whole
//                      tiles of one plain frame; sf_trace_queue1 (and 1c, which records unit costs): the lean loop
//                      over pair units, two adjacent tiles per wave (traverse_pair).
//   sf_order_scan / sf_order_scatter -- the next render's unit order from this render's tile costs.
//   sf_trace_wave{1,2,4} -- the same traversal, one workgroup per tile group (non-persistent A/B path).
//   sf_fixup_wave   -- re-traces the tiles flagged as needing more LDS levels than provisioned, with
//                      SF_MAX_LEVELS levels, and those with an exact tie under the front-first child order,
//                      in index order.
//   sf_trace_ray    -- one thread per ray with a private traversal stack (the straightforward
//                      formulation; cross-check and comparison point).
//   sf_band_unpack  -- packed band slabs of a multi-GPU frame -> the G-buffer at frame positions.
//   sf_mt_draws / sf_packet_* / sf_progressive_* -- frame-less progressive mode.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stddef.h>
#include <stdint.h>

#include "sf_internal.h"
#include "sf_rootforms.h"

#pragma clang fp contract(off)

#define SF_MAX_LEVELS 31         // SF_MAX_DEPTH_LIMIT (ebits is 32 bits)

namespace {

// Wave64 ballot straight on the compare mask (no bool -> int -> compare round trip).
__device__ __forceinline__ uint64_t wave_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }

// x86 rsqrtps (SIMD_AVX.h:173), reproduced exactly from the measured table.
__device__ __forceinline__ float rsqrtps_x86(float x, const uint32_t* __restrict__ lut)
{
    const uint32_t b = __float_as_uint(x);
    const uint32_t E = (b >> 23) & 0xffu;
    const uint32_t key = ((E & 1u) << 10) | ((b & 0x7fffffu) >> 13);
    const int32_t E0 = (E & 1u) ? 127 : 128;
    const int32_t k = ((int32_t)E - E0) / 2;
    uint32_t r = (uint32_t)((int32_t)lut[key] - k * (1 << 23));
    if ((b & 0x7fffffffu) > 0x7f800000u) r = b | 0x00400000u;     // NaN -> quiet NaN
    else if (E == 0u) r = (b & 0x80000000u) | 0x7f800000u;        // +-0 / denormal -> +-inf
    else if (b & 0x80000000u) r = 0xffc00000u;                    // negative -> default NaN
    else if (E == 0xffu) r = 0u;                                  // +inf -> +0
    return __uint_as_float(r);
}

// SIMD::Normalize (SIMD_AVX.h:170-180): rsqrt + one Newton-Raphson step.
__device__ __forceinline__ void normalize3(float& x, float& y, float& z, const uint32_t* __restrict__ lut)
{
    const float len = (x * x + y * y) + z * z;
    const float nr = rsqrtps_x86(len, lut);
    const float muls = (len * nr) * nr;
    const float s = (0.5f * nr) * (3.0f - muls);
    x = x * s;
    y = y * s;
    z = z * s;
}

// rsqrtps_x86 for a positive, normal, finite x: the table entry of (exponent parity, mantissa >> 13) less the
// exponent's half -- ((E - E0) / 2) << 23 with E0 = 127 or 128 of E's parity is (E + (E & 1) - 128) << 22
__device__ __forceinline__ float rsqrtps_pos(float x, const uint32_t* __restrict__ lut)
{
    const uint32_t b = __float_as_uint(x);
    const uint32_t E = b >> 23;
    return __uint_as_float(lut[(b >> 13) & 0x7ffu] - ((E + (E & 1u) - 128u) << 22));
}

// normalize3 (SIMD::Normalize) with rsqrtps_pos, falling back to rsqrtps_x86 for the whole wave when a live lane's
// length is zero, denormal, negative, infinite or NaN
__device__ __forceinline__ void normalize3_fast(float& x, float& y, float& z, const uint32_t* __restrict__ lut, bool live)
{
    const float len = (x * x + y * y) + z * z;
    float nr;
    if (wave_ballot(live && !(__float_as_uint(len) - 0x00800000u < 0x7f000000u)) != 0ull) nr = rsqrtps_x86(len, lut);
    else nr = rsqrtps_pos(len, lut);
    const float muls = (len * nr) * nr;
    const float s = (0.5f * nr) * (3.0f - muls);
    x = x * s;
    y = y * s;
    z = z * s;
}

// normalize3_fast for the two rays of a pair unit: one wave-uniform test over both rays' live lanes -- both rays take
// rsqrtps_x86 if any fails it --, and otherwise both table gathers in flight before either is used (one wait)
__device__ __forceinline__ void normalize3_fast2(float& ax, float& ay, float& az, bool liveA, float& bx, float& by, float& bz,
                                                 bool liveB, const uint32_t* __restrict__ lut)
{
    const float lenA = (ax * ax + ay * ay) + az * az;
    const float lenB = (bx * bx + by * by) + bz * bz;
    float nrA, nrB;
    const bool plainA = __float_as_uint(lenA) - 0x00800000u < 0x7f000000u;
    const bool plainB = __float_as_uint(lenB) - 0x00800000u < 0x7f000000u;
    if (__builtin_expect((wave_ballot(liveA && !plainA) | wave_ballot(liveB && !plainB)) != 0ull, 0)) {
        nrA = rsqrtps_x86(lenA, lut);
        nrB = rsqrtps_x86(lenB, lut);
    } else {
        nrA = rsqrtps_pos(lenA, lut);
        nrB = rsqrtps_pos(lenB, lut);
    }
    const float sA = (0.5f * nrA) * (3.0f - (lenA * nrA) * nrA);
    const float sB = (0.5f * nrB) * (3.0f - (lenB * nrB) * nrB);
    ax = ax * sA;
    ay = ay * sA;
    az = az * sA;
    bx = bx * sB;
    by = by * sB;
    bz = bz * sB;
}

// Ray direction (Sphereflake.cpp:149-150, 162-167): u = x/W, v = y/H at the pixel corner.
// The per-context words of the constant block {rw, rh, fast_div, tx_magic} (DeviceConsts) as one scalar load
// (the pair loop gets one vector load: forcing the scalar form there cost more scalar instructions than the vector
// ones it saved and no fewer wave cycles, profiles/unit_path/)
struct FrameConsts {
    float rw, rh;
    uint32_t fast_div, tx_magic;
};
static_assert(offsetof(DeviceConsts, rw) % 16 == 0 && offsetof(DeviceConsts, tx_magic) == offsetof(DeviceConsts, rw) + 12,
              "rw, rh, fast_div, tx_magic: one aligned 16-byte load");
__device__ __forceinline__ FrameConsts frame_consts(const DeviceConsts* K)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) uint4* ConstU4;
    const uint4 w = *(ConstU4)(const void*)&K->rw;
    return FrameConsts{ __uint_as_float(w.x), __uint_as_float(w.y), w.z, w.w };
#else
    return FrameConsts{ K->rw, K->rh, K->fast_div, K->tx_magic };
#endif
}

__device__ __forceinline__ void ray_dir(const FrameArgs& a, float x, float y, float& dx, float& dy, float& dz,
                                        const uint32_t* __restrict__ lut, const FrameConsts* fc = nullptr,
                                        const bool* live = nullptr)
{
    // (live: the lean loops -- the lane traces this ray; the direction by normalize3_fast, in wave-uniform code)
    float u, v;
    // (uniform) RN(x / W) as one product and one fma correction (sfhost::division_by_reciprocal_exact); the
    // context's reciprocals by scalar loads from the constant block (fc: already loaded, with tile_of's word)
    float rw, rh;
    uint32_t fast;
    if (fc) {
        rw = fc->rw, rh = fc->rh, fast = fc->fast_div;
    } else {
#if defined(__HIP_DEVICE_COMPILE__)
        typedef const __attribute__((address_space(4))) DeviceConsts* ConstK;
        const ConstK kc = (ConstK)(const void*)a.consts;
        rw = kc->rw, rh = kc->rh, fast = kc->fast_div;
#else
        rw = a.consts->rw, rh = a.consts->rh, fast = a.consts->fast_div;
#endif
    }
    if (fast) {
        const float qu = x * rw, qv = y * rh;
        u = __builtin_fmaf(__builtin_fmaf(-qu, a.fw, x), rw, qu);
        v = __builtin_fmaf(__builtin_fmaf(-qv, a.fh, y), rh, qv);
    } else {
        u = x / a.fw;
        v = y / a.fh;
    }
    dx = ((a.tl[0] + a.dh[0] * u) + a.dv[0] * v) - a.o[0];
    dy = ((a.tl[1] + a.dh[1] * u) + a.dv[1] * v) - a.o[1];
    dz = ((a.tl[2] + a.dh[2] * u) + a.dv[2] * v) - a.o[2];
    if (live) normalize3_fast(dx, dy, dz, lut, *live);
    else normalize3(dx, dy, dz, lut);
}

// ray_dir for the two rays of a pair unit (pixels (xa, y) and (xb, y), the lean loop's constants): v and the three
// dv x v products once -- the same operands, so the same floats for both --, u and the dh x u sums per ray, and the
// two directions normalised together (normalize3_fast2)
__device__ __forceinline__ void ray_dir_pair(const FrameArgs& a, const FrameConsts& fc, float xa, float xb, float y,
                                             bool liveA, bool liveB, float& ax, float& ay, float& az, float& bx, float& by,
                                             float& bz, const uint32_t* __restrict__ lut)
{
    float ua, ub, v;
    if (fc.fast_div) {   // (uniform)
        const float qa = xa * fc.rw, qb = xb * fc.rw, qv = y * fc.rh;
        ua = __builtin_fmaf(__builtin_fmaf(-qa, a.fw, xa), fc.rw, qa);
        ub = __builtin_fmaf(__builtin_fmaf(-qb, a.fw, xb), fc.rw, qb);
        v = __builtin_fmaf(__builtin_fmaf(-qv, a.fh, y), fc.rh, qv);
    } else {
        ua = xa / a.fw;
        ub = xb / a.fw;
        v = y / a.fh;
    }
    const float vx = a.dv[0] * v, vy = a.dv[1] * v, vz = a.dv[2] * v;
    ax = ((a.tl[0] + a.dh[0] * ua) + vx) - a.o[0];
    ay = ((a.tl[1] + a.dh[1] * ua) + vy) - a.o[1];
    az = ((a.tl[2] + a.dh[2] * ua) + vz) - a.o[2];
    bx = ((a.tl[0] + a.dh[0] * ub) + vx) - a.o[0];
    by = ((a.tl[1] + a.dh[1] * ub) + vy) - a.o[1];
    bz = ((a.tl[2] + a.dh[2] * ub) + vz) - a.o[2];
    normalize3_fast2(ax, ay, az, liveA, bx, by, bz, liveB, lut);
}

// Near root of RaySphereIntersection (SIMD_AVX.h:260-267); NaN when R2 < d2 (lanes that missed).
__device__ __forceinline__ float near_root(float tca, float d2, float R2)
{
    const float thc = __builtin_sqrtf(R2 - d2);
    const float t0 = tca + thc;
    const float t1 = tca - thc;
    return (t0 <= t1) ? t0 : t1;
}

// One level down the transform chain (Sphereflake.h:162-164, SIMD_AVX.h:59-81 product without FMA): `out` = the
// frame of child i of a depth-p node whose frame is P, both as 3 x 4 {column-major xyz} (xf[3 c + r]). The child's
// unit frame has its translation column scaled by (4/3) r_p. The per-ray kernel and the slab unpack both chain
// with it, so a node's frame is the same float values whichever computes it.
// (child: the 9 unit child frames, scale: the per-depth child translation scales -- from the constant block, or an
// LDS image of them in the slab unpack)
// SF_AFFINE_FMA (round 6): the unit child frames are affine -- row 3 of column c is exactly 0 (c < 3) or 1 (c = 3), as
// glm's translate/rotate make them (Sphereflake.cpp:216-249; sf_set_setup refuses any other) -- so the 4th product
// P[9 + r] * b3 is exact (+-0 or P[9 + r] itself) and s + P[9 + r] * b3 rounds once either way: fma(P[9 + r], b3, s)
// is the same float bit for bit (also for -0, inf and NaN), one VALU instead of two. The traversal's cooperative child
// build (expand) and the slab unpack's centre use the same form.
__device__ __forceinline__ void child_frame(const float (*child)[16], const float* scale, uint32_t p, uint32_t i,
                                            const float* P, float* out)
{
    const float s = scale[p];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float* B = child[i] + 4 * c;
        const float b0 = c == 3 ? B[0] * s : B[0];
        const float b1 = c == 3 ? B[1] * s : B[1];
        const float b2 = c == 3 ? B[2] * s : B[2];
        const float b3 = B[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            out[3 * c + r] = __builtin_fmaf(P[9 + r], b3, (P[r] * b0 + P[3 + r] * b1) + P[6 + r] * b2);   // (SF_AFFINE_FMA)
    }
}
__device__ __forceinline__ void child_frame(const DeviceConsts* __restrict__ K, uint32_t p, uint32_t i,
                                            const float* P, float* out)
{
    child_frame(K->child, K->dt.scale, p, i, P, out);
}

struct HitState {
    float minT;
    float cx, cy, cz;     // centre of the nearest accepted sphere
    uint32_t index;       // its heap index (low 32 bits)
    int32_t depth;        // its depth (wave traversal: tie-breaking, see accept_self)
    bool hit;
};

// Position and normal of the nearest hit (Sphereflake.h:218-224). Computed once from the winning
// t and centre: the same operations on the same operands as the reference's per-acceptance update.
__device__ __forceinline__ void shade(float dx, float dy, float dz, const HitState& h, const uint32_t* __restrict__ lut,
                                      float& px, float& py, float& pz, float& nx, float& ny, float& nz)
{
    px = py = pz = nx = ny = nz = 0.f;
    if (h.hit) {
        px = dx * h.minT;
        py = dy * h.minT;
        pz = dz * h.minT;
        nx = px - h.cx;
        ny = py - h.cy;
        nz = pz - h.cz;
        normalize3(nx, ny, nz, lut);
    }
}

// shade's position and its normal before normalisation, for every lane (the lean loops shade in wave-uniform code:
// normalize3_fast / normalize3_fast2 on the normal, then the zeros of the lanes that missed)
__device__ __forceinline__ void hit_point(float dx, float dy, float dz, const HitState& h, float& px, float& py, float& pz,
                                          float& nx, float& ny, float& nz)
{
    px = dx * h.minT;
    py = dy * h.minT;
    pz = dz * h.minT;
    nx = px - h.cx;
    ny = py - h.cy;
    nz = pz - h.cz;
}

// max over the wave of a non-negative float (ordered as its bit pattern), all 64 lanes active.
// DPP row operations (six v_max_u32_dpp and one v_readlane, no LDS round trip): within each row of 16 lanes by
// quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror and row_mirror -- every lane then holds its row's
// maximum --, row 0 into row 1 and row 2 into row 3 by row_bcast:15 (row mask 0xa), rows 0-1 into rows 2-3 by
// row_bcast:31 (row mask 0xc): lane 63 holds the wave's. A lane a step does not write keeps max(b, 0) = b.
__device__ __forceinline__ float wave_max_pos(float v)
{
    uint32_t b = __float_as_uint(v);
    b = max(b, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)b, 0xb1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
    b = max(b, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)b, 0x4e, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
    b = max(b, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)b, 0x141, 0xf, 0xf, false));   // row_half_mirror
    b = max(b, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)b, 0x140, 0xf, 0xf, false));   // row_mirror
    b = max(b, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)b, 0x142, 0xa, 0xf, false));   // row_bcast:15
    b = max(b, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)b, 0x143, 0xc, 0xf, false));   // row_bcast:31
    return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)b, 63));
}

__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m, 64));
    return v;
}

// (lane in m) ? b : a -- one v_cndmask on an SGPR lane mask (a wave ballot), no per-lane bool
__device__ __forceinline__ float sel_mask(float a, float b, uint64_t m)
{
    float r;
    __asm__("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(m));
    return r;
}

// dst = (lane in m) ? src : dst, in dst's own register (tied operand): one v_cndmask on an SGPR lane
// mask, no per-lane bool materialised and no copy between a pre- and a post-update register
__device__ __forceinline__ void sel_in_place(float& dst, float src, uint64_t m)
{
    __asm__("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(dst) : "v"(src), "s"(m));
}
__device__ __forceinline__ void sel_in_place(uint32_t& dst, uint32_t src, uint64_t m)
{
    __asm__("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(dst) : "v"(src), "s"(m));
}

// Near root with sqrt_rn(x) for x = R2 - d2 >= 2^-96 (finite): the hardware estimate and its +-1 ulp correction
// by two fma residuals -- the sequence the compiler emits for a correctly rounded sqrtf, without the scaling of
// tiny arguments and the zero/inf class fix-up that x >= 2^-96 never needs, so bit for bit its result there.
// The correction and the choice between the two roots as arithmetic, without a compare -> select pair and its wait
// states (sf_rootforms.h, with the proofs): eight VALU instructions behind the v_sqrt where the selects took twelve
// and three s_nop.
__device__ __forceinline__ float near_root_big(float tca, float x)
{
    return near_root_of(tca, sqrt_fix(__builtin_amdgcn_sqrtf(x), x));
}

// Exact near root for the rare undecided lanes of the LOD bracket. Inlined: its uniform branch stays a
// real branch (the structurizer leaves wave-uniform regions alone), and without a call no SGPRs are saved
// around it (round 1 kept it out of line so it would not be if-converted into every child test).
__device__ __forceinline__ float near_root_exact(float tca, float d2, float R2)
{
    return near_root(tca, d2, R2);
}

// "Any lane of my group": the PW lanes of a reference packet (packet semantics: movemask early-outs,
// SIMD_AVX.h:247,255, Sphereflake.h:140,149,207; PW = 8 for the AVX path, 4 for the SSE path, SIMD_SSE.h).
template <int PW>
__device__ __forceinline__ bool group_any(bool p)
{
    const uint64_t b = wave_ballot(p);
    return ((b >> (threadIdx.x & (64u - PW))) & ((1ull << PW) - 1ull)) != 0ull;
}

// ------------------------------------------------------------------------------------------
// Wave-coherent traversal of IntersectSphereflake (Sphereflake.h:86-226).
//
// The DFS runs over EXPANDED nodes only (nodes that passed bounding sphere + LOD for at least one
// lane of the wave). When a node expands, the wave
//   1. builds its 9 child world transforms cooperatively into the LDS table of its level
//      (36 lanes: one column each; child translation scaled by (4/3) r, world = parent * child,
//      SIMD_AVX.h:59-81, Sphereflake.h:162-172) plus Dot(centre, centre) of each child;
//   2. culls the children no ray of the tile's cone can reach (9 centre lanes in parallel), then tests
//      the remaining ones one after the other (a uniform loop over a 9-bit mask): the per-ray traversals
//      (traverse_ray, traverse_pair, traverse_mixed) enter a child as soon as its test passes; the packet
//      traversal (traverse_packet) first gives each lane a 9-bit "child expands" vector E and the wave a 9-bit
//      "pending" mask of children some lane expands, and enters those after.
// A node's own sphere is tested when the node is entered (pre-order) with an ancestor tie-break that
// reproduces the reference's post-order "first strictly smaller t wins" (Sphereflake.h:174-224) -- see
// accept_self. Children that no lane expands cost only their bounding test, as in the reference.
//
// Per node (group = the lane itself for per-ray semantics, the 8 lanes of a reference AVX packet
// for packet semantics):
//   bounding   hb = active && any_g(tca >= 0) && any_g(d2 <= (2r)^2)
//   LOD        ex = hb && any_g(t < T_d)          [T_d exact threshold of sqrtf(t/r) < 70 || t < 0]
//   self       hs = active && any_g(tca >= 0) && any_g(d2 <= r^2); accept lanes with d2 <= r^2 && t < minT
// For per-ray groups these are exactly the reference's per-lane tests.
// ------------------------------------------------------------------------------------------
// Per-wave LDS image (floats): [root: 16][cone: 8][per level: table | E 32 | pad 3]. A transform is
// {cx cy cz cc} (cc = Dot(centre, centre)) and its three axis columns. The root keeps them as 4 contiguous
// float4; a level table keeps plane 0 = the 9 children's {centre, cc} float4, then planes 1..3 = their
// column j as float3 (9 x 3 floats each): 117 floats per level instead of 144, so 8 waves fit per SIMD.
struct TraverseLds {
    float* base;
    __device__ __forceinline__ float* root() const { return base; }
    __device__ __forceinline__ float* cone() const { return base + SF_LDS_ROOT; }
    __device__ __forceinline__ float* table(uint32_t lvl) const
    {
        return base + SF_LDS_ROOT + SF_LDS_CONE + lvl * SF_LDS_LEVEL;
    }
    __device__ __forceinline__ uint16_t* E(uint32_t lvl) const
    {
        return reinterpret_cast<uint16_t*>(base + SF_LDS_ROOT + SF_LDS_CONE + lvl * SF_LDS_LEVEL + SF_LDS_TABLE);
    }
};

template <bool B> struct BoolC { static constexpr bool value = B; };

__device__ __forceinline__ void lds_fence()
{
    __builtin_amdgcn_wave_barrier();
    __asm__ volatile("" ::: "memory");
}

__device__ __forceinline__ float readlane_f(float v, uint32_t l)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)l));
}
// Lane l of `old` := v (uniform v and l) as a per-lane select: no divergent region, no asm.
__device__ __forceinline__ uint32_t writelane_u(uint32_t v, uint32_t l, uint32_t old)
{
    return (threadIdx.x & 63u) == l ? v : old;
}

// Lane l of `old` := v (uniform v and l): one v_writelane_b32 (traverse_ray's push; a select costs v_cmp, v_mov and
// v_cndmask per word)
__device__ int sf_amdgcn_writelane(int v, int l, int old) __asm("llvm.amdgcn.writelane.i32");   // (no clang builtin)
__device__ __forceinline__ uint32_t writelane_s(uint32_t v, uint32_t l, uint32_t old)
{
    return (uint32_t)sf_amdgcn_writelane((int)v, (int)l, (int)old);
}

// One lane's 64-bit global atomic add on behalf of the wave (EXEC forced to lane 0 inside the asm).
__device__ __forceinline__ void wave_atomic_add_u64(uint64_t* p, uint64_t v)
{
    uint64_t saved;
    const uint32_t zero = 0u;
    __asm__ volatile(
        "s_mov_b64 %0, exec\n\t"
        "s_mov_b64 exec, 1\n\t"
        "global_atomic_add_x2 %1, %2, %3\n\t"
        "s_waitcnt vmcnt(0)\n\t"
        "s_mov_b64 exec, %0\n\t"
        : "=&s"(saved)
        : "v"(zero), "v"(v), "s"(p)
        : "memory");
}

// Diagnostic build only (make PHASES=1): s_memtime stamps at the DFS segment boundaries, summed per
// segment into 64-bit scalars and added to phase_sums once per wave. Segments: 0->1 push bookkeeping,
// 1->2 expand (node read, build, child tests), 3->4 self test, 4->5 pop; 0 is taken at the loop head (and sums
// what ran since the previous stamp: the child tests no lane passed).
// Never compiled into the product library; read its SHARES, not its run time.
#ifdef SF_PHASE_STAMPS
#define SF_STAMP_DECL uint64_t ph_last = __builtin_amdgcn_s_memtime(), ph_sum[7] = {0, 0, 0, 0, 0, 0, 0}
#define SF_STAMP(k)                                                                            \
    do {                                                                                       \
        uint64_t t_;                                                                           \
        __builtin_amdgcn_sched_barrier(0);                                                     \
        __asm__ volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");         \
        __builtin_amdgcn_sched_barrier(0);                                                     \
        ph_sum[k] += t_ - ph_last;                                                             \
        ph_last = t_;                                                                          \
    } while (0)
#define SF_STAMP_FLUSH(p)                                                                      \
    do {                                                                                       \
        if (p) {                                                                               \
            for (int k_ = 0; k_ < 7; ++k_) wave_atomic_add_u64((uint64_t*)(p) + k_, ph_sum[k_]);  \
        }                                                                                      \
    } while (0)
#elif defined(SF_COUNTS)
// Diagnostic build only (make COUNTS=1): per-wave event counts instead of stamps, summed into
// phase_sums[k]: 0 nodes whose children are tested, 1 child-loop iterations, 2 iterations no lane
// hits (bounding), 3 children entered, 4 leaf skips; lane utilisation: 5 active lanes summed over
// child-loop iterations, 6 bounding-hit lanes summed over them, 7 active lanes summed over expanded
// nodes, 8 inline leaf self tests, 9 their active lanes, 10 leaf-level nodes that took leaf_children (they are
// among 0, and neither pushed nor popped), 11 their children (tested by leaf_children: not among 1),
// 12 entries the occlusion cull left no lane for, 13 occlusion culls run, 14 iterations with <= 32 active lanes,
// 15 waves traced.
#define SF_STAMP_DECL uint64_t ph_sum[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define SF_STAMP(k)
#define SF_COUNT(k, v) (ph_sum[k] += (v))
#define SF_STAMP_FLUSH(p)                                                                      \
    do {                                                                                       \
        if (p) {                                                                               \
            ph_sum[15] = 1;                                                                    \
            for (int k_ = 0; k_ < 16; ++k_) wave_atomic_add_u64((uint64_t*)(p) + k_, ph_sum[k_]); \
        }                                                                                      \
    } while (0)
#else
#define SF_STAMP_DECL
#define SF_STAMP(k)
#define SF_STAMP_FLUSH(p) (void)(p)
#endif
#ifndef SF_COUNT
#define SF_COUNT(k, v)
#endif

// Per-depth constants {(2r)^2, r^2, (4/3) r, T} through the constant address space, so a uniform depth
// gives one s_load_dwordx4 from the scalar cache. Through a generic pointer the compiler cannot rule
// out aliasing with the kernel's global stores and emits a vector load plus a vmcnt wait instead.
__device__ __forceinline__ float4 depth_consts(const DeviceConsts* K, uint32_t d)
{
#if defined(__HIP_DEVICE_COMPILE__)
    // a 32-bit byte offset added to the table base: the scalar load takes it as its SGPR offset, with no
    // 64-bit address arithmetic on the scalar unit per access
    typedef const __attribute__((address_space(4))) float4* ConstF4;
    typedef const __attribute__((address_space(4))) char* ConstC;
    return *(ConstF4)((ConstC)(const void*)K->depth8 + (d << 5));
#else
    return reinterpret_cast<const float4*>(K->depth8)[2u * d];   // host pass: never executed
#endif
}
// depth_consts, and word w of the eight (DeviceConsts::depth8), of the depth whose byte offset `o` = d << 5 the caller
// carries
__device__ __forceinline__ float4 depth_consts_at(const DeviceConsts* K, uint32_t o)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) float4* ConstF4;
    typedef const __attribute__((address_space(4))) char* ConstC;
    return *(ConstF4)((ConstC)(const void*)K->depth8 + o);
#else
    return reinterpret_cast<const float4*>(K->depth8)[o >> 4];
#endif
}
__device__ __forceinline__ float depth_word_at(const DeviceConsts* K, uint32_t o, uint32_t w)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) float* ConstF;
    typedef const __attribute__((address_space(4))) char* ConstC;
    return *(ConstF)((ConstC)(const void*)K->depth8 + o + 4u * w);
#else
    return reinterpret_cast<const float*>(K->depth8)[(o >> 2) + w];
#endif
}
// {leaf, 0, 0, 0} of depth d (see DeviceConsts::depth8)
__device__ __forceinline__ float depth_leaf(const DeviceConsts* K, uint32_t d)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) float* ConstF;
    typedef const __attribute__((address_space(4))) char* ConstC;
    return *(ConstF)((ConstC)(const void*)K->depth8 + (d << 5) + 16u);
#else
    return reinterpret_cast<const float4*>(K->depth8)[2u * d + 1u].x;
#endif
}

// the traversals' status bits: the tile needs more levels than provisioned; an exact tie under the front-first order
#define SF_STATUS_OVERFLOW 1u
#define SF_STATUS_TIE 2u

// Root transform -> the wave's LDS image in the transform layout (Sphereflake.cpp:83). The same for
// every tile of a frame: kernels stage it once per wave, before any tile loop.
__device__ __forceinline__ void stage_root(float* __restrict__ Lbase, const float* root)
{
    const uint32_t lane = threadIdx.x & 63u;
    if (lane < 16u) {
        const float rcc = (root[9] * root[9] + root[10] * root[10]) + root[11] * root[11];
        float v = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            float rk = 0.f;
            if (k < 3) rk = root[9 + k];
            else if (k == 3) rk = rcc;
            else if ((k & 3) != 3) rk = root[3 * ((k >> 2) - 1) + (k & 3)];
            v = (lane == (uint32_t)k) ? rk : v;
        }
        Lbase[lane] = v;   // TraverseLds::root()
    }
}

// The same staging without a branch on the lane (the multi-frame trace re-stages the root inside its persistent loop,
// where a lane-dependent region made the compiler allocate the whole loop's registers worse: 62 -> 30 SGPR spills):
// lane l writes word l & 15 -- the lanes above 15 repeat a lower lane's store, same address and value.
__device__ __forceinline__ void stage_root_all_lanes(float* __restrict__ Lbase, const float* root)
{
    const uint32_t l = threadIdx.x & 15u;
    const float rcc = (root[9] * root[9] + root[10] * root[10]) + root[11] * root[11];
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        float rk = 0.f;
        if (k < 3) rk = root[9 + k];
        else if (k == 3) rk = rcc;
        else if ((k & 3) != 3) rk = root[3 * ((k >> 2) - 1) + (k & 3)];
        v = (l == (uint32_t)k) ? rk : v;
    }
    Lbase[l] = v;   // TraverseLds::root()
}

// Lane -> (child bi, column bc) of the cooperative child build: lanes 0..26 the axis columns of child lane % 9
// (bc = lane / 9), lanes 27..63 centres (bc = 3) -- lanes 32 + i child i (the ballot lanes), lanes 27..31 child 8,
// the rest repeats (see BuildLane for the layout and its bank-conflict reasons).
__device__ __forceinline__ uint32_t build_child(uint32_t lane)
{
    return lane < 27u ? lane % 9u : lane < 32u ? 8u : (lane - 32u) % 9u;
}

// This lane's column of the cooperative child build (see build_child). Loaded once per wave, before any tile
// loop: a global load in every traversal would wait (vmcnt, in order on this ISA) for the previous tile's
// G-buffer stores.
__device__ __forceinline__ float4 build_column(const DeviceConsts* __restrict__ K)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t bi = build_child(lane);
    const uint32_t bc = lane < 27u ? lane / 9u : 3u;
    const float4 r = make_float4(K->child[bi][4u * bc + 0u], K->child[bi][4u * bc + 1u], K->child[bi][4u * bc + 2u],
                                 K->child[bi][4u * bc + 3u]);
    // retire the loads here (vmcnt(0)): otherwise the wait is placed at the first use inside the traversal,
    // where it would also wait for every tile's G-buffer stores
    __builtin_amdgcn_s_waitcnt(0x0f70);
    return r;
}

// ------------------------------------------------------------------------------------------
// The building blocks the traversals below share. Their exact operation order is the contract (frames are bit
// exact against the reference), so each exists once.
// ------------------------------------------------------------------------------------------

__device__ __forceinline__ void reset_hit(HitState& h, float minT)
{
    h.minT = minT;
    h.cx = h.cy = h.cz = 0.f;
    h.index = 0xffffffffu;
    h.depth = -1;
    h.hit = false;   // set on return: hit <=> depth >= 0
}

// This lane's part in the cooperative child build: column bc of child bi, the column's constants b0..b3
// (build_column) and where the built column goes in a level table (slot). The 27 axis columns (column bc = lane / 9 of child
// bi = lane % 9) are built by lanes 0..26 of the first 32-lane LDS bank group, the 9 centres (column 3) by lanes
// 32 + i of the second group: lanes 32..40 hold the 9 child centres (read back by v_readlane), and a ballot's
// per-child mask is bits 0..8 of its high word, one scalar AND (centres on lanes 31..39 had a mask straddling the
// two words: a 64-bit shift and an AND per ballot). Every other lane repeats a builder (27..31: child 8's centre;
// 41..63: children (lane - 32) % 9 again) -- the same value, so there is no divergent region, and the build's VALU
// cost is per wave either way.
// slot: centre lanes (bc = 3) store xyz + cc at plane 0 (child i at float 4 i), the others xyz in their column
// plane; the centre lanes' cc store goes to plane 0, the others' to one junk word of the cone block, so both stores
// are unconditional. With the column planes skewed by 2 floats (SF_LDS_PLANE) no store of the build has two
// distinct addresses on one bank within a lane group -- except child 8's centre: the centres are 16-B aligned,
// child i's x at bank 4 i mod 32, so child 8's and child 0's stores from one lane group of ds_write_b32 were a
// 2-way bank conflict on every table store of every expansion. So child 8's centre is stored by lanes 27..31 of
// the low group, and the high group's child-8 lanes store into the level's E words, which the per-ray traversals
// do not use, at a float offset of 2 mod 4 (the levels are 32-B aligned): store k then hits bank 2 + k mod 4, no
// centre store's 4 i + k. (An earlier layout -- centres on lanes 27..35, lanes 36..63 mirroring 0..27 -- put
// 4.9 M extra cycles per 1080p frame into bank conflicts, 40 % of the LDS instruction cycles.)
// (The packet traversal keeps its E words: its lanes 32 + 8 store child 8's centre in place, see traverse_packet.)
struct BuildLane {
    uint32_t bi, bc, slot;
    float b0, b1, b2, b3;
};
__device__ __forceinline__ BuildLane build_lane(const float4 bcol, uint32_t lane, uint32_t bi)
{
    const uint32_t bc = lane < 27u ? lane / 9u : 3u;
    const uint32_t slot = bc == 3u ? (lane >= 32u && bi == 8u ? (uint32_t)SF_LDS_TABLE + 3u : bi * 4u)
                                   : SF_LDS_PLANE + bc * SF_LDS_COLS + bi * 3u;
    return BuildLane{ bi, bc, slot, bcol.x, bcol.y, bcol.z, bcol.w };
}

// ---- The wave's ray cone: axis a = the axis lane's direction (the tile's centre pixel), sinT bounds the sine of
// every ray's angle to it. cone_s2m: one ray's |d x a|^2 (|d|, |a| = 1 +- 2^-20), 1 for a ray pointing away from the
// axis. stage_cone: s2m = this lane's largest over its rays; the wave's largest, plus 2^-16 slack, is sinT. A wide
// cone (scattered packets of the frame-less mode, or sinT >= 1/2) -- or cone_cull off -- disables the child cone cull
// through cosT = 0, sinT = 1. {a, cosT, sinT} are kept in LDS (read with the node at every expansion): as uniform
// registers they would spill SGPRs.
__device__ __forceinline__ float cone_s2m(float dx, float dy, float dz, float ax, float ay, float az)
{
    const float cx_ = dy * az - dz * ay, cy_ = dz * ax - dx * az, cz_ = dx * ay - dy * ax;
    const float s2 = (cx_ * cx_ + cy_ * cy_) + cz_ * cz_;
    const bool fwd = (dx * ax + dy * ay) + dz * az > 0.0f;
    return fwd ? s2 : 1.0f;
}
template <class S2m>   // (s2m: a callable, so that its arithmetic stays inside the cone_cull branch)
__device__ __forceinline__ void stage_cone(const TraverseLds& L, uint32_t lane, bool cone_cull, float ax, float ay,
                                           float az, S2m s2m)
{
    float cosT = 0.0f, sinT = 1.0f;
    if (cone_cull) {
        const float sm = __builtin_amdgcn_sqrtf(wave_max_pos(s2m())) * (1.0f + 0x1p-16f) + 0x1p-16f;
        if (sm < 0.5f) {
            sinT = sm;
            cosT = __builtin_amdgcn_sqrtf(1.0f - sm * sm) * (1.0f - 0x1p-16f);
        }
    }
    if (lane < 5u) L.cone()[lane] = lane == 0u ? ax : lane == 1u ? ay : lane == 2u ? az : lane == 3u ? cosT : sinT;
}

// ---- LOD of one node whose bounding sphere the lanes of hbm hit (hb: this lane's bit of hbm; xs = R2b - d2; the
// node's depth constants R2b = (2r)^2, T, Tfar): the lanes that expand it, i.e. whose t = fl(tca - sqrt_rn(R2b - d2))
// (SIMD_AVX.h:260-267; t0 <= t1 picks t1 for thc >= 0) is below T. The bounds on t hold for any centre and bounding
// radius, the root's included.
// Most bounding hits are decided without the root: t = fl(tca - s) <= tca (s >= 0, rounding is monotone), so
// tca < T expands. And on a bounding hit s <= 2r (1 + 2^-19) + 2^-9.7 tca (d2 can be negative by rounding, down to
// -2^-19.4 |c|^2, |c|^2 <= tca^2 + R2b), so tca (1 - 2^-8) >= T + 2r (1 + 2^-18) (`Tfar`, rounded up) means t >= T:
// no expansion. Only lanes in between take the bracket (rare: a band of width ~2r + 2^-8 tca around T).
// The bracket: the hardware sqrt is within 2 ulp of sqrt_rn and t is monotone in it, so
// t_lo = fl(tca - (s + 2ulp)) <= t <= t_hi = fl(tca - (s - 2ulp)): t_hi < T decides "expands", t_lo >= T decides
// "does not"; the exact IEEE root runs only for lanes in between, or with a tiny sqrt argument.
__device__ __forceinline__ uint64_t lod_expands(float tca, float d2, float xs, bool hb, uint64_t hbm, float R2b, float T,
                                                float Tfar)
{
    const uint64_t nearm = wave_ballot(tca < T);
    const uint64_t farm = wave_ballot(tca * (1.0f - 0x1p-8f) >= Tfar);
    if ((hbm & ~(nearm | farm)) == 0ull) return hbm & nearm;
    const float sq = __builtin_amdgcn_sqrtf(xs);
    const float s_lo = __uint_as_float((uint32_t)max((int32_t)__float_as_uint(sq) - 2, 0));
    const float s_hi = __uint_as_float(__float_as_uint(sq) + 2u);
    const float t_hi = tca - s_lo;
    const float t_lo = tca - s_hi;
    // The decision as per-lane values instead of scalar mask algebra: th / tl are t_hi / t_lo on the lanes with a
    // bounding hit and +inf elsewhere; a tiny sqrt argument makes the bracket (-inf, +inf), i.e. undecided.
    // expands: th < T; undecided: tl < T <= th.
    const uint64_t tinym = wave_ballot(xs < 0x1p-96f);
    // (the tiny select is opaque asm, so the hb select below stays one v_cndmask on the VCC of the bounding compare
    // instead of being merged into scalar mask algebra)
    const float thx = sel_mask(t_hi, __builtin_inff(), tinym);
    const float tlx = sel_mask(t_lo, -__builtin_inff(), tinym);
    const float th = hb ? thx : __builtin_inff();
    const float tl = hb ? tlx : __builtin_inff();
    uint64_t exm = wave_ballot(th < T);
    const uint64_t undm = wave_ballot(sel_mask(tl, __builtin_inff(), exm) < T);
    if (undm) {   // rare: exact IEEE root for the undecided lanes (disjoint from exm)
        const float te = near_root_exact(tca, d2, R2b);
        exm |= undm & wave_ballot(te < T);
    }
    return exm;
}

// Bounding (SIMD_AVX.h:247-258) + LOD of the child with centre c, |c|^2 cc for one ray of every lane (actv: +inf on
// the lanes visiting the parent, -1 elsewhere): does any lane expand it? tca >= 0 && d2 <= R2b as ONE compare,
// min(tca, R2b - d2, actv) >= 0: with denormals kept, fl(R2b - d2) >= 0 exactly when d2 <= R2b (no NaN operands).
__device__ __forceinline__ bool child_expands(float cx, float cy, float cz, float cc, float dx, float dy, float dz,
                                              float actv, float R2b, float T, float Tfar)
{
    const float tca = (cx * dx + cy * dy) + cz * dz;
    const float d2 = cc - tca * tca;
    const float xs = R2b - d2;
    const bool hb = __builtin_fminf(__builtin_fminf(tca, xs), actv) >= 0.0f;
    const uint64_t hbm = wave_ballot(hb);
    return hbm != 0ull && lod_expands(tca, d2, xs, hb, hbm, R2b, T, Tfar) != 0ull;
}

// ---- The own sphere (radius^2 R2s) of a node with centre/|c|^2 pc, depth dd, heap index idx (Sphereflake.h:174-224,
// SIMD_AVX.h:236-270), tested when the node is entered for the lanes of actv (+inf on them, -1 elsewhere: one v_min3
// folds the visiting lanes into the hit compare), with tca and d2 as the node's child test formed them. Returns the
// accepting lanes.
// The reference tests a node's sphere after its children (post-order) and accepts strictly smaller t, so on an exact
// tie the earlier node in post-order wins. Pre-order differs from post-order only for ancestor/descendant pairs,
// hence: a tie is accepted iff the lane's current best is an ancestor of this node -- ancm, a wave lane mask, so the
// rule and its updates are scalar mask algebra; the caller clears a lane when the node at its best's depth is
// finished. A tie with a best that is not an ancestor: in index order that sphere came first in the reference's
// post-order too (rejecting is right); under the front-first child order it may not have, so with flag_ties the tile
// is flagged (SF_STATUS_TIE) and re-traced in index order (never seen on the BASELINE views).
// ANYHIT (the shadow traces): only "some visited sphere has ts < h.minT, the lane's bound" is wanted, so an
// accepting lane only gets its finished flag (h.depth >= 0); a tie is not `<`: never accepted, never flagged.
// INDEX_ORDER (traverse_mixed): the children are always entered in index order, nothing is ever flagged, and the tie
// rule is applied without a branch of its own.
// accept_hits: the accept part alone, for the lanes of hsm (not empty), which hit the sphere (leaf_children forms the
// hit mask itself, before the LOD and occlusion tests).
template <bool ANYHIT, bool INDEX_ORDER = false>
__device__ __forceinline__ uint64_t accept_hits(HitState& h, uint64_t& ancm, uint32_t& status, bool flag_ties,
                                                const float4 pc, float tca, float d2, uint32_t dd, uint64_t hsm,
                                                uint32_t idx, float R2s)
{
    {
        // (the general correctly rounded root only when a hitting lane's argument is tiny: a uniform branch)
        const float xs = R2s - d2;
        float ts;
        if ((wave_ballot(!(xs >= 0x1p-96f)) & hsm) != 0ull) ts = near_root_exact(tca, d2, R2s);
        else ts = near_root_big(tca, xs);
        // strictly nearer lanes accept; exact ties (rare) take a branch of their own
        uint64_t accm = hsm & wave_ballot(ts < h.minT);
        if constexpr (ANYHIT) {   // (the finished flag only)
            uint32_t hd = (uint32_t)h.depth;
            sel_in_place(hd, dd, accm);
            h.depth = (int32_t)hd;
            return accm;
        }
        const uint64_t tie = hsm & wave_ballot(ts == h.minT);
        if constexpr (INDEX_ORDER) accm |= tie & ancm;
        else if (tie != 0ull) {
            accm |= tie & ancm;
            if (flag_ties && (tie & ~ancm) != 0ull) status |= SF_STATUS_TIE;
        }
        sel_in_place(h.minT, ts, accm);
        sel_in_place(h.cx, pc.x, accm);
        sel_in_place(h.cy, pc.y, accm);
        sel_in_place(h.cz, pc.z, accm);
        sel_in_place(h.index, idx, accm);
        uint32_t hd = (uint32_t)h.depth;
        sel_in_place(hd, dd, accm);
        h.depth = (int32_t)hd;
        ancm |= accm;
        return accm;
    }
}
template <bool ANYHIT, bool INDEX_ORDER = false>
__device__ __forceinline__ uint64_t accept_self(HitState& h, uint64_t& ancm, uint32_t& status, bool flag_ties,
                                                const float4 pc, float tca, float d2, uint32_t dd, float actv,
                                                uint32_t idx, float R2s)
{
    const uint64_t hsm = wave_ballot(__builtin_fminf(__builtin_fminf(tca, R2s - d2), actv) >= 0.0f);
    if (hsm) return accept_hits<ANYHIT, INDEX_ORDER>(h, ancm, status, flag_ties, pc, tca, d2, dd, hsm, idx, R2s);
    return 0ull;
}

// ---- Occlusion cull of a child (centre c, a lane's tca = c.d) that passed bounding + LOD: the lanes that need not
// enter it. Every sphere of the child's subtree, and every bounding sphere the subtree's LOD tests use, lies in the
// child's bounding ball (radius R = 2r around c). A lane whose float test of any of them accepts has
// t >= c.d - rho, rho = R + m (|c| + R), m = SF_OCCL_MARGIN covering every rounding of those tests (tca, the d2
// cancellation -- the dominant 2^-9.2 (|c| + R) --, the centres' transform chain, |d| != 1). So where
// c.d - rho > minT the lane can accept nothing in the subtree (ties included: strict), and where c.d - rho >= cull_t,
// the LOD threshold of the depth after the deepest already reached, no node of the subtree can pass LOD deeper than
// that depth (T falls with depth): the max-depth statistic is unchanged. (The child itself passed LOD for some
// lane: the caller's maxd counts it either way.)
// rho without |c|: a lane that hit the bounding sphere has |c|^2 = d2 + tca^2 <= R^2 + tca^2 (+ the float test's
// slack, 2^-9.6 |c|), so |c| <= tca + R (+ 2^-9.6 |c|, whose m multiple is far inside m's safety factor) and
// rho <= R (1 + 2 m) + m tca = cull_r + m tca per lane (cull_r: the `cull` word of DeviceConsts::depth8), no square root.
// ANYHIT: the distance condition alone -- no sphere of the subtree nearer than the lane's bound; there is no
// max-depth statistic to protect.
template <bool ANYHIT>
__device__ __forceinline__ uint64_t occluded(float tca, float minT, float cull_t, float cull_r)
{
    float v = tca - minT;
    if constexpr (!ANYHIT) v = __builtin_fminf(v, tca - cull_t);
    return wave_ballot(v - SF_OCCL_MARGIN * tca > cull_r);
}

// ---- The children of a leaf-level node: a node whose children (those the cone cull kept, entry order in Cl, their
// {centre, cc} in table tb, depth dd, constants dc / dk = the depth's eight words, child 0's heap index idx0) are all
// inline leaves (ChildBuild::leaf_level), for the lanes of avx (+inf on the lanes visiting the node, -1 elsewhere).
// Three fifths of a frame's child iterations sit at such nodes. The only thing a leaf child can change is a lane's
// hit, through its own sphere (radius r inside the bounding ball 2r), so the node is not opened: no push, no pop, the
// depth's constants loaded once, and per child the own sphere first -- a child whose sphere no visiting lane hits ends
// there (one compare), where the child loop takes it through LOD, the occlusion cull and the self test for its
// bounding hit alone. Then LOD and the occlusion cull for the lanes that hit, and the accept.
// Bit for bit the child loop's results:
//  - An own hit is a bounding hit, exactly: R2s < R2b, and with denormals kept fl(a - b) >= 0 exactly when b <= a, so
//    R2s - d2 >= 0 implies R2b - d2 >= 0 (tca >= 0 and the visiting lanes are the same operands in both compares).
//  - lod_expands decides per lane: a lane's result is its reference decision t < T whichever other lanes are in the
//    mask; the uniform shortcuts only choose how it is computed. So the lanes that hit the own sphere get here the
//    decision they get there.
//  - The occlusion cull is per lane too, and an occluded lane accepts nothing either way (its condition is strict).
//  So a lane reaches the accept for a leaf child here exactly when it does in the child loop (own hit, bounding hit,
//  LOD, not occluded), with the same tca, d2, root form (accept_hits) and tie rule; the children come in the same
//  entry order, so the tie flags are the same; leaves never overflow, so status is.
//  - ancm: a finished leaf clears the lanes whose best is at its depth. Lanes of ancm have their best at an ancestor
//    of the open node, i.e. above the leaf's depth, except those that have just accepted the leaf: ancm &= ~accepted.
//  - The max-depth statistic is the caller's part: the child loop raises maxd when some lane passes bounding + LOD,
//    own hit or not. The caller takes this loop only where depth dd is already counted (dd <= max(maxd, seed)):
//    then neither the statistic nor cull_t can change.
__device__ __forceinline__ void leaf_children(HitState& h, uint64_t& ancm, uint32_t& status, bool flag_ties,
                                              bool occl_cull, const float* tb, uint32_t Cl, float dx, float dy, float dz,
                                              float avx, uint32_t idx0, uint32_t dd, const float4 dc, const float4 dk,
                                              float cull_t)
{
    const float R2b = dc.x, R2s = dc.y, T = dc.w, Tfar = dk.z, cull_r = dk.y;
    while (Cl) {
        const uint32_t p = __builtin_ctz(Cl);
        __asm__("s_bitset0_b32 %0, %1" : "+s"(Cl) : "s"(p));
        const uint32_t c = p & 15u;
        lds_fence();
        const float4 pc = *reinterpret_cast<const float4*>(tb + c * 4u);
        const float tca = (pc.x * dx + pc.y * dy) + pc.z * dz;
        const float d2 = pc.w - tca * tca;
        const bool hs = __builtin_fminf(__builtin_fminf(tca, R2s - d2), avx) >= 0.0f;
        const uint64_t hsm = wave_ballot(hs);
        if (hsm == 0ull) continue;
        uint64_t amx = lod_expands(tca, d2, R2b - d2, hs, hsm, R2b, T, Tfar);
        if (amx == 0ull) continue;
        if (occl_cull) {
            amx &= ~occluded<false>(tca, h.minT, cull_t, cull_r);
            if (amx == 0ull) continue;
        }
        ancm &= ~accept_hits<false>(h, ancm, status, flag_ties, pc, tca, d2, dd, amx, idx0 + c, R2s);
    }
}

// leaf_children for the two rays of a pair unit (traverse_pair's two-ray loop): per ray what the one-ray form does, a
// branch taken on the union of the two rays' ballots.
template <class Ray>
__device__ __forceinline__ void leaf_children_pair(Ray& ra, Ray& rb, uint64_t& ancA, uint64_t& ancB, uint32_t& status,
                                                   bool flag_ties, bool occl_cull, const float* tb, uint32_t Cl,
                                                   float avxA, float avxB, uint32_t idx0, uint32_t dd, const float4 dc,
                                                   const float4 dk, float cull_t)
{
    const float R2b = dc.x, R2s = dc.y, T = dc.w, Tfar = dk.z, cull_r = dk.y;
    while (Cl) {
        const uint32_t p = __builtin_ctz(Cl);
        __asm__("s_bitset0_b32 %0, %1" : "+s"(Cl) : "s"(p));
        const uint32_t c = p & 15u;
        lds_fence();
        const float4 pc = *reinterpret_cast<const float4*>(tb + c * 4u);
        const float tcaA = (pc.x * ra.dx + pc.y * ra.dy) + pc.z * ra.dz;
        const float tcaB = (pc.x * rb.dx + pc.y * rb.dy) + pc.z * rb.dz;
        const float d2A = pc.w - tcaA * tcaA;
        const float d2B = pc.w - tcaB * tcaB;
        const bool hsA = __builtin_fminf(__builtin_fminf(tcaA, R2s - d2A), avxA) >= 0.0f;
        const bool hsB = __builtin_fminf(__builtin_fminf(tcaB, R2s - d2B), avxB) >= 0.0f;
        const uint64_t hsmA = wave_ballot(hsA), hsmB = wave_ballot(hsB);
        if ((hsmA | hsmB) == 0ull) continue;
        uint64_t amxA = hsmA ? lod_expands(tcaA, d2A, R2b - d2A, hsA, hsmA, R2b, T, Tfar) : 0ull;
        uint64_t amxB = hsmB ? lod_expands(tcaB, d2B, R2b - d2B, hsB, hsmB, R2b, T, Tfar) : 0ull;
        if ((amxA | amxB) == 0ull) continue;
        if (occl_cull) {
            amxA &= ~occluded<false>(tcaA, ra.h.minT, cull_t, cull_r);
            amxB &= ~occluded<false>(tcaB, rb.h.minT, cull_t, cull_r);
        }
        if (amxA) ancA &= ~accept_hits<false>(ra.h, ancA, status, flag_ties, pc, tcaA, d2A, dd, amxA, idx0 + c, R2s);
        if (amxB) ancB &= ~accept_hits<false>(rb.h, ancB, status, flag_ties, pc, tcaB, d2B, dd, amxB, idx0 + c, R2s);
    }
}

// ---- Expand the node with centre/|c|^2 pc (its axis columns j = 0..2 at col + j cs: col = root image + 4, cs = 4
// for the root; the parent table's column planes + 3 c, cs = SF_LDS_COLS for child c of a level): build its 9 child
// transforms into table tb and cull the children no ray of the wave's cone can reach. Returns the children left to
// test, in entry order (front child i at bit i, the others at 16 + i).
// (ko: byte offset of the children's depth constants; lv32: the provisioned levels in the same units; kp: the node
// centre's projection on the cone axis; index_order: 0x1ff to enter the children in index order, else 0)
// table(levels - 1) is never read -- entering a child of the deepest provisioned level overflows first --, so it is
// neither allocated nor stored: there the children are tested here, from the centre lanes (`expands(cx, cy, cz, cc,
// R2b, T, Tfar)`: does the child expand for any of the caller's rays?); one that does flags the tile for the deeper
// re-trace (SF_STATUS_OVERFLOW), and none is entered.
//
// Cone cull of child bi (centre c in lanes 32..40): no ray of the wave's cone (axis a, half-angle theta) can hit its
// bounding sphere. With ca = c.a and |q|^2 = |c|^2 - ca^2 (q = c - ca a), every ray's angle phi to c is at least
// c's angle to the axis less theta, so its line passes at distance |c| sin(phi) >= X = |q| cosT - ca sinT from c. A
// float hit (tca >= 0, cc - tca^2 <= R^2, SIMD_AVX.h:247-258) needs |c| sin(phi) <= sqrt(R^2 + dl), dl = 2^-18
// |c|^2 covering the rounding of tca, d2, |c|^2 and |d| (~12 ulp + 2^-21). Skip when ca > 0, |c|^2 > 2 (R^2 + dl)
// (c's angle to the axis below 45 deg while theta < 30 deg keeps every phi in a range that also covers the 8-lane
// packet tests), X > 0 and X^2 > R^2 + dl + 2^-19 |c|^2. The added 32 u |c|^2 covers this test's own rounding:
// |q|^2 is off by <= 10 u |c|^2 (cancellation), which moves X^2 by <= 2 X dq <= 10 u |c|^2; the hardware sqrt, X and
// X^2 add <= 7 u |c|^2. (|c|^2 - ca^2 is clamped at 0: no NaN, which the min would drop.) Such a child changes
// nothing for any lane in the reference: it is skipped for the whole wave.
// The test is this kernel's own arithmetic, not the reference's, so it fuses: ca, |c|^2 - ca^2, X and Y by fma --
// each fused step rounds once where the unfused one rounds twice, so the bounds behind the slack hold -- and the
// regime condition as w (1 - 2^-16) > 2 R^2, a slightly stronger one. 15 VALU per expansion. The four conditions
// are compares of a v_min3 and a v_min (with denormals kept, a > b exactly when fl(a - b) > 0; every operand is
// finite): the kept children come from one ballot. (w itself stays the reference's |c|^2: it is the table's cc.)
struct LeafLevel {   // what a traversal's expand() tells its caller for leaf_children
    float4 dc;       // the children's depth constants
    bool on;         // uniform: the kept children are all inline leaves, and their table is stored
};
struct ChildBuild {
    float x, y, z, w;    // this lane's built column (BuildLane), w = its |.|^2: child i's centre and cc on lane 32 + i
    uint32_t M, front;   // uniform: the children the cone cull kept; the front children (all, in index order)
    float4 dtc;          // the children's depth constants
    bool leaf_level;     // uniform: every child the cone cull kept is an inline leaf (see leaf_children)
};
// KP_CONE: kp is formed here, from the cone axis as read with the node -- the same operands, so the same float --
// instead of being passed in (the pair unit's one-ray loop, whose ray registers may hold either ray: no uniform copy
// of the axis is carried through the traversal)
template <bool KP_CONE = false>
__device__ __forceinline__ ChildBuild build_children(const DeviceConsts* K, const TraverseLds& L, const BuildLane& B,
                                                     const float4 pc, const float* col, uint32_t cs, uint32_t ko,
                                                     float kp, uint32_t index_order)
{
    lds_fence();
    const float3 p0 = *reinterpret_cast<const float3*>(col);
    const float3 p1 = *reinterpret_cast<const float3*>(col + cs);
    const float3 p2 = *reinterpret_cast<const float3*>(col + 2u * cs);
    // the wave's ray cone, read with the node (before this level's stores: the junk cc store below goes to the cone
    // block, so a read after it would wait for a second LDS round trip)
    const float4 cn = *reinterpret_cast<const float4*>(L.cone());
    const float sinT = L.cone()[4];
    const float4 dtn = depth_consts_at(K, ko - (1u << 5));   // this node: (4/3) r
    const float4 dtc = depth_consts_at(K, ko);               // children: (2r)^2, T
    const float leafw = depth_word_at(K, ko, 4u);            // children: leaf threshold
    // world = parent * child (SIMD_AVX.h:59-81), child translation scaled by (4/3) r (Sphereflake.h:162-172):
    // column 3 lanes multiply b0..b2 by s, the others by 1 (exact)
    const float sm = B.bc == 3u ? dtn.z : 1.0f;
    const float b0 = B.b0 * sm, b1 = B.b1 * sm, b2 = B.b2 * sm;
    const float x = __builtin_fmaf(pc.x, B.b3, (p0.x * b0 + p1.x * b1) + p2.x * b2);
    const float y = __builtin_fmaf(pc.y, B.b3, (p0.y * b0 + p1.y * b1) + p2.y * b2);
    const float z = __builtin_fmaf(pc.z, B.b3, (p0.z * b0 + p1.z * b1) + p2.z * b2);
    const float w = (x * x + y * y) + z * z;   // Dot(centre, centre) on the centre lanes (bc = 3)
    const float R2b = dtc.x;
    const float ax = cn.x, ay = cn.y, az = cn.z, cosT = cn.w;
    const float ca = __builtin_fmaf(x, ax, __builtin_fmaf(y, ay, z * az));
    const float sq = __builtin_amdgcn_sqrtf(__builtin_fmaxf(__builtin_fmaf(-ca, ca, w), 0.0f));
    const float X = __builtin_fmaf(sq, cosT, -(ca * sinT));
    const float Y = __builtin_fmaf(X, X, -(R2b + w * (0x1p-18f + 0x1p-19f)));
    const float reg = __builtin_fmaf(w, 1.0f - 0x1p-16f, -2.0f * R2b);
    const float mk = __builtin_fminf(__builtin_fminf(ca, reg), __builtin_fminf(X, Y));
    uint32_t M = (uint32_t)(wave_ballot(!(mk > 0.0f)) >> 32) & 0x1ffu;
    M = __builtin_amdgcn_readfirstlane(M);
    // entry order as bit order: the front children (nearer than this node's centre along the cone axis) at bits 0..8,
    // the others at 16..24 -- one find-first-set per child picks the next, and its low 4 bits are the child's number
    // (index order: every child "front" -- an OR with a per-traversal mask, not a branch)
    if constexpr (KP_CONE) kp = (pc.x * ax + pc.y * ay) + pc.z * az;
    const uint32_t front = ((uint32_t)(wave_ballot(ca < kp) >> 32) & 0x1ffu) | index_order;
    // the inline leaves among the children (the child loop's own test, pc.w > leaf, on the value the table gets)
    const uint32_t leafm = (uint32_t)(wave_ballot(w > leafw) >> 32);
    return ChildBuild{ x, y, z, w, M, front, dtc, (M & ~leafm) == 0u };
}

// ------------------------------------------------------------------------------------------
// Packet semantics (the frame-less progressive mode, progressive_trace): the original traversal. PW = the reference
// packet's width, 8 (AVX) or 4 (SSE): every test is "any lane of my packet" (group_any), as the reference's movemask
// early-outs are. It tests all children of a node first, keeps each lane's 9 "expands" bits in LDS (the level's E
// words) and enters the pending children after, in index order; inline leaves and the cone cull as in the per-ray
// traversals below, no occlusion cull and no front-first order (both rest on per-ray bounds).
// ------------------------------------------------------------------------------------------
template <int PW>
__device__ __forceinline__ void traverse_packet(const DeviceConsts* __restrict__ K, const float* root,
                                                float* __restrict__ Lbase, const float4 bcol, uint32_t levels, float dx,
                                                float dy, float dz, bool valid, HitState& h, int32_t& maxd,
                                                uint32_t& status, uint32_t K_flags)
{
    const uint32_t lane = threadIdx.x & 63u;
    const TraverseLds L{ Lbase };
    const bool cone_cull = (K_flags & SF_FLAG_NO_CONE_CULL) == 0u;
    SF_STAMP_DECL;   // (diagnostic builds: stamps and counts are taken, but this traversal has nowhere to flush them)

    reset_hit(h, FLT_MAX);
    uint64_t ancm = 0ull;   // lanes whose current best sphere is an ancestor of the open node (see accept_self)

    // ---- root node (depth 0): bounding sphere + LOD, centre straight from the kernel arguments
    const float rcx = root[9], rcy = root[10], rcz = root[11];
    const float rcc = (rcx * rcx + rcy * rcy) + rcz * rcz;
    bool ex0;
    {
        const float4 dt0 = depth_consts(K, 0u);
        const float tca = (rcx * dx + rcy * dy) + rcz * dz;
        const float d2 = rcc - tca * tca;
        const bool hb = valid && group_any<PW>(tca >= 0.0f) && group_any<PW>(d2 <= dt0.x);
        ex0 = hb && group_any<PW>(near_root(tca, d2, dt0.x) < dt0.w);
    }
    if (!wave_ballot(ex0)) return;
    maxd = 0;

    // ---- the wave's ray cone, around lane 36's ray (scattered packets make it wide: no cull then)
    {
        const float ax = readlane_f(dx, 36u), ay = readlane_f(dy, 36u), az = readlane_f(dz, 36u);
        stage_cone(L, lane, cone_cull, ax, ay, az, [&] { return cone_s2m(dx, dy, dz, ax, ay, az); });
    }

    // This lane's column of the cooperative child build (BuildLane's lanes). This traversal uses the levels' E words,
    // so every centre lane stores in place: child 8's centre from lanes 32 + 8 and 27..31 alike.
    const uint32_t bi = build_child(lane);
    const uint32_t bc = lane < 27u ? lane / 9u : 3u;
    // The leaf-threshold skip bounds t from below for every ray. In packet semantics a lane with tca < 0
    // can also pass LOD through another lane's bounding hit (negative t, SIMD_AVX.h:254), which that
    // bound does not cover: there the skip additionally needs every sphere of the child's subtree in
    // front of every lane (leaf_front below).
    const bool lod_cull = (K_flags & SF_FLAG_NO_LOD_CULL) == 0u;
    // Every sphere of a node's subtree lies inside its bounding sphere (radius 2r around its centre c).
    // If c.d >= 2r for every lane's unit direction d, each such sphere (centre c', radius R') has
    // c'.d - R' >= c.d - 2r >= 0, so its near root t >= 0 for every lane: no negative t, and the
    // per-ray leaf threshold applies. Checked as tca >= 0 and tca^2 >= (2r)^2 (1 + 2^-6), the margin
    // covering the rounding of tca, |d| and the threshold.
    auto leaf_front = [&](const float4 pc, float R2b) -> bool {
        const float tca = (pc.x * dx + pc.y * dy) + pc.z * dz;
        return wave_ballot(!(tca >= 0.0f && tca * tca >= R2b * (1.0f + 0x1p-6f))) == 0ull;
    };
    const float b[4] = { bcol.x, bcol.y, bcol.z, bcol.w };   // (build_column)
    const uint32_t slot = bc == 3u ? bi * 4u : SF_LDS_PLANE + bc * SF_LDS_COLS + bi * 3u;

    uint32_t d = 0;                 // uniform: depth of the open (expanded) node
    uint32_t idxB = 1;              // uniform: 9 x its heap index + 1 mod 2^32 (root 0, child i of n: 9n+1+i),
                                    // i.e. the heap index of its child 0

    // ---- the own sphere of a node with centre/|c|^2 `pc`, depth dd, heap index idx, tested when the node opens for
    // the lanes of actm: accept_self's rule (pre-order, a tie accepted iff the best is an ancestor) in packet form --
    // the hit test is the packet's, and there is no front-first order, so nothing is flagged
    auto self_test = [&](const float4 pc, uint32_t dd, uint64_t actm, uint32_t idx, float R2s) {
        const float tca = (pc.x * dx + pc.y * dy) + pc.z * dz;
        const float d2 = pc.w - tca * tca;
        const bool f0 = tca >= 0.0f, in = d2 <= R2s;
        const uint64_t hsm = actm & wave_ballot(group_any<PW>(f0) && group_any<PW>(in));
        if (hsm) {
            // (the general correctly rounded path only when a hitting lane's argument is tiny: a uniform branch)
            const float xs = R2s - d2;
            float ts;
            if ((wave_ballot(!(xs >= 0x1p-96f)) & hsm) != 0ull) ts = near_root_exact(tca, d2, R2s);
            else ts = near_root_big(tca, xs);
            const uint64_t eqm = wave_ballot(ts == h.minT);
            const uint64_t accm = hsm & (wave_ballot(ts < h.minT) | (eqm & ancm));
            sel_in_place(h.minT, ts, accm);
            sel_in_place(h.cx, pc.x, accm);
            sel_in_place(h.cy, pc.y, accm);
            sel_in_place(h.cz, pc.z, accm);
            sel_in_place(h.index, idx, accm);
            uint32_t hd = (uint32_t)h.depth;
            sel_in_place(hd, dd, accm);
            h.depth = (int32_t)hd;
            ancm |= accm;
        }
    };

    // ---- expand the node with centre/|c|^2 `pc` (depth d, columns in LDS): build its 9 child transforms into
    // table(d), then test the children (depth d+1) for the lanes in `act`. Returns this lane's 9-bit
    // "child expands" vector; pend = the wave's mask of children some lane expands; leafm = the children that are
    // inline leaves.
    // (pc: the node's {centre, cc}, read by the caller; its columns j = 0..2 (xyz) at col + j * cs, as build_children's)
    // (the node's own sphere is tested by the caller when the node is entered, before this)
    auto expand = [&](const float4 pc, const float* col, uint32_t cs, uint32_t d, bool act, uint32_t& pend,
                      uint32_t& leafm) -> uint32_t {
        d = __builtin_amdgcn_readfirstlane(d);   // wave-uniform: depth constants come by scalar loads
        lds_fence();
        const float3 p0 = *reinterpret_cast<const float3*>(col);
        const float3 p1 = *reinterpret_cast<const float3*>(col + cs);
        const float3 p2 = *reinterpret_cast<const float3*>(col + 2u * cs);
        // the wave's ray cone, read with the node (before this level's stores, see build_children)
        const float4 cn = *reinterpret_cast<const float4*>(L.cone());
        const float sinT = L.cone()[4];
        const float4 dtn = depth_consts(K, d);        // this node: (4/3) r
        const float4 dtc = depth_consts(K, d + 1u);   // children: (2r)^2, T
        // children's leaf threshold (+inf: no inline leaves when the LOD cull is off), loaded with the others
        const float leaf1 = depth_leaf(K, d + 1u);
        const float leafc = lod_cull ? leaf1 : __builtin_inff();
        // world = parent * child, as build_children's
        const float sm = bc == 3u ? dtn.z : 1.0f;
        const float b0 = b[0] * sm, b1 = b[1] * sm, b2 = b[2] * sm;
        const float x = __builtin_fmaf(pc.x, b[3], (p0.x * b0 + p1.x * b1) + p2.x * b2);
        const float y = __builtin_fmaf(pc.y, b[3], (p0.y * b0 + p1.y * b1) + p2.y * b2);
        const float z = __builtin_fmaf(pc.z, b[3], (p0.z * b0 + p1.z * b1) + p2.z * b2);
        const float w = (x * x + y * y) + z * z;   // Dot(centre, centre) on the centre lanes (bc = 3)
        // table(levels-1) is never read: entering a child of the deepest provisioned level overflows
        // first. Not allocated, not stored (uniform branch).
        if (d + 1u < levels) {
            float* const tb = L.table(d);
            *reinterpret_cast<float3*>(tb + slot) = make_float3(x, y, z);
            *(bc == 3u ? tb + slot + 3u : L.cone() + 5u) = w;
        }
        const float R2b = dtc.x;
        const float T = dtc.w;
        // Cone cull of child bi: build_children's test and slack, in its unfused form (each product and sum rounded
        // on its own, the regime condition as w > 2 (R2b + dl), dl = 2^-18 |c|^2).
        const float ax = cn.x, ay = cn.y, az = cn.z, cosT = cn.w;
        const float dl = w * 0x1p-18f;
        const float ca = (x * ax + y * ay) + z * az;
        const float sq = __builtin_amdgcn_sqrtf(__builtin_fmaxf(w - ca * ca, 0.0f));
        const float X = sq * cosT - ca * sinT;
        const float Y = X * X - (R2b + w * (0x1p-18f + 0x1p-19f));
        const float mk = __builtin_fminf(__builtin_fminf(ca, w - 2.0f * (R2b + dl)), __builtin_fminf(X, Y));
        uint32_t M = (uint32_t)(wave_ballot(!(mk > 0.0f)) >> 32) & 0x1ffu;
        M = __builtin_amdgcn_readfirstlane(M);
        SF_STAMP(6);
        uint32_t e = 0, pm = 0;
        // The children some ray of the cone can reach, in index order, with the early-outs over the PW lanes of a
        // reference packet. Child i's {centre, cc}: a broadcast LDS read of plane 0 of the table just stored (one
        // LDS instruction instead of four v_readlane on the VALU); the deepest provisioned level keeps no table,
        // there the centre lanes are read back. (The loop is instantiated for both sources, so the choice is not
        // re-tested in every iteration.) LOD by lod_expands' 2-ulp bracket, per lane.
        auto packet_loop = [&](auto tab) {
        const float* ctab = L.table(d);
        while (M) {
            const uint32_t i = __builtin_ctz(M);
            M &= M - 1u;
            float cx, cy, cz, cc;
            if constexpr (decltype(tab)::value) {
                const float4 c4 = *reinterpret_cast<const float4*>(ctab + i * 4u);
                cx = c4.x, cy = c4.y, cz = c4.z, cc = c4.w;
            } else {
                cx = readlane_f(x, 32u + i), cy = readlane_f(y, 32u + i);
                cz = readlane_f(z, 32u + i), cc = readlane_f(w, 32u + i);
            }
            const float tca = (cx * dx + cy * dy) + cz * dz;
            const float d2 = cc - tca * tca;
            const bool hb = act & group_any<PW>(tca >= 0.0f) & group_any<PW>(d2 <= R2b);
            if (wave_ballot(hb)) {
                const float xs = R2b - d2;
                const float sq = __builtin_amdgcn_sqrtf(xs);
                const float s_lo = __uint_as_float((uint32_t)max((int32_t)__float_as_uint(sq) - 2, 0));
                const float s_hi = __uint_as_float(__float_as_uint(sq) + 2u);
                const float t_hi = tca - s_lo;           // >= t
                const float t_lo = tca - s_hi;           // <= t
                float t_dec = t_hi < T ? t_hi : t_lo;    // on the same side of T as t when decided
                const bool undecided = hb & ((!(t_hi < T) & !(t_lo >= T)) | (xs < 0x1p-96f));
                if (wave_ballot(undecided)) t_dec = undecided ? near_root_exact(tca, d2, R2b) : t_dec;
                const bool exi = hb & group_any<PW>(t_dec < T);
                const uint64_t mi = wave_ballot(exi);
                e |= exi ? (1u << i) : 0u;
                pm |= (mi != 0ull ? 1u : 0u) << i;
            }
        }
        };
        if (d + 1u < levels) packet_loop(BoolC<true>{});
        else packet_loop(BoolC<false>{});
        // children of a node at the deepest provisioned level (no table) would need a level that does not exist:
        // flag the tile for the deeper re-trace instead of entering them
        if (d + 1u >= levels) {
            if (pm != 0u) status |= SF_STATUS_OVERFLOW;
            pm = 0u;
        }
        pend = pm;
        // children none of whose own children can pass LOD for any ray (sfhost::leaf_threshold of their depth;
        // |c|^2 of child i is w on lane 32 + i): entered as inline leaves
        leafm = (uint32_t)(wave_ballot(w > leafc) >> 32) & 0x1ffu;
        return e;
    };

    // DFS stack in VGPR lanes (lane L = level L): {pending children | leaves << 9}, heap index.
    // Lane selects: no LDS traffic and no lane-0-only region in the loop.
    uint32_t stk_pc = 0u, stk_ix = 0u;
    uint32_t pend = 0u, eN = 0u;
    uint32_t leafN = 0u;            // uniform: the open node's children that are inline leaves (bit i: child i)
    {
        // the root: its own sphere, then -- unless no child of it can pass LOD for any ray
        // (sfhost::leaf_threshold, with leaf_front) -- its children
        lds_fence();
        const float4 pc = *reinterpret_cast<const float4*>(L.root());
        self_test(pc, 0u, wave_ballot(ex0), 0u, depth_consts(K, 0u).y);
        if (!(lod_cull && __builtin_amdgcn_readfirstlane((int)(pc.w > depth_leaf(K, 0u))) &&
              leaf_front(pc, depth_consts(K, 0u).x)))
            eN = expand(pc, L.root() + 4u, 4u, 0u, ex0, pend, leafN);
        else SF_COUNT(4, 1);
    }

    for (;;) {
        d = __builtin_amdgcn_readfirstlane(d);
        SF_STAMP(0);
        if (pend) {
            // (bits 9..17 of leafN were the per-ray traversal's front children: always 0 here, but the compiler cannot
            // see that through the stack, and dropping the select changes the progressive kernels' code -- kept until a
            // measured change removes it)
            const uint32_t fp = pend & (leafN >> 9);
            const uint32_t c = __builtin_ctz(fp ? fp : pend);
            const uint32_t cbit = 1u << c;
            pend &= ~cbit;
            // (d + 1 < levels here: expand never leaves children pending at the deepest provisioned level)
            const bool a = (eN & cbit) != 0u;
            const uint64_t am = wave_ballot(a);
            const float* node = L.table(d) + c * 4u;
            // enter child c: its own sphere first (pre-order, self_test above), in one place for every child
            maxd = (int32_t)d + 1 > maxd ? (int32_t)d + 1 : maxd;   // Sphereflake.h:157-160
            const uint32_t ko = (d + 1u) << 5;   // byte offset of the child's depth constants
            lds_fence();
            const float4 pc = *reinterpret_cast<const float4*>(node);
            const float4 dc1 = depth_consts_at(K, ko);
            self_test(pc, d + 1u, am, idxB + c, dc1.y);
            // A child none of whose children can pass LOD for any ray (sfhost::leaf_threshold) only needs its
            // own sphere: no push, no level, no child build. (leafN: decided for all 9 children when the parent
            // expanded)
            if ((leafN & cbit) != 0u && leaf_front(pc, dc1.x)) {
                SF_COUNT(4, 1);
                SF_COUNT(8, 1);
                SF_COUNT(9, __builtin_popcountll(am));
                ancm &= wave_ballot(h.depth != (int32_t)d + 1);   // the child is finished
                continue;
            }
            // save the open node's state, enter child c
            stk_pc = writelane_u(pend | (leafN << 9), d, stk_pc);
            stk_ix = writelane_u(idxB, d, stk_ix);
            L.E(d)[lane] = (uint16_t)eN;
            idxB = 9u * (idxB + c) + 1u;
            d += 1u;
            SF_STAMP(1);
            eN = expand(pc, L.table(d - 1u) + SF_LDS_PLANE + 3u * c, SF_LDS_COLS, d, a, pend, leafN);
            SF_STAMP(2);
            continue;
        }
        // ---- the node at depth d is finished: a best sphere at depth d is no longer an ancestor
        ancm &= wave_ballot(h.depth != (int32_t)d);
        SF_STAMP(4);
        if (d == 0u) break;
        // ---- back to the parent
        d -= 1u;
        lds_fence();
        {
            const uint32_t pc = __builtin_amdgcn_readlane(stk_pc, d);
            pend = pc & 0x1ffu;
            leafN = pc >> 9;
            idxB = (uint32_t)__builtin_amdgcn_readlane(stk_ix, d);
        }
        eN = L.E(d)[lane];
        (void)__builtin_amdgcn_readfirstlane(eN);   // (stamp builds: close the pop segment after its reads)
        SF_STAMP(5);
    }
    h.hit = h.depth >= 0;
}

// ------------------------------------------------------------------------------------------
// Per-ray semantics (full frames): a child is entered as soon as its own test passes. The reference
// itself recurses into child i before testing child i + 1 (Sphereflake.h:162-172); traverse_packet above tests all
// children of a node first, keeps each lane's 9 "expands" bits in LDS and enters the pending children after.
// Per-ray, the tests of child i + 1 do not depend on anything child i's subtree does (bounding and LOD involve
// only the ray and the child; acceptance is the self test's, at entry), so entering at once gives the same
// visits, and the child test's values carry into the entry: its centre and |c|^2 (no second LDS read), tca and
// d2 (the self test's own, not recomputed), the expanding lanes (no per-lane E bits in LDS: no store at the
// push, no load at the pop). A node keeps on the VGPR stack its untested children (the cone-culled mask,
// front children first, as before) instead of its pending ones, and its visiting lanes as one bit per level
// (`actbits`).
// The depth seed of the occlusion cull (traverse_ray). The max-depth word stats[0] is a running maximum: it is raised
// only by depths some traversal really reached, and lowered only by a reset, which the host orders after every launch
// that updates it and completes before the next one. So a depth M read from the word during a launch -- or reached
// earlier by this wave in the launch, which publishes it to the same word -- is a lower bound of the word's value
// after the launch, and an occluded subtree that cannot pass LOD deeper than M cannot change that value.
struct DepthSeed {
    int32_t own = -1;    // uniform: the deepest node this wave reached so far under the word (-1: none)
    int32_t word = -1;   // stats_word(): the word as loaded, not yet made uniform -- depth() waits for the load, and
                         // trace_tile calls it after the unit's ray generation
    // The seed (uniform, >= 0), or -1 -- every tile on its own, as without the seed -- with the cull or the seed
    // switched off. (Depths are below 32, SF_MAX_DEPTH_LIMIT; the mask only keeps a corrupt word inside the depth
    // table, as a smaller seed: the cull reads depth seed + 1's threshold.)
    __device__ __forceinline__ int32_t depth(uint32_t flags) const
    {
        int32_t seed = -1;
        if ((flags & (SF_FLAG_NO_OCCL_CULL | SF_FLAG_NO_DEPTH_SEED)) == 0u) {
            const int32_t w = __builtin_amdgcn_readfirstlane(word);
            const int32_t o = __builtin_amdgcn_readfirstlane(own);
            const int32_t m = o > w ? o : w;
            seed = (m > 0 ? m : 0) & 31;
        }
        return __builtin_amdgcn_readfirstlane(seed);
    }
};
// The word: a relaxed agent-scope vector load of a uniform address (not a scalar load: the scalar cache is not
// coherent with the atomics that raise the word). A stale value is only a smaller seed.
__device__ __forceinline__ int32_t stats_word(const FrameArgs& a)
{
    return __hip_atomic_load(&a.stats[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Entry-order mask (bits c and 16 + c, see traverse_ray) of the children c of a node whose child 0 has heap index
// idxB that belong to subtree part q: (idxB + c) mod 4 == q.
__device__ __forceinline__ uint32_t split_mask(uint32_t q, uint32_t idxB)
{
    const uint32_t m9 = (0x111u << ((q - idxB) & 3u)) & 0x1ffu;
    return m9 | (m9 << 16);
}

// SPLIT: a subtree part unit (SF_FLAG_SUBTREE): of the nodes at depth split_depth, only those whose heap index is
// split_q mod 4 are entered (their own sphere and their subtree); everything above is traced as for the whole tile.
// SHADOW: the any-hit mode of sf_trace_shadow. Only the predicate "some visited sphere has
// ts < bound" is wanted per lane, so h.minT starts at the lane's `bound`, a lane whose self test accepts is finished
// and leaves the active set for good (actv, every bit of actbits), a tie is not an acceptance and never flags (it is
// not `<`), the occlusion cull keeps only its distance condition (no max-depth statistic to protect: maxd is not
// maintained past 0), and the traversal ends when no lane is live. On return h.depth >= 0 (h.hit) marks the finished
// lanes; the other fields of h are not maintained. The visits are a subset of the closest-hit traversal's and every
// sphere left out cannot be accepted below `bound`, so h.hit is exactly (the closest hit's min_t < bound).
// LEAFNODES: leaf-level nodes take leaf_children (the plain traversal only; the fixup's deep re-trace keeps the child loop).
template <bool COMPACT = false, bool SPLIT = false, bool SHADOW = false, bool LEAFNODES = !(COMPACT || SPLIT || SHADOW)>
__device__ __forceinline__ void traverse_ray(const DeviceConsts* __restrict__ K, const float* root, float* __restrict__ Lbase,
                                             const float4 bcol, uint32_t levels, float dx, float dy, float dz, bool valid,
                                             HitState& h, int32_t& maxd, uint32_t& status, uint32_t K_flags,
                                             uint64_t* phase_sums = nullptr, uint32_t axl = 36u,
                                             uint64_t* tile_counts = nullptr, uint32_t split_q = 0u,
                                             uint32_t split_depth = 0u, int32_t seed = -1, float bound = FLT_MAX)
{
    // seed (uniform; -1: none; DepthSeed::depth): a depth already counted in the stats word this traversal's maxd is
    // published to. The occlusion cull's depth bound starts from it.
    const uint32_t lane = threadIdx.x & 63u;
    const TraverseLds L{ Lbase };
    const bool cone_cull = (K_flags & SF_FLAG_NO_CONE_CULL) == 0u;
    const bool occl_cull = (K_flags & SF_FLAG_NO_OCCL_CULL) == 0u;
    const bool front_first = (K_flags & (SF_FLAG_NO_OCCL_CULL | SF_FLAG_NO_FRONT_FIRST)) == 0u;
    SF_STAMP_DECL;

    reset_hit(h, SHADOW ? bound : FLT_MAX);
    uint64_t ancm = 0ull;   // lanes whose current best sphere is an ancestor of the open node (see accept_self)

    // ---- root node (depth 0): bounding sphere + LOD, decided as a child's is (lod_expands with depth 0's constants)
    const float rcx = root[9], rcy = root[10], rcz = root[11];
    const float rcc = (rcx * rcx + rcy * rcy) + rcz * rcz;
    uint64_t ex0m;   // the lanes that expand the root
    {
        const float4 dt0 = depth_consts(K, 0u);
        const float tca = (rcx * dx + rcy * dy) + rcz * dz;
        const float d2 = rcc - tca * tca;
        const bool hb = valid && tca >= 0.0f && d2 <= dt0.x;
        const uint64_t hbm = wave_ballot(hb);
        if (hbm == 0ull) return;   // (maxd stays the caller's -1, whatever the seed: this traversal reached no depth)
        ex0m = lod_expands(tca, d2, dt0.x - d2, hb, hbm, dt0.x, dt0.w, depth_word_at(K, 0u, 6u));
        if (ex0m == 0ull) return;
    }
    maxd = 0;

    // ---- the wave's ray cone
    // (half units: axl = the centre pixel of the traced half, (4, 2) or (4, 6))
    {
        const float ax = readlane_f(dx, axl), ay = readlane_f(dy, axl), az = readlane_f(dz, axl);
        stage_cone(L, lane, cone_cull, ax, ay, az, [&] { return cone_s2m(dx, dy, dz, ax, ay, az); });
    }

    // The cull's depth bound starts from the seed: the word maxd is published to holds at least that already, so the
    // cull below skips every occluded subtree that cannot pass LOD deeper than max(maxd, seed). maxd itself stays the
    // depth this traversal reached (started from the seed it would be carried through the loops in a VGPR: +7 % VALU).
    // uniform: depth max(maxd, seed) + 1's LOD threshold, reloaded when maxd grows beyond the seed
    float cull_t = depth_consts(K, (uint32_t)(seed > 0 ? seed : 0) + 1u).w;

    const BuildLane B = build_lane(bcol, lane, build_child(lane));

    uint32_t d = 0;      // uniform: depth of the open node
    uint32_t idxB = 1;   // uniform: the heap index of the open node's child 0 (9 n + 1)

    // (the own sphere of a node, tested when it is entered: accept_self)
    auto self_test = [&](const float4 pc, float tca, float d2, uint32_t dd, float actv, uint32_t idx,
                         float R2s) -> uint64_t {
        return accept_self<SHADOW>(h, ancm, status, front_first, pc, tca, d2, dd, actv, idx, R2s);
    };

    const uint32_t lv32 = __builtin_amdgcn_readfirstlane(levels << 5);   // levels, in depth-constant offset units
    const uint32_t index_order = front_first ? 0u : 0x1ffu;
    // (expand_node for this traversal's ray. tb: table(d), ko: d + 1's constants offset -- the caller's carried values,
    // not formed here again; kp: the caller passes the axis lane's tca of the node, (pc.x ax + pc.y ay) + pc.z az on the
    // same operands -- the cone axis IS that lane's direction)
    // (lf: the children's constants, and whether they are all inline leaves with their table stored -- leaf_children)
    auto expand = [&](const float4 pc, const float* col, uint32_t cs, uint32_t d, float actv,
                      float* tb, uint32_t ko, float kp, LeafLevel& lf) -> uint32_t {
        d = __builtin_amdgcn_readfirstlane(d);
        SF_COUNT(0, 1);
        SF_COUNT(7, __builtin_popcountll(wave_ballot(actv >= 0.0f)));   // (COUNTS builds: lanes visiting the node)
        const ChildBuild cb = build_children(K, L, B, pc, col, cs, ko, kp, index_order);
        lf.dc = cb.dtc;
        lf.on = false;
        // (one levels test for both outcomes: stored after the cull, the table is read only once this returns)
        if (ko < lv32) {   // (d + 1 < levels)
            *reinterpret_cast<float3*>(tb + B.slot) = make_float3(cb.x, cb.y, cb.z);
            *(B.bc == 3u ? tb + B.slot + 3u : L.cone() + 5u) = cb.w;
            lf.on = cb.leaf_level;
            return (cb.M & cb.front) | ((cb.M & ~cb.front) << 16);
        }
        {   // (d + 1 >= levels)
            const float R2b = cb.dtc.x, T = cb.dtc.w, Tfar = depth_word_at(K, ko, 6u);   // (depth8: far)
            uint32_t M = cb.M;
            while (M) {
                const uint32_t i = __builtin_ctz(M);
                M &= ~(1u << i);
                const float cx = readlane_f(cb.x, 32u + i), cy = readlane_f(cb.y, 32u + i);
                const float cz = readlane_f(cb.z, 32u + i), cc = readlane_f(cb.w, 32u + i);
                if (child_expands(cx, cy, cz, cc, dx, dy, dz, actv, R2b, T, Tfar)) {
                    status |= SF_STATUS_OVERFLOW;
                    break;
                }
            }
            return 0u;
        }
    };

    uint32_t stk_pc = 0u, stk_ix = 0u;   // VGPR stack, lane k = level k: untested children, idxB
    float* tcur = L.table(0u);           // uniform: L.table(d), moved at push / pop (not formed per child)
    uint32_t kofs = 1u << 5;             // uniform: byte offset of depth d + 1's constants, moved likewise
    float R2c = depth_consts_at(K, kofs).x;   // uniform: depth d + 1's bounding radius^2, reloaded likewise
    uint32_t C = 0u;                     // uniform: the open node's untested children in entry order (child i at bit
                                         // i if it is a front child, else at bit 16 + i)
    float actv;                          // per lane: +inf if the lane visits the open node, -1 otherwise
    uint32_t actbits;                    // per lane: bit k set if the lane visits the open node's level-k ancestor
    {
        lds_fence();
        const float4 pc = *reinterpret_cast<const float4*>(L.root());
        actv = sel_mask(-1.0f, __builtin_inff(), ex0m);
        actbits = 0u;
        sel_in_place(actbits, 1u, ex0m);
        const float tca = (pc.x * dx + pc.y * dy) + pc.z * dz;
        const float d2 = pc.w - tca * tca;
        const uint64_t acc0 = self_test(pc, tca, d2, 0u, actv, 0u, depth_consts(K, 0u).y);
        bool live = true;   // (uniform)
        if constexpr (SHADOW) {   // the lanes the root's sphere finished leave; with none left nothing is expanded
            actv = sel_mask(actv, -1.0f, acc0);
            sel_in_place(actbits, 0u, acc0);
            live = wave_ballot(actbits != 0u) != 0ull;
        }
        LeafLevel lf0;   // (the root is opened as ever)
        if (live && !__builtin_amdgcn_readfirstlane((int)(pc.w > depth_leaf(K, 0u))))
            C = expand(pc, L.root() + 4u, 4u, 0u, actv, tcur, kofs, readlane_f(tca, axl), lf0);
        else SF_COUNT(4, 1);
        if constexpr (SPLIT) {
            if (split_depth == 1u) C &= split_mask(split_q, 1u);
        }
    }

    // (the scalar unit is shared by the CU's four SIMDs and measured ~3x a VALU op per instruction here: the child
    // loop keeps its scalar bookkeeping to a find-first-set, a clear-lowest and the index)
    for (;;) {
        d = __builtin_amdgcn_readfirstlane(d);
        SF_STAMP(0);
        if (C) {
            const uint32_t p = __builtin_ctz(C);
            __asm__("s_bitset0_b32 %0, %1" : "+s"(C) : "s"(p));   // (one scalar op; C &= C - 1 is two)
            const uint32_t c = p & 15u;   // (front child p, or child p - 16)
            // the children's depth constants (scalar loads, in flight with the centre's LDS read)
            const float4 dc = depth_consts_at(K, kofs);
            lds_fence();
            const float4 pc = *reinterpret_cast<const float4*>(tcur + c * 4u);
            const float tca = (pc.x * dx + pc.y * dy) + pc.z * dz;
            const float d2 = pc.w - tca * tca;
            // bounding (SIMD_AVX.h:247-258) for the visiting lanes: one v_min3 compare, its VCC the branch
            const float xs = R2c - d2;
            const bool hb = __builtin_fminf(__builtin_fminf(tca, xs), actv) >= 0.0f;
            const uint64_t hbm = wave_ballot(hb);
            SF_COUNT(1, 1);
#ifdef SF_COUNTS
            {   // lane utilisation of the child loop (COUNTS builds only)
                const uint32_t na = __builtin_popcountll(wave_ballot(actv >= 0.0f));
                SF_COUNT(5, na);
                SF_COUNT(6, __builtin_popcountll(hbm));
                SF_COUNT(14, na <= 32u ? 1 : 0);
            }
#endif
            if (hbm == 0ull) {
                SF_COUNT(2, 1);
                continue;
            }
            // depth d + 1's {leaf, cull, far} words: one scalar load
            const float4 dk = depth_consts_at(K, kofs + 16u);
            const float Tfar = dk.z;     // (depth8: far)
            const float cull_r = dk.y;   // (depth8: cull)
            const uint64_t exm = lod_expands(tca, d2, xs, hb, hbm, dc.x, dc.w, Tfar);
            SF_STAMP(2);
            if (exm == 0ull) continue;
            // ---- child c passed bounding + LOD for the lanes of exm: enter it
            SF_COUNT(3, 1);
            if (!SHADOW && (int32_t)d + 1 > maxd) {   // Sphereflake.h:157-160
                maxd = (int32_t)d + 1;
                if ((int32_t)d + 1 > seed) cull_t = depth_consts_at(K, kofs + (1u << 5)).w;
            }
            // occlusion cull (occluded): lanes for which no sphere of the child's subtree can be accepted or
            // pass LOD deeper than the depth already reached do not enter. "Already reached" is max(maxd, seed):
            // the seed is a depth the stats word already holds (the word is a running maximum, only raised by depths
            // really reached and only lowered by a reset, which is ordered after every launch), so a subtree that
            // cannot go deeper than it cannot change the word's final value -- and the pixels never depend on this
            // condition.
            uint64_t amx = exm;
            if (occl_cull) {
                amx = exm & ~occluded<SHADOW>(tca, h.minT, cull_t, cull_r);
                SF_COUNT(13, 1);
                SF_COUNT(12, amx == 0ull ? 1 : 0);
                if (amx == 0ull) continue;
            }
            float avx = sel_mask(-1.0f, __builtin_inff(), amx);
            const uint64_t acc = self_test(pc, tca, d2, d + 1u, avx, idxB + c, dc.y);
            SF_STAMP(4);
            if constexpr (SHADOW) {
                if (acc != 0ull) {   // finished lanes leave the child, the open node and every ancestor
                    amx &= ~acc;
                    avx = sel_mask(avx, -1.0f, acc);
                    actv = sel_mask(actv, -1.0f, acc);
                    sel_in_place(actbits, 0u, acc);
                    if (wave_ballot(actbits != 0u) == 0ull) break;   // no lane is live
                    if (amx == 0ull) continue;
                }
            }
            // an inline leaf -- its own sphere only (sfhost::leaf_threshold): |c|^2 beyond depth d + 1's leaf
            // threshold; the centre's w is broadcast, so one compare is the branch (round 5: no per-level leaf mask
            // formed at the expansion and carried through the stack)
            // (the leaf skip is always on in this traversal: SF_FLAG_NO_LOD_CULL is the packet traversal's A/B switch)
            if (wave_ballot(pc.w > dk.x) != 0ull) {
                SF_COUNT(4, 1);
                SF_COUNT(8, 1);
                SF_COUNT(9, __builtin_popcountll(amx));
                ancm &= wave_ballot(h.depth != (int32_t)d + 1);   // the child is finished
                continue;
            }
            const float* const col = tcur + SF_LDS_PLANE + 3u * c;   // the entered child's axis columns
            // push the open node, open child c
            auto push = [&]() {
                stk_pc = writelane_s(C, d, stk_pc);
                stk_ix = writelane_s(idxB, d, stk_ix);
                {
                    const uint32_t bit = 2u << d;   // level d + 1
                    uint32_t ab = actbits & ~bit;
                    sel_in_place(ab, ab | bit, amx);
                    actbits = ab;
                }
                idxB = 9u * (idxB + c) + 1u;
                d += 1u;
                actv = avx;
                tcur += SF_LDS_LEVEL;
                kofs += 1u << 5;
            };
            LeafLevel lf;
            if constexpr (LEAFNODES) {
                // child c's children are built first: if they are all inline leaves (at depth d + 2, already counted
                // in the max-depth statistic), leaf_children tests them from here and the open node stays open
                SF_STAMP(1);
                const uint32_t Cn = expand(pc, col, SF_LDS_COLS, d + 1u, avx, tcur + SF_LDS_LEVEL, kofs + (1u << 5),
                                           readlane_f(tca, axl), lf);
                if (lf.on && (Cn == 0u || (int32_t)d + 2 <= (maxd > seed ? maxd : seed))) {   // (no child kept: nothing to count)
                    SF_COUNT(10, 1);
                    SF_COUNT(11, __builtin_popcount(Cn));
                    leaf_children(h, ancm, status, front_first, occl_cull, tcur + SF_LDS_LEVEL, Cn, dx, dy, dz, avx,
                                  9u * (idxB + c) + 1u, d + 2u, lf.dc, depth_consts_at(K, kofs + (1u << 5) + 16u), cull_t);
                    ancm &= wave_ballot(h.depth != (int32_t)d + 1);   // child c is finished
                    SF_STAMP(6);
                    continue;
                }
                push();
                C = Cn;
            } else {
                push();
                SF_STAMP(1);
                C = expand(pc, col, SF_LDS_COLS, d, avx, tcur, kofs, readlane_f(tca, axl), lf);
            }
            if constexpr (SPLIT) {   // (the children are at depth d + 1)
                if (d + 1u == split_depth) C &= split_mask(split_q, idxB);
            }
            // (depth d + 1's bounding radius^2, the open node's children's: with LEAFNODES the expansion has it)
            if constexpr (LEAFNODES) R2c = lf.dc.x;
            else R2c = depth_consts_at(K, kofs).x;
            if (COMPACT && C != 0u) {
                // ---- Active-ray compaction of sparse nodes (north star: "wavefront ballot / prefix-sum active-ray
                // compaction down the recursion"; sf_trace_queue2c, opt-in). Deep in the tree a node is often visited
                // by a handful of the tile's rays, and each of its children then costs a wave-wide test for those few
                // lanes. Where at most 7 lanes visit the node and 3 or more children are left, the visiting rays are
                // packed by their prefix-sum rank (mbcnt of the ballot) into 7 LDS slots, replicated into 9 groups of 7
                // lanes, and group g tests child g: every child's bounding test in ONE wave pass, the same float
                // operations on bit-identical directions. Children no visiting ray hits leave the mask; the loop then
                // tests the others per lane as before. A filter: no decision changes (results bit for bit).
                __builtin_amdgcn_sched_barrier(0);   // (not interleaved with the expansion: register pressure)
                const uint64_t actm = wave_ballot(avx > 0.0f);
                const uint32_t na = (uint32_t)__builtin_popcountll(actm);
                const uint32_t M = (C | (C >> 16)) & 0x1ffu;   // the untested children by index
                if (na <= 7u && __builtin_popcount(M) >= 3) {
                    const float R2b = depth_consts(K, d + 1u).x;
                    // pack through the level's E words (unused by this traversal): visiting lane of rank k writes its
                    // direction to slot k (16 B), the others to a junk slot; every lane reads the slot of its group
                    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(actm >> 32),
                                                                    __builtin_amdgcn_mbcnt_lo((uint32_t)actm, 0u));
                    float* const sc = reinterpret_cast<float*>(L.E(d)) + 1;   // (16-byte aligned; 32 floats)
                    *reinterpret_cast<float4*>(sc + (avx > 0.0f ? 4u * rank : 28u)) = make_float4(dx, dy, dz, 0.0f);
                    lds_fence();
                    uint32_t ln = lane;
                    __asm__ volatile("" : "+v"(ln));   // (formed here, not hoisted and kept live across the DFS)
                    const uint32_t g = (ln * 37u) >> 8;   // lane / 7 (exact for lanes 0..63)
                    const uint32_t sl = ln - 7u * g;      // lane % 7
                    const float4 q = *reinterpret_cast<const float4*>(sc + 4u * sl);
                    const bool ok = sl < na && g < 9u && ((M >> g) & 1u) != 0u;
                    const uint32_t gi = g < 9u ? g : 8u;
                    const float4 cg = *reinterpret_cast<const float4*>(L.table(d) + gi * 4u);   // child g
                    const float tca = (cg.x * q.x + cg.y * q.y) + cg.z * q.z;
                    const float d2 = cg.w - tca * tca;
                    const float xs = R2b - d2;
                    const uint64_t bal =
                        wave_ballot(__builtin_fminf(__builtin_fminf(tca, xs), ok ? __builtin_inff() : -1.0f) >= 0.0f);
                    // child k is hit by some visiting ray iff bits 7k..7k+6 of the ballot are not all zero (lane k asks)
                    const uint32_t kk = ln < 9u ? ln : 0u;
                    const uint64_t grp = (bal >> (7u * kk)) & 0x7full;
                    const uint32_t hitm = (uint32_t)wave_ballot(ln < 9u && grp != 0ull) & 0x1ffu;
                    const uint32_t keep = __builtin_amdgcn_readfirstlane(hitm);
                    C &= keep | (keep << 16);
                }
            }
            SF_STAMP(6);
            continue;
        }
        // ---- the node at depth d is finished: a best sphere at depth d is no longer an ancestor
        ancm &= wave_ballot(h.depth != (int32_t)d);
        if (d == 0u) break;
        d -= 1u;
        tcur -= SF_LDS_LEVEL;
        kofs -= 1u << 5;
        R2c = depth_consts_at(K, kofs).x;
        {
            const uint32_t pw = __builtin_amdgcn_readlane(stk_pc, d);
            C = pw;
            idxB = (uint32_t)__builtin_amdgcn_readlane(stk_ix, d);
        }
        actv = ((actbits >> d) & 1u) ? __builtin_inff() : -1.0f;
        SF_STAMP(5);
    }
    h.hit = h.depth >= 0;
    SF_STAMP_FLUSH(phase_sums);
#ifdef SF_COUNTS
    if (tile_counts) {
        auto sat = [](uint64_t v) { return v > 0xffffull ? 0xffffull : v; };
        *tile_counts = sat(ph_sum[0]) | (sat(ph_sum[1]) << 16) | (sat(ph_sum[1] - ph_sum[2]) << 32) | (sat(ph_sum[8]) << 48);
    }
#else
    (void)tile_counts;
#endif
}

// ---- The pair unit (sf_trace_queue1): two horizontally adjacent 8x8 tiles traced by one wave. Lane l
// carries ray A (its pixel of the left tile) and ray B (the same pixel of the right tile). Neighbouring tiles walk the
// same upper nodes of the flake; the pair walks them once: one LDS level table, one VGPR stack, one cone, one child
// build, cone cull, push and pop per node for both rays. Everything per ray -- the direction, the hit, the visiting
// lanes (actv, actbits), the ancestor mask -- is doubled (PairRay, ancm), and every per-ray float operation is exactly
// the one traverse_ray does on that ray, so results are the single tile's bit for bit. A branch the one-ray loop takes
// on a ballot is taken on the union of the two rays' ballots.
// A child that no lane enters with both its rays stays so for its whole subtree (a lane's activity only shrinks down
// the tree): every lane has at most one ray in it, so it runs the one-ray loop (dfs_one) on the "A" registers until it
// pops back to the level it was entered from. Around it the lanes that enter with ray B exchange their two register
// sets (one_ray_subtree): there A's set carries ray B, and B's set parks ray A, which does not visit the subtree. A
// child of one tile only is the special case (no lane, or every entering lane, exchanged); the other is a node that
// straddles the tiles' boundary with a footprint under 9 pixels, entered by A's right columns and B's left ones.
// Nothing the one-ray loop reads is a tile's: the cone, kp (from the cone's axis), maxd, cull_t and status are the
// unit's, and the overflow test at the deepest level takes both sets (the parked rays have actv -1).
struct PairRay {
    float dx, dy, dz;
    HitState h;
    float actv;         // +inf if the lane's ray visits the open node, -1 otherwise
    uint32_t actbits;   // bit k set if it visits the open node's level-k ancestor
};

__device__ __forceinline__ void traverse_pair(const DeviceConsts* __restrict__ K, const float* root, float* __restrict__ Lbase,
                                              const float4 bcol, uint32_t levels, PairRay& ra, PairRay& rb, bool validA,
                                              bool validB, int32_t& maxd, uint32_t& status, uint32_t K_flags,
                                              int32_t seed)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t axl = 39u;   // ray A of pixel (7, 4) of the left tile: next to the pair's centre
    const TraverseLds L{ Lbase };
    const bool cone_cull = (K_flags & SF_FLAG_NO_CONE_CULL) == 0u;
    const bool occl_cull = (K_flags & SF_FLAG_NO_OCCL_CULL) == 0u;
    const bool front_first = (K_flags & (SF_FLAG_NO_OCCL_CULL | SF_FLAG_NO_FRONT_FIRST)) == 0u;

    reset_hit(ra.h, FLT_MAX);
    reset_hit(rb.h, FLT_MAX);
    uint64_t ancA = 0ull, ancB = 0ull;   // per ray: lanes whose best sphere is an ancestor of the open node

    // ---- root: bounding + LOD per ray; the pair leaves only when neither ray expands the root
    const float rcx = root[9], rcy = root[10], rcz = root[11];
    const float rcc = (rcx * rcx + rcy * rcy) + rcz * rcz;
    uint64_t ex0A = 0ull, ex0B = 0ull;
    {
        const float4 dt0 = depth_consts(K, 0u);
        const float Tfar0 = depth_word_at(K, 0u, 6u);
        auto root_lod = [&](const PairRay& r, bool valid) -> uint64_t {
            const float tca = (rcx * r.dx + rcy * r.dy) + rcz * r.dz;
            const float d2 = rcc - tca * tca;
            const bool hb = valid && tca >= 0.0f && d2 <= dt0.x;
            const uint64_t hbm = wave_ballot(hb);
            if (hbm == 0ull) return 0ull;
            return lod_expands(tca, d2, dt0.x - d2, hb, hbm, dt0.x, dt0.w, Tfar0);
        };
        ex0A = root_lod(ra, validA);
        ex0B = root_lod(rb, validB);
        if ((ex0A | ex0B) == 0ull) return;
    }
    maxd = 0;

    // ---- one cone for both rays
    // (the axis: ray A of the axis lane; the one-ray loop's kp reads it back from the cone block, see build_children)
    const float ax = readlane_f(ra.dx, axl), ay = readlane_f(ra.dy, axl), az = readlane_f(ra.dz, axl);
    {
        // (cone_s2m's text on a ray held by reference: called as a function, the compiler commutes two of its additions)
        auto s2m_of = [&](const PairRay& r) -> float {
            const float cx_ = r.dy * az - r.dz * ay, cy_ = r.dz * ax - r.dx * az, cz_ = r.dx * ay - r.dy * ax;
            const float s2 = (cx_ * cx_ + cy_ * cy_) + cz_ * cz_;
            const bool fwd = (r.dx * ax + r.dy * ay) + r.dz * az > 0.0f;
            return fwd ? s2 : 1.0f;
        };
        // (the lane as an opaque value: its compares in stage_cone are then formed here, per unit -- hoisted out of the
        // unit loop they were carried through the whole traversal as 64-bit masks, and spilled)
        uint32_t ln = lane;
        __asm__ volatile("" : "+v"(ln));
        stage_cone(L, ln, cone_cull, ax, ay, az, [&] { return __builtin_fmaxf(s2m_of(ra), s2m_of(rb)); });
    }

    float cull_t = depth_consts(K, (uint32_t)(seed > 0 ? seed : 0) + 1u).w;

    const BuildLane B = build_lane(bcol, lane, build_child(lane));

    uint32_t d = 0;
    uint32_t idxB = 1;

    auto self_test = [&](PairRay& r, uint64_t& ancm, const float4 pc, float tca, float d2, uint32_t dd, float actv,
                         uint32_t idx, float R2s) {
        accept_self<false>(r.h, ancm, status, front_first, pc, tca, d2, dd, actv, idx, R2s);
    };

    const uint32_t lv32 = __builtin_amdgcn_readfirstlane(levels << 5);
    const uint32_t index_order = front_first ? 0u : 0x1ffu;
    // (expand_node for both rays: at the deepest provisioned level a ray that does not visit the node has actv -1 and
    // passes nothing. actvA / actvB: the two rays' lanes visiting the node, which is not open yet; lf: as traverse_ray's)
    // (kp_cone: BoolC<true> -- kp from the cone axis, see build_children)
    auto expand = [&](const float4 pc, const float* col, uint32_t cs, float* tb, uint32_t ko, float kp, auto kp_cone,
                      float actvA, float actvB, LeafLevel& lf) -> uint32_t {
        const ChildBuild cb = build_children<decltype(kp_cone)::value>(K, L, B, pc, col, cs, ko, kp, index_order);
        lf.dc = cb.dtc;
        lf.on = false;
        if (ko < lv32) {
            *reinterpret_cast<float3*>(tb + B.slot) = make_float3(cb.x, cb.y, cb.z);
            *(B.bc == 3u ? tb + B.slot + 3u : L.cone() + 5u) = cb.w;
            lf.on = cb.leaf_level;
            return (cb.M & cb.front) | ((cb.M & ~cb.front) << 16);
        }
        {
            const float R2b = cb.dtc.x, T = cb.dtc.w, Tfar = depth_word_at(K, ko, 6u);
            uint32_t M = cb.M;
            while (M) {
                const uint32_t i = __builtin_ctz(M);
                M &= ~(1u << i);
                const float cx = readlane_f(cb.x, 32u + i), cy = readlane_f(cb.y, 32u + i);
                const float cz = readlane_f(cb.z, 32u + i), cc = readlane_f(cb.w, 32u + i);
                auto passes = [&](const PairRay& r, float actv) -> bool {
                    return child_expands(cx, cy, cz, cc, r.dx, r.dy, r.dz, actv, R2b, T, Tfar);
                };
                if (passes(ra, actvA) || passes(rb, actvB)) {
                    status |= SF_STATUS_OVERFLOW;
                    break;
                }
            }
            return 0u;
        }
    };

    uint32_t stk_pc = 0u, stk_ix = 0u;
    float* tcur = L.table(0u);
    uint32_t kofs = 1u << 5;
    float R2c = depth_consts_at(K, kofs).x;
    uint32_t C = 0u;

    // ---- the one-ray loop (traverse_ray's) on ray A's registers, from the open node at depth `base`, whose children
    // are in C, until that node is finished (C == 0 at depth base; its pop is the caller's)
    auto dfs_one = [&](const uint32_t base) {
        for (;;) {
            d = __builtin_amdgcn_readfirstlane(d);
            if (C) {
                const uint32_t p = __builtin_ctz(C);
                __asm__("s_bitset0_b32 %0, %1" : "+s"(C) : "s"(p));
                const uint32_t c = p & 15u;
                const float4 dc = depth_consts_at(K, kofs);
                lds_fence();
                const float4 pc = *reinterpret_cast<const float4*>(tcur + c * 4u);
                const float tca = (pc.x * ra.dx + pc.y * ra.dy) + pc.z * ra.dz;
                const float d2 = pc.w - tca * tca;
                const float xs = R2c - d2;
                const bool hb = __builtin_fminf(__builtin_fminf(tca, xs), ra.actv) >= 0.0f;
                const uint64_t hbm = wave_ballot(hb);
                if (hbm == 0ull) continue;
                const float4 dk = depth_consts_at(K, kofs + 16u);
                const float Tfar = dk.z;
                const float cull_r = dk.y;
                const uint64_t exm = lod_expands(tca, d2, xs, hb, hbm, dc.x, dc.w, Tfar);
                if (exm == 0ull) continue;
                if ((int32_t)d + 1 > maxd) {
                    maxd = (int32_t)d + 1;
                    if ((int32_t)d + 1 > seed) cull_t = depth_consts_at(K, kofs + (1u << 5)).w;
                }
                uint64_t amx = exm;
                if (occl_cull) {
                    amx = exm & ~occluded<false>(tca, ra.h.minT, cull_t, cull_r);
                    if (amx == 0ull) continue;
                }
                const float avx = sel_mask(-1.0f, __builtin_inff(), amx);
                self_test(ra, ancA, pc, tca, d2, d + 1u, avx, idxB + c, dc.y);
                if (wave_ballot(pc.w > dk.x) != 0ull) {
                    ancA &= wave_ballot(ra.h.depth != (int32_t)d + 1);
                    continue;
                }
                // child c's children first (traverse_ray): a leaf-level node is not opened
                // (kp from the axis itself: the axis lane's tca of the node, whichever ray these registers hold)
                LeafLevel lf;
                const uint32_t Cn = expand(pc, tcur + SF_LDS_PLANE + 3u * c, SF_LDS_COLS, tcur + SF_LDS_LEVEL,
                                           kofs + (1u << 5), 0.0f, BoolC<true>(), avx, rb.actv, lf);
                if (lf.on && (Cn == 0u || (int32_t)d + 2 <= (maxd > seed ? maxd : seed))) {   // (no child kept: nothing to count)
                    leaf_children(ra.h, ancA, status, front_first, occl_cull, tcur + SF_LDS_LEVEL, Cn, ra.dx, ra.dy, ra.dz,
                                  avx, 9u * (idxB + c) + 1u, d + 2u, lf.dc, depth_consts_at(K, kofs + (1u << 5) + 16u), cull_t);
                    ancA &= wave_ballot(ra.h.depth != (int32_t)d + 1);
                    continue;
                }
                stk_pc = writelane_s(C, d, stk_pc);
                stk_ix = writelane_s(idxB, d, stk_ix);
                {
                    const uint32_t bit = 2u << d;
                    uint32_t ab = ra.actbits & ~bit;
                    sel_in_place(ab, ab | bit, amx);
                    ra.actbits = ab;
                }
                idxB = 9u * (idxB + c) + 1u;
                d += 1u;
                ra.actv = avx;
                tcur += SF_LDS_LEVEL;
                kofs += 1u << 5;
                C = Cn;
                R2c = lf.dc.x;
                continue;
            }
            ancA &= wave_ballot(ra.h.depth != (int32_t)d);
            if (d == base) break;
            d -= 1u;
            tcur -= SF_LDS_LEVEL;
            kofs -= 1u << 5;
            R2c = depth_consts_at(K, kofs).x;
            C = (uint32_t)__builtin_amdgcn_readlane(stk_pc, d);
            idxB = (uint32_t)__builtin_amdgcn_readlane(stk_ix, d);
            ra.actv = ((ra.actbits >> d) & 1u) ? __builtin_inff() : -1.0f;
        }
    };
    // the subtree of the open node (depth d) when no lane visits it with both rays (mB: the lanes whose ray B does):
    // the one-ray loop on A's registers, with the lanes of mB exchanged between the two sets around it -- there A's
    // registers carry ray B and B's park ray A, which does not visit the node. v_swap_b32 under EXEC = mB: one VALU
    // instruction per register, in place; the exchange is its own inverse.
    auto exchange = [&](const uint64_t mB) {
        {
            // (EXEC kept in VCC meanwhile: no SGPR pair of its own)
            __asm__("s_mov_b64 vcc, exec\n\t"
                    "s_mov_b64 exec, %22\n\t"
                    "v_swap_b32 %0, %11\n\t"
                    "v_swap_b32 %1, %12\n\t"
                    "v_swap_b32 %2, %13\n\t"
                    "v_swap_b32 %3, %14\n\t"
                    "v_swap_b32 %4, %15\n\t"
                    "v_swap_b32 %5, %16\n\t"
                    "v_swap_b32 %6, %17\n\t"
                    "v_swap_b32 %7, %18\n\t"
                    "v_swap_b32 %8, %19\n\t"
                    "v_swap_b32 %9, %20\n\t"
                    "v_swap_b32 %10, %21\n\t"
                    "s_mov_b64 exec, vcc"
                    : "+v"(ra.dx), "+v"(ra.dy), "+v"(ra.dz), "+v"(ra.h.minT), "+v"(ra.h.cx), "+v"(ra.h.cy), "+v"(ra.h.cz),
                      "+v"(ra.h.index), "+v"(ra.h.depth), "+v"(ra.actv), "+v"(ra.actbits), "+v"(rb.dx), "+v"(rb.dy),
                      "+v"(rb.dz), "+v"(rb.h.minT), "+v"(rb.h.cx), "+v"(rb.h.cy), "+v"(rb.h.cz), "+v"(rb.h.index),
                      "+v"(rb.h.depth), "+v"(rb.actv), "+v"(rb.actbits)
                    : "s"(mB)
                    : "vcc");
            const uint64_t x = (ancA ^ ancB) & mB;
            ancA ^= x;
            ancB ^= x;
        }
    };
    auto one_ray_subtree = [&](const uint64_t mB) {
        if (mB) exchange(mB);
        dfs_one(d);
        if (mB) exchange(mB);
    };
    // likewise the children of a leaf-level node that no lane enters with both rays (mB: the lanes entering with ray
    // B; avx: the entering lanes of either ray): the one-ray leaf_children between the two exchanges
    auto one_ray_leaves = [&](const uint64_t mB, const float* tb, uint32_t Cl, float avx, uint32_t idx0, uint32_t dd,
                              const LeafLevel& lf) {
        if (mB) exchange(mB);
        leaf_children(ra.h, ancA, status, front_first, occl_cull, tb, Cl, ra.dx, ra.dy, ra.dz, avx, idx0, dd, lf.dc, depth_consts_at(K, kofs + (1u << 5) + 16u),
                      cull_t);
        if (mB) exchange(mB);
    };

    {
        lds_fence();
        const float4 pc = *reinterpret_cast<const float4*>(L.root());
        const float R2s0 = depth_consts(K, 0u).y;
        auto enter_root = [&](PairRay& r, uint64_t& ancm, uint64_t ex0m) -> float {
            r.actv = sel_mask(-1.0f, __builtin_inff(), ex0m);
            r.actbits = 0u;
            sel_in_place(r.actbits, 1u, ex0m);
            const float tca = (pc.x * r.dx + pc.y * r.dy) + pc.z * r.dz;
            const float d2 = pc.w - tca * tca;
            self_test(r, ancm, pc, tca, d2, 0u, r.actv, 0u, R2s0);
            return tca;
        };
        const float tcaA = enter_root(ra, ancA, ex0A);
        enter_root(rb, ancB, ex0B);
        LeafLevel lf0;   // (the root is opened as ever)
        if (!__builtin_amdgcn_readfirstlane((int)(pc.w > depth_leaf(K, 0u))))
            C = expand(pc, L.root() + 4u, 4u, tcur, kofs, readlane_f(tcaA, axl), BoolC<false>(), ra.actv, rb.actv, lf0);
    }
    if ((ex0A & ex0B) == 0ull) {   // no lane expands the root with both rays (one half empty, or missing the root, is
        one_ray_subtree(ex0B);     // the common case): the one-ray loop from the start
        C = 0u;
    }

    for (;;) {
        d = __builtin_amdgcn_readfirstlane(d);
        if (C) {
            const uint32_t p = __builtin_ctz(C);
            __asm__("s_bitset0_b32 %0, %1" : "+s"(C) : "s"(p));
            const uint32_t c = p & 15u;
            const float4 dc = depth_consts_at(K, kofs);
            lds_fence();
            const float4 pc = *reinterpret_cast<const float4*>(tcur + c * 4u);
            const float tcaA = (pc.x * ra.dx + pc.y * ra.dy) + pc.z * ra.dz;
            const float tcaB = (pc.x * rb.dx + pc.y * rb.dy) + pc.z * rb.dz;
            const float d2A = pc.w - tcaA * tcaA;
            const float d2B = pc.w - tcaB * tcaB;
            const float xsA = R2c - d2A;
            const float xsB = R2c - d2B;
            const bool hbA = __builtin_fminf(__builtin_fminf(tcaA, xsA), ra.actv) >= 0.0f;
            const bool hbB = __builtin_fminf(__builtin_fminf(tcaB, xsB), rb.actv) >= 0.0f;
            const uint64_t hbmA = wave_ballot(hbA), hbmB = wave_ballot(hbB);
            if ((hbmA | hbmB) == 0ull) continue;
            const float4 dk = depth_consts_at(K, kofs + 16u);
            const float Tfar = dk.z;
            const float cull_r = dk.y;
            const uint64_t exmA = hbmA ? lod_expands(tcaA, d2A, xsA, hbA, hbmA, dc.x, dc.w, Tfar) : 0ull;
            const uint64_t exmB = hbmB ? lod_expands(tcaB, d2B, xsB, hbB, hbmB, dc.x, dc.w, Tfar) : 0ull;
            if ((exmA | exmB) == 0ull) continue;
            if ((int32_t)d + 1 > maxd) {
                maxd = (int32_t)d + 1;
                if ((int32_t)d + 1 > seed) cull_t = depth_consts_at(K, kofs + (1u << 5)).w;
            }
            uint64_t amxA = exmA, amxB = exmB;
            if (occl_cull) {
                // (occluded, for the two rays at once: both distances before the two ballots -- called per ray the
                // schedule of this loop changes)
                const float vA = __builtin_fminf(tcaA - ra.h.minT, tcaA - cull_t);
                const float vB = __builtin_fminf(tcaB - rb.h.minT, tcaB - cull_t);
                amxA = exmA & ~wave_ballot(vA - SF_OCCL_MARGIN * tcaA > cull_r);
                amxB = exmB & ~wave_ballot(vB - SF_OCCL_MARGIN * tcaB > cull_r);
                if ((amxA | amxB) == 0ull) continue;
            }
            const float avxA = sel_mask(-1.0f, __builtin_inff(), amxA);
            const float avxB = sel_mask(-1.0f, __builtin_inff(), amxB);
            self_test(ra, ancA, pc, tcaA, d2A, d + 1u, avxA, idxB + c, dc.y);
            self_test(rb, ancB, pc, tcaB, d2B, d + 1u, avxB, idxB + c, dc.y);
            if (wave_ballot(pc.w > dk.x) != 0ull) {   // an inline leaf: the child is finished
                ancA &= wave_ballot(ra.h.depth != (int32_t)d + 1);
                ancB &= wave_ballot(rb.h.depth != (int32_t)d + 1);
                continue;
            }
            // child c's children first (traverse_ray): a leaf-level node is not opened
            LeafLevel lf;
            const uint32_t Cn = expand(pc, tcur + SF_LDS_PLANE + 3u * c, SF_LDS_COLS, tcur + SF_LDS_LEVEL, kofs + (1u << 5),
                                       readlane_f(tcaA, axl), BoolC<false>(), avxA, avxB, lf);
            if (lf.on && (Cn == 0u || (int32_t)d + 2 <= (maxd > seed ? maxd : seed))) {   // (no child kept: nothing to count)
                if ((amxA & amxB) == 0ull)
                    one_ray_leaves(amxB, tcur + SF_LDS_LEVEL, Cn, sel_mask(avxA, __builtin_inff(), amxB),
                                   9u * (idxB + c) + 1u, d + 2u, lf);
                else
                    leaf_children_pair(ra, rb, ancA, ancB, status, front_first, occl_cull, tcur + SF_LDS_LEVEL, Cn, avxA,
                                       avxB, 9u * (idxB + c) + 1u, d + 2u, lf.dc, depth_consts_at(K, kofs + (1u << 5) + 16u), cull_t);
                ancA &= wave_ballot(ra.h.depth != (int32_t)d + 1);
                ancB &= wave_ballot(rb.h.depth != (int32_t)d + 1);
                continue;
            }
            stk_pc = writelane_s(C, d, stk_pc);
            stk_ix = writelane_s(idxB, d, stk_ix);
            {
                const uint32_t bit = 2u << d;
                uint32_t abA = ra.actbits & ~bit, abB = rb.actbits & ~bit;
                sel_in_place(abA, abA | bit, amxA);
                sel_in_place(abB, abB | bit, amxB);
                ra.actbits = abA;
                rb.actbits = abB;
            }
            idxB = 9u * (idxB + c) + 1u;
            d += 1u;
            ra.actv = avxA;
            rb.actv = avxB;
            tcur += SF_LDS_LEVEL;
            kofs += 1u << 5;
            C = Cn;
            R2c = lf.dc.x;
            // entered by no lane with both rays: its subtree on the one-ray loop, back here with the node finished
            if ((amxA & amxB) == 0ull) one_ray_subtree(amxB);
            continue;
        }
        ancA &= wave_ballot(ra.h.depth != (int32_t)d);
        ancB &= wave_ballot(rb.h.depth != (int32_t)d);
        if (d == 0u) break;
        d -= 1u;
        tcur -= SF_LDS_LEVEL;
        kofs -= 1u << 5;
        R2c = depth_consts_at(K, kofs).x;
        C = (uint32_t)__builtin_amdgcn_readlane(stk_pc, d);
        idxB = (uint32_t)__builtin_amdgcn_readlane(stk_ix, d);
        ra.actv = ((ra.actbits >> d) & 1u) ? __builtin_inff() : -1.0f;
        rb.actv = ((rb.actbits >> d) & 1u) ? __builtin_inff() : -1.0f;
    }
    ra.h.hit = ra.h.depth >= 0;
    rb.h.hit = rb.h.depth >= 0;
}

struct Tile {
    uint32_t x, y, orow;
    bool valid;
};

// Tile of a wave: owned tile row k (band sharding) -> frame tile row.
// LEAN (the whole frame's tiles as whole units, plain rows: one band, not compact; txm: the constant block's tx_magic,
// already loaded): frame tile row = owned tile row, every lane in the unit.
template <bool LEAN = false>
__device__ __forceinline__ Tile tile_of(const FrameArgs& a, uint32_t tile, uint32_t lane, uint32_t part = 0u, uint32_t txm_lean = 0u)
{
    // tile -> (k, tx) and k -> (band, row in band) by multiply-high with host magic numbers and one correction
    // (m = floor((2^32 - 1) / D) underestimates n / D by less than 1 for n < 2^31: q or q + 1), scalar
    auto divmod = [](uint32_t n, uint32_t D, uint32_t m, uint32_t& r) {
        uint32_t q = __umulhi(n, m);
        r = n - q * D;
        if (r >= D) {
            q += 1u;
            r -= D;
        }
        return q;
    };
    uint32_t tx, kr;
    if constexpr (LEAN) {
        const uint32_t k = divmod(tile, a.tiles_x, txm_lean, tx);
        uint32_t l = lane;
        __asm__ volatile("" : "+v"(l));
        Tile t;
        t.x = tx * SF_TILE + (l & 7u);
        t.y = k * SF_TILE + (l >> 3);
        t.valid = t.x < a.W && t.y < a.H;
        t.orow = t.y;
        return t;
    }
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) DeviceConsts* ConstK;
    const uint32_t txm = ((ConstK)(const void*)a.consts)->tx_magic;
#else
    const uint32_t txm = a.consts->tx_magic;
#endif
    const uint32_t k = divmod(tile, a.tiles_x, txm, tx);
    const uint32_t kb = divmod(k, a.tiles_per_band, a.tpb_magic, kr);
    const uint32_t band = a.band_index + kb * a.band_count;
    const uint32_t ty = band * a.tiles_per_band + kr;
    // (opaque copy: recompute the lane's column/row per tile rather than keep them live, or spilled,
    // across a persistent loop)
    uint32_t l = lane;
    __asm__ volatile("" : "+v"(l));
    Tile t;
    t.x = tx * SF_TILE + (l & 7u);
    t.y = ty * SF_TILE + (l >> 3);
    // part unit: only the lanes of pixel rows 0-3 / 4-7 (halves) or of one 4x4 block (quarters) take part
    const uint32_t q = part - SF_PART_QUARTER0;
    const bool in = part == 0u || (part < SF_PART_QUARTER0 ? (l >> 5) + SF_PART_HALF0 == part
                                                           : ((l >> 5) == (q >> 1) && ((l >> 2) & 1u) == (q & 1u)));
    t.valid = t.x < a.W && t.y < a.H && in;
    t.orow = a.compact ? (k * SF_TILE + (l >> 3)) : t.y;
    return t;
}

// G-buffer write (Sphereflake.cpp:186-196): (pos, 1), (nrm, 1); a miss writes (0,0,0,1).
// Packed slabs (multi-GPU bands, a.packed): one float4 (nx, ny, nz, minT) -- the position is dir * minT, which
// the receiving side recomputes bit for bit (sf_unpack_bands), so a band ships 16 B per pixel instead of 32.
// LEAN: the plain G-buffer only (no packed slab, no aux channels).
template <bool LEAN = false>
__device__ __forceinline__ void write_pixel(const FrameArgs& a, const Tile& t, float dx, float dy, float dz,
                                            const HitState& h, const uint32_t* __restrict__ lut)
{
    float px, py, pz, nx, ny, nz;
    const size_t o = (size_t)t.orow * a.W + t.x;
    if constexpr (LEAN) {   // (called by every lane, in wave-uniform code; the lanes of the frame store)
        const bool live = t.valid && h.hit;
        hit_point(dx, dy, dz, h, px, py, pz, nx, ny, nz);
        normalize3_fast(nx, ny, nz, lut, live);
        if (t.valid) {
            reinterpret_cast<float4*>(a.pos)[o] = make_float4(live ? px : 0.f, live ? py : 0.f, live ? pz : 0.f, 1.0f);
            reinterpret_cast<float4*>(a.nrm)[o] = make_float4(live ? nx : 0.f, live ? ny : 0.f, live ? nz : 0.f, 1.0f);
        }
        return;
    }
    shade(dx, dy, dz, h, lut, px, py, pz, nx, ny, nz);
    if (a.packed) {   // (uniform)
        if (a.packed >= SF_PACKED_INDEX) {
            // 4 B: the hit's heap index; the receiver rebuilds the rest. (The host selects this format only where
            // no hit can lie deeper than SF_INDEX_SLAB_DEPTH, whose heap indices are below 2^32; a deeper one would
            // be ambiguous and is written as SF_SLAB_BAD instead.)
            const int32_t lim = a.packed == SF_PACKED_INDEX ? SF_INDEX_SLAB_DEPTH : SF_DIAG_SLAB_DEPTH;   // (tests)
            const bool bad = h.hit && h.depth > lim;
            reinterpret_cast<uint32_t*>(a.pos)[o] = !h.hit ? SF_SLAB_MISS : bad ? SF_SLAB_BAD : h.index;
            // such a pixel counts as unresolved (stats[2]): sf_synchronize then reports SF_EDEPTH instead of the gather
            // silently carrying a NaN pixel (the host's depth proof and the device must never disagree)
            if (bad) atomicAdd(reinterpret_cast<uint32_t*>(a.stats) + 2, 1u);
            return;
        }
        reinterpret_cast<float4*>(a.pos)[o] = make_float4(nx, ny, nz, h.minT);
        return;
    }
    reinterpret_cast<float4*>(a.pos)[o] = make_float4(px, py, pz, 1.0f);
    reinterpret_cast<float4*>(a.nrm)[o] = make_float4(nx, ny, nz, 1.0f);
    if (a.emit_aux) {
        if (a.min_t) a.min_t[o] = h.minT;
        if (a.hit_index) a.hit_index[o] = h.hit ? h.index : 0xffffffffu;
    }
}

// write_pixel<true> for the two tiles of a pair unit (every lane, in wave-uniform code): both rays shaded first --
// the two table gathers in flight together behind one wait (normalize3_fast2) --, then the misses' zeros, then the
// four 16-byte stores: no store precedes the gathers' wait and nothing waits for a store.
__device__ __forceinline__ void write_pair(const FrameArgs& a, const Tile& tA, const Tile& tB, const PairRay& ra,
                                           const PairRay& rb, const uint32_t* __restrict__ lut)
{
    const bool liveA = tA.valid && ra.h.hit, liveB = tB.valid && rb.h.hit;
    float pax, pay, paz, nax, nay, naz, pbx, pby, pbz, nbx, nby, nbz;
    hit_point(ra.dx, ra.dy, ra.dz, ra.h, pax, pay, paz, nax, nay, naz);
    hit_point(rb.dx, rb.dy, rb.dz, rb.h, pbx, pby, pbz, nbx, nby, nbz);
    normalize3_fast2(nax, nay, naz, liveA, nbx, nby, nbz, liveB, lut);
    const size_t o = (size_t)tA.orow * a.W + tA.x;   // (tile B: the same row, SF_TILE pixels on)
    if (tA.valid) {
        reinterpret_cast<float4*>(a.pos)[o] = make_float4(liveA ? pax : 0.f, liveA ? pay : 0.f, liveA ? paz : 0.f, 1.0f);
        reinterpret_cast<float4*>(a.nrm)[o] = make_float4(liveA ? nax : 0.f, liveA ? nay : 0.f, liveA ? naz : 0.f, 1.0f);
    }
    if (tB.valid) {
        reinterpret_cast<float4*>(a.pos)[o + SF_TILE] = make_float4(liveB ? pbx : 0.f, liveB ? pby : 0.f, liveB ? pbz : 0.f, 1.0f);
        reinterpret_cast<float4*>(a.nrm)[o + SF_TILE] = make_float4(liveB ? nbx : 0.f, liveB ? nby : 0.f, liveB ? nbz : 0.f, 1.0f);
    }
}

struct TileStats {
    int32_t maxd;       // uniform: deepest expanded node (-1: none)
    int32_t seed;       // uniform: the depth seed its cull started from (DepthSeed::depth; -1: none)
    float closest;      // per lane: its minT (FLT_MAX for invalid lanes); reduced in publish_stats
    bool overflowed;    // uniform: the tile needs more LDS levels than provisioned
};

// One lane's global atomic add on behalf of the wave, result broadcast to every lane. EXEC is set to
// lane 0 inside the asm block, so the compiler's CFG has no lane-0-only region: such regions inside a
// loop let the structurizer run lanes in different iterations, which breaks wave-uniform code.
// A wave-uniform address, said to be so: it can go to an asm "s" operand (an SGPR pair) whatever the compiler's
// divergence analysis concludes about how it was formed (the -fgpu-rdc link's can differ from the compile's).
__device__ __forceinline__ uint32_t* uniform_ptr(uint32_t* p)
{
    const uint64_t pi = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)pi), hi = __builtin_amdgcn_readfirstlane((uint32_t)(pi >> 32));
    return reinterpret_cast<uint32_t*>((uint64_t)lo | ((uint64_t)hi << 32));
}

__device__ __forceinline__ uint32_t wave_fetch_add(uint32_t* p, uint32_t v)
{
    p = uniform_ptr(p);   // the address is uniform: say so, so that it can go to the asm in an SGPR pair
    uint32_t r, out;
    uint64_t saved;
    const uint32_t zero = 0u;
    __asm__ volatile(
        "s_mov_b64 %1, exec\n\t"
        "s_mov_b64 exec, 1\n\t"
        "global_atomic_add %0, %3, %4, %5 sc0\n\t"
        "s_waitcnt vmcnt(0)\n\t"
        "s_mov_b64 exec, %1\n\t"
        "s_nop 4\n\t"
        "v_readlane_b32 %2, %0, 0\n\t"
        : "=&v"(r), "=&s"(saved), "=s"(out)
        : "v"(zero), "v"(v), "s"(p)
        : "memory");
    return __builtin_amdgcn_readfirstlane(out);   // asm results count as divergent: say it is uniform
}

// One lane's global atomic increment on behalf of the wave, fire and forget (no return, no wait):
// EXEC is forced to lane 0 inside the asm. The op stays counted in vmcnt, which only makes the
// compiler's own later waits stricter.
__device__ __forceinline__ void wave_atomic_inc_nowait(uint32_t* p)
{
    p = uniform_ptr(p);
    uint64_t saved;
    const uint32_t zero = 0u, one = 1u;
    __asm__ volatile(
        "s_mov_b64 %0, exec\n\t"
        "s_mov_b64 exec, 1\n\t"
        "global_atomic_add %1, %2, %3\n\t"
        "s_mov_b64 exec, %0\n\t"
        : "=&s"(saved)
        : "v"(zero), "v"(one), "s"(p)
        : "memory");
}

// One lane's global atomic max on behalf of the wave, completed before it returns (EXEC forced to lane 0).
__device__ __forceinline__ void wave_atomic_max(uint32_t* p, uint32_t v)
{
    p = uniform_ptr(p);
    uint64_t saved;
    const uint32_t zero = 0u;
    __asm__ volatile(
        "s_mov_b64 %0, exec\n\t"
        "s_mov_b64 exec, 1\n\t"
        "global_atomic_umax %1, %2, %3\n\t"
        "s_waitcnt vmcnt(0)\n\t"
        "s_mov_b64 exec, %0\n\t"
        : "=&s"(saved)
        : "v"(zero), "v"(v), "s"(p)
        : "memory");
}

__device__ __forceinline__ uint32_t cost_bucket(uint32_t c)
{
    const uint32_t k = __float_as_uint((float)(c | 1u)) >> 22;   // exponent and 1 mantissa bit
    const uint32_t b = k - (135u << 1);                            // c < 2^8 -> 0
    return b < SF_ORDER_BUCKETS ? b : (k < (135u << 1) ? 0u : SF_ORDER_BUCKETS - 1u);
}

// The ray-cone axis lane of a unit: the centre pixel of what it traces -- (4, 4) for a whole tile,
// (4, 2) / (4, 6) for the halves, (2 + 4 (q & 1), 2 + 4 (q >> 1)) for quarter q.
__device__ __forceinline__ uint32_t part_axis_lane(uint32_t part)
{
    if (part == 0u) return 36u;
    if (part < SF_PART_QUARTER0) return part == SF_PART_HALF0 ? 20u : 52u;
    const uint32_t q = part - SF_PART_QUARTER0;
    return (2u + 4u * (q >> 1)) * 8u + 2u + 4u * (q & 1u);
}

struct NoPrefetch {
    __device__ void operator()(bool) const {}
};

// `pre` runs right after the traversal, before the tile's shading and stores: the persistent kernel takes
// its next queue ticket there, so the atomic's round trip overlaps the shading instead of following the
// G-buffer stores (whose completion a later wait would otherwise include: vmcnt counts in order).
// Heap index a is n or an ancestor of n (child i of node m is 9 m + 1 + i; indices of depth <= 10, whose heap
// indices fit the 32 bits HitState keeps).
__device__ __forceinline__ bool heap_ancestor(uint32_t a, uint32_t n)
{
    while (n > a) n = (n - 1u) / 9u;
    return n == a;
}

// Subtree part records (SF_FLAG_SUBTREE): part q of split slot s at part_rec + (4 s + q) x 192 u64, three 64-lane
// planes. Stored and loaded with agent scope (sc1: past the writer's and the reader's caches); each part's add to the
// tile's counter follows an agent-scope release fence and the merger (the last to add) acquires before reading them.
__device__ __forceinline__ uint64_t* part_record(const FrameArgs& a, uint32_t slot, uint32_t q)
{
    return a.part_rec + (size_t)(slot * 4u + q) * 192u;
}

// The launch's FrameArgs once more from the kernel argument segment (the only kernel argument: offset 0), through an
// address the compiler may not reason about: the fields read from the copy are scalar loads where they are used, and
// none of them is held in a register from an earlier copy.
__device__ __forceinline__ void kernarg_frame(FrameArgs& at, const FrameArgs& a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) FrameArgs* KernargArgs;
    KernargArgs pa = (KernargArgs)__builtin_amdgcn_kernarg_segment_ptr();
    __asm__ volatile("" : "+s"(pa));
    __builtin_memcpy(&at, (const FrameArgs*)pa, sizeof(FrameArgs));
    (void)a;
#else
    at = a;
#endif
}

// LEAN (sf_trace_queue1t, the product launch's single-tile loop; trace_queue_body): a whole tile of a plain frame -- no part
// units, no diagnostics (tile trace, diagnostic flags), no tile cost, no packed slab, no aux channels. `a` is then the
// kernel's own argument: the epilogue reads the G-buffer pointers, W and the overflow list from the kernel argument
// segment again instead of carrying them across the traversal.
template <bool FIXUP, class Prefetch = NoPrefetch, bool COMPACT = false, bool SPLIT = false, bool LEAN = false>
__device__ __forceinline__ TileStats trace_tile(const FrameArgs& a, float* __restrict__ L, const float4 bcol, uint32_t tile,
                                                uint32_t levels, uint32_t* overflow_list, uint32_t* overflow_count,
                                                uint32_t part = 0u, const Prefetch& pre = Prefetch(), uint32_t fl = ~0u,
                                                uint32_t slot = 0u, const DepthSeed seen = DepthSeed())
{
    // (fl: the launch's flags, with SF_FLAG_REDO_PASS | SF_FLAG_NO_FRONT_FIRST on a re-trace pass; ~0u: flags)
    // (slot: a subtree part unit's split slot -- its position in the unit order / 4)
    // (seen: the depth seed of the occlusion cull, see DepthSeed; the seed used is returned beside the tile's maxd)
    const uint32_t flags = fl == ~0u ? a.flags : fl;
    const DeviceConsts* __restrict__ K = a.consts;
    const uint32_t lane = threadIdx.x & 63u;
    if constexpr (LEAN) {
        static_assert(!FIXUP && !SPLIT && !COMPACT, "the lean tile is the plain persistent loop's");
        const FrameConsts fc = frame_consts(K);
        const Tile t = tile_of<true>(a, tile, lane, 0u, fc.tx_magic);
        float dx, dy, dz;
        ray_dir(a, (float)t.x, (float)t.y, dx, dy, dz, K->lut, &fc, &t.valid);
        const int32_t seed = seen.depth(flags);
        HitState h;
        int32_t maxd = -1;
        uint32_t status = 0u;
        traverse_ray<>(K, a.root, L, bcol, levels, dx, dy, dz, t.valid, h, maxd, status, flags, nullptr, 36u, nullptr, 0u, 0u,
                       seed);
        const bool overflowed = status != 0u;
        const bool retrace = __builtin_amdgcn_readfirstlane((int)(status == SF_STATUS_TIE && (flags & SF_FLAG_TIE_INLINE))) != 0;
        pre(retrace);
        FrameArgs ae;
        kernarg_frame(ae, a);
        if (overflowed && !retrace) {
            const uint32_t slot = wave_fetch_add(ae.counters + ae.parity, 1u);
            ae.overflow_list[slot] = tile;   // uniform value and address
        }
        write_pixel<true>(ae, t, dx, dy, dz, h, K->lut);
        TileStats st;
        st.maxd = maxd;
        st.seed = seed;
        st.closest = t.valid ? h.minT : FLT_MAX;
        st.overflowed = overflowed;
        return st;
    }
    if (flags & SF_FLAG_DIAG_HALF) part = (flags & SF_FLAG_DIAG_HALF_SEL) ? 2u : 1u;
    // a subtree part unit: all 64 pixels, the depth-split_depth subtrees of heap index q mod 4 (SF_FLAG_SUBTREE)
    // (only the SPLIT kernel, sf_trace_queue1s, carries the split logic)
    const bool sub = SPLIT && !FIXUP && (flags & SF_FLAG_SUBTREE) != 0u && part >= SF_PART_QUARTER0;
    const Tile t = tile_of(a, tile, lane, sub ? 0u : part);
    const uint64_t t_start = a.tile_trace ? __builtin_amdgcn_s_memrealtime() : 0ull;
    const uint64_t c_start = (!FIXUP && a.tile_cost) ? __builtin_amdgcn_s_memtime() : 0ull;
    float dx, dy, dz;
    ray_dir(a, (float)t.x, (float)t.y, dx, dy, dz, K->lut);
    const int32_t seed = seen.depth(flags);

    HitState h;
    int32_t maxd = -1;
    uint32_t status = 0u;
    uint64_t tile_counts = 0;
    // The main kernels enter children front-first (with the occlusion cull); an exact non-ancestor tie under
    // that order flags the tile like an overflow, and the fixup re-traces it in index order -- the reference's
    // tie rule (see accept_self). The fixup kernel always traces in index order.
    if constexpr (SPLIT)   // one traversal: the split depth never matches on whole units
        traverse_ray<COMPACT, true>(K, a.root, L, bcol, levels, dx, dy, dz, t.valid, h, maxd, status,
                                    FIXUP ? (flags | SF_FLAG_NO_FRONT_FIRST) : flags,
                                    FIXUP ? nullptr : a.phase_sums, part_axis_lane(sub ? 0u : part), &tile_counts,
                                    sub ? part - SF_PART_QUARTER0 : 0u, sub ? a.split_depth : 0xffffffffu, seed);
    else
        traverse_ray<COMPACT, false, false, !FIXUP && !COMPACT>(K, a.root, L, bcol, levels, dx, dy, dz, t.valid, h, maxd, status,
                              FIXUP ? (flags | SF_FLAG_NO_FRONT_FIRST) : flags,
                              FIXUP ? nullptr : a.phase_sums, part_axis_lane(part), &tile_counts, 0u, 0u, seed);
    if (!FIXUP && (flags & (SF_FLAG_DIAG_FORCE_RETRACE | SF_FLAG_REDO_PASS)) == SF_FLAG_DIAG_FORCE_RETRACE)
        status |= SF_STATUS_TIE;
    bool merger = true;   // this wave writes the tile (a subtree part: only the part that merges)
    if (sub) {
        // ---- subtree part: publish this part's per-pixel result; the part that finishes last merges the four
        // and goes on as a whole tile would (re-trace decision, scheduling cost, G-buffer write)
        const bool rec_cost = a.tile_cost != nullptr && !(flags & SF_FLAG_DIAG_HALF);
        if (rec_cost) {   // the slowest part, in whole-tile terms (x 2, as for quarters)
            const uint64_t cyc = __builtin_amdgcn_s_memtime() - c_start;
            wave_atomic_max(a.part_cost + tile, cyc > 0x7fffffffull ? 0xffffffffu : 2u * (uint32_t)cyc);
        }
        const uint32_t q = part - SF_PART_QUARTER0;
        uint64_t* const R = part_record(a, slot, q);
        __hip_atomic_store(R + lane, ((uint64_t)__float_as_uint(h.cx) << 32) | __float_as_uint(h.minT),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(R + 64u + lane, ((uint64_t)__float_as_uint(h.cz) << 32) | __float_as_uint(h.cy),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(R + 128u + lane, ((uint64_t)(uint32_t)h.depth << 32) | h.index,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // release: the records are visible at agent scope before the counter add that publishes them (the
        // memory model, not a hand-placed waitcnt, orders the stores before the add; the merger acquires below)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        // counter: parts done (low byte), parts that flagged an overflow (byte 1), a tie (byte 2)
        const uint32_t add = 1u | ((status & SF_STATUS_OVERFLOW) ? 0x100u : 0u) | ((status & SF_STATUS_TIE) ? 0x10000u : 0u);
        const uint32_t st0 = status;
        const uint32_t old = wave_fetch_add(a.part_done + tile, add);
        merger = (old & 0xffu) == 3u;   // the last part; the others are done with this tile (no write, no flag)
        status = 0u;
      if (merger) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // the other parts' records, published before their adds
        a.part_done[tile] = 0u;   // for the next render (uniform value and address)
        // merge: per pixel the nearest sphere over the parts. An exact tie between two parts' spheres is the
        // reference's ancestor rule where one is the other's ancestor (a node's sphere is tested before its
        // subtree, and a tie with an ancestor is accepted, self_test) -- the parts share every node above
        // split_depth, so each part's own result already holds it against the shared spheres -- and otherwise a
        // tie the index-order re-trace resolves, as within a traversal.
        bool tie = false;
#pragma unroll 1
        for (uint32_t p = 0u; p < 4u; ++p) {   // (one part at a time: few registers live)
            if (p == q) continue;
            const uint64_t* const Rp = part_record(a, slot, p);
            const uint64_t r0 = __hip_atomic_load(Rp + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint64_t r1 = __hip_atomic_load(Rp + 64u + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint64_t r2 = __hip_atomic_load(Rp + 128u + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const float m = __uint_as_float((uint32_t)r0);
            const uint32_t idx = (uint32_t)r2;
            const int32_t dep = (int32_t)(uint32_t)(r2 >> 32);
            bool take = m < h.minT;
            if (m == h.minT && idx != h.index) {
                const bool both = h.depth >= 0 && dep >= 0 && h.depth <= 10 && dep <= 10;
                if (both && heap_ancestor(h.index, idx)) take = true;          // the deeper sphere wins the tie
                else if (!(both && heap_ancestor(idx, h.index))) tie = true;   // unrelated spheres: re-trace
            }
            if (take) {
                h.minT = m;
                h.cx = __uint_as_float((uint32_t)(r0 >> 32));
                h.cy = __uint_as_float((uint32_t)r1);
                h.cz = __uint_as_float((uint32_t)(r1 >> 32));
                h.index = idx;
                h.depth = dep;
            }
        }
        h.hit = h.depth >= 0;
        status = st0;
        if ((old & 0xff00u) != 0u) status |= SF_STATUS_OVERFLOW;
        if ((old & 0xff0000u) != 0u || wave_ballot(tie) != 0ull) status |= SF_STATUS_TIE;
        if (rec_cost) {
            const uint32_t cost = __builtin_amdgcn_readfirstlane(
                (int)__hip_atomic_load(a.part_cost + tile, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            a.part_cost[tile] = 0u;
            a.tile_cost[tile] = cost;
            if (a.chunk_cnt) {
                const uint32_t cs = __builtin_amdgcn_readfirstlane((tile >> 6) * SF_ORDER_BUCKETS + cost_bucket(cost));
                wave_atomic_inc_nowait(a.chunk_cnt + cs);
            }
        }
      }
    }
    const bool overflowed = status != 0u;
    // a tie under the front-first order with the levels proven (SF_FLAG_TIE_INLINE): this wave re-traces the unit
    // in index order right after (trace_queue_body, told by `pre`); anything else flagged goes to the overflow list
    const bool retrace = !FIXUP && __builtin_amdgcn_readfirstlane(
                                       (int)(status == SF_STATUS_TIE && (flags & SF_FLAG_TIE_INLINE))) != 0;
    pre(retrace);
    if (!FIXUP && a.tile_trace) {
        // diagnostics only: never read by the kernel, never feeds an output value. Every lane stores
        // the same (uniform) words: no lane-0-only region.
        const uint64_t t_end = __builtin_amdgcn_s_memrealtime();
        uint32_t hw;
        __asm__ volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        uint32_t xcc;
        __asm__ volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        a.tile_trace[3u * tile + 0u] = t_start;
        a.tile_trace[3u * tile + 1u] = t_end;
#ifdef SF_COUNTS
        a.tile_trace[3u * tile + 2u] = tile_counts;   // COUNTS=1 builds: the tile's event counts instead
#else
        a.tile_trace[3u * tile + 2u] = ((uint64_t)xcc << 32) | hw;
#endif
    }

    if (!FIXUP && !sub && a.tile_cost && !(flags & (SF_FLAG_DIAG_HALF | SF_FLAG_REDO_PASS))) {
        // scheduling hint for the next render (sf_order_scan / sf_order_scatter); uniform values.
        const uint64_t cyc = __builtin_amdgcn_s_memtime() - c_start;
        uint32_t cost = cyc > 0xffffffffull ? 0xffffffffu : (uint32_t)cyc;
        bool last = true;
        if (part != 0u) {
            // a split tile: the slowest of its parts, in whole-tile terms (x 3/2 for halves, x 2 for
            // quarters), recorded by the part that finishes last
            const uint32_t scaled = part < SF_PART_QUARTER0 ? cost + (cost >> 1) : (cost > 0x7fffffffu ? 0xffffffffu : 2u * cost);
            const uint32_t nparts = part < SF_PART_QUARTER0 ? 2u : 4u;
            wave_atomic_max(a.part_cost + tile, scaled);
            last = wave_fetch_add(a.part_done + tile, 1u) == nparts - 1u;
            if (last) {
                cost = __builtin_amdgcn_readfirstlane(
                    (int)__hip_atomic_load(a.part_cost + tile, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                a.part_cost[tile] = 0u;   // for the next render (uniform values and addresses)
                a.part_done[tile] = 0u;
            }
        }
        if (last) {
            a.tile_cost[tile] = cost;
            if (a.chunk_cnt) {   // (renders that rebuild the order: the histogram for sf_order_scan)
                const uint32_t slot = __builtin_amdgcn_readfirstlane((tile >> 6) * SF_ORDER_BUCKETS + cost_bucket(cost));
                wave_atomic_inc_nowait(a.chunk_cnt + slot);
            }
        }
    }
    if (!FIXUP && overflowed && !retrace) {
        // a deeper (or index-order) re-trace (sf_fixup_wave) rewrites this whole tile
        const uint32_t slot = wave_fetch_add(overflow_count, 1u);
        overflow_list[slot] = tile;   // uniform value and address
    }
    if (t.valid && merger) write_pixel(a, t, dx, dy, dz, h, K->lut);

    // stats: max depth reached, closest sphere distance (Sphereflake.h:157-160, Sphereflake.cpp:197-200)
    TileStats st;
    st.maxd = maxd;
    st.seed = seed;
    st.closest = t.valid ? h.minT : FLT_MAX;
    st.overflowed = overflowed;
    return st;
}

// A pair unit of the lean loop (trace_queue_body<PAIR>): what trace_tile<LEAN> does, for the tiles (2 px, ty) and
// (2 px + 1, ty) of pair `unit` = ty x pairs_x + px. With an odd tiles_x the last pair of a row has no B tile: its B
// lanes lie beyond W and are invalid. The pair loop serves SF_FLAG_DIAG_FORCE_RETRACE itself (one scalar test per
// unit). COST: the unit's cycles into tile_cost[unit] and the chunk histogram, as the general loop records a tile's.
template <bool COST, class Prefetch>
__device__ __forceinline__ TileStats trace_pair(const FrameArgs& a, float* __restrict__ L, const float4 bcol, uint32_t unit,
                                                uint32_t levels, const Prefetch& pre, uint32_t flags, const DepthSeed seen)
{
    const DeviceConsts* __restrict__ K = a.consts;
    const FrameConsts fc = frame_consts(K);
    // (the counter's low word only: one SGPR across the traversal; a unit's cycles are far below 2^32)
    const uint32_t c_start = COST ? (uint32_t)__builtin_amdgcn_s_memtime() : 0u;
    const uint32_t pairs_x = (a.tiles_x + 1u) >> 1;
    uint32_t ty = __umulhi(unit, a.px_magic);   // (tile_of's divmod)
    uint32_t px = unit - ty * pairs_x;
    if (px >= pairs_x) {
        ty += 1u;
        px -= pairs_x;
    }
    uint32_t l = threadIdx.x & 63u;
    __asm__ volatile("" : "+v"(l));
    Tile tA, tB;
    tA.x = px * (2u * SF_TILE) + (l & 7u);
    tA.y = tB.y = ty * SF_TILE + (l >> 3);
    tB.x = tA.x + SF_TILE;
    tA.orow = tB.orow = tA.y;
    tA.valid = tA.x < a.W && tA.y < a.H;
    tB.valid = tB.x < a.W && tA.y < a.H;
    PairRay ra, rb;
    ray_dir_pair(a, fc, (float)tA.x, (float)tB.x, (float)tA.y, tA.valid, tB.valid, ra.dx, ra.dy, ra.dz, rb.dx, rb.dy, rb.dz,
                 K->lut);
    const int32_t seed = seen.depth(flags);
    int32_t maxd = -1;
    uint32_t status = 0u;
    traverse_pair(K, a.root, L, bcol, levels, ra, rb, tA.valid, tB.valid, maxd, status, flags, seed);
    if ((flags & (SF_FLAG_DIAG_FORCE_RETRACE | SF_FLAG_REDO_PASS)) == SF_FLAG_DIAG_FORCE_RETRACE) status |= SF_STATUS_TIE;
    const bool overflowed = status != 0u;
    const bool retrace = __builtin_amdgcn_readfirstlane((int)(status == SF_STATUS_TIE && (flags & SF_FLAG_TIE_INLINE))) != 0;
    pre(retrace);
    FrameArgs ae;
    kernarg_frame(ae, a);
    if constexpr (COST) {
        if (ae.tile_cost && !(flags & SF_FLAG_REDO_PASS)) {   // (uniform values and addresses)
            const uint32_t cost = (uint32_t)__builtin_amdgcn_s_memtime() - c_start;
            ae.tile_cost[unit] = cost;
            if (ae.chunk_cnt) {
                const uint32_t cs = __builtin_amdgcn_readfirstlane((unit >> 6) * SF_ORDER_BUCKETS + cost_bucket(cost));
                wave_atomic_inc_nowait(ae.chunk_cnt + cs);
            }
        }
    }
    if (overflowed && !retrace) {
        // both tiles to the overflow list (sf_fixup_wave re-traces tiles), their slots reserved by one add
        const uint32_t tile = ty * ae.tiles_x + 2u * px;
        const uint32_t n = 2u * px + 1u < ae.tiles_x ? 2u : 1u;
        const uint32_t slot = wave_fetch_add(ae.counters + ae.parity, n);
        ae.overflow_list[slot] = tile;   // uniform values and addresses
        if (n == 2u) ae.overflow_list[slot + 1u] = tile + 1u;
    }
    write_pair(ae, tA, tB, ra, rb, K->lut);
    TileStats st;
    st.maxd = maxd;
    st.seed = seed;
    st.closest = fminf(tA.valid ? ra.h.minT : FLT_MAX, tB.valid ? rb.h.minT : FLT_MAX);
    st.overflowed = overflowed;
    return st;
}

// Publish one wave's stats (outside any loop: lane-0 regions are harmless here). `closest` per lane.
// Thousands of waves end together and atomics on one address serialise (~10 ns each), so a wave
// first reads the current value and issues the atomic only if it would change it. The read may be
// stale, never wrong: the values only move one way within a render.
__device__ __forceinline__ void publish_stats(const FrameArgs& a, int32_t maxd, float closest, uint32_t unresolved)
{
    closest = wave_min(closest);
    if ((threadIdx.x & 63u) == 0u) {
        const int32_t key = sf_float_key(closest);
        const int32_t cur_d = __hip_atomic_load(&a.stats[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int32_t cur_k = __hip_atomic_load(&a.stats[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (maxd > cur_d) atomicMax(&a.stats[0], maxd);
        if (key < cur_k) atomicMin(&a.stats[1], key);
        if (unresolved) atomicAdd(&a.stats[2], (int32_t)unresolved);
    }
}

// publish_stats for a call inside a wave-uniform loop (the multi-frame trace publishes a frame's stats when the
// wave leaves the frame): no lane-0 region -- each atomic runs with EXEC forced to lane 0 inside its asm block, as
// wave_atomic_max does (signed max / min: the words start at -1 and at the key of FLT_MAX).
__device__ __forceinline__ void wave_atomic_smax(int32_t* p, int32_t v)
{
    p = reinterpret_cast<int32_t*>(uniform_ptr(reinterpret_cast<uint32_t*>(p)));
    uint64_t saved;
    const uint32_t zero = 0u;
    __asm__ volatile(
        "s_mov_b64 %0, exec\n\t"
        "s_mov_b64 exec, 1\n\t"
        "global_atomic_smax %1, %2, %3\n\t"
        "s_mov_b64 exec, %0\n\t"
        : "=&s"(saved)
        : "v"(zero), "v"(v), "s"(p)
        : "memory");
}
__device__ __forceinline__ void wave_atomic_smin(int32_t* p, int32_t v)
{
    p = reinterpret_cast<int32_t*>(uniform_ptr(reinterpret_cast<uint32_t*>(p)));
    uint64_t saved;
    const uint32_t zero = 0u;
    __asm__ volatile(
        "s_mov_b64 %0, exec\n\t"
        "s_mov_b64 exec, 1\n\t"
        "global_atomic_smin %1, %2, %3\n\t"
        "s_mov_b64 exec, %0\n\t"
        : "=&s"(saved)
        : "v"(zero), "v"(v), "s"(p)
        : "memory");
}
// Read before the atomic, as publish_stats does: thousands of waves leave a frame together, and atomics on one
// address serialise (~10 ns each) -- issued unconditionally they made a 4-frame launch take twice as long.
__device__ __forceinline__ void publish_stats_in_loop(const FrameArgs& a, int32_t maxd, float closest)
{
    const int32_t key = __builtin_amdgcn_readfirstlane(sf_float_key(wave_min(closest)));
    maxd = __builtin_amdgcn_readfirstlane(maxd);
    const int32_t cur_d = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&a.stats[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    const int32_t cur_k = __builtin_amdgcn_readfirstlane(__hip_atomic_load(&a.stats[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    if (maxd > cur_d) wave_atomic_smax(a.stats + 0, maxd);
    if (key < cur_k) wave_atomic_smin(a.stats + 1, key);
}

// A unit went deeper (maxd) than its seed: raise the word at once, so that the other waves' seeds follow within the
// frame (the first frame after a reset; afterwards the word already holds the frame's depth and no unit gets here).
// Read before the atomic, as publish_stats_in_loop does. For wave-uniform loops (no lane-0 region).
__device__ __forceinline__ void publish_depth_early(const FrameArgs& a, int32_t maxd)
{
    maxd = __builtin_amdgcn_readfirstlane(maxd);
    if (maxd > __builtin_amdgcn_readfirstlane(stats_word(a))) wave_atomic_smax(a.stats + 0, maxd);
}

}  // namespace

// One wave (one 8x8 tile) per workgroup: LDS is the occupancy limit, so the finest granularity packs best.
// WAVES independent waves per workgroup (adjacent tiles, similar cost); the host picks the variant.
template <int WAVES>
__device__ __forceinline__ void trace_wave_body(const FrameArgs& a, uint32_t* overflow_list, uint32_t* overflow_count)
{
    extern __shared__ float lds[];
    const uint32_t wv = threadIdx.x >> 6;
    const uint32_t tile = blockIdx.x * WAVES + wv;
    if (tile >= a.tiles_x * a.tile_rows) return;
    float* const L = lds + wv * SF_LDS_WAVE_FLOATS(a.max_depth);
    stage_root(L, a.root);
    const TileStats st = trace_tile<false>(a, L, build_column(a.consts), tile, a.max_depth, overflow_list, overflow_count,
                                           0u, NoPrefetch(), ~0u, 0u, DepthSeed{ -1, stats_word(a) });
    publish_stats(a, st.maxd, st.closest, 0u);
}

extern "C" __global__ __launch_bounds__(64) void sf_trace_wave1(FrameArgs a, uint32_t* ol, uint32_t* oc)
{
    trace_wave_body<1>(a, ol, oc);
}
extern "C" __global__ __launch_bounds__(128) void sf_trace_wave2(FrameArgs a, uint32_t* ol, uint32_t* oc)
{
    trace_wave_body<2>(a, ol, oc);
}
extern "C" __global__ __launch_bounds__(256) void sf_trace_wave4(FrameArgs a, uint32_t* ol, uint32_t* oc)
{
    trace_wave_body<4>(a, ol, oc);
}

// Persistent variant: a grid of resident workgroups; each wave pulls 8x8 tiles from a frame-wide
// atomic queue until it runs dry. Dynamic balancing: tile costs vary ~100x (sky vs. deep flake),
// and the in-order workgroup dispatcher otherwise idles CUs behind long tiles. counters: [0,1]
// overflow counts, [2,3] tile queues, alternating per render (this render zeroes the next one's).
// LEAN: the product launch's instantiation (sf_trace_queue1t; the host launches it exactly when the launch asks for
// none of what it leaves out, sf_render_to): whole-tile units of one plain frame -- row-major or the ordered units
// with their priority levels, the depth seed, the inline tie re-trace, the overflow list, the stats and the clock
// probe; no part units (halves, quarters, subtree parts), no tile trace or diagnostic flags, no tile costs, no packed
// slab, no aux channels, no band mapping. Every launch word is read from the kernel argument segment where it is used.
// PAIR (with LEAN; 1: sf_trace_queue1, 2: sf_trace_queue1c, which also records unit costs for the render that rebuilds
// the order): the lean loop over pair units (trace_pair) -- the unit word's tile field holds the pair index, the
// row-major units are the ceil(tiles_x / 2) x tile_rows pairs.
template <int WAVES, bool COMPACT = false, bool SPLIT = false, bool LEAN = false, int PAIR = 0>
__device__ __forceinline__ void trace_queue_body(const FrameArgs& a)
{
    static_assert(PAIR == 0 || LEAN, "pair units are the lean loop's");
    extern __shared__ float lds[];
    const uint64_t w_start = __builtin_amdgcn_s_memrealtime();
    const uint32_t wv = threadIdx.x >> 6;
    // measurement: the live shader clock, delta s_memtime / delta s_memrealtime x 100 MHz over this wave's
    // life (the start pair stored now, so nothing stays live across the tile loop; uniform values and
    // addresses; read by sf_kernel_clocks, never by a kernel)
    if (a.clock_probe && wv == 0u && blockIdx.x < SF_CLOCK_WAVES) {
        uint64_t* cp = a.clock_probe + 4u * blockIdx.x;
        cp[0] = __builtin_amdgcn_s_memtime();
        cp[1] = w_start;
    }
    // a.queues (<= SF_QUEUES) tile queues per render, one cache line each: queue k hands out the units
    // after the static first ones with index = k mod a.queues
    // A wave starts on its own XCD's queue and moves on to the next one when it runs dry. One queue
    // for the whole chip serialises ~100 atomics/us on one address (measured: ~11 us per fetch).
    if (blockIdx.x == 0 && threadIdx.x < SF_QUEUES)
        a.counters[SF_QUEUE_WORD(a.parity ^ 1u, threadIdx.x)] = 0u;   // the next render's queues
    if (blockIdx.x == 0 && threadIdx.x == 0) a.counters[a.parity ^ 1u] = 0u;   // and overflow count
    float* const L = lds + wv * SF_LDS_WAVE_FLOATS(a.max_depth);
    const uint32_t ntiles = (PAIR ? (a.tiles_x + 1u) >> 1 : a.tiles_x) * a.tile_rows;
    // work units: tiles in row-major order, or the previous render's heavy-first order in which the
    // heaviest tiles come as two half units (order_meta[0] entries)
    uint32_t nunits = ntiles;
    if (a.tile_order) {
#if defined(__HIP_DEVICE_COMPILE__)
        typedef const __attribute__((address_space(4))) uint32_t* ConstU32;
        nunits = ((ConstU32)(const void*)a.order_meta)[0];
#else
        nunits = a.order_meta[0];
#endif
    } else if (!LEAN && (a.flags & SF_FLAG_HALVES)) {
        nunits = 2u * ntiles;
    }
    stage_root(L, a.root);
    const float4 bcol = build_column(a.consts);
    // One queue per XCD (a.queues of them); a wave drains its own group's queue and then exits. Stealing
    // from the other queues once the own one ran dry cost every wave up to 7 more atomics on queue words
    // contended chip-wide at the end of the frame: the last wave exited ~60 us after the last tile
    // ended. Every queue still drains: its group's waves only leave when it is empty.
    const uint32_t nq = a.queues, nx = a.xcds;
    // queue k = block group (k % nx) + nx x sub-queue; a group's waves spread over its nq / nx sub-queues by
    // their position in the grid. The group is blockIdx mod nx, not the XCD id: blocks are observed to be
    // dealt round-robin over the XCDs, so a group is one XCD's blocks (its queue word stays in that XCD's
    // traffic), but every group has waves whatever the placement (a CU-masked stream, a partitioned chip):
    // the host keeps nx <= the grid's blocks, so every queue drains.
    uint32_t k = blockIdx.x & (nx - 1u);
    if (nq > nx) {   // (powers of two: shifts, no division)
        const uint32_t lx = __builtin_ctz(nx);
        k += nx * (((blockIdx.x >> lx) * WAVES + wv) & ((nq >> lx) - 1u));
        k = __builtin_amdgcn_readfirstlane(k);
    }
    int32_t maxd = -1;
    float closest = FLT_MAX;   // per lane
    // The first unit of every wave is static: wave w (in dispatch order) takes unit w, so the head of the
    // heavy-first order starts as the waves arrive instead of behind ~900 simultaneous atomics per queue;
    // the queues hand out units nwaves, nwaves + 1, ...
    const uint32_t nwaves = gridDim.x * WAVES;
    uint32_t first = __builtin_amdgcn_readfirstlane(blockIdx.x * WAVES + wv);   // (wv is wave-uniform)
    for (;;) {
        // Re-read the launch arguments every tile (scalar loads from the kernarg segment) instead of
        // keeping ~40 of them live in SGPRs across the whole persistent loop.
        // (FrameArgs is the only kernel argument: offset 0 of the kernarg segment)
        FrameArgs at;
#if defined(__HIP_DEVICE_COMPILE__)
        {
            typedef const __attribute__((address_space(4))) FrameArgs* KernargArgs;
            KernargArgs pa = (KernargArgs)__builtin_amdgcn_kernarg_segment_ptr();
            __asm__ volatile("" : "+s"(pa));
            __builtin_memcpy(&at, (const FrameArgs*)pa, sizeof(FrameArgs));
        }
#else
        at = a;
#endif
        // position in the render's unit order: the static first unit, then the ticket the previous tile
        // took after its traversal (past the end: the XCD's queue is empty)
        // (or, bit 31 set, a unit to re-trace in index order: part << SF_UNIT_PRIO_SHIFT | tile -- a tie under the
        // front-first order with SF_FLAG_TIE_INLINE; the ticket is taken after that pass)
        const uint32_t g = first;
        const bool again = (g >> 31) != 0u;
        if (!again && g >= nunits) break;
        // the cull's depth seed (DepthSeed): the word's load is issued per unit, here, ahead of the unit's ray
        // generation, and waited for after it (trace_tile)
        const DepthSeed seen{ maxd, stats_word(at) };
        uint32_t t = g, part = 0u;
        if (again) {
            t = g & SF_UNIT_TILE_MASK;
            if constexpr (!LEAN) part = (g >> SF_UNIT_PRIO_SHIFT) & 7u;
        } else if (at.tile_order) {      // heaviest tiles of the previous render first (scalar load)
#if defined(__HIP_DEVICE_COMPILE__)
            typedef const __attribute__((address_space(4))) uint32_t* ConstU32;
            const uint32_t u = ((ConstU32)(const void*)at.tile_order)[g];
#else
            const uint32_t u = at.tile_order[g];
#endif
            t = u & SF_UNIT_TILE_MASK;
            if constexpr (!LEAN) part = u >> SF_UNIT_PART_SHIFT;
            // critical-path tiles (top cost buckets of the last render, order_meta[3]) at raised priority:
            // the SIMD's issue arbitration serves them first, the cheap tiles absorb the wait. Graded: the
            // raised buckets' lowest 3 (1.5 octaves) at 2, the ones above at 3, so the very heaviest tiles
            // also win the arbitration against the merely heavy (8 buckets: 0.1607 -> 0.1578 ms/frame against
            // all raised buckets at one level). The level comes with the unit (sf_order_scatter).
            const uint32_t pr = (u >> SF_UNIT_PRIO_SHIFT) & 3u;
            if (pr == 2u && (LEAN || !(at.flags & SF_FLAG_PRIO_FLAT))) __builtin_amdgcn_s_setprio(3);
            else if (pr != 0u) __builtin_amdgcn_s_setprio(2);
            else __builtin_amdgcn_s_setprio(0);
        } else if (!LEAN && (at.flags & SF_FLAG_HALVES)) {   // (row-major halves: unit g = half g & 1 of tile g / 2)
            t = g >> 1;
            part = SF_PART_HALF0 + (g & 1u);
        }
        if constexpr (LEAN) {
            // the next unit's ticket, taken when this tile's traversal ends (the queue words' address from the kernel
            // argument segment again, not carried across the traversal)
            auto ticket = [&](bool retrace) {
                if (retrace) {
                    first = 0x80000000u | t;
                } else {
                    FrameArgs aq;
                    kernarg_frame(aq, a);
                    first = nwaves + wave_fetch_add(aq.counters + SF_QUEUE_WORD(aq.parity, k), 1u) * nq + k;   // uniform
                }
            };
            const uint32_t ufl = again ? (at.flags | SF_FLAG_NO_FRONT_FIRST | SF_FLAG_REDO_PASS) : at.flags;
            TileStats st;
            if constexpr (PAIR != 0)
                st = trace_pair<PAIR == 2>(at, L, bcol, t, at.max_depth, ticket, ufl, seen);
            else
                st = trace_tile<false, decltype(ticket), false, false, true>(
                    at, L, bcol, t, at.max_depth, nullptr, nullptr, 0u, ticket, ufl, 0u, seen);
            maxd = st.maxd > maxd ? st.maxd : maxd;
            if (st.seed >= 0 && st.maxd > st.seed) {   // (rare: see the general loop below)
                FrameArgs ap;
                kernarg_frame(ap, a);
                publish_depth_early(ap, st.maxd);
            }
            closest = fminf(closest, st.closest);
            continue;
        }
        const uint64_t u_start = (at.flags & SF_FLAG_DIAG_UNITS) ? __builtin_amdgcn_s_memrealtime() : 0ull;
        // the next unit's ticket, taken when this tile's traversal ends (see trace_tile)
        // (an agent-coherent load of the queue word before the atomic, to skip dry queues, made the frame
        // 1.7x slower: it contends with the atomics on the line)
        // (a subtree part's re-trace is its whole tile's: the part that merged the tile takes it, as part 0)
        auto ticket = [&](bool retrace) {
            const uint32_t rp = ((at.flags & SF_FLAG_SUBTREE) && part >= SF_PART_QUARTER0) ? 0u : part;
            first = retrace ? (0x80000000u | (rp << SF_UNIT_PRIO_SHIFT) | t)
                            : nwaves + wave_fetch_add(at.counters + SF_QUEUE_WORD(at.parity, k), 1u) * nq + k;   // uniform
        };
        const TileStats st = trace_tile<false, decltype(ticket), COMPACT, SPLIT>(at, L, bcol, t, at.max_depth, at.overflow_list,
                                                                               at.counters + at.parity, part,
                                               ticket, again ? (at.flags | SF_FLAG_NO_FRONT_FIRST | SF_FLAG_REDO_PASS)
                                                             : at.flags, g >> 2, seen);
        if ((at.flags & SF_FLAG_DIAG_UNITS) && at.tile_trace && (g >> 31) == 0u) {   // diagnostics only (uniform words)
            // (slot g: the unit's position in the order. A re-trace pass -- its ticket word carries bit 31 -- records
            // nothing: its word is no position, and the slot of the unit it repeats already holds that unit's record)
            uint64_t* ut = at.tile_trace + 3u * (at.tiles_x * at.tile_rows) + SF_DIAG_SLOTS + 3u * g;
            ut[0] = u_start;
            ut[1] = __builtin_amdgcn_s_memrealtime();
            ut[2] = t | (part << SF_UNIT_PART_SHIFT);
        }
        maxd = st.maxd > maxd ? st.maxd : maxd;
        if (st.seed >= 0 && st.maxd > st.seed) {
            // the unit went deeper than the word it read and this wave's earlier units: raise the word at once
            // (rare -- at most once per depth and wave: the arguments once more from the kernarg segment, so that the
            // stats pointer is not held in registers across the traversal)
            FrameArgs ap;
#if defined(__HIP_DEVICE_COMPILE__)
            {
                typedef const __attribute__((address_space(4))) FrameArgs* KernargArgs;
                KernargArgs pa = (KernargArgs)__builtin_amdgcn_kernarg_segment_ptr();
                __asm__ volatile("" : "+s"(pa));
                __builtin_memcpy(&ap, (const FrameArgs*)pa, sizeof(FrameArgs));
            }
#else
            ap = a;
#endif
            publish_depth_early(ap, st.maxd);
        }
        closest = fminf(closest, st.closest);
    }
    // the launch arguments again from the kernarg segment, so that none of them is held in a register
    // across the tile loop for the code below
    FrameArgs e;
#if defined(__HIP_DEVICE_COMPILE__)
    {
        typedef const __attribute__((address_space(4))) FrameArgs* KernargArgs;
        KernargArgs pa = (KernargArgs)__builtin_amdgcn_kernarg_segment_ptr();
        __asm__ volatile("" : "+s"(pa));
        __builtin_memcpy(&e, (const FrameArgs*)pa, sizeof(FrameArgs));
    }
#else
    e = a;
#endif
    publish_stats(e, maxd, closest, 0u);
    if (e.clock_probe && wv == 0u && blockIdx.x < SF_CLOCK_WAVES) {   // measurement: the end pair (see above)
        uint64_t* cp = e.clock_probe + 4u * blockIdx.x;
        cp[2] = __builtin_amdgcn_s_memtime();
        cp[3] = __builtin_amdgcn_s_memrealtime();
    }
    if (!LEAN && (e.flags & SF_FLAG_DIAG_UNITS) && e.tile_trace) {   // diagnostics: this wave's {start, end}
        const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * WAVES + wv);
        if (w < SF_DIAG_WAVES) {
            uint64_t* wt = e.tile_trace + (SF_TRACE_WORDS(e.tiles_x * e.tile_rows) - 2u * SF_DIAG_WAVES) + 2u * w;
            wt[0] = w_start;
            wt[1] = __builtin_amdgcn_s_memrealtime();
        }
    }
}

// the product launch of frames of many tiles (1080p and up): the lean loop over pair units -- two adjacent tiles per
// wave, sharing the traversal's upper levels (traverse_pair)
extern "C" __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SF_PAIR_WAVES_PER_EU, SF_PAIR_WAVES_PER_EU)))
void sf_trace_queue1(FrameArgs a)
{
    trace_queue_body<1, false, false, true, 1>(a);
}
// the same recording unit costs: the render that rebuilds the order of pair units
extern "C" __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SF_PAIR_WAVES_PER_EU, SF_PAIR_WAVES_PER_EU)))
void sf_trace_queue1c(FrameArgs a)
{
    trace_queue_body<1, false, false, true, 2>(a);
}
// the lean loop over single tiles (whole tiles of one plain frame, see trace_queue_body): the product launch of the
// smaller frames
extern "C" __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SF_WAVES_PER_EU, 8))) void sf_trace_queue1t(FrameArgs a)
{
    trace_queue_body<1, false, false, true>(a);
}
// the general instantiation: every mode of the tile loop (part units, diagnostics, tile costs, packed slabs, aux
// channels, band shares)
extern "C" __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SF_WAVES_PER_EU, 8))) void sf_trace_queue1g(FrameArgs a)
{
    trace_queue_body<1>(a);
}
// the same with subtree-split units (SF_FLAG_SUBTREE): renders whose unit order holds split tiles
extern "C" __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SF_WAVES_PER_EU, 8))) void sf_trace_queue1s(FrameArgs a)
{
    trace_queue_body<1, false, true>(a);
}
extern "C" __global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(SF_WAVES_PER_EU, 8))) void sf_trace_queue2(FrameArgs a)
{
    trace_queue_body<2>(a);
}
extern "C" __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SF_WAVES_PER_EU, 8))) void sf_trace_queue4(FrameArgs a)
{
    trace_queue_body<4>(a);
}
// active-ray compaction of sparse nodes (opt-in, SF_COMPACT=1; see traverse_ray): measured against the default
extern "C" __global__ __launch_bounds__(128) __attribute__((amdgpu_waves_per_eu(SF_WAVES_PER_EU, 8))) void sf_trace_queue2c(FrameArgs a)
{
    trace_queue_body<2, true>(a);
}

// Multi-frame persistent trace (round 6, sf_render_frames): ONE resident grid takes the work units of
// up to SF_BATCH_MAX frames -- each a slot context's own view, G-buffer and stats -- from one set of tile queues. A
// wave whose frame runs dry goes on with the next frame's units, so there is no per-frame launch, no hardware queue
// per frame and no frame boundary where waves wait for a successor grid; and the launch's sequence starts with the
// `heavy` heaviest units of EVERY frame of the batch, interleaved (the static first unit of wave w is position w), so
// no frame's heaviest tiles start late and leave a serial tail (the reference's workers likewise trace continuously,
// Sphereflake.cpp:67-74,112-213). Position G of the sequence:
// (units: the shared order's unit count, read on the device like trace_queue_body's; heavy: at most units)
//   G < nframes x heavy:  frame G % nframes, order position G / nframes (the interleaved heads)
//   else (q = G - nframes x heavy): frame q / (units - heavy), order position heavy + q % (units - heavy)
// Per frame everything is as in trace_queue_body<1>: the frame's FrameArgs re-read from the kernel argument segment
// per unit (scalar loads), its root staged in the wave's LDS when the wave's frame changes, its stats published when
// the wave leaves the frame. The frames share the unit order (the camera moves little between frames), the queues
// and their parity (the host gives every frame the first context's); only one frame may record tile costs.
// The batch in the kernel argument segment, through an address the compiler may not reason about: every read is a
// scalar load where it is used, so no batch word stays live in an SGPR across the tile loop (the loop's state is a few
// words: the wave's next position, its frame, its queue, its stats).
__device__ __forceinline__ const __attribute__((address_space(4))) FrameBatch* kernarg_batch()
{
    typedef const __attribute__((address_space(4))) FrameBatch* KernargBatch;
    KernargBatch pa = (KernargBatch)__builtin_amdgcn_kernarg_segment_ptr();
    __asm__ volatile("" : "+s"(pa));
    return pa;
}

__device__ __forceinline__ void load_frame(FrameArgs& at, uint32_t f)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const __attribute__((address_space(4))) FrameArgs* KernargArgs;
    KernargArgs pf = &((const __attribute__((address_space(4))) FrameBatch*)__builtin_amdgcn_kernarg_segment_ptr())->f[f];
    __asm__ volatile("" : "+s"(pf));   // (opaque: the fields are loaded where trace_tile uses them, as in trace_queue_body)
    __builtin_memcpy(&at, (const FrameArgs*)pf, sizeof(FrameArgs));
#else
    (void)at;
    (void)f;
#endif
}

template <int WAVES = 1>   // (one wave per workgroup; a template like trace_queue_body, for the shared `lds` declaration)
__device__ __forceinline__ void trace_frames_body()
{
    extern __shared__ float lds[];
    const uint64_t w_start = __builtin_amdgcn_s_memrealtime();
    {
        const auto pb = kernarg_batch();
        if (blockIdx.x == 0 && threadIdx.x < SF_QUEUES)   // the next launch's queues and overflow count
            pb->f[0].counters[SF_QUEUE_WORD(pb->f[0].parity ^ 1u, threadIdx.x)] = 0u;
        if (blockIdx.x == 0 && threadIdx.x == 0) pb->f[0].counters[pb->f[0].parity ^ 1u] = 0u;
        if (pb->f[0].clock_probe && blockIdx.x < SF_CLOCK_WAVES) {   // measurement: the live clock (trace_queue_body)
            uint64_t* cp = pb->f[0].clock_probe + 4u * blockIdx.x;
            cp[0] = __builtin_amdgcn_s_memtime();
            cp[1] = w_start;
        }
    }
    float* const L = lds;
    const float4 bcol = build_column(kernarg_batch()->f[0].consts);   // (the slot contexts' constant blocks are equal)
    uint32_t k;
    {
        const auto pb = kernarg_batch();
        const uint32_t nq = pb->f[0].queues, nx = pb->f[0].xcds;
        k = blockIdx.x & (nx - 1u);
        if (nq > nx) {
            const uint32_t lx = __builtin_ctz(nx);
            k += nx * ((blockIdx.x >> lx) & ((nq >> lx) - 1u));
        }
        k = __builtin_amdgcn_readfirstlane(k);
    }
    // per-frame stats in the lanes of two VGPRs -- lane f: frame f's max depth and closest-hit key so far -- published
    // once per frame when the wave ends: publishing at every frame switch (two agent-scope loads, maybe atomics) put a
    // ~2-us latency on the switch, which a wave of a banded share meets at nearly every unit
    uint32_t stat_d = 0xffffffffu;                  // (int -1)
    uint32_t stat_k = (uint32_t)sf_float_key(FLT_MAX);
    uint32_t cur = 0xffffffffu;   // the frame of the last unit (uniform)
    uint32_t staged = 0xffffffffu;   // the frame whose root is staged in LDS (uniform)
    uint32_t first = __builtin_amdgcn_readfirstlane(blockIdx.x);
    for (;;) {
        const uint32_t G = first;
        const bool again = (G >> 31) != 0u;
        uint32_t f = cur, pos = 0u;
        if (!again) {
            const auto pb = kernarg_batch();
            const uint32_t nframes = pb->nframes;
            // units per frame: the shared order's (order_meta[0]: split tiles count as their parts), else the tiles
            uint32_t units = pb->units;
            if (pb->f[0].tile_order) {
#if defined(__HIP_DEVICE_COMPILE__)
                typedef const __attribute__((address_space(4))) uint32_t* ConstU32;
                units = ((ConstU32)(const void*)pb->f[0].order_meta)[0];
#else
                units = pb->f[0].order_meta[0];
#endif
            }
            const uint32_t heavy = pb->heavy < units ? pb->heavy : units;
            if (G >= nframes * units) break;
            // (no integer division per unit: a division by a uniform value is a ~35-instruction scalar sequence, and
            // four of them per unit measured +18 % SALU against trace_queue_body)
            const uint32_t hh = nframes * heavy;
            if (G < hh) {
                pos = __builtin_amdgcn_readfirstlane(__umulhi(G, pb->magic));   // G / nframes (exact for G < 2^29)
                f = G - pos * nframes;
            } else {
                uint32_t q = G - hh;
                const uint32_t rest = units - heavy;
                f = 0u;
                while (q >= rest) {   // (<= SF_BATCH_MAX - 1 trips)
                    q -= rest;
                    ++f;
                }
                pos = heavy + q;
            }
            f = __builtin_amdgcn_readfirstlane(f);
            pos = __builtin_amdgcn_readfirstlane(pos);
        }
        cur = f;
        FrameArgs at;
        load_frame(at, f);
        if (f != staged) {   // (the frame's root transform into the wave's LDS image)
            stage_root_all_lanes(L, at.root);
            staged = f;
        }
        uint32_t t = pos, part = 0u;
        if (again) {
            t = G & SF_UNIT_TILE_MASK;
            part = (G >> SF_UNIT_PRIO_SHIFT) & 7u;
        } else if (at.tile_order) {
#if defined(__HIP_DEVICE_COMPILE__)
            typedef const __attribute__((address_space(4))) uint32_t* ConstU32;
            const uint32_t u = ((ConstU32)(const void*)at.tile_order)[pos];
#else
            const uint32_t u = at.tile_order[pos];
#endif
            t = u & SF_UNIT_TILE_MASK;
            part = u >> SF_UNIT_PART_SHIFT;
            const uint32_t pr = (u >> SF_UNIT_PRIO_SHIFT) & 3u;
            if (pr == 2u && !(at.flags & SF_FLAG_PRIO_FLAT)) __builtin_amdgcn_s_setprio(3);
            else if (pr != 0u) __builtin_amdgcn_s_setprio(2);
            else __builtin_amdgcn_s_setprio(0);
        }
        auto ticket = [&](bool retrace) {
            first = retrace ? (0x80000000u | (part << SF_UNIT_PRIO_SHIFT) | t)
                            : gridDim.x + wave_fetch_add(at.counters + SF_QUEUE_WORD(at.parity, k), 1u) * at.queues + k;
        };
        // the cull's depth seed is per frame, as the stats words are: frame f's word and this wave's maximum in frame f
        const DepthSeed seen{ (int32_t)__builtin_amdgcn_readlane(stat_d, f), stats_word(at) };
        const TileStats st = trace_tile<false, decltype(ticket)>(at, L, bcol, t, at.max_depth, at.overflow_list,
                                                                      at.counters + at.parity, part, ticket,
                                                                      again ? (at.flags | SF_FLAG_NO_FRONT_FIRST |
                                                                               SF_FLAG_REDO_PASS)
                                                                            : at.flags, 0u, seen);
        {   // frame cur's stats: the unit's max depth and closest hit into lane cur of the accumulators
            const int32_t ud = __builtin_amdgcn_readfirstlane(st.maxd);
            const int32_t uk = __builtin_amdgcn_readfirstlane(sf_float_key(wave_min(st.closest)));
            const int32_t od = (int32_t)__builtin_amdgcn_readlane(stat_d, cur);
            const int32_t ok = (int32_t)__builtin_amdgcn_readlane(stat_k, cur);
            stat_d = writelane_s((uint32_t)(ud > od ? ud : od), cur, stat_d);
            stat_k = writelane_s((uint32_t)(uk < ok ? uk : ok), cur, stat_k);
            if (st.seed >= 0 && ud > st.seed) {   // (rare: the frame's word follows at once, see publish_depth_early)
                FrameArgs ap;
                load_frame(ap, cur);
                publish_depth_early(ap, ud);
            }
        }
    }
    {   // every frame's stats once (read before the atomics: thousands of waves end together, publish_stats)
        const uint32_t nframes = kernarg_batch()->nframes;
        for (uint32_t fr = 0u; fr < nframes; ++fr) {
            const int32_t dd = (int32_t)__builtin_amdgcn_readlane(stat_d, fr);
            const int32_t kk = (int32_t)__builtin_amdgcn_readlane(stat_k, fr);
            if (dd < 0 && kk == sf_float_key(FLT_MAX)) continue;   // (no unit of that frame)
            FrameArgs e;
            load_frame(e, fr);
            publish_stats_in_loop(e, dd, sf_key_float(kk));
        }
    }
    const auto pb = kernarg_batch();
    if (pb->f[0].clock_probe && blockIdx.x < SF_CLOCK_WAVES) {
        uint64_t* cp = pb->f[0].clock_probe + 4u * blockIdx.x;
        cp[2] = __builtin_amdgcn_s_memtime();
        cp[3] = __builtin_amdgcn_s_memrealtime();
    }
}

extern "C" __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SF_WAVES_PER_EU, 8))) void sf_trace_frames1(FrameBatch b)
{
    (void)b;   // (read through the kernel argument segment, per unit: trace_frames_body)
    trace_frames_body<1>();
}

// Tile order for the next render: tiles sorted by this render's cost, heaviest first (LPT list
// scheduling of the persistent kernel), as a counting sort over SF_ORDER_BUCKETS log-spaced cost
// buckets (2 per octave of cycles). The trace kernel counts every finished tile into its 64-tile
// chunk's bucket histogram (one fire-and-forget atomic); sf_order_scan turns the histograms into
// per-(chunk, bucket) output offsets, heaviest bucket first and chunks in order within a bucket;
// sf_order_scatter (one wave per chunk) writes the permutation and clears the histograms. Stable and
// deterministic. Any permutation gives the same image: only the schedule changes.
// One 64-item chunk c of the scatter, one wave (lane = item within the chunk).
// (rank_out, when not NULL: rank_out[i] = item i's position, the inverse permutation; unsplit orders only)
// (offs: lane b's value is bucket b & 31's output offset for this chunk)
__device__ __forceinline__ void order_scatter_chunk(uint32_t c, uint32_t lane, const uint32_t* __restrict__ cost,
                                                    uint32_t n, uint32_t* __restrict__ chunk_cnt, uint32_t offs,
                                                    uint32_t split_from, uint32_t parts, uint32_t pb,
                                                    uint32_t* __restrict__ order, uint32_t* __restrict__ rank_out)
{
    const uint32_t i = c * 64u + lane;
    const uint32_t first = parts == 4u ? SF_PART_QUARTER0 : SF_PART_HALF0;
    const uint32_t bk = i < n ? cost_bucket(cost[i]) : SF_ORDER_BUCKETS;   // sentinel: no tile
    uint64_t pending = __builtin_amdgcn_ballot_w64(bk < SF_ORDER_BUCKETS);
    while (pending) {   // one round per distinct bucket in the chunk
        const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)bk, (int)__builtin_ctzll(pending));
        const uint64_t m = __builtin_amdgcn_ballot_w64(bk == b);
        const uint32_t off = (uint32_t)__builtin_amdgcn_readlane((int)offs, (int)b);
        if (bk == b) {
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            // the unit's wave priority next render (see SF_UNIT_PRIO_SHIFT)
            const uint32_t u = i | ((b >= pb + 3u ? 2u : b >= pb ? 1u : 0u) << SF_UNIT_PRIO_SHIFT);
            if (b >= split_from) {   // `parts` part units, adjacent
                for (uint32_t p = 0; p < parts; ++p) order[off + parts * rank + p] = u | ((first + p) << SF_UNIT_PART_SHIFT);
            } else {
                order[off + rank] = u;
                if (rank_out) rank_out[i] = off + rank;
            }
        }
        pending &= ~m;
    }
    if (lane < SF_ORDER_BUCKETS) chunk_cnt[c * SF_ORDER_BUCKETS + lane] = 0u;   // for the next render
}

// The order's split and priority decisions and the bucket output offsets, by one wave: lane l holds bucket l's
// tile count t (lanes 32..63: 0). Returns the first split bucket and the first raised-priority bucket; X_excl = the
// units of the buckets heavier than l (lane l), units = all the units.
struct OrderPlan {
    int bs, bp;
    uint32_t X_excl, units;
};
__device__ __forceinline__ OrderPlan order_decide(uint32_t t, uint32_t l, uint32_t n_tiles, uint32_t split_buckets,
                                                  uint32_t parts, uint32_t spare, uint32_t waves, uint32_t prio_buckets,
                                                  uint32_t split_cap)
{
    // One wave, lane = bucket (lanes 32..63 hold 0): the split and priority decisions and the bucket
    // offsets from suffix sums over the buckets (heaviest first), instead of serial loops on one thread.
    // Split tiles into `parts` units each, heaviest buckets first (bucket 0 never): automatically as
    // many whole buckets as fit into `spare` idle wave slots, or the top `split_buckets` occupied
    // buckets (at most an eighth of the tiles).
    uint32_t S = t;   // S(l) = sum of tot[bb] over bb >= l
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_down((int)S, o, 64);
        S += l + (uint32_t)o < SF_ORDER_BUCKETS ? up : 0u;
    }
    const uint64_t nz = __builtin_amdgcn_ballot_w64(t != 0u);
    const int btop = nz ? 63 - __builtin_clzll(nz) : 0;   // highest occupied bucket (0 if none)
    int bs = (int)SF_ORDER_BUCKETS;
    if (split_buckets == SF_SPLIT_AUTO) {
        // S is non-increasing in the bucket: the buckets that fit form a suffix
        const uint64_t ok = __builtin_amdgcn_ballot_w64(l >= 1u && l < SF_ORDER_BUCKETS && S * (parts - 1u) <= spare);
        if (ok >> (SF_ORDER_BUCKETS - 1u) & 1ull) bs = __builtin_ctzll(ok);
    } else if (split_buckets == SF_SPLIT_MODEL && waves > 0u) {
        // Makespan model (LPT list scheduling on `waves` slots, the last render's costs): unsplit, the
        // frame takes at least max(C / waves, c_top); splitting buckets >= l into `parts` units adds their
        // work x (parts x rho - 1) and leaves max(the heaviest unsplit bucket, rho x c_top) as the longest
        // unit (rho: the slowest part's share of its tile, measured 0.6 for quarters, 0.68 for halves).
        // Take the l of the least estimate when it is >= 10 % below the unsplit one.
        const float rho = parts == 4u ? 0.6f : 0.68f;
        const uint32_t e = (l + 16u) >> 1;   // bucket l covers [2^e (1 + m/2), ...) cycles, m = (l + 16) & 1
        const float c = l < SF_ORDER_BUCKETS ? __builtin_ldexpf((l + 16u) & 1u ? 1.75f : 1.25f, (int)e) : 0.0f;
        const float w = (float)t * c;   // this bucket's work
        float A = w;                    // A(l) = work of the buckets >= l
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) {
            const float up = __shfl_down(A, o, 64);
            A += l + (uint32_t)o < SF_ORDER_BUCKETS ? up : 0.0f;
        }
        const float C = __shfl(A, 0, 64);                 // all the work
        const float ctop = __shfl(c, btop, 64);
        const uint64_t below = nz & ((1ull << l) - 1ull);   // occupied buckets under l
        const float cun = below ? __shfl(c, 63 - __builtin_clzll(below), 64) : 0.0f;
        const float Tn = fmaxf(C / (float)waves, ctop);
        float T = fmaxf(fmaxf((C + A * ((float)parts * rho - 1.0f)) / (float)waves, cun), rho * ctop);
        if (!(l >= 1u && (int)l <= btop)) T = __builtin_inff();
        float Tm = T;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) Tm = fminf(Tm, __shfl_xor(Tm, o, 64));
        const uint64_t best = __builtin_amdgcn_ballot_w64(T == Tm);
        if (Tm < 0.9f * Tn && best) bs = 63 - __builtin_clzll(best);   // (ties: the fewest splits)
    } else if (split_buckets != 0u) {
        int b0 = btop - (int)split_buckets + 1;
        if (b0 < 1) b0 = 1;
        // then drop buckets from the bottom of the range while more than an eighth of the tiles split
        const uint64_t ok = __builtin_amdgcn_ballot_w64((int)l >= b0 && l < SF_ORDER_BUCKETS && 8u * S <= n_tiles);
        bs = ok ? __builtin_ctzll(ok) : (int)SF_ORDER_BUCKETS;
    }
    // at most split_cap split tiles (the subtree parts' records are per split slot): S(l) is non-increasing
    {
        const uint64_t capok = __builtin_amdgcn_ballot_w64(l < SF_ORDER_BUCKETS && S <= split_cap);
        const int bcap = capok ? __builtin_ctzll(capok) : (int)SF_ORDER_BUCKETS;
        if (bs < bcap) bs = bcap;
    }
    // the top `prio_buckets` occupied cost buckets run at raised wave priority next render (their
    // serial DFS is the frame's critical path)
    const int bp = btop - (int)prio_buckets + 1;
    // units per bucket -> exclusive offsets, heaviest first: X(l) = sum of units over bb > l
    const uint32_t x = t * ((int)l >= bs ? parts : 1u);
    uint32_t X = x;
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_down((int)X, o, 64);
        X += l + (uint32_t)o < SF_ORDER_BUCKETS ? up : 0u;
    }
    OrderPlan r;
    r.bs = bs;
    r.bp = bp;
    r.X_excl = X - x;
    r.units = (uint32_t)__shfl(X, 0, 64);
    return r;
}

#define SF_SCAN_BATCH 16   // chunk counts a scan thread loads at once (independent loads, one wait)

extern "C" __global__ __launch_bounds__(1024) void sf_order_scan(uint32_t* __restrict__ chunk_cnt, uint32_t nc,
                                                                   uint32_t n_tiles, uint32_t split_buckets, uint32_t parts,
                                                                   uint32_t spare, uint32_t waves, uint32_t prio_buckets,
                                                                   uint32_t* __restrict__ chunk_off,
                                                                   uint32_t* __restrict__ order_meta,
                                                                   const uint32_t* __restrict__ fuse_cost,
                                                                   uint32_t* __restrict__ fuse_order, uint32_t split_cap)
{
    // fuse_cost / fuse_order not NULL: this workgroup also does sf_order_scatter's work afterwards (its 16 waves
    // over the chunks), one launch instead of two -- for frames of few chunks, where the second launch's host
    // cost and dispatch latency exceed the scatter itself
    // (with frames in flight this one workgroup shares the CUs with other frames' trace waves, whose heavy
    // tiles run at raised priority: without its own it waited ~125 us instead of ~8 for issue slots)
    __builtin_amdgcn_s_setprio(3);
    // thread = (bucket b = tid % 32, slice k = tid / 32): chunks [k * per, (k + 1) * per) of bucket b
    __shared__ uint32_t part[32][SF_ORDER_BUCKETS + 1];
    __shared__ uint32_t tot[SF_ORDER_BUCKETS];
    const uint32_t tid = threadIdx.x, b = tid % SF_ORDER_BUCKETS, k = tid / SF_ORDER_BUCKETS;
    const uint32_t per = (nc + 31u) / 32u, c0 = k * per, c1 = min(nc, c0 + per);
    uint32_t s_ = 0u;
    uint32_t v0[SF_SCAN_BATCH];   // the first batch stays in registers for the offsets pass below (frames of up
                                  // to 32 x SF_SCAN_BATCH chunks, 1080p included, need no second read)
#pragma unroll
    for (int j = 0; j < SF_SCAN_BATCH; ++j) v0[j] = c0 + j < c1 ? chunk_cnt[(c0 + j) * SF_ORDER_BUCKETS + b] : 0u;
#pragma unroll
    for (int j = 0; j < SF_SCAN_BATCH; ++j) s_ += v0[j];
    for (uint32_t cb = c0 + SF_SCAN_BATCH; cb < c1; cb += SF_SCAN_BATCH) {
        uint32_t v[SF_SCAN_BATCH];
#pragma unroll
        for (int j = 0; j < SF_SCAN_BATCH; ++j) v[j] = cb + j < c1 ? chunk_cnt[(cb + j) * SF_ORDER_BUCKETS + b] : 0u;
#pragma unroll
        for (int j = 0; j < SF_SCAN_BATCH; ++j) s_ += v[j];
    }
    part[k][b] = s_;
    __syncthreads();
    if (tid < SF_ORDER_BUCKETS) {   // per bucket: slices -> exclusive prefix; bucket total
        uint32_t acc = 0u;
        for (uint32_t j = 0; j < 32u; ++j) {
            const uint32_t x = part[j][tid];
            part[j][tid] = acc;
            acc += x;
        }
        tot[tid] = acc;
    }
    __syncthreads();
    __shared__ uint32_t split_from;
    if (tid < 64u) {
        const uint32_t l = tid;
        const uint32_t t = l < SF_ORDER_BUCKETS ? tot[l] : 0u;
        const OrderPlan pl = order_decide(t, l, n_tiles, split_buckets, parts, spare, waves, prio_buckets, split_cap);
        const int bs = pl.bs, bp = pl.bp;
        const uint32_t X = pl.units;
        if (l < SF_ORDER_BUCKETS) tot[l] = pl.X_excl;
        if (l == 0u) {
            split_from = (uint32_t)bs;
            order_meta[0] = X;              // units of the next render
            order_meta[1] = (uint32_t)bs;   // first split bucket
            order_meta[2] = parts;          // units per split tile
            order_meta[3] = prio_buckets == 0u ? SF_ORDER_BUCKETS : (uint32_t)(bp < 0 ? 0 : bp);
        }
    }
    __syncthreads();
    const uint32_t mult = b >= split_from ? parts : 1u;
    uint32_t off = tot[b] + part[k][b] * mult;
#pragma unroll
    for (int j = 0; j < SF_SCAN_BATCH; ++j) {
        if (c0 + j < c1) chunk_off[(c0 + j) * SF_ORDER_BUCKETS + b] = off;
        off += v0[j] * mult;
    }
    for (uint32_t cb = c0 + SF_SCAN_BATCH; cb < c1; cb += SF_SCAN_BATCH) {
        uint32_t v[SF_SCAN_BATCH];
#pragma unroll
        for (int j = 0; j < SF_SCAN_BATCH; ++j) v[j] = cb + j < c1 ? chunk_cnt[(cb + j) * SF_ORDER_BUCKETS + b] : 0u;
#pragma unroll
        for (int j = 0; j < SF_SCAN_BATCH; ++j) {
            if (cb + j < c1) chunk_off[(cb + j) * SF_ORDER_BUCKETS + b] = off;
            off += v[j] * mult;
        }
    }
    if (fuse_order) {
        // chunk_off and the counts were written / read by this workgroup only: a workgroup barrier orders them
        __syncthreads();
        const uint32_t pb = order_meta[3];
        for (uint32_t c = tid >> 6; c < nc; c += blockDim.x >> 6)
            order_scatter_chunk(c, tid & 63u, fuse_cost, n_tiles, chunk_cnt,
                                chunk_off[c * SF_ORDER_BUCKETS + (tid & (SF_ORDER_BUCKETS - 1u))], split_from, parts, pb,
                                fuse_order, nullptr);
    }
}

extern "C" __global__ __launch_bounds__(64) void sf_order_scatter(const uint32_t* __restrict__ cost, uint32_t n,
                                                                    uint32_t* __restrict__ chunk_cnt,
                                                                    const uint32_t* __restrict__ chunk_off,
                                                                    const uint32_t* __restrict__ order_meta,
                                                                    uint32_t* __restrict__ order,
                                                                    uint32_t* __restrict__ rank_out)
{
    __builtin_amdgcn_s_setprio(3);   // (see sf_order_scan)
    order_scatter_chunk(blockIdx.x, threadIdx.x, cost, n, chunk_cnt,
                        chunk_off[blockIdx.x * SF_ORDER_BUCKETS + (threadIdx.x & (SF_ORDER_BUCKETS - 1u))],
                        order_meta[1], order_meta[2], order_meta[3], order, rank_out);
}

// The order rebuild of frames of many chunks in one-wave workgroups only (round 5): with frames in flight the
// persistent trace grids of the other frames refill every wave slot that frees, and sf_order_scan's 16-wave
// workgroup waited for 16 free slots on one CU -- 64 us median, up to 1.6 ms in the bench, its slot's next frame
// queued behind it (profiles/r5/order/). sf_order_bucket_scan: workgroup b (one wave) forms bucket b's per-chunk
// prefix over the chunks (lane l: chunks [l per, (l + 1) per)) and its total; sf_order_scatter_plan: every chunk's
// wave redoes the 32-lane plan (order_decide) from the totals and scatters its chunk.
extern "C" __global__ __launch_bounds__(64) void sf_order_bucket_scan(const uint32_t* __restrict__ chunk_cnt, uint32_t nc,
                                                                        uint32_t* __restrict__ chunk_rel,
                                                                        uint32_t* __restrict__ tot)
{
    __builtin_amdgcn_s_setprio(3);
    const uint32_t b = blockIdx.x, l = threadIdx.x;
    const uint32_t per = (nc + 63u) / 64u, c0 = l * per, c1 = min(nc, c0 + per);
    uint32_t s_ = 0u;
    for (uint32_t cb = c0; cb < c1; cb += SF_SCAN_BATCH) {
        uint32_t v[SF_SCAN_BATCH];
#pragma unroll
        for (int j = 0; j < SF_SCAN_BATCH; ++j) v[j] = cb + j < c1 ? chunk_cnt[(cb + j) * SF_ORDER_BUCKETS + b] : 0u;
#pragma unroll
        for (int j = 0; j < SF_SCAN_BATCH; ++j) s_ += v[j];
    }
    uint32_t incl = s_;   // inclusive prefix over the lanes
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, o, 64);
        incl += l >= (uint32_t)o ? up : 0u;
    }
    uint32_t off = incl - s_;
    for (uint32_t cb = c0; cb < c1; cb += SF_SCAN_BATCH) {
        uint32_t v[SF_SCAN_BATCH];
#pragma unroll
        for (int j = 0; j < SF_SCAN_BATCH; ++j) v[j] = cb + j < c1 ? chunk_cnt[(cb + j) * SF_ORDER_BUCKETS + b] : 0u;
#pragma unroll
        for (int j = 0; j < SF_SCAN_BATCH; ++j) {
            if (cb + j < c1) chunk_rel[(cb + j) * SF_ORDER_BUCKETS + b] = off;
            off += v[j];
        }
    }
    if (l == 63u) tot[b] = incl;
}

extern "C" __global__ __launch_bounds__(64) void sf_order_scatter_plan(const uint32_t* __restrict__ cost, uint32_t n,
                                                                         uint32_t* __restrict__ chunk_cnt,
                                                                         const uint32_t* __restrict__ chunk_rel,
                                                                         const uint32_t* __restrict__ tot,
                                                                         uint32_t split_buckets, uint32_t parts,
                                                                         uint32_t spare, uint32_t waves,
                                                                         uint32_t prio_buckets, uint32_t split_cap,
                                                                         uint32_t* __restrict__ order_meta,
                                                                         uint32_t* __restrict__ order)
{
    __builtin_amdgcn_s_setprio(3);
    const uint32_t l = threadIdx.x, c = blockIdx.x, bl = l & (SF_ORDER_BUCKETS - 1u);
    const uint32_t t = l < SF_ORDER_BUCKETS ? tot[l] : 0u;
    const uint32_t rel = chunk_rel[c * SF_ORDER_BUCKETS + bl];   // (in flight with the plan)
    const OrderPlan pl = order_decide(t, l, n, split_buckets, parts, spare, waves, prio_buckets, split_cap);
    const uint32_t pb = prio_buckets == 0u ? SF_ORDER_BUCKETS : (uint32_t)(pl.bp < 0 ? 0 : pl.bp);
    if (c == 0u && l == 0u) {
        order_meta[0] = pl.units;
        order_meta[1] = (uint32_t)pl.bs;
        order_meta[2] = parts;
        order_meta[3] = pb;
    }
    const uint32_t base = (uint32_t)__shfl((int)pl.X_excl, (int)bl, 64);
    const uint32_t offs = base + rel * ((int)bl >= pl.bs ? parts : 1u);
    order_scatter_chunk(c, l, cost, n, chunk_cnt, offs, (uint32_t)pl.bs, parts, pb, order, nullptr);
}

// Packed band slabs -> the frame G-buffer (multi-GPU gather). `stage` holds `members` slabs
// of members first .. first + members - 1 of a (band_rows, n) band split, each stage_rows x W float4
// (nx, ny, nz, minT) in the compact row order of sf_render_params.compact (member k's bands k, k + n, ...).
// Every pixel is rewritten at its frame position exactly as write_pixel would have: pos = (dir * t, 1) with
// dir recomputed by ray_dir from the same view (t < FLT_MAX: a hit; a miss leaves minT = FLT_MAX) or
// (0, 0, 0, 1), nrm = (n, 1). One thread per staged pixel, consecutive threads along a row: coalesced.
extern "C" __global__ __launch_bounds__(256) void sf_band_unpack(FrameArgs a, const float4* __restrict__ stage,
                                                                  uint32_t stage_rows, uint32_t band_rows, uint32_t n,
                                                                  uint32_t first, uint32_t members, uint32_t row0)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    const uint32_t sr = row0 + blockIdx.y;            // slab row (launches of <= 65535 rows)
    const uint32_t m = blockIdx.z;                    // member first + m
    if (x >= a.W || m >= members) return;
    const uint32_t k = first + m, i = sr / band_rows, r = sr % band_rows;
    const uint32_t y = (i * n + k) * band_rows + r;   // frame row
    if (y >= a.H) return;                             // (rows past this member's slab)
    const float4 v = stage[((size_t)m * stage_rows + sr) * a.W + x];
    float dx, dy, dz;
    ray_dir(a, (float)x, (float)y, dx, dy, dz, a.consts->lut);
    const bool hit = v.w < FLT_MAX;
    const size_t o = (size_t)y * a.W + x;
    reinterpret_cast<float4*>(a.pos)[o] = hit ? make_float4(dx * v.w, dy * v.w, dz * v.w, 1.0f) : make_float4(0.f, 0.f, 0.f, 1.0f);
    reinterpret_cast<float4*>(a.nrm)[o] = make_float4(v.x, v.y, v.z, 1.0f);
}

// Heap index -> its path digits (child numbers), deepest first, 4 bits each, and its depth (the reference's heap
// numbering: child i of node n is 9 n + 1 + i, Sphereflake.h:162-172). Indices of depth <= SF_INDEX_SLAB_DEPTH.
__device__ __forceinline__ uint32_t heap_path(uint32_t n, uint64_t& path)
{
    uint32_t d = 0;
    path = 0;
    while (n) {
        const uint32_t q = (n - 1u) / 9u;
        path |= (uint64_t)(n - 1u - 9u * q) << (4u * d);
        n = q;
        ++d;
    }
    return d;
}

// The frames of every node of depth <= SF_NODE_TABLE_DEPTH under the view's root transform, for the index slab
// unpack: node n's 12 floats (xf layout of child_frame) as 3 float4. One thread per node, chained from the root
// with child_frame -- the same float values the traversal builds (its per-ray form is sf_trace_ray's chain).
extern "C" __global__ __launch_bounds__(256) void sf_node_table(FrameArgs a, float4* __restrict__ table, uint32_t nodes)
{
    const uint32_t n = blockIdx.x * 256u + threadIdx.x;
    if (n >= nodes) return;
    uint64_t path;
    const uint32_t d = heap_path(n, path);
    float xf[12], nx[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) xf[k] = a.root[k];
    for (uint32_t j = 0; j < d; ++j) {
        child_frame(a.consts, j, (uint32_t)(path >> (4u * (d - 1u - j))) & 15u, xf, nx);
#pragma unroll
        for (int k = 0; k < 12; ++k) xf[k] = nx[k];
    }
    table[3u * n + 0u] = make_float4(xf[0], xf[1], xf[2], xf[3]);
    table[3u * n + 1u] = make_float4(xf[4], xf[5], xf[6], xf[7]);
    table[3u * n + 2u] = make_float4(xf[8], xf[9], xf[10], xf[11]);
}

// Index slabs -> the frame G-buffer (multi-GPU gather at 4 B per pixel). `stage` holds `members`
// slabs of uint32 heap indices (SF_SLAB_MISS: no hit) laid out as sf_band_unpack's. A hit's pixel is rebuilt with
// the tracer's own operations: the sphere's frame from the node table (its ancestor at depth <= table_depth) and
// child_frame for the levels below, then the node's self test (Sphereflake.h:174-224: tca, d2, the near root with
// r_d^2) gives minT, and shade's position dir * minT and normal Normalize(position - centre). Coalesced 4-B reads
// along a slab row, 2 x 16-B writes per pixel.
// A grid of resident workgroups, each first copying into LDS the constants every pixel reads at a lane-dependent
// index -- the rsqrtps table (ray_dir, shade), the 9 unit child frames, the depth scales and self radii^2, the first
// heap index of each depth -- then taking 256-pixel segments (member, slab row, x / 256) G = gridDim.x apart.
// Round 6:
//  * two items deep: while item i is rebuilt, item i + G's node-table frame and item i + 2G's slab word are already
//    loading, and no memory operation sits under a branch. gfx9 counts loads and stores on one in-order counter
//    (vmcnt), so a load consumed after a store waits for that store too, and at a join of paths that issued different
//    memory operations the compiler waits for all of them: round 5's loop (a branch around each item's stores, the
//    miss branch) waited for its own stores before every item (`s_waitcnt vmcnt(0)` at the loop head). Here a lane
//    past the frame's width redoes the row's last pixel and an item past a member's slab redoes item 0 -- the same
//    inputs, so the same bits stored twice -- and a miss is rebuilt as the root with its outputs selected after;
//  * the depth of an index from its leading-zero count and one threshold compare (was ten compares), the correctly
//    rounded square root and x86 rsqrtps in their fast forms with a wave-uniform fallback to the general ones (never
//    taken on the views the tests and the bench render), the frame constants read once per launch.
#define SF_DEPTH_MSB_BITS 0x92491249u   // bit k set iff some depth's first heap index (9^d - 1) / 8 has its MSB at k

struct UnpackLds {
    uint32_t lut[2048];
    float child[9][16];
    float scale[SF_DEPTH_TABLE];
    float r2_self[SF_DEPTH_TABLE];
    uint32_t first[12];   // first[c] = (9^(c+1) - 1) / 8: the first heap index of depth c + 1 (first[11]: none)
};

extern "C" __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void sf_slab_unpack4(
    FrameArgs a, const uint32_t* __restrict__ stage, const float4* __restrict__ table, uint32_t table_depth,
    uint32_t stage_rows, uint32_t band_rows, uint32_t n, uint32_t first, uint32_t members)
{
    __shared__ UnpackLds S;
    const DeviceConsts* __restrict__ K = a.consts;
    {
        for (uint32_t i = threadIdx.x; i < 2048u; i += 256u) S.lut[i] = K->lut[i];
        if (threadIdx.x < 144u) S.child[threadIdx.x >> 4][threadIdx.x & 15u] = K->child[threadIdx.x >> 4][threadIdx.x & 15u];
        if (threadIdx.x < SF_DEPTH_TABLE) {
            S.scale[threadIdx.x] = K->dt.scale[threadIdx.x];
            S.r2_self[threadIdx.x] = K->dt.r2_self[threadIdx.x];
        }
        if (threadIdx.x < 12u) {
            uint32_t f = 1u;
            for (uint32_t k = 0; k < threadIdx.x; ++k) f = 9u * f + 1u;
            S.first[threadIdx.x] = threadIdx.x < 11u ? f : 0xffffffffu;
        }
    }
    // ray_dir's constants (uniform, read once; ray_dir reads them per call)
    const float rw = K->rw, rh = K->rh;
    const bool fast = K->fast_div != 0u;
    __syncthreads();
    const uint32_t segs = (a.W + 255u) >> 8;
    const uint32_t items = members * stage_rows * segs;   // (< 2^32: 16384^2 frames give 2^22)
    const uint32_t G = gridDim.x;
    const uint32_t lane_x = threadIdx.x;
    // item -> its frame row y, its slab row's first word and its segment's first x (uniform, in SGPRs: located once
    // per item); the lane's pixel is x = min(xb + lane, W - 1) -- past the width, the row's last pixel again
    struct Loc { uint32_t y, row, xb; };
    auto locate = [&](uint32_t it) -> Loc {
        const uint32_t seg = it % segs, rest = it / segs;
        const uint32_t sr = rest % stage_rows, m = rest / stage_rows;
        const uint32_t k = first + m, i = sr / band_rows, r = sr % band_rows;
        return Loc{ (i * n + k) * band_rows + r, (m * stage_rows + sr) * a.W, seg << 8 };
    };
    // item 0 has the lowest frame row of the launch: without it no item has a row
    const Loc l0 = locate(0u);
    if (l0.y >= a.H) return;
    // the item it rebuilds: it itself, or item 0 past the items or past a member's slab
    auto item = [&](uint32_t it) -> Loc {
        const Loc l = locate(it < items ? it : 0u);
        return it < items && l.y < a.H ? l : l0;
    };
    auto lane_px = [&](const Loc& l) -> uint32_t { return min(l.xb + lane_x, a.W - 1u); };
    // one item in flight: its location, slab word, and once prepared its depth, table depth, the child digits below
    // the table's depth (the deepest in the highest nibble, depth td + 1's in the lowest) and its ancestor's table frame
    struct Slot {
        Loc l;
        uint32_t idx, d, td, path;
        float4 f0, f1, f2;
    };
    auto prepare = [&](Slot& q) {
        const uint32_t e = q.idx < SF_SLAB_BAD ? q.idx : 0u;   // (a miss: the root, its outputs replaced)
        const uint32_t c = __builtin_popcount(SF_DEPTH_MSB_BITS & (0x7fffffffu >> __builtin_clz(e | 1u)));
        const uint32_t d = c + (e >= S.first[c] ? 1u : 0u);
        const uint32_t td = d < table_depth ? d : table_depth;
        uint32_t anc = e, p = 0u;
        for (uint32_t j = d; j > td; --j) {
            const uint32_t qq = (anc - 1u) / 9u;
            p = (p << 4) | (anc - 1u - 9u * qq);
            anc = qq;
        }
        q.d = d;
        q.td = td;
        q.path = p;
        q.f0 = table[3u * anc];
        q.f1 = table[3u * anc + 1u];
        q.f2 = table[3u * anc + 2u];
    };
    // item it in slot P (its frame loaded), item it + G in slot Q (its slab word loaded): Q's frame loads and item
    // it + 2G's slab word (into P, once P's item is written) go out first, then P's pixel is rebuilt and stored
    auto step = [&](Slot& P, Slot& Q, uint32_t it) {
        prepare(Q);
        const Loc l2 = item(it + 2u * G);
        const uint32_t idx2 = stage[l2.row + lane_px(l2)];

        const uint32_t px_ = lane_px(P.l), py_ = P.l.y;
        float dx, dy, dz;
        {   // ray_dir with the constants read above
            const float fx = (float)px_, fy = (float)py_;
            float u, v;
            if (fast) {
                const float qu = fx * rw, qv = fy * rh;
                u = __builtin_fmaf(__builtin_fmaf(-qu, a.fw, fx), rw, qu);
                v = __builtin_fmaf(__builtin_fmaf(-qv, a.fh, fy), rh, qv);
            } else {
                u = fx / a.fw;
                v = fy / a.fh;
            }
            dx = ((a.tl[0] + a.dh[0] * u) + a.dv[0] * v) - a.o[0];
            dy = ((a.tl[1] + a.dh[1] * u) + a.dv[1] * v) - a.o[1];
            dz = ((a.tl[2] + a.dh[2] * u) + a.dv[2] * v) - a.o[2];
            normalize3_fast(dx, dy, dz, S.lut, true);
        }
        const bool hit = P.idx < SF_SLAB_BAD;
        float xf[12] = { P.f0.x, P.f0.y, P.f0.z, P.f0.w, P.f1.x, P.f1.y, P.f1.z, P.f1.w, P.f2.x, P.f2.y, P.f2.z, P.f2.w };
        uint32_t path = P.path;
        // the frames down to the parent, then only the sphere's centre: child_frame's translation column (the same
        // operations on the same operands)
        for (uint32_t j = P.td; j + 1u < P.d; ++j) {
            float nf[12];
            child_frame(S.child, S.scale, j, path & 15u, xf, nf);
            path >>= 4;
#pragma unroll
            for (int q = 0; q < 12; ++q) xf[q] = nf[q];
        }
        float cx, cy, cz;
        {
            const float sc = S.scale[P.d > 0u ? P.d - 1u : 0u];
            const float* B = S.child[path & 15u] + 12;   // (path & 15 <= 8; 0 where the table holds the sphere)
            const float b0 = B[0] * sc, b1 = B[1] * sc, b2 = B[2] * sc, b3 = B[3];
            const float ex = __builtin_fmaf(xf[9], b3, (xf[0] * b0 + xf[3] * b1) + xf[6] * b2);   // (SF_AFFINE_FMA)
            const float ey = __builtin_fmaf(xf[10], b3, (xf[1] * b0 + xf[4] * b1) + xf[7] * b2);
            const float ez = __builtin_fmaf(xf[11], b3, (xf[2] * b0 + xf[5] * b1) + xf[8] * b2);
            const bool below = P.d > P.td;
            cx = below ? ex : xf[9];
            cy = below ? ey : xf[10];
            cz = below ? ez : xf[11];
        }
        const float tca = (cx * dx + cy * dy) + cz * dz;
        const float d2 = ((cx * cx + cy * cy) + cz * cz) - tca * tca;
        const float R2 = S.r2_self[P.d];
        const float xs = R2 - d2;
        float t;   // (a hit's own self test passed: xs >= 0)
        if (wave_ballot(hit && !(xs >= 0x1p-96f)) != 0ull) t = near_root(tca, d2, R2);
        else t = near_root_big(tca, xs);
        // shade (Sphereflake.h:218-224)
        const float px = dx * t, py = dy * t, pz = dz * t;
        float qx = px - cx, qy = py - cy, qz = pz - cz;
        normalize3_fast(qx, qy, qz, S.lut, hit);
        const float mv = P.idx == SF_SLAB_MISS ? 0.0f : __builtin_nanf("");   // (SF_SLAB_BAD: never made by a correct split)
        const size_t o = (size_t)py_ * a.W + px_;
        reinterpret_cast<float4*>(a.pos)[o] = hit ? make_float4(px, py, pz, 1.0f) : make_float4(mv, mv, mv, 1.0f);
        reinterpret_cast<float4*>(a.nrm)[o] = hit ? make_float4(qx, qy, qz, 1.0f) : make_float4(mv, mv, mv, 1.0f);
        P.l = l2;
        P.idx = idx2;
    };

    Slot A, B;
    A.l = item(blockIdx.x);
    A.idx = stage[A.l.row + lane_px(A.l)];
    B.l = item(blockIdx.x + G);
    B.idx = stage[B.l.row + lane_px(B.l)];
    prepare(A);
    // unrolled twice, so the two slots swap roles without register moves
    for (uint32_t it = blockIdx.x; it < items; it += 2u * G) {
        step(A, B, it);
        if (it + G >= items) break;
        step(B, A, it + G);
    }
}

extern "C" __global__ __launch_bounds__(64) void sf_fixup_wave(FrameArgs a, const uint32_t* overflow_list,
                                                               uint32_t* counters, uint32_t parity)
{
    extern __shared__ float lds[];
    if (blockIdx.x == 0 && threadIdx.x == 0) counters[parity ^ 1u] = 0u;
    const uint32_t n = counters[parity];
    // workgroups without a tile leave at once (the usual case: no tile flagged), before the LDS setup: this
    // kernel sits between a frame's trace and the next render of its slot
    if (blockIdx.x >= n) return;
    int32_t maxd = -1;
    float closest = FLT_MAX;
    uint32_t unresolved = 0u;
    stage_root(lds, a.root);
    const float4 bcol = build_column(a.consts);
    // (the cull's depth seed, DepthSeed: the word and this wave's own tiles)
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const TileStats st = trace_tile<true>(a, lds, bcol, overflow_list[i], SF_MAX_LEVELS, nullptr, nullptr, 0u,
                                              NoPrefetch(), ~0u, 0u, DepthSeed{ maxd, stats_word(a) });
        maxd = st.maxd > maxd ? st.maxd : maxd;
        closest = fminf(closest, st.closest);
        unresolved += st.overflowed ? 1u : 0u;
    }
    publish_stats(a, maxd, closest, unresolved);
}

// ------------------------------------------------------------------------------------------
// Caller-supplied directions (sf_trace_dirs_to): ray i is the reference's ray with
// D = Normalize(dirs[i]) (SIMD_AVX.h:170-180) from the view's origin -- everything after ray generation
// (Sphereflake.cpp:167) is a function of D, the root transform, the child frames and the LOD constant only, so
// the frame's per-ray traversal (traverse_ray) serves it unchanged. One wave64 per group of rays: an 8x8 tile of
// the direction image (a.W x a.H, a.tiles_x tiles per row), or 64 consecutive rays of a list (a.H == 1). Outputs
// in ray order, the frame's pixel layout; any of the four may be NULL.
// ------------------------------------------------------------------------------------------
namespace {

// ---- what the groups of the seven list traces (this section and the six after it) share

// The lane's ray of a group. A lane past the end of the list or off the image edge takes the nearest ray inside (a
// real direction for the wave's cone) and traverses as an invalid lane: no load or store beyond the last ray.
struct GroupLane {
    uint32_t ray;      // index of the lane's ray or pixel, clamped into the list or image (< 2^31 of them)
    bool valid;        // the lane's own ray exists
    uint32_t mid;      // the cone axis lane: the tile's centre pixel (4, 4), or a mid lane of a list
    uint32_t tx, ty;   // the group's tile (an image)
    uint32_t x, y;     // the lane's own pixel, not clamped (an image)
};

// an 8x8 tile of the a.W x a.H image, a.tiles_x tiles per row
__device__ __forceinline__ GroupLane tile_lane(const FrameArgs& a, uint32_t group)
{
    const uint32_t lane = threadIdx.x & 63u;
    GroupLane g;
    g.ty = group / a.tiles_x;
    g.tx = group - g.ty * a.tiles_x;
    g.x = g.tx * SF_TILE + (lane & 7u);
    g.y = g.ty * SF_TILE + (lane >> 3);
    g.valid = g.x < a.W && g.y < a.H;
    g.ray = (g.y < a.H ? g.y : a.H - 1u) * a.W + (g.x < a.W ? g.x : a.W - 1u);
    g.mid = 36u;
    return g;
}

// 64 consecutive rays of a list (a.H == 1), else a tile
__device__ __forceinline__ GroupLane group_lane(const FrameArgs& a, uint32_t group)
{
    if (a.H != 1u) return tile_lane(a, group);
    GroupLane g;
    const uint32_t i = group * 64u + (threadIdx.x & 63u);   // (< 2^31 + 64)
    g.valid = i < a.W;
    g.ray = g.valid ? i : a.W - 1u;
    g.mid = 32u;
    g.tx = g.ty = g.x = g.y = 0u;
    return g;
}

// three finite numbers (no NaN, no infinity)
__device__ __forceinline__ bool finite3(float x, float y, float z)
{
    auto finite = [](float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; };
    return finite(x) && finite(y) && finite(z);
}

__device__ __forceinline__ HitState miss_state()
{
    HitState h;
    h.minT = FLT_MAX;
    h.cx = h.cy = h.cz = 0.f;
    h.index = 0xffffffffu;
    h.depth = -1;
    h.hit = false;
    return h;
}

// The cone axis lane of the live lanes `m` (not empty): the mid lane if it is one, else the first of them (`first`,
// where the caller has it already).
__device__ __forceinline__ uint32_t axis_lane(uint64_t m, uint32_t mid, uint32_t first)
{
    return __builtin_amdgcn_readfirstlane(((m >> mid) & 1ull) ? mid : first);
}
__device__ __forceinline__ uint32_t axis_lane(uint64_t m, uint32_t mid)
{
    return axis_lane(m, mid, (uint32_t)__builtin_ctzll(m));
}

// The wave kernel flags its group (uniform): the fixup kernel re-traces it at SF_MAX_LEVELS and rewrites its rays.
__device__ __forceinline__ void flag_group(uint32_t* overflow_list, uint32_t* overflow_count, uint32_t group)
{
    const uint32_t slot = wave_fetch_add(overflow_count, 1u);
    overflow_list[slot] = group;   // uniform value and address
}

// The four outputs of a valid lane's ray, any of them NULL.
__device__ __forceinline__ void store_ray(const FrameArgs& a, uint32_t ray, float dx, float dy, float dz,
                                          const HitState& h, const uint32_t* __restrict__ lut)
{
    float px, py, pz, nx, ny, nz;
    shade(dx, dy, dz, h, lut, px, py, pz, nx, ny, nz);
    if (a.pos) reinterpret_cast<float4*>(a.pos)[ray] = make_float4(px, py, pz, 1.0f);
    if (a.nrm) reinterpret_cast<float4*>(a.nrm)[ray] = make_float4(nx, ny, nz, 1.0f);
    if (a.min_t) a.min_t[ray] = h.minT;
    if (a.hit_index) a.hit_index[ray] = h.hit ? h.index : 0xffffffffu;
}

__device__ __forceinline__ TileStats group_stats(int32_t maxd, float closest, bool flagged)
{
    TileStats st;
    st.maxd = maxd;
    st.closest = closest;
    st.overflowed = flagged;
    return st;
}

// The shadow ray of the shadow traces, from the surface point w and the ray's origin l (the
// light): d = (w - l) + 0, len = sqrt((d.x d.x + d.y d.y) + d.z d.z), bound = len keep, d normalised -- every
// operation rounded on its own, in this order: the bits are the contract.
// (__builtin_sqrtf is the correctly rounded square root under the build's -fhip-fp32-correctly-rounded-divide-sqrt,
// as in near_root; __fsqrt_rn compiles to the bare v_sqrt_f32 here, 1 ulp off for some arguments)
__device__ __forceinline__ void shadow_ray(float wx, float wy, float wz, float lx, float ly, float lz, float keep,
                                           const uint32_t* __restrict__ lut, float& dx, float& dy, float& dz,
                                           float& bound)
{
    dx = __fadd_rn(__fsub_rn(wx, lx), 0.0f);
    dy = __fadd_rn(__fsub_rn(wy, ly), 0.0f);
    dz = __fadd_rn(__fsub_rn(wz, lz), 0.0f);
    const float len = __builtin_sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz)));
    bound = __fmul_rn(len, keep);
    normalize3(dx, dy, dz, lut);
}

// A tile's 64 visibility bytes (255 where the lane's ray was not stopped) from the ballot of `hit`. A whole tile of an
// image whose rows are 8-byte aligned is written by 8 lanes, one 8-byte row each (bit k of the row's byte of the
// ballot -> byte k, 255 where lit).
__device__ __forceinline__ void store_vis_tile(const FrameArgs& a, uint8_t* __restrict__ vis, const GroupLane& g,
                                               bool hit)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t litm = ~wave_ballot(hit);
    const bool rows8 = (a.W & 7u) == 0u && (reinterpret_cast<uintptr_t>(vis) & 7u) == 0u &&
                       g.tx * SF_TILE + SF_TILE <= a.W && g.ty * SF_TILE + SF_TILE <= a.H;   // (uniform)
    if (rows8) {
        if (lane < 8u) {
            const uint64_t b = (litm >> (8u * lane)) & 0xffull;
            const uint64_t s = (b * 0x0101010101010101ull) & 0x8040201008040201ull;   // byte k: bit k of b, in place
            const uint64_t n = ((s + 0x7f7f7f7f7f7f7f7full) >> 7) & 0x0101010101010101ull;   // byte k: 1 if set
            *reinterpret_cast<uint64_t*>(vis + (size_t)(g.ty * SF_TILE + lane) * a.W + g.tx * SF_TILE) = n * 0xffull;
        }
    } else if (g.valid) {
        vis[(size_t)g.y * a.W + g.x] = hit ? (uint8_t)0 : (uint8_t)255;
    }
}

// Where a fixup kernel stages the root image (stage_root of a.root) for the groups it re-traces.
enum class RootStage {
    Once,       // before the loop: the group reads the image and never writes it
    PerGroup,   // before every group, behind an lds_fence: the group may overwrite the image (per-origin passes)
    InGroup,    // not at all: the group stages what it needs itself
};

// The body of the seven fixup kernels (as sf_fixup_wave): re-trace counters[parity] groups of `overflow_list` with
// group_fn(group, bcol), one block at a time over the list; zero the next trace's counter and add this trace's to
// counters[2], the re-traced groups sf_get_stats reports. STATS: group_fn returns the group's TileStats, published as
// the renders' are (the shadow traces touch no statistic). (`a` by value: through a reference, sf_trace_rays_fixup
// had stage_root's lane compares hoisted out of its loop, 3 more SGPR spills. `lds` is the group's own L: no restrict.)
template <RootStage STAGE, bool STATS, class GroupFn>
__device__ __forceinline__ void fixup_groups(const FrameArgs a, float* lds, const uint32_t* overflow_list,
                                             uint32_t* counters, uint32_t parity, GroupFn group_fn)
{
    const uint32_t n = counters[parity];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        counters[parity ^ 1u] = 0u;
        counters[2] += n;
    }
    if (blockIdx.x >= n) return;
    int32_t maxd = -1;
    float closest = FLT_MAX;
    uint32_t unresolved = 0u;
    if constexpr (STAGE == RootStage::Once) stage_root(lds, a.root);
    const float4 bcol = build_column(a.consts);
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        if constexpr (STAGE == RootStage::PerGroup) {
            lds_fence();
            stage_root(lds, a.root);
        }
        if constexpr (STATS) {
            const TileStats st = group_fn(overflow_list[i], bcol);
            maxd = st.maxd > maxd ? st.maxd : maxd;
            closest = fminf(closest, st.closest);
            unresolved += st.overflowed ? 1u : 0u;
        } else {
            group_fn(overflow_list[i], bcol);
        }
    }
    if constexpr (STATS) publish_stats(a, maxd, closest, unresolved);
}

template <bool FIXUP>
__device__ __forceinline__ TileStats trace_dir_group(const FrameArgs& a, const float* __restrict__ dirs, uint32_t stride,
                                                     float* __restrict__ L, const float4 bcol, uint32_t group,
                                                     uint32_t levels, uint32_t* overflow_list, uint32_t* overflow_count)
{
    const DeviceConsts* __restrict__ K = a.consts;
    const GroupLane g = group_lane(a, group);
    const float* const dp = dirs + (size_t)g.ray * stride;
    float dx = dp[0], dy = dp[1], dz = dp[2];
    normalize3(dx, dy, dz, K->lut);
    // A direction that does not normalise to three finite numbers (zero, tiny, huge, NaN or infinite input) misses
    // in the reference: the root's tca = (cx dx + cy dy) + cz dz is then NaN or -inf, which fails tca >= 0
    // (SIMD_AVX.h:247-258), or +inf, where d2 = -inf passes the bounding test but the near root inf - inf = NaN
    // fails the LOD test (Sphereflake.h:146) -- the root is never entered. Such a lane is traced as an invalid
    // lane carrying the axis lane's direction, so the traversal's wave-level arithmetic (the cone, whose min
    // instructions drop NaNs) only ever sees finite directions; the axis lane is the mid lane, or where that one
    // is not finite the first lane that is.
    const bool fin = finite3(dx, dy, dz);
    const uint64_t finm = wave_ballot(fin);
    HitState h = miss_state();
    int32_t maxd = -1;
    uint32_t status = 0u;
    if (finm != 0ull) {   // (uniform; no finite lane: every ray of the group misses)
        const uint32_t axl = axis_lane(finm, g.mid);
        const float ax = readlane_f(dx, axl), ay = readlane_f(dy, axl), az = readlane_f(dz, axl);
        dx = fin ? dx : ax;
        dy = fin ? dy : ay;
        dz = fin ? dz : az;
        // only the culls' A/B switches of the context's flags reach this traversal; the fixup traces in index order
        const uint32_t flags = (a.flags & (SF_FLAG_NO_CONE_CULL | SF_FLAG_NO_OCCL_CULL | SF_FLAG_NO_FRONT_FIRST)) |
                               (FIXUP ? SF_FLAG_NO_FRONT_FIRST : 0u);
        traverse_ray<>(K, a.root, L, bcol, levels, dx, dy, dz, g.valid && fin, h, maxd, status, flags, nullptr, axl);
    }
    const bool flagged = status != 0u;   // (uniform) more levels needed, or a tie under the front-first order
    if (!FIXUP && flagged) flag_group(overflow_list, overflow_count, group);   // (re-traced in index order)
    if (g.valid) store_ray(a, g.ray, dx, dy, dz, h, K->lut);
    return group_stats(maxd, g.valid ? h.minT : FLT_MAX, flagged);
}

}  // namespace

// One group per one-wave workgroup, dynamic LDS for a.max_depth levels (as sf_trace_wave1).
extern "C" __global__ __launch_bounds__(64) void sf_trace_dirs_wave(FrameArgs a, const float* dirs, uint32_t stride,
                                                                    uint32_t groups, uint32_t* overflow_list,
                                                                    uint32_t* overflow_count)
{
    extern __shared__ float lds[];
    if (blockIdx.x >= groups) return;
    stage_root(lds, a.root);
    const TileStats st = trace_dir_group<false>(a, dirs, stride, lds, build_column(a.consts), blockIdx.x, a.max_depth,
                                                overflow_list, overflow_count);
    publish_stats(a, st.maxd, st.closest, 0u);
}

// Re-trace of the flagged groups at SF_MAX_LEVELS (fixup_groups). The traversal only reads the root image: staged once.
extern "C" __global__ __launch_bounds__(64) void sf_trace_dirs_fixup(FrameArgs a, const float* dirs, uint32_t stride,
                                                                     const uint32_t* overflow_list, uint32_t* counters,
                                                                     uint32_t parity)
{
    extern __shared__ float lds[];
    fixup_groups<RootStage::Once, true>(a, lds, overflow_list, counters, parity,
                                        [&](uint32_t group, const float4 bcol) {
        return trace_dir_group<true>(a, dirs, stride, lds, bcol, group, SF_MAX_LEVELS, nullptr, nullptr);
    });
}

// ------------------------------------------------------------------------------------------
// Caller-supplied origins and directions (sf_trace_rays_to): ray i is the reference's ray with
// D = Normalize(dirs[i]) under the root transform whose columns 0..2 are the context's and whose translation is
// 0 - origin (Sphereflake.cpp:83) -- what the reference returns for that direction after SetView at that origin.
// The rays of a group are grouped as sf_trace_dirs_wave groups them. A group whose rays share one origin (the same
// bits) runs the frame's own traversal (traverse_ray) on that origin's root image. A group of several origins runs
// traverse_mixed below: world = parent * child (SIMD_AVX.h:59-81) splits into the axis columns and the centre offset
// S = (P0 Tx + P1 Ty) + P2 Tz, which do not depend on the origin, and one addition per ray, centre = parent centre + S
// (fma(parent centre, 1, S): one rounding) -- so the wave still expands a node once for all its rays, and each lane
// carries its own centres.
// ------------------------------------------------------------------------------------------
namespace {

// traverse_mixed's third status bit: a shared axis-column sum was an exact -0. The reference adds parent centre x 0
// to it, a zero with the sign of the ray's own centre component, so the column's zero sign is then per ray (and can
// reach a normal's zero sign through n = p - C): the group is traced once per distinct origin instead.
#define SF_STATUS_ZSIGN 4u

// Index order, no cone, no front-first: the visits are the reference's, the ancestor rule of self_test the only tie
// to handle. Lbase: root image (its axis columns are read; the centre is per lane: ocx, ocy, ocz) and `levels` level
// tables, whose plane 0 holds the children's S instead of centres; cstk: the centre stack, `levels` x [3][64].
// ANYHIT: the any-hit mode of sf_trace_sun, traverse_ray's SHADOW mode on per-lane origins: h.minT
// starts at the lane's `bound`, a lane whose self test accepts (ts < bound; a tie is not `<`) is finished and leaves
// actv and every bit of actbits, there is no ancestor bookkeeping, the occlusion cull keeps only its distance
// condition, maxd is not maintained past 0, and the traversal ends when no lane is live. Only h.hit (the finished
// lanes) is meaningful on return. SF_STATUS_ZSIGN is not raised: a zero's sign cannot reach a comparison (§6.13).
template <bool ANYHIT = false>
__device__ __forceinline__ void traverse_mixed(const DeviceConsts* __restrict__ K, float* __restrict__ Lbase,
                                               float* __restrict__ cstk, const float4 bcol, uint32_t levels, float dx,
                                               float dy, float dz, float ocx, float ocy, float ocz, bool valid,
                                               HitState& h, int32_t& maxd, uint32_t& status, uint32_t K_flags,
                                               float bound = FLT_MAX)
{
    const uint32_t lane = threadIdx.x & 63u;
    const TraverseLds L{ Lbase };
    const bool occl_cull = (K_flags & SF_FLAG_NO_OCCL_CULL) == 0u;

    reset_hit(h, ANYHIT ? bound : FLT_MAX);
    uint64_t ancm = 0ull;   // lanes whose current best sphere is an ancestor of the open node

    // ---- root node (depth 0): bounding sphere + LOD, per lane on the lane's own root centre
    const float occ0 = (ocx * ocx + ocy * ocy) + ocz * ocz;
    const float4 dt0 = depth_consts(K, 0u);
    const float tca0 = (ocx * dx + ocy * dy) + ocz * dz;
    const float d20 = occ0 - tca0 * tca0;
    const bool ex0 = valid && tca0 >= 0.0f && d20 <= dt0.x && near_root(tca0, d20, dt0.x) < dt0.w;
    if (!wave_ballot(ex0)) return;
    maxd = 0;
    float cull_t = depth_consts(K, 1u).w;

    const BuildLane B = build_lane(bcol, lane, build_child(lane));

    // (accept_self in index order: a tie is accepted where the best is an ancestor, else dropped, never flagged)
    auto self_test = [&](const float4 pc, float tca, float d2, uint32_t dd, float actv, uint32_t idx,
                         float R2s) -> uint64_t {
        return accept_self<ANYHIT, true>(h, ancm, status, false, pc, tca, d2, dd, actv, idx, R2s);
    };

    // ---- the shared part of the 9 children of the node whose axis columns are at col + j cs, into table tb: their
    // axis columns (lanes 0..26) and their centre offsets S (the other lanes), the sums of build_children
    // without its fma of the parent centre (ko: byte offset of the children's depth constants)
    auto expand = [&](const float* col, uint32_t cs, float* tb, uint32_t ko) {
        lds_fence();
        const float3 p0 = *reinterpret_cast<const float3*>(col);
        const float3 p1 = *reinterpret_cast<const float3*>(col + cs);
        const float3 p2 = *reinterpret_cast<const float3*>(col + 2u * cs);
        const float sm = B.bc == 3u ? depth_word_at(K, ko - (1u << 5), 2u) : 1.0f;   // (4/3) r of the node's depth
        const float b0 = B.b0 * sm, b1 = B.b1 * sm, b2 = B.b2 * sm;
        const float x = (p0.x * b0 + p1.x * b1) + p2.x * b2;
        const float y = (p0.y * b0 + p1.y * b1) + p2.y * b2;
        const float z = (p0.z * b0 + p1.z * b1) + p2.z * b2;
        if constexpr (!ANYHIT) {
            const bool negz = B.bc != 3u && (__float_as_uint(x) == 0x80000000u || __float_as_uint(y) == 0x80000000u ||
                                           __float_as_uint(z) == 0x80000000u);
            if (wave_ballot(negz) != 0ull) status |= SF_STATUS_ZSIGN;
        }
        *reinterpret_cast<float3*>(tb + B.slot) = make_float3(x, y, z);
    };

    uint32_t stk_pc = 0u, stk_ix = 0u;   // VGPR stack, lane k = level k: untested children, idxB
    float* tcur = L.table(0u);
    float* const cs = cstk + lane;       // this lane's centre of the open node at depth k: cs[192 k + 64 j]
    uint32_t kofs = 1u << 5;
    float R2c = depth_consts_at(K, kofs).x;
    const uint32_t lv32 = __builtin_amdgcn_readfirstlane(levels << 5);
    uint32_t d = 0, idxB = 1, C;
    float actv;
    uint32_t actbits;
    {
        const float av0 = ex0 ? __builtin_inff() : -1.0f;
        const uint64_t acc0 = self_test(make_float4(ocx, ocy, ocz, occ0), tca0, d20, 0u, av0, 0u, dt0.y);
        // per lane: beyond the leaf threshold no child of the node can pass LOD for any ray (sfhost::leaf_threshold),
        // and a child is only ever tested for its own sphere once entered -- such a lane stops visiting here
        // (any-hit mode: so does a lane the root's own sphere finished)
        uint64_t live = wave_ballot(ex0 && !(occ0 > depth_leaf(K, 0u)));
        if constexpr (ANYHIT) live &= ~acc0;
        if (live == 0ull) {
            h.hit = h.depth >= 0;
            return;
        }
        actv = sel_mask(-1.0f, __builtin_inff(), live);
        actbits = actv > 0.0f ? 1u : 0u;
        cs[0] = ocx;
        cs[64] = ocy;
        cs[128] = ocz;
        expand(L.root() + 4u, 4u, tcur, kofs);
        C = 0x1ffu;
    }

    for (;;) {
        d = __builtin_amdgcn_readfirstlane(d);
        if (C) {
            const uint32_t c = __builtin_ctz(C);
            __asm__("s_bitset0_b32 %0, %1" : "+s"(C) : "s"(c));
            const float4 dc = depth_consts_at(K, kofs);
            lds_fence();
            const float3 S = *reinterpret_cast<const float3*>(tcur + c * 4u);
            const float cx = ocx + S.x, cy = ocy + S.y, cz = ocz + S.z;
            const float cc = (cx * cx + cy * cy) + cz * cz;
            const float tca = (cx * dx + cy * dy) + cz * dz;
            const float d2 = cc - tca * tca;
            const float xs = R2c - d2;
            const bool hb = __builtin_fminf(__builtin_fminf(tca, xs), actv) >= 0.0f;
            const uint64_t hbm = wave_ballot(hb);
            if (hbm == 0ull) continue;
            const float4 dk = depth_consts_at(K, kofs + 16u);   // depth d + 1's {leaf, cull, far}
            const uint64_t exm = lod_expands(tca, d2, xs, hb, hbm, dc.x, dc.w, dk.z);
            if (exm == 0ull) continue;
            if (kofs >= lv32) {   // (d + 1 >= levels) the group is re-traced with more levels: nothing here is kept
                status |= SF_STATUS_OVERFLOW;
                break;
            }
            if (!ANYHIT && (int32_t)d + 1 > maxd) {   // Sphereflake.h:157-160
                maxd = (int32_t)d + 1;
                cull_t = depth_consts_at(K, kofs + (1u << 5)).w;
            }
            // occlusion cull, per lane (occluded)
            uint64_t amx = exm;
            if (occl_cull) {
                amx = exm & ~occluded<ANYHIT>(tca, h.minT, cull_t, dk.y);
                if (amx == 0ull) continue;
            }
            const float avx = sel_mask(-1.0f, __builtin_inff(), amx);
            const uint64_t acc = self_test(make_float4(cx, cy, cz, cc), tca, d2, d + 1u, avx, idxB + c, dc.y);
            if constexpr (ANYHIT) {
                if (acc != 0ull) {   // finished lanes leave the child, the open node and every ancestor
                    amx &= ~acc;
                    actv = sel_mask(actv, -1.0f, acc);
                    sel_in_place(actbits, 0u, acc);
                    if (wave_ballot(actbits != 0u) == 0ull) break;   // no lane is live
                    if (amx == 0ull) continue;
                }
            }
            const uint64_t live = amx & ~wave_ballot(cc > dk.x);   // (the per-lane leaf cut, as at the root)
            if (live == 0ull) {
                if constexpr (!ANYHIT) ancm &= wave_ballot(h.depth != (int32_t)d + 1);   // the child is finished
                continue;
            }
            // push the open node, open child c
            stk_pc = writelane_s(C, d, stk_pc);
            stk_ix = writelane_s(idxB, d, stk_ix);
            {
                const uint32_t bit = 2u << d;   // level d + 1
                uint32_t ab = actbits & ~bit;
                sel_in_place(ab, ab | bit, live);
                actbits = ab;
            }
            idxB = 9u * (idxB + c) + 1u;
            d += 1u;
            actv = sel_mask(-1.0f, __builtin_inff(), live);
            ocx = cx;
            ocy = cy;
            ocz = cz;
            float* const cl = cs + d * SF_RAYS_CSTACK;
            cl[0] = cx;
            cl[64] = cy;
            cl[128] = cz;
            const float* const col = tcur + SF_LDS_PLANE + 3u * c;   // the entered child's axis columns
            tcur += SF_LDS_LEVEL;
            kofs += 1u << 5;
            expand(col, SF_LDS_COLS, tcur, kofs);
            R2c = depth_consts_at(K, kofs).x;
            C = 0x1ffu;
            continue;
        }
        // ---- the node at depth d is finished: a best sphere at depth d is no longer an ancestor
        ancm &= wave_ballot(h.depth != (int32_t)d);
        if (d == 0u) break;
        d -= 1u;
        tcur -= SF_LDS_LEVEL;
        kofs -= 1u << 5;
        R2c = depth_consts_at(K, kofs).x;
        C = (uint32_t)__builtin_amdgcn_readlane(stk_pc, d);
        idxB = (uint32_t)__builtin_amdgcn_readlane(stk_ix, d);
        actv = ((actbits >> d) & 1u) ? __builtin_inff() : -1.0f;
        const float* const cl = cs + d * SF_RAYS_CSTACK;
        ocx = cl[0];
        ocy = cl[64];
        ocz = cl[128];
    }
    h.hit = h.depth >= 0;
}

// One group of rays. mixed_ok: the launch provisioned the mixed traversal's LDS (SF_LDS_RAYS_FLOATS); without it a
// group of several origins is traced once per distinct origin, which is always exact. ONE: the host proved from the
// grouping that the rays of every group share an origin index (sf_trace_rays_one) -- one pass of the frame's
// traversal, no test, and no mixed traversal compiled in.
template <bool FIXUP, bool ONE = false>
__device__ __forceinline__ TileStats trace_ray_group(const FrameArgs& a, const float* __restrict__ origins,
                                                     const float* __restrict__ dirs, uint32_t ostride, uint32_t dstride,
                                                     uint32_t rpo, uint32_t mixed_ok, float* __restrict__ L,
                                                     const float4 bcol, uint32_t group, uint32_t levels,
                                                     uint32_t* overflow_list, uint32_t* overflow_count)
{
    const DeviceConsts* __restrict__ K = a.consts;
    const uint32_t lane = threadIdx.x & 63u;
    const GroupLane g = group_lane(a, group);
    const uint32_t ray = g.ray, mid = g.mid;
    const bool valid = g.valid;
    const float* const dp = dirs + (size_t)ray * dstride;
    const float* const op = origins + (size_t)(rpo > 1u ? ray / rpo : ray) * ostride;
    float dx = dp[0], dy = dp[1], dz = dp[2];
    // the root transform's translation for this origin (Sphereflake.cpp:83: 0 - origin per component)
    const float rx = 0.0f - op[0], ry = 0.0f - op[1], rz = 0.0f - op[2];
    normalize3(dx, dy, dz, K->lut);
    // a direction that does not normalise to finite numbers is a miss (see trace_dir_group). So is an origin that is
    // not finite: the root's tca is then NaN, -inf, or +inf with d2 = inf - inf = NaN, and the root is not entered --
    // traverse_mixed finds that by the reference's own arithmetic per lane, and a group that shares such an origin
    // leaves traverse_ray at its root test, before the cone.
    const bool on = valid && finite3(dx, dy, dz);
    const uint64_t onm = wave_ballot(on);
    HitState h = miss_state();
    int32_t maxd = -1;
    uint32_t status = 0u;
    if (onm != 0ull) {   // (uniform; else every ray of the group misses)
        const uint32_t f0 = __builtin_amdgcn_readfirstlane((uint32_t)__builtin_ctzll(onm));
        const bool same = __float_as_uint(rx) == __float_as_uint(readlane_f(rx, f0)) &&
                          __float_as_uint(ry) == __float_as_uint(readlane_f(ry, f0)) &&
                          __float_as_uint(rz) == __float_as_uint(readlane_f(rz, f0));
        const bool mixed = !ONE && ((onm & ~wave_ballot(same)) != 0ull || (a.flags & SF_FLAG_FORCE_MIXED) != 0u);
        const uint32_t culls = a.flags & (SF_FLAG_NO_CONE_CULL | SF_FLAG_NO_OCCL_CULL | SF_FLAG_NO_FRONT_FIRST);
        uint64_t todo = onm;
        if (!ONE && mixed && mixed_ok != 0u) {
            float* const cstk = L + SF_LDS_WAVE_FLOATS(levels + 1u);
            traverse_mixed(K, L, cstk, bcol, levels, dx, dy, dz, rx, ry, rz, on, h, maxd, status, culls);
            if (status & SF_STATUS_ZSIGN) {   // per-ray zero signs: nothing of this pass is kept
                status = 0u;
                maxd = -1;
                h = miss_state();
            } else {
                todo = 0ull;
            }
        }
        // ---- one origin at a time: the frame's traversal on that origin's root image, for the lanes that start
        // there (one pass for a group of one origin). The other lanes carry the axis lane's direction, invalid, so
        // the cone is the members'.
        while (todo != 0ull) {
            const uint32_t l0 = __builtin_amdgcn_readfirstlane((uint32_t)__builtin_ctzll(todo));
            float r[12];
#pragma unroll
            for (int k = 0; k < 9; ++k) r[k] = a.root[k];
            r[9] = readlane_f(rx, l0);
            r[10] = readlane_f(ry, l0);
            r[11] = readlane_f(rz, l0);
            const bool mine = on && (ONE || (__float_as_uint(rx) == __float_as_uint(r[9]) &&
                                             __float_as_uint(ry) == __float_as_uint(r[10]) &&
                                             __float_as_uint(rz) == __float_as_uint(r[11])));
            const uint64_t m = todo & wave_ballot(mine);   // (holds l0)
            const bool member = ((m >> lane) & 1ull) != 0ull;
            const uint32_t axl = axis_lane(m, mid, l0);   // (the first lane of m is l0)
            const float ax = readlane_f(dx, axl), ay = readlane_f(dy, axl), az = readlane_f(dz, axl);
            lds_fence();
            stage_root(L, r);
            HitState h1;
            int32_t md = -1;
            uint32_t st = 0u;
            traverse_ray<>(K, r, L, bcol, levels, member ? dx : ax, member ? dy : ay, member ? dz : az, member, h1, md,
                           st, culls | (FIXUP ? SF_FLAG_NO_FRONT_FIRST : 0u), nullptr, axl);
            if (member) h = h1;
            maxd = md > maxd ? md : maxd;
            status |= st;
            todo &= ~m;
            if (ONE) break;
        }
    }
    const bool flagged = status != 0u;   // (uniform) more levels needed, or a tie under the front-first order
    if (!FIXUP && flagged) flag_group(overflow_list, overflow_count, group);
    // (a lane that is not `on` kept the initial miss; its direction may be non-finite and shade ignores it)
    if (valid) store_ray(a, ray, dx, dy, dz, h, K->lut);
    return group_stats(maxd, valid ? h.minT : FLT_MAX, flagged);
}

}  // namespace

// One group per one-wave workgroup; dynamic LDS: SF_LDS_RAYS_FLOATS(a.max_depth) with mixed_ok, else
// SF_LDS_WAVE_FLOATS(a.max_depth).
extern "C" __global__ __launch_bounds__(64) void sf_trace_rays_wave(FrameArgs a, const float* origins, const float* dirs,
                                                                    uint32_t ostride, uint32_t dstride, uint32_t rpo,
                                                                    uint32_t mixed_ok, uint32_t groups,
                                                                    uint32_t* overflow_list, uint32_t* overflow_count)
{
    extern __shared__ float lds[];
    if (blockIdx.x >= groups) return;
    stage_root(lds, a.root);
    const TileStats st = trace_ray_group<false>(a, origins, dirs, ostride, dstride, rpo, mixed_ok, lds,
                                                build_column(a.consts), blockIdx.x, a.max_depth, overflow_list,
                                                overflow_count);
    publish_stats(a, st.maxd, st.closest, 0u);
}

// The same where the host proved one origin per group (one origin for all rays, or a list whose rays_per_origin is
// a multiple of 64): dynamic LDS SF_LDS_WAVE_FLOATS(a.max_depth), the launch of sf_trace_dirs_wave plus the origin.
extern "C" __global__ __launch_bounds__(64) void sf_trace_rays_one(FrameArgs a, const float* origins, const float* dirs,
                                                                   uint32_t ostride, uint32_t dstride, uint32_t rpo,
                                                                   uint32_t groups, uint32_t* overflow_list,
                                                                   uint32_t* overflow_count)
{
    extern __shared__ float lds[];
    if (blockIdx.x >= groups) return;
    const TileStats st = trace_ray_group<false, true>(a, origins, dirs, ostride, dstride, rpo, 0u, lds,
                                                      build_column(a.consts), blockIdx.x, a.max_depth, overflow_list,
                                                      overflow_count);
    publish_stats(a, st.maxd, st.closest, 0u);
}

// Re-trace of the flagged groups at SF_MAX_LEVELS (fixup_groups; sf_trace_dirs_fixup's list and counters). A group
// traced per origin overwrites the root image: restaged before every group.
extern "C" __global__ __launch_bounds__(64) void sf_trace_rays_fixup(FrameArgs a, const float* origins, const float* dirs,
                                                                     uint32_t ostride, uint32_t dstride, uint32_t rpo,
                                                                     const uint32_t* overflow_list, uint32_t* counters,
                                                                     uint32_t parity)
{
    extern __shared__ float lds[];
    fixup_groups<RootStage::PerGroup, true>(a, lds, overflow_list, counters, parity,
                                            [&](uint32_t group, const float4 bcol) {
        return trace_ray_group<true>(a, origins, dirs, ostride, dstride, rpo, 1u, lds, bcol, group, SF_MAX_LEVELS,
                                     nullptr, nullptr);
    });
}

// ------------------------------------------------------------------------------------------
// The light traces: nine traces over the 8x8 tiles of a position image, one _wave and one
// _fixup kernel each. A trace is a pose -- where the ray of entry i to the lane's pixel starts and ends -- run through
// one of two entry loops (trace_parallel_entries: a ray origin per lane, traverse_mixed; trace_point_entries: one
// origin per entry, traverse_ray) and closed by one of two endings (light_mask_end, light_sum_end). The two kernel
// bodies and what they hand a group come first.
// ------------------------------------------------------------------------------------------
namespace {

// What a kernel body hands a group: the wave's LDS image, the builder column, the tile, the levels provisioned, and
// where a first pass flags the tile (null in the re-trace, which flags nothing).
template <bool FIXUP>
struct LightTile {
    float* L;
    float4 bcol;
    uint32_t group, levels;
    uint32_t* overflow_list;
    uint32_t* overflow_count;
};
using WaveTile = LightTile<false>;
using FixupTile = LightTile<true>;

// The body of a _wave kernel: one tile per one-wave workgroup; `lds` is the dynamic LDS for a.max_depth levels,
// SF_LDS_WAVE_FLOATS for the traces of trace_point_entries and SF_LDS_RAYS_FLOATS (the mixed traversal's tables and
// centre stack) for those of trace_parallel_entries. STAGE: Once where the group reads the root image and never writes
// it, InGroup where it stages what it needs itself (and a tile without a surface pixel stages nothing). Plain vector
// stores only; no statistic and none of the renders' state is touched.
template <RootStage STAGE, class GroupFn>
__device__ __forceinline__ void light_wave(const FrameArgs& a, float* lds, uint32_t groups, uint32_t* overflow_list,
                                           uint32_t* overflow_count, GroupFn group_fn)
{
    if (blockIdx.x >= groups) return;
    if constexpr (STAGE == RootStage::Once) stage_root(lds, a.root);
    group_fn(WaveTile{lds, build_column(a.consts), blockIdx.x, a.max_depth, overflow_list, overflow_count});
}

// The body of a _fixup kernel: the re-trace of the flagged tiles, for every entry, at SF_MAX_LEVELS (fixup_groups;
// sf_trace_dirs_fixup's list and counters).
template <RootStage STAGE, class GroupFn>
__device__ __forceinline__ void light_fixup(const FrameArgs& a, float* lds, const uint32_t* overflow_list,
                                            uint32_t* counters, uint32_t parity, GroupFn group_fn)
{
    fixup_groups<STAGE, false>(a, lds, overflow_list, counters, parity, [&](uint32_t group, const float4 bcol) {
        group_fn(FixupTile{lds, bcol, group, SF_MAX_LEVELS, nullptr, nullptr});
    });
}

// a pixel's float4 of a position or normal image
__device__ __forceinline__ float4 px4(const float* __restrict__ image, uint32_t px)
{
    return reinterpret_cast<const float4*>(image)[px];
}

// The lane's ray of one entry: from F to the surface point w, where there is one.
struct RayPose {
    float wx, wy, wz, Fx, Fy, Fz;
    bool ray;
};

// The entry loop of the traces whose rays have an origin per lane: suns, shafts, AO and its sum.
// A FIX MADE HERE IS MADE IN trace_suns_sum_group TOO: it keeps this loop written out (the reason is given there).
// pose(i) is the lane's RayPose of entry i (a uniform index: what the pose reads of the argument segment are scalar
// loads). Per entry d, len and bound are formed by shadow_ray and the lane's root centre is 0 - F (Sphereflake.cpp:83
// at F); an entry that leaves no lane on (no ray, or a d that is zero or not finite) is skipped and keeps its bit; else
// traverse_mixed runs in its any-hit mode, unchanged, on the axis columns staged once. Returns the word whose bit i is
// set where entry i's ray to the lane's pixel is stopped, and ORs the traversals' status into `status`.
template <bool FIXUP, class Pose>
__device__ __forceinline__ uint64_t trace_parallel_entries(const FrameArgs& a, uint32_t n, float keep,
                                                           const LightTile<FIXUP>& t, uint32_t& status, Pose pose)
{
    const DeviceConsts* __restrict__ K = a.consts;
    const uint32_t culls = a.flags & SF_FLAG_NO_OCCL_CULL;   // (the mixed traversal has no cone and no order)
    float* const cstk = t.L + SF_LDS_WAVE_FLOATS(t.levels + 1u);
    uint64_t shadowed = 0ull;
#pragma clang loop unroll(disable)
    for (uint32_t i = 0u; i < n; ++i) {
        const RayPose p = pose(i);
        float dx, dy, dz, bound;
        shadow_ray(p.wx, p.wy, p.wz, p.Fx, p.Fy, p.Fz, keep, K->lut, dx, dy, dz, bound);
        const float rx = __fsub_rn(0.0f, p.Fx), ry = __fsub_rn(0.0f, p.Fy), rz = __fsub_rn(0.0f, p.Fz);
        const bool on = p.ray && finite3(dx, dy, dz);
        if (wave_ballot(on) == 0ull) continue;   // (uniform)
        HitState h;
        h.hit = false;
        int32_t md = -1;
        uint32_t st = 0u;
        lds_fence();   // (the entry before, or the re-trace's earlier tile, has read its tables)
        traverse_mixed<true>(K, t.L, cstk, t.bcol, t.levels, dx, dy, dz, rx, ry, rz, on, h, md, st, culls, bound);
        status |= st;
        shadowed |= h.hit ? (1ull << i) : 0ull;   // (bits >= 32 are live)
    }
    return shadowed;
}

// The part of stage_root's image that depends on the light: words 0..2 the translation, word 3 its squared length
// (the columns stay). Without a branch on the lane, as stage_root_all_lanes: lane l writes word l & 3. (stage_root
// itself inside the loop over the lights had its 16 lane compares hoisted into 32 SGPRs: occupancy 7.)
__device__ __forceinline__ void stage_root_translation(float* __restrict__ Lbase, float tx, float ty, float tz)
{
    const uint32_t l = threadIdx.x & 3u;
    const float tcc = (tx * tx + ty * ty) + tz * tz;
    Lbase[l] = l == 0u ? tx : l == 1u ? ty : l == 2u ? tz : tcc;   // TraverseLds::root()
}

// The entry loop of the traces whose rays start at one point per entry (shadows and its sum): entry i is the light
// ls.l[i] (a uniform index, scalar loads from the argument segment), (wx, wy, wz) the lane's surface point. The
// context's columns are staged once per tile; per light d, len and bound are formed by shadow_ray, the root image's
// translation is restaged as 0 - l_i (as trace_ray_group does per origin) and traverse_ray runs in its shadow mode,
// unchanged. A light that leaves no lane on (one that is not finite) is skipped and keeps its bit. The result and
// `status` are trace_parallel_entries'.
template <bool FIXUP, class Lights>
__device__ __forceinline__ uint64_t trace_point_entries(const FrameArgs& a, const GroupLane& g, bool surface, float wx,
                                                        float wy, float wz, const Lights& ls, const LightTile<FIXUP>& t,
                                                        uint32_t& status)
{
    const DeviceConsts* __restrict__ K = a.consts;
    const uint32_t culls = a.flags & (SF_FLAG_NO_CONE_CULL | SF_FLAG_NO_OCCL_CULL | SF_FLAG_NO_FRONT_FIRST);
    const uint32_t n = ls.n;   // (uniform, 1..64)
    uint64_t shadowed = 0ull;
    lds_fence();
    stage_root(t.L, a.root);   // the columns, once per tile; each light restages its translation
#pragma clang loop unroll(disable)
    for (uint32_t i = 0u; i < n; ++i) {
        const float lx = ls.l[i][0], ly = ls.l[i][1], lz = ls.l[i][2];
        float dx, dy, dz, bound;
        shadow_ray(wx, wy, wz, lx, ly, lz, ls.keep, K->lut, dx, dy, dz, bound);
        const bool on = surface && finite3(dx, dy, dz);
        const uint64_t onm = wave_ballot(on);
        if (onm == 0ull) continue;   // (uniform)
        const uint32_t axl = axis_lane(onm, g.mid);
        const float ax = readlane_f(dx, axl), ay = readlane_f(dy, axl), az = readlane_f(dz, axl);
        float r[12];   // (traverse_ray reads the translation only; the columns are in the staged image)
#pragma unroll
        for (int k = 0; k < 9; ++k) r[k] = 0.0f;
        r[9] = __fsub_rn(0.0f, lx);   // (Sphereflake.cpp:83 at the light)
        r[10] = __fsub_rn(0.0f, ly);
        r[11] = __fsub_rn(0.0f, lz);
        lds_fence();
        stage_root_translation(t.L, r[9], r[10], r[11]);   // (the light before left its own)
        HitState h;
        h.hit = false;
        int32_t md = -1;
        uint32_t st = 0u;
        traverse_ray<false, false, true>(K, r, t.L, t.bcol, t.levels, on ? dx : ax, on ? dy : ay, on ? dz : az, on, h,
                                         md, st, culls, nullptr, axl, nullptr, 0u, 0u, -1, bound);
        status |= st;
        shadowed |= h.hit ? (1ull << i) : 0ull;   // (bits >= 32 are live)
    }
    return shadowed;
}

// The mask ending: bit i of mask[p] is set where entry i reaches the pixel (what the single-entry trace writes as
// 255), bits n..63 are 0. A tile flagged for any entry (uniform: more levels needed) goes onto the overflow list once
// and is re-traced for all of them. A tile row is 64 contiguous bytes: one 8-byte vector store per valid lane.
template <bool FIXUP>
__device__ __forceinline__ void light_mask_end(const FrameArgs& a, const GroupLane& g, uint32_t n, uint64_t shadowed,
                                               uint32_t status, uint64_t* __restrict__ mask, const LightTile<FIXUP>& t)
{
    if (!FIXUP && status != 0u) flag_group(t.overflow_list, t.overflow_count, t.group);
    const uint64_t all = n >= 64u ? ~0ull : (1ull << n) - 1ull;
    if (g.valid) mask[(size_t)g.y * a.W + g.x] = all & ~shadowed;
}

// The summing ending. Across the traversals a lane carries what it carries under the mask ending --
// its position, the 64-bit `shadowed` word, the surface flag; the normal N, the base and the three sums exist only
// here: colour_i (lit_i ? lam(N, i) : 0) is added per channel in index order onto the base, then one 16-byte vector
// store. lam(N, i) is the Lambert term of entry i at the lane's pixel. A tile flagged for more levels is re-traced for
// ALL of the chunk's entries, so its first pass stores nothing (the flag is uniform and known when the loop ends): an
// accumulating call would otherwise add the chunk twice. The fixup kernel reads the base, sums and stores.
template <bool FIXUP, class Sum, class Lam>
__device__ __forceinline__ void light_sum_end(const FrameArgs& a, const GroupLane& g, bool surface, uint64_t shadowed,
                                              uint32_t status, const Sum& ss, const float* __restrict__ nrm4,
                                              float* __restrict__ out, const LightTile<FIXUP>& t, Lam lam)
{
    if (!FIXUP && status != 0u) {
        flag_group(t.overflow_list, t.overflow_count, t.group);
        return;
    }
    if (!g.valid) return;   // (a partial tile: nothing outside the image)
    float4* const o = reinterpret_cast<float4*>(out) + ((size_t)g.y * a.W + g.x);
    if (!surface) {   // a miss of the frame: an accumulating call leaves it, an overwriting one zeroes it
        if (!ss.accumulate) *o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const float4 N = px4(nrm4, g.ray);   // (AO's lam ignores N: there the load is dead and the compiler drops it)
    float4 S = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (ss.accumulate) S = *o;   // (uniform)
#pragma clang loop unroll(disable)
    for (uint32_t i = 0u; i < ss.n; ++i) {
        const float k = ((shadowed >> i) & 1ull) ? 0.0f : lam(N, i);
        S.x = __fadd_rn(S.x, __fmul_rn(ss.c[i][0], k));
        S.y = __fadd_rn(S.y, __fmul_rn(ss.c[i][1], k));
        S.z = __fadd_rn(S.z, __fmul_rn(ss.c[i][2], k));
    }
    *o = S;   // (.w: the base's)
}

}  // namespace

// ------------------------------------------------------------------------------------------
// Shadows from a point light (sf_trace_shadow_to). Pixel p of a view-space position image (float4,
// as the renders write it; origin o) is a frame miss where P == (0, 0, 0) (Shaders/post_final.glsl:20): vis = 255, no
// ray. Else w = o + P, d = (w - l) + 0, len = sqrt((d.x d.x + d.y d.y) + d.z d.z), bound = len (1 - bias), every
// operation rounded on its own; the ray is the reference's ray for Normalize(d) under the root transform whose
// translation is 0 - l (sf_trace_rays_to's ray from the one origin l), and vis = (its min_t < bound) ? 0 : 255. All
// rays start at the light, so every group takes the one-origin traversal (traverse_ray) on the light's root image,
// in its shadow mode: any hit below the bound finishes a lane. One wave64 per 8x8 tile of the image (a.W x a.H,
// a.tiles_x tiles per row), the grouping of sf_trace_dirs_wave; a.root[9..11] is 0 - l.
// ------------------------------------------------------------------------------------------
namespace {

template <bool FIXUP>
__device__ __forceinline__ void trace_shadow_group(const FrameArgs& a, const float* __restrict__ pos4,
                                                   const ShadowArgs& sa, uint8_t* __restrict__ vis,
                                                   const LightTile<FIXUP>& t)
{
    const DeviceConsts* __restrict__ K = a.consts;
    const GroupLane g = tile_lane(a, t.group);
    const float4 P = px4(pos4, g.ray);
    const bool surface = !(P.x == 0.0f && P.y == 0.0f && P.z == 0.0f);
    float dx, dy, dz, bound;
    shadow_ray(__fadd_rn(sa.o[0], P.x), __fadd_rn(sa.o[1], P.y), __fadd_rn(sa.o[2], P.z), sa.l[0], sa.l[1], sa.l[2],
               sa.keep, K->lut, dx, dy, dz, bound);
    // a d that does not normalise to finite numbers misses (see trace_dir_group); a light that is not finite makes d
    // so for every pixel, and the root is not entered either (trace_ray_group)
    const bool on = g.valid && surface && finite3(dx, dy, dz);
    const uint64_t onm = wave_ballot(on);
    HitState h;
    h.hit = false;
    uint32_t status = 0u;
    if (onm != 0ull) {   // (uniform; else no ray of the group is traced)
        const uint32_t axl = axis_lane(onm, g.mid);
        const float ax = readlane_f(dx, axl), ay = readlane_f(dy, axl), az = readlane_f(dz, axl);
        const uint32_t culls = a.flags & (SF_FLAG_NO_CONE_CULL | SF_FLAG_NO_OCCL_CULL | SF_FLAG_NO_FRONT_FIRST);
        int32_t md = -1;
#ifdef SF_SHADOW_CLOSEST
        // measurement builds only: the closest-hit traversal and the comparison afterwards (no early exit, no bound
        // seed) -- what the any-hit mode is measured against
        traverse_ray<>(K, a.root, t.L, t.bcol, t.levels, on ? dx : ax, on ? dy : ay, on ? dz : az, on, h, md, status,
                       culls | (FIXUP ? SF_FLAG_NO_FRONT_FIRST : 0u), nullptr, axl);
        h.hit = on && h.minT < bound;
#else
        // (a tie never flags in the shadow mode, so the re-trace keeps the front-first order)
        traverse_ray<false, false, true>(K, a.root, t.L, t.bcol, t.levels, on ? dx : ax, on ? dy : ay, on ? dz : az,
                                         on, h, md, status, culls, nullptr, axl, nullptr, 0u, 0u, -1, bound);
#endif
    }
    // (uniform) more levels needed
    if (!FIXUP && status != 0u) flag_group(t.overflow_list, t.overflow_count, t.group);
    store_vis_tile(a, vis, g, h.hit);
}

}  // namespace

// The traversal only reads the light's root image: staged once.
extern "C" __global__ __launch_bounds__(64) void sf_trace_shadow_wave(FrameArgs a, const float* pos4, ShadowArgs sa,
                                                                      uint8_t* vis, uint32_t groups,
                                                                      uint32_t* overflow_list, uint32_t* overflow_count)
{
    extern __shared__ float lds[];
    light_wave<RootStage::Once>(a, lds, groups, overflow_list, overflow_count,
                                [&](const WaveTile& t) { trace_shadow_group(a, pos4, sa, vis, t); });
}

extern "C" __global__ __launch_bounds__(64) void sf_trace_shadow_fixup(FrameArgs a, const float* pos4, ShadowArgs sa,
                                                                       uint8_t* vis, const uint32_t* overflow_list,
                                                                       uint32_t* counters, uint32_t parity)
{
    extern __shared__ float lds[];
    light_fixup<RootStage::Once>(a, lds, overflow_list, counters, parity,
                                 [&](const FixupTile& t) { trace_shadow_group(a, pos4, sa, vis, t); });
}

// ------------------------------------------------------------------------------------------
// Many lights per pixel in one launch (sf_trace_shadows_to). Bit i of mask[p] is what
// sf_trace_shadow_wave writes for light i at p (1 = 255, 0 = 0), bits n..63 are 0. The pose is the lane's surface point
// w = o + P, formed once; the entries are the lights (trace_point_entries), the ending the mask's. A tile with no
// surface pixel traces nothing. The launch's levels are one value for all lights.
// ------------------------------------------------------------------------------------------
namespace {

template <bool FIXUP>
__device__ __forceinline__ void trace_shadows_group(const FrameArgs& a, const float* __restrict__ pos4,
                                                    const ShadowLights& sl, uint64_t* __restrict__ mask,
                                                    const LightTile<FIXUP>& t)
{
    const GroupLane g = tile_lane(a, t.group);
    const float4 P = px4(pos4, g.ray);
    const bool surface = g.valid && !(P.x == 0.0f && P.y == 0.0f && P.z == 0.0f);
    uint64_t shadowed = 0ull;   // bit i: light i does not reach the lane's pixel
    uint32_t status = 0u;
    if (wave_ballot(surface) != 0ull) {   // (uniform; else the tile is all frame miss: every light's bit is set)
        const float wx = __fadd_rn(sl.o[0], P.x), wy = __fadd_rn(sl.o[1], P.y), wz = __fadd_rn(sl.o[2], P.z);
        shadowed = trace_point_entries(a, g, surface, wx, wy, wz, sl, t, status);
    }
    light_mask_end(a, g, sl.n, shadowed, status, mask, t);
}

}  // namespace

// The group stages the columns itself, and a tile without a surface pixel stages nothing.
extern "C" __global__ __launch_bounds__(64) void sf_trace_shadows_wave(FrameArgs a, const float* pos4, ShadowLights sl,
                                                                       uint64_t* mask, uint32_t groups,
                                                                       uint32_t* overflow_list, uint32_t* overflow_count)
{
    extern __shared__ float lds[];
    light_wave<RootStage::InGroup>(a, lds, groups, overflow_list, overflow_count,
                                   [&](const WaveTile& t) { trace_shadows_group(a, pos4, sl, mask, t); });
}

extern "C" __global__ __launch_bounds__(64) void sf_trace_shadows_fixup(FrameArgs a, const float* pos4, ShadowLights sl,
                                                                        uint64_t* mask, const uint32_t* overflow_list,
                                                                        uint32_t* counters, uint32_t parity)
{
    extern __shared__ float lds[];
    light_fixup<RootStage::InGroup>(a, lds, overflow_list, counters, parity,
                                    [&](const FixupTile& t) { trace_shadows_group(a, pos4, sl, mask, t); });
}

// ------------------------------------------------------------------------------------------
// Shadows from a directional light (sf_trace_sun_to). Pixel p of a position image (as
// sf_trace_shadow_wave reads it) is a frame miss where P == (0, 0, 0): vis = 255, no ray. Else w = o + P,
// F = w + f with f = s tau (formed by the host: one product per component), d = (w - F) + 0,
// len = sqrt((d.x d.x + d.y d.y) + d.z d.z), bound = len (1 - bias), every operation rounded on its own; the ray is
// sf_trace_rays_to's ray from the origin F with direction Normalize(d), and vis = (its min_t < bound) ? 0 : 255. Every
// lane has its own origin, so the tile takes the mixed-origin traversal (traverse_mixed) in its any-hit mode: the
// context's axis columns staged once, the lane's own root centre 0 - F. One wave64 per 8x8 tile, the grouping and the
// row store of sf_trace_shadow_wave.
// ------------------------------------------------------------------------------------------
namespace {

template <bool FIXUP>
__device__ __forceinline__ void trace_sun_group(const FrameArgs& a, const float* __restrict__ pos4, const SunArgs& sa,
                                                uint8_t* __restrict__ vis, const LightTile<FIXUP>& t)
{
    const DeviceConsts* __restrict__ K = a.consts;
    const GroupLane g = tile_lane(a, t.group);
    const float4 P = px4(pos4, g.ray);
    const bool surface = !(P.x == 0.0f && P.y == 0.0f && P.z == 0.0f);
    const float wx = __fadd_rn(sa.o[0], P.x), wy = __fadd_rn(sa.o[1], P.y), wz = __fadd_rn(sa.o[2], P.z);
    const float Fx = __fadd_rn(wx, sa.f[0]), Fy = __fadd_rn(wy, sa.f[1]), Fz = __fadd_rn(wz, sa.f[2]);
    float dx, dy, dz, bound;
    shadow_ray(wx, wy, wz, Fx, Fy, Fz, sa.keep, K->lut, dx, dy, dz, bound);
    // the lane's root centre (Sphereflake.cpp:83 at F)
    const float rx = __fsub_rn(0.0f, Fx), ry = __fsub_rn(0.0f, Fy), rz = __fsub_rn(0.0f, Fz);
    // a d that does not normalise to finite numbers misses (see trace_dir_group); an F that is not finite makes d so
    const bool on = g.valid && surface && finite3(dx, dy, dz);
    HitState h;
    h.hit = false;
    uint32_t status = 0u;
    if (wave_ballot(on) != 0ull) {   // (uniform; else no ray of the group is traced)
        const uint32_t culls = a.flags & SF_FLAG_NO_OCCL_CULL;   // (the mixed traversal has no cone and no order)
        float* const cstk = t.L + SF_LDS_WAVE_FLOATS(t.levels + 1u);
        int32_t md = -1;
        lds_fence();   // (the re-trace's earlier tile has read its tables)
        traverse_mixed<true>(K, t.L, cstk, t.bcol, t.levels, dx, dy, dz, rx, ry, rz, on, h, md, status, culls, bound);
    }
    // (uniform) more levels needed
    if (!FIXUP && status != 0u) flag_group(t.overflow_list, t.overflow_count, t.group);
    store_vis_tile(a, vis, g, h.hit);
}

}  // namespace

// The mixed traversal reads the root image's columns and never writes it: staged once (as in every trace below whose
// rays have an origin per lane).
extern "C" __global__ __launch_bounds__(64) void sf_trace_sun_wave(FrameArgs a, const float* pos4, SunArgs sa,
                                                                   uint8_t* vis, uint32_t groups,
                                                                   uint32_t* overflow_list, uint32_t* overflow_count)
{
    extern __shared__ float lds[];
    light_wave<RootStage::Once>(a, lds, groups, overflow_list, overflow_count,
                                [&](const WaveTile& t) { trace_sun_group(a, pos4, sa, vis, t); });
}

extern "C" __global__ __launch_bounds__(64) void sf_trace_sun_fixup(FrameArgs a, const float* pos4, SunArgs sa,
                                                                    uint8_t* vis, const uint32_t* overflow_list,
                                                                    uint32_t* counters, uint32_t parity)
{
    extern __shared__ float lds[];
    light_fixup<RootStage::Once>(a, lds, overflow_list, counters, parity,
                                 [&](const FixupTile& t) { trace_sun_group(a, pos4, sa, vis, t); });
}

// ------------------------------------------------------------------------------------------
// Many sun directions per pixel in one launch (sf_trace_suns_to): a soft sun, a sky dome of parallel
// rays. Bit i of mask[p] is what sf_trace_sun_wave writes for direction i at p (1 = 255, 0 = 0), bits n..63 are 0. The
// pose: the lane's position is loaded and w = o + P formed once; per direction F = w + f_i, the f_i = s_i tau scalar
// loads from the argument segment (trace_sun_group's F). A tile with no surface pixel traces nothing; a direction that
// is zero or not finite leaves no lane on.
// ------------------------------------------------------------------------------------------
namespace {

template <bool FIXUP>
__device__ __forceinline__ void trace_suns_group(const FrameArgs& a, const float* __restrict__ pos4, const SunDirs& sd,
                                                 uint64_t* __restrict__ mask, const LightTile<FIXUP>& t)
{
    const GroupLane g = tile_lane(a, t.group);
    const float4 P = px4(pos4, g.ray);
    const bool surface = g.valid && !(P.x == 0.0f && P.y == 0.0f && P.z == 0.0f);
    uint64_t shadowed = 0ull;   // bit i: direction i's ray to the lane's pixel is stopped
    uint32_t status = 0u;
    if (wave_ballot(surface) != 0ull) {   // (uniform; else the tile is all frame miss: every direction's bit is set)
        const float wx = __fadd_rn(sd.o[0], P.x), wy = __fadd_rn(sd.o[1], P.y), wz = __fadd_rn(sd.o[2], P.z);
        shadowed = trace_parallel_entries(a, sd.n, sd.keep, t, status, [&](uint32_t i) {
            return RayPose{wx, wy, wz, __fadd_rn(wx, sd.f[i][0]), __fadd_rn(wy, sd.f[i][1]), __fadd_rn(wz, sd.f[i][2]),
                           surface};
        });
    }
    light_mask_end(a, g, sd.n, shadowed, status, mask, t);
}

}  // namespace

extern "C" __global__ __launch_bounds__(64) void sf_trace_suns_wave(FrameArgs a, const float* pos4, SunDirs sd,
                                                                    uint64_t* mask, uint32_t groups,
                                                                    uint32_t* overflow_list, uint32_t* overflow_count)
{
    extern __shared__ float lds[];
    light_wave<RootStage::Once>(a, lds, groups, overflow_list, overflow_count,
                                [&](const WaveTile& t) { trace_suns_group(a, pos4, sd, mask, t); });
}

extern "C" __global__ __launch_bounds__(64) void sf_trace_suns_fixup(FrameArgs a, const float* pos4, SunDirs sd,
                                                                     uint64_t* mask, const uint32_t* overflow_list,
                                                                     uint32_t* counters, uint32_t parity)
{
    extern __shared__ float lds[];
    light_fixup<RootStage::Once>(a, lds, overflow_list, counters, parity,
                                 [&](const FixupTile& t) { trace_suns_group(a, pos4, sd, mask, t); });
}

// ------------------------------------------------------------------------------------------
// The summing traces (sf_trace_suns_sum_to, sf_trace_shadows_sum_to): the entries of sf_trace_suns_to
// and sf_trace_shadows_to under the summing ending, one chunk of the call's entries per launch. The Lambert terms are
// sf_light_image_suns_px's and sf_light_image_many_px's (sf_internal.h).
// ------------------------------------------------------------------------------------------
namespace {

template <bool FIXUP>
__device__ __forceinline__ void trace_suns_sum_group(const FrameArgs& a, const float* __restrict__ pos4,
                                                     const float* __restrict__ nrm4, const SunSum& ss,
                                                     float* __restrict__ out, const LightTile<FIXUP>& t)
{
    const GroupLane g = tile_lane(a, t.group);
    const float4 P = px4(pos4, g.ray);
    const bool surface = g.valid && !(P.x == 0.0f && P.y == 0.0f && P.z == 0.0f);
    const uint32_t n = ss.n;   // (uniform, 1..64)
    uint64_t shadowed = 0ull;   // bit i: direction i's ray to the lane's pixel is stopped
    uint32_t status = 0u;
    // trace_suns_group's entries with trace_parallel_entries' loop written out.
    // A FIX MADE IN trace_parallel_entries IS MADE HERE TOO.
    // Why the copy: through the shared loop this kernel's traversal kept its instructions but got other registers and
    // ran 2.4-3.0 % slower at n = 16..256 (measured).
    if (wave_ballot(surface) != 0ull) {   // (uniform; else the tile is all frame miss)
        const DeviceConsts* __restrict__ K = a.consts;
        const float wx = __fadd_rn(ss.o[0], P.x), wy = __fadd_rn(ss.o[1], P.y), wz = __fadd_rn(ss.o[2], P.z);
        const uint32_t culls = a.flags & SF_FLAG_NO_OCCL_CULL;
        float* const cstk = t.L + SF_LDS_WAVE_FLOATS(t.levels + 1u);
#pragma clang loop unroll(disable)
        for (uint32_t i = 0u; i < n; ++i) {
            const float Fx = __fadd_rn(wx, ss.f[i][0]), Fy = __fadd_rn(wy, ss.f[i][1]), Fz = __fadd_rn(wz, ss.f[i][2]);
            float dx, dy, dz, bound;
            shadow_ray(wx, wy, wz, Fx, Fy, Fz, ss.keep, K->lut, dx, dy, dz, bound);
            const float rx = __fsub_rn(0.0f, Fx), ry = __fsub_rn(0.0f, Fy), rz = __fsub_rn(0.0f, Fz);
            const bool on = surface && finite3(dx, dy, dz);
            if (wave_ballot(on) == 0ull) continue;
            HitState h;
            h.hit = false;
            int32_t md = -1;
            uint32_t st = 0u;
            lds_fence();
            traverse_mixed<true>(K, t.L, cstk, t.bcol, t.levels, dx, dy, dz, rx, ry, rz, on, h, md, st, culls, bound);
            status |= st;
            shadowed |= h.hit ? (1ull << i) : 0ull;
        }
    }
    light_sum_end(a, g, surface, shadowed, status, ss, nrm4, out, t, [&](const float4 N, uint32_t i) {
        return sf_lambert_sun(N, ss.s[i][0], ss.s[i][1], ss.s[i][2]);
    });
}

template <bool FIXUP>
__device__ __forceinline__ void trace_shadows_sum_group(const FrameArgs& a, const float* __restrict__ pos4,
                                                        const float* __restrict__ nrm4, const ShadowSum& ss,
                                                        float* __restrict__ out, const LightTile<FIXUP>& t)
{
    const GroupLane g = tile_lane(a, t.group);
    const float4 P = px4(pos4, g.ray);
    const bool surface = g.valid && !(P.x == 0.0f && P.y == 0.0f && P.z == 0.0f);
    const float wx = __fadd_rn(ss.o[0], P.x), wy = __fadd_rn(ss.o[1], P.y), wz = __fadd_rn(ss.o[2], P.z);
    uint64_t shadowed = 0ull;   // bit i: light i does not reach the lane's pixel
    uint32_t status = 0u;
    // (uniform; else the tile is all frame miss)
    if (wave_ballot(surface) != 0ull) shadowed = trace_point_entries(a, g, surface, wx, wy, wz, ss, t, status);
    light_sum_end(a, g, surface, shadowed, status, ss, nrm4, out, t, [&](const float4 N, uint32_t i) {
        return sf_lambert_point(N, wx, wy, wz, ss.l[i][0], ss.l[i][1], ss.l[i][2]);
    });
}

}  // namespace

extern "C" __global__ __launch_bounds__(64) void sf_trace_suns_sum_wave(FrameArgs a, const float* pos4,
                                                                        const float* nrm4, SunSum ss, float* out,
                                                                        uint32_t groups, uint32_t* overflow_list,
                                                                        uint32_t* overflow_count)
{
    extern __shared__ float lds[];
    light_wave<RootStage::Once>(a, lds, groups, overflow_list, overflow_count,
                                [&](const WaveTile& t) { trace_suns_sum_group(a, pos4, nrm4, ss, out, t); });
}

extern "C" __global__ __launch_bounds__(64) void sf_trace_suns_sum_fixup(FrameArgs a, const float* pos4,
                                                                         const float* nrm4, SunSum ss, float* out,
                                                                         const uint32_t* overflow_list,
                                                                         uint32_t* counters, uint32_t parity)
{
    extern __shared__ float lds[];
    light_fixup<RootStage::Once>(a, lds, overflow_list, counters, parity,
                                 [&](const FixupTile& t) { trace_suns_sum_group(a, pos4, nrm4, ss, out, t); });
}

extern "C" __global__ __launch_bounds__(64) void sf_trace_shadows_sum_wave(FrameArgs a, const float* pos4,
                                                                           const float* nrm4, ShadowSum ss, float* out,
                                                                           uint32_t groups, uint32_t* overflow_list,
                                                                           uint32_t* overflow_count)
{
    extern __shared__ float lds[];
    light_wave<RootStage::InGroup>(a, lds, groups, overflow_list, overflow_count,
                                   [&](const WaveTile& t) { trace_shadows_sum_group(a, pos4, nrm4, ss, out, t); });
}

extern "C" __global__ __launch_bounds__(64) void sf_trace_shadows_sum_fixup(FrameArgs a, const float* pos4,
                                                                            const float* nrm4, ShadowSum ss, float* out,
                                                                            const uint32_t* overflow_list,
                                                                            uint32_t* counters, uint32_t parity)
{
    extern __shared__ float lds[];
    light_fixup<RootStage::InGroup>(a, lds, overflow_list, counters, parity,
                                    [&](const FixupTile& t) { trace_shadows_sum_group(a, pos4, nrm4, ss, out, t); });
}

// ------------------------------------------------------------------------------------------
// Ambient occlusion about each pixel's normal in one launch (sf_trace_ao_to / sf_trace_ao_sum_to).
// trace_suns_group with a direction that depends on the lane. The pose: the lane's position AND normal are loaded
// once, and w = o + P and the frame (T, B) about N (the branch-free frame of Duff et al.: one division per pixel) are
// formed once; per sample (a uniform index, the local-frame samples h_i are scalar loads from the argument segment)
// s_i = ((T h.x) + (B h.y)) + (N h.z), f_i = s_i tau and F = w + f_i. Every operation is its own rounding (sf.h), so
// a constant normal image gives trace_suns_group's bits for the directions s_i. A tile with no surface pixel traces
// nothing.
// ------------------------------------------------------------------------------------------
namespace {

// The lane's frame about N: T and B of sf.h's step 2, in the order written there.
__device__ __forceinline__ void ao_frame(const float4 N, float T[3], float B[3])
{
    const float sg = __builtin_copysignf(1.0f, N.z);
    const float a = __fdiv_rn(-1.0f, __fadd_rn(sg, N.z));   // (sg + N.z is +-(1 + |N.z|): never zero)
    const float b = __fmul_rn(__fmul_rn(N.x, N.y), a);
    T[0] = __fadd_rn(1.0f, __fmul_rn(sg, __fmul_rn(__fmul_rn(N.x, N.x), a)));
    T[1] = __fmul_rn(sg, b);
    T[2] = -__fmul_rn(sg, N.x);
    B[0] = b;
    B[1] = __fadd_rn(sg, __fmul_rn(__fmul_rn(N.y, N.y), a));
    B[2] = -N.y;
}

// The entries of sf_trace_ao_to and sf_trace_ao_sum_to: AO is AoArgs or AoSum (o, keep, tau, n, h).
template <bool FIXUP, class AO>
__device__ __forceinline__ uint64_t trace_ao_entries(const FrameArgs& a, const float4 P, const float4 N, bool surface,
                                                     const AO& ao, const LightTile<FIXUP>& t, uint32_t& status)
{
    const float wx = __fadd_rn(ao.o[0], P.x), wy = __fadd_rn(ao.o[1], P.y), wz = __fadd_rn(ao.o[2], P.z);
    float T[3], B[3];
    ao_frame(N, T, B);
    // (finiteness depends on the sample and the lane's normal: a NaN, infinite or zero one leaves the lane off)
    return trace_parallel_entries(a, ao.n, ao.keep, t, status, [&](uint32_t i) {
        const float hx = ao.h[i][0], hy = ao.h[i][1], hz = ao.h[i][2];
        const float sx = __fadd_rn(__fadd_rn(__fmul_rn(T[0], hx), __fmul_rn(B[0], hy)), __fmul_rn(N.x, hz));
        const float sy = __fadd_rn(__fadd_rn(__fmul_rn(T[1], hx), __fmul_rn(B[1], hy)), __fmul_rn(N.y, hz));
        const float sz = __fadd_rn(__fadd_rn(__fmul_rn(T[2], hx), __fmul_rn(B[2], hy)), __fmul_rn(N.z, hz));
        return RayPose{wx, wy, wz, __fadd_rn(wx, __fmul_rn(sx, ao.tau)), __fadd_rn(wy, __fmul_rn(sy, ao.tau)),
                       __fadd_rn(wz, __fmul_rn(sz, ao.tau)), surface};
    });
}

template <bool FIXUP>
__device__ __forceinline__ void trace_ao_group(const FrameArgs& a, const float* __restrict__ pos4,
                                               const float* __restrict__ nrm4, const AoArgs& ao,
                                               uint64_t* __restrict__ mask, const LightTile<FIXUP>& t)
{
    const GroupLane g = tile_lane(a, t.group);
    const float4 P = px4(pos4, g.ray);
    const bool surface = g.valid && !(P.x == 0.0f && P.y == 0.0f && P.z == 0.0f);
    uint64_t shadowed = 0ull;   // bit i: sample i's ray to the lane's pixel is stopped
    uint32_t status = 0u;
    // (uniform; else the tile is all frame miss: every sample's bit is set. g.ray is clamped into the image)
    if (wave_ballot(surface) != 0ull) shadowed = trace_ao_entries(a, P, px4(nrm4, g.ray), surface, ao, t, status);
    light_mask_end(a, g, ao.n, shadowed, status, mask, t);
}

// The summing ending with lam == 1: the weighting lives in the sample set and the colours.
template <bool FIXUP>
__device__ __forceinline__ void trace_ao_sum_group(const FrameArgs& a, const float* __restrict__ pos4,
                                                   const float* __restrict__ nrm4, const AoSum& ao,
                                                   float* __restrict__ out, const LightTile<FIXUP>& t)
{
    const GroupLane g = tile_lane(a, t.group);
    const float4 P = px4(pos4, g.ray);
    const bool surface = g.valid && !(P.x == 0.0f && P.y == 0.0f && P.z == 0.0f);
    uint64_t shadowed = 0ull;
    uint32_t status = 0u;
    // (uniform; else the tile is all frame miss)
    if (wave_ballot(surface) != 0ull) shadowed = trace_ao_entries(a, P, px4(nrm4, g.ray), surface, ao, t, status);
    light_sum_end(a, g, surface, shadowed, status, ao, nrm4, out, t, [](const float4, uint32_t) { return 1.0f; });
}

}  // namespace

extern "C" __global__ __launch_bounds__(64) void sf_trace_ao_wave(FrameArgs a, const float* pos4, const float* nrm4,
                                                                  AoArgs ao, uint64_t* mask, uint32_t groups,
                                                                  uint32_t* overflow_list, uint32_t* overflow_count)
{
    extern __shared__ float lds[];
    light_wave<RootStage::Once>(a, lds, groups, overflow_list, overflow_count,
                                [&](const WaveTile& t) { trace_ao_group(a, pos4, nrm4, ao, mask, t); });
}

extern "C" __global__ __launch_bounds__(64) void sf_trace_ao_fixup(FrameArgs a, const float* pos4, const float* nrm4,
                                                                   AoArgs ao, uint64_t* mask,
                                                                   const uint32_t* overflow_list, uint32_t* counters,
                                                                   uint32_t parity)
{
    extern __shared__ float lds[];
    light_fixup<RootStage::Once>(a, lds, overflow_list, counters, parity,
                                 [&](const FixupTile& t) { trace_ao_group(a, pos4, nrm4, ao, mask, t); });
}

extern "C" __global__ __launch_bounds__(64) void sf_trace_ao_sum_wave(FrameArgs a, const float* pos4,
                                                                      const float* nrm4, AoSum ao, float* out,
                                                                      uint32_t groups, uint32_t* overflow_list,
                                                                      uint32_t* overflow_count)
{
    extern __shared__ float lds[];
    light_wave<RootStage::Once>(a, lds, groups, overflow_list, overflow_count,
                                [&](const WaveTile& t) { trace_ao_sum_group(a, pos4, nrm4, ao, out, t); });
}

extern "C" __global__ __launch_bounds__(64) void sf_trace_ao_sum_fixup(FrameArgs a, const float* pos4,
                                                                       const float* nrm4, AoSum ao, float* out,
                                                                       const uint32_t* overflow_list,
                                                                       uint32_t* counters, uint32_t parity)
{
    extern __shared__ float lds[];
    light_fixup<RootStage::Once>(a, lds, overflow_list, counters, parity,
                                 [&](const FixupTile& t) { trace_ao_sum_group(a, pos4, nrm4, ao, out, t); });
}

// ------------------------------------------------------------------------------------------
// Ambient occlusion with a per-pixel spin (sf_trace_ao_spin_to / sf_trace_ao_spin_sum_to): the four
// kernels above with each lane's frame turned about its normal by its pixel's own (c, s), once per tile, before the
// sample loop: T' = (T c) + (B s), B' = (B c) - (T s) (sf.h). The lane reads its entry of the table in the argument
// segment at (g.y % size) * size + (g.x % size): a vector load, since the index is the lane's. The sample loop, the
// endings and the re-trace are the unspun kernels'. trace_ao_entries is not touched and not shared: a traversal's call
// site decides its registers and its time (§6.18), so the spun pose is a function of its own.
// ------------------------------------------------------------------------------------------
namespace {

// The entries of the spun calls: ao_frame, the turn, then trace_ao_entries' pose with T' and B'.
template <bool FIXUP, class AO>
__device__ __forceinline__ uint64_t trace_ao_spin_entries(const FrameArgs& a, const GroupLane& g, const float4 P,
                                                          const float4 N, bool surface, const AO& ao,
                                                          const AoSpin& sp, const LightTile<FIXUP>& t,
                                                          uint32_t& status)
{
    const float wx = __fadd_rn(ao.o[0], P.x), wy = __fadd_rn(ao.o[1], P.y), wz = __fadd_rn(ao.o[2], P.z);
    float T0[3], B0[3], T[3], B[3];
    ao_frame(N, T0, B0);
    const uint32_t e = (g.y % sp.size) * sp.size + (g.x % sp.size);   // (< size^2 <= 64 for any pixel)
    const float c = sp.cs[e][0], s = sp.cs[e][1];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        T[k] = __fadd_rn(__fmul_rn(T0[k], c), __fmul_rn(B0[k], s));
        B[k] = __fsub_rn(__fmul_rn(B0[k], c), __fmul_rn(T0[k], s));
    }
    return trace_parallel_entries(a, ao.n, ao.keep, t, status, [&](uint32_t i) {
        const float hx = ao.h[i][0], hy = ao.h[i][1], hz = ao.h[i][2];
        const float sx = __fadd_rn(__fadd_rn(__fmul_rn(T[0], hx), __fmul_rn(B[0], hy)), __fmul_rn(N.x, hz));
        const float sy = __fadd_rn(__fadd_rn(__fmul_rn(T[1], hx), __fmul_rn(B[1], hy)), __fmul_rn(N.y, hz));
        const float sz = __fadd_rn(__fadd_rn(__fmul_rn(T[2], hx), __fmul_rn(B[2], hy)), __fmul_rn(N.z, hz));
        return RayPose{wx, wy, wz, __fadd_rn(wx, __fmul_rn(sx, ao.tau)), __fadd_rn(wy, __fmul_rn(sy, ao.tau)),
                       __fadd_rn(wz, __fmul_rn(sz, ao.tau)), surface};
    });
}

template <bool FIXUP>
__device__ __forceinline__ void trace_ao_spin_group(const FrameArgs& a, const float* __restrict__ pos4,
                                                    const float* __restrict__ nrm4, const AoArgs& ao,
                                                    const AoSpin& sp, uint64_t* __restrict__ mask,
                                                    const LightTile<FIXUP>& t)
{
    const GroupLane g = tile_lane(a, t.group);
    const float4 P = px4(pos4, g.ray);
    const bool surface = g.valid && !(P.x == 0.0f && P.y == 0.0f && P.z == 0.0f);
    uint64_t shadowed = 0ull;
    uint32_t status = 0u;
    // (uniform; else the tile is all frame miss)
    if (wave_ballot(surface) != 0ull)
        shadowed = trace_ao_spin_entries(a, g, P, px4(nrm4, g.ray), surface, ao, sp, t, status);
    light_mask_end(a, g, ao.n, shadowed, status, mask, t);
}

template <bool FIXUP>
__device__ __forceinline__ void trace_ao_spin_sum_group(const FrameArgs& a, const float* __restrict__ pos4,
                                                        const float* __restrict__ nrm4, const AoSum& ao,
                                                        const AoSpin& sp, float* __restrict__ out,
                                                        const LightTile<FIXUP>& t)
{
    const GroupLane g = tile_lane(a, t.group);
    const float4 P = px4(pos4, g.ray);
    const bool surface = g.valid && !(P.x == 0.0f && P.y == 0.0f && P.z == 0.0f);
    uint64_t shadowed = 0ull;
    uint32_t status = 0u;
    // (uniform; else the tile is all frame miss)
    if (wave_ballot(surface) != 0ull)
        shadowed = trace_ao_spin_entries(a, g, P, px4(nrm4, g.ray), surface, ao, sp, t, status);
    light_sum_end(a, g, surface, shadowed, status, ao, nrm4, out, t, [](const float4, uint32_t) { return 1.0f; });
}

}  // namespace

extern "C" __global__ __launch_bounds__(64) void sf_trace_ao_spin_wave(FrameArgs a, const float* pos4,
                                                                       const float* nrm4, AoArgs ao, AoSpin sp,
                                                                       uint64_t* mask, uint32_t groups,
                                                                       uint32_t* overflow_list,
                                                                       uint32_t* overflow_count)
{
    extern __shared__ float lds[];
    light_wave<RootStage::Once>(a, lds, groups, overflow_list, overflow_count,
                                [&](const WaveTile& t) { trace_ao_spin_group(a, pos4, nrm4, ao, sp, mask, t); });
}

extern "C" __global__ __launch_bounds__(64) void sf_trace_ao_spin_fixup(FrameArgs a, const float* pos4,
                                                                        const float* nrm4, AoArgs ao, AoSpin sp,
                                                                        uint64_t* mask, const uint32_t* overflow_list,
                                                                        uint32_t* counters, uint32_t parity)
{
    extern __shared__ float lds[];
    light_fixup<RootStage::Once>(a, lds, overflow_list, counters, parity,
                                 [&](const FixupTile& t) { trace_ao_spin_group(a, pos4, nrm4, ao, sp, mask, t); });
}

extern "C" __global__ __launch_bounds__(64) void sf_trace_ao_spin_sum_wave(FrameArgs a, const float* pos4,
                                                                           const float* nrm4, AoSum ao, AoSpin sp,
                                                                           float* out, uint32_t groups,
                                                                           uint32_t* overflow_list,
                                                                           uint32_t* overflow_count)
{
    extern __shared__ float lds[];
    light_wave<RootStage::Once>(a, lds, groups, overflow_list, overflow_count,
                                [&](const WaveTile& t) { trace_ao_spin_sum_group(a, pos4, nrm4, ao, sp, out, t); });
}

extern "C" __global__ __launch_bounds__(64) void sf_trace_ao_spin_sum_fixup(FrameArgs a, const float* pos4,
                                                                            const float* nrm4, AoSum ao, AoSpin sp,
                                                                            float* out, const uint32_t* overflow_list,
                                                                            uint32_t* counters, uint32_t parity)
{
    extern __shared__ float lds[];
    light_fixup<RootStage::Once>(a, lds, overflow_list, counters, parity,
                                 [&](const FixupTile& t) { trace_ao_spin_sum_group(a, pos4, nrm4, ao, sp, out, t); });
}

// ------------------------------------------------------------------------------------------
// Sky reflections: a lobe of rays about each pixel's mirror direction (sf_trace_mirror_to / sf_trace_mirror_sum_to,
// DESIGN.md §6.21). The spun AO kernels with another axis: the lane forms the mirror direction A of its view vector
// about its normal (sf.h's steps 2 and 3: one square root and three divisions per pixel), then the frame about A and
// the turn by its table entry, once per tile; the sample loop is trace_ao_entries' with A where N was. Across the
// traversals the lane keeps w, T, B and A -- what the spun AO lane keeps with N -- and N is dead once A is formed. The
// unspun call travels as the 1 x 1 table {(1, 0)}: bit-identical (sf.h), one kernel set. The mask ending is the
// shared one; the summing ending is new: entry i's factor is the sky's RGB colour in the direction s_i of the lane's
// own ray, formed from the SAME T, B and A the pose keeps, through the same device function (mirror_dir) -- the same
// bits. (Forming the frame a second time from P and N for the ending was tried first: the compiler then kept P, N and
// both frames live, 63 / 71 VGPRs and occupancy 7 in the fixup kernel; kept once it is 51 / 60 and occupancy 8.)
// The pose is a function of its own, as trace_ao_spin_entries is (§6.18).
// ------------------------------------------------------------------------------------------
namespace {

// What a lane keeps across the traversals: w = o + P and the turned frame (T, B, A) about its mirror axis.
struct MirrorPose {
    float w[3], T[3], B[3];
    float4 A;
};

// The pose of sf.h's steps 2-4: the mirror axis, ao_frame about it, the turn. MR is MirrorArgs or MirrorSum.
template <class MR>
__device__ __forceinline__ MirrorPose mirror_pose(const GroupLane& g, const float4 P, const float4 N, const MR& mr,
                                                  const AoSpin& sp)
{
    MirrorPose m;
    m.w[0] = __fadd_rn(mr.o[0], P.x);
    m.w[1] = __fadd_rn(mr.o[1], P.y);
    m.w[2] = __fadd_rn(mr.o[2], P.z);
    // V: the position as given (relative to the viewer), or the world point less the eye -- other roundings
    const float vx = mr.use_eye ? __fsub_rn(m.w[0], mr.eye[0]) : P.x;   // (uniform)
    const float vy = mr.use_eye ? __fsub_rn(m.w[1], mr.eye[1]) : P.y;
    const float vz = mr.use_eye ? __fsub_rn(m.w[2], mr.eye[2]) : P.z;
    const float nv = __fadd_rn(__fadd_rn(__fmul_rn(N.x, vx), __fmul_rn(N.y, vy)), __fmul_rn(N.z, vz));
    const float k = __fadd_rn(nv, nv);
    const float rx = __fsub_rn(vx, __fmul_rn(k, N.x));
    const float ry = __fsub_rn(vy, __fmul_rn(k, N.y));
    const float rz = __fsub_rn(vz, __fmul_rn(k, N.z));
    // (__builtin_sqrtf: the correctly rounded square root, as in shadow_ray)
    const float len = __builtin_sqrtf(__fadd_rn(__fadd_rn(__fmul_rn(rx, rx), __fmul_rn(ry, ry)), __fmul_rn(rz, rz)));
    m.A = make_float4(__fdiv_rn(rx, len), __fdiv_rn(ry, len), __fdiv_rn(rz, len), 0.0f);
    float T0[3], B0[3];
    ao_frame(m.A, T0, B0);
    const uint32_t e = (g.y % sp.size) * sp.size + (g.x % sp.size);   // (< size^2 <= 64 for any pixel)
    const float c = sp.cs[e][0], s = sp.cs[e][1];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        m.T[q] = __fadd_rn(__fmul_rn(T0[q], c), __fmul_rn(B0[q], s));
        m.B[q] = __fsub_rn(__fmul_rn(B0[q], c), __fmul_rn(T0[q], s));
    }
    return m;
}

// s_i of step 3 of sf_trace_ao_to's definition about A.
__device__ __forceinline__ void mirror_dir(const MirrorPose& m, float hx, float hy, float hz, float& sx, float& sy,
                                           float& sz)
{
    sx = __fadd_rn(__fadd_rn(__fmul_rn(m.T[0], hx), __fmul_rn(m.B[0], hy)), __fmul_rn(m.A.x, hz));
    sy = __fadd_rn(__fadd_rn(__fmul_rn(m.T[1], hx), __fmul_rn(m.B[1], hy)), __fmul_rn(m.A.y, hz));
    sz = __fadd_rn(__fadd_rn(__fmul_rn(m.T[2], hx), __fmul_rn(m.B[2], hy)), __fmul_rn(m.A.z, hz));
}

// The entries of the mirror calls: trace_ao_entries' sample loop on the pose.
template <bool FIXUP, class MR>
__device__ __forceinline__ uint64_t trace_mirror_entries(const FrameArgs& a, bool surface, const MR& mr,
                                                         const MirrorPose& m, const LightTile<FIXUP>& t,
                                                         uint32_t& status)
{
    // (a NaN normal or a zero-length R makes A, every s_i and every F not finite: the lane stays off)
    return trace_parallel_entries(a, mr.n, mr.keep, t, status, [&](uint32_t i) {
        float sx, sy, sz;
        mirror_dir(m, mr.h[i][0], mr.h[i][1], mr.h[i][2], sx, sy, sz);
        return RayPose{m.w[0], m.w[1], m.w[2], __fadd_rn(m.w[0], __fmul_rn(sx, mr.tau)),
                       __fadd_rn(m.w[1], __fmul_rn(sy, mr.tau)), __fadd_rn(m.w[2], __fmul_rn(sz, mr.tau)), surface};
    });
}

// The summing ending with an RGB factor per entry: light_sum_end's steps (the flagged tile that stores nothing, the
// miss of the frame, the base, the index order, .w), with S.c = S.c + (colours[i].c (open_i ? E.c : 0)) where fac(i, E)
// gives entry i's factor at the lane's pixel.
template <bool FIXUP, class Sum, class Fac>
__device__ __forceinline__ void light_sum_rgb_end(const FrameArgs& a, const GroupLane& g, bool surface,
                                                  uint64_t shadowed, uint32_t status, const Sum& ss,
                                                  float* __restrict__ out, const LightTile<FIXUP>& t, Fac fac)
{
    if (!FIXUP && status != 0u) {
        flag_group(t.overflow_list, t.overflow_count, t.group);
        return;
    }
    if (!g.valid) return;   // (a partial tile: nothing outside the image)
    float4* const o = reinterpret_cast<float4*>(out) + ((size_t)g.y * a.W + g.x);
    if (!surface) {   // a miss of the frame: an accumulating call leaves it, an overwriting one zeroes it
        if (!ss.accumulate) *o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    float4 S = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (ss.accumulate) S = *o;   // (uniform)
#pragma clang loop unroll(disable)
    for (uint32_t i = 0u; i < ss.n; ++i) {
        float E[3];
        fac(i, E);
        const bool open = ((shadowed >> i) & 1ull) == 0ull;
        S.x = __fadd_rn(S.x, __fmul_rn(ss.c[i][0], open ? E[0] : 0.0f));
        S.y = __fadd_rn(S.y, __fmul_rn(ss.c[i][1], open ? E[1] : 0.0f));
        S.z = __fadd_rn(S.z, __fmul_rn(ss.c[i][2], open ? E[2] : 0.0f));
    }
    *o = S;   // (.w: the base's)
}

template <bool FIXUP>
__device__ __forceinline__ void trace_mirror_group(const FrameArgs& a, const float* __restrict__ pos4,
                                                   const float* __restrict__ nrm4, const MirrorArgs& mr,
                                                   const AoSpin& sp, uint64_t* __restrict__ mask,
                                                   const LightTile<FIXUP>& t)
{
    const GroupLane g = tile_lane(a, t.group);
    const float4 P = px4(pos4, g.ray);
    const bool surface = g.valid && !(P.x == 0.0f && P.y == 0.0f && P.z == 0.0f);
    uint64_t shadowed = 0ull;   // bit i: sample i's ray to the lane's pixel is stopped
    uint32_t status = 0u;
    // (uniform; else the tile is all frame miss: every sample's bit is set)
    if (wave_ballot(surface) != 0ull) {
        const MirrorPose m = mirror_pose(g, P, px4(nrm4, g.ray), mr, sp);
        shadowed = trace_mirror_entries(a, surface, mr, m, t, status);
    }
    light_mask_end(a, g, mr.n, shadowed, status, mask, t);
}

// The sky's colour along s_i: t = min(max(s_i . up, 0), 1), +0 where the product is -0 or NaN;
// E = horizon + (span t), span = zenith - horizon formed by the host (one rounding).
template <bool FIXUP>
__device__ __forceinline__ void trace_mirror_sum_group(const FrameArgs& a, const float* __restrict__ pos4,
                                                       const float* __restrict__ nrm4, const MirrorSum& mr,
                                                       const AoSpin& sp, float* __restrict__ out,
                                                       const LightTile<FIXUP>& t)
{
    const GroupLane g = tile_lane(a, t.group);
    const float4 P = px4(pos4, g.ray);
    const bool surface = g.valid && !(P.x == 0.0f && P.y == 0.0f && P.z == 0.0f);
    uint64_t shadowed = 0ull;
    uint32_t status = 0u;
    MirrorPose m = {};
    if (wave_ballot(surface) != 0ull) {   // (uniform; else the tile is all frame miss)
        m = mirror_pose(g, P, px4(nrm4, g.ray), mr, sp);
        shadowed = trace_mirror_entries(a, surface, mr, m, t, status);
    }
    light_sum_rgb_end(a, g, surface, shadowed, status, mr, out, t, [&](uint32_t i, float E[3]) {
        float sx, sy, sz;
        mirror_dir(m, mr.h[i][0], mr.h[i][1], mr.h[i][2], sx, sy, sz);
        const float u = __fadd_rn(__fadd_rn(__fmul_rn(sx, mr.up[0]), __fmul_rn(sy, mr.up[1])), __fmul_rn(sz, mr.up[2]));
        const float tt = u > 0.0f ? (u < 1.0f ? u : 1.0f) : 0.0f;   // (a NaN fails the compare)
#pragma unroll
        for (int q = 0; q < 3; ++q) E[q] = __fadd_rn(mr.horizon[q], __fmul_rn(mr.span[q], tt));
    });
}

}  // namespace

extern "C" __global__ __launch_bounds__(64) void sf_trace_mirror_wave(FrameArgs a, const float* pos4,
                                                                      const float* nrm4, MirrorArgs mr, AoSpin sp,
                                                                      uint64_t* mask, uint32_t groups,
                                                                      uint32_t* overflow_list,
                                                                      uint32_t* overflow_count)
{
    extern __shared__ float lds[];
    light_wave<RootStage::Once>(a, lds, groups, overflow_list, overflow_count,
                                [&](const WaveTile& t) { trace_mirror_group(a, pos4, nrm4, mr, sp, mask, t); });
}

extern "C" __global__ __launch_bounds__(64) void sf_trace_mirror_fixup(FrameArgs a, const float* pos4,
                                                                       const float* nrm4, MirrorArgs mr, AoSpin sp,
                                                                       uint64_t* mask, const uint32_t* overflow_list,
                                                                       uint32_t* counters, uint32_t parity)
{
    extern __shared__ float lds[];
    light_fixup<RootStage::Once>(a, lds, overflow_list, counters, parity,
                                 [&](const FixupTile& t) { trace_mirror_group(a, pos4, nrm4, mr, sp, mask, t); });
}

extern "C" __global__ __launch_bounds__(64) void sf_trace_mirror_sum_wave(FrameArgs a, const float* pos4,
                                                                          const float* nrm4, MirrorSum mr, AoSpin sp,
                                                                          float* out, uint32_t groups,
                                                                          uint32_t* overflow_list,
                                                                          uint32_t* overflow_count)
{
    extern __shared__ float lds[];
    light_wave<RootStage::Once>(a, lds, groups, overflow_list, overflow_count,
                                [&](const WaveTile& t) { trace_mirror_sum_group(a, pos4, nrm4, mr, sp, out, t); });
}

extern "C" __global__ __launch_bounds__(64) void sf_trace_mirror_sum_fixup(FrameArgs a, const float* pos4,
                                                                           const float* nrm4, MirrorSum mr, AoSpin sp,
                                                                           float* out, const uint32_t* overflow_list,
                                                                           uint32_t* counters, uint32_t parity)
{
    extern __shared__ float lds[];
    light_fixup<RootStage::Once>(a, lds, overflow_list, counters, parity,
                                 [&](const FixupTile& t) { trace_mirror_sum_group(a, pos4, nrm4, mr, sp, out, t); });
}

// ------------------------------------------------------------------------------------------
// Light shafts: sun visibility along each pixel's view ray in one launch (sf_trace_shafts_to). Bit i
// of mask[p] is what sf_trace_sun_wave writes at a pixel whose position is Q_i = E sigma_i (1 = 255, 0 = 0), bits
// n..63 are 0. The lane's position is loaded and its march end E formed once -- P, or where P == 0 and a direction
// image was given, dirs[p] far (loaded in those lanes only). The pose, per sample (a uniform index, the sigma_i are
// scalar loads from the argument segment): Q_i, w = o + Q_i and F = w + f -- all of them per sample: d is nearly -f
// every time, but its roundings follow w. A tile whose E are all zero traces nothing; a sample that leaves no lane on
// (a zero or non-finite sun, products that all underflow) is skipped and keeps its bit.
// ------------------------------------------------------------------------------------------
namespace {

template <bool FIXUP>
__device__ __forceinline__ void trace_shafts_group(const FrameArgs& a, const float* __restrict__ pos4,
                                                   const ShaftArgs& sh, uint64_t* __restrict__ mask,
                                                   const LightTile<FIXUP>& t)
{
    const GroupLane g = tile_lane(a, t.group);
    const float4 P = px4(pos4, g.ray);
    float Ex = P.x, Ey = P.y, Ez = P.z;
    if (sh.dirs != nullptr && P.x == 0.0f && P.y == 0.0f && P.z == 0.0f) {   // a miss of the frame: marched to far
        const float* __restrict__ dp = sh.dirs + (size_t)g.ray * sh.dirs_stride;
        Ex = __fmul_rn(dp[0], sh.far);
        Ey = __fmul_rn(dp[1], sh.far);
        Ez = __fmul_rn(dp[2], sh.far);
    }
    const bool marched = g.valid && !(Ex == 0.0f && Ey == 0.0f && Ez == 0.0f);
    uint64_t shadowed = 0ull;   // bit i: the sun's ray to the lane's sample i is stopped
    uint32_t status = 0u;
    if (wave_ballot(marched) != 0ull) {   // (uniform; else no pixel of the tile is marched: every sample's bit is set)
        shadowed = trace_parallel_entries(a, sh.n, sh.keep, t, status, [&](uint32_t i) {
            const float sg = sh.sigma[i];
            const float Qx = __fmul_rn(Ex, sg), Qy = __fmul_rn(Ey, sg), Qz = __fmul_rn(Ez, sg);
            const float wx = __fadd_rn(sh.o[0], Qx), wy = __fadd_rn(sh.o[1], Qy), wz = __fadd_rn(sh.o[2], Qz);
            // (a sample at 0 is a frame miss to sf_trace_sun_to: no ray)
            return RayPose{wx, wy, wz, __fadd_rn(wx, sh.f[0]), __fadd_rn(wy, sh.f[1]), __fadd_rn(wz, sh.f[2]),
                           marched && !(Qx == 0.0f && Qy == 0.0f && Qz == 0.0f)};
        });
    }
    light_mask_end(a, g, sh.n, shadowed, status, mask, t);
}

}  // namespace

extern "C" __global__ __launch_bounds__(64) void sf_trace_shafts_wave(FrameArgs a, const float* pos4, ShaftArgs sh,
                                                                      uint64_t* mask, uint32_t groups,
                                                                      uint32_t* overflow_list,
                                                                      uint32_t* overflow_count)
{
    extern __shared__ float lds[];
    light_wave<RootStage::Once>(a, lds, groups, overflow_list, overflow_count,
                                [&](const WaveTile& t) { trace_shafts_group(a, pos4, sh, mask, t); });
}

extern "C" __global__ __launch_bounds__(64) void sf_trace_shafts_fixup(FrameArgs a, const float* pos4, ShaftArgs sh,
                                                                       uint64_t* mask, const uint32_t* overflow_list,
                                                                       uint32_t* counters, uint32_t parity)
{
    extern __shared__ float lds[];
    light_fixup<RootStage::Once>(a, lds, overflow_list, counters, parity,
                                 [&](const FixupTile& t) { trace_shafts_group(a, pos4, sh, mask, t); });
}

// ------------------------------------------------------------------------------------------
// One thread per ray, private stack (Sphereflake.h:86-226 restated as an explicit DFS).
// ------------------------------------------------------------------------------------------
extern "C" __global__ __launch_bounds__(256) void sf_trace_ray(FrameArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t tile = blockIdx.x * SF_WAVES_PER_BLOCK + (threadIdx.x >> 6);
    if (tile >= a.tiles_x * a.tile_rows) return;
    const DeviceConsts* __restrict__ K = a.consts;
    const uint32_t* __restrict__ lut = K->lut;
    const Tile t = tile_of(a, tile, lane);
    float dx, dy, dz;
    ray_dir(a, (float)t.x, (float)t.y, dx, dy, dz, lut);

    float xf[SF_MAX_LEVELS + 1][12];
    uint8_t cur[SF_MAX_LEVELS + 1];
#pragma unroll
    for (int k = 0; k < 12; ++k) xf[0][k] = a.root[k];

    HitState h;
    h.minT = FLT_MAX;
    h.cx = h.cy = h.cz = 0.f;
    h.index = 0xffffffffu;
    h.hit = false;
    int32_t maxd = -1;
    bool overflowed = false;

    auto make_child = [&](uint32_t p, uint32_t i) { child_frame(K, p, i, xf[p], xf[p + 1]); };

    if (t.valid) {
        uint32_t d = 0;
        uint64_t idx = 0;
        for (;;) {
            bool ex = false;
            {
                const float cx = xf[d][9], cy = xf[d][10], cz = xf[d][11];
                const float tca = (cx * dx + cy * dy) + cz * dz;
                const float d2 = ((cx * cx + cy * cy) + cz * cz) - tca * tca;
                const float R2b = K->dt.r2_bound[d];
                if (tca >= 0.0f && d2 <= R2b) ex = near_root(tca, d2, R2b) < K->dt.lod[d];
            }
            if (ex) {
                maxd = (int32_t)d > maxd ? (int32_t)d : maxd;
                if (d < SF_MAX_LEVELS) {
                    cur[d] = 0;
                    make_child(d, 0);
                    d += 1;
                    idx = 9u * idx + 1u;
                    continue;
                }
                overflowed = true;
            }
            bool finished = false;
            for (;;) {
                if (d == 0) { finished = true; break; }
                const uint32_t p = d - 1;
                if (cur[p] < 8) {
                    cur[p] += 1;
                    make_child(p, cur[p]);
                    idx += 1u;
                    break;
                }
                idx = (idx - 9u) / 9u;
                d = p;
                const float cx = xf[p][9], cy = xf[p][10], cz = xf[p][11];
                const float tca = (cx * dx + cy * dy) + cz * dz;
                const float d2 = ((cx * cx + cy * cy) + cz * cz) - tca * tca;
                const float R2s = K->dt.r2_self[p];
                if (tca >= 0.0f && d2 <= R2s) {
                    const float ts = near_root(tca, d2, R2s);
                    if (ts < h.minT) {
                        h.minT = ts;
                        h.cx = cx;
                        h.cy = cy;
                        h.cz = cz;
                        h.index = (uint32_t)idx;
                        h.hit = true;
                    }
                }
            }
            if (finished) break;
        }
        write_pixel(a, t, dx, dy, dz, h, lut);
    }
    // wave-level stats
    float closest = wave_min(t.valid ? h.minT : FLT_MAX);
    int32_t md = maxd;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) md = max(md, __shfl_xor(md, m, 64));
    const bool anyov = wave_ballot(overflowed) != 0;
    if (lane == 0u) {
        if (md >= 0) atomicMax(&a.stats[0], md);
        atomicMin(&a.stats[1], sf_float_key(closest));
        if (anyov) atomicAdd(&a.stats[2], 1);
    }
}

// ------------------------------------------------------------------------------------------
// Frame-less progressive mode (Sphereflake.cpp:86-214): random 8-ray packets.
// ------------------------------------------------------------------------------------------

// std::mt19937 continuation: state[0..623] + next index state[624]; writes n tempered 32-bit outputs
// (std::uniform_int_distribution<unsigned>(0) over the full range returns them unchanged).
// One workgroup. The twist runs as 227 independent chains: thread j < 227 makes words j, j + 227 and
// (j < 169) j + 454 of the new block, each from the old block and the chain's own previous word (the
// offset 397 - 624 = -227), in registers -- no barrier inside a twist, one between blocks (there were 3).
// Word 623 of a new block needs new words 0 and 396 (two chains): it is made lazily, in the next twist, by
// the two threads that use it (226: offset 397; 168: offset 1), from the old block's word 623 that the
// buffer being refilled still holds at index 623 (thread 226 writes it back for the twist after).
#define SF_MT_THREADS 256
extern "C" __global__ __launch_bounds__(SF_MT_THREADS) void sf_mt_draws(uint32_t* state, uint32_t* out, uint32_t n)
{
    __shared__ uint32_t buf[2][624];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < 624u; i += SF_MT_THREADS) buf[0][i] = state[i];
    const uint32_t pos0 = min(state[624], 624u);
    __syncthreads();
    auto f = [](uint32_t a, uint32_t b, uint32_t c) {
        const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
        return c ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    };
    auto temper = [](uint32_t y) {
        y ^= y >> 11;
        y ^= (y << 7) & 0x9d2c5680u;
        y ^= (y << 15) & 0xefc60000u;
        y ^= y >> 18;
        return y;
    };
    // the rest of the loaded (complete) block
    const uint32_t m0 = min(624u - pos0, n);
    for (uint32_t k = tid; k < m0; k += SF_MT_THREADS) out[k] = temper(buf[0][pos0 + k]);
    uint32_t done = m0;    // outputs written (uniform)
    uint32_t cur = 0;      // buffer of the newest block
    bool full = true;      // the newest block's word 623 is in the buffer (only the loaded block's)
    uint32_t pos = pos0 + m0;
    while (done < n) {
        const uint32_t* sb = buf[cur];
        uint32_t* tb = buf[cur ^ 1u];
        // output index of the new block's word 0: after the newest block's word 623 when that is still due
        const uint32_t o = done + (full ? 0u : 1u);
        if (tid < 227u) {
            const uint32_t j = tid;
            uint32_t x623 = 0u;   // the newest block's word 623 (threads 226 and 168)
            if (j == 226u || j == 168u) {
                x623 = full ? sb[623] : f(tb[623], sb[0], sb[396]);
                if (j == 226u && !full) {
                    buf[cur][623] = x623;                    // for the lazy word 623 of the block made now
                    if (done < n) out[done] = temper(x623);   // its place in the stream
                }
            }
            const uint32_t wa = f(sb[j], sb[j + 1u], j == 226u ? x623 : sb[j + 397u]);
            tb[j] = wa;
            if (o + j < n) out[o + j] = temper(wa);
            const uint32_t wb = f(sb[j + 227u], sb[j + 228u], wa);
            tb[j + 227u] = wb;
            if (o + j + 227u < n) out[o + j + 227u] = temper(wb);
            if (j < 168u || j == 168u) {
                const uint32_t wc = f(sb[j + 454u], j == 168u ? x623 : sb[j + 455u], wb);
                tb[j + 454u] = wc;
                if (o + j + 454u < n) out[o + j + 454u] = temper(wc);
            }
        }
        __syncthreads();
        done = min(n, o + 623u);   // words 0..622 of the new block (623 is due with the next twist)
        pos = done - o;
        cur ^= 1u;
        full = false;
    }
    // state: the newest block, its word 623 made now if it is lazy
    if (!full && tid == 0u) buf[cur][623] = f(buf[cur ^ 1u][623], buf[cur][0], buf[cur][396]);
    __syncthreads();
    for (uint32_t i = tid; i < 624u; i += SF_MT_THREADS) state[i] = buf[cur][i];
    if (tid == 0) state[624] = pos;
}

// ---- parallel mt19937 draws (jump-ahead; host side sf_mtjump.cpp). A batch's n draws: the r = 624 - pos still
// in the loaded buffer, then n - r "post-buffer" draws cut into K segments of L; segment j starts from the window
// V_{jL} = (t^{jL} mod phi)(A) V_0 (V_0 = the buffer), i.e. word k of it is the XOR of x_{i+k} over the set
// coefficients i of the polynomial -- a convolution of the raw sequence x (sf_mt_raw) split over P workgroups
// per segment (sf_mt_jump_partial), then each segment's workgroup XORs its P partial windows and generates its
// draws (sf_mt_segments). Same stream, bit for bit, as the sequential sf_mt_draws.
namespace {
__device__ __forceinline__ uint32_t mt_f(uint32_t a, uint32_t b, uint32_t c)
{
    const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
    return c ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}
__device__ __forceinline__ uint32_t mt_temper(uint32_t y)
{
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}
// One twist in LDS: nb = the block after ob (both 624 words); 227 threads run the chains (words j, j + 227,
// j + 454) and thread 0 also word 623 = f(ob[623], nb[0], nb[396]): nb[396] is thread 169's second word, which
// thread 0 forms again from ob (two more f) instead of waiting for it behind a barrier. Returns after ONE barrier
// (nb complete), with this thread's words in w[0..2] (w[3]: word 623 on thread 0) for callers that store them
// straight from registers. (Round 4: a barrier before word 623 and a second after it, and the callers re-read nb
// from LDS for their global stores: sf_mt_raw 16.8 us for 33 twists, profiles/r4/final3.)
__device__ __forceinline__ void mt_twist(const uint32_t* ob, uint32_t* nb, uint32_t w[4])
{
    const uint32_t j = threadIdx.x;
    if (j < 227u) {
        const uint32_t a = mt_f(ob[j], ob[j + 1u], ob[j + 397u]);
        nb[j] = a;
        const uint32_t b = mt_f(ob[j + 227u], ob[j + 228u], a);
        nb[j + 227u] = b;
        w[0] = a;
        w[1] = b;
        if (j < 169u) {
            w[2] = mt_f(ob[j + 454u], ob[j + 455u], b);
            nb[j + 454u] = w[2];
        }
        if (j == 0u) {
            const uint32_t a169 = mt_f(ob[169], ob[170], ob[566]);
            const uint32_t b169 = mt_f(ob[396], ob[397], a169);   // nb[396]
            w[3] = mt_f(ob[623], a, b169);
            nb[623] = w[3];
        }
    }
    __syncthreads();
}
}  // namespace

#define SF_MT_PAR_THREADS 256

// The raw sequence x_0..x_{nraw-1} from the state's buffer (x_0..x_623 = the buffer). One workgroup.
extern "C" __global__ __launch_bounds__(SF_MT_PAR_THREADS) void sf_mt_raw(const uint32_t* __restrict__ state,
                                                                           uint32_t* __restrict__ raw, uint32_t blocks)
{
    __shared__ uint32_t buf[2][624];
    for (uint32_t i = threadIdx.x; i < 624u; i += SF_MT_PAR_THREADS) {
        buf[0][i] = state[i];
        raw[i] = state[i];
    }
    __syncthreads();
    const uint32_t j = threadIdx.x;
    for (uint32_t b = 1; b < blocks; ++b) {
        uint32_t w[4];
        mt_twist(buf[(b - 1u) & 1u], buf[b & 1u], w);
        uint32_t* rb = raw + b * 624u;   // this thread's new words, from registers
        if (j < 227u) {
            rb[j] = w[0];
            rb[j + 227u] = w[1];
            if (j < 169u) rb[j + 454u] = w[2];
            if (j == 0u) rb[623] = w[3];
        }
    }
}

// Partial jumped windows: workgroup (s, p) XORs x_{i+k} (k < 624) over the set coefficients i of segment
// s + 1's polynomial within [p C, (p + 1) C), C = ceil(19937 / P); the raw words it needs are staged in LDS.
#define SF_MT_CHUNK ((19937u + SF_MT_PARTS - 1u) / SF_MT_PARTS)
extern "C" __global__ __launch_bounds__(SF_MT_PAR_THREADS) void sf_mt_jump_partial(const uint32_t* __restrict__ raw,
                                                                                    const uint64_t* __restrict__ polys,
                                                                                    uint32_t poly_words,
                                                                                    uint32_t* __restrict__ partial)
{
    // xs: the chunk's raw words, then 624 zeros that the unused slots of an unrolled batch read (XOR 0)
    __shared__ uint32_t xs[SF_MT_CHUNK + 624u + 624u];
    const uint32_t seg = blockIdx.x + 1u, part = blockIdx.y;   // segment 0 needs no jump
    const uint32_t i0 = part * SF_MT_CHUNK, i1 = min(19937u, i0 + SF_MT_CHUNK);
    const uint32_t nx = (i1 - i0) + 624u;
    for (uint32_t i = threadIdx.x; i < nx + 624u; i += SF_MT_PAR_THREADS) xs[i] = i < nx ? raw[i0 + i] : 0u;
    __syncthreads();
    const uint32_t k0 = threadIdx.x, k1 = k0 + 256u, k2 = k0 < 112u ? k0 + 512u : k0;   // window words (k2: 624 total; unused past 112)
    uint32_t a0 = 0u, a1 = 0u, a2 = 0u;
    const uint64_t* pl = polys + (size_t)seg * poly_words;
    for (uint32_t q = i0 >> 6; q <= (i1 - 1u) >> 6; ++q) {
        uint64_t bits = pl[q];   // (uniform)
        const uint32_t lo = q * 64u;
        if (lo < i0) bits &= ~0ull << (i0 - lo);
        if (lo + 64u > i1) bits &= (i1 - lo) >= 64u ? ~0ull : ((1ull << (i1 - lo)) - 1ull);
        // 8 coefficients per batch, their 24 LDS reads issued together (the zero block stands in for the
        // coefficients past the word's last set bit): the loop is LDS-latency bound otherwise
        while (bits) {
            uint32_t ix[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                ix[u] = bits ? lo + (uint32_t)__builtin_ctzll(bits) - i0 : nx;
                bits &= bits - 1ull;
            }
            uint32_t v0[8], v1[8], v2[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                v0[u] = xs[ix[u] + k0];
                v1[u] = xs[ix[u] + k1];
                v2[u] = xs[ix[u] + k2];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                a0 ^= v0[u];
                a1 ^= v1[u];
                a2 ^= v2[u];
            }
        }
    }
    uint32_t* out = partial + ((size_t)blockIdx.x * SF_MT_PARTS + part) * 624u;
    out[k0] = a0;
    out[k1] = a1;
    if (k0 < 112u) out[k0 + 512u] = a2;
}

// Segment j of the batch's n draws: workgroup j builds its window (segment 0: the buffer; others: the XOR of
// their partial windows), then twists and tempers its L post-buffer draws; workgroup 0 also emits the r draws
// left in the buffer. The workgroup holding the last draw stores the generator state after the batch
// (libstdc++ layout) into state_out -- not into `state`, which the other workgroups may still be reading.
extern "C" __global__ __launch_bounds__(SF_MT_PAR_THREADS) void sf_mt_segments(const uint32_t* __restrict__ state,
                                                                                const uint32_t* __restrict__ partial,
                                                                                uint32_t L, uint32_t n,
                                                                                uint32_t* __restrict__ out,
                                                                                uint32_t* __restrict__ state_out)
{
    __shared__ uint32_t buf[2][624];
    const uint32_t j = blockIdx.x, tid = threadIdx.x;
    const uint32_t pos = min(state[624], 624u);
    const uint32_t r = min(624u - pos, n);            // draws still in the buffer
    const uint32_t m = n - r;                         // post-buffer draws
    const uint32_t s0 = j * L;
    if (j == 0u)
        for (uint32_t i = tid; i < r; i += SF_MT_PAR_THREADS) out[i] = mt_temper(state[pos + i]);
    if (m == 0u) {   // the batch ends inside the buffer
        if (j == 0u) {
            for (uint32_t k = tid; k < 624u; k += SF_MT_PAR_THREADS) state_out[k] = state[k];
            if (tid == 0u) state_out[624] = pos + n;
        }
        return;
    }
    if (s0 >= m) return;   // (workgroup-uniform)
    const uint32_t cnt = min(L, m - s0);
    for (uint32_t k = tid; k < 624u; k += SF_MT_PAR_THREADS) {
        uint32_t w;
        if (j == 0u) {
            w = state[k];
        } else {
            const uint32_t* pp = partial + (size_t)(j - 1u) * SF_MT_PARTS * 624u + k;
            w = 0u;
#pragma unroll
            for (uint32_t p = 0; p < SF_MT_PARTS; ++p) w ^= pp[(size_t)p * 624u];
        }
        buf[0][k] = w;
    }
    __syncthreads();
    uint32_t cur = 0, done = 0;
    while (done < cnt) {
        uint32_t w[4];
        mt_twist(buf[cur], buf[cur ^ 1u], w);
        cur ^= 1u;
        const uint32_t take = min(624u, cnt - done);
        uint32_t* ob = out + r + s0 + done;   // this thread's new words, tempered from registers
        if (tid < 227u) {
            if (tid < take) ob[tid] = mt_temper(w[0]);
            if (tid + 227u < take) ob[tid + 227u] = mt_temper(w[1]);
            if (tid < 169u && tid + 454u < take) ob[tid + 454u] = mt_temper(w[2]);
            if (tid == 0u && 623u < take) ob[623] = mt_temper(w[3]);
        }
        done += take;
    }
    if (s0 + cnt == m) {   // the last draw of the batch: the state for the next batch
        for (uint32_t k = tid; k < 624u; k += SF_MT_PAR_THREADS) state_out[k] = buf[cur][k];
        if (tid == 0u) state_out[624] = ((cnt - 1u) % 624u) + 1u;
    }
}

namespace {
// Sobol::Sample (Sobol.cpp:41-55) for dims 0/1.
__device__ __forceinline__ float sobol_sample(uint64_t index, const uint32_t* __restrict__ m, uint32_t scramble)
{
    uint32_t r = scramble;
    for (uint32_t i = 0; index; index >>= 1, ++i)
        if (index & 1u) r ^= m[i];
    return (float)r * (1.f / 4294967296.0f);
}
}  // namespace

// Trace `packets` packets: one 8-lane group per packet, 8 packets per wave. Lane q of packet j uses
// the footprint of Sphereflake.cpp:143-147 around (x0, y0) drawn at Sobol index counter0 + j with
// scrambles draws[2j], draws[2j+1] (Sphereflake.cpp:139-141). Results are staged per lane; the
// owner word of each pixel keeps the highest ticket, so the scatter reproduces sequential order.
// One wave = 64 / PW packets of PW lanes (Sphereflake.cpp:115-160): the AVX footprint is 8 pixels
// around (x0, y0) = 1 + floor(S (W - 2)), 1 + floor(S (H - 2)); the SSE footprint the 2x2 block at
// (x0, y0) = floor(S (W - 1)), floor(S (H - 1)).
template <int PW>
__device__ __forceinline__ void packet_origin(const FrameArgs& a, const DeviceConsts* __restrict__ K,
                                              const uint32_t* draws, uint64_t counter0, uint32_t packet,
                                              float& x0, float& y0)
{
    const uint64_t c = counter0 + packet;
    const float s0 = sobol_sample(c, K->sobol[0], draws[2u * packet]);
    const float s1 = sobol_sample(c, K->sobol[1], draws[2u * packet + 1u]);
    if constexpr (PW == 8) {
        x0 = 1.0f + floorf(s0 * (float)(a.W - 2u));
        y0 = 1.0f + floorf(s1 * (float)(a.H - 2u));
    } else {
        x0 = floorf(s0 * (float)(a.W - 1u));
        y0 = floorf(s1 * (float)(a.H - 1u));
    }
}

// Spatial binning of a batch's packets (the trace order only: results, tickets and the scatter are
// per packet). The reference's packets land uniformly at random, so a wave of 64 / PW consecutive
// packets shares almost no traversal; binned by a square of 2^bin_shift pixels around (x0, y0) they
// share most of it. Counting sort: sf_packet_bin (histogram), sf_packet_scan (exclusive offsets,
// one workgroup), sf_packet_place (slot by atomic cursor; order inside a bin is arbitrary).
template <int PW>
__device__ __forceinline__ uint32_t packet_bin(const FrameArgs& a, const DeviceConsts* __restrict__ K,
                                               const uint32_t* draws, uint64_t counter0, uint32_t packet,
                                               uint32_t bin_shift, uint32_t bins_x)
{
    float x0, y0;
    packet_origin<PW>(a, K, draws, counter0, packet, x0, y0);
    return ((uint32_t)y0 >> bin_shift) * bins_x + ((uint32_t)x0 >> bin_shift);
}

extern "C" __global__ __launch_bounds__(256) void sf_packet_bin(FrameArgs a, const uint32_t* draws, uint64_t counter0,
                                                                 uint32_t packets, uint32_t pw, uint32_t bin_shift,
                                                                 uint32_t bins_x, uint32_t* bin_cnt)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= packets) return;
    const uint32_t b = pw == 8u ? packet_bin<8>(a, a.consts, draws, counter0, p, bin_shift, bins_x)
                                : packet_bin<4>(a, a.consts, draws, counter0, p, bin_shift, bins_x);
    atomicAdd(bin_cnt + b, 1u);
}

extern "C" __global__ __launch_bounds__(1024) void sf_packet_scan(uint32_t* bin_cnt, uint32_t nbins,
                                                                  const uint32_t* __restrict__ rank)
{
    // Counts -> exclusive offsets in place (the place cursors), the bins taken in the order rank[]
    // (heaviest first, from the last batch's per-bin wave cycles) or in index order (rank NULL). Staged
    // through LDS (at the bin's rank) so that global reads and writes are coalesced; thread t scans
    // ranks [t * per, (t + 1) * per) of the staged copy (index padded by 1 per 32 against bank conflicts).
    __shared__ uint32_t cnt[SF_PROG_MAX_BINS + SF_PROG_MAX_BINS / 32u];
    __shared__ uint32_t part[16];
    const uint32_t t = threadIdx.x, per = (nbins + 1023u) / 1024u, b0 = t * per, b1 = min(nbins, b0 + per);
    for (uint32_t i = t; i < nbins; i += 1024u) {
        const uint32_t r = rank ? rank[i] : i;
        cnt[r + (r >> 5)] = bin_cnt[i];
    }
    __syncthreads();
    uint32_t s_ = 0u;
    for (uint32_t b = b0; b < b1; ++b) s_ += cnt[b + (b >> 5)];
    // exclusive scan of the 1024 partials: in-wave shuffles, then the 16 wave totals
    const uint32_t lane = t & 63u, w = t >> 6;
    uint32_t x = s_;
#pragma unroll
    for (uint32_t o = 1u; o < 64u; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        x += lane >= o ? y : 0u;
    }
    if (lane == 63u) part[w] = x;
    __syncthreads();
    if (t == 0u) {
        uint32_t acc = 0u;
        for (uint32_t k = 0; k < 16u; ++k) {
            const uint32_t y = part[k];
            part[k] = acc;
            acc += y;
        }
    }
    __syncthreads();
    uint32_t off = part[w] + x - s_;
    for (uint32_t b = b0; b < b1; ++b) {
        const uint32_t c = cnt[b + (b >> 5)];
        cnt[b + (b >> 5)] = off;
        off += c;
    }
    __syncthreads();
    for (uint32_t i = t; i < nbins; i += 1024u) {
        const uint32_t r = rank ? rank[i] : i;
        bin_cnt[i] = cnt[r + (r >> 5)];
    }
}

// Frame-less heavy-first order: per 64-bin chunk, the cost-bucket histogram of the bins' last recorded
// wave cycles (input of sf_order_scan / sf_order_scatter, which then rank the bins heaviest first).
extern "C" __global__ __launch_bounds__(64) void sf_bin_hist(const uint32_t* __restrict__ bin_cost, uint32_t nbins,
                                                             uint32_t* __restrict__ chunk_cnt)
{
    const uint32_t c = blockIdx.x, lane = threadIdx.x, i = c * 64u + lane;
    const uint32_t bk = i < nbins ? cost_bucket(bin_cost[i]) : SF_ORDER_BUCKETS;
    uint32_t mine = 0u;
#pragma unroll 1
    for (uint32_t b = 0; b < SF_ORDER_BUCKETS; ++b) {
        const uint32_t n = (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(bk == b));
        mine = lane == b ? n : mine;
    }
    if (lane < SF_ORDER_BUCKETS) chunk_cnt[c * SF_ORDER_BUCKETS + lane] = mine;
}

extern "C" __global__ __launch_bounds__(256) void sf_packet_place(FrameArgs a, const uint32_t* draws, uint64_t counter0,
                                                                   uint32_t packets, uint32_t pw, uint32_t bin_shift,
                                                                   uint32_t bins_x, uint32_t* bin_cur, uint32_t* perm)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= packets) return;
    const uint32_t b = pw == 8u ? packet_bin<8>(a, a.consts, draws, counter0, p, bin_shift, bins_x)
                                : packet_bin<4>(a, a.consts, draws, counter0, p, bin_shift, bins_x);
    perm[atomicAdd(bin_cur + b, 1u)] = p;
}

template <int PW>
__device__ __forceinline__ void progressive_trace(const FrameArgs& a, const uint32_t* draws, uint64_t counter0,
                                                  uint32_t packets, uint64_t ticket0, PacketLane* lanes,
                                                  unsigned long long* owner, const uint32_t* perm, uint32_t wave,
                                                  uint32_t levels, uint32_t* ovf_list, uint32_t* ovf_cnt)
{
    extern __shared__ float lds[];
    constexpr uint32_t PPW = 64u / PW;   // packets per wave
    const DeviceConsts* __restrict__ K = a.consts;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t slot = wave * PPW + lane / PW;   // position in the (binned) trace order
    if (wave * PPW >= packets) return;   // wave-uniform
    const uint64_t w_start = (a.flags & SF_FLAG_DIAG_UNITS) ? __builtin_amdgcn_s_memrealtime() : 0ull;
    const uint64_t c_start = a.bin_cost ? __builtin_amdgcn_s_memtime() : 0ull;
    const bool valid = slot < packets;
    const uint32_t packet = valid ? (perm ? perm[slot] : slot) : slot;
    const uint32_t q = lane % PW;
    float x0 = 0.f, y0 = 0.f;
    if (valid) packet_origin<PW>(a, K, draws, counter0, packet, x0, y0);
    float ox, oy;
    if constexpr (PW == 8) {
        // xa = {x0, x0+1, x0+1, x0, x0, x0+1, x0-1, x0-1}, ya = {y0, y0+1, y0, y0+1, y0-1, y0-1, y0, y0-1}
        ox = (q == 1u || q == 2u || q == 5u) ? 1.0f : (q >= 6u ? -1.0f : 0.0f);
        oy = (q == 1u || q == 3u) ? 1.0f : ((q == 4u || q == 5u || q == 7u) ? -1.0f : 0.0f);
    } else {
        // xa = {x0, x0+1, x0, x0+1}, ya = {y0, y0, y0+1, y0+1}
        ox = (q & 1u) ? 1.0f : 0.0f;
        oy = (q & 2u) ? 1.0f : 0.0f;
    }
    const float xf = x0 + ox, yf = y0 + oy;
    float dx, dy, dz;
    ray_dir(a, xf, yf, dx, dy, dz, K->lut);

    HitState h;
    int32_t maxd = -1;
    uint32_t status = 0u;
    stage_root(lds, a.root);
    traverse_packet<PW>(K, a.root, lds, build_column(K), levels, dx, dy, dz, valid, h, maxd, status, a.flags);
    const bool overflowed = (status & SF_STATUS_OVERFLOW) != 0u;

    PacketLane out;
    shade(dx, dy, dz, h, K->lut, out.px, out.py, out.pz, out.nx, out.ny, out.nz);
    out.min_t = h.minT;
    // idx = (size_t)xa + (size_t)ya * W; the reference skips idx > size (Sphereflake.cpp:188-191)
    const uint64_t pix = (uint64_t)xf + (uint64_t)yf * a.W;
    const bool inb = valid && pix < (uint64_t)a.W * a.H;
    out.pixel = inb ? (uint32_t)pix : 0xffffffffu;
    if (valid) lanes[(size_t)packet * PW + q] = out;
    if (inb && !(a.flags & SF_FLAG_DIAG_NO_OWNER)) atomicMax(owner + pix, (unsigned long long)(ticket0 + packet));

    const float closest = wave_min(inb ? h.minT : FLT_MAX);
    const bool anyov = wave_ballot(overflowed) != 0ull;
    if (lane == 0u) {   // read before the atomic: issued only when it changes the word (one address)
        const int32_t key = sf_float_key(closest);
        const int32_t cur_d = __hip_atomic_load(&a.stats[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int32_t cur_k = __hip_atomic_load(&a.stats[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (maxd > cur_d) atomicMax(&a.stats[0], maxd);
        if (key < cur_k) atomicMin(&a.stats[1], key);
        if (anyov && !ovf_list) atomicAdd(&a.stats[2], 1);
    }
    // adaptive levels: a wave that needed more is re-traced whole by sf_progressive_fixup (its partial
    // lanes, owner words and stats are all superseded or implied by the complete traversal)
    if (anyov && ovf_list) {
        const uint32_t k = wave_fetch_add(ovf_cnt, 1u);
        ovf_list[k] = wave;   // uniform value and address
    }
    if (a.bin_cost && perm) {
        // scheduling hint for the next batch (sf_bin_hist): this wave's cycles, for the bin of its first
        // packet (uniform value and address; bins with several waves keep the last one's)
        const uint64_t cyc = __builtin_amdgcn_s_memtime() - c_start;
        const uint32_t p0 = __builtin_amdgcn_readfirstlane(perm[wave * PPW]);
        const uint32_t b = __builtin_amdgcn_readfirstlane(
            packet_bin<PW>(a, K, draws, counter0, p0, a.bin_shift, a.bins_x));
        // quantised to a power of 4: cost classes two octaves wide, so that bins of one class keep their
        // index (screen) order and a wave straddling two bins still gets spatial neighbours
        const uint32_t c32 = cyc > 0x7fffffffull ? 0x7fffffffu : ((uint32_t)cyc | 1u);
        a.bin_cost[b] = 1u << ((31u - (uint32_t)__builtin_clz(c32)) & ~1u);
    }
    if ((a.flags & SF_FLAG_DIAG_UNITS) && a.tile_trace && wave < SF_DIAG_WAVES) {   // diagnostics: this wave's
        // {start, end}, in the per-wave records of the context's trace buffer (sf_set_tile_trace)
        uint64_t* wt = a.tile_trace + (SF_TRACE_WORDS((uint64_t)((a.W + 7u) / 8u) * ((a.H + 7u) / 8u)) - 2u * SF_DIAG_WAVES);
        wt[2u * wave] = w_start;
        wt[2u * wave + 1u] = __builtin_amdgcn_s_memrealtime();
    }
}

template <int PW>
__device__ __forceinline__ void progressive_fixup(const FrameArgs& a, const uint32_t* draws, uint64_t counter0,
                                                  uint32_t packets, uint64_t ticket0, PacketLane* lanes,
                                                  unsigned long long* owner, const uint32_t* perm,
                                                  const uint32_t* ovf_list, uint32_t* counters, uint32_t parity)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) counters[parity ^ 1u] = 0u;   // the next batch's list
    const uint32_t n = counters[parity];
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x)
        progressive_trace<PW>(a, draws, counter0, packets, ticket0, lanes, owner, perm,
                              __builtin_amdgcn_readfirstlane(ovf_list[i]),
                              SF_PROGRESSIVE_LEVELS, nullptr, nullptr);
}

extern "C" __global__ __launch_bounds__(64) void sf_progressive_trace(FrameArgs a, const uint32_t* draws,
                                                                       uint64_t counter0, uint32_t packets,
                                                                       uint64_t ticket0, PacketLane* lanes,
                                                                       unsigned long long* owner, const uint32_t* perm,
                                                                       uint32_t levels, uint32_t* ovf_list,
                                                                       uint32_t* ovf_cnt)
{
    progressive_trace<8>(a, draws, counter0, packets, ticket0, lanes, owner, perm, blockIdx.x, levels, ovf_list,
                         ovf_cnt);
}
extern "C" __global__ __launch_bounds__(64) void sf_progressive_trace_sse(FrameArgs a, const uint32_t* draws,
                                                                           uint64_t counter0, uint32_t packets,
                                                                           uint64_t ticket0, PacketLane* lanes,
                                                                           unsigned long long* owner, const uint32_t* perm,
                                                                           uint32_t levels, uint32_t* ovf_list,
                                                                           uint32_t* ovf_cnt)
{
    progressive_trace<4>(a, draws, counter0, packets, ticket0, lanes, owner, perm, blockIdx.x, levels, ovf_list,
                         ovf_cnt);
}
extern "C" __global__ __launch_bounds__(64) void sf_progressive_fixup(FrameArgs a, const uint32_t* draws,
                                                                       uint64_t counter0, uint32_t packets,
                                                                       uint64_t ticket0, PacketLane* lanes,
                                                                       unsigned long long* owner, const uint32_t* perm,
                                                                       const uint32_t* ovf_list, uint32_t* counters,
                                                                       uint32_t parity)
{
    progressive_fixup<8>(a, draws, counter0, packets, ticket0, lanes, owner, perm, ovf_list, counters, parity);
}
extern "C" __global__ __launch_bounds__(64) void sf_progressive_fixup_sse(FrameArgs a, const uint32_t* draws,
                                                                           uint64_t counter0, uint32_t packets,
                                                                           uint64_t ticket0, PacketLane* lanes,
                                                                           unsigned long long* owner,
                                                                           const uint32_t* perm,
                                                                           const uint32_t* ovf_list,
                                                                           uint32_t* counters, uint32_t parity)
{
    progressive_fixup<4>(a, draws, counter0, packets, ticket0, lanes, owner, perm, ovf_list, counters, parity);
}

// Last writer wins by ticket (= the reference worker's sequential packet order).
extern "C" __global__ __launch_bounds__(256) void sf_progressive_scatter(FrameArgs a, uint32_t packets, uint64_t ticket0,
                                                                         const PacketLane* lanes,
                                                                         const unsigned long long* owner)
{
    const uint32_t pl = a.packet_lanes;   // lanes per packet (8 AVX, 4 SSE)
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= packets * pl) return;
    const PacketLane l = lanes[i];
    if (l.pixel == 0xffffffffu) return;
    if (owner[l.pixel] != (unsigned long long)(ticket0 + i / pl)) return;
    reinterpret_cast<float4*>(a.pos)[l.pixel] = make_float4(l.px, l.py, l.pz, 1.0f);
    reinterpret_cast<float4*>(a.nrm)[l.pixel] = make_float4(l.nx, l.ny, l.nz, 1.0f);
    if (a.emit_aux && a.min_t) a.min_t[l.pixel] = l.min_t;
}
