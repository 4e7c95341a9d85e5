/*
 * sf.h -- C ABI of the MI355X (gfx950) Sphereflake primary-ray G-buffer renderer.
 *
 * This is the drop-in boundary for the reference hot path. The reference has no
 * FFI: its boundary is the C++ class SphereflakeRaytracer::Sphereflake
 * (/root/reference/sphereflake/Sphereflake.h:13-58). Each entry point below names
 * the member of that class (or the reference code) it replaces; the C++ class of
 * the same name and surface, layered on this ABI, is
 * sphereflake-raytracer_amd/csrc/Sphereflake.hpp.
 *
 * Conventions
 *   - Every call returns 0 on success and a negative SF_E* code on failure
 *     (sf_strerror() names it). HIP runtime errors map to SF_EHIP; the HIP code
 *     is kept in the context (sf_last_hip_error()).
 *   - The caller owns host buffers; the context owns its device buffers.
 *   - One context per device per host thread. Calls are stream-ordered on the
 *     context stream (or params->stream); sf_download() synchronises. Calls on
 *     different streams of one context run in call order; a caller's stream is
 *     not touched after the call that used it returns (it may be destroyed once
 *     its work is done).
 *   - G-buffer layout is the reference's: float4 (x, y, z, 1) per pixel,
 *     row-major x + y*W, y = 0 is the TOP edge (Sphereflake.cpp:186-196). Misses
 *     are (0, 0, 0, 1), so the GL SSAO post-process consumes it unchanged
 *     (Shaders/post_final.glsl:20, post_ssao.glsl:33).
 *   - Arithmetic is IEEE binary32 reproducing the reference AVX path bit for bit
 *     (per-ray semantics).
 */
#ifndef SPHEREFLAKE_SF_H
#define SPHEREFLAKE_SF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SF_ABI_VERSION 1

enum sf_status {
    SF_OK = 0,
    SF_EINVAL = -1,      /* bad argument (null pointer, zero size, out-of-range band) */
    SF_ENOMEM = -2,      /* device or host allocation failed */
    SF_EHIP = -3,        /* HIP runtime error (see sf_last_hip_error) */
    SF_ENODEV = -4,      /* no such device / not a gfx950 device */
    SF_ENOVIEW = -5,     /* sf_render before sf_set_view */
    SF_EDEPTH = -6,      /* traversal exceeded SF_MAX_DEPTH_LIMIT levels */
    SF_ESTATE = -7,      /* call not valid in the current state (e.g. progressive mode running) */
    SF_ECOMM = -8        /* RCCL error (see sf_dist_last_error) */
};

/* Traversal kernels. */
enum sf_kernel {
    SF_KERNEL_WAVE = 0,      /* default: wave-coherent traversal, one 8x8 pixel tile per wave64,
                                child transforms built cooperatively into LDS */
    SF_KERNEL_PER_RAY = 1    /* one thread per ray, private traversal stack */
};

#define SF_MAX_DEPTH_LIMIT 31   /* traversal levels (expanding depths 0..30) the kernels support */

typedef struct sf_ctx sf_ctx;

/* Per-render options. Zero-initialise and set what you need. */
typedef struct sf_render_params {
    /* Row sharding for multi-GPU. The frame is cut into bands of
       band_rows rows (must be a multiple of 8; 0 = one band = whole frame); this call
       renders the bands b with b % band_count == band_index (band_count 0 or 1 = all). */
    uint32_t band_rows;
    uint32_t band_count;
    uint32_t band_index;
    /* 1: write only the owned bands, packed contiguously (a "slab": band k of this
       rank at rows [k*band_rows, (k+1)*band_rows)); 0: write at frame positions. */
    uint32_t compact;
    uint32_t kernel;          /* enum sf_kernel */
    uint32_t emit_aux;        /* 1: also write minT (float) and hit index (uint32) channels */
    uint32_t max_depth;       /* traversal stack levels to provision (0 = auto: 12, retried at
                                 SF_MAX_DEPTH_LIMIT if a tile needs more) */
    uint32_t packed;          /* band slab formats of the multi-GPU gather (wave kernel only; nrm4 unused):
                                 1: ONE float4 (nx, ny, nz, minT) per pixel into pos4, 16 B/pixel instead of 32;
                                    the receiver forms the position dir * minT bit for bit (sf_unpack_slabs);
                                 2: ONE uint32 per pixel into pos4: the hit sphere's heap index (9n+1+i,
                                    0xffffffff = miss), 4 B/pixel; the receiver rebuilds the sphere's frame, the
                                    self test's minT, position and normal bit for bit. Only where sf_slab_bytes()
                                    is 4 for the view (else SF_EINVAL) */
    void* stream;             /* hipStream_t to launch on; NULL = the context stream */
} sf_render_params;

/* Frame statistics; mirrors Sphereflake::GetMaxDepthReached / GetRaysPerSecond /
   GetClosestSphereDistance (Sphereflake.h:30-58). Accumulated over renders until reset. */
typedef struct sf_stats {
    int32_t max_depth;        /* deepest node that passed bounding + LOD (Sphereflake.h:157-160) */
    float closest;            /* min minT over rays (FLT_MAX if none; may be negative) */
    int64_t rays;             /* rays traced */
    int64_t overflow_tiles;   /* tiles re-rendered because they needed a deeper stack */
} sf_stats;

/* --- lifetime ------------------------------------------------------------ */

/* Replaces Sphereflake::Sphereflake(width, height) (Sphereflake.cpp:43-55): allocates the
   device G-buffer (2 x W*H float4, zeroed like glm's vec4() default) and the aux channels,
   computes the 9 child transforms (ComputeChildTransformations, Sphereflake.cpp:216-249). */
int sf_create(int device, uint32_t width, uint32_t height, sf_ctx** out);

/* Replaces Sphereflake::~Sphereflake (Sphereflake.cpp:57-65). */
void sf_destroy(sf_ctx* ctx);

/* --- view and setup ------------------------------------------------------ */

/* Replaces Sphereflake::SetView (Sphereflake.cpp:76-84): stores the ray origin and image-plane
   corners; root transform = translate(-origin) * CreateRotationMatrix((90,0,0)). */
int sf_set_view(sf_ctx* ctx, const float origin[3], const float top_left[3],
                const float top_right[3], const float bottom_left[3]);

/* Override the host-computed setup constants (root transform and 9 unit child frames,
   glm column-major 4x4). For parity tests against fixture dumps. The child frames must be affine
   (row 3 exactly 0, 0, 0, 1, as Sphereflake.cpp:216-249 makes them): SF_EINVAL otherwise. */
int sf_set_setup(sf_ctx* ctx, const float child[9][16], const float root[16]);

/* Read back the setup constants currently in use. */
int sf_get_setup(const sf_ctx* ctx, float child[9][16], float root[16]);

/* --- rendering ----------------------------------------------------------- */

/* One full-frame (or banded) render into the context's device G-buffer. Replaces the
   std::thread sampling loop Sphereflake::DoImagePart (Sphereflake.cpp:86-214) with a
   deterministic frame. params may be NULL (defaults). Asynchronous on the stream. */
int sf_render(sf_ctx* ctx, const sf_render_params* params);

/* Same, into caller-owned DEVICE buffers (e.g. torch tensors): pos4/nrm4 are float4 arrays
   of rows*W elements, where rows = H (compact = 0) or the slab height (compact = 1);
   min_t / hit_index may be NULL. */
int sf_render_to(sf_ctx* ctx, const sf_render_params* params, float* pos4, float* nrm4,
                 float* min_t, uint32_t* hit_index);

/* --- caller-supplied directions ------------------------------------------- */
/* The reference traces only the pixels of its pinhole frame (ray generation, Sphereflake.cpp:149-167), and brakes the
   camera by the nearest sphere among those rays (GetClosestSphereDistance, main.cpp:213) -- moves along directions no
   pixel covers (main.cpp:214-242) are unguarded, its README's "flying into a sphere". Everything after ray generation
   depends on the ray's normalised direction, the root transform, the child frames and the LOD constant only
   (Sphereflake.h:86-226), so any direction can be traced from the view's origin: collision probes, picking and
   ranging, other camera models (panoramas, fisheye, cube faces) for the same G-buffer consumers.
   Ray i is the reference's ray with D = Normalize(dirs[i]) (SIMD_AVX.h:170-180: rsqrtps and one Newton step), from the
   origin, root transform and child frames of sf_set_view / sf_set_setup, with the context's variant and per-ray
   semantics. It gets exactly what a frame pixel with that direction gets: pos4 (x, y, z, 1), nrm4 likewise, a miss
   (0, 0, 0, 1); min_t FLT_MAX on a miss; hit_index the low 32 bits of the heap index, 0xffffffff on a miss. A
   direction that does not normalise to finite numbers (zero, tiny, NaN, infinite) is a miss, as the reference's
   arithmetic makes it. Results never depend on the order or grouping of the rays. */
typedef struct sf_dirs_params {
    uint32_t width, height;   /* rays = width * height, row-major; height == 1: a plain list */
    uint32_t stride;          /* floats per direction in `dirs`: 3 or 4 (the 4th is ignored) */
    uint32_t max_depth;       /* levels to provision, as sf_render_params.max_depth (0 = auto: the view's geometric
                                 bound; groups of rays that need more are re-traced at SF_MAX_DEPTH_LIMIT) */
    void* stream;             /* NULL = the context stream */
} sf_dirs_params;

/* Into caller-owned DEVICE buffers, in ray order (`dirs` is a device array too); any output may be NULL, not all
   four. Asynchronous on the stream, ordered with the context's other calls as sf_render_to is. Stats accumulate as
   for a render (max depth, closest, rays += width * height; overflow_tiles counts the re-traced groups of 64 rays).
   SF_ENOVIEW before a view is set; SF_EINVAL for a stride other than 3 or 4, null dirs, all outputs null or more
   than 2^31 - 1 rays; zero rays: SF_OK, nothing done. A later render is not affected in any way. */
int sf_trace_dirs_to(sf_ctx* ctx, const sf_dirs_params* params, const float* dirs, float* pos4, float* nrm4,
                     float* min_t, uint32_t* hit_index);
/* Into the context's own G-buffer and aux channels (sf_download, sf_post_process, sf_save_image then see a frame
   of another camera model); width x height must equal the context's frame (SF_EINVAL otherwise). */
int sf_trace_dirs(sf_ctx* ctx, const sf_dirs_params* params, const float* dirs);
/* Host convenience for a few rays (picking, collision probes along the move axes of main.cpp:214-242): HOST arrays
   in (n x 3 floats) and out, synchronous. Outputs may be NULL (not all four). */
int sf_probe_dirs(sf_ctx* ctx, const float* dirs3, uint32_t n, float* min_t, uint32_t* hit_index, float* pos4,
                  float* nrm4);

/* --- caller-supplied origins and directions -------------------------------- */
/* The origin enters the reference's ray only through the translation column of the root transform
   (Sphereflake.cpp:83); everything after ray generation depends on the normalised direction, the root transform, the
   child frames and the LOD constant only (Sphereflake.h:86-226). So "ray i from origins[i]" has an exact meaning:
   what the reference returns for that direction after SetView at that origin. Uses: a batch of cameras (stereo
   pairs, cube-map probes, thumbnails along a path) in one launch; the brake of main.cpp:213 probed from where the
   camera WILL be (sphereflake_amd/rays.py: look_ahead); picking and ranging from points that are not the camera;
   secondary rays from hit points.
   Ray i is the reference's ray with D = Normalize(dirs[i]) (SIMD_AVX.h:170-180) under a root transform whose columns
   0..2 are the context's current root's (sf_set_view / sf_set_setup) and whose column 3 is that of
   sf_root_transform(origin), 0 - origin per component; with the context's child frames and variant. Outputs as
   sf_trace_dirs_to, except: pos4 is relative to the ray's OWN origin (D t, the reference's view space); min_t may be
   negative where the origin is inside a sphere; an origin that is not three finite numbers is a miss, as the
   reference's arithmetic makes it (the root's tca is NaN or infinite, SIMD_AVX.h:247-258). Results never depend on
   the order or grouping of the rays.
   THE REFERENCE'S QUIRK, reproduced: RaySphereIntersection rejects a sphere whose centre is behind the ray
   (tca >= 0, SIMD_AVX.h:247-258), also when the origin is inside it, and the root's bounding ball is tested first.
   A ray that starts on the flake and heads away from the flake's centre therefore sees NOTHING, whatever lies along
   it (shadow feelers that START ON THE FLAKE and head for a light outside it all miss); rays heading inwards behave
   as expected. This entry point is no occlusion query for rays that start on the flake. Shadows from a point light
   are traced the other way round, from the light, where the quirk cannot bite: sf_trace_shadow_to below. */
typedef struct sf_rays_params {
    uint32_t width, height;     /* rays = width * height, row-major; height == 1: a plain list (as sf_dirs_params) */
    uint32_t dir_stride;        /* floats per direction: 3 or 4 */
    uint32_t origin_stride;     /* floats per origin: 3 or 4 */
    uint32_t rays_per_origin;   /* ray i starts at origins[i / rays_per_origin]; 0 or 1: one origin per ray */
    uint32_t max_depth;         /* levels to provision; 0 = auto: 12, flagged groups re-traced at SF_MAX_DEPTH_LIMIT */
    void* stream;               /* NULL = the context stream */
} sf_rays_params;

/* Into caller-owned DEVICE buffers, in ray order (`origins` and `dirs` are device arrays too); any output may be NULL,
   not all four. Asynchronous on the stream, ordered with the context's other calls as sf_render_to is; stats
   accumulate as for sf_trace_dirs_to. SF_ENOVIEW before a view is set; SF_EINVAL for a stride other than 3 or 4, null
   origins or dirs, all outputs null or more than 2^31 - 1 rays; zero rays: SF_OK, nothing done. A later render is not
   affected in any way. (There is no variant into the context's own G-buffer: its consumers assume one origin.) */
int sf_trace_rays_to(sf_ctx* ctx, const sf_rays_params* params, const float* origins, const float* dirs,
                     float* pos4, float* nrm4, float* min_t, uint32_t* hit_index);
/* Host convenience for a few rays (the look-ahead brake beside main.cpp:213-242): HOST arrays in (n x 3 directions,
   ceil(n / rays_per_origin) x 3 origins) and out, synchronous. Outputs may be NULL (not all four). */
int sf_probe_rays(sf_ctx* ctx, const float* origins3, const float* dirs3, uint32_t n, uint32_t rays_per_origin,
                  float* min_t, uint32_t* hit_index, float* pos4, float* nrm4);

/* --- shadows from a point light -------------------------------------------- */
/* Is the surface point of pixel p lit by a point light at l? No ray has to start on the flake for that (see THE
   REFERENCE'S QUIRK above): the ray is traced FROM THE LIGHT towards the surface point and its nearest hit compared
   with the distance to the point. Every such ray starts at l; with l outside the flake's bounding ball (radius 2
   about the flake's centre, which encloses every sphere and every nested bounding ball) no sphere the ray can meet
   has its centre behind the ray, so the reference's own arithmetic gives the geometrically right answer. The rays
   share one origin: the coherent one-origin traversal of sf_trace_rays_to, in an any-hit mode that stops a ray at
   its first occluder, fused with the read of the position image; one byte per pixel comes out.
   DEFINITION (exact). Inputs: a position image pos4 (width x height float4, view space, as sf_render writes it), the
   origin o it is relative to, the light l (world), a relative bias b in [0, 1). All arithmetic is binary32, round to
   nearest, every operation rounded on its own (no fused multiply-add). For pixel p with P = pos4[p].xyz:
     1. P == (0, 0, 0) is a miss of the frame (the test of Shaders/post_final.glsl:20): vis[p] = 255, no ray.
     2. w = o + P per component; d = (w - l) + 0.0f per component (the + 0.0f removes -0).
     3. len = sqrt((d.x d.x + d.y d.y) + d.z d.z); bound = len (1.0f - b).
     4. The ray is the reference's ray for Normalize(d) (SIMD_AVX.h:170-180) under the root transform whose columns
        0..2 are the context's and whose column 3 is 0 - l: sf_trace_rays_to's ray from the single origin l, with the
        context's child frames and variant.
     5. With m the min_t of that ray (what sf_trace_rays_to returns): vis[p] = (m < bound) ? 0 : 255.
     6. A d that does not normalise to finite numbers, or a light that is not finite, misses the root: vis[p] = 255.
   sphereflake_amd/lights.py (shadow_model) states steps 1-3 on the host.
   CONSEQUENCES, not engineered away:
   - THE LEVEL OF DETAIL IS THE LIGHT'S. A node refines while sqrt(t / r) < 70 with t measured FROM THE LIGHT
     (Sphereflake.h:146), not from the camera: a distant light -- a "directional" one placed far off -- casts coarse
     shadows, and spheres the camera sees may cast none. sf_set_shadow_lod below replaces the 70 for the shadow
     traces; a directional light proper is sf_trace_sun_to.
   - A LIGHT INSIDE THE RADIUS-2 BALL gets the reference's answer, quirk included: spheres whose centre is behind a
     ray, as seen from the light, do not occlude.
   - Self-shadow acne is governed by the bias b: the camera's and the light's traversals stop at different levels of
     detail and round differently, so the sphere a pixel lies on is met at a distance near len, on either side. */
typedef struct sf_shadow_params {
    float light[3];           /* l, world space */
    float bias;               /* b, 0 <= b < 1 (sf_shadow_defaults: 2^-10) */
    float origin[3];          /* o, with use_origin != 0 */
    uint32_t use_origin;      /* 0: o is the context's view origin (sf_set_view) */
    uint32_t width, height;   /* size of the position image; 0, 0: the context's frame size */
    uint32_t max_depth;       /* levels to provision; 0 = auto: the geometric bound of the LIGHT's position (as
                                 sf_dirs_params.max_depth for the view's); flagged tiles are re-traced at
                                 SF_MAX_DEPTH_LIMIT */
    void* stream;             /* NULL = the context stream */
} sf_shadow_params;

/* light (0, 0, 0), the default bias, the context's origin and frame size, auto levels, the context stream. */
int sf_shadow_defaults(const sf_ctx* ctx, sf_shadow_params* params);
/* pos4: DEVICE position image (NULL = the context's G-buffer; the sizes must then be 0 or the context's); vis: DEVICE
   output, width * height bytes, row-major as pos4. Asynchronous on the stream, ordered with the context's other
   calls as sf_trace_dirs_to is. Touches none of the context's statistics (max depth, closest, rays) and none of the
   renders' state; re-traced tiles count in overflow_tiles as sf_trace_dirs_to's groups do. SF_ENOVIEW before a view
   is set; SF_EINVAL for a null vis, a bias outside [0, 1) or NaN, max_depth > SF_MAX_DEPTH_LIMIT, sizes that disagree
   with a NULL pos4, one size zero and the other not, or more than 2^31 - 1 pixels. */
int sf_trace_shadow_to(sf_ctx* ctx, const sf_shadow_params* params, const float* pos4, uint8_t* vis);
/* The context's G-buffer into the context's own visibility buffer (W * H bytes, allocated on first use). */
int sf_trace_shadow(sf_ctx* ctx, const sf_shadow_params* params);
/* Synchronous D2H of that buffer (W * H bytes); SF_ESTATE before any sf_trace_shadow. */
int sf_download_shadow(sf_ctx* ctx, uint8_t* vis);
/* Its device pointer (NULL before any sf_trace_shadow); see sf_device_buffers. */
int sf_shadow_buffer(sf_ctx* ctx, uint8_t** vis);
/* Light the RGBA8 image of sf_post_process in place, after it. Per pixel, with P, w and len as above (the same exact
   arithmetic; the division is correctly rounded) and n = nrm4[p].xyz: a frame miss (P == 0) is left untouched; else
   e = l - w per component, lam = max(0, ((n.x e.x + n.y e.y) + n.z e.z) / len) (0 where that is NaN),
   k = ambient + (1 - ambient) (vis[p] ? lam : 0), and each of r, g, b becomes (uint8) min(c k + 0.5f, 255); alpha
   stays. params: light, origin / use_origin, stream (the image has the context's frame size). NULL pos4 / nrm4 / vis
   / rgba select the context's G-buffer, visibility buffer and image; SF_ESTATE where a context buffer selected that
   way was never written (no sf_post_process, no sf_trace_shadow); SF_EINVAL for an ambient outside [0, 1] or NaN.
   Asynchronous on the stream. sphereflake_amd/lights.py: light_model. */
int sf_light_image(sf_ctx* ctx, const sf_shadow_params* params, float ambient, const float* pos4, const float* nrm4,
                   const uint8_t* vis, uint8_t* rgba);

/* --- many lights per pixel: soft shadows, sky light ------------------------- */
/* Extends sf_trace_shadow_to from one light to n <= SF_SHADOW_LIGHTS_MAX lights in ONE launch: an area light sampled
   at n points (a penumbra), or n lights placed outside the radius-2 ball as a ray-traced sky occlusion term (the only
   way to occlusion here: feelers that start on the flake see nothing, THE REFERENCE'S QUIRK above). Each tile's wave
   loads its positions once and loops over the lights; one 64-bit word per pixel comes out instead of n byte images.
   DEFINITION OF THE MASK (exact). Bit i (i < n) of mask[p] is 1 iff sf_trace_shadow_to with light = lights[i] and
   the same bias, origin, sizes and position image writes 255 at p, and 0 iff it writes 0: steps 1-6 of its
   definition apply per light, unchanged. Bits n..63 are 0. So a miss of the frame (P == 0) has its low n bits all
   set, and a light that is not finite sets its own bit everywhere and leaves the other lights' bits alone. THE LEVEL
   OF DETAIL IS EACH LIGHT'S OWN, and a light inside the radius-2 ball gets the reference's answer, as there. */
#define SF_SHADOW_LIGHTS_MAX 64
typedef struct sf_shadows_params {
    const float* lights;      /* HOST, n x 3 floats, world space; read before the call returns */
    const float* weights;     /* HOST, n floats, or NULL = every weight (float)1 / (float)n; sf_light_image_many only */
    uint32_t n;               /* 1 .. SF_SHADOW_LIGHTS_MAX */
    float bias;               /* as sf_shadow_params.bias; one bias for all lights */
    float origin[3];          /* as sf_shadow_params.origin */
    uint32_t use_origin;      /* as sf_shadow_params.use_origin */
    uint32_t width, height;   /* as sf_shadow_params */
    uint32_t max_depth;       /* 0 = auto: the largest geometric bound over the n lights */
    void* stream;             /* NULL = the context stream */
} sf_shadows_params;

/* Zeroed (n = 0, lights NULL: the caller sets both), the default bias of sf_shadow_defaults. */
int sf_shadows_defaults(const sf_ctx* ctx, sf_shadows_params* params);
/* As sf_trace_shadow_to (pos4 DEVICE or NULL = the context's G-buffer; asynchronous and ordered as it is; no statistic
   and none of the renders' state touched; re-traced tiles -- a tile flagged for any light is re-traced once, for all
   of them -- count in overflow_tiles). mask: DEVICE output, width * height uint64_t, row-major as pos4. Errors as
   sf_trace_shadow_to's, and SF_EINVAL for n == 0, n > SF_SHADOW_LIGHTS_MAX, a null lights or a null mask. */
int sf_trace_shadows_to(sf_ctx* ctx, const sf_shadows_params* params, const float* pos4, uint64_t* mask);
/* The context's G-buffer into the context's own mask buffer (W * H * 8 bytes, allocated on first use); extends
   sf_trace_shadow. */
int sf_trace_shadows(sf_ctx* ctx, const sf_shadows_params* params);
/* Synchronous D2H of that buffer (W * H uint64_t); SF_ESTATE before any sf_trace_shadows. Extends sf_download_shadow. */
int sf_download_shadow_masks(sf_ctx* ctx, uint64_t* mask);
/* Its device pointer (NULL before any sf_trace_shadows); extends sf_shadow_buffer. */
int sf_shadow_mask_buffer(sf_ctx* ctx, uint64_t** mask);
/* Extends sf_light_image from a product to a SUM over lights (sf_light_image scales in place, so two calls multiply).
   Exact, binary32, one rounding per operation, no fma: a frame miss is left untouched; else S = 0, then for
   i = 0 .. n-1 in that order S = S + w_i (bit i of mask[p] ? lam_i : 0) with lam_i exactly sf_light_image's lam for
   lights[i] (0 where NaN); k = ambient + (1 - ambient) S, and each of r, g, b becomes (uint8) min(c k + 0.5f, 255);
   alpha stays. S is not clamped: with n = 1 and weight 1 the result is sf_light_image's, byte for byte. params:
   lights, weights, n, origin / use_origin, stream. NULL pos4 / nrm4 / mask / rgba select the context's G-buffer, mask
   buffer and image; SF_ESTATE where a context buffer selected that way was never written; SF_EINVAL for an ambient
   outside [0, 1] or NaN, n or lights as above, or a weight that is negative or NaN. Asynchronous on the stream.
   sphereflake_amd/lights.py: light_model_many. */
int sf_light_image_many(sf_ctx* ctx, const sf_shadows_params* params, float ambient, const float* pos4,
                        const float* nrm4, const uint64_t* mask, uint8_t* rgba);

/* --- the level of detail of the shadow traces -------------------------------- */
/* THE LEVEL OF DETAIL IS THE LIGHT'S (above) because a shadow ray refines a node while sqrtf(t / r) < C with t measured
   from the ray's origin and C the variant's constant (70 AVX, 60 SSE). This sets C for the shadow traces -- and for
   them only: sf_trace_shadow(_to), sf_trace_shadows(_to), sf_trace_sun(_to), sf_trace_suns(_to) and
   sf_trace_shafts(_to). In their definitions "the reference's ray" then reads "the reference's ray with C in place of the variant's constant in
   sqrtf(t / r) < C || t < 0 (Sphereflake.h:146, SSE :129)"; the oracle takes the same constant
   (sfo_set_lod_constant). C == 0 (the default) means the variant's own, so a context that never calls this traces
   what it always traced. Renders, sf_trace_dirs_to, sf_trace_rays_to, the frame-less mode and the multi-GPU paths keep
   the variant's constant whatever is set here.
   A ray refined with C sees what a viewer (C / C_variant)^2 times nearer would: to give a light at distance D from a
   surface the detail the camera has at distance t_ref, C = C_variant sqrt(D / t_ref)
   (sphereflake_amd/lights.py: matched_lod). Synchronous (drains the context, as sf_set_variant does). SF_EINVAL for a
   NaN, negative or infinite C. A larger C goes deeper: levels beyond SF_MAX_DEPTH_LIMIT are not traced. */
int sf_set_shadow_lod(sf_ctx* ctx, float lod_constant);
float sf_get_shadow_lod(const sf_ctx* ctx);   /* the value set (0 = the variant's own); NaN for a null ctx */

/* --- shadows from a directional light ---------------------------------------- */
/* A sun: every shadow ray is parallel to s, the direction TOWARDS the light (the reference's one directional light is
   lightDir = (0.7, 0.7, 0.2), Shaders/post_final.glsl:11). A point light placed far off is no substitute: its level
   of detail falls with its distance, and so does the precision of the light-relative centres. Here pixel p's ray
   starts at its own origin F, a fixed distance tau up the sun direction from its own surface point, and runs down to
   it: the mixed-origin traversal of sf_trace_rays_to, in an any-hit mode, fused with the read of the position image.
   DEFINITION (exact). Inputs: a position image pos4 and its origin o as for sf_trace_shadow_to, s = dir (used AS
   GIVEN: not normalised here -- sphereflake_amd/lights.py sun_direction normalises), tau = distance, a relative bias b
   in [0, 1). All arithmetic is binary32, round to nearest, every operation rounded on its own (no fused
   multiply-add). For pixel p with P = pos4[p].xyz:
     1. P == (0, 0, 0) is a miss of the frame: vis[p] = 255, no ray.
     2. w = o + P per component; f = s tau per component; F = w + f per component.
     3. d = (w - F) + 0.0f per component; len = sqrt((d.x d.x + d.y d.y) + d.z d.z), correctly rounded;
        bound = len (1.0f - b).
     4. The ray is sf_trace_rays_to's ray from the origin F with direction Normalize(d): the root transform's columns
        0..2 are the context's, its column 3 is 0 - F; the context's child frames and variant; the shadow LOD constant
        (sf_set_shadow_lod).
     5. With m the min_t of that ray: vis[p] = (m < bound) ? 0 : 255.
     6. A d that does not normalise to finite numbers, or an F that is not finite (a non-finite or zero dir among
        them), misses the root: vis[p] = 255.
   sphereflake_amd/lights.py (sun_model) states steps 1-3 on the host.
   CONSEQUENCES:
   - tau >= 4 puts every F outside the flake's bounding ball (radius 2; |w| <= 2 for a surface point and |s| = 1), where
     THE REFERENCE'S QUIRK cannot bite. A smaller tau gets the reference's answer, quirk included.
   - THE LEVEL OF DETAIL IS THAT OF A VIEWER AT DISTANCE tau from each surface point -- the same for every pixel, and
     the caller's choice. sf_set_shadow_lod with matched_lod(tau, t_ref) makes it the camera's at camera distance t_ref
     (e.g. sf_get_stats' closest).
   - Self-shadow acne is governed by the bias, as for sf_trace_shadow_to. */
typedef struct sf_sun_params {
    float dir[3];             /* s, towards the sun, world space, as given */
    float distance;           /* tau, finite and > 0 (sf_sun_defaults: 4) */
    float bias;               /* as sf_shadow_params.bias */
    float origin[3];          /* as sf_shadow_params.origin */
    uint32_t use_origin;      /* as sf_shadow_params.use_origin */
    uint32_t width, height;   /* as sf_shadow_params */
    uint32_t max_depth;       /* levels to provision; 0 = 12, as sf_rays_params.max_depth (the rays have no common
                                 origin to bound them from); flagged tiles are re-traced at SF_MAX_DEPTH_LIMIT */
    void* stream;             /* NULL = the context stream */
} sf_sun_params;

/* dir (0, 0, 1), distance 4, the default bias of sf_shadow_defaults, the rest zero. */
int sf_sun_defaults(const sf_ctx* ctx, sf_sun_params* params);
/* As sf_trace_shadow_to in every respect but the light: pos4 DEVICE or NULL = the context's G-buffer, vis DEVICE
   width * height bytes, asynchronous on the stream and ordered with the context's other calls, no statistic and none
   of the renders' state touched, re-traced tiles counted in overflow_tiles. Errors as sf_trace_shadow_to's, and
   SF_EINVAL for a distance that is not finite and > 0. */
int sf_trace_sun_to(sf_ctx* ctx, const sf_sun_params* params, const float* pos4, uint8_t* vis);
/* The context's G-buffer into the context's visibility buffer -- the one sf_trace_shadow writes: sf_download_shadow
   and sf_shadow_buffer serve both. */
int sf_trace_sun(sf_ctx* ctx, const sf_sun_params* params);
/* sf_light_image for a sun: identical but for lam = max(0, (n.x s.x + n.y s.y) + n.z s.z) (0 where that is NaN) --
   no light position, no division. params: dir, stream. sphereflake_amd/lights.py: light_model_sun. */
int sf_light_image_sun(sf_ctx* ctx, const sf_sun_params* params, float ambient, const float* pos4, const float* nrm4,
                       const uint8_t* vis, uint8_t* rgba);

/* --- many sun directions per pixel: a soft sun, a sky dome ------------------- */
/* Extends sf_trace_sun_to from one direction to n <= SF_SUN_DIRS_MAX directions in ONE launch, as sf_trace_shadows_to
   extends sf_trace_shadow_to: a sun with an angular size sampled at n directions inside its cone (a penumbra), or n
   directions over the upper hemisphere as a sky-dome occlusion term of parallel rays. Each tile's wave loads its
   positions once and loops over the directions; one 64-bit word per pixel comes out instead of n byte images. Against
   a sky of point lights (sf_trace_shadows_to with lights.sky) every pixel and every direction gets THE SAME LEVEL OF
   DETAIL, that of a viewer at distance tau, and with tau >= 4 no ray starts inside the radius-2 ball.
   DEFINITION OF THE MASK (exact). Bit i (i < n) of mask[p] is 1 iff sf_trace_sun_to with dir = dirs[i] and the same
   distance, bias, origin, sizes, position image and shadow LOD constant writes 255 at p, and 0 iff it writes 0: steps
   1-6 of its definition apply per direction, unchanged, with f_i = s_i tau per component (one rounding, formed on the
   host). Bits n..63 are 0. So a miss of the frame (P == 0) has its low n bits all set, and a direction that is zero
   or not finite sets its own bit everywhere and leaves the other directions' bits alone. */
#define SF_SUN_DIRS_MAX 64
typedef struct sf_suns_params {
    const float* dirs;        /* HOST, n x 3 floats, towards the sun, used as given; read before the call returns */
    const float* weights;     /* HOST, n floats, or NULL = every weight (float)1 / (float)n; sf_light_image_suns only */
    uint32_t n;               /* 1 .. SF_SUN_DIRS_MAX */
    float distance;           /* tau, finite and > 0 (sf_suns_defaults: 4); one distance for all directions */
    float bias;               /* as sf_sun_params.bias; one bias for all directions */
    float origin[3];          /* as sf_sun_params.origin */
    uint32_t use_origin;      /* as sf_sun_params.use_origin */
    uint32_t width, height;   /* as sf_sun_params */
    uint32_t max_depth;       /* 0 = 12, as sf_sun_params.max_depth */
    void* stream;             /* NULL = the context stream */
} sf_suns_params;

/* Zeroed (n = 0, dirs NULL: the caller sets both), distance 4, the default bias of sf_shadow_defaults. */
int sf_suns_defaults(const sf_ctx* ctx, sf_suns_params* params);
/* As sf_trace_sun_to (pos4 DEVICE or NULL = the context's G-buffer; asynchronous and ordered as it is; no statistic and
   none of the renders' state touched; re-traced tiles -- a tile flagged for any direction is re-traced once, for all
   of them -- count in overflow_tiles). mask: DEVICE output, width * height uint64_t, row-major as pos4. Errors as
   sf_trace_sun_to's, and SF_EINVAL for n == 0, n > SF_SUN_DIRS_MAX, a null dirs or a null mask. */
int sf_trace_suns_to(sf_ctx* ctx, const sf_suns_params* params, const float* pos4, uint64_t* mask);
/* The context's G-buffer into the context's mask buffer -- the one sf_trace_shadows writes: sf_download_shadow_masks
   and sf_shadow_mask_buffer serve both, as the visibility buffer serves sf_trace_shadow and sf_trace_sun. */
int sf_trace_suns(sf_ctx* ctx, const sf_suns_params* params);
/* sf_light_image_many for sun directions: identical but for lam_i, which is sf_light_image_sun's for dirs[i]:
   lam_i = max(0, (n.x s.x + n.y s.y) + n.z s.z) (0 where that is NaN) -- no light position, no division. Exact,
   binary32, one rounding per operation, no fma: a frame miss is left untouched; else S = 0, then for i = 0 .. n-1 in
   that order S = S + w_i (bit i of mask[p] ? lam_i : 0); k = ambient + (1 - ambient) S, and each of r, g, b becomes
   (uint8) min(c k + 0.5f, 255); alpha stays. S is not clamped: with n = 1 and weight 1 the result is
   sf_light_image_sun's, byte for byte. params: dirs, weights, n, stream. NULL pos4 / nrm4 / mask / rgba select the
   context's G-buffer, mask buffer and image; SF_ESTATE where a context buffer selected that way was never written;
   SF_EINVAL for an ambient outside [0, 1] or NaN, n or dirs as above, or a weight that is negative or NaN.
   Asynchronous on the stream. sphereflake_amd/lights.py: light_model_suns; sun_cone and sky_dirs make directions. */
int sf_light_image_suns(sf_ctx* ctx, const sf_suns_params* params, float ambient, const float* pos4,
                        const float* nrm4, const uint64_t* mask, uint8_t* rgba);

/* --- light shafts: sun visibility along each pixel's view ray ----------------- */
/* The calls above all ask "is this surface point lit?". This one asks it of the air between the camera and the
   surface: n <= SF_SHAFT_SAMPLES_MAX points along each pixel's view ray, from the position image's origin to the
   pixel's surface point (or, for a miss of the frame, to a point `far` along a caller's direction), each tested against
   the sun in ONE launch. Light that passes the gaps of the flake leaves shafts in front of it and on the background.
   Each tile's wave loads its pixel once and loops over the samples; one 64-bit word per pixel comes out.
   DEFINITION OF THE MASK (exact; binary32, round to nearest, every operation rounded on its own, no fused
   multiply-add). Inputs: a position image pos4 and its origin o as for sf_trace_sun_to; the sun s = dir (as given),
   tau = distance, the bias and the shadow LOD constant (sf_set_shadow_lod); the march fractions sigma_0 .. sigma_{n-1};
   optionally a direction image dirs and a distance far. For pixel p with P = pos4[p].xyz:
     1. The march end E = P where P != (0, 0, 0); where P == 0, dirs is not NULL and far > 0,
        E = (dirs[p].x far, dirs[p].y far, dirs[p].z far), one rounding each; otherwise E = 0.
     2. For i < n the sample Q_i = (E.x sigma_i, E.y sigma_i, E.z sigma_i), one rounding each.
     3. Bit i of mask[p] is 1 iff sf_trace_sun_to with the same dir, distance, bias, origin and shadow LOD constant
        writes 255 at a pixel whose position is Q_i, and 0 iff it writes 0: steps 1-6 of its definition apply
        unchanged. So Q_i == 0 (E == 0, or a product that underflows) sets the bit without a ray, and a zero or
        non-finite dir sets every bit.
     4. Bits n..63 are 0.
   CONSEQUENCES:
   - A sample with sigma_i == 1 is the surface point itself: its bit is exactly sf_trace_sun_to's byte.
   - THE REFERENCE'S QUIRK cannot bite when every ray's origin o + Q_i + s tau lies outside the radius-2 ball;
     tau >= 2 + max |o + E| guarantees that (for |s| = 1 and fractions <= 1; sphereflake_amd/lights.py: shaft_distance).
   - THE LEVEL OF DETAIL IS THAT OF A VIEWER AT DISTANCE tau, so a larger tau is coarser; sf_set_shadow_lod with
     matched_lod corrects this, as for sf_trace_sun_to.
   sphereflake_amd/lights.py states steps 1-2 on the host (shaft_ends, shafts_model). */
#define SF_SHAFT_SAMPLES_MAX 64
typedef struct sf_shafts_params {
    float dir[3];             /* s, towards the sun, world space, as given */
    float distance;           /* tau, finite and > 0 (sf_shafts_defaults: 4) */
    float bias;               /* as sf_sun_params.bias */
    const float* fractions;   /* HOST, n floats, each finite and > 0; read before the call returns */
    const float* weights;     /* HOST, n floats, or NULL = every weight (float)1 / (float)n; the image pass only */
    uint32_t n;               /* 1 .. SF_SHAFT_SAMPLES_MAX */
    const float* dirs;        /* DEVICE, width * height directions for the frame's misses, used as given (not
                                 normalised), or NULL = a miss is not marched */
    uint32_t dirs_stride;     /* floats per pixel of dirs: 3 or 4 */
    float far;                /* how far a miss is marched along its direction; finite and >= 0, 0 = not marched */
    float origin[3];          /* as sf_sun_params.origin */
    uint32_t use_origin;      /* as sf_sun_params.use_origin */
    uint32_t width, height;   /* as sf_sun_params */
    uint32_t max_depth;       /* 0 = 12, as sf_sun_params.max_depth */
    void* stream;             /* NULL = the context stream */
} sf_shafts_params;

/* dir (0, 0, 1), distance 4, the default bias of sf_shadow_defaults, the rest zero (n = 0, fractions NULL: the caller
   sets both). */
int sf_shafts_defaults(const sf_ctx* ctx, sf_shafts_params* params);
/* As sf_trace_suns_to (pos4 DEVICE or NULL = the context's G-buffer; asynchronous and ordered as it is; no statistic
   and none of the renders' state touched; re-traced tiles -- a tile flagged for any sample is re-traced once, for all of
   them -- count in overflow_tiles). mask: DEVICE output, width * height uint64_t, row-major as pos4. Errors as
   sf_trace_suns_to's, and SF_EINVAL for n == 0, n > SF_SHAFT_SAMPLES_MAX, a null fractions, a fraction that is not
   finite and > 0, a far that is negative, infinite or NaN, or a dirs_stride other than 3 or 4 with a non-null dirs. */
int sf_trace_shafts_to(sf_ctx* ctx, const sf_shafts_params* params, const float* pos4, uint64_t* mask);
/* The context's G-buffer into the context's mask buffer -- the one sf_trace_shadows and sf_trace_suns write:
   sf_download_shadow_masks and sf_shadow_mask_buffer serve it. */
int sf_trace_shafts(sf_ctx* ctx, const sf_shafts_params* params);
/* The in-scatter pass: blends the image of sf_post towards `colour` (r, g, b in [0, 255]) where the march was lit.
   Exact, binary32, one rounding per operation, no fma. Per pixel, with E as in step 1 above: a pixel with E == 0 is
   left untouched; else len = sqrt((E.x E.x + E.y E.y) + E.z E.z), correctly rounded; S = 0, then for i = 0 .. n-1 in
   that order S = S + (bit i of mask[p] ? w_i : 0); a = min((gain len) S, 1), and 0 where that is NaN; each of r, g,
   b with float value c becomes (uint8) min((c + (colour_c - c) a) + 0.5f, 255); alpha stays. Unlike the other image
   passes it does touch the frame's misses, where they were marched. params: fractions (for n only), weights, n, dirs,
   dirs_stride, far, stream. NULL pos4 / mask / rgba select the context's G-buffer, mask buffer and image; SF_ESTATE
   where a context buffer selected that way was never written; SF_EINVAL for n, fractions, far or dirs_stride as
   above, a gain that is negative, infinite or NaN, a colour component outside [0, 255] or NaN, or a weight that is
   negative or NaN. Asynchronous on the stream. sphereflake_amd/lights.py: light_model_shafts. */
int sf_light_image_shafts(sf_ctx* ctx, const sf_shafts_params* params, float gain, const float colour[3],
                          const float* pos4, const uint64_t* mask, uint8_t* rgba);

/* --- the colour light buffer: sum any number of suns and lights while tracing -- */
/* The image passes above each MULTIPLY the 8-bit image in place, so a second call cannot add a light, a launch stops at
   64 entries, and a weight is one grey float. The light buffer removes all three limits: a width x height image of
   float4 (row-major as the G-buffer; .xyz the RGB irradiance factor, .w reserved: written 0 by an overwriting call and
   carried through by an accumulating one) that the two summing traces below ADD into while they trace, each entry with
   its own RGB colour, and that sf_light_image_buffer applies to the image once, at the end. The context owns one,
   allocated on first use; a caller's DEVICE buffer of width * height * 4 floats (16-byte aligned) serves as well.
   DEFINITION OF THE SUM (exact; binary32, round to nearest, every operation rounded on its own, no fused
   multiply-add). For pixel p with P = pos4[p].xyz and N = nrm4[p].xyz:
     1. base = accumulate ? out[p] : (0, 0, 0, 0).
     2. P == (0, 0, 0) is a miss of the frame: an accumulating call does not write out[p], an overwriting call writes
        (0, 0, 0, 0).
     3. Otherwise S = base.xyz, and then for i = 0 .. n-1 IN THAT ORDER, per channel c,
        S.c = S.c + colours[i].c (lit_i ? lam_i : 0). lit_i is bit i as sf_trace_suns_to (sf_trace_shadows_to) defines
        it for entry i alone, with the same distance, bias, origin, position image and shadow LOD constant: an entry
        that traces no ray -- a zero or non-finite direction or light -- is lit. lam_i is exactly the term of
        sf_light_image_suns, max(0, (N.x s.x + N.y s.y) + N.z s.z), or of sf_light_image_many, max(0, dot / len) with
        dot and len as sf_light_image forms them; 0 where that is NaN.
     4. out[p] = (S, base.w).
   CONSEQUENCES, both bit for bit:
   - A call with n entries equals an overwriting call with the first k followed by an accumulating call with the rest,
     for every k. That is how n > 64 is carried out: one launch per 64 entries on the stream.
   - The result equals the host sum over the masks that sf_trace_suns_to (sf_trace_shadows_to) gives for consecutive
     chunks of 64 entries (sphereflake_amd/lights.py: sum_model).
   With one overwriting sf_trace_suns_sum of n <= 64 directions and colours (w_i, w_i, w_i), sf_light_image_buffer makes
   the image of sf_light_image_suns with ambient 0, byte for byte (0 + (1 - 0) S is S); likewise the point lights and
   sf_light_image_many. */
#define SF_LIGHT_SUM_MAX 65536
typedef struct sf_light_sum_params {
    const float* points;      /* HOST, n x 3 floats: directions towards the sun (the suns call) or light positions (the
                                 shadows call), world space, used as given; read before the call returns */
    const float* colours;     /* HOST, n x 3 floats (r, g, b per entry), each finite and >= 0, or NULL = every
                                 component (float)1 / (float)n; read before the call returns */
    uint32_t n;               /* 1 .. SF_LIGHT_SUM_MAX */
    uint32_t accumulate;      /* 0 = overwrite the output, 1 = add to what it holds */
    float distance;           /* tau, the suns call only: as sf_suns_params.distance (sf_light_sum_defaults: 4) */
    float bias;               /* as sf_suns_params.bias / sf_shadows_params.bias */
    float origin[3];          /* as sf_sun_params.origin */
    uint32_t use_origin;      /* as sf_sun_params.use_origin */
    uint32_t width, height;   /* as sf_sun_params */
    uint32_t max_depth;       /* as sf_suns_params.max_depth / sf_shadows_params.max_depth */
    void* stream;             /* NULL = the context stream */
} sf_light_sum_params;

/* Zeroed (n = 0, points NULL: the caller sets both; overwriting), distance 4, the default bias of sf_shadow_defaults. */
int sf_light_sum_defaults(const sf_ctx* ctx, sf_light_sum_params* params);
/* The sum over sun directions. pos4, nrm4 and out are DEVICE pointers; NULL selects the context's G-buffer (positions,
   normals) and light buffer, at the context's size only. Asynchronous on the stream and ordered with the context's
   other calls; one launch pair per 64 entries; no statistic and none of the renders' state touched; re-traced tiles
   count in overflow_tiles once per launch that re-traced them. SF_EINVAL for n == 0, n > SF_LIGHT_SUM_MAX, a null
   points, a colour component that is negative, infinite or NaN, and everything sf_trace_suns_to rejects; SF_ESTATE
   for a null out before anything has written the context's light buffer. A failing call writes nothing. */
int sf_trace_suns_sum_to(sf_ctx* ctx, const sf_light_sum_params* params, const float* pos4, const float* nrm4,
                         float* out);
/* The context's G-buffer into the context's light buffer, which an overwriting call allocates on first use
   (SF_ESTATE for an accumulating call before anything has written it). */
int sf_trace_suns_sum(sf_ctx* ctx, const sf_light_sum_params* params);
/* The same for point lights: points are light positions, lit_i and lam_i those of sf_trace_shadows_to and
   sf_light_image_many; distance is not used. Errors as above, with sf_trace_shadows_to's in place of
   sf_trace_suns_to's. */
int sf_trace_shadows_sum_to(sf_ctx* ctx, const sf_light_sum_params* params, const float* pos4, const float* nrm4,
                            float* out);
int sf_trace_shadows_sum(sf_ctx* ctx, const sf_light_sum_params* params);
/* The ambient term: every pixel of buf (DEVICE, NULL = the context's light buffer, allocated here on first use) becomes
   (r, g, b, 0). Asynchronous on the stream (NULL = the context stream). SF_EINVAL for a component that is negative,
   infinite or NaN. */
int sf_light_fill(sf_ctx* ctx, const float rgb[3], float* buf, void* stream);
/* The context's light buffer (DEVICE), and a synchronous copy of it to width * height * 4 HOST floats. SF_ESTATE before
   anything has written it. */
int sf_light_buffer(sf_ctx* ctx, float** buf);
int sf_download_light(sf_ctx* ctx, float* buf4);
/* The resolve pass: what the sf_light_image passes are to a mask, for the buffer. A frame miss (P == 0) is left
   untouched; else with E = buf[p] each of r, g, b with float value c becomes (uint8) min(c E.c + 0.5f, 255), one
   rounding per operation; alpha stays. NULL pos4 / buf / rgba select the context's G-buffer, light buffer and image;
   SF_ESTATE where a context buffer selected that way was never written. Asynchronous on the stream (NULL = the
   context stream). sphereflake_amd/lights.py: light_model_buffer. */
int sf_light_image_buffer(sf_ctx* ctx, void* stream, const float* pos4, const float* buf, uint8_t* rgba);

/* --- ambient occlusion about each pixel's normal ------------------------------ */
/* The directions of sf_trace_suns_to are fixed in the world: under a sky dome a surface that faces down or sideways
   spends half its samples behind its own tangent plane, and no pixel gets the cosine weighting of its own normal.
   Here the n <= SF_AO_SAMPLES_MAX directions are given in a LOCAL frame and each pixel turns them about its own
   normal: n rays over the hemisphere about N, in ONE launch. Each tile's wave loads its positions and normals once,
   forms each lane's frame once (one division per pixel) and loops over the samples; one 64-bit word per pixel comes
   out, or, from the summing call, a sum in the light buffer. The rays are posed as the sun's are: from a point tau up
   the direction, down to the surface point.
   DEFINITION OF THE MASK (exact; binary32, round to nearest, every operation rounded on its own, no fused
   multiply-add). Inputs: a position image pos4 and a normal image nrm4, and the origin o as for sf_trace_sun_to; n
   local-frame samples h_i = (h.x, h.y, h.z), given on the host and used AS GIVEN (sphereflake_amd/lights.py
   ao_samples makes unit ones with h.z > 0); tau = distance, the bias b and the shadow LOD constant
   (sf_set_shadow_lod). For pixel p with P = pos4[p].xyz and N = nrm4[p].xyz (as given, not normalised):
     1. P == (0, 0, 0) is a miss of the frame: no ray is traced and every bit i < n is set.
     2. The frame about N is the branch-free one of Duff et al. ("Building an Orthonormal Basis, Revisited", 2017):
        sg = copysignf(1, N.z); a = -1 / (sg + N.z), a correctly rounded division; b = (N.x N.y) a;
        T = (1 + sg ((N.x N.x) a), sg b, -sg N.x); B = (b, sg + (N.y N.y) a, -N.y). Products by sg and negations are
        exact, so only the order written matters.
     3. Per component c, s_i.c = ((T.c h_i.x) + (B.c h_i.y)) + (N.c h_i.z); per component, f_i.c = s_i.c tau.
     4. Steps 2-6 of sf_trace_sun_to's definition follow with this f_i: w = o + P, F = w + f_i, d = (w - F) + 0.0f,
        bound = |d| (1.0f - b); the ray is sf_trace_rays_to's ray from F along Normalize(d); bit i is 0 iff its
        min_t < bound. A d or an F that is not finite sets the bit without a ray: a NaN or infinite sample or normal
        component is such a case, and so is a zero sample.
     5. Bits n..63 are 0.
   CONSEQUENCES:
   - h = (0, 0, 1) gives s = N exactly.
   - A normal image that holds one constant N0 gives, bit for bit, sf_trace_suns_to with dirs[i] = s_i(N0): the one
     product s tau is formed on the host there and on the device here, and is the same rounding
     (sphereflake_amd/lights.py: ao_directions).
   - tau >= 4 keeps every ray's origin outside the flake's radius-2 ball for |N| = |h| = 1, where THE REFERENCE'S QUIRK
     cannot bite.
   - THE LEVEL OF DETAIL IS THAT OF A VIEWER AT DISTANCE tau, the caller's through sf_set_shadow_lod, as for
     sf_trace_sun_to.
   sphereflake_amd/lights.py states steps 1-4 on the host (ao_basis, ao_directions, ao_model). */
#define SF_AO_SAMPLES_MAX 64
typedef struct sf_ao_params {
    const float* samples;     /* HOST, n x 3 floats: the samples in the frame about the normal (z along it), used as
                                 given; read before the call returns */
    const float* colours;     /* HOST, n x 3 floats (r, g, b per sample), each finite and >= 0, or NULL = every
                                 component (float)1 / (float)n; the summing call only; read before the call returns */
    uint32_t n;               /* 1 .. SF_AO_SAMPLES_MAX */
    uint32_t accumulate;      /* the summing call only: 0 = overwrite the output, 1 = add to what it holds */
    float distance;           /* tau, finite and > 0 (sf_ao_defaults: 4); one distance for all samples */
    float bias;               /* as sf_sun_params.bias; one bias for all samples */
    float origin[3];          /* as sf_sun_params.origin */
    uint32_t use_origin;      /* as sf_sun_params.use_origin */
    uint32_t width, height;   /* as sf_sun_params */
    uint32_t max_depth;       /* 0 = 12, as sf_sun_params.max_depth */
    void* stream;             /* NULL = the context stream */
} sf_ao_params;

/* Zeroed (n = 0, samples NULL: the caller sets both; overwriting), distance 4, the default bias of
   sf_shadow_defaults. */
int sf_ao_defaults(const sf_ctx* ctx, sf_ao_params* params);
/* As sf_trace_suns_to (asynchronous on the stream and ordered as it is; no statistic and none of the renders' state
   touched; re-traced tiles -- a tile flagged for any sample is re-traced once, for all of them -- count in
   overflow_tiles). pos4 and nrm4 are DEVICE images of width * height float4; NULL selects the context's G-buffer, at
   the context's size only. mask: DEVICE output, width * height uint64_t, row-major as pos4. Errors as
   sf_trace_suns_to's, and SF_EINVAL for n == 0, n > SF_AO_SAMPLES_MAX, a null samples or a null mask. A failing call
   writes nothing. */
int sf_trace_ao_to(sf_ctx* ctx, const sf_ao_params* params, const float* pos4, const float* nrm4, uint64_t* mask);
/* The context's G-buffer into the context's mask buffer -- the one sf_trace_shadows, sf_trace_suns and sf_trace_shafts
   write: sf_download_shadow_masks and sf_shadow_mask_buffer serve it. */
int sf_trace_ao(sf_ctx* ctx, const sf_ao_params* params);
/* The sum into the light buffer: steps 1-4 of the DEFINITION OF THE SUM above, unchanged, with lit_i the bit defined
   here and lam_i = 1: S.c = S.c + colours[i].c (lit_i ? 1.0f : 0.0f) in index order -- the weighting lives in the
   sample set and the colours (sphereflake_amd/lights.py: ao_colours, ao_sum_model). It overwrites or accumulates,
   handles a miss of the frame and carries .w exactly as sf_trace_suns_sum_to does, and a call equals its split into an
   overwriting and an accumulating call at any k. n <= SF_AO_SAMPLES_MAX per call: more samples are further
   accumulating calls. pos4, nrm4 and out as sf_trace_suns_sum_to's; errors as sf_trace_ao_to's and
   sf_trace_suns_sum_to's (a colour component that is negative, infinite or NaN: SF_EINVAL; a null out before anything
   has written the context's light buffer: SF_ESTATE). A failing call writes nothing. */
int sf_trace_ao_sum_to(sf_ctx* ctx, const sf_ao_params* params, const float* pos4, const float* nrm4, float* out);
/* The context's G-buffer into the context's light buffer, which an overwriting call allocates on first use
   (SF_ESTATE for an accumulating call before anything has written it). */
int sf_trace_ao_sum(sf_ctx* ctx, const sf_ao_params* params);

/* --- fewer rays per pixel: a per-pixel spin and an edge-aware filter of the light buffer ---- */
/* sf_trace_ao_to gives every pixel the same sample set, so a small n shows as banding. Interleaved sampling spreads
   a small n over neighbouring pixels and gathers it back: each pixel of a size x size block turns the shared sample
   set by its own angle about its normal, so a block sees n size^2 directions, and sf_light_filter_to then averages the
   block, stopped at normal and plane discontinuities.
   DEFINITION OF THE SPUN MASK (exact; binary32, round to nearest, every operation rounded on its own, no fused
   multiply-add). Steps 1-5 of sf_trace_ao_to's definition hold. Between step 2 and step 3, with (c, s) the table entry
   of pixel (x, y) -- x the column and y the row of the image the call is given (width x height of the params, or the
   context's frame) -- per component k:
       T'.k = (T.k c) + (B.k s)        B'.k = (B.k c) - (T.k s)
   and step 3 uses T' and B'. The frame is turned ONCE PER PIXEL, not once per sample. (c, s) is used as given: it is
   not normalised, and cos and sin of an angle make the turn a rotation about N.
   CONSEQUENCES, all bit for bit:
   - The 1 x 1 table {(1, 0)} gives sf_trace_ao_to's mask and sf_trace_ao_sum_to's sum. T' = T + (B 0) and
     B' = B - (T 0) differ from T and B in the sign of a zero at most, and no later step sees it: F = w + f and the
     root centre 0 - F carry no sign of a zero f that matters, and d = (w - F) + 0.0f has none.
   - A table whose entries are all equal gives the 1 x 1 table's result.
   - A constant normal N0 with a 1 x 1 table (c, s) gives sf_trace_suns_to's bits for the directions
     sphereflake_amd/lights.py ao_directions(N0, samples, spin=(c, s)).
   - A crop of the images whose top-left corner is at multiples of `size` gives the crop of the whole's result. */
#define SF_AO_SPIN_MAX 8
typedef struct sf_ao_spin {
    const float* cs;   /* HOST, size x size x 2 floats, row-major: (c, s) of pixel (x, y) is entry
                          (y % size) * size + (x % size); used as given, not normalised; every value finite; read
                          before the call returns */
    uint32_t size;     /* 1 .. SF_AO_SPIN_MAX */
} sf_ao_spin;
/* sf_trace_ao_to, sf_trace_ao, sf_trace_ao_sum_to and sf_trace_ao_sum with the spin: everything after the spin argument
   is as in the unspun call, and so are the buffers, the ordering, the statistics and the re-trace. The summing calls
   are sf_trace_ao_sum_to's definition with the spun bit: a call equals its split at any k, a flagged tile stores
   nothing in its first pass, .w and the frame's misses are handled the same way. Errors: everything the unspun call
   rejects, and SF_EINVAL for a null spin, a null cs, a size of 0 or above SF_AO_SPIN_MAX, or a table value that is not
   finite. A failing call writes nothing. */
int sf_trace_ao_spin_to(sf_ctx* ctx, const sf_ao_params* params, const sf_ao_spin* spin, const float* pos4,
                        const float* nrm4, uint64_t* mask);
int sf_trace_ao_spin(sf_ctx* ctx, const sf_ao_params* params, const sf_ao_spin* spin);
int sf_trace_ao_spin_sum_to(sf_ctx* ctx, const sf_ao_params* params, const sf_ao_spin* spin, const float* pos4,
                            const float* nrm4, float* out);
int sf_trace_ao_spin_sum(sf_ctx* ctx, const sf_ao_params* params, const sf_ao_spin* spin);

/* The filter: an R x R box over the light buffer that accepts a neighbour only on the same surface.
   DEFINITION (exact, as above). For pixel p = (x, y) with P_p = pos4[p].xyz and N_p = nrm4[p].xyz:
     1. P_p == (0, 0, 0) is a miss of the frame: out[p] = in[p].
     2. Else the taps q = (x + dx, y + dy) are visited with dy outer and dx inner, both from -floor(R / 2) to
        R - 1 - floor(R / 2) (-2 .. +1 for R = 4): any such window holds every entry of an R x R spin table once.
     3. A tap outside the image, or one that is a miss of the frame, is skipped. The tap q == p is always accepted. Any
        other tap is accepted iff nn >= normal_min, with nn = ((N_p.x N_q.x) + (N_p.y N_q.y)) + (N_p.z N_q.z), and
        (e e) <= (k2 pp), with D = P_q - P_p per component, e = ((N_p.x D.x) + (N_p.y D.y)) + (N_p.z D.z),
        pp = ((P_p.x P_p.x) + (P_p.y P_p.y)) + (P_p.z P_p.z) and k2 = plane_max plane_max formed on the host in
        binary32. A comparison with a NaN is false: that tap is rejected.
     4. Per channel S starts at 0 and an accepted tap does S = S + in[q].c, in visiting order; a rejected tap leaves S
        as it is. out[p].xyz = S / (float)count, a correctly rounded division; out[p].w = in[p].w.
   R = 1 is a copy. The defaults (0.9, 0.02) were picked from three candidates on an 80 x 45 fixture at n = 4; THEY ARE
   NOT TUNED AT 1920 x 1080. sphereflake_amd/lights.py: light_filter_model. */
typedef struct sf_light_filter_params {
    uint32_t size;          /* R, 1 .. SF_AO_SPIN_MAX: the window is R x R pixels (sf_light_filter_defaults: 4) */
    float normal_min;       /* a tap q is accepted only if N_p . N_q >= normal_min (defaults: 0.9f); not NaN */
    float plane_max;        /* ... and its distance from p's tangent plane <= plane_max |P_p| (defaults: 0.02f);
                               finite and >= 0 */
    uint32_t width, height; /* as sf_sun_params */
    void* stream;           /* NULL = the context stream */
} sf_light_filter_params;
int sf_light_filter_defaults(const sf_ctx* ctx, sf_light_filter_params* params);
/* pos4, nrm4, in and out are DEVICE images of width * height float4. NULL pos4 / nrm4 / in select the context's
   G-buffer and light buffer, at the context's size only (SF_ESTATE for a null `in` before anything has written the
   light buffer). Asynchronous on the stream and ordered with the context's other calls; no statistic is touched.
   SF_EINVAL for a null out, in == out (the context's light buffer included), a size of 0 or above SF_AO_SPIN_MAX, a NaN
   normal_min, a plane_max that is negative, infinite or NaN, and sizes as sf_trace_ao_to's. A failing call writes
   nothing. */
int sf_light_filter_to(sf_ctx* ctx, const sf_light_filter_params* params, const float* pos4, const float* nrm4,
                       const float* in, float* out);
/* The context's G-buffer and light buffer, in place for the caller: filtered into a second buffer the context owns
   (allocated on first use) and copied back on the stream, so the pointer sf_light_buffer returns never changes.
   SF_ESTATE before anything has written the light buffer. */
int sf_light_filter(sf_ctx* ctx, const sf_light_filter_params* params);

/* --- sky reflections: a lobe of rays about each pixel's mirror direction ----------------------- */
/* Every term above is diffuse: nothing depends on where the viewer stands. Here the axis the samples are turned about
   is the MIRROR DIRECTION of the pixel's view vector about its normal, formed on the device, and the summing call
   weighs each open ray by the sky's colour IN THAT RAY'S OWN WORLD DIRECTION. The rays are posed as AO's are -- from a
   point tau up the direction, down to the surface point, as an any-hit query -- so no ray starts on the flake, and
   the answer is "is this direction open to the sky?": a sky reflection with self-occlusion.
   DEFINITION OF THE MASK (exact; binary32, round to nearest, every operation rounded on its own, no fused
   multiply-add). Inputs: sf_trace_ao_to's (position image, normal image, origin o, n <= SF_AO_SAMPLES_MAX local-frame
   samples h_i used as given, tau, bias, the shadow LOD constant, optionally sf_trace_ao_spin_to's table) and an eye.
   For pixel p with P = pos4[p].xyz and N = nrm4[p].xyz (as given, not normalised):
     1. P == (0, 0, 0) is a miss of the frame: no ray is traced and every bit i < n is set.
     2. The view vector V: with use_eye == 0, V = P (the positions are relative to the viewer); otherwise
        V = (o + P) - eye per component. THESE ARE DIFFERENT BITS, even for eye == o: (o + P) - o is not P in binary32
        (on the 80 x 45 fixture it changes 3022 of 3600 axes in their last bits).
     3. The mirror axis A: nv = ((N.x V.x) + (N.y V.y)) + (N.z V.z); k = nv + nv; R.c = V.c - (k N.c);
        rr = ((R.x R.x) + (R.y R.y)) + (R.z R.z); len = sqrtf(rr), correctly rounded; A.c = R.c / len, a correctly
        rounded division.
     4. Steps 2-5 of sf_trace_ao_to's definition follow with A in place of N: the frame of Duff et al. about A; where a
        spin is given, the turn of sf_trace_ao_spin_to by the pixel's table entry; s_i.c = ((T.c h_i.x) + (B.c h_i.y))
        + (A.c h_i.z); f_i = s_i tau; F, d and bound as sf_trace_ao_to forms them; bit i is 0 iff min_t < bound; a d or
        an F that is not finite sets the bit without a ray -- a NaN normal and a zero-length R are such cases; bits
        n..63 are 0.
   DEFINITION OF THE SUM. Steps 1-4 of the DEFINITION OF THE SUM of sf_trace_suns_sum_to hold for the base, the misses
   of the frame, .w and the order. The term of entry i takes the sky's colour along s_i:
       u_i = ((s_i.x up.x) + (s_i.y up.y)) + (s_i.z up.z)
       t_i = min(max(u_i, 0), 1), and +0 where u_i is -0 or NaN
       E_i.c = horizon.c + ((zenith.c - horizon.c) t_i)
       S.c = S.c + (colours[i].c (open_i ? E_i.c : 0.0f))
   `up` is used as given, not normalised. open_i is bit i of the mask defined above. A closed direction adds
   colours[i].c 0.0f: the flake's own reflection is black.
   CONSEQUENCES, all bit for bit:
   - The mask equals sf_trace_ao_spin_to's mask (sf_trace_ao_to's without a spin) on a normal image that holds A
     (sphereflake_amd/lights.py: mirror_axes makes that image on the host).
   - With zenith == horizon == (1, 1, 1) the sum equals sf_trace_ao_spin_sum_to's (sf_trace_ao_sum_to's) on that
     image: E is exactly 1, and a closed entry adds colours 0, as there.
   - h = (0, 0, 1) gives s = A exactly, with or without a spin.
   - A call equals its split into an overwriting call with the first k entries and an accumulating call with the
     rest, for every k.
   - A flagged tile stores nothing in its first pass.
   - A crop of the images whose top-left corner is at multiples of the spin's `size` gives the crop of the whole's
     result.
   - tau >= 4 keeps every ray's origin outside the flake's radius-2 ball for |h| = 1 (|A| is 1 to rounding).
   WHAT THIS IS NOT: the flake does not reflect itself, there is no Fresnel term, and sf_light_image_buffer still
   multiplies the image by the buffer: c (diffuse + specular).
   sphereflake_amd/lights.py states all of it on the host (mirror_axes, mirror_model, sky_gradient, mirror_sum_model,
   lobe_samples). */
typedef struct sf_mirror_params {
    const float* samples;     /* as sf_ao_params.samples: the lobe about the mirror axis (z along it) */
    const float* colours;     /* as sf_ao_params.colours; the summing call only */
    uint32_t n;               /* 1 .. SF_AO_SAMPLES_MAX */
    uint32_t accumulate;      /* the summing call only: 0 = overwrite the output, 1 = add to what it holds */
    float distance;           /* tau, finite and > 0 (sf_mirror_defaults: 4) */
    float bias;               /* as sf_sun_params.bias */
    float origin[3];          /* as sf_sun_params.origin */
    uint32_t use_origin;      /* as sf_sun_params.use_origin */
    uint32_t width, height;   /* as sf_sun_params */
    uint32_t max_depth;       /* 0 = 12, as sf_sun_params.max_depth */
    void* stream;             /* NULL = the context stream */
    float eye[3];             /* the viewer, world space; read where use_eye != 0, then finite */
    uint32_t use_eye;         /* 0 = the view vector is P itself; 1 = (o + P) - eye */
    float zenith[3];          /* the sky's colour where s . up >= 1; each finite and >= 0; the summing call only */
    float horizon[3];         /* ... and where s . up <= 0 */
    float up[3];              /* used as given, not normalised; finite; the summing call only */
} sf_mirror_params;

/* Zeroed (n = 0, samples NULL: the caller sets both; overwriting; use_eye 0), distance 4, the default bias of
   sf_shadow_defaults, zenith = horizon = (1, 1, 1), up = (0, 0, 1). */
int sf_mirror_defaults(const sf_ctx* ctx, sf_mirror_params* params);
/* The four calls. spin NULL means unspun; otherwise as sf_trace_ao_spin_to's. The buffers (NULL pos4 / nrm4 select the
   context's G-buffer; the context's mask buffer and light buffer), the stream ordering, the statistics (none touched)
   and the re-trace accounting (a flagged tile is re-traced once for all samples and counts in overflow_tiles) are the
   spun AO calls'. Errors: everything sf_trace_ao_spin_to / sf_trace_ao_spin_sum_to rejects, with a NULL spin allowed;
   SF_EINVAL as well for an eye component that is not finite under use_eye, and, in the summing calls, a zenith or
   horizon component that is negative, infinite or NaN or an up component that is not finite. A failing call writes
   nothing. */
int sf_trace_mirror_to(sf_ctx* ctx, const sf_mirror_params* params, const sf_ao_spin* spin, const float* pos4,
                       const float* nrm4, uint64_t* mask);
int sf_trace_mirror(sf_ctx* ctx, const sf_mirror_params* params, const sf_ao_spin* spin);
int sf_trace_mirror_sum_to(sf_ctx* ctx, const sf_mirror_params* params, const sf_ao_spin* spin, const float* pos4,
                           const float* nrm4, float* out);
int sf_trace_mirror_sum(sf_ctx* ctx, const sf_mirror_params* params, const sf_ao_spin* spin);

/* --- the light buffer over several frames: reproject, test, blend ---------------------------- */
/* A camera that moves every frame starts every light trace from nothing. The flake is static, so the last frame's light
   buffer can be carried into the new view by geometry alone: a pixel's world point is taken back through the LAST
   view's ray generation to the pixel of the last frame it falls in, that pixel's light is kept where it lies on the same
   surface (sf_light_filter_to's test), and the new value is blended in. .w of the light buffer, which the traces and the
   filter only carry, counts the frames blended into a pixel.

   sf_reproject_matrix: the inverse of a view's ray generation. view is origin o, top-left tl, top-right tr, bottom-left
   bl (12 floats, as sf_set_view takes them). a = tr - tl, b = bl - tl and c = tl - o are formed in binary32, promoted
   to double and put as the COLUMNS of a 3 x 3 matrix; m is its inverse, row-major, adjugate over determinant in double,
   every operation rounded on its own (no fused multiply-add), in this order:
       bc = (b.y c.z - b.z c.y, b.z c.x - b.x c.z, b.x c.y - b.y c.x)
       ca = (c.y a.z - c.z a.y, c.z a.x - c.x a.z, c.x a.y - c.y a.x)
       ab = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x)
       det = ((a.x bc.x) + (a.y bc.y)) + (a.z bc.z)
       m[0..2] = bc / det     m[3..5] = ca / det     m[6..8] = ab / det
   and each entry rounded once to binary32. m (a u + b v + c) = (u, v, 1) to rounding: pixel (x, y) of a W x H frame
   looks along a u + b v + c with u = x / W and v = y / H, no half-pixel offset (sphereflake_amd/dirs.py pinhole), so
   for a point at D from the origin, q = m D gives the pixel coordinates (W q.x / q.z, H q.y / q.z) and q.z > 0 in front
   of the viewer. SF_EINVAL for a null pointer, an input that is not finite, or a determinant that is 0 or not finite;
   m is then not written. No context, no device. sphereflake_amd/lights.py: reproject_matrix. */
int sf_reproject_matrix(const float view[12], float m[9]);

/* DEFINITION OF THE ACCUMULATION (exact; binary32, round to nearest, every operation rounded on its own, no fused
   multiply-add). Inputs: the current frame's position image pos4, normal image nrm4 and light buffer `in`, relative to
   the origin o (origin / use_origin); the history's position image hist_pos4, normal image hist_nrm4 and light buffer
   hist, relative to o' = hist_origin, with m = hist_m the sf_reproject_matrix of the history's view, used AS GIVEN.
   For pixel p = (x, y) with P = pos4[p].xyz and N = nrm4[p].xyz:
     1. P == (0, 0, 0) is a miss of the frame: out[p] = (in[p].xyz, 0).
     2. w = o + P per component; D = w - o'; q.k = ((m[3k] D.x) + (m[3k+1] D.y)) + (m[3k+2] D.z) for k = 0, 1, 2.
     3. u = q.x / q.z and v = q.y / q.z, correctly rounded divisions; fx = (u (float)W) + 0.5f, fy = (v (float)H) + 0.5f;
        X = floorf(fx), Y = floorf(fy). The tap exists iff q.z > 0, 0 <= X < (float)W and 0 <= Y < (float)H. A
        comparison with a NaN is false.
     4. With t = (X, Y), P' = hist_pos4[t].xyz, N' = hist_nrm4[t].xyz and h = hist[t], the tap is accepted iff all of:
        P' != (0, 0, 0); h.w >= 1; nn >= normal_min, with nn = ((N.x N'.x) + (N.y N'.y)) + (N.z N'.z); and
        (e e) <= (k2 pp), with E = (o' + P') - w per component, e = ((N.x E.x) + (N.y E.y)) + (N.z E.z),
        pp = ((P.x P.x) + (P.y P.y)) + (P.z P.z) and k2 = plane_max plane_max formed on the host in binary32.
     5. Accepted: m = min(h.w + 1.0f, (float)max_history); per channel out.c = h.c + ((in.c - h.c) / m), a correctly
        rounded division; out.w = m. Otherwise out[p] = (in[p].xyz, 1).
   CONSEQUENCES:
   - A history whose .w is 0 everywhere (a fresh sf_light_fill) gives (in.xyz, 1) on every surface pixel: the first
     frame needs no special case.
   - With the history's view equal to the current one, t = p for every surface pixel (checked on the fixtures; the
     largest |fx - x - 0.5| seen is 0.001 at 1920 wide and 0.004 at 3840).
   - K calls from a still view with max_history >= K leave the running mean of the K inputs, rounded in the order of
     step 5, and .w = K.
   - Once .w has reached max_history the blend is an exponential average with weight 1 / max_history.
   - max_history = 1 gives h + (in - h), WHICH IS NOT `in` TO THE LAST BIT.
   - Only the term accumulated is carried: what is sharp (suns, shadows, shafts) is added per frame, after this call.
   The thresholds are sf_light_filter_to's and as little tuned. sphereflake_amd/lights.py: light_accumulate_model. */
typedef struct sf_light_accumulate_params {
    uint32_t max_history;   /* 1 .. 65535: the most frames a pixel's value stands for (sf_light_accumulate_defaults: 16) */
    float normal_min;       /* the tap is accepted only if N . N' >= normal_min (defaults: 0.9f); not NaN */
    float plane_max;        /* ... and its distance from p's tangent plane <= plane_max |P| (defaults: 0.02f); finite
                               and >= 0 */
    float origin[3];        /* as sf_sun_params.origin */
    uint32_t use_origin;    /* as sf_sun_params.use_origin */
    float hist_origin[3];   /* o': the origin the history's positions are relative to; finite */
    float hist_m[9];        /* sf_reproject_matrix of the history's view, used as given; finite */
    uint32_t width, height; /* as sf_sun_params */
    void* stream;           /* NULL = the context stream */
} sf_light_accumulate_params;
/* Zeroed, then max_history 16, normal_min 0.9f, plane_max 0.02f. */
int sf_light_accumulate_defaults(const sf_ctx* ctx, sf_light_accumulate_params* params);
/* All seven images are DEVICE images of width * height float4, none NULL. Asynchronous on the stream and ordered with the
   context's other calls; no statistic is touched. SF_EINVAL for a null image, an `out` that is one of the inputs, a
   max_history of 0 or above 65535, a NaN normal_min, a plane_max that is negative, infinite or NaN, a hist_m or
   hist_origin value that is not finite, and sizes as sf_trace_ao_to's; SF_ENOVIEW for use_origin == 0 before
   sf_set_view. A failing call writes nothing. */
int sf_light_accumulate_to(sf_ctx* ctx, const sf_light_accumulate_params* params, const float* pos4, const float* nrm4,
                           const float* in, const float* hist_pos4, const float* hist_nrm4, const float* hist,
                           float* out);
/* The context form: the context's G-buffer, light buffer and current view (sf_set_view's) against a history the context
   owns -- positions, normals, light, the view they belong to and a valid flag; made on first use, freed by sf_destroy.
   hist_*, origin and use_origin of the params are ignored, and width / height must be 0 or the context's. The result
   goes to the second buffer sf_light_filter keeps and is copied back, so the pointer sf_light_buffer returns never
   changes; positions, normals and the result are then copied into the history and the view recorded: four copies, all
   on the stream. Without a valid history (the first call, or after sf_light_history_reset) every surface pixel takes the
   "otherwise" branch of step 5. The history is a copy: a later in-place sf_light_filter, or further summing traces,
   do not reach it. SF_ENOVIEW before sf_set_view; SF_ESTATE before anything has written the light buffer; SF_EINVAL
   for a view sf_reproject_matrix rejects. */
int sf_light_accumulate(sf_ctx* ctx, const sf_light_accumulate_params* params);
/* Forget the history: the next sf_light_accumulate is a first call. The buffers are kept. */
int sf_light_history_reset(sf_ctx* ctx);

/* Several frames in ONE persistent launch (round 6): frame k is ctxs[k]'s current view, rendered into ctxs[k]'s
   G-buffer and stats exactly as sf_render(ctxs[k], params) would (bit for bit), but one resident grid takes the
   work units of all n frames from one set of tile queues -- a wave whose frame runs dry goes on with the next
   frame's units, and the heaviest tiles of every frame start first -- instead of n launches each ending on its
   own heaviest tiles. For frames of a camera path rendered ahead (the reference's workers trace continuously,
   Sphereflake.cpp:67-74; bench.py's frames in flight). n <= SF_RENDER_FRAMES_MAX contexts on one device, of
   one frame size, each with a view. Launched on params->stream or ctxs[0]'s stream, ordered after every
   context's earlier work; every context's later calls are ordered after it. params: as sf_render, but whole
   frames or bands at frame positions only (compact / packed / per-ray kernel / max_depth: SF_EINVAL). Where the
   batch cannot take one launch (levels not proven for some view, diagnostics on, the subtree-split or
   compaction kernels), the frames are rendered one launch each, with the same results. */
#define SF_RENDER_FRAMES_MAX 8
int sf_render_frames(sf_ctx* const* ctxs, uint32_t n, const sf_render_params* params);

/* Rows of the slab a (band_rows, band_count, band_index) shard owns (compact layout). */
uint32_t sf_slab_rows(uint32_t height, uint32_t band_rows, uint32_t band_count, uint32_t band_index);

/* Bytes per pixel of the smallest lossless band slab for the context's current view: 4 (params.packed = 2, the
   hit index) when the view proves every hit at depth <= 10 -- heap indices below 2^32 --, else 16 (packed = 1);
   0 before sf_set_view. A pure function of the view: every rank of a split computes the same value. */
uint32_t sf_slab_bytes(const sf_ctx* ctx);

/* The receiving end of a banded frame, either slab format: `stage` (device) holds the packed compact slabs of
   members first_member .. first_member + members - 1 of a (band_rows, band_count) split, each stage_rows x W
   pixels of bytes_per_pixel (16: packed = 1, 4: packed = 2) bytes; every pixel is written to the context's G-buffer
   at its frame position, bit for bit what an unbanded render writes (recomputed from the context's current view:
   call it with the view the slabs were traced with). stage_rows must hold every member's slab (SF_EINVAL
   otherwise). Asynchronous on `stream`. */
int sf_unpack_slabs(sf_ctx* ctx, const void* stage, uint32_t bytes_per_pixel, uint32_t stage_rows, uint32_t band_rows,
                    uint32_t band_count, uint32_t first_member, uint32_t members, void* stream);

/* The receiving end of a banded frame: `stage4` (device) holds the packed slabs (params.packed = 1,
   compact = 1) of members first_member .. first_member + members - 1 of a (band_rows, band_count) split, each
   stage_rows x W float4; every pixel is written to the context's G-buffer at its frame position in the
   reference layout, bit for bit what an unbanded render writes (positions recomputed from the context's
   current view: call it with the view the slabs were traced with). Asynchronous on `stream`. */
int sf_unpack_bands(sf_ctx* ctx, const float* stage4, uint32_t stage_rows, uint32_t band_rows, uint32_t band_count,
                    uint32_t first_member, uint32_t members, void* stream);

/* Replaces GetGBuffer() + the GL PBO upload source (Sphereflake.h:25-28,
   GLPixelBufferObject.h:24-29): synchronous D2H copy of the context G-buffer into host
   float4 arrays of W*H elements. Any pointer may be NULL to skip that channel. */
int sf_download(sf_ctx* ctx, float* pos4, float* nrm4, float* min_t, uint32_t* hit_index);

/* Stream-ordered D2H of the context G-buffer (and aux channels) on `stream` (NULL = the context
   stream); returns at once. With page-locked destinations (sf_host_register) it runs at PCIe DMA
   rate and overlaps host work; completion: sf_synchronize (context stream) or the caller's stream. */
int sf_download_async(sf_ctx* ctx, float* pos4, float* nrm4, float* min_t, uint32_t* hit_index, void* stream);

/* Page-lock existing host memory (e.g. the std::vector storage of the C++ class's GBuffer, which the
   reference's PBO upload reads, GLPixelBufferObject.h:24-29) so device copies into it use DMA. */
int sf_host_register(void* ptr, size_t bytes);
int sf_host_unregister(void* ptr);

/* --- reference variant ----------------------------------- */
/* The reference compiles one of two SIMD paths (Sphereflake.cpp:29-33): AVX (SIMD_AVX.h: LOD constant
   70, 8-lane packets, 8-pixel frame-less footprint) or, with __ARCH_NO_AVX (its Linux CMake build),
   SSE (SIMD_SSE.h: LOD constant 60, 4-lane packets, 2x2 footprint, Sphereflake.cpp:115-138). A context
   reproduces either bit for bit; default AVX. Synchronous; later renders use the chosen variant. */
#define SF_VARIANT_AVX 0
#define SF_VARIANT_SSE 1
int sf_set_variant(sf_ctx* ctx, int variant);
int sf_get_variant(const sf_ctx* ctx);   /* SF_VARIANT_* or SF_EINVAL */
/* Exact threshold T: sqrtf(t / r) < lod_constant || t < 0  <=>  t < T (Sphereflake.h:129,146). Host only. */
int sf_lod_threshold(float r, float lod_constant, float* T);
/* 1 when ray generation's u = x / n (Sphereflake.cpp:149-150) may be formed as q0 = RN(x RN(1/n)) corrected by one
   fma residual (RN(q0 + (x - q0 n) RN(1/n))) with the same bits as the division for every integer x in [0, n];
   a context uses the shortcut only for a frame size where this holds (checked at sf_create). Host only. */
int sf_division_by_reciprocal_exact(uint32_t n);

/* --- SSAO post-process ---------------------------------- */
/* The reference's GL passes over the G-buffer (SSAO.cpp:106-142: SSAO, blur x, blur y;
   main.cpp:312-330: final composite), run headless as HIP kernels. Output: RGBA8 image, W*H*4
   bytes, row j = G-buffer row j (GL framebuffer row j counted from the bottom). */
#define SF_POST_GENERAL      1u   /* always run the multi-pass path (A/B; results identical) */
#define SF_POST_UNIT_NORMALS 2u   /* caller's external normals have length <= 1.004 (enables fusion) */

typedef struct sf_post_params {
    float sample_radius;      /* SSAOSampleRadius; < 0: 8 x GetClosestSphereDistance() of this
                                 context, read on the device (main.cpp:316, SSAO.h:15-18) */
    float intensity;          /* SSAO.cpp:51   0.51 */
    float scale;              /* SSAO.cpp:52   3.28 */
    float bias;               /* SSAO.cpp:53   0.23 */
    float normal_threshold;   /* SSAO.cpp:54   2.47 */
    float depth_threshold;    /* SSAO.cpp:55   0.01 */
    float camera_position[3]; /* post_final.glsl cameraPosition (main.cpp:325: the view origin) */
    uint32_t downscale;       /* SSAO target = (W / d, H / d) (SSAO ctor, main.cpp:118 uses 1) */
    uint32_t flags;           /* SF_POST_* */
    void* stream;             /* NULL = the context stream */
} sf_post_params;

/* Reference defaults; camera_position = the context's SetView origin. */
int sf_post_defaults(const sf_ctx* ctx, sf_post_params* params);

/* Post-process a G-buffer on the device. pos4 / nrm4: device float4 G-buffer of W*H pixels (NULL =
   the context's). rgba: device output W*H*4 bytes (NULL = the context's image buffer, see
   sf_download_image). ao: optional device output of the SSAO target before blurring
   ((W/d)*(H/d) bytes, the r channel). Asynchronous on the stream. */
int sf_post_process(sf_ctx* ctx, const sf_post_params* params, const float* pos4, const float* nrm4,
                    uint8_t* rgba, uint8_t* ao);

/* Synchronous D2H of the context image buffer (W*H*4 bytes) written by sf_post_process. */
int sf_download_image(sf_ctx* ctx, uint8_t* rgba);

/* The SSAO noise texture (SSAO.cpp:144-164): 64*64 RGBA32F texels into out[16384]. Host only. */
int sf_ssao_noise(float* out);

/* --- headless image dump ("a PPM/EXR dump for inspection") ------------ */
/* The reference only shows its output in the GL window (main.cpp:306-330); a headless host (no GL)
   inspects a frame through these files. Rows are written top row first (G-buffer row 0 = the top
   edge, Sphereflake.cpp:186-196), so the picture reads the right way up in any viewer. */
#define SF_DUMP_IMAGE         0   /* PPM (P6, 8-bit RGB) of the RGBA8 image of the last sf_post_process;
                                     alpha dropped; SF_ESTATE before any post-process */
#define SF_DUMP_NORMALS       1   /* PPM of the normal channel as clamp(0.5 n + 0.5) * 255, misses black */
#define SF_DUMP_POSITIONS_PFM 2   /* PFM (little-endian float RGB, lossless) of the position channel (x, y, z) */
#define SF_DUMP_NORMALS_PFM   3   /* PFM of the normal channel */
/* Download the context's frame (synchronises) and write it to `path` as `what` (SF_DUMP_*). */
int sf_save_image(sf_ctx* ctx, const char* path, int what);
/* Host-only writers of the same formats: rgba = w*h*4 bytes; v4 = w*h float4 (w component dropped). */
int sf_write_ppm(const char* path, uint32_t width, uint32_t height, const uint8_t* rgba);
int sf_write_pfm(const char* path, uint32_t width, uint32_t height, const float* v4);
/* Frame size of a context. */
int sf_get_size(const sf_ctx* ctx, uint32_t* width, uint32_t* height);

/* Device pointers of the context buffers (any out-pointer may be NULL). */
int sf_device_buffers(sf_ctx* ctx, float** pos4, float** nrm4, float** min_t, uint32_t** hit_index);

/* Block until all work on the context stream is done. */
int sf_synchronize(sf_ctx* ctx);

/* --- stats (Sphereflake.h:30-58) ---------------------------------------- */

int sf_get_stats(sf_ctx* ctx, sf_stats* out);          /* synchronises */
int sf_reset_max_depth(sf_ctx* ctx);                   /* ResetMaxDepthReached */
int sf_reset_rays(sf_ctx* ctx);                        /* ResetRaysPerSecond */
int sf_reset_closest(sf_ctx* ctx);                     /* ResetClosestSphereDistance */

/* --- frame-less progressive mode (Initialize + DoImagePart, Sphereflake.cpp:67-74,86-214) --- */

/* Trace `packets` random 8-ray packets into the context G-buffer, exactly as one reference
   worker thread would: pixel pairs from Sobol dims 0/1 (Sobol.cpp:41-55) scrambled by an
   mt19937 stream seeded with `seed` (std::uniform_int_distribution<unsigned>(0) draws),
   packet footprint of Sphereflake.cpp:143-147, scatter of :186-201, sobol counter starting at
   `counter0`. Packets are traced in parallel; later packets overwrite earlier ones at shared
   pixels, as in the reference's sequential order. */
int sf_progressive(sf_ctx* ctx, uint32_t seed, uint64_t counter0, uint32_t packets, void* stream);

/* --- host setup helpers (reference host math, fixture-pinned) ------------ */

/* Camera corners of reference camera.h:37-53 (FOV, quaternion from (yaw, pitch, roll),
   aspect W/H, scaling tan(fov/2)/3). Angles in radians, fov in degrees. */
int sf_camera_corners(uint32_t width, uint32_t height, const float position[3], float pitch,
                      float yaw, float roll, float fov_deg, float origin[3], float top_left[3],
                      float top_right[3], float bottom_left[3]);

/* The 9 unit child frames of ComputeChildTransformations (Sphereflake.cpp:216-249). */
int sf_child_transforms(float child[9][16]);

/* Root transform of SetView (Sphereflake.cpp:83) for a ray origin. */
int sf_root_transform(const float origin[3], float root[16]);

/* Per-depth constants the kernels use: radius r_d (Sphereflake.h:97), and the exact float
   threshold T_d with  sqrtf(t / r_d) < 70 || t < 0   <=>   t < T_d  (Sphereflake.h:146). */
int sf_depth_constants(uint32_t depth, float* radius, float* lod_threshold);

/* std::mt19937 jump-ahead (host; the frame-less draws' parallel generation): the state (624 words + next
   index, libstdc++ layout: sf_progressive's generator state) after `outputs` more draws, computed with the
   generator's characteristic polynomial (t^m mod phi), not by stepping. */
int sf_mt19937_jump(const uint32_t state_in[625], uint64_t outputs, uint32_t state_out[625]);

/* Reproduction of x86 rsqrtps (the table the kernels use). */
float sf_rsqrtps(float x);

/* --- diagnostics --------------------------------------------------------- */

/* Per-tile timing of the wave kernel (s_memrealtime, 100 MHz) for schedule analysis: when enabled,
   every full-frame render records {start, end, (XCC id << 32) | HW_ID} per 8x8 tile. Off by default;
   never changes results. */
int sf_set_tile_trace(sf_ctx* ctx, int enable);
int sf_get_tile_trace(sf_ctx* ctx, uint64_t* out, size_t n);   /* n >= 3 * tiles; synchronises */
/* Heavy-first tile schedule: the work units the next persistent render takes in order (computed from
   the last render's per-tile costs, heaviest cost bucket first, stable within a bucket; a unit is
   tile | part << 29: part 0 = the whole 8x8 tile, 1/2 = its pixel rows 0-3/4-7, 3..6 = its 4x4 quarters,
   or with env SF_SPLIT_PARTS=subtree its 4 subtree parts -- the tiles of the heaviest buckets may be traced
   as 2 or 4 part units, env SF_SPLIT_BUCKETS / SF_SPLIT_PARTS) and those costs (shader cycles, one per tile
   of the render the order was built for -- a band share's tiles when that render was one; a split tile's
   slowest part, scaled). Either pointer may be NULL; n >= 4 * tiles (order) or tiles (cost only), tiles of
   the whole frame. Returns the unit count, 0 when no order exists yet, or a negative SF_E*. Synchronises. */
int sf_get_tile_order(sf_ctx* ctx, uint32_t* order, uint32_t* cost, size_t n);

/* --- measurement ---------------------------------------------------------- */

/* enable = k > 0: every k-th full-frame render (counting from the call) records HIP events on its
   launch stream around its main trace kernel (the dominant kernel; the roofline in bench.py is priced
   on it). An event pair costs a few us of stream time, so sampling keeps the measurement out of the
   frame rate. enable = 0 turns it off. */
int sf_set_kernel_timing(sf_ctx* ctx, int enable);
/* Durations (ms) of the main trace kernel of the last min(n, 64) timed renders, oldest first;
   returns how many were written (>= 0) or a negative SF_E*. Synchronises. */
int sf_kernel_times(sf_ctx* ctx, float* ms, uint32_t n);
/* Live shader clock (MHz) of the same timed renders, oldest first: per render the median over the first
   wave of 8 workgroups of delta s_memtime / delta s_memrealtime x 100 MHz across that wave's life in the
   trace kernel (it runs for nearly the whole kernel). Returns how many were written; synchronises. */
int sf_kernel_clocks(sf_ctx* ctx, float* mhz, uint32_t n);

/* --- multi-GPU ------------------------------------------ */
/* One process, n member devices (the reference's host thread pool, Sphereflake.cpp:67-74, becomes n
   GPUs). The frame is cut into interleaved bands of band_rows rows, band b traced by member b % n;
   member 0 holds the final G-buffer (its context's buffers): it writes its bands in place; member k > 0
   traces its bands as a packed slab (4 B/pixel hit indices where sf_slab_bytes allows, else 16 B/pixel;
   sf_render_params.packed) and copies it over xGMI into member 0's stage on a copy stream of its own
   (overlapping its next frame's trace); member 0 unpacks the stage into its G-buffer (sf_unpack_slabs) on an
   unpack stream of its own, beside its own trace, and its context stream waits for that. Slabs and stages are
   double-buffered by frame parity, so members run a frame ahead of member 0. A device may appear more than
   once (n contexts on one GPU: the single-GPU test of the path). Stats combine: max depth max, closest min,
   rays and overflow tiles summed. */
typedef struct sf_group sf_group;
int sf_group_create(const int* devices, int n, uint32_t width, uint32_t height, sf_group** out);
void sf_group_destroy(sf_group* group);
int sf_group_size(const sf_group* group);
sf_ctx* sf_group_member(sf_group* group, int k);          /* member k's context (k = 0: the final G-buffer) */
int sf_group_set_view(sf_group* group, const float origin[3], const float top_left[3],
                      const float top_right[3], const float bottom_left[3]);
int sf_group_set_variant(sf_group* group, int variant);
/* One frame across the members (asynchronous; band_rows a multiple of 8, 0 = 8). Work queued on member
   0's context afterwards (sf_download, sf_post_process, ...) sees the whole frame. */
int sf_group_render(sf_group* group, uint32_t band_rows);
int sf_group_synchronize(sf_group* group);
int sf_group_download(sf_group* group, float* pos4, float* nrm4);   /* synchronous D2H of the frame */
int sf_group_get_stats(sf_group* group, sf_stats* out);             /* synchronises */
int sf_group_reset_stats(sf_group* group);                          /* all three counters, every member */
int sf_group_last_hip_error(const sf_group* group);
/* Bytes per pixel a member ships for the current view (sf_slab_bytes of member 0). */
int sf_group_slab_bytes(const sf_group* group);

/* --- multi-GPU, one process per GPU ------------------------------------------------------
   The reference's worker pool (Sphereflake.cpp:67-74) as nranks processes, one GPU each (the torch.distributed /
   MPI model): every rank traces the interleaved bands b = rank (mod nranks) of each frame; ranks k > 0 trace
   theirs as packed slabs (4 B/pixel hit indices where sf_slab_bytes allows, else 16 B/pixel;
   sf_render_params.packed) and send them to rank 0 with RCCL over xGMI (ncclSend behind the trace on the frame's
   stream); rank 0 traces its own bands in place while it receives the others' (one grouped ncclRecv) and unpacks
   them (sf_unpack_slabs) on a receive stream of its own; the slot's context stream then waits for the unpack: the
   frame in rank 0's G-buffer bit for bit the single-GPU frame.
   `slots` frames may be in flight: frame i runs on slot i % slots (its own context, stream, communicator and
   buffers), so a frame's trace fills the GPU while the previous frame's heaviest tiles and gather finish.
   Without ids there is no communicator, whatever nranks: frames in flight on one GPU (nranks = 1), or this rank's
   bands of a distributed G-buffer (sf_dist_render_bands; sf_dist_render returns SF_ESTATE, sf_dist_get_stats this
   rank's stats alone). Every rank must issue the same calls in the same order (set_view, render, get_stats) with
   the same views. */
#define SF_DIST_ID_BYTES 128   /* ncclUniqueId */
#define SF_DIST_MAX_SLOTS 16
typedef struct sf_dist sf_dist;
/* Rank 0 makes one id per slot and hands them to every rank (any channel: MPI, a torch.distributed broadcast). */
int sf_dist_unique_id(uint8_t id[SF_DIST_ID_BYTES]);
/* Collective over the ranks when ids are given (RCCL communicator init per slot). ids: slots x SF_DIST_ID_BYTES,
   or NULL: no communicator at all (bands only, see above); nranks = 1 with ids makes a one-rank communicator.
   band_rows: a multiple of 8 (8 = one tile row). */
int sf_dist_create(int device, uint32_t width, uint32_t height, uint32_t band_rows, int rank, int nranks, int slots,
                   const uint8_t* ids, sf_dist** out);
void sf_dist_destroy(sf_dist* dist);
int sf_dist_slots(const sf_dist* dist);
sf_ctx* sf_dist_context(sf_dist* dist, int slot);     /* slot's context; on rank 0 it holds that slot's frames */
int sf_dist_last_slot(const sf_dist* dist);           /* slot of the last frame issued (SF_ESTATE before any) */
int sf_dist_set_view(sf_dist* dist, const float origin[3], const float top_left[3], const float top_right[3],
                     const float bottom_left[3]);     /* the view of the next frames (kept by the dist and set on
                                                         a slot's context when a frame is rendered on it) */
int sf_dist_render(sf_dist* dist);                    /* one frame, asynchronous (this rank's share + gather;
                                                         SF_ESTATE for nranks > 1 without communicators) */
/* One frame as a distributed G-buffer: this rank's bands into its slot's G-buffer at frame positions (reference
   layout), no gather -- every rank holds its own rows in its own HBM. Asynchronous; no collective. */
int sf_dist_render_bands(sf_dist* dist);

/* The next n frames of a camera path (views[k][0..11] = origin, top-left, top-right, bottom-left) as this rank's
   bands, frame k into slot (frames + k) % slots's G-buffer (n <= slots, n <= SF_RENDER_FRAMES_MAX), in ONE
   multi-frame persistent launch (sf_render_frames): sf_dist_render_bands for n frames without a launch each.
   The views are set on the slots (sf_dist_set_view is not needed). Asynchronous. */
int sf_dist_render_bands_frames(sf_dist* dist, uint32_t n, const float (*views)[12]);
int sf_dist_synchronize(sf_dist* dist);               /* every slot of this rank done */
int sf_dist_download(sf_dist* dist, float* pos4, float* nrm4);   /* rank 0: D2H of the last frame (synchronises) */
int sf_dist_get_stats(sf_dist* dist, sf_stats* out);  /* over slots, and over ranks when made with ids
                                                         (then collective); synchronises */
int sf_dist_reset_stats(sf_dist* dist);
int sf_dist_last_error(const sf_dist* dist, int* hip_error, int* rccl_error);
/* The RCCL communicator of `slot` as RCCL reports it: ncclCommCount, ncclCommUserRank, ncclCommCuDevice
   (SF_ESTATE when the dist was made without ids). */
int sf_dist_comm_info(const sf_dist* dist, int slot, int* count, int* rank, int* device);
/* Bytes per pixel the gather ships for the current view (sf_slab_bytes of the slots' contexts). */
int sf_dist_slab_bytes(const sf_dist* dist);

/* The context's own stream (hipStream_t) -- where calls with a NULL stream are queued. */
void* sf_context_stream(sf_ctx* ctx);
/* Trace launches of this context that took the lean tile loop (kernels sf_trace_queue1t, and sf_trace_queue1 / 1c over
   pair units: whole units of one plain frame -- no aux channels, packed slab, band share, part units or diagnostics;
   SF_LEAN=0 in the environment of sf_create forces the general loop, sf_trace_queue1g, everywhere). For tests and
   measurements. */
uint32_t sf_lean_launches(const sf_ctx* ctx);
/* Those of them that took the pair-unit loop (sf_trace_queue1, and sf_trace_queue1c on the render that rebuilds the
   unit order): two horizontally adjacent 8x8 tiles per wave, which share the traversal's upper levels. By default a
   launch the lean loop can serve takes it where the frame has more tiles than twice the pair kernel's persistent grid
   (1920x1080 and up); SF_PAIR=0 in the environment of sf_create turns pair units off, SF_PAIR=1 takes them at every
   frame size. Results are the same bit for bit. */
uint32_t sf_pair_launches(const sf_ctx* ctx);
/* Units the context's current unit order was built over -- tiles, or pair units where the renders take those: the
   entries of sf_get_tile_order's `cost` that are meaningful (0: no order yet). */
uint32_t sf_order_units(const sf_ctx* ctx);

/* --- misc ---------------------------------------------------------------- */

const char* sf_strerror(int status);
int sf_last_hip_error(const sf_ctx* ctx);
int sf_abi_version(void);
/* Hash of the sources this library was built from (scripts/source_hash.py): ties a measurement to a build. */
const char* sf_build_id(void);
int sf_device_count(void);

#ifdef __cplusplus
}
#endif

#endif /* SPHEREFLAKE_SF_H */
