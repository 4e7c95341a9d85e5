"""Host statement of the point-light arithmetic of ``Sphereflake.trace_shadow`` / ``Sphereflake.light_image``
(sf_trace_shadow_to, sf_light_image; the definition is in include/sphereflake/sf.h).

Everything is numpy float32, one rounding per operation, in the order the header gives -- the device kernels form
the same bits (tests/test_gpu_shadow.py).

A shadow ray is traced FROM THE LIGHT towards the surface point and its nearest hit compared with the distance to
the point, so no ray starts on the flake and the reference's ``tca >= 0`` quirk (sphereflake_amd/rays.py) cannot
bite while the light stays outside the flake's bounding ball (radius 2 about its centre). The level of detail is
the light's: a node refines by its distance from the light, so a far light casts coarse shadows.

A directional light (``Sphereflake.trace_sun`` / ``light_image_sun``: sun_model, light_model_sun, sun_direction)
starts every pixel's ray a fixed distance up the sun direction from its own surface point instead, and
``Sphereflake.set_shadow_lod`` with matched_lod chooses the level of detail of all the shadow traces. Many such
directions in one launch (``Sphereflake.trace_suns`` / ``light_image_suns``: sun_cone, sky_dirs, suns_model,
light_model_suns) make a sun with an angular size or a sky dome of parallel rays. Light shafts
(``Sphereflake.trace_shafts`` / ``light_image_shafts``: shaft_fractions, shaft_ends, shaft_samples, shafts_model,
shaft_distance, light_model_shafts) ask the sun's question of points along each pixel's view ray. The colour light
buffer (``Sphereflake.trace_suns_sum`` / ``trace_shadows_sum`` / ``light_fill`` / ``light_image_buffer``: sum_model,
light_model_buffer, sky_colours) adds any number of coloured suns and lights per pixel instead of multiplying the
image once per call. Ambient occlusion (``Sphereflake.trace_ao`` / ``trace_ao_sum``: ao_samples, ao_colours, ao_basis,
ao_directions, ao_model, ao_sum_model) traces a hemisphere of such sun rays about each pixel's own normal; a per-pixel
spin and an edge-aware filter (ao_spins, light_filter_model) make four such rays stand for sixty-four, and temporal
accumulation (``Sphereflake.light_accumulate``: reproject_matrix, light_accumulate_model, ao_phase) carries the light
buffer from one frame of a moving camera to the next. Sky reflections (``Sphereflake.trace_mirror`` /
``trace_mirror_sum``: lobe_samples, mirror_axes, mirror_model, sky_gradient, mirror_sum_model) turn a lobe of such rays
about each pixel's mirror direction and weigh every open one by the sky's colour along it.
"""
from __future__ import annotations

import numpy as np

_F = np.float32

# sf_shadow_defaults' relative bias (scripts/experiments/shadow_bias.py)
DEFAULT_BIAS = 2.0 ** -10


def _world(pos4, origin):
    P = np.asarray(pos4, _F)[..., :3]
    o = np.asarray(origin, _F).reshape(3)
    return P, o + P


def _length(d):
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def shadow_model(pos4, origin, light, bias):
    """Steps 1-3 of the definition for a position image pos4 [..., 3 | 4] relative to `origin`, a light at `light`
    and the relative bias `bias`: (d [..., 3], bound [...], is_surface [...]).

    is_surface is False where P == (0, 0, 0), a miss of the frame (no ray: visible). d = (w - light) + 0 with
    w = origin + P is the unnormalised direction of the ray from the light (no -0 component), and
    bound = |d| (1 - bias) the distance a hit must stay under to shadow the pixel. d and bound of a miss pixel are
    formed all the same and mean nothing."""
    if not 0.0 <= float(bias) < 1.0:
        raise ValueError("bias must be in [0, 1)")
    P, w = _world(pos4, origin)
    l = np.asarray(light, _F).reshape(3)
    with np.errstate(invalid="ignore", over="ignore"):
        d = (w - l) + _F(0.0)
        bound = _length(d) * (_F(1.0) - _F(bias))
    is_surface = ~((P[..., 0] == 0) & (P[..., 1] == 0) & (P[..., 2] == 0))
    assert d.dtype == _F and bound.dtype == _F
    return d, bound, is_surface


def light_model(rgba, pos4, nrm4, vis, origin, light, ambient=0.25):
    """What sf_light_image makes of the RGBA8 image `rgba` [..., 4]: a new uint8 array. pos4 / nrm4 [..., 4] are the
    G-buffer the image was made from, vis [...] the visibility bytes of trace_shadow for the same light.

    A miss pixel stays; else with e = light - w and len = |(w - light) + 0| as in shadow_model,
    lam = max(0, ((n.x e.x + n.y e.y) + n.z e.z) / len) (0 where that is NaN), k = ambient + (1 - ambient)
    (vis ? lam : 0), and each of r, g, b becomes uint8(min(c k + 0.5, 255)); alpha stays."""
    a = _F(ambient)
    if not 0.0 <= float(a) <= 1.0:
        raise ValueError("ambient must be in [0, 1]")
    out = np.array(rgba, np.uint8, copy=True)
    P, w = _world(pos4, origin)
    n = np.asarray(nrm4, _F)[..., :3]
    l = np.asarray(light, _F).reshape(3)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        length = _length((w - l) + _F(0.0))
        e = l - w
        dot = (n[..., 0] * e[..., 0] + n[..., 1] * e[..., 1]) + n[..., 2] * e[..., 2]
        lam = np.fmax(_F(0.0), dot / length)
        k = a + (_F(1.0) - a) * np.where(np.asarray(vis) != 0, lam, _F(0.0)).astype(_F)
        rgb = np.fmin(out[..., :3].astype(_F) * k[..., None] + _F(0.5), _F(255.0))
    assert rgb.dtype == _F
    surface = ~((P[..., 0] == 0) & (P[..., 1] == 0) & (P[..., 2] == 0))
    out[..., :3] = np.where(surface[..., None], rgb.astype(np.uint8), out[..., :3])
    return out


# --- a directional light (sf_trace_sun_to, sf_light_image_sun, sf_set_shadow_lod) ---------------------------------
# sf_sun_defaults' distance: |w| <= 2 for a surface point, so every ray starts outside the flake's radius-2 ball
DEFAULT_SUN_DISTANCE = 4.0


def sun_direction(v):
    """The float32 unit vector along v (normalised in float64, then rounded): the `direction` of trace_sun, which
    uses it as given. The reference's one directional light is sun_direction((0.7, 0.7, 0.2))
    (Shaders/post_final.glsl:11). A zero or non-finite v has no direction: ValueError."""
    v = np.asarray(v, np.float64).reshape(3)
    n = np.linalg.norm(v)
    if not (np.isfinite(n) and n > 0):
        raise ValueError("the sun direction must be finite and not zero")
    return (v / n).astype(_F)


def matched_lod(distance, t_ref, base=70.0):
    """The LOD constant for set_shadow_lod that gives a shadow ray starting `distance` from a surface the level of
    detail the camera has at camera distance t_ref (e.g. stats().closest): a node refines while sqrt(t / r) < C, so
    C = base sqrt(distance / t_ref) refines at `distance` exactly what `base` (the variant's constant: 70 AVX, 60
    SSE) refines at t_ref. float32."""
    distance, t_ref, base = float(distance), float(t_ref), float(base)
    if not (np.isfinite(distance) and distance > 0 and np.isfinite(t_ref) and t_ref > 0 and np.isfinite(base) and base > 0):
        raise ValueError("distance, t_ref and base must be finite and > 0")
    return _F(base * np.sqrt(distance / t_ref))


def sun_model(pos4, origin, direction, distance, bias):
    """Steps 1-3 of sf_trace_sun_to's definition for a position image pos4 [..., 3 | 4] relative to `origin`, the
    direction s towards the sun (as given), the distance tau and the relative bias:
    (F [..., 3], d [..., 3], bound [...], is_surface [...]).

    w = origin + P, f = s tau, F = w + f is the origin of the pixel's ray, d = (w - F) + 0 its unnormalised direction
    (no -0 component) and bound = |d| (1 - bias) the distance a hit must stay under to shadow the pixel. is_surface is
    False where P == (0, 0, 0), a miss of the frame (no ray: visible); F, d and bound of a miss pixel are formed all
    the same and mean nothing."""
    if not 0.0 <= float(bias) < 1.0:
        raise ValueError("bias must be in [0, 1)")
    tau = _F(distance)
    if not (np.isfinite(tau) and tau > 0):
        raise ValueError("distance must be finite and > 0")
    P, w = _world(pos4, origin)
    s = np.asarray(direction, _F).reshape(3)
    with np.errstate(invalid="ignore", over="ignore"):
        f = s * tau
        Fo = w + f
        d = (w - Fo) + _F(0.0)
        bound = _length(d) * (_F(1.0) - _F(bias))
    is_surface = ~((P[..., 0] == 0) & (P[..., 1] == 0) & (P[..., 2] == 0))
    assert Fo.dtype == _F and d.dtype == _F and bound.dtype == _F
    return Fo, d, bound, is_surface


def light_model_sun(rgba, pos4, nrm4, vis, direction, ambient=0.25):
    """What sf_light_image_sun makes of the RGBA8 image `rgba` [..., 4]: a new uint8 array. light_model with
    lam = max(0, (n.x s.x + n.y s.y) + n.z s.z) (0 where that is NaN) for the direction s towards the sun, as given:
    no light position and no division. vis [...] are the bytes of trace_sun for the same direction."""
    a = _F(ambient)
    if not 0.0 <= float(a) <= 1.0:
        raise ValueError("ambient must be in [0, 1]")
    out = np.array(rgba, np.uint8, copy=True)
    P = np.asarray(pos4, _F)[..., :3]
    n = np.asarray(nrm4, _F)[..., :3]
    s = np.asarray(direction, _F).reshape(3)
    with np.errstate(invalid="ignore", over="ignore"):
        dot = (n[..., 0] * s[0] + n[..., 1] * s[1]) + n[..., 2] * s[2]
        lam = np.fmax(_F(0.0), dot)
        k = a + (_F(1.0) - a) * np.where(np.asarray(vis) != 0, lam, _F(0.0)).astype(_F)
        rgb = np.fmin(out[..., :3].astype(_F) * k[..., None] + _F(0.5), _F(255.0))
    assert rgb.dtype == _F
    surface = ~((P[..., 0] == 0) & (P[..., 1] == 0) & (P[..., 2] == 0))
    out[..., :3] = np.where(surface[..., None], rgb.astype(np.uint8), out[..., :3])
    return out


# --- many lights per pixel (sf_trace_shadows_to, sf_light_image_many) ---------------------------------------------
LIGHTS_MAX = 64          # SF_SHADOW_LIGHTS_MAX: one bit of the mask word per light
_GOLDEN = np.pi * (3.0 - np.sqrt(5.0))   # the golden angle


def _count(n, limit=LIGHTS_MAX):
    n = int(n)
    if not 1 <= n <= limit:
        raise ValueError(f"1..{limit} lights, not {n}")
    return n


def masks_from_vis(vis_list):
    """The mask word of trace_shadows from the visibility bytes of trace_shadow, one image per light in the lights'
    order: bit i = (vis_list[i] != 0), bits len(vis_list)..63 zero. uint64, the images' shape."""
    n = _count(len(vis_list))
    mask = np.zeros(np.asarray(vis_list[0]).shape, np.uint64)
    for i in range(n):
        mask |= (np.asarray(vis_list[i]) != 0).astype(np.uint64) << np.uint64(i)
    return mask


def vis_from_masks(mask, n):
    """The inverse: n visibility images (255 / 0) from the mask words."""
    mask = np.asarray(mask, np.uint64)
    return [np.where((mask >> np.uint64(i)) & np.uint64(1), 255, 0).astype(np.uint8) for i in range(_count(n))]


def light_model_many(rgba, pos4, nrm4, mask, origin, lights, weights=None, ambient=0.25):
    """What sf_light_image_many makes of the RGBA8 image `rgba` [..., 4]: a new uint8 array. mask [...] are the words
    of trace_shadows for the same lights [n, 3]; weights [n] (None: float32(1) / float32(n) each).

    A miss pixel stays; else S = 0, then for i = 0 .. n-1 in that order S = S + w_i (bit i ? lam_i : 0) with lam_i
    exactly light_model's lam for light i, k = ambient + (1 - ambient) S (S is not clamped), and each of r, g, b
    becomes uint8(min(c k + 0.5, 255)); alpha stays."""
    a = _F(ambient)
    if not 0.0 <= float(a) <= 1.0:
        raise ValueError("ambient must be in [0, 1]")
    L = np.asarray(lights, _F).reshape(-1, 3)
    n = _count(L.shape[0])
    if weights is None:
        w = np.full(n, _F(1.0) / _F(n), _F)
    else:
        w = np.asarray(weights, _F).reshape(-1)
        if w.shape[0] != n or not (w >= 0).all():
            raise ValueError("one weight per light, none negative or NaN")
    out = np.array(rgba, np.uint8, copy=True)
    P, wpos = _world(pos4, origin)
    nr = np.asarray(nrm4, _F)[..., :3]
    mask = np.asarray(mask, np.uint64)
    S = np.zeros(P.shape[:-1], _F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for i in range(n):
            l = L[i]
            length = _length((wpos - l) + _F(0.0))
            e = l - wpos
            dot = (nr[..., 0] * e[..., 0] + nr[..., 1] * e[..., 1]) + nr[..., 2] * e[..., 2]
            lam = np.fmax(_F(0.0), dot / length)
            bit = ((mask >> np.uint64(i)) & np.uint64(1)) != 0
            S = S + w[i] * np.where(bit, lam, _F(0.0)).astype(_F)
        k = a + (_F(1.0) - a) * S
        rgb = np.fmin(out[..., :3].astype(_F) * k[..., None] + _F(0.5), _F(255.0))
    assert S.dtype == _F and rgb.dtype == _F
    surface = ~((P[..., 0] == 0) & (P[..., 1] == 0) & (P[..., 2] == 0))
    out[..., :3] = np.where(surface[..., None], rgb.astype(np.uint8), out[..., :3])
    return out


def disc(centre, radius, n, limit=LIGHTS_MAX):
    """n points of a sunflower disc of `radius` about `centre` that faces the flake's centre (the world origin): an
    area light's samples (limit: the most the caller's trace takes -- SUM_MAX for trace_shadows_sum). In float64
    a = -c / |c|, u = normalize(a x (0, 0, 1)), v = a x u, r_i = radius
    sqrt((i + 0.5) / n), theta_i = i pi (3 - sqrt 5), point c + r_i cos(theta_i) u + r_i sin(theta_i) v; float32
    [n, 3]. Deterministic. (A centre on the z axis has no such u: ValueError.)"""
    n = _count(n, limit)
    c = np.asarray(centre, np.float64).reshape(3)
    norm = np.linalg.norm(c)
    if not norm > 0:
        raise ValueError("the disc's centre must not be the flake's centre")
    a = -c / norm
    u = np.cross(a, (0.0, 0.0, 1.0))
    if not np.linalg.norm(u) > 0:
        raise ValueError("a disc centred on the z axis has no horizontal direction")
    u = u / np.linalg.norm(u)
    v = np.cross(a, u)
    i = np.arange(n, dtype=np.float64)
    r = float(radius) * np.sqrt((i + 0.5) / n)
    th = i * _GOLDEN
    pts = c + (r * np.cos(th))[:, None] * u + (r * np.sin(th))[:, None] * v
    return pts.astype(_F)


def sky(n, radius=4.0, up=(0.0, 0.0, 1.0), limit=LIGHTS_MAX):
    """n points of a Fibonacci upper hemisphere of `radius` about the flake's centre (the world origin), the pole
    along `up`: the lights of a ray-traced sky occlusion term (keep radius > 2: outside the flake's bounding ball).
    In float64 z_i = (i + 0.5) / n along `up`, s_i = sqrt(1 - z_i^2), theta_i = i pi (3 - sqrt 5), point
    radius (s_i cos(theta_i) e1 + s_i sin(theta_i) e2 + z_i up) with e1, e2 completing `up` to a right-handed
    frame; float32 [n, 3]. Deterministic. limit as disc's."""
    return (float(radius) * _hemisphere(n, up, limit)).astype(_F)


def _frame(axis, what):
    """float64 (e1, e2, w): w along `axis`, e1 and e2 completing it to a right-handed frame."""
    w = np.asarray(axis, np.float64).reshape(3)
    norm = np.linalg.norm(w)
    if not (np.isfinite(norm) and norm > 0):
        raise ValueError(f"{what} must be finite and not zero")
    w = w / norm
    t = np.array((1.0, 0.0, 0.0)) if abs(w[0]) < 0.9 else np.array((0.0, 1.0, 0.0))
    e1 = t - w * np.dot(t, w)
    e1 = e1 / np.linalg.norm(e1)
    return e1, np.cross(w, e1), w


def _hemisphere(n, up, limit=LIGHTS_MAX):
    """sky()'s points at radius 1, float64 [n, 3]."""
    n = _count(n, limit)
    e1, e2, w = _frame(up, "up")
    i = np.arange(n, dtype=np.float64)
    z = (i + 0.5) / n
    s = np.sqrt(1.0 - z * z)
    th = i * _GOLDEN
    return (s * np.cos(th))[:, None] * e1 + (s * np.sin(th))[:, None] * e2 + z[:, None] * w


# --- many sun directions per pixel (sf_trace_suns_to, sf_light_image_suns) ----------------------------------------
def _unit32(v):
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(_F)


def sun_cone(direction, half_angle, n, limit=LIGHTS_MAX):
    """n unit directions inside the cone of `half_angle` (radians, 0 <= half_angle < pi / 2) about `direction`: the
    samples of a sun with an angular size, the `dirs` of trace_suns. A Vogel disc on the cone's cap, in float64: with
    (e1, e2, a) the frame of sky() about a = direction / |direction|, alpha_i = half_angle sqrt((i + 0.5) / n) (the
    first directions are nearest the axis), theta_i = i pi (3 - sqrt 5), direction cos(alpha_i) a + sin(alpha_i)
    (cos(theta_i) e1 + sin(theta_i) e2), normalised; float32 [n, 3]. Deterministic. limit: the most the caller's
    trace takes (SUM_MAX for trace_suns_sum)."""
    n = _count(n, limit)
    half_angle = float(half_angle)
    if not 0.0 <= half_angle < np.pi / 2:
        raise ValueError("half_angle must be in [0, pi / 2) radians")
    e1, e2, a = _frame(direction, "the sun direction")
    i = np.arange(n, dtype=np.float64)
    al = half_angle * np.sqrt((i + 0.5) / n)
    th = i * _GOLDEN
    v = np.cos(al)[:, None] * a + (np.sin(al) * np.cos(th))[:, None] * e1 + (np.sin(al) * np.sin(th))[:, None] * e2
    return _unit32(v)


def sky_dirs(n, up=(0.0, 0.0, 1.0), limit=LIGHTS_MAX):
    """n unit directions over the upper hemisphere about `up`: sky()'s points, normalised (in float64, then rounded);
    float32 [n, 3]. The `dirs` of trace_suns for a sky dome of parallel rays: every pixel gets the same level of
    detail, whereas a sky() point light refines by its own distance from each node. Deterministic. limit as
    sun_cone's."""
    return _unit32(_hemisphere(n, up, limit))


def suns_model(pos4, origin, dirs, distance, bias):
    """sun_model per direction, stacked: (F [n, ..., 3], d [n, ..., 3], bound [n, ...], is_surface [...]) for the
    directions dirs [n, 3] -- slice i is sun_model(pos4, origin, dirs[i], distance, bias), bit for bit."""
    D = np.asarray(dirs, _F).reshape(-1, 3)
    parts = [sun_model(pos4, origin, D[i], distance, bias) for i in range(_count(D.shape[0]))]
    return (np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), np.stack([p[2] for p in parts]),
            parts[0][3])


def light_model_suns(rgba, pos4, nrm4, mask, dirs, weights=None, ambient=0.25):
    """What sf_light_image_suns makes of the RGBA8 image `rgba` [..., 4]: a new uint8 array. mask [...] are the words
    of trace_suns for the same directions dirs [n, 3]; weights [n] (None: float32(1) / float32(n) each).

    light_model_many with light_model_sun's lam: a miss pixel stays; else S = 0, then for i = 0 .. n-1 in that order
    S = S + w_i (bit i ? lam_i : 0) with lam_i = max(0, (n.x s.x + n.y s.y) + n.z s.z) (0 where that is NaN) for
    s = dirs[i], k = ambient + (1 - ambient) S (S is not clamped), and each of r, g, b becomes
    uint8(min(c k + 0.5, 255)); alpha stays."""
    a = _F(ambient)
    if not 0.0 <= float(a) <= 1.0:
        raise ValueError("ambient must be in [0, 1]")
    D = np.asarray(dirs, _F).reshape(-1, 3)
    n = _count(D.shape[0])
    if weights is None:
        w = np.full(n, _F(1.0) / _F(n), _F)
    else:
        w = np.asarray(weights, _F).reshape(-1)
        if w.shape[0] != n or not (w >= 0).all():
            raise ValueError("one weight per direction, none negative or NaN")
    out = np.array(rgba, np.uint8, copy=True)
    P = np.asarray(pos4, _F)[..., :3]
    nr = np.asarray(nrm4, _F)[..., :3]
    mask = np.asarray(mask, np.uint64)
    S = np.zeros(P.shape[:-1], _F)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(n):
            s = D[i]
            dot = (nr[..., 0] * s[0] + nr[..., 1] * s[1]) + nr[..., 2] * s[2]
            lam = np.fmax(_F(0.0), dot)
            bit = ((mask >> np.uint64(i)) & np.uint64(1)) != 0
            S = S + w[i] * np.where(bit, lam, _F(0.0)).astype(_F)
        k = a + (_F(1.0) - a) * S
        rgb = np.fmin(out[..., :3].astype(_F) * k[..., None] + _F(0.5), _F(255.0))
    assert S.dtype == _F and rgb.dtype == _F
    surface = ~((P[..., 0] == 0) & (P[..., 1] == 0) & (P[..., 2] == 0))
    out[..., :3] = np.where(surface[..., None], rgb.astype(np.uint8), out[..., :3])
    return out


# --- light shafts: sun visibility along each pixel's view ray (sf_trace_shafts_to, sf_light_image_shafts) ----------
SHAFT_SAMPLES_MAX = 64   # SF_SHAFT_SAMPLES_MAX: one bit of the mask word per sample


def shaft_fractions(n):
    """n march fractions at the midpoints of n equal steps from the origin to the march end: (i + 0.5) / n, formed in
    float64 and rounded; float32 [n]. The `fractions` of trace_shafts; their even weights are 1 / n."""
    n = _count(n)
    return ((np.arange(n, dtype=np.float64) + 0.5) / n).astype(_F)


def shaft_ends(pos4, dirs=None, far=0.0):
    """Step 1 of sf_trace_shafts_to's definition: the march ends E [..., 3] of a position image pos4 [..., 3 | 4].
    E = P where P != (0, 0, 0); at a miss of the frame E = dirs[p] far per component (dirs [..., 3 | 4], used as
    given) where dirs is not None and far > 0, else 0."""
    P = np.asarray(pos4, _F)[..., :3]
    far = _F(far)
    if not (np.isfinite(far) and far >= 0):
        raise ValueError("far must be finite and >= 0")
    E = np.array(P, _F, copy=True)
    if dirs is not None and far > 0:
        D = np.asarray(dirs, _F)[..., :3]
        if D.shape != P.shape:
            raise ValueError("dirs and pos4 must have the same height and width")
        miss = (P[..., 0] == 0) & (P[..., 1] == 0) & (P[..., 2] == 0)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            E = np.where(miss[..., None], D * far, P).astype(_F)
    return E


def _fractions(fractions):
    sg = np.asarray(fractions, _F).reshape(-1)
    if not 1 <= sg.shape[0] <= SHAFT_SAMPLES_MAX:
        raise ValueError(f"1..{SHAFT_SAMPLES_MAX} samples, not {sg.shape[0]}")
    if not (np.isfinite(sg) & (sg > 0)).all():
        raise ValueError("every fraction must be finite and > 0")
    return sg


def shaft_samples(ends, fractions):
    """Step 2: the samples Q [n, ..., 3], Q_i = E sigma_i per component, one rounding each. Q_i is the position image
    whose trace_sun byte is bit i of trace_shafts' word."""
    E = np.asarray(ends, _F)[..., :3]
    sg = _fractions(fractions)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        Q = np.stack([E * s for s in sg])
    assert Q.dtype == _F
    return Q


def shafts_model(pos4, origin, direction, distance, bias, fractions, dirs=None, far=0.0):
    """Steps 1-2, then sun_model per sample, stacked: (F [n, ..., 3], d [n, ..., 3], bound [n, ...],
    is_surface [n, ...]) -- slice i is sun_model(Q_i, origin, direction, distance, bias), bit for bit, with Q_i the
    i-th image of shaft_samples(shaft_ends(pos4, dirs, far), fractions). is_surface[i] is False where Q_i == 0: no
    ray, the bit is set."""
    Q = shaft_samples(shaft_ends(pos4, dirs, far), fractions)
    parts = [sun_model(Q[i], origin, direction, distance, bias) for i in range(Q.shape[0])]
    return tuple(np.stack([p[k] for p in parts]) for k in range(4))


def shaft_distance(origin, ends):
    """A `distance` for trace_shafts that keeps the reference's quirk out: 2 + max |origin + E| over the march ends
    E [..., 3], float32, rounded up. With a unit sun direction and fractions <= 1 every sample origin + E sigma lies
    within max(|origin|, |origin + E|) of the flake's centre, so every ray starts outside the radius-2 ball. Ends
    that are not finite are ignored."""
    o = np.asarray(origin, np.float64).reshape(3)
    E = np.asarray(ends, np.float64)[..., :3].reshape(-1, 3)
    r = np.linalg.norm(np.concatenate([o[None, :], o + E]), axis=-1)
    r = r[np.isfinite(r)]
    tau = 2.0 + float(r.max())
    t32 = _F(tau)
    if float(t32) < tau:
        t32 = np.nextafter(t32, _F(np.inf))
    return t32


def light_model_shafts(rgba, pos4, mask, fractions, weights=None, gain=1.0, colour=(255.0, 255.0, 255.0), dirs=None,
                       far=0.0):
    """What sf_light_image_shafts makes of the RGBA8 image `rgba` [..., 4]: a new uint8 array. mask [...] are the
    words of trace_shafts for the same fractions [n] (used for n only); weights [n] (None: float32(1) / float32(n)
    each); dirs and far as given to trace_shafts.

    With E = shaft_ends(pos4, dirs, far): a pixel with E == 0 stays; else len = sqrt((E.x E.x + E.y E.y) + E.z E.z),
    S = 0, then for i = 0 .. n-1 in that order S = S + (bit i ? w_i : 0), a = min((gain len) S, 1) (0 where that is
    NaN), and each of r, g, b becomes uint8(min((c + (colour_c - c) a) + 0.5, 255)); alpha stays."""
    g = _F(gain)
    if not (np.isfinite(g) and g >= 0):
        raise ValueError("gain must be finite and >= 0")
    col = np.asarray(colour, _F).reshape(3)
    if not ((col >= 0) & (col <= 255)).all():
        raise ValueError("colour components must be in [0, 255]")
    n = _fractions(fractions).shape[0]
    if weights is None:
        w = np.full(n, _F(1.0) / _F(n), _F)
    else:
        w = np.asarray(weights, _F).reshape(-1)
        if w.shape[0] != n or not (w >= 0).all():
            raise ValueError("one weight per sample, none negative or NaN")
    out = np.array(rgba, np.uint8, copy=True)
    E = shaft_ends(pos4, dirs, far)
    mask = np.asarray(mask, np.uint64)
    S = np.zeros(E.shape[:-1], _F)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        length = _length(E)
        for i in range(n):
            bit = ((mask >> np.uint64(i)) & np.uint64(1)) != 0
            S = S + np.where(bit, w[i], _F(0.0)).astype(_F)
        t = (g * length) * S
        a = np.where(np.isnan(t), _F(0.0), np.fmin(t, _F(1.0))).astype(_F)
        c = out[..., :3].astype(_F)
        rgb = np.fmin((c + (col - c) * a[..., None]) + _F(0.5), _F(255.0))
    assert S.dtype == _F and length.dtype == _F and rgb.dtype == _F
    marched = ~((E[..., 0] == 0) & (E[..., 1] == 0) & (E[..., 2] == 0))
    out[..., :3] = np.where(marched[..., None], rgb.astype(np.uint8), out[..., :3])
    return out


# --- the colour light buffer (sf_trace_suns_sum_to, sf_trace_shadows_sum_to, sf_light_fill, sf_light_image_buffer) ---
SUM_MAX = 65536          # SF_LIGHT_SUM_MAX: entries per summing call
SUM_CHUNK = 64           # entries per launch, and per mask of trace_suns / trace_shadows


def sum_model(base, pos4, nrm4, masks, points, colours=None, kind="suns", origin=(0.0, 0.0, 0.0)):
    """Steps 1-4 of sf.h's definition of the sum, on the host: a new float32 array [..., 4].

    base [..., 4] is what the output held (an accumulating call), or None (an overwriting call: the base is 0).
    masks is a list of uint64 images [...]: the words of trace_suns (kind "suns") or trace_shadows (kind "shadows")
    for consecutive chunks of 64 of the points [n, 3] -- entry i is bit i % 64 of masks[i // 64]. colours [n, 3]
    (None: float32(1) / float32(n) per component). origin is what pos4 is relative to (the point lights only).

    A miss pixel (P == 0) keeps the base (None: becomes 0). Else S = base.xyz, then for i = 0 .. n-1 in that order
    and per channel S = S + colours[i] (bit i ? lam_i : 0), lam_i being light_model_suns' / light_model_many's; the
    result is (S, base.w)."""
    if kind not in ("suns", "shadows"):
        raise ValueError("kind is 'suns' or 'shadows'")
    pts = np.asarray(points, _F).reshape(-1, 3)
    n = _count(pts.shape[0], SUM_MAX)
    if colours is None:
        col = np.full((n, 3), _F(1.0) / _F(n), _F)
    else:
        col = np.asarray(colours, _F).reshape(-1, 3)
        if col.shape[0] != n or not (np.isfinite(col) & (col >= 0)).all():
            raise ValueError("one colour per entry, every component finite and not negative")
    masks = [np.asarray(m, np.uint64) for m in masks]
    if len(masks) != (n + SUM_CHUNK - 1) // SUM_CHUNK:
        raise ValueError("one mask image per chunk of 64 entries")
    P, wpos = _world(pos4, origin)
    nr = np.asarray(nrm4, _F)[..., :3]
    out = np.zeros(P.shape[:-1] + (4,), _F) if base is None else np.array(base, _F, copy=True)
    if out.shape != P.shape[:-1] + (4,):
        raise ValueError("base must be [..., 4] over the images' pixels")
    S = out[..., :3].copy()
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for i in range(n):
            if kind == "suns":
                s = pts[i]
                dot = (nr[..., 0] * s[0] + nr[..., 1] * s[1]) + nr[..., 2] * s[2]
                lam = np.fmax(_F(0.0), dot)
            else:
                l = pts[i]
                length = _length((wpos - l) + _F(0.0))
                e = l - wpos
                dot = (nr[..., 0] * e[..., 0] + nr[..., 1] * e[..., 1]) + nr[..., 2] * e[..., 2]
                lam = np.fmax(_F(0.0), dot / length)
            bit = ((masks[i // SUM_CHUNK] >> np.uint64(i % SUM_CHUNK)) & np.uint64(1)) != 0
            k = np.where(bit, lam, _F(0.0)).astype(_F)
            S = S + col[i] * k[..., None]
    assert S.dtype == _F
    surface = ~((P[..., 0] == 0) & (P[..., 1] == 0) & (P[..., 2] == 0))
    out[..., :3] = np.where(surface[..., None], S, out[..., :3])
    return out


def light_model_buffer(rgba, pos4, buf):
    """What sf_light_image_buffer makes of the RGBA8 image `rgba` [..., 4]: a new uint8 array. buf [..., 4] is the
    light buffer. A miss pixel stays; else each of r, g, b becomes uint8(min(c buf.c + 0.5, 255)); alpha stays."""
    out = np.array(rgba, np.uint8, copy=True)
    P = np.asarray(pos4, _F)[..., :3]
    E = np.asarray(buf, _F)[..., :3]
    with np.errstate(invalid="ignore", over="ignore"):
        rgb = np.fmin(out[..., :3].astype(_F) * E + _F(0.5), _F(255.0))
    assert rgb.dtype == _F
    surface = ~((P[..., 0] == 0) & (P[..., 1] == 0) & (P[..., 2] == 0))
    out[..., :3] = np.where(surface[..., None], rgb.astype(np.uint8), out[..., :3])
    return out


def sky_colours(dirs, zenith=(0.25, 0.45, 1.0), horizon=(1.0, 0.8, 0.6), up=(0.0, 0.0, 1.0)):
    """Colours [n, 3] float32 for the sky directions dirs [n, 3]: a two-colour gradient by elevation, pre-divided by
    n, so the colours of a whole dome sum to about one sky. In float64 t_i = clip(dirs[i] . up / (|dirs[i]| |up|), 0, 1)
    (0 at the horizon, 1 at the zenith) and colour_i = (horizon + (zenith - horizon) t_i) / n, then rounded."""
    D = np.asarray(dirs, np.float64).reshape(-1, 3)
    n = _count(D.shape[0], SUM_MAX)
    z = np.asarray(zenith, np.float64).reshape(3)
    h = np.asarray(horizon, np.float64).reshape(3)
    if not ((np.isfinite(z) & (z >= 0)).all() and (np.isfinite(h) & (h >= 0)).all()):
        raise ValueError("colour components must be finite and not negative")
    _, _, w = _frame(up, "up")
    norm = np.linalg.norm(D, axis=-1)
    if not (np.isfinite(norm) & (norm > 0)).all():
        raise ValueError("every direction must be finite and not zero")
    t = np.clip((D @ w) / norm, 0.0, 1.0)
    return ((h + (z - h) * t[:, None]) / n).astype(_F)


# --- ambient occlusion about each pixel's normal (sf_trace_ao_to, sf_trace_ao_sum_to) ------------------------------
AO_SAMPLES_MAX = 64      # SF_AO_SAMPLES_MAX: one bit of the mask word per sample


def ao_samples(n, kind="cosine"):
    """n local-frame unit samples h [n, 3] over the hemisphere h.z > 0, the `samples` of trace_ao: a golden-angle
    spiral, made in float64 and rounded to float32. Deterministic. With u_i = (i + 0.5) / n and
    theta_i = i pi (3 - sqrt 5): kind "cosine" (density proportional to h.z) has radius sqrt(u_i) and
    h.z = sqrt(1 - u_i); kind "uniform" (equal solid angle) has h.z = u_i and radius sqrt(1 - u_i^2);
    h = (radius cos(theta_i), radius sin(theta_i), h.z)."""
    n = _count(n, AO_SAMPLES_MAX)
    if kind not in ("cosine", "uniform"):
        raise ValueError("kind is 'cosine' or 'uniform'")
    i = np.arange(n, dtype=np.float64)
    u = (i + 0.5) / n
    th = i * _GOLDEN
    if kind == "cosine":
        r, z = np.sqrt(u), np.sqrt(1.0 - u)
    else:
        r, z = np.sqrt(1.0 - u * u), u
    return np.stack([r * np.cos(th), r * np.sin(th), z], axis=-1).astype(_F)


def ao_colours(samples, colour=(1.0, 1.0, 1.0), kind="cosine"):
    """Colours [n, 3] float32 for trace_ao_sum that make the sum the cosine-weighted mean of the sky `colour` over the
    open part of the hemisphere: colour / n for a "cosine" sample set (the weighting is in the samples' density),
    colour 2 h.z / n for a "uniform" one. Formed in float64, then rounded."""
    h = np.asarray(samples, np.float64).reshape(-1, 3)
    n = _count(h.shape[0], AO_SAMPLES_MAX)
    if kind not in ("cosine", "uniform"):
        raise ValueError("kind is 'cosine' or 'uniform'")
    c = np.asarray(colour, np.float64).reshape(3)
    if not (np.isfinite(c) & (c >= 0)).all():
        raise ValueError("colour components must be finite and not negative")
    wgt = np.full(n, 1.0 / n) if kind == "cosine" else 2.0 * h[:, 2] / n
    if not (np.isfinite(wgt) & (wgt >= 0)).all():
        raise ValueError("a uniform sample set needs finite h.z >= 0")
    return (wgt[:, None] * c).astype(_F)


AO_SPIN_MAX = 8          # SF_AO_SPIN_MAX: the spin table is at most 8 x 8


def ao_spins(size, phase=0.0):
    """The spin table [size, size, 2] float32 of trace_ao(spin=...): entry k = y size + x holds (cos, sin) of the angle
    2 pi ((7 k mod size^2) + 0.5) / size^2, formed in float64 and rounded. The size^2 angles are evenly spaced over the
    turn, and 7 k mod size^2 keeps neighbouring pixels' angles apart (7 is coprime to size^2 for every size but 7, where
    the table repeats 7 angles); any size x size window of pixels holds every entry once.
    phase, in turns, is added to every entry's angle (2 pi phase, in float64): a frame's own turn of the whole table
    for light_accumulate (ao_phase). phase == 0 takes the expression above unchanged, bit for bit."""
    size = int(size)
    if not 1 <= size <= AO_SPIN_MAX:
        raise ValueError(f"size is 1..{AO_SPIN_MAX}")
    phase = float(phase)
    if not np.isfinite(phase):
        raise ValueError("phase must be finite")
    m = size * size
    k = np.arange(m, dtype=np.int64)
    ang = 2.0 * np.pi * (((7 * k) % m) + 0.5) / m
    if phase != 0.0:
        ang = ang + 2.0 * np.pi * phase
    return np.stack([np.cos(ang), np.sin(ang)], axis=-1).astype(_F).reshape(size, size, 2)


AO_PHASE_STEP = 0.7548776662466927   # 1 / the plastic number (the real root of x^3 = x + 1)


def ao_phase(frame):
    """The phase, in turns, of frame `frame`'s spin table: frac(frame 0.7548776662466927), the additive sequence of the
    plastic number's reciprocal. NOT THE GOLDEN RATIO: ao_samples' azimuths advance by the golden angle, a turn of
    frac(0.618 k) therefore lays frame k's samples onto the azimuths other frames' samples already hold, and 16 such
    frames accumulated measured WORSE than one frame (RMS 0.236 against 0.170 on the 80 x 45 fixture, n = 4). A step
    that is no multiple of the golden angle's fraction of a turn keeps the frames' sample sets apart."""
    return float(np.modf(float(frame) * AO_PHASE_STEP)[0])


def _spin_of(spin, shape):
    """(c, s) float32, each broadcastable over the normals of `shape` [...]: one pair as given, or a table
    [size, size, 2] tiled over the image's pixel coordinates -- pixel (x, y) takes entry (y % size, x % size)."""
    t = np.asarray(spin, _F)
    if t.shape == (2,):
        return t[0], t[1]
    if t.ndim != 3 or t.shape[0] != t.shape[1] or t.shape[2] != 2 or not 1 <= t.shape[0] <= AO_SPIN_MAX:
        raise ValueError(f"spin is one (c, s) pair or a table [size, size, 2], size 1..{AO_SPIN_MAX}")
    if len(shape) != 2:
        raise ValueError("a spin table needs a normal image [H, W, 3 | 4]")
    size = t.shape[0]
    e = t[np.arange(shape[0])[:, None] % size, np.arange(shape[1])[None, :] % size]
    return e[..., 0, None], e[..., 1, None]


def ao_basis(nrm4, spin=None):
    """Step 2 of sf_trace_ao_to's definition: the frame (T, B, N), each [..., 3] float32, about the normals
    nrm4 [..., 3 | 4], used as given (not normalised). The branch-free frame of Duff et al., one rounding per
    operation in the order written: sg = copysign(1, N.z), a = -1 / (sg + N.z), b = (N.x N.y) a,
    T = (1 + sg ((N.x N.x) a), sg b, -sg N.x), B = (b, sg + (N.y N.y) a, -N.y). Orthonormal, to rounding, for a
    unit N; sg + N.z is never zero.
    spin (trace_ao(spin=...), sf_trace_ao_spin_to): one (c, s) pair, or a table [size, size, 2] indexed by the pixel
    coordinates of the normal image [H, W, 3 | 4]; the frame is then turned about N, per component
    T' = (T c) + (B s), B' = (B c) - (T s), one rounding per operation. None: not turned, today's bits."""
    N = np.array(np.asarray(nrm4, _F)[..., :3], _F, copy=True)
    x, y, z = N[..., 0], N[..., 1], N[..., 2]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        sg = np.copysign(_F(1.0), z)
        a = _F(-1.0) / (sg + z)
        b = (x * y) * a
        T = np.stack([_F(1.0) + sg * ((x * x) * a), sg * b, -(sg * x)], axis=-1)
        B = np.stack([b, sg + (y * y) * a, -y], axis=-1)
        if spin is not None:
            c, s = _spin_of(spin, N.shape[:-1])
            T, B = (T * c) + (B * s), (B * c) - (T * s)
    assert T.dtype == _F and B.dtype == _F
    return T, B, N


def ao_directions(nrm4, samples, spin=None):
    """Step 3: the world directions s [n, ..., 3] of the local-frame samples h [n, 3] about the normals
    nrm4 [..., 3 | 4]: per component c, s_i.c = ((T.c h_i.x) + (B.c h_i.y)) + (N.c h_i.z) with (T, B, N) of ao_basis,
    one rounding per operation. For one normal [3 | 4] the result [n, 3] is the `dirs` of trace_suns that trace_ao
    equals on a constant normal image. spin: as ao_basis'; with one normal, one (c, s) pair."""
    T, B, N = ao_basis(nrm4, spin)
    h = np.asarray(samples, _F).reshape(-1, 3)
    _count(h.shape[0], AO_SAMPLES_MAX)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        s = np.stack([((T * hi[0]) + (B * hi[1])) + (N * hi[2]) for hi in h])
    assert s.dtype == _F
    return s


def ao_model(pos4, nrm4, origin, samples, distance, bias, spin=None):
    """Steps 1-4 of sf_trace_ao_to's definition up to the ray, stacked per sample as suns_model stacks them:
    (F [n, ..., 3], d [n, ..., 3], bound [n, ...], is_surface [...]) for a position image pos4 [..., 3 | 4] relative
    to `origin`, its normal image nrm4 and the samples [n, 3]. With s_i = ao_directions(nrm4, samples)[i] (a
    direction per pixel): w = origin + P, f_i = s_i tau, F_i = w + f_i the ray's origin, d_i = (w - F_i) + 0 its
    unnormalised direction, bound_i = |d_i| (1 - bias). is_surface is False where P == (0, 0, 0): no ray, every bit
    set. spin: as ao_basis' (sf_trace_ao_spin_to's definition); None is the unspun call."""
    if not 0.0 <= float(bias) < 1.0:
        raise ValueError("bias must be in [0, 1)")
    tau = _F(distance)
    if not (np.isfinite(tau) and tau > 0):
        raise ValueError("distance must be finite and > 0")
    P, w = _world(pos4, origin)
    s = ao_directions(nrm4, samples, spin)
    if s.shape[1:] != P.shape:
        raise ValueError("nrm4 and pos4 must have the same height and width")
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        f = s * tau
        Fo = w + f
        d = (w - Fo) + _F(0.0)
        bound = _length(d) * (_F(1.0) - _F(bias))
    is_surface = ~((P[..., 0] == 0) & (P[..., 1] == 0) & (P[..., 2] == 0))
    assert Fo.dtype == _F and d.dtype == _F and bound.dtype == _F
    return Fo, d, bound, is_surface


def ao_sum_model(base, pos4, masks, colours, accumulate=False):
    """What trace_ao_sum leaves in the light buffer: a new float32 array [..., 4]. sum_model with lam_i = 1: base
    [..., 4] is what the output held (read by an accumulating call only; None otherwise), masks [...] the uint64 words
    of trace_ao for the same samples, colours [n, 3] the call's (its default is float32(1) / float32(n) per
    component). A miss pixel (P == 0) keeps the base (an overwriting call: becomes 0). Else S = base.xyz (or 0), then
    for i = 0 .. n-1 in that order and per channel S = S + colours[i] (bit i ? 1 : 0); the result is (S, base.w)."""
    col = np.asarray(colours, _F).reshape(-1, 3)
    n = _count(col.shape[0], AO_SAMPLES_MAX)
    if not (np.isfinite(col) & (col >= 0)).all():
        raise ValueError("every colour component must be finite and not negative")
    P = np.asarray(pos4, _F)[..., :3]
    mask = np.asarray(masks, np.uint64)
    if accumulate:
        if base is None:
            raise ValueError("an accumulating call needs its base")
        out = np.array(base, _F, copy=True)
    else:
        out = np.zeros(P.shape[:-1] + (4,), _F)
    if out.shape != P.shape[:-1] + (4,) or mask.shape != P.shape[:-1]:
        raise ValueError("base must be [..., 4] and masks [...] over the images' pixels")
    S = out[..., :3].copy()
    for i in range(n):
        bit = ((mask >> np.uint64(i)) & np.uint64(1)) != 0
        k = np.where(bit, _F(1.0), _F(0.0)).astype(_F)
        S = S + col[i] * k[..., None]
    assert S.dtype == _F
    surface = ~((P[..., 0] == 0) & (P[..., 1] == 0) & (P[..., 2] == 0))
    out[..., :3] = np.where(surface[..., None], S, out[..., :3])
    return out


# --- sky reflections about each pixel's mirror direction (sf_trace_mirror_to, sf_trace_mirror_sum_to) ---------------
def lobe_samples(n, exponent):
    """n local-frame unit samples h [n, 3] of a Phong lobe about +z (density proportional to h.z ^ exponent), the
    `samples` of trace_mirror: ao_samples' golden-angle spiral with another height. With u_i = (i + 0.5) / n and
    theta_i = i pi (3 - sqrt 5): h.z = (1 - u_i) ^ (1 / (exponent + 1)), radius sqrt(1 - h.z^2),
    h = (radius cos(theta_i), radius sin(theta_i), h.z); made in float64 and rounded to float32. exponent 1 is
    ao_samples(n)'s cosine distribution; a large exponent narrows the lobe towards the mirror direction."""
    n = _count(n, AO_SAMPLES_MAX)
    e = float(exponent)
    if not (np.isfinite(e) and e >= 0.0):
        raise ValueError("exponent must be finite and not negative")
    i = np.arange(n, dtype=np.float64)
    u = (i + 0.5) / n
    th = i * _GOLDEN
    z = (1.0 - u) ** (1.0 / (e + 1.0))
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(th), r * np.sin(th), z], axis=-1).astype(_F)


def mirror_axes(pos4, nrm4, origin=None, eye=None):
    """Steps 2 and 3 of sf_trace_mirror_to's definition: the image [..., 4] float32 with the mirror axis A in xyz and
    .w = 0 -- the normal image on which trace_ao equals trace_mirror. eye None: V = P, the positions as given
    (`origin` is not read); else V = (origin + P) - eye per component, other bits even for eye == origin. Then, one
    rounding per operation: nv = ((N.x V.x) + (N.y V.y)) + (N.z V.z), k = nv + nv, R = V - (k N),
    len = sqrt(((R.x R.x) + (R.y R.y)) + (R.z R.z)), A = R / len. A miss of the frame (P == 0 with eye None) gives
    NaN: nothing reads it."""
    P = np.asarray(pos4, _F)[..., :3]
    N = np.asarray(nrm4, _F)[..., :3]
    if P.shape != N.shape:
        raise ValueError("nrm4 and pos4 must have the same height and width")
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        if eye is None:
            V = P
        else:
            if origin is None:
                raise ValueError("an eye needs the origin the positions are relative to")
            V = (np.asarray(origin, _F).reshape(3) + P) - np.asarray(eye, _F).reshape(3)
        nv = (N[..., 0] * V[..., 0] + N[..., 1] * V[..., 1]) + N[..., 2] * V[..., 2]
        k = nv + nv
        R = V - k[..., None] * N
        A = R / _length(R)[..., None]
    assert A.dtype == _F
    out = np.zeros(A.shape[:-1] + (4,), _F)
    out[..., :3] = A
    return out


def mirror_model(pos4, nrm4, origin, samples, distance, bias, spin=None, eye=None):
    """Steps 1-4 of sf_trace_mirror_to's definition up to the ray: ao_model on the mirror axes --
    (F [n, ..., 3], d [n, ..., 3], bound [n, ...], is_surface [...])."""
    return ao_model(pos4, mirror_axes(pos4, nrm4, origin, eye), origin, samples, distance, bias, spin=spin)


def sky_gradient(dirs, zenith=(0.25, 0.45, 1.0), horizon=(1.0, 0.8, 0.6), up=(0.0, 0.0, 1.0)):
    """E [..., 3] float32 of sf_trace_mirror_sum_to's definition for the directions dirs [..., 3], one rounding per
    operation: u = ((s.x up.x) + (s.y up.y)) + (s.z up.z), t = min(max(u, 0), 1) and +0 where u is -0 or NaN,
    E.c = horizon.c + ((zenith.c - horizon.c) t). `up` is used as given, not normalised. NOT sky_colours, which works
    in float64, normalises and pre-divides by n."""
    s = np.asarray(dirs, _F)
    z = np.asarray(zenith, _F).reshape(3)
    h = np.asarray(horizon, _F).reshape(3)
    w = np.asarray(up, _F).reshape(3)
    if not ((np.isfinite(z) & (z >= 0)).all() and (np.isfinite(h) & (h >= 0)).all()):
        raise ValueError("colour components must be finite and not negative")
    if not np.isfinite(w).all():
        raise ValueError("up must be finite")
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        u = (s[..., 0] * w[0] + s[..., 1] * w[1]) + s[..., 2] * w[2]
        t = np.where(u > 0, np.where(u < 1, u, _F(1.0)), _F(0.0)).astype(_F)
        E = h + (z - h) * t[..., None]
    assert E.dtype == _F
    return E


def mirror_sum_model(base, pos4, nrm4, origin, masks, samples, colours, zenith=(1.0, 1.0, 1.0),
                     horizon=(1.0, 1.0, 1.0), up=(0.0, 0.0, 1.0), accumulate=False, spin=None, eye=None):
    """What trace_mirror_sum leaves in the light buffer: a new float32 array [..., 4]. ao_sum_model with the factor of
    entry i the sky's colour along that pixel's own ray: S = S + colours[i] (bit i ? E_i : 0) per channel, in index
    order, with E_i = sky_gradient(s_i) and s_i = ao_directions(mirror_axes(...), samples, spin)[i]. masks [...] are
    the uint64 words of trace_mirror for the same samples, spin and eye."""
    col = np.asarray(colours, _F).reshape(-1, 3)
    n = _count(col.shape[0], AO_SAMPLES_MAX)
    if not (np.isfinite(col) & (col >= 0)).all():
        raise ValueError("every colour component must be finite and not negative")
    P = np.asarray(pos4, _F)[..., :3]
    mask = np.asarray(masks, np.uint64)
    s = ao_directions(mirror_axes(pos4, nrm4, origin, eye), samples, spin)
    if s.shape[0] != n:
        raise ValueError("one colour per sample")
    if accumulate:
        if base is None:
            raise ValueError("an accumulating call needs its base")
        out = np.array(base, _F, copy=True)
    else:
        out = np.zeros(P.shape[:-1] + (4,), _F)
    if out.shape != P.shape[:-1] + (4,) or mask.shape != P.shape[:-1]:
        raise ValueError("base must be [..., 4] and masks [...] over the images' pixels")
    S = out[..., :3].copy()
    for i in range(n):
        bit = ((mask >> np.uint64(i)) & np.uint64(1)) != 0
        E = sky_gradient(s[i], zenith, horizon, up)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            S = S + col[i] * np.where(bit[..., None], E, _F(0.0)).astype(_F)
    assert S.dtype == _F
    surface = ~((P[..., 0] == 0) & (P[..., 1] == 0) & (P[..., 2] == 0))
    out[..., :3] = np.where(surface[..., None], S, out[..., :3])
    return out


# --- the edge-aware box filter of the light buffer (sf_light_filter_to) ---------------------------------------------
def light_filter_model(buf, pos4, nrm4, size, normal_min=0.9, plane_max=0.02):
    """What sf_light_filter_to makes of the light buffer buf [H, W, 4]: a new float32 array, sf.h's definition on the
    host. A miss pixel (P == 0) is copied. Else the taps q = p + (dx, dy), dy outer and dx inner, both from -(size // 2)
    to size - 1 - size // 2, are visited in that order; a tap outside the image or a miss is skipped; q == p is
    accepted; any other tap iff ((N_p.x N_q.x) + (N_p.y N_q.y)) + (N_p.z N_q.z) >= normal_min and e e <= k2 pp with
    e = ((N_p.x D.x) + (N_p.y D.y)) + (N_p.z D.z), D = P_q - P_p, pp = |P_p|^2 summed in that order and
    k2 = float32(plane_max) float32(plane_max); a comparison with a NaN rejects. Per channel S = S + buf[q] over the
    accepted taps in visiting order, out.xyz = S / float32(count), out.w = buf[p].w."""
    size = int(size)
    if not 1 <= size <= AO_SPIN_MAX:
        raise ValueError(f"size is 1..{AO_SPIN_MAX}")
    nmin, pmax = _F(normal_min), _F(plane_max)
    if np.isnan(nmin) or not (np.isfinite(pmax) and pmax >= 0):
        raise ValueError("normal_min must not be NaN; plane_max must be finite and not negative")
    src = np.asarray(buf, _F)
    P = np.asarray(pos4, _F)[..., :3]
    N = np.asarray(nrm4, _F)[..., :3]
    if src.ndim != 3 or src.shape[-1] != 4 or P.shape != src.shape[:2] + (3,) or N.shape != P.shape:
        raise ValueError("buf, pos4 and nrm4 must be [H, W, 4] images of one size")
    H, W = src.shape[:2]
    k2 = pmax * pmax
    surface = ~((P[..., 0] == 0) & (P[..., 1] == 0) & (P[..., 2] == 0))
    S = np.zeros((H, W, 3), _F)
    count = np.zeros((H, W), np.int64)
    lo, hi = -(size // 2), size - 1 - size // 2
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        pp = (P[..., 0] * P[..., 0] + P[..., 1] * P[..., 1]) + P[..., 2] * P[..., 2]
        limit = k2 * pp
        for dy in range(lo, hi + 1):
            for dx in range(lo, hi + 1):
                # the pixels p whose tap q = p + (dx, dy) lies in the image, and their taps
                ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
                yq, xq = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
                Pp, Np, Pq, Nq = P[ys, xs], N[ys, xs], P[yq, xq], N[yq, xq]
                if dx == 0 and dy == 0:
                    ok = np.ones(Pp.shape[:2], bool)
                else:
                    nn = (Np[..., 0] * Nq[..., 0] + Np[..., 1] * Nq[..., 1]) + Np[..., 2] * Nq[..., 2]
                    D = Pq - Pp
                    e = (Np[..., 0] * D[..., 0] + Np[..., 1] * D[..., 1]) + Np[..., 2] * D[..., 2]
                    ok = surface[yq, xq] & (nn >= nmin) & ((e * e) <= limit[ys, xs])
                S[ys, xs] = np.where(ok[..., None], S[ys, xs] + src[yq, xq, :3], S[ys, xs])
                count[ys, xs] += ok
        mean = S / np.maximum(count, 1).astype(_F)[..., None]
    assert mean.dtype == _F
    out = np.array(src, _F, copy=True)
    out[..., :3] = np.where(surface[..., None], mean, src[..., :3])
    return out


# --- the light buffer over several frames (sf_reproject_matrix, sf_light_accumulate_to) ------------------------------
def reproject_matrix(view):
    """sf_reproject_matrix on the host: the inverse [9] float32 (row-major 3 x 3) of the ray generation of the view
    (origin, top-left, top-right, bottom-left; 12 floats). a = tr - tl, b = bl - tl, c = tl - o in float32, promoted to
    float64 and put as the columns of a matrix; its inverse is adjugate over determinant in float64, one rounding per
    operation, in sf.h's order: the rows are (b x c) / det, (c x a) / det, (a x b) / det with
    det = ((a.x bc.x) + (a.y bc.y)) + (a.z bc.z); each entry is then rounded once to float32. m (a u + b v + c) =
    (u, v, 1) to rounding."""
    v = np.concatenate([np.asarray(x, _F).reshape(-1) for x in view]) if isinstance(view, (tuple, list)) \
        else np.asarray(view, _F).reshape(-1)
    if v.shape != (12,) or not np.isfinite(v).all():
        raise ValueError("view is 12 finite floats: origin, top-left, top-right, bottom-left")
    o, tl, tr, bl = v[0:3], v[3:6], v[6:9], v[9:12]
    a, b, c = ((tr - tl).astype(np.float64), (bl - tl).astype(np.float64), (tl - o).astype(np.float64))

    def cross(p, q):
        return np.array([p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]], np.float64)
    bc, ca, ab = cross(b, c), cross(c, a), cross(a, b)
    det = (a[0] * bc[0] + a[1] * bc[1]) + a[2] * bc[2]
    if det == 0.0 or not np.isfinite(det):
        raise ValueError("the view's corners and origin span no volume")
    return np.concatenate([bc / det, ca / det, ab / det]).astype(_F)


def light_accumulate_model(buf, pos4, nrm4, origin, hist, hist_pos4, hist_nrm4, hist_view, max_history=16,
                           normal_min=0.9, plane_max=0.02, hist_m=None):
    """What sf_light_accumulate_to makes of the light buffer buf [H, W, 4] of the current frame (pos4, nrm4, relative to
    `origin`) and the history hist [H, W, 4] (hist_pos4, hist_nrm4) seen from hist_view (origin, top-left, top-right,
    bottom-left): (out [H, W, 4] float32, accepted [H, W] bool, taps [H, W, 2] int64), sf.h's definition on the host.
    taps holds (X, Y) of each pixel's tap, (-1, -1) where there is none (a miss of the frame, q.z <= 0, a tap off the
    image, a NaN). hist_m [9] given: used in place of reproject_matrix(hist_view), whose origin alone is then read.
      1. P == 0: out = (buf.xyz, 0).
      2. w = origin + P, D = w - o', q.k = ((m[3k] D.x) + (m[3k+1] D.y)) + (m[3k+2] D.z).
      3. X = floor((q.x / q.z) float32(W) + 0.5), Y likewise; the tap exists iff q.z > 0, 0 <= X < W, 0 <= Y < H.
      4. accepted iff P' != 0, h.w >= 1, ((N.x N'.x) + (N.y N'.y)) + (N.z N'.z) >= normal_min and e e <= k2 pp with
         E = (o' + P') - w, e = ((N.x E.x) + (N.y E.y)) + (N.z E.z), pp = |P|^2 summed in that order,
         k2 = float32(plane_max) float32(plane_max).
      5. accepted: m = min(h.w + 1, float32(max_history)), out = (h + (buf - h) / m, m); else (buf.xyz, 1).
    One float32 rounding per operation; a comparison with a NaN is false."""
    mh = int(max_history)
    if not 1 <= mh <= 65535:
        raise ValueError("max_history is 1..65535")
    nmin, pmax = _F(normal_min), _F(plane_max)
    if np.isnan(nmin) or not (np.isfinite(pmax) and pmax >= 0):
        raise ValueError("normal_min must not be NaN; plane_max must be finite and not negative")
    src, old = np.asarray(buf, _F), np.asarray(hist, _F)
    P, w = _world(pos4, origin)
    N = np.asarray(nrm4, _F)[..., :3]
    Pq_all = np.asarray(hist_pos4, _F)[..., :3]
    Nq_all = np.asarray(hist_nrm4, _F)[..., :3]
    if src.ndim != 3 or src.shape[-1] != 4 or old.shape != src.shape or any(
            a.shape != src.shape[:2] + (3,) for a in (P, N, Pq_all, Nq_all)):
        raise ValueError("the six images must be [H, W, 4] of one size")
    hv = np.concatenate([np.asarray(x, _F).reshape(-1) for x in hist_view]) if isinstance(hist_view, (tuple, list)) \
        else np.asarray(hist_view, _F).reshape(-1)
    ho = hv[:3]
    m = reproject_matrix(hv) if hist_m is None else np.asarray(hist_m, _F).reshape(9)
    H, W = src.shape[:2]
    fW, fH, k2 = _F(W), _F(H), pmax * pmax
    surface = ~((P[..., 0] == 0) & (P[..., 1] == 0) & (P[..., 2] == 0))
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        D = w - ho
        q = [(m[3 * k] * D[..., 0] + m[3 * k + 1] * D[..., 1]) + m[3 * k + 2] * D[..., 2] for k in range(3)]
        X = np.floor((q[0] / q[2]) * fW + _F(0.5))
        Y = np.floor((q[1] / q[2]) * fH + _F(0.5))
        assert X.dtype == _F and Y.dtype == _F
        exists = surface & (q[2] > 0) & (X >= 0) & (X < fW) & (Y >= 0) & (Y < fH)
        xi = np.where(exists, X, 0).astype(np.int64)
        yi = np.where(exists, Y, 0).astype(np.int64)
        Pq, Nq, h = Pq_all[yi, xi], Nq_all[yi, xi], old[yi, xi]
        nn = (N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]
        E = (ho + Pq) - w
        e = (N[..., 0] * E[..., 0] + N[..., 1] * E[..., 1]) + N[..., 2] * E[..., 2]
        pp = (P[..., 0] * P[..., 0] + P[..., 1] * P[..., 1]) + P[..., 2] * P[..., 2]
        there = ~((Pq[..., 0] == 0) & (Pq[..., 1] == 0) & (Pq[..., 2] == 0))
        accepted = exists & there & (h[..., 3] >= 1) & (nn >= nmin) & ((e * e) <= (k2 * pp))
        cnt = np.minimum(h[..., 3] + _F(1.0), _F(mh))
        cnt = np.where(accepted, cnt, _F(1.0)).astype(_F)
        blend = h[..., :3] + (src[..., :3] - h[..., :3]) / cnt[..., None]
    assert blend.dtype == _F
    out = np.empty(src.shape, _F)
    out[..., :3] = np.where(accepted[..., None], blend, src[..., :3])
    out[..., 3] = np.where(accepted, cnt, np.where(surface, _F(1.0), _F(0.0)))
    taps = np.where(exists[..., None], np.stack([xi, yi], axis=-1), -1)
    return out, accepted, taps
