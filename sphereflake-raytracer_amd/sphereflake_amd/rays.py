"""Host-side ray generators for ``Sphereflake.trace_rays`` / ``Sphereflake.probe_rays`` (sf_trace_rays_to).

All return float32 numpy arrays; directions are *unnormalised* (the renderer normalises each one the way the
reference normalises a pixel's ray, SIMD_AVX.h:170-180) and carry no -0 component.

What a secondary ray sees is the reference's answer, quirk included: a sphere whose centre is behind the ray is
rejected even when the ray starts inside it (``tca >= 0``, SIMD_AVX.h:247-258), and the root's bounding ball is
tested first -- so a ray that starts on the flake and heads away from the flake's centre sees nothing at all.
``reflect`` and ``towards`` are for rays that head inwards; they are no occlusion query. Shadows from a point light
are traced the other way round, from the light towards the surface point, where the quirk cannot bite:
``Sphereflake.trace_shadow`` (sphereflake_amd/lights.py, sf_trace_shadow_to).
"""
from __future__ import annotations

import numpy as np

from . import dirs as _dirs

_F = np.float32


def look_ahead(camera, steps: int, step: float):
    """The look-ahead brake's rays: the reference brakes on the nearest sphere seen from where the camera IS
    (GetClosestSphereDistance, main.cpp:213); this probes the six move axes (dirs.move_axes, main.cpp:214-242) from
    where it WILL be after 1..steps moves of length `step` along each of them.

    Returns (origins [6 * steps, 3], dirs [36 * steps, 3]) for rays_per_origin = 6: origin a * steps + (k - 1) is
    position + axis_a * (k * step) in float32, and its six rays are the six axes in move_axes' order."""
    steps = int(steps)
    if steps < 1:
        raise ValueError("steps must be at least 1")
    axes = _dirs.move_axes(camera)
    pos = np.asarray(camera.GetPosition(), _F).reshape(1, 1, 3)
    k = (np.arange(1, steps + 1, dtype=_F) * _F(step)).reshape(1, steps, 1)
    origins = (pos + axes.reshape(6, 1, 3) * k).reshape(6 * steps, 3)
    assert origins.dtype == _F
    d = np.broadcast_to(axes.reshape(1, 6, 3), (6 * steps, 6, 3)).reshape(36 * steps, 3)
    return np.ascontiguousarray(origins), np.ascontiguousarray(d)


def _hits(pos4, nrm4, origin, eps):
    """(mask of hits, world hit points offset by eps n, unit normals) of a downloaded G-buffer, in float32."""
    pos = np.asarray(pos4, _F)[..., :3]
    nrm = np.asarray(nrm4, _F)[..., :3]
    if pos.shape != nrm.shape:
        raise ValueError("pos4 and nrm4 differ in shape")
    mask = (nrm != 0).any(axis=-1)   # a miss is (0, 0, 0, 1) in both channels
    o = np.broadcast_to(np.asarray(origin, _F), pos.shape)
    p = (o[mask] + pos[mask]) + nrm[mask] * _F(eps)
    return mask, p, nrm[mask]


def reflect(pos4, nrm4, origin, dirs, eps: float = 1e-3):
    """Mirror reflections off the hits of a traced frame: `origin` [3] (or one per ray) and `dirs` [..., 3 | 4] are
    what the frame was traced with, pos4 / nrm4 [..., 4] what it returned. Returns (origins [M, 3], dirs [M, 3],
    mask [...]) for the M hits: the world hit point origin + pos, offset by eps n, and d - 2 (d . n) n for the
    normalised incoming direction d."""
    mask, p, n = _hits(pos4, nrm4, origin, eps)
    d = np.asarray(dirs, np.float64)[..., :3][mask]
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    n64 = n.astype(np.float64)
    r = d - 2.0 * (d * n64).sum(axis=-1, keepdims=True) * n64
    return np.ascontiguousarray(p), np.ascontiguousarray(r.astype(_F) + _F(0.0)), mask


def towards(pos4, nrm4, origin, point, eps: float = 1e-3):
    """Rays from the hits of a traced frame towards `point` [3] (a light, a probe): (origins [M, 3], dirs [M, 3],
    mask [...]) for the M hits, origins as for reflect, dirs = point - origin."""
    mask, p, _ = _hits(pos4, nrm4, origin, eps)
    t = np.asarray(point, _F).reshape(1, 3) - p
    return np.ascontiguousarray(p), np.ascontiguousarray(t + _F(0.0)), mask
