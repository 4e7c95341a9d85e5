"""Host statement of the point-light arithmetic of ``Sphereflake.trace_shadow`` / ``Sphereflake.light_image``
(sf_trace_shadow_to, sf_light_image; the definition is in include/sphereflake/sf.h).

Everything is numpy float32, one rounding per operation, in the order the header gives -- the device kernels form
the same bits (tests/test_gpu_shadow.py).

A shadow ray is traced FROM THE LIGHT towards the surface point and its nearest hit compared with the distance to
the point, so no ray starts on the flake and the reference's ``tca >= 0`` quirk (sphereflake_amd/rays.py) cannot
bite while the light stays outside the flake's bounding ball (radius 2 about its centre). The level of detail is
the light's: a node refines by its distance from the light, so a far light casts coarse shadows.
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
