"""Host-side direction generators for ``Sphereflake.trace_dirs`` / ``Sphereflake.probe`` (sf_trace_dirs_to).

All return float32 numpy arrays of *unnormalised* directions: the renderer normalises each one the way the
reference normalises a pixel's ray (SIMD_AVX.h:170-180), so a direction image built here and the frame's own ray
generation give the same bits where they describe the same rays.
"""
from __future__ import annotations

import numpy as np

_F = np.float32


def _v3(v) -> np.ndarray:
    a = np.asarray(v, _F).reshape(-1)
    if a.size != 3:
        raise ValueError(f"expected 3 floats, got {a.size}")
    return a


def pinhole(origin, tl, tr, bl, W: int, H: int) -> np.ndarray:
    """The frame's own pre-normalised pixel vectors, [H, W, 3]: pixel (x, y) is
    ((tl + (tr - tl) u) + (bl - tl) v) - origin with u = x / W, v = y / H in float32, the operation order of the
    reference's ray generation (Sphereflake.cpp:149-150, 162-167). Tracing this image gives the frame Render()
    gives, bit for bit."""
    o, tl, tr, bl = _v3(origin), _v3(tl), _v3(tr), _v3(bl)
    W, H = int(W), int(H)
    u = (np.arange(W, dtype=_F) / _F(W)).reshape(1, W, 1)
    v = (np.arange(H, dtype=_F) / _F(H)).reshape(H, 1, 1)
    dh = (tr - tl).reshape(1, 1, 3)
    dv = (bl - tl).reshape(1, 1, 3)
    d = ((tl.reshape(1, 1, 3) + dh * u) + dv * v) - o.reshape(1, 1, 3)
    assert d.dtype == _F
    return np.ascontiguousarray(d)


def _unit(v) -> np.ndarray:
    a = np.asarray(v, np.float64).reshape(3)
    n = np.linalg.norm(a)
    if not n > 0.0:
        raise ValueError("zero-length vector")
    return a / n


def equirect(W: int, H: int, forward, up) -> np.ndarray:
    """A 360 x 180 degree equirectangular panorama, [H, W, 3]. Pixel (x, y) samples its top-left corner like the
    frame's pixels do (u = x / W, v = y / H): longitude (u - 1/2) 2 pi to the right of `forward`, latitude
    (1/2 - v) pi towards `up` -- the image centre looks along `forward`, the left edge (and, one pixel on, the
    right edge) backwards, the top row along `up`. `up` is made orthogonal to `forward`. No component is -0."""
    f = _unit(forward)
    u0 = np.asarray(up, np.float64).reshape(3)
    u = _unit(u0 - f * np.dot(u0, f))
    r = np.cross(f, u)
    lon = ((np.arange(W, dtype=np.float64) / W) - 0.5) * (2.0 * np.pi)
    lat = (0.5 - (np.arange(H, dtype=np.float64) / H)) * np.pi
    cl, sl = np.cos(lon).reshape(1, W, 1), np.sin(lon).reshape(1, W, 1)
    cp, sp = np.cos(lat).reshape(H, 1, 1), np.sin(lat).reshape(H, 1, 1)
    d = cp * (cl * f.reshape(1, 1, 3) + sl * r.reshape(1, 1, 3)) + sp * u.reshape(1, 1, 3)
    return np.ascontiguousarray(d.astype(_F) + _F(0.0))   # (+ 0: a -0 component becomes +0)


def move_axes(camera) -> np.ndarray:
    """The six directions the reference's ProcessInput moves the camera along (main.cpp:214-242), [6, 3], in its
    key order D, A, S, W, Q, E: orientation * (+-1, 0, 0), (0, 0, +-1), (0, +-1, 0). The orientation's basis comes
    from the camera's image-plane corners (camera.h:37-53): x along top-right - top-left, y along top-left -
    bottom-left, z = x cross y (the camera looks along -z). Probing them (Sphereflake.probe) gives the distance to
    the nearest sphere along each move, which no pixel of the frame covers except W's."""
    _, tl, tr, bl = camera.corners()
    x = _unit(np.asarray(tr, np.float64) - np.asarray(tl, np.float64))
    y = _unit(np.asarray(tl, np.float64) - np.asarray(bl, np.float64))
    z = np.cross(x, y)
    return np.ascontiguousarray(np.stack([x, -x, z, -z, y, -y]).astype(_F) + _F(0.0))
