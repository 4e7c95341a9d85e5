"""Oracle helper of the directional-light tests (tests/test_sun_host.py, tests/test_gpu_sun.py,
tests/test_gpu_shadow_lod.py).

A pixel's sun ray starts at its own origin F = w + s tau: it is sf_trace_rays_to's ray from F, so the oracle traces it
with root = sf.root_transform(F) -- one dirscheck.oracle_rays call per surface pixel (rayscheck.oracle_multi), for the
origin, direction and bound that sphereflake_amd.lights.sun_model states on the host, and with the LOD constant the
shadow traces are set to. The frames are the oracle's own."""
import functools

import numpy as np

from sphereflake_amd import lights
from oracle import pyoracle
from rayscheck import LOD, frame, oracle_multi

FLT_MAX = np.finfo(np.float32).max
TAU = 4.0
B10 = 2.0 ** -10
# towards the sun: `side` is the direction of shadowcheck's side light, `cam` t3's camera position (the sun behind
# the viewer)
VECTORS = {"side": (-1.5, -2.5, 2.0), "cam": (-5.4098, -7.2139, 1.19006)}
CASES = (("t1", "side"), ("t3", "cam"))
T3_CLOSEST = 0.1258   # t3's closest camera distance, as the matched constant's t_ref


def direction(name):
    return lights.sun_direction(VECTORS[name])


def matched():
    """The constant that gives a sun ray at distance TAU the camera's detail at t3's closest distance (~394.7)."""
    return float(lights.matched_lod(TAU, T3_CLOSEST, 70.0))


def oracle_sun_rays(children, pos4, origin, s, tau, lod, every=1):
    """The oracle's closest-hit min_t [...] of the sun ray of every `every`-th surface pixel in row-major order
    (FLT_MAX elsewhere) and the mask of the pixels traced. Independent of the bias."""
    Fo, d, _, surf = lights.sun_model(pos4, origin, s, tau, 0.0)
    pick = np.zeros(surf.shape, bool).reshape(-1)
    pick[np.nonzero(surf.reshape(-1))[0][::every]] = True
    pick = pick.reshape(surf.shape)
    mint = np.full(surf.shape, FLT_MAX, np.float32)
    deepest = 0
    if pick.any():
        r = oracle_multi(children, Fo[pick], d[pick], 1, lod=lod)
        mint[pick] = r["minT"]
        deepest = r["stats"]["max_depth"]
    return mint, pick, deepest


def vis_of(pos4, origin, s, tau, bias, mint, pick=None):
    """The definition's step 5 on the oracle's min_t: 0 where a traced surface pixel has min_t < bound, else 255."""
    _, _, bound, surf = lights.sun_model(pos4, origin, s, tau, bias)
    if pick is not None:
        surf = surf & pick
    with np.errstate(invalid="ignore"):
        return np.where(surf & (mint < bound), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def frame_rays(name, dir_name, tau=TAU, variant="avx", lod=None, every=1):
    """(min_t, traced mask, deepest node) of fixture `name`'s own oracle frame (computed once, shared). lod None: the
    variant's own constant."""
    S = pyoracle.load_setup(name)
    mint, pick, deepest = oracle_sun_rays(S["children"], frame(name, variant)["pos4"], S["origin"], direction(dir_name),
                                          tau, LOD[variant] if lod is None else lod, every)
    mint.setflags(write=False)
    pick.setflags(write=False)
    return mint, pick, deepest


def oracle_vis(name, dir_name, bias, tau=TAU, variant="avx", lod=None):
    S = pyoracle.load_setup(name)
    mint, _, _ = frame_rays(name, dir_name, tau, variant, lod)
    return vis_of(frame(name, variant)["pos4"], S["origin"], direction(dir_name), tau, bias, mint)
