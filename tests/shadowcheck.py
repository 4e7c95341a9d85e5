"""Oracle helper of the point-light shadow tests (tests/test_shadow_host.py, tests/test_gpu_shadow.py).

A pixel's shadow ray starts at the light: it is sf_trace_rays_to's ray from the single origin `light`, so the oracle
traces it with root = sf.root_transform(light) in one dirscheck.oracle_rays call (tests/rayscheck.py), for the
direction and bound that sphereflake_amd.lights.shadow_model states on the host. The frames are the oracle's own."""
import functools

import numpy as np

import sphereflake_amd as sf
from sphereflake_amd import lights
from dirscheck import oracle_rays
from oracle import pyoracle
from rayscheck import LOD, frame

# (light, fixtures it is used with); counts at bias 2^-9 on the oracle, shadowed / lit of the surface pixels:
# t1 454 / 376 (of 830), t3 2505 / 1095 (of 3600); t3 3358 / 242; t1 618 / 212
LIGHTS = {"side": (-1.5, -2.5, 2.0), "top": (0.0, 0.0, 6.0), "low": (0.5, -3.0, 0.3)}
CASES = (("t1", "side"), ("t3", "side"), ("t3", "top"), ("t1", "low"))
INSIDE = (0.3, 0.2, 0.1)   # a light inside the flake's radius-2 ball: the reference's answer, quirk included


def oracle_shadow_rays(children, pos4, origin, light, variant="avx"):
    """(min_t [...], hit index [...]): the oracle's closest hit of every surface pixel's ray from the light;
    FLT_MAX / 0xffffffff for the pixels that are no surface. Independent of the bias."""
    d, _, surf = lights.shadow_model(pos4, origin, light, 0.0)
    mint = np.full(surf.shape, np.finfo(np.float32).max, np.float32)
    idx = np.full(surf.shape, 0xffffffff, np.uint32)
    if surf.any():
        r = oracle_rays(sf.root_transform(np.asarray(light, np.float32)), children, d[surf], lod=LOD[variant])
        mint[surf] = r["minT"]
        idx[surf] = r["index"]
    return mint, idx


def vis_of(pos4, origin, light, bias, mint):
    """The definition's step 5 on the oracle's min_t: 255 where the pixel is no surface or min_t >= bound, else 0."""
    _, bound, surf = lights.shadow_model(pos4, origin, light, bias)
    with np.errstate(invalid="ignore"):
        return np.where(surf & (mint < bound), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def frame_rays(name, light_name, variant="avx"):
    """The oracle's light-side min_t and hit index of fixture `name`'s own oracle frame (computed once, shared)."""
    S = pyoracle.load_setup(name)
    light = INSIDE if light_name == "inside" else LIGHTS[light_name]
    mint, idx = oracle_shadow_rays(S["children"], frame(name, variant)["pos4"], S["origin"], light, variant)
    mint.setflags(write=False)
    idx.setflags(write=False)
    return mint, idx


def oracle_vis(name, light_name, bias, variant="avx"):
    S = pyoracle.load_setup(name)
    light = INSIDE if light_name == "inside" else LIGHTS[light_name]
    return vis_of(frame(name, variant)["pos4"], S["origin"], light, bias, frame_rays(name, light_name, variant)[0])
