"""Oracle helper of the many-sun-directions tests (tests/test_suns_host.py, tests/test_gpu_suns.py).

Bit i of a pixel's mask word is the visibility byte of sf_trace_sun_to for direction i, so the oracle mask is
suncheck's per direction (oracle_sun_rays, vis_of: one oracle ray per traced surface pixel, from the origin, direction
and bound that sphereflake_amd.lights.sun_model states), packed by lights.masks_from_vis. The oracle's min_t does not
depend on the bias and is computed once per (fixture, directions, tau, variant, lod, every)."""
import functools

import numpy as np

from sphereflake_amd import lights
from maskcheck import bit  # noqa: F401
from oracle import pyoracle
from rayscheck import LOD, frame
import suncheck as su

HALF_ANGLE = np.radians(5.0)
# (fixture, the cone's axis, every): t1 all 830 surface pixels, t3 every 3rd of 3600
CONE_CASES = {"t1": ("side", 1), "t3": ("cam", 3)}
SKY_EVERY = 8   # t1 under sky_dirs(64): every 8th surface pixel (104)


def cone(name, n=8):
    """The soft sun of fixture `name`: n directions within 5 degrees of its suncheck direction."""
    return lights.sun_cone(su.VECTORS[CONE_CASES[name][0]], HALF_ANGLE, n)


def rays_for(children, pos4, origin, dirs, tau, lod, every=1):
    """(min_t [n, ...], traced mask [...], deepest node) of the oracle for the directions dirs [n, 3]."""
    D = np.asarray(dirs, np.float32).reshape(-1, 3)
    mints, pick, deepest = [], None, 0
    for s in D:
        mint, pick, deep = su.oracle_sun_rays(children, pos4, origin, s, tau, lod, every)
        mints.append(mint)
        deepest = max(deepest, deep)
    return np.stack(mints), pick, deepest


def mask_of(pos4, origin, dirs, tau, bias, mints, pick):
    """The mask words from the oracle's min_t: bit i is suncheck.vis_of for direction i. A surface pixel that was not
    traced has all its low n bits set and means nothing: compare where `compared(pos4, pick)` holds."""
    D = np.asarray(dirs, np.float32).reshape(-1, 3)
    return lights.masks_from_vis([su.vis_of(pos4, origin, D[i], tau, bias, mints[i], pick) for i in range(len(D))])


def compared(pos4, pick):
    """The pixels a sampled oracle speaks for: the traced ones and every miss of the frame."""
    P = np.asarray(pos4)[..., :3]
    return pick | ((P[..., 0] == 0) & (P[..., 1] == 0) & (P[..., 2] == 0))


@functools.lru_cache(maxsize=None)
def _frame_rays(name, dirs_bytes, tau, variant, lod, every):
    S = pyoracle.load_setup(name)
    D = np.frombuffer(dirs_bytes, np.float32).reshape(-1, 3)
    mints, pick, deepest = rays_for(S["children"], frame(name, variant)["pos4"], S["origin"], D, tau,
                                    LOD[variant] if lod is None else lod, every)
    mints.setflags(write=False)
    pick.setflags(write=False)
    return mints, pick, deepest


def frame_rays(name, dirs, tau=su.TAU, variant="avx", lod=None, every=1):
    """rays_for on fixture `name`'s own oracle frame (computed once, shared). lod None: the variant's own constant."""
    D = np.ascontiguousarray(np.asarray(dirs, np.float32).reshape(-1, 3))
    return _frame_rays(name, D.tobytes(), float(tau), variant, None if lod is None else float(lod), int(every))


def oracle_mask(name, dirs, tau=su.TAU, bias=su.B10, variant="avx", lod=None, every=1):
    """(oracle mask [H, W] uint64, traced mask [H, W]) of fixture `name` for the directions dirs [n, 3]."""
    S = pyoracle.load_setup(name)
    mints, pick, _ = frame_rays(name, dirs, tau, variant, lod, every)
    return mask_of(frame(name, variant)["pos4"], S["origin"], dirs, tau, bias, mints, pick), pick


def mixed(mask, n, where):
    """Pixels of `where` whose low n bits are neither all set nor all clear."""
    low = np.asarray(mask, np.uint64) & np.uint64((1 << n) - 1)
    return where & (low != 0) & (low != np.uint64((1 << n) - 1))
