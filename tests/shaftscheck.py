"""Oracle helper of the light-shaft tests (tests/test_shafts_host.py, tests/test_gpu_shafts.py).

Bit i of a pixel's mask word is the visibility byte of sf_trace_sun_to at a pixel whose position is the sample
Q_i = E sigma_i, so the oracle mask is suncheck's (oracle_sun_rays, vis_of: one oracle ray per traced pixel, from the
origin, direction and bound that sphereflake_amd.lights.sun_model states) applied to the images Q_i that
lights.shaft_ends and lights.shaft_samples state, packed by lights.masks_from_vis. "Every k-th surface pixel" and
"every k-th miss pixel" are oracle_sun_rays' row-major pick on Q_i restricted to the frame's surface pixels, and on Q_i
restricted to the frame's misses (the rest zeroed: no ray). The oracle's min_t does not depend on the bias and is
computed once per case."""
import functools

import numpy as np

from sphereflake_amd import lights
from maskcheck import bit, low, surface_of  # noqa: F401
from oracle import pyoracle
from rayscheck import LOD, frame, pinhole
import suncheck as su

# fixture -> the sun (towards it, normalised by lights.sun_direction), tau, far (0: no direction image)
CASES = {"t1": ((4.0, 7.0, 2.0), 16.0, 13.0), "t3": ((0.0, 0.0, 1.0), 4.0, 0.0)}
# fixture -> ((part, every, traced pixels), ...) of the 8-sample oracle comparison
PARITY = {"t1": (("surface", 4, 208), ("miss", 8, 185)), "t3": (("surface", 12, 300),)}
# the bits that have at least `count` traced pixels of either outcome under the avx variant (n = 8)
BOTH = {("t1", "surface"): (range(3, 8), 34), ("t1", "miss"): (range(2, 6), 22), ("t3", "surface"): (range(2, 8), 42)}
ALL64_EVERY = 8   # t1, n = 64: every 8th surface pixel (104); bits 32..55 have at least 20 of either outcome


def sun(name):
    return lights.sun_direction(CASES[name][0])


@functools.lru_cache(maxsize=None)
def unit_dirs(name):
    """The fixture's pinhole directions divided by their float32 length, [H, W, 3]."""
    d = np.asarray(pinhole(name), np.float32)
    u = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(np.float32)
    u.setflags(write=False)
    return u


def dirs_of(name):
    """The direction image of the fixture's case, or None where its misses are not marched."""
    return unit_dirs(name) if CASES[name][2] > 0 else None


def samples(name, fractions, variant="avx"):
    """Q [n, H, W, 3] of the fixture's own oracle frame under its case."""
    E = lights.shaft_ends(frame(name, variant)["pos4"], dirs_of(name), CASES[name][2])
    return lights.shaft_samples(E, fractions)


def part_of(name, part, variant="avx"):
    surf = surface_of(frame(name, variant)["pos4"])
    return surf if part == "surface" else ~surf


def rays_for(children, Q, origin, s, tau, lod, every, where):
    """(min_t [n, ...], traced mask [...]) of the oracle for the sample images Q [n, ..., 3] restricted to `where`:
    every `every`-th pixel of `where` in row-major order, the same pixels for every sample."""
    mints, pick = [], None
    for Qi in Q:
        mint, pk, _ = su.oracle_sun_rays(children, np.where(where[..., None], Qi, np.float32(0.0)), origin, s, tau, lod,
                                         every)
        assert pick is None or np.array_equal(pk, pick), "a sample underflowed to 0: the picks differ"
        mints.append(mint)
        pick = pk
    return np.stack(mints), pick


def mask_of(Q, origin, s, tau, bias, mints, pick):
    """The mask words from the oracle's min_t: bit i is suncheck.vis_of on Q_i. A pixel that was not traced has all its
    low n bits set and means nothing: compare where `pick` holds."""
    return lights.masks_from_vis([su.vis_of(Q[i], origin, s, tau, bias, mints[i], pick) for i in range(len(Q))])


@functools.lru_cache(maxsize=None)
def _frame_rays(name, frac_bytes, variant, every, part):
    S = pyoracle.load_setup(name)
    Q = samples(name, np.frombuffer(frac_bytes, np.float32), variant)
    mints, pick = rays_for(S["children"], Q, S["origin"], sun(name), CASES[name][1], LOD[variant], every,
                           part_of(name, part, variant))
    mints.setflags(write=False)
    pick.setflags(write=False)
    return mints, pick


def oracle_mask(name, fractions, bias, variant="avx", every=1, part="surface"):
    """(oracle mask [H, W] uint64, traced mask [H, W]) of fixture `name` under its case."""
    S = pyoracle.load_setup(name)
    F = np.ascontiguousarray(np.asarray(fractions, np.float32).reshape(-1))
    mints, pick = _frame_rays(name, F.tobytes(), variant, int(every), part)
    return mask_of(samples(name, F, variant), S["origin"], sun(name), CASES[name][1], bias, mints, pick), pick


def outcomes(mask, pick, i):
    """(shadowed, lit) counts of bit i among the traced pixels."""
    return int((pick & ~bit(mask, i)).sum()), int((pick & bit(mask, i)).sum())
