"""Oracle helper of the ambient-occlusion tests (tests/test_ao_host.py, tests/test_gpu_ao.py).

Bit i of a pixel's mask word says whether the ray of sample i, turned about the pixel's own normal, reaches the pixel.
That ray is sf_trace_rays_to's ray from its own origin F, so the oracle traces one rayscheck.oracle_multi ray per traced
surface pixel and sample, from the origin, direction and bound that sphereflake_amd.lights.ao_model states on the host,
as sunscheck.py does per sun direction. The oracle's min_t does not depend on the bias and is computed once per
(fixture, samples, tau, variant, lod, every). The frames -- positions and normals -- are the oracle's own."""
import functools

import numpy as np

from sphereflake_amd import lights
from maskcheck import bit  # noqa: F401
from oracle import pyoracle
from rayscheck import LOD, frame, oracle_multi
import suncheck as su

FLT_MAX = su.FLT_MAX
TAU = su.TAU
B10 = su.B10
EVERY = {"t1": 1, "t3": 3}   # t1 all 830 surface pixels, t3 every 3rd of 3600
SKY_EVERY = 8                # t1 under ao_samples(64): every 8th surface pixel (104)
# the constant normals of the identity test: both poles of the frame's sign, an axis in the plane, a general one
CONSTANT_NORMALS = ((0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (0.6, -0.64, 0.48))


def rays_for(children, pos4, nrm4, origin, samples, tau, lod, every=1, spin=None):
    """(min_t [n, ...], traced mask [...], deepest node) of the oracle: the closest hit of the ray of every sample at
    every `every`-th surface pixel in row-major order (FLT_MAX elsewhere). spin: the frames turned by the table
    (tests/aospincheck.py); None is the unspun call itself."""
    Fo, d, _, surf = lights.ao_model(pos4, nrm4, origin, samples, tau, 0.0, spin=spin)
    n = Fo.shape[0]
    pick = np.zeros(surf.shape, bool).reshape(-1)
    pick[np.nonzero(surf.reshape(-1))[0][::every]] = True
    pick = pick.reshape(surf.shape)
    mints = np.full((n,) + surf.shape, FLT_MAX, np.float32)
    deepest = 0
    if pick.any():
        r = oracle_multi(children, Fo[:, pick].reshape(-1, 3), d[:, pick].reshape(-1, 3), 1, lod=lod)
        mints[:, pick] = r["minT"].reshape(n, -1)
        deepest = r["stats"]["max_depth"]
    return mints, pick, deepest


def mask_of(pos4, nrm4, origin, samples, tau, bias, mints, pick, spin=None):
    """The mask words from the oracle's min_t: bit i is 0 where a traced surface pixel has min_t < bound_i, else 1;
    bits n..63 are 0. A surface pixel that was not traced has all its low n bits set and means nothing: compare where
    `compared(pos4, pick)` holds. spin: as rays_for's."""
    _, _, bound, surf = lights.ao_model(pos4, nrm4, origin, samples, tau, bias, spin=spin)
    mask = np.zeros(surf.shape, np.uint64)
    with np.errstate(invalid="ignore"):
        for i in range(bound.shape[0]):
            lit = ~(surf & pick & (mints[i] < bound[i]))
            mask |= lit.astype(np.uint64) << np.uint64(i)
    return mask


def compared(pos4, pick):
    """The pixels a sampled oracle speaks for: the traced ones and every miss of the frame."""
    P = np.asarray(pos4)[..., :3]
    return pick | ((P[..., 0] == 0) & (P[..., 1] == 0) & (P[..., 2] == 0))


@functools.lru_cache(maxsize=None)
def _frame_rays(name, samples_bytes, tau, variant, lod, every):
    S = pyoracle.load_setup(name)
    h = np.frombuffer(samples_bytes, np.float32).reshape(-1, 3)
    f = frame(name, variant)
    mints, pick, deepest = rays_for(S["children"], f["pos4"], f["nrm4"], S["origin"], h, tau,
                                    LOD[variant] if lod is None else lod, every)
    mints.setflags(write=False)
    pick.setflags(write=False)
    return mints, pick, deepest


def frame_rays(name, samples, tau=TAU, variant="avx", lod=None, every=1):
    """rays_for on fixture `name`'s own oracle frame (computed once, shared). lod None: the variant's own constant."""
    h = np.ascontiguousarray(np.asarray(samples, np.float32).reshape(-1, 3))
    return _frame_rays(name, h.tobytes(), float(tau), variant, None if lod is None else float(lod), int(every))


def oracle_mask(name, samples, tau=TAU, bias=B10, variant="avx", lod=None, every=1):
    """(oracle mask [H, W] uint64, traced mask [H, W]) of fixture `name` for the samples [n, 3]."""
    S = pyoracle.load_setup(name)
    f = frame(name, variant)
    mints, pick, _ = frame_rays(name, samples, tau, variant, lod, every)
    return mask_of(f["pos4"], f["nrm4"], S["origin"], samples, tau, bias, mints, pick), pick


def counts(mask, n, where):
    """Per sample i < n: (lit, occluded) pixels of `where`."""
    return [(int((where & bit(mask, i)).sum()), int((where & ~bit(mask, i)).sum())) for i in range(n)]


def mixed(mask, n, where):
    """Pixels of `where` whose low n bits are neither all set nor all clear."""
    full = np.uint64((1 << n) - 1)
    low = np.asarray(mask, np.uint64) & full
    return where & (low != 0) & (low != full)
