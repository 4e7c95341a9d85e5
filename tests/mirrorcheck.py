"""Oracle helper of the sky-reflection tests (tests/test_mirror_host.py, tests/test_gpu_mirror.py).

aospincheck.py about another axis: the oracle traces one rayscheck.oracle_multi ray per surface pixel and sample from
the origin, direction and bound that sphereflake_amd.lights.mirror_model states on the host -- ao_model on the image of
mirror axes. The oracle's min_t does not depend on the bias and is computed once per argument set; every surface pixel
is traced (830 on t1, 3600 on t3)."""
import functools

import numpy as np

from sphereflake_amd import lights
from oracle import pyoracle
from rayscheck import LOD, frame
import aospincheck as sc
from aospincheck import B10, TAU, bit, surface_of  # noqa: F401

F = np.float32
ZENITH = (0.25, 0.45, 1.0)
HORIZON = (1.0, 0.8, 0.6)
UP = (0.0, 0.0, 1.0)
EYE_SHIFT = (0.3, -0.2, 0.1)      # the displaced eye: the origin plus this
S4 = lights.ao_spins(4)
MIRROR = np.array([[0.0, 0.0, 1.0]], F)   # n = 1: the mirror ray alone
LOBE8 = lights.lobe_samples(8, 8)
LOBE64 = lights.lobe_samples(64, 8)


def eye_of(name):
    """The displaced eye of fixture `name`."""
    o = np.asarray(pyoracle.load_setup(name)["origin"], F).reshape(3)
    return o + np.array(EYE_SHIFT, F)


def axes(name, variant="avx", eye=None):
    """lights.mirror_axes of the fixture's own oracle frame."""
    S = pyoracle.load_setup(name)
    f = frame(name, variant)
    return lights.mirror_axes(f["pos4"], f["nrm4"], S["origin"], eye)


@functools.lru_cache(maxsize=None)
def _rays(name, samples_bytes, spin_bytes, size, eye_bytes, tau, variant):
    S = pyoracle.load_setup(name)
    h = np.frombuffer(samples_bytes, F).reshape(-1, 3)
    spin = None if spin_bytes is None else np.frombuffer(spin_bytes, F).reshape(size, size, 2)
    eye = None if eye_bytes is None else np.frombuffer(eye_bytes, F)
    f = frame(name, variant)
    Fo, d, _, pick = lights.ao_model(f["pos4"], axes(name, variant, eye), S["origin"], h, tau, 0.0, spin=spin)
    n = Fo.shape[0]
    # (the oracle's batch entry: rayscheck.oracle_multi's answers, without its Python loop over the origins)
    r = pyoracle.trace_rays(S["children"], Fo[:, pick].reshape(-1, 3), d[:, pick].reshape(-1, 3), LOD[variant])
    mints = np.full((n,) + pick.shape, sc.FLT_MAX, F)
    mints[:, pick] = r["minT"].reshape(n, -1)
    deepest = r["stats"]["max_depth"]
    mints.setflags(write=False)
    pick.setflags(write=False)
    return mints, pick, deepest


def _key(samples, spin, eye):
    h = np.ascontiguousarray(np.asarray(samples, F).reshape(-1, 3))
    t = None if spin is None else np.ascontiguousarray(np.asarray(spin, F))
    e = None if eye is None else np.ascontiguousarray(np.asarray(eye, F).reshape(3))
    return h, t, e


def oracle_mask(name, samples, spin=None, eye=None, tau=TAU, bias=B10, variant="avx"):
    """(oracle mask [H, W] uint64, deepest node) of trace_mirror on fixture `name`'s own oracle frame: every surface
    pixel traced, every miss of the frame all ones. Computed once per argument set and shared."""
    S = pyoracle.load_setup(name)
    f = frame(name, variant)
    h, t, e = _key(samples, spin, eye)
    mints, pick, deepest = _rays(name, h.tobytes(), None if t is None else t.tobytes(), 0 if t is None else t.shape[0],
                                 None if e is None else e.tobytes(), float(tau), variant)
    assert np.array_equal(pick, surface_of(f["pos4"]))
    return sc.mask_of(f["pos4"], axes(name, variant, e), S["origin"], h, t, tau, bias, mints, pick), deepest


def red_rms(a, b, where):
    d = (np.asarray(a, F)[..., 0].astype(np.float64) - np.asarray(b, F)[..., 0].astype(np.float64))[where]
    return float(np.sqrt(np.mean(d * d)))
