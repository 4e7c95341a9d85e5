"""Oracle helper of the spun ambient-occlusion tests and of the light-filter tests (tests/test_ao_spin_host.py,
tests/test_gpu_ao_spin.py, tests/test_light_filter_host.py, tests/test_gpu_light_filter.py).

aocheck.py with a spin: the oracle traces one rayscheck.oracle_multi ray per traced surface pixel and sample from the
origin, direction and bound that sphereflake_amd.lights.ao_model states on the host for the spun frame. The oracle's
min_t does not depend on the bias and is computed once per (fixture, samples, table, tau, variant, every)."""
import functools

import numpy as np

import sphereflake_amd as sf
from sphereflake_amd import lights
from maskcheck import assert_mask, assert_shape_of_mask, bit, low, surface_of  # noqa: F401
from oracle import pyoracle
from rayscheck import LOD, frame
import aocheck as ac
from aocheck import B10, CONSTANT_NORMALS, EVERY, FLT_MAX, TAU, compared, counts, mixed  # noqa: F401

F = np.float32
IDENTITY = np.array([[[1.0, 0.0]]], F)   # the 1 x 1 table that turns nothing
PAIR = (0.6, 0.8)                        # the (c, s) of the constant-normal identity: a rotation, exact in binary32
H4 = lights.ao_samples(4)
H8 = lights.ao_samples(8)
THRESHOLDS = ((0.9, 0.02), (0.8, 0.05), (0.95, 0.01))   # the defaults and the two other candidates


def rays_for(children, pos4, nrm4, origin, samples, spin, tau, lod, every=1):
    """aocheck.rays_for with the frame turned by `spin`: (min_t [n, ...], traced mask [...], deepest node)."""
    return ac.rays_for(children, pos4, nrm4, origin, samples, tau, lod, every, spin=spin)


def mask_of(pos4, nrm4, origin, samples, spin, tau, bias, mints, pick):
    """aocheck.mask_of with the spun bounds."""
    return ac.mask_of(pos4, nrm4, origin, samples, tau, bias, mints, pick, spin=spin)


@functools.lru_cache(maxsize=None)
def _frame_rays(name, samples_bytes, spin_bytes, size, tau, variant, every):
    S = pyoracle.load_setup(name)
    h = np.frombuffer(samples_bytes, F).reshape(-1, 3)
    spin = None if spin_bytes is None else np.frombuffer(spin_bytes, F).reshape(size, size, 2)
    f = frame(name, variant)
    mints, pick, deepest = rays_for(S["children"], f["pos4"], f["nrm4"], S["origin"], h, spin, tau, LOD[variant], every)
    mints.setflags(write=False)
    pick.setflags(write=False)
    return mints, pick, deepest


def _table(spin):
    if spin is None:
        return None
    t = np.ascontiguousarray(np.asarray(spin, F))
    assert t.ndim == 3 and t.shape[0] == t.shape[1] and t.shape[2] == 2
    return t


def oracle_mask(name, samples, spin, tau=TAU, bias=B10, variant="avx", every=1):
    """(oracle mask [H, W] uint64, traced mask [H, W]) of fixture `name` for the samples [n, 3] under the table `spin`
    [size, size, 2] (None: unspun). Computed once per argument set and shared."""
    S = pyoracle.load_setup(name)
    f = frame(name, variant)
    h = np.ascontiguousarray(np.asarray(samples, F).reshape(-1, 3))
    t = _table(spin)
    mints, pick, _ = _frame_rays(name, h.tobytes(), None if t is None else t.tobytes(), 0 if t is None else t.shape[0],
                                 float(tau), variant, int(every))
    return mask_of(f["pos4"], f["nrm4"], S["origin"], h, t, tau, bias, mints, pick), pick


def flake(name, variant="avx"):
    """A context at fixture `name`'s size and view."""
    S = pyoracle.load_setup(name)
    s = sf.Sphereflake(S["W"], S["H"])
    s.SetVariant(variant)
    s.SetView(S["origin"], S["tl"], S["tr"], S["bl"])
    return s


def constant_image(shape, N0):
    nrm = np.empty(tuple(shape) + (4,), F)
    nrm[...] = np.array(tuple(N0) + (0.0,), F)
    return nrm


def entry_of(shape, size):
    """The table entry y % size * size + x % size of every pixel of an image [H, W]."""
    return (np.arange(shape[0])[:, None] % size) * size + (np.arange(shape[1])[None, :] % size)


def open_fraction(buf):
    """The open fraction a sum with colours 1 / n leaves: its red channel."""
    return np.asarray(buf, F)[..., 0].astype(np.float64)


def rms(a, b, where):
    d = (open_fraction(a) - open_fraction(b))[where]
    return float(np.sqrt(np.mean(d * d)))


def even_colours(n):
    return np.full((n, 3), F(1.0) / F(n), F)


def accepted_counts(pos4, nrm4, size, normal_min=0.9, plane_max=0.02):
    """The number of accepted taps per surface pixel (0 at a miss) under sf.h's acceptance rule, restated here on its
    own: lights.light_filter_model returns the mean only. tests/test_light_filter_host.py ties the two together (a
    buffer of ones with a single 2 in it moves exactly the pixels whose count this gives)."""
    P = np.asarray(pos4, F)[..., :3]
    N = np.asarray(nrm4, F)[..., :3]
    H, W = P.shape[:2]
    surf = surface_of(P)
    count = np.zeros((H, W), np.int64)
    lo, hi = -(size // 2), size - 1 - size // 2
    k2 = F(plane_max) * F(plane_max)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        pp = (P[..., 0] * P[..., 0] + P[..., 1] * P[..., 1]) + P[..., 2] * P[..., 2]
        limit = k2 * pp
        for dy in range(lo, hi + 1):
            for dx in range(lo, hi + 1):
                ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
                yq, xq = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
                if dx == 0 and dy == 0:
                    ok = np.ones((H, W), bool)[ys, xs]
                else:
                    Np, Nq = N[ys, xs], N[yq, xq]
                    nn = (Np[..., 0] * Nq[..., 0] + Np[..., 1] * Nq[..., 1]) + Np[..., 2] * Nq[..., 2]
                    D = P[yq, xq] - P[ys, xs]
                    e = (Np[..., 0] * D[..., 0] + Np[..., 1] * D[..., 1]) + Np[..., 2] * D[..., 2]
                    ok = surf[yq, xq] & (nn >= F(normal_min)) & ((e * e) <= limit[ys, xs])
                count[ys, xs] += ok
    return np.where(surf, count, 0)
