"""Shared helper of the light-accumulation tests (tests/test_light_accumulate_host.py,
tests/test_gpu_light_accumulate.py): views moved off a fixture's, their oracle frames, and the spun n = 4 sums of a
camera path on the oracle.

"Moved by delta" is the fixture's origin and three corners, each + delta in binary32, with the root translation
-origin (sf.root_transform). right = normalize(tr - tl) and fwd = normalize(tl + (tr - tl) / 2 + (bl - tl) / 2 - origin)
are formed in float64 from the fixture's float32 values; delta is their multiple rounded to float32."""
import functools

import numpy as np

import sphereflake_amd as sf
from sphereflake_amd import lights
from oracle import pyoracle
from rayscheck import LOD, frame
import aospincheck as sc

F = np.float32
# (fixture, direction, distance): the current frame is the moved view, the history the fixture's own
PAIRS = (("t1", "right", 0.01), ("t1", "fwd", 0.03), ("t3", "right", 0.01), ("t3", "fwd", 0.03), ("t3", "right", 0.03))
PATH_FRAMES = 16
PATH_STEP = 0.0005          # per frame, along 0.8 fwd + 0.6 right
H4 = sc.H4
H64 = lights.ao_samples(64)


def view_of(S):
    """(origin, tl, tr, bl) float32 of a setup."""
    return tuple(np.asarray(S[k], F) for k in ("origin", "tl", "tr", "bl"))


def axes(S):
    """(right, fwd) float64 unit vectors of a setup's view."""
    o, tl, tr, bl = (np.asarray(v, np.float64) for v in view_of(S))
    right = tr - tl
    fwd = tl + (tr - tl) / 2 + (bl - tl) / 2 - o
    return right / np.linalg.norm(right), fwd / np.linalg.norm(fwd)


def moved_setup(name, delta):
    """Fixture `name`'s setup moved by delta [3]: origin and corners + float32(delta), root = root_transform(origin)."""
    S = dict(pyoracle.load_setup(name))
    d = np.asarray(delta, F).reshape(3)
    for k in ("origin", "tl", "tr", "bl"):
        S[k] = (np.asarray(S[k], F) + d).astype(F)
    S["root"] = sf.root_transform(S["origin"])
    return S


def delta_of(name, direction, distance):
    right, fwd = axes(pyoracle.load_setup(name))
    along = {"right": right, "fwd": fwd, "path": 0.8 * fwd + 0.6 * right}[direction]
    return (float(distance) * along).astype(F)


@functools.lru_cache(maxsize=None)
def moved_frame(name, direction, distance, variant="avx"):
    """(setup, the oracle's frame) of fixture `name` moved `distance` along `direction`; read-only, computed once."""
    S = moved_setup(name, delta_of(name, direction, distance))
    f = pyoracle.render(S, lod=LOD[variant])
    for a in f.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return S, f


def path_view(k):
    """(direction, distance) of view k of the 16-view path that ends at t3: t3 moved by (k - 15) 0.0005 along
    0.8 fwd + 0.6 right."""
    return "path", (k - (PATH_FRAMES - 1)) * PATH_STEP


def oracle_sum(S, f, samples, spin):
    """What trace_ao_sum(samples, spin=spin) leaves on a zero base for the oracle's frame f of setup S (colours 1 / n,
    tau 4, bias 2^-10): aospincheck.rays_for's rays -- origin, direction and bound as lights.ao_model states them -- in
    one pyoracle.trace_rays batch."""
    n = len(samples)
    Fo, d, _, surf = lights.ao_model(f["pos4"], f["nrm4"], S["origin"], samples, sc.TAU, 0.0, spin=spin)
    mints = np.full((n,) + surf.shape, sc.FLT_MAX, F)
    if surf.any():
        r = pyoracle.trace_rays(S["children"], Fo[:, surf].reshape(-1, 3), d[:, surf].reshape(-1, 3), lod=LOD["avx"])
        mints[:, surf] = r["minT"].reshape(n, -1)
    mask = sc.mask_of(f["pos4"], f["nrm4"], S["origin"], samples, spin, sc.TAU, sc.B10, mints, surf)
    return lights.ao_sum_model(None, f["pos4"], mask, sc.even_colours(n))


@functools.lru_cache(maxsize=None)
def spun_sum(name, direction, distance, k):
    """The oracle's n = 4 sum (colours 1 / n, tau 4, bias 2^-10) of that moved view under ao_spins(4, ao_phase(k)):
    what trace_ao_sum(H4, spin=...) leaves on a zero base. Read-only, computed once."""
    S, f = moved_frame(name, direction, distance)
    out = oracle_sum(S, f, H4, lights.ao_spins(4, lights.ao_phase(k)))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def truth64(name):
    """The oracle's unspun n = 64 sum of fixture `name`'s own view."""
    out = oracle_sum(pyoracle.load_setup(name), frame(name), H64, None)
    out.setflags(write=False)
    return out


def accumulate_path(views, max_history=16):
    """lights.light_accumulate_model chained over `views` [(direction, distance), ...] of t3 with frame k's spun sum:
    (the last buffer, the accepted mask of the last step)."""
    hist = acc = None
    for k, (direction, distance) in enumerate(views):
        S, f = moved_frame("t3", direction, distance)
        new = spun_sum("t3", direction, distance, k)
        if hist is None:
            zero = np.zeros_like(new)
            cur, acc, _ = lights.light_accumulate_model(new, f["pos4"], f["nrm4"], S["origin"], zero, zero, zero,
                                                        view_of(S), max_history)
        else:
            hS, hf, hbuf = hist
            cur, acc, _ = lights.light_accumulate_model(new, f["pos4"], f["nrm4"], S["origin"], hbuf, hf["pos4"],
                                                        hf["nrm4"], view_of(hS), max_history)
        hist = (S, f, cur)
    return hist[2], acc


def seeded_history(shape, seed):
    """A history light buffer [H, W, 4]: seeded values, .w drawn from {0, 1, 3, 16, 70000, NaN}."""
    rng = np.random.default_rng(seed)
    buf = rng.uniform(0.0, 1.0, tuple(shape) + (4,)).astype(F)
    buf[..., 3] = rng.choice(np.array([0.0, 1.0, 3.0, 16.0, 70000.0, np.nan], F), size=tuple(shape))
    return buf
