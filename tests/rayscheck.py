"""Oracle helper and shared ray sets of the ray-tracing tests (tests/test_rays_host.py, tests/test_gpu_rays.py).

"Ray i from origins[i]" means what the reference returns for that direction after SetView at that origin: the
origin enters only through the root transform's translation column (Sphereflake.cpp:83), so the oracle traces it
with root = sf.root_transform(origin) -- one dirscheck.oracle_rays call per distinct origin."""
import functools

import numpy as np

import sphereflake_amd as sf
from sphereflake_amd import dirs, rays
from dirscheck import FLT_MAX, oracle_rays
from oracle import pyoracle

CHANNELS = ("pos4", "nrm4", "minT", "index")
LOD = {"avx": 70.0, "sse": 60.0}


def oracle_multi(children, origins, d, rays_per_origin=1, lod=70.0):
    """origins [M, 3], d [N, 3], ray i from origins[i // rays_per_origin]: dict of pos4 [N, 4], nrm4 [N, 4],
    minT [N], index [N] and stats (max_depth, closest, hits)."""
    d = np.ascontiguousarray(d, np.float32).reshape(-1, 3)
    o = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    n = d.shape[0]
    per_ray = o[np.arange(n) // max(int(rays_per_origin), 1)]
    out = {"pos4": np.empty((n, 4), np.float32), "nrm4": np.empty((n, 4), np.float32),
           "minT": np.empty(n, np.float32), "index": np.empty(n, np.uint32)}
    maxd, closest = 0, float(FLT_MAX)
    # distinct origins by bit pattern (NaN and -0 included)
    _, first, inverse = np.unique(per_ray.view(np.uint32), axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    for k, f in enumerate(first):
        sel = np.nonzero(inverse == k)[0]
        r = oracle_rays(sf.root_transform(per_ray[f]), children, d[sel], lod=lod)
        for c in CHANNELS:
            out[c][sel] = r[c]
        maxd = max(maxd, r["stats"]["max_depth"])
        closest = min(closest, r["stats"]["closest"])
    out["stats"] = {"max_depth": maxd, "closest": closest, "hits": int((out["minT"] < FLT_MAX).sum())}
    return out


@functools.lru_cache(maxsize=None)
def pinhole(name):
    S = pyoracle.load_setup(name)
    return dirs.pinhole(S["origin"], S["tl"], S["tr"], S["bl"], S["W"], S["H"])


@functools.lru_cache(maxsize=None)
def frame(name, variant="avx"):
    return pyoracle.render(pyoracle.load_setup(name), lod=LOD[variant])


# ---- the seeded ray sets: (origins [N, 3], dirs [N, 3]), one origin per ray ---------------------------
@functools.lru_cache(maxsize=None)
def jitter():
    """t1's pixel directions (64 x 36), each from t1's origin plus a seeded offset within a ball of radius 0.5."""
    S = pyoracle.load_setup("t1")
    d = pinhole("t1").reshape(-1, 3)
    rng = np.random.default_rng(101)
    v = rng.normal(size=(d.shape[0], 3))
    v *= (0.5 * rng.random(d.shape[0]) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1)).reshape(-1, 1)
    o = np.asarray(S["origin"], np.float32).reshape(1, 3) + v.astype(np.float32)
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


@functools.lru_cache(maxsize=None)
def _t3_hits():
    """1024 seeded hit pixels of t3's oracle frame: (pos4, nrm4, dirs) of them."""
    S = pyoracle.load_setup("t3")
    f = frame("t3")
    hit = np.nonzero((f["minT"] < FLT_MAX).reshape(-1))[0]
    assert hit.size >= 1024
    pix = np.sort(np.random.default_rng(103).choice(hit, size=1024, replace=False))
    W = S["W"]
    y, x = pix // W, pix % W
    return f["pos4"][y, x], f["nrm4"][y, x], pinhole("t3")[y, x], np.asarray(S["origin"], np.float32)


@functools.lru_cache(maxsize=None)
def reflect():
    pos, nrm, d, o = _t3_hits()
    ro, rd, mask = rays.reflect(pos, nrm, o, d, 1e-3)
    assert mask.all()
    return ro, rd


@functools.lru_cache(maxsize=None)
def towards_in():
    pos, nrm, _, o = _t3_hits()
    ro, rd, mask = rays.towards(pos, nrm, o, (0.0, 0.0, 3.0), 1e-3)
    assert mask.all()
    return ro, rd


@functools.lru_cache(maxsize=None)
def towards_out():
    pos, nrm, _, o = _t3_hits()
    ro, rd, _ = rays.towards(pos[:64], nrm[:64], o, (0.5, -3.0, 0.3), 1e-3)
    return ro, rd


SETS = {"jitter": (jitter, "t1"), "reflect": (reflect, "t3"), "towards_in": (towards_in, "t3"),
        "towards_out": (towards_out, "t3")}


@functools.lru_cache(maxsize=None)
def set_oracle(name):
    gen, setup = SETS[name]
    o, d = gen()
    return oracle_multi(pyoracle.load_setup(setup)["children"], o, d)
