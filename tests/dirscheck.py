"""Oracle helpers shared by the direction-tracing tests (tests/test_dirs_host.py, tests/test_gpu_dirs.py).

The reference's per-ray result is a function of the normalised direction, the root transform, the child frames and
the LOD constant only (oracle/sf_oracle.c), so the oracle traces an arbitrary direction d as a 1 x 1 frame with
origin 0 and top-left = top-right = bottom-left = d: its ray generation then forms D = Normalize(d) -- except that
a -0 component of d comes out as +0, so test directions avoid exact zeros unless a miss is expected."""
import functools

import numpy as np

from oracle import pyoracle

FLT_MAX = np.float32(np.finfo(np.float32).max)
ZERO3 = np.zeros(3, np.float32)


@functools.lru_cache(maxsize=None)
def _lut():
    return pyoracle.load_lut()


def oracle_rays(root, children, dirs, lod=70.0):
    """One oracle call per direction of dirs [..., 3]: dict of pos4 [..., 4], nrm4 [..., 4], minT [...],
    index [...] and stats (max_depth, closest, hits) over them."""
    d = np.ascontiguousarray(dirs, np.float32)
    lead = d.shape[:-1]
    flat = d.reshape(-1, 3)
    n = flat.shape[0]
    pos, nrm = np.empty((n, 4), np.float32), np.empty((n, 4), np.float32)
    mint, idx = np.empty(n, np.float32), np.empty(n, np.uint32)
    maxd, closest = 0, float(FLT_MAX)
    for i in range(n):
        v = flat[i].copy()
        r = pyoracle.render({"W": 1, "H": 1, "origin": ZERO3, "tl": v, "tr": v, "bl": v, "root": root,
                             "children": children}, threads=1, lut=_lut(), lod=lod)
        pos[i], nrm[i], mint[i], idx[i] = r["pos4"][0, 0], r["nrm4"][0, 0], r["minT"][0, 0], r["index"][0, 0]
        maxd = max(maxd, r["stats"]["max_depth"])
        closest = min(closest, r["stats"]["closest"])
    return {"pos4": pos.reshape(lead + (4,)), "nrm4": nrm.reshape(lead + (4,)), "minT": mint.reshape(lead),
            "index": idx.reshape(lead),
            "stats": {"max_depth": maxd, "closest": closest, "hits": int((mint < FLT_MAX).sum())}}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and \
        np.array_equal(a.view(np.uint8), b.view(np.uint8))
