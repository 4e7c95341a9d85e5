#!/usr/bin/env python3
"""Search the seeded random views of tests/test_gpu_depth_seed.py (seeded_view) for views whose deepest node is
occluded: views where the occlusion cull WITHOUT its depth condition (occl_sim.c mode + 128) reports a smaller max
depth than the reference. A cull that ignores the statistic fails on such a view; the depth seed must not. CPU only.
Usage: depth_seed_view_search.py [views=200]"""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "sphereflake-raytracer_amd"))
from oracle import pyoracle  # noqa: E402
from test_gpu_depth_seed import seeded_view  # noqa: E402

so = os.path.join(tempfile.mkdtemp(), "occl_sim.so")
subprocess.check_call(["gcc", "-O2", "-mno-fma", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                       os.path.join(HERE, "occl_sim.c"), "-lm"])
L = ctypes.CDLL(so)
fp = ctypes.POINTER(ctypes.c_float)
up = ctypes.POINTER(ctypes.c_uint32)
L.sim_rows.argtypes = [ctypes.c_uint32, ctypes.c_uint32, fp, fp, fp, fp, fp, fp, up, ctypes.c_uint32,
                       ctypes.c_uint32, ctypes.c_float, ctypes.c_int, fp, up, ctypes.POINTER(ctypes.c_longlong)]
lut = np.ascontiguousarray(pyoracle.load_lut(), np.uint32)
n = int(sys.argv[1]) if len(sys.argv) > 1 else 200
found = []
for seed in range(n):
    view, setup, K = seeded_view(seed)
    W, H = setup["W"], setup["H"]
    ref = pyoracle.render(setup, threads=8)
    a = {k: np.ascontiguousarray(np.asarray(setup[k], np.float32).reshape(-1)) for k in
         ("origin", "tl", "tr", "bl", "root", "children")}
    mint = np.empty((H, W), np.float32)
    idx = np.empty((H, W), np.uint32)
    st = np.zeros(4, np.int64)
    # index order, lb = tca - rho, margin 3 * 2^-10, no depth condition
    L.sim_rows(W, H, *(a[k].ctypes.data_as(fp) for k in ("origin", "tl", "tr", "bl", "root", "children")),
               lut.ctypes.data_as(up), 0, H, ctypes.c_float(3 * 2.0 ** -10), 1 | 128, mint.ctypes.data_as(fp),
               idx.ctypes.data_as(up), st.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)))
    same = np.array_equal(mint.view(np.uint32), ref["minT"].view(np.uint32)) and np.array_equal(idx, ref["index"])
    if not same:
        print(f"seed {seed}: the model's pixels differ from the oracle's", flush=True)
    if st[0] < ref["stats"]["max_depth"]:
        found.append(seed)
        print(f"seed {seed} K={K:.4f}: max depth {ref['stats']['max_depth']}, {st[0]} without the depth condition", flush=True)
print(f"{len(found)} of {n} views: {found}")
