#!/usr/bin/env python3
"""Cost of point-light shadows (sf_trace_shadow_to, sf_light_image), one process, one GPU, at 1920 x 1080, K = 0.25,
light (-1.5, -2.5, 2.0), the default bias:
  a  trace_shadow on the context's own frame into the context's visibility buffer (1 B per pixel out)
  b  what it replaces on the device: trace_rays of the same d from the one origin `light`, writing all four outputs
     (the comparison min_t < bound is not even counted)
  c  a with the early exit and the bound seed compiled out: a library built with -DSF_SHADOW_CLOSEST
     (make -C sphereflake-raytracer_amd SHADOW_CLOSEST=1 -> build_shadow_closest/), loaded beside the
     product library; skipped when that build is missing. Same bits as a, checked.
  d  light_image on the post-processed image
  r  Render() of the frame itself, for scale
each lone (synchronised each time) and queued back to back. After a 300 ms settle under load the cases run
interleaved, REPS rounds; medians, the spread between rounds, ratios, the live shader clock and the build are printed,
the last line as JSON.
Usage: shadow_probe.py [N=50] [REPS=5]"""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sphereflake-raytracer_amd"))
import sphereflake_amd as sf  # noqa: E402
from sphereflake_amd import lights  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 50
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
W, H, K = 1920, 1080, 0.25
LIGHT = (-1.5, -2.5, 2.0)
CLOSEST_LIB = os.path.join(sf.ROOT_DIR, "build_shadow_closest", "libsphereflake_hip.so")

cam = sf.config_camera(W, H, K)
o, tl, tr, bl = cam.corners()
s = sf.Sphereflake(W, H)
s.SetCamera(cam)
s.Render()
pos_h, nrm_h, _, _ = s.download()
p = s.shadow_params(LIGHT)
bias = float(p.bias)
s.trace_shadow(LIGHT)
vis_a = s.download_shadow()

# b: the same rays through trace_rays
d_h, bound_h, surf_h = lights.shadow_model(pos_h, o, LIGHT, bias)
d_t = torch.from_numpy(np.ascontiguousarray(d_h)).cuda()
org = torch.from_numpy(np.asarray(LIGHT, np.float32).reshape(1, 3)).cuda()
out_b = (torch.empty((H, W, 4), dtype=torch.float32, device="cuda"), torch.empty((H, W, 4), dtype=torch.float32, device="cuda"),
         torch.empty((H, W), dtype=torch.float32, device="cuda"), torch.empty((H, W), dtype=torch.int32, device="cuda"))
torch.cuda.synchronize()
s.trace_rays(org, d_t, rays_per_origin=W * H, out=out_b)
s.Synchronize()
vis_b = np.where(surf_h & (out_b[2].cpu().numpy() < bound_h), 0, 255).astype(np.uint8)
same_b = bool(np.array_equal(vis_a, vis_b))
assert same_b, "trace_shadow differs from trace_rays + comparison"


class Closest:
    """The -DSF_SHADOW_CLOSEST build through its C ABI: a context of its own with the same view and frame."""

    def __init__(self, path):
        L = self.L = ctypes.CDLL(path)
        V = ctypes.c_void_p
        F = ctypes.POINTER(ctypes.c_float)
        L.sf_create.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(V)]
        L.sf_set_view.argtypes = [V, F, F, F, F]
        L.sf_render.argtypes = [V, V]
        L.sf_trace_shadow.argtypes = [V, ctypes.POINTER(sf.sf_shadow_params)]
        L.sf_download_shadow.argtypes = [V, V]
        L.sf_synchronize.argtypes = [V]
        L.sf_destroy.argtypes = [V]
        L.sf_destroy.restype = None
        self.ctx = V()
        assert L.sf_create(0, W, H, ctypes.byref(self.ctx)) == 0
        v = [np.ascontiguousarray(x, np.float32) for x in (o, tl, tr, bl)]
        assert L.sf_set_view(self.ctx, *[x.ctypes.data_as(F) for x in v]) == 0
        assert L.sf_render(self.ctx, None) == 0
        self.p = s.shadow_params(LIGHT)

    def trace(self):
        assert self.L.sf_trace_shadow(self.ctx, ctypes.byref(self.p)) == 0

    def Synchronize(self):
        assert self.L.sf_synchronize(self.ctx) == 0

    def download(self):
        v = np.empty((H, W), np.uint8)
        assert self.L.sf_download_shadow(self.ctx, v.ctypes.data_as(ctypes.c_void_p)) == 0
        return v

    def close(self):
        self.L.sf_destroy(self.ctx)


sc = Closest(CLOSEST_LIB) if os.path.exists(CLOSEST_LIB) else None
same_c = None
if sc:
    sc.trace()
    same_c = bool(np.array_equal(sc.download(), vis_a))
    assert same_c, "the closest-hit build's visibility differs"
s.PostProcess()
s.Synchronize()


def lone(call, ctx):
    ts = []
    for _ in range(N):
        t = time.perf_counter()
        call()
        ctx.Synchronize()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e3


def queued(call, ctx):
    call()
    ctx.Synchronize()
    t = time.perf_counter()
    for _ in range(N):
        call()
    ctx.Synchronize()
    return (time.perf_counter() - t) / N * 1e3


calls = {
    "a shadow": (lambda: s.trace_shadow(LIGHT), s),
    "b rays one origin": (lambda: s.trace_rays(org, d_t, rays_per_origin=W * H, out=out_b), s),
    "d light_image": (lambda: s.light_image(LIGHT), s),
    "r render": (lambda: s.Render(), s),
}
if sc:
    calls["c shadow closest-hit build"] = (sc.trace, sc)
cases = {}
for name, (call, ctx) in calls.items():
    cases[name + " lone"] = (lambda call=call, ctx=ctx: lone(call, ctx))
    cases[name + " queued"] = (lambda call=call, ctx=ctx: queued(call, ctx))
t0 = time.perf_counter()
while time.perf_counter() - t0 < 0.3:   # clock settle under load
    queued(lambda: s.Render(), s)
s.kernel_timing(True, period=8)
res = {k: [] for k in cases}
for _ in range(REPS):
    for k, f in cases.items():
        res[k].append(f())
    s.Render()   # (the live clock samples come from timed renders)
    s.Synchronize()
clocks = s.kernel_clocks()
s.kernel_timing(False)
med = {k: float(np.median(v)) for k, v in res.items()}
for k, v in res.items():
    print(f"{k:34s}: ms {np.round(v, 4)} median {med[k]:.4f}")
spread = {k: round((max(v) - min(v)) / med[k], 3) for k, v in res.items()}
ratio = lambda x, y: round(med[x] / med[y], 3)
ratios = {"a / b lone": ratio("a shadow lone", "b rays one origin lone"),
          "a / b queued": ratio("a shadow queued", "b rays one origin queued"),
          "a / r queued": ratio("a shadow queued", "r render queued")}
if sc:
    ratios["a / c lone"] = ratio("a shadow lone", "c shadow closest-hit build lone")
    ratios["a / c queued"] = ratio("a shadow queued", "c shadow closest-hit build queued")
summary = {
    "device": torch.cuda.get_device_name(0), "build": sf.build_info()["source_sha256"],
    "clock_mhz_live_median": float(np.median(clocks)) if len(clocks) else None,
    "n": N, "reps": REPS, "size": [W, H], "K": K, "light": LIGHT, "bias": bias,
    "ms_median": {k: round(v, 4) for k, v in med.items()}, "spread_of_median": spread, "ratio": ratios,
    "surface_pixels": int(surf_h.sum()), "shadowed": int((vis_a == 0).sum()),
    "shadow_equals_rays_plus_compare": same_b, "closest_hit_build_equals_shadow": same_c,
    "overflow_groups": int(s.stats().overflow_tiles),
}
print(json.dumps(summary))
if sc:
    sc.close()
s.close()
