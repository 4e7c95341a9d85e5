#!/usr/bin/env python3
"""Cost of shadows from a directional light (sf_trace_sun_to, sf_light_image_sun, sf_set_shadow_lod), one process, one
GPU, at 1920 x 1080, K = 0.25, tau = 4, bias 2^-10, the sun towards `side` = normalize(-1.5, -2.5, 2.0):
  a   trace_sun on the frame's own G-buffer: the fused any-hit launch
  b   what it replaces on the device: trace_rays of the same per-pixel origins F and directions d through
      sf_trace_rays_wave (closest hit, mixed origins), all four outputs; the host's min_t < bound gives a's bytes
      (checked)
  b1  the same writing min_t only (separates the outputs from the any-hit mode)
  p   trace_shadow from a point light at 4 s: the price of parallel rays over one origin
  m   a with set_shadow_lod(matched_lod(4, closest)): the price of the camera's detail
  l   light_image_sun, l0 light_image
  r   Render() of the frame itself, for scale
each lone (synchronised each time) and queued back to back. After a 300 ms settle under load the cases run interleaved,
REPS rounds; medians, the spread between rounds, ratios, the live shader clock and the build are printed, the last line
as JSON.
Usage: sun_probe.py [N=20] [REPS=5] [JSON path]"""
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

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
OUT = sys.argv[3] if len(sys.argv) > 3 else None
W, H, K = 1920, 1080, 0.25
TAU = 4.0
BIAS = 2.0 ** -10
SUN = lights.sun_direction((-1.5, -2.5, 2.0))
POINT = (SUN * np.float32(TAU)).astype(np.float32)

cam = sf.config_camera(W, H, K)
s = sf.Sphereflake(W, H)
s.SetCamera(cam)
s.Render()
pos, _, _, _ = s.download()
closest = float(s.stats().closest)
C = float(lights.matched_lod(TAU, closest))
origin = cam.corners()[0]
Fo, d, bound, surf = lights.sun_model(pos, origin, SUN, TAU, BIAS)
Ft = torch.from_numpy(np.ascontiguousarray(Fo.reshape(-1, 3))).cuda()
dt = torch.from_numpy(np.ascontiguousarray(d)).cuda()
mk = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device="cuda")
out4 = (mk(H, W, 4), mk(H, W, 4), mk(H, W), mk(H, W, dtype=torch.int32))
out1 = (None, None, mk(H, W), None)
torch.cuda.synchronize()

# the bits of the compared pair
s.trace_sun(SUN, TAU, bias=BIAS)
vis_a = s.download_shadow()
s.trace_rays(Ft, dt, out=out4)
s.Synchronize()
want = np.where(surf & (out4[2].cpu().numpy() < bound), 0, 255).astype(np.uint8)
same_b = bool(np.array_equal(vis_a, want))
assert same_b, "trace_sun differs from trace_rays and min_t < bound"
s.trace_rays(Ft, dt, out=out1)
s.Synchronize()
assert np.array_equal(out1[2].cpu().numpy().view(np.uint32), out4[2].cpu().numpy().view(np.uint32))
s.set_shadow_lod(C)
s.trace_sun(SUN, TAU, bias=BIAS)
vis_m = s.download_shadow()
s.set_shadow_lod(0.0)
s.trace_shadow(POINT, bias=BIAS)
vis_p = s.download_shadow()
overflow_setup = int(s.stats().overflow_tiles)
s.trace_sun(SUN, TAU, bias=BIAS)   # the context's visibility buffer, for l
s.PostProcess()
s.Synchronize()


def lone(call):
    ts = []
    for _ in range(N):
        t = time.perf_counter()
        call()
        s.Synchronize()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e3


def queued(call):
    call()
    s.Synchronize()
    t = time.perf_counter()
    for _ in range(N):
        call()
    s.Synchronize()
    return (time.perf_counter() - t) / N * 1e3


def at_matched(measure):
    """`measure` with the shadow traces at the matched constant (set and reset outside the timed calls)."""
    s.set_shadow_lod(C)
    try:
        return measure()
    finally:
        s.set_shadow_lod(0.0)


sun = lambda: s.trace_sun(SUN, TAU, bias=BIAS)
calls = {
    "a sun": (sun, False),
    "b rays 4 outputs": (lambda: s.trace_rays(Ft, dt, out=out4), False),
    "b1 rays min_t only": (lambda: s.trace_rays(Ft, dt, out=out1), False),
    "p point shadow at 4 s": (lambda: s.trace_shadow(POINT, bias=BIAS), False),
    "m sun at matched lod": (sun, True),
    "l light_image_sun": (lambda: s.light_image_sun(SUN), False),
    "l0 light_image": (lambda: s.light_image(POINT), False),
    "r render": (lambda: s.Render(), False),
}
cases = {}
for name, (call, fine) in calls.items():
    for mode, how in (("lone", lone), ("queued", queued)):
        run = (lambda call=call, how=how: how(call))
        cases[f"{name} {mode}"] = (lambda run=run: at_matched(run)) if fine else run
t0 = time.perf_counter()
while time.perf_counter() - t0 < 0.3:   # clock settle under load
    queued(lambda: s.Render())
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
ratios = {}
for mode in ("lone", "queued"):
    ratios[f"a / b {mode}"] = ratio(f"a sun {mode}", f"b rays 4 outputs {mode}")
    ratios[f"a / b1 {mode}"] = ratio(f"a sun {mode}", f"b1 rays min_t only {mode}")
    ratios[f"b1 / b {mode}"] = ratio(f"b1 rays min_t only {mode}", f"b rays 4 outputs {mode}")
    ratios[f"a / p {mode}"] = ratio(f"a sun {mode}", f"p point shadow at 4 s {mode}")
    ratios[f"m / a {mode}"] = ratio(f"m sun at matched lod {mode}", f"a sun {mode}")
    ratios[f"l / l0 {mode}"] = ratio(f"l light_image_sun {mode}", f"l0 light_image {mode}")
nsurf = int(surf.sum())
summary = {
    "device": torch.cuda.get_device_name(0), "build": sf.build_info()["source_sha256"],
    "clock_mhz_live_median": float(np.median(clocks)) if len(clocks) else None,
    "n": N, "reps": REPS, "size": [W, H], "K": K, "sun": [float(x) for x in SUN], "tau": TAU, "bias": BIAS,
    "closest": closest, "matched_lod": C,
    "ms_median": {k: round(v, 4) for k, v in med.items()}, "spread_of_median": spread, "ratio": ratios,
    "rounds_ms": {k: [round(x, 4) for x in v] for k, v in res.items()},
    "surface_pixels": nsurf, "shadowed_a": int((vis_a == 0).sum()), "shadowed_m": int((vis_m == 0).sum()),
    "a_differs_from_m": int((vis_a != vis_m).sum()), "shadowed_p": int((vis_p == 0).sum()),
    "sun_equals_rays": same_b,
    "overflow_tiles_after_setup": overflow_setup, "overflow_tiles": int(s.stats().overflow_tiles),
}
print(json.dumps(summary))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
s.close()
