#!/usr/bin/env python3
"""Cost of many lights per pixel in one launch (sf_trace_shadows_to, sf_light_image_many), one process, one GPU, at
1920 x 1080, K = 0.25, bias 2^-10:
  a   trace_shadow from the `side` light (-1.5, -2.5, 2.0): the single-light kernel, the basis
  a1  trace_shadows with n = 1 from the same light (8 B per pixel out instead of 1)
  b0  16 queued trace_shadow calls for lights.disc(side, 0.25, 16) into 16 byte images
  b   the fused n = 16 launch (same bits, checked)
  c   n = 64, lights.sky(64)
  d   light_image_many at n = 16
  r   Render() of the frame itself, for scale
each lone (synchronised each time) and queued back to back. The bits of every compared pair are checked equal before
timing. After a 300 ms settle under load the cases run interleaved, REPS rounds; medians, the spread between rounds,
ratios, the live shader clock and the build are printed, the last line as JSON.
Usage: shadows_probe.py [N=20] [REPS=5] [JSON path]"""
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
SIDE = (-1.5, -2.5, 2.0)
BIAS = 2.0 ** -10

cam = sf.config_camera(W, H, K)
s = sf.Sphereflake(W, H)
s.SetCamera(cam)
s.Render()
DISC = lights.disc(SIDE, 0.25, 16)
SKY = lights.sky(64)
vis16 = [torch.empty((H, W), dtype=torch.uint8, device="cuda") for _ in range(16)]
m16 = torch.empty((H, W), dtype=torch.int64, device="cuda")
m64 = torch.empty((H, W), dtype=torch.int64, device="cuda")
m1 = torch.empty((H, W), dtype=torch.int64, device="cuda")
torch.cuda.synchronize()


def b0():
    for i in range(16):
        s.trace_shadow(DISC[i], bias=BIAS, out=vis16[i])


as_u64 = lambda t: t.cpu().numpy().view(np.uint64)
# the bits of every compared pair
s.trace_shadow(SIDE, bias=BIAS)
vis_a = s.download_shadow()
s.trace_shadows([SIDE], bias=BIAS, out=m1)
s.Synchronize()
same_a1 = bool(np.array_equal(as_u64(m1), lights.masks_from_vis([vis_a])))
assert same_a1, "trace_shadows with n = 1 differs from trace_shadow"
b0()
s.trace_shadows(DISC, bias=BIAS, out=m16)
s.Synchronize()
mask16 = as_u64(m16)
same_b = bool(np.array_equal(mask16, lights.masks_from_vis([v.cpu().numpy() for v in vis16])))
assert same_b, "the fused n = 16 launch differs from 16 trace_shadow calls"
s.trace_shadows(SKY, bias=BIAS, out=m64)
s.Synchronize()
mask64 = as_u64(m64)
overflow_setup = int(s.stats().overflow_tiles)
s.trace_shadows(DISC, bias=BIAS)   # the context's mask buffer, for d
s.PostProcess()
s.Synchronize()


def popcount(a):
    return np.unpackbits(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (-1,)), axis=-1).sum(axis=-1)


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


calls = {
    "a shadow": lambda: s.trace_shadow(SIDE, bias=BIAS),
    "a1 shadows n=1": lambda: s.trace_shadows([SIDE], bias=BIAS, out=m1),
    "b0 16 x shadow": b0,
    "b shadows n=16": lambda: s.trace_shadows(DISC, bias=BIAS, out=m16),
    "c shadows n=64 sky": lambda: s.trace_shadows(SKY, bias=BIAS, out=m64),
    "d light_image_many n=16": lambda: s.light_image_many(DISC),
    "r render": lambda: s.Render(),
}
cases = {}
for name, call in calls.items():
    cases[name + " lone"] = (lambda call=call: lone(call))
    cases[name + " queued"] = (lambda call=call: queued(call))
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
    ratios[f"a1 / a {mode}"] = ratio(f"a1 shadows n=1 {mode}", f"a shadow {mode}")
    ratios[f"b / b0 {mode}"] = ratio(f"b shadows n=16 {mode}", f"b0 16 x shadow {mode}")
    ratios[f"b / (16 a) {mode}"] = round(med[f"b shadows n=16 {mode}"] / (16 * med[f"a shadow {mode}"]), 3)
    ratios[f"c / (64 a) {mode}"] = round(med[f"c shadows n=64 sky {mode}"] / (64 * med[f"a shadow {mode}"]), 3)
pc16 = popcount(mask16)
summary = {
    "device": torch.cuda.get_device_name(0), "build": sf.build_info()["source_sha256"],
    "clock_mhz_live_median": float(np.median(clocks)) if len(clocks) else None,
    "n": N, "reps": REPS, "size": [W, H], "K": K, "side": SIDE, "bias": BIAS,
    "ms_median": {k: round(v, 4) for k, v in med.items()}, "spread_of_median": spread, "ratio": ratios,
    "rounds_ms": {k: [round(x, 4) for x in v] for k, v in res.items()},
    "shadowed_a": int((vis_a == 0).sum()),
    "disc16": {"all_shadowed": int((pc16 == 0).sum()), "all_lit": int((pc16 == 16).sum()),
               "penumbra": int(((pc16 > 0) & (pc16 < 16)).sum())},
    "sky64_mean_visible_fraction": float(popcount(mask64).mean() / 64.0),
    "n1_equals_shadow": same_a1, "n16_equals_16_shadows": same_b,
    "overflow_tiles_after_setup": overflow_setup, "overflow_tiles": int(s.stats().overflow_tiles),
}
print(json.dumps(summary))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
s.close()
