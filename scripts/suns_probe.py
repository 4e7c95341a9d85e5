#!/usr/bin/env python3
"""Cost of many sun directions per pixel in one launch (sf_trace_suns_to, sf_light_image_suns), one process, one GPU, at
1920 x 1080, K = 0.25, tau = 4, bias 2^-10, the sun towards `side` = normalize(-1.5, -2.5, 2.0):
  a   one trace_sun on the frame's own G-buffer
  a1  trace_suns, n = 1, the same direction (the price of the loop and the 8-byte word)
  b0  what the fused launch replaces: 16 trace_sun calls, one per direction of sun_cone(side, 5 degrees, 16)
  b   trace_suns of those 16 directions: one launch, one mask word per pixel
  c   trace_suns of sky_dirs(64): the sky dome
  d   light_image_suns, n = 16
  r   Render() of the frame itself, for scale
each lone (synchronised each time) and queued back to back. The bits are checked first: bit i of a1, b and c is
trace_sun's byte for direction i. After a 300 ms settle under load the cases run interleaved, REPS rounds; medians, the
spread between rounds, ratios, the live shader clock and the build are printed, the last line as JSON.
Usage: suns_probe.py [N=20] [REPS=5] [JSON path]"""
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
SIDE = (-1.5, -2.5, 2.0)
SUN = lights.sun_direction(SIDE)
CONE = lights.sun_cone(SIDE, np.radians(5.0), 16)
SKY = lights.sky_dirs(64)

cam = sf.config_camera(W, H, K)
s = sf.Sphereflake(W, H)
s.SetCamera(cam)
s.Render()
pos, _, _, _ = s.download()
surf = ~((pos[..., 0] == 0) & (pos[..., 1] == 0) & (pos[..., 2] == 0))


def single(dirs):
    """The mask words from one trace_sun per direction."""
    vis = []
    for sdir in dirs:
        s.trace_sun(sdir, TAU, bias=BIAS)
        vis.append(s.download_shadow())
    return lights.masks_from_vis(vis)


def fused(dirs):
    s.trace_suns(dirs, TAU, bias=BIAS)
    return s.download_shadow_masks()


# the bits of the compared pairs
want_b, want_c = single(CONE), single(SKY)
got_a1, got_b, got_c = fused([SUN]), fused(CONE), fused(SKY)
assert np.array_equal(got_a1, single([SUN])), "trace_suns n = 1 differs from trace_sun"
assert np.array_equal(got_b, want_b), "trace_suns of the cone differs from 16 trace_sun calls"
assert np.array_equal(got_c, want_c), "trace_suns of the sky differs from 64 trace_sun calls"
popcount = lambda m: np.unpackbits(np.ascontiguousarray(m).view(np.uint8).reshape(m.shape + (8,)), axis=-1).sum(axis=-1)
pc_b, pc_c = popcount(got_b), popcount(got_c)
overflow_setup = int(s.stats().overflow_tiles)
fused(CONE)   # the context's mask buffer, for d
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


def sixteen():
    for sdir in CONE:
        s.trace_sun(sdir, TAU, bias=BIAS)


calls = {
    "a sun": lambda: s.trace_sun(SUN, TAU, bias=BIAS),
    "a1 suns n=1": lambda: s.trace_suns([SUN], TAU, bias=BIAS),
    "b0 16 suns, 16 launches": sixteen,
    "b suns n=16": lambda: s.trace_suns(CONE, TAU, bias=BIAS),
    "c suns n=64 sky": lambda: s.trace_suns(SKY, TAU, bias=BIAS),
    "d light_image_suns n=16": lambda: s.light_image_suns(CONE),
    "r render": lambda: s.Render(),
}
cases = {}
for name, call in calls.items():
    for mode, how in (("lone", lone), ("queued", queued)):
        cases[f"{name} {mode}"] = (lambda call=call, how=how: how(call))
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
ratios, ratio_rounds = {}, {}
for mode in ("lone", "queued"):
    ratios[f"a1 / a {mode}"] = ratio(f"a1 suns n=1 {mode}", f"a sun {mode}")
    ratios[f"b / b0 {mode}"] = ratio(f"b suns n=16 {mode}", f"b0 16 suns, 16 launches {mode}")
    ratios[f"b / 16 a {mode}"] = round(med[f"b suns n=16 {mode}"] / (16.0 * med[f"a sun {mode}"]), 3)
    ratios[f"c / 4 b {mode}"] = round(med[f"c suns n=64 sky {mode}"] / (4.0 * med[f"b suns n=16 {mode}"]), 3)
    ratio_rounds[f"b / b0 {mode}"] = [round(x / y, 3) for x, y in zip(res[f"b suns n=16 {mode}"],
                                                                      res[f"b0 16 suns, 16 launches {mode}"])]
nsurf = int(surf.sum())
summary = {
    "device": torch.cuda.get_device_name(0), "build": sf.build_info()["source_sha256"],
    "clock_mhz_live_median": float(np.median(clocks)) if len(clocks) else None,
    "n": N, "reps": REPS, "size": [W, H], "K": K, "sun": [float(x) for x in SUN], "tau": TAU, "bias": BIAS,
    "ms_median": {k: round(v, 4) for k, v in med.items()}, "spread_of_median": spread, "ratio": ratios,
    "ratio_per_round": ratio_rounds,
    "rounds_ms": {k: [round(x, 4) for x in v] for k, v in res.items()},
    "surface_pixels": nsurf, "bits_equal_the_single_launches": True,
    "cone_penumbra_pixels": int((surf & (pc_b > 0) & (pc_b < 16)).sum()),
    "cone_all_shadowed": int((surf & (pc_b == 0)).sum()), "cone_all_lit": int((surf & (pc_b == 16)).sum()),
    "sky_mean_visible_fraction": float(pc_c[surf].mean() / 64.0),
    "overflow_tiles_after_setup": overflow_setup, "overflow_tiles": int(s.stats().overflow_tiles),
}
print(json.dumps(summary))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
s.close()
