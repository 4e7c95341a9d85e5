#!/usr/bin/env python3
"""Cost of the light shafts (sf_trace_shafts_to, sf_light_image_shafts), one process, one GPU, at 1920 x 1080, K = 0.25,
bias 2^-10, the sun towards normalize(SUN) (default (-1.5, -2.5, 2.0), scripts/sun_probe.py's: about two pixels in five
part lit; (4, 7, 2) is the README's back-lit sun, which this close camera sees all shadowed), the frame's misses marched
to far = |origin| + 2 along the unit pinhole directions, tau = lights.shaft_distance of those march ends, fractions
(i + 0.5) / n:
  a   one trace_sun on the frame's own G-buffer
  a1  trace_shafts, n = 1, sigma = 1, no direction image (the price of the loop and the 8-byte word)
  b0  what the fused launch replaces on the device: 16 trace_sun calls, one per pre-scaled device image Q_i, each into
      its own device byte image (the host-side scaling and the uploads it also replaces are not timed)
  b   trace_shafts of those 16 samples: one launch, one mask word per pixel
  c   trace_shafts, n = 64
  d   light_image_shafts, n = 16
  r   Render() of the frame itself, for scale
each lone (synchronised each time) and queued back to back. The bits are checked first: bit i of a1, b and c is
trace_sun's byte on Q_i. After a 300 ms settle under load the cases run interleaved, REPS rounds; medians, the spread
between rounds, ratios, the live shader clock and the build are printed, the last line as JSON.
With `unfused` as the fourth argument only a, b0 and r run, through entry points every earlier build of the library has:
SF_LIB=<another build> SF_LIB_PARTIAL=1 then times that build's own trace_sun.
Usage: shafts_probe.py [N=20] [REPS=5] [JSON path | -] [unfused | fused] [SUN = x,y,z]"""
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sphereflake-raytracer_amd"))
import sphereflake_amd as sf  # noqa: E402
from sphereflake_amd import dirs as sfdirs, lights  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 20
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
OUT = sys.argv[3] if len(sys.argv) > 3 and sys.argv[3] != "-" else None
UNFUSED = len(sys.argv) > 4 and sys.argv[4] == "unfused"
W, H, K = 1920, 1080, 0.25
BIAS = 2.0 ** -10
SUN = lights.sun_direction([float(x) for x in sys.argv[5].split(",")] if len(sys.argv) > 5 else (-1.5, -2.5, 2.0))
F16 = np.array([(i + 0.5) / 16 for i in range(16)], np.float32)
F64 = np.array([(i + 0.5) / 64 for i in range(64)], np.float32)

cam = sf.config_camera(W, H, K)
s = sf.Sphereflake(W, H)
s.SetCamera(cam)
s.Render()
pos, _, _, _ = s.download()
surf = ~((pos[..., 0] == 0) & (pos[..., 1] == 0) & (pos[..., 2] == 0))
o, tl, tr, bl = cam.corners()
D = np.asarray(sfdirs.pinhole(o, tl, tr, bl, W, H), np.float32)
D = np.ascontiguousarray((D / np.linalg.norm(D, axis=-1, keepdims=True)).astype(np.float32))
FAR = float(np.float32(np.linalg.norm(np.asarray(o, np.float64)) + 2.0))


def ends():
    E = np.array(pos[..., :3], np.float32, copy=True)
    E[~surf] = D[~surf] * np.float32(FAR)
    return E


E = ends()
r = np.linalg.norm(np.asarray(o, np.float64) + E.astype(np.float64), axis=-1).max()
TAU = float(np.nextafter(np.float32(2.0 + max(r, np.linalg.norm(np.asarray(o, np.float64)))), np.float32(np.inf)))


def scaled(sigma):
    """The device image Q = E sigma as a [H, W, 4] position image."""
    Q = np.zeros((H, W, 4), np.float32)
    Q[..., :3] = E * np.float32(sigma)
    return torch.from_numpy(Q).cuda()


Qt = [scaled(x) for x in F16]
vis16 = [torch.empty((H, W), dtype=torch.uint8, device="cuda") for _ in F16]
dt = torch.from_numpy(D).cuda()
torch.cuda.synchronize()


def sixteen():
    for q, v in zip(Qt, vis16):
        s.trace_sun(SUN, TAU, bias=BIAS, pos=q, out=v)


def single(fractions):
    """The mask words from one trace_sun per pre-scaled image."""
    vis = []
    out = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    for x in fractions:
        s.trace_sun(SUN, TAU, bias=BIAS, pos=scaled(x), out=out)
        s.Synchronize()
        vis.append(out.cpu().numpy())
    return lights.masks_from_vis(vis)


def fused(fractions, marched=True):
    s.trace_shafts(SUN, fractions, TAU, bias=BIAS, dirs=dt if marched else None, far=FAR if marched else 0.0)
    return s.download_shadow_masks()


extra = {}
if not UNFUSED:
    # the bits of the compared pairs
    s.trace_sun(SUN, TAU, bias=BIAS)
    assert np.array_equal(fused([1.0], False), np.where(s.download_shadow() != 0, 1, 0).astype(np.uint64)), \
        "trace_shafts n = 1, sigma = 1 differs from trace_sun"
    got_b, got_c = fused(F16), fused(F64)
    assert np.array_equal(got_b, single(F16)), "trace_shafts n = 16 differs from 16 trace_sun calls"
    assert np.array_equal(got_c, single(F64)), "trace_shafts n = 64 differs from 64 trace_sun calls"
    popcount = lambda m: np.unpackbits(np.ascontiguousarray(m).view(np.uint8).reshape(m.shape + (8,)), axis=-1).sum(axis=-1)
    pc_b = popcount(got_b)
    extra = {"bits_equal_the_single_launches": True,
             "surface_part_lit": int((surf & (pc_b > 0) & (pc_b < 16)).sum()),
             "surface_all_shadowed": int((surf & (pc_b == 0)).sum()), "surface_all_lit": int((surf & (pc_b == 16)).sum()),
             "miss_part_lit": int((~surf & (pc_b > 0) & (pc_b < 16)).sum()),
             "miss_all_lit": int((~surf & (pc_b == 16)).sum()),
             "mean_lit_fraction_n64": float(popcount(got_c).mean() / 64.0)}
    fused(F16)   # the context's mask buffer, for d
overflow_setup = int(s.stats().overflow_tiles)
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


calls = {"a sun": lambda: s.trace_sun(SUN, TAU, bias=BIAS), "b0 16 suns, 16 launches": sixteen}
if not UNFUSED:
    calls.update({
        "a1 shafts n=1": lambda: s.trace_shafts(SUN, [1.0], TAU, bias=BIAS),
        "b shafts n=16": lambda: s.trace_shafts(SUN, F16, TAU, bias=BIAS, dirs=dt, far=FAR),
        "c shafts n=64": lambda: s.trace_shafts(SUN, F64, TAU, bias=BIAS, dirs=dt, far=FAR),
        "d light_image_shafts n=16": lambda: s.light_image_shafts(F16, None, 0.05, (255.0, 240.0, 200.0), dirs=dt, far=FAR),
    })
calls["r render"] = lambda: s.Render()
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
    ratios[f"b0 / 16 a {mode}"] = round(med[f"b0 16 suns, 16 launches {mode}"] / (16.0 * med[f"a sun {mode}"]), 3)
    if UNFUSED:
        continue
    ratios[f"a1 / a {mode}"] = ratio(f"a1 shafts n=1 {mode}", f"a sun {mode}")
    ratios[f"b / b0 {mode}"] = ratio(f"b shafts n=16 {mode}", f"b0 16 suns, 16 launches {mode}")
    ratios[f"c / 4 b {mode}"] = round(med[f"c shafts n=64 {mode}"] / (4.0 * med[f"b shafts n=16 {mode}"]), 3)
    ratio_rounds[f"b / b0 {mode}"] = [round(x / y, 3) for x, y in zip(res[f"b shafts n=16 {mode}"],
                                                                      res[f"b0 16 suns, 16 launches {mode}"])]
summary = {
    "device": torch.cuda.get_device_name(0), "build": sf.build_info()["source_sha256"], "library": os.path.relpath(sf.LIB_PATH, REPO),
    "unfused_only": UNFUSED,
    "clock_mhz_live_median": float(np.median(clocks)) if len(clocks) else None,
    "n": N, "reps": REPS, "size": [W, H], "K": K, "sun": [float(x) for x in SUN], "tau": TAU, "far": FAR, "bias": BIAS,
    "ms_median": {k: round(v, 4) for k, v in med.items()}, "spread_of_median": spread, "ratio": ratios,
    "ratio_per_round": ratio_rounds,
    "rounds_ms": {k: [round(x, 4) for x in v] for k, v in res.items()},
    "surface_pixels": int(surf.sum()), **extra,
    "overflow_tiles_after_setup": overflow_setup, "overflow_tiles": int(s.stats().overflow_tiles),
}
print(json.dumps(summary))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
s.close()
