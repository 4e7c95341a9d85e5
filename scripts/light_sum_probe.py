#!/usr/bin/env python3
"""Cost of the colour light buffer (sf_trace_suns_sum_to, sf_trace_shadows_sum_to, sf_light_image_buffer) against what
the same light costs without it, one process, one GPU, at 1920 x 1080, K = 0.25, tau = 4, bias 2^-10:
  s16   sun_cone(side, 5 degrees, 16):  new = trace_suns_sum + light_image_buffer
                                        old = trace_suns + light_image_suns
  s64   sky_dirs(64):                   the same pair
  s256  sky_dirs(256):                  new = ONE trace_suns_sum + light_image_buffer
                                        old = per chunk of 64: trace_suns + download_shadow_masks (the host then has
                                              to unpack and sum the four mask images: timed once, `host_sum_ms`)
  l16   disc(side, 0.25, 16):           new = trace_shadows_sum + light_image_buffer
                                        old = trace_shadows + light_image_many
  l64   sky(64):                        the same pair
each lone (synchronised each time) and queued back to back (s256 old is synchronous by its downloads: lone only).
The "old" side runs the mask kernels of this same library. The bits are checked first on s16 and l16: the buffer equals
lights.sum_model over the mask. After a 300 ms settle under load the cases run interleaved, REPS rounds; medians, the
spread between rounds, ratios new / old, the live shader clock and the build are printed, the last line as JSON.
Usage: light_sum_probe.py [N=10] [REPS=5] [JSON path]"""
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

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
OUT = sys.argv[3] if len(sys.argv) > 3 else None
W, H, K = 1920, 1080, 0.25
TAU = 4.0
BIAS = 2.0 ** -10
SIDE = (-1.5, -2.5, 2.0)
CONE = lights.sun_cone(SIDE, np.radians(5.0), 16)
SKY64 = lights.sky_dirs(64)
SKY256 = lights.sky_dirs(256, limit=lights.SUM_MAX)
DISC = lights.disc(SIDE, 0.25, 16)
LSKY = lights.sky(64)
grey = lambda n: np.full((n, 3), np.float32(1.0) / np.float32(n), np.float32)

cam = sf.config_camera(W, H, K)
s = sf.Sphereflake(W, H)
s.SetCamera(cam)
s.Render()
s.PostProcess()
pos, nrm, _, _ = s.download()
origin = cam.corners()[0]

# the bits of the two 16-entry cases
s.trace_suns(CONE, TAU, bias=BIAS)
want = lights.sum_model(None, pos, nrm, [s.download_shadow_masks()], CONE, None, "suns")
s.trace_suns_sum(CONE, None, distance=TAU, bias=BIAS)
assert np.array_equal(s.download_light().view(np.uint32), want.view(np.uint32)), "s16 differs from the model"
s.trace_shadows(DISC, bias=BIAS)
want = lights.sum_model(None, pos, nrm, [s.download_shadow_masks()], DISC, None, "shadows", origin)
s.trace_shadows_sum(DISC, None, bias=BIAS)
assert np.array_equal(s.download_light().view(np.uint32), want.view(np.uint32)), "l16 differs from the model"
overflow_setup = int(s.stats().overflow_tiles)


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


def new_suns(D):
    s.trace_suns_sum(D, None, distance=TAU, bias=BIAS)
    s.light_image_buffer()


def old_suns(D):
    s.trace_suns(D, TAU, bias=BIAS)
    s.light_image_suns(D, None, ambient=0.0)


def old_suns_chunks(D):
    return [(s.trace_suns(D[j:j + 64], TAU, bias=BIAS), s.download_shadow_masks())[1] for j in range(0, len(D), 64)]


def new_lights(L):
    s.trace_shadows_sum(L, None, bias=BIAS)
    s.light_image_buffer()


def old_lights(L):
    s.trace_shadows(L, bias=BIAS)
    s.light_image_many(L, None, ambient=0.0)


def host_sum(masks, n):
    """The README's host sum of a sky beyond 64 directions: unpack every mask image and add the lit fractions."""
    t = time.perf_counter()
    acc = np.zeros(masks[0].shape, np.float32)
    for m in masks:
        acc += np.unpackbits(m.view(np.uint8).reshape(m.shape + (8,)), axis=-1).sum(axis=-1, dtype=np.float32)
    acc /= np.float32(n)
    return (time.perf_counter() - t) * 1e3


pairs = {
    "s16": (lambda: new_suns(CONE), lambda: old_suns(CONE)),
    "s64": (lambda: new_suns(SKY64), lambda: old_suns(SKY64)),
    "s256": (lambda: new_suns(SKY256), lambda: old_suns_chunks(SKY256)),
    "l16": (lambda: new_lights(DISC), lambda: old_lights(DISC)),
    "l64": (lambda: new_lights(LSKY), lambda: old_lights(LSKY)),
}
cases = {}
for name, (new, old) in pairs.items():
    for side, call in (("new", new), ("old", old)):
        cases[f"{name} {side} lone"] = (lambda call=call: lone(call))
        if not (name == "s256" and side == "old"):
            cases[f"{name} {side} queued"] = (lambda call=call: queued(call))
cases["r render lone"] = lambda: lone(lambda: s.Render())
host_sum_ms = host_sum(old_suns_chunks(SKY256), 256)
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
    print(f"{k:24s}: ms {np.round(v, 4)} median {med[k]:.4f}")
spread = {k: round((max(v) - min(v)) / med[k], 3) for k, v in res.items()}
ratios, ratio_rounds = {}, {}
for name in pairs:
    for mode in ("lone", "queued"):
        a, b = f"{name} new {mode}", f"{name} old {mode}"
        if b not in med:
            b = f"{name} old lone"
        ratios[f"{name} new / old {mode}"] = round(med[a] / med[b], 3)
        ratio_rounds[f"{name} new / old {mode}"] = [round(x / y, 3) for x, y in zip(res[a], res[b])]
summary = {
    "device": torch.cuda.get_device_name(0), "build": sf.build_info()["source_sha256"],
    "clock_mhz_live_median": float(np.median(clocks)) if len(clocks) else None,
    "n": N, "reps": REPS, "size": [W, H], "K": K, "tau": TAU, "bias": BIAS,
    "ms_median": {k: round(v, 4) for k, v in med.items()}, "spread_of_median": spread, "ratio": ratios,
    "ratio_per_round": ratio_rounds, "rounds_ms": {k: [round(x, 4) for x in v] for k, v in res.items()},
    "s256_old_host_sum_ms_once": round(host_sum_ms, 2), "bits_equal_the_model": True,
    "overflow_tiles_after_setup": overflow_setup, "overflow_tiles": int(s.stats().overflow_tiles),
}
print(json.dumps(summary))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
s.close()
