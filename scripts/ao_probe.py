#!/usr/bin/env python3
"""Cost of ambient occlusion about each pixel's normal (sf_trace_ao, sf_trace_ao_sum) against the world-fixed sky dome
(sf_trace_suns, sf_trace_suns_sum), one process, one GPU, at 1920 x 1080, K = 0.25 (the bench's camera), tau = 4, bias
2^-10, on the frame's own G-buffer, for n = 16 and n = 64:
  ao   trace_ao(ao_samples(n))                      su   trace_suns(sky_dirs(n))
  aos  trace_ao_sum(...) + light_image_buffer()      sus  trace_suns_sum(...) + light_image_buffer()
  aoc  trace_ao on the same positions under the constant normal (0, 0, 1)
  suc  trace_suns(ao_directions((0, 0, 1), samples)) on them: the same rays as aoc, bit for bit -- the kernel's own cost
       apart from what differing normals do to the traversal
  r    Render() of the frame itself, for scale
each queued back to back on the context's stream (and lone, synchronised each time). The bits are checked first: on a
normal image that holds the constant (0, 0, 1), trace_ao equals trace_suns of lights.ao_directions, and trace_ao_sum
equals lights.ao_sum_model over trace_ao's mask. After a 300 ms settle under load the cases run interleaved, REPS rounds;
medians, the spread between rounds, ratios, the live shader clock and the build are printed, the last line as JSON.
Usage: ao_probe.py [N=20] [REPS=5] [JSON path]"""
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
SIZES = (16, 64)
SKY_COLOUR = (0.5, 0.75, 1.0)

cam = sf.config_camera(W, H, K)
s = sf.Sphereflake(W, H)
s.SetCamera(cam)
s.Render()
s.PostProcess()
pos, nrm, _, _ = s.download()
surf = ~((pos[..., 0] == 0) & (pos[..., 1] == 0) & (pos[..., 2] == 0))

# the bits first: the constant-normal identity on the frame's positions, and the sum against the host model
h16 = lights.ao_samples(16)
pt = torch.from_numpy(np.ascontiguousarray(pos)).cuda()
up = np.zeros_like(nrm)
up[..., 2] = 1.0
nt = torch.from_numpy(up).cuda()
m_ao = torch.zeros((H, W), dtype=torch.int64, device="cuda")
m_su = torch.zeros((H, W), dtype=torch.int64, device="cuda")
s.trace_ao(h16, TAU, BIAS, pos=pt, nrm=nt, out=m_ao)
s.trace_suns(lights.ao_directions(np.array((0.0, 0.0, 1.0), np.float32), h16), TAU, bias=BIAS, pos=pt, out=m_su)
s.Synchronize()
assert torch.equal(m_ao, m_su), "trace_ao on a constant normal differs from trace_suns of ao_directions"
col16 = lights.ao_colours(h16, SKY_COLOUR)
s.trace_ao(h16, TAU, BIAS)
mask16 = s.download_shadow_masks()
s.trace_ao_sum(h16, col16, False, TAU, BIAS)
buf16 = s.download_light()
want = lights.ao_sum_model(None, pos, mask16, col16)
assert np.array_equal(buf16.view(np.uint32), want.view(np.uint32)), "trace_ao_sum differs from ao_sum_model"
popcount = lambda m: np.unpackbits(np.ascontiguousarray(m).view(np.uint8).reshape(m.shape + (8,)), axis=-1).sum(axis=-1)
s.trace_suns(lights.sky_dirs(16), TAU, bias=BIAS)
open_ao, open_sky = popcount(mask16)[surf].mean() / 16.0, popcount(s.download_shadow_masks())[surf].mean() / 16.0
overflow_setup = int(s.stats().overflow_tiles)
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


def summed(trace, pts, col):
    def call():
        trace(pts, col, False, TAU, BIAS)
        s.light_image_buffer()
    return call


calls = {"r render": lambda: s.Render()}
for n in SIZES:
    hs, sky = lights.ao_samples(n), lights.sky_dirs(n)
    calls[f"ao n={n}"] = lambda hs=hs: s.trace_ao(hs, TAU, BIAS)
    calls[f"su n={n}"] = lambda sky=sky: s.trace_suns(sky, TAU, bias=BIAS)
    up_dirs = lights.ao_directions(np.array((0.0, 0.0, 1.0), np.float32), hs)
    calls[f"aoc n={n}"] = lambda hs=hs: s.trace_ao(hs, TAU, BIAS, pos=pt, nrm=nt, out=m_ao)
    calls[f"suc n={n}"] = lambda up_dirs=up_dirs: s.trace_suns(up_dirs, TAU, bias=BIAS, pos=pt, out=m_su)
    calls[f"aos n={n}"] = summed(s.trace_ao_sum, hs, lights.ao_colours(hs, SKY_COLOUR))
    calls[f"sus n={n}"] = summed(s.trace_suns_sum, sky, lights.sky_colours(sky))
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
    print(f"{k:24s}: ms {np.round(v, 4)} median {med[k]:.4f}")
spread = {k: round((max(v) - min(v)) / med[k], 3) for k, v in res.items()}
ratios, ratio_rounds = {}, {}
for mode in ("lone", "queued"):
    for n in SIZES:
        for a, b in (("ao", "su"), ("aos", "sus"), ("aoc", "suc"), ("ao", "aoc")):
            ratios[f"{a} / {b} n={n} {mode}"] = round(med[f"{a} n={n} {mode}"] / med[f"{b} n={n} {mode}"], 3)
            ratio_rounds[f"{a} / {b} n={n} {mode}"] = [round(x / y, 3) for x, y in zip(res[f"{a} n={n} {mode}"],
                                                                                         res[f"{b} n={n} {mode}"])]
summary = {
    "device": torch.cuda.get_device_name(0), "build": sf.build_info()["source_sha256"],
    "clock_mhz_live_median": float(np.median(clocks)) if len(clocks) else None,
    "n": N, "reps": REPS, "size": [W, H], "K": K, "tau": TAU, "bias": BIAS,
    "ms_median": {k: round(v, 4) for k, v in med.items()}, "spread_of_median": spread, "ratio": ratios,
    "ratio_per_round": ratio_rounds,
    "rounds_ms": {k: [round(x, 4) for x in v] for k, v in res.items()},
    "surface_pixels": int(surf.sum()), "bits_checked": True,
    "open_fraction_ao_n16": float(open_ao), "open_fraction_sky_dome_n16": float(open_sky),
    "overflow_tiles_after_setup": overflow_setup, "overflow_tiles": int(s.stats().overflow_tiles),
}
print(json.dumps(summary))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
s.close()
