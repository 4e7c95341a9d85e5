#!/usr/bin/env python3
"""Cost of tracing caller-supplied directions (sf_trace_dirs_to) beside Render(), one process, one GPU:
  render        Render() of the 1080p K = 0.25 view: a lone frame (synchronised each time), frames queued back to
                back on one context, and 3 frames in flight over 3 slots (the bench's loop) -- the yardsticks
  dirs pinhole  trace_dirs of that view's own pixel directions (dirs.pinhole: the same rays, bit for bit -- checked)
  dirs equirect trace_dirs of a 2048 x 1024 panorama from the same origin
each lone and queued. After a 300 ms settle under load the cases run interleaved, REPS rounds; medians, ratios to
the Render() figure of the same kind, the live shader clock and the build are printed, the last line as JSON.
Usage: dirs_probe.py [N=100] [REPS=5]"""
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sphereflake-raytracer_amd"))
import sphereflake_amd as sf  # noqa: E402
from sphereflake_amd import dirs  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 100
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
W, H, K = 1920, 1080, 0.25
PW, PH = 2048, 1024

cam = sf.config_camera(W, H, K)
o, tl, tr, bl = cam.corners()
s = sf.Sphereflake(W, H)
s.SetCamera(cam)
d3 = sf.SphereflakeDist(0, W, H, slots=3)
d3.SetView(o, tl, tr, bl)


def outputs(n):
    return (torch.empty((n, 4), dtype=torch.float32, device="cuda"), torch.empty((n, 4), dtype=torch.float32, device="cuda"),
            torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"))


pin = torch.from_numpy(dirs.pinhole(o, tl, tr, bl, W, H)).cuda()
fwd = (tl + (tr - tl) * np.float32(0.5) + (bl - tl) * np.float32(0.5)) - o
pano = torch.from_numpy(dirs.equirect(PW, PH, fwd, (0.0, 0.0, 1.0))).cuda()
out_pin, out_pano = outputs(W * H), outputs(PW * PH)
torch.cuda.synchronize()

# the pinhole image is the frame: same bits in all four channels
s.Render(emit_aux=True)
s.trace_dirs(pin, out=out_pin)
pos, nrm, mint, idx = s.download(aux=True)
same = all(np.array_equal(a.reshape(-1).view(np.uint32), t.cpu().numpy().reshape(-1).view(np.uint32))
           for a, t in zip((pos, nrm, mint, idx), out_pin))
assert same, "trace_dirs(pinhole) differs from Render()"


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


def in_flight3():
    for _ in range(6):
        d3.RenderBands()
    d3.Synchronize()
    t = time.perf_counter()
    for _ in range(N):
        d3.RenderBands()
    d3.Synchronize()
    return (time.perf_counter() - t) / N * 1e3


render = lambda: s.Render()
t_pin = lambda: s.trace_dirs(pin, out=out_pin)
t_pano = lambda: s.trace_dirs(pano, out=out_pano)
cases = {
    "render lone": lambda: lone(render), "render queued": lambda: queued(render), "render 3 in flight": in_flight3,
    "dirs pinhole lone": lambda: lone(t_pin), "dirs pinhole queued": lambda: queued(t_pin),
    "dirs equirect lone": lambda: lone(t_pano), "dirs equirect queued": lambda: queued(t_pano),
}
t0 = time.perf_counter()
while time.perf_counter() - t0 < 0.3:   # clock settle under load
    queued(render)
s.kernel_timing(True, period=8)
res = {k: [] for k in cases}
for _ in range(REPS):
    for k, f in cases.items():
        res[k].append(f())
clocks = s.kernel_clocks()
s.kernel_timing(False)
med = {k: float(np.median(v)) for k, v in res.items()}
for k, v in res.items():
    print(f"{k:22s}: ms {np.round(v, 4)} median {med[k]:.4f}")
st = s.stats()
hits = int((out_pano[2] < sf.FLT_MAX).sum().item())
summary = {
    "device": torch.cuda.get_device_name(0), "build": sf.build_info()["source_sha256"],
    "clock_mhz_live_median": float(np.median(clocks)) if len(clocks) else None,
    "n": N, "reps": REPS, "ms_median": {k: round(v, 4) for k, v in med.items()},
    "ratio_to_render": {
        "pinhole lone": round(med["dirs pinhole lone"] / med["render lone"], 2),
        "pinhole queued / render queued": round(med["dirs pinhole queued"] / med["render queued"], 2),
        "pinhole queued / render 3 in flight": round(med["dirs pinhole queued"] / med["render 3 in flight"], 2),
        "equirect lone, per ray": round(med["dirs equirect lone"] / med["render lone"] * (W * H) / (PW * PH), 2),
        "equirect queued, per ray": round(med["dirs equirect queued"] / med["render queued"] * (W * H) / (PW * PH), 2),
    },
    "equirect": {"size": [PW, PH], "hits": hits, "max_depth": int(st.max_depth)},
    "overflow_groups": int(st.overflow_tiles), "pinhole_equals_render": bool(same),
}
print(json.dumps(summary))
d3.close()
s.close()
