#!/usr/bin/env python3
"""Cost and quality of ambient occlusion with a per-pixel spin and the edge-aware light filter (sf_trace_ao_spin,
sf_trace_ao_spin_sum, sf_light_filter), one process, one GPU, at 1920 x 1080, K = 0.25 (the bench's camera), tau = 4,
bias 2^-10, on the frame's own G-buffer (scripts/ao_probe.py's camera, rounds and settle):
  ao    trace_ao(ao_samples(n))                          n = 4, 16, 64
  sp    trace_ao(ao_samples(n), spin=ao_spins(4))        the same n: what the spin costs per ray
  f4    light_filter(4) into a caller's buffer           the kernel alone, against its HBM floor (48 B read + 16 B
                                                         written per pixel at the achievable 6.29 TB/s)
  f4o   light_filter(4) in place                         the kernel and the copy back
  p4    trace_ao_sum(h4, spin=ao_spins(4)) + light_filter(4)
  p8    trace_ao_sum(h8, spin=ao_spins(2)) + light_filter(2)
  s16, s64   trace_ao_sum(ao_samples(n)) unspun, what p4 and p8 stand in for
  r     Render() of the frame itself, for scale
each queued back to back on the context's stream (and lone, synchronised each time). The bits are checked first: the
identity table gives trace_ao's mask, the spun sum equals lights.ao_sum_model over the spun mask, and light_filter equals
lights.light_filter_model. Then the RMS error of the open fraction against the unspun n = 64 sum, over the surface
pixels, of p4, p8, s16 and of unspun n = 4 and n = 8. After a 300 ms settle under load the cases run interleaved, REPS
rounds; medians, the spread between rounds, ratios, the live shader clock and the build are printed, the last line as
JSON.
Usage: ao_spin_probe.py [N=20] [REPS=5] [JSON path]"""
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
SIZES = (4, 16, 64)
HBM_ACHIEVABLE = 6.29e12   # bytes / s, a float4 copy on this part
FILTER_BYTES = W * H * 64   # pos4, nrm4 and the buffer read, the result written

cam = sf.config_camera(W, H, K)
s = sf.Sphereflake(W, H)
s.SetCamera(cam)
s.Render()
s.PostProcess()
pos, nrm, _, _ = s.download()
surf = ~((pos[..., 0] == 0) & (pos[..., 1] == 0) & (pos[..., 2] == 0))
S4, S2 = lights.ao_spins(4), lights.ao_spins(2)
h4, h8, h16, h64 = (lights.ao_samples(n) for n in (4, 8, 16, 64))
same = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))

# the bits first
s.trace_ao(h16, TAU, BIAS)
plain16 = s.download_shadow_masks()
s.trace_ao(h16, TAU, BIAS, spin=np.array([[[1.0, 0.0]]], np.float32))
assert np.array_equal(s.download_shadow_masks(), plain16), "the identity table differs from trace_ao"
s.trace_ao(h4, TAU, BIAS, spin=S4)
mask4 = s.download_shadow_masks()
s.trace_ao_sum(h4, None, False, TAU, BIAS, spin=S4)
sum4 = s.download_light()
assert same(sum4, lights.ao_sum_model(None, pos, mask4, np.full((4, 3), np.float32(0.25)))), "the spun sum differs"
s.light_filter(4)
p4_buf = s.download_light()
assert same(p4_buf, lights.light_filter_model(sum4, pos, nrm, 4)), "light_filter differs from light_filter_model"
assert s.light_buffer() != 0


def summed(samples, spin=None, size=0):
    s.trace_ao_sum(samples, None, False, TAU, BIAS, spin=spin)
    if size:
        s.light_filter(size)
    return s.download_light()


truth = summed(h64)
frac = lambda b: b[..., 0].astype(np.float64)
rms = lambda b: float(np.sqrt(np.mean((frac(b) - frac(truth))[surf] ** 2)))
quality = {
    "p4: n=4 spun 4x4 + filter(4)": rms(p4_buf), "p8: n=8 spun 2x2 + filter(2)": rms(summed(h8, S2, 2)),
    "n=4 unspun + filter(4)": rms(summed(h4, None, 4)), "n=4 spun 4x4, unfiltered": rms(sum4),
    "n=4 unspun": rms(summed(h4)), "n=8 unspun": rms(summed(h8)), "s16: n=16 unspun": rms(summed(h16)),
}
for k, v in quality.items():
    print(f"RMS error against unspun n = 64  {k:32s}: {v:.4f}")
overflow_setup = int(s.stats().overflow_tiles)
tmp = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
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


def pipeline(samples, spin, size):
    def call():
        s.trace_ao_sum(samples, None, False, TAU, BIAS, spin=spin)
        s.light_filter(size)
    return call


calls = {"r render": lambda: s.Render()}
for n in SIZES:
    hs = lights.ao_samples(n)
    calls[f"ao n={n}"] = lambda hs=hs: s.trace_ao(hs, TAU, BIAS)
    calls[f"sp n={n}"] = lambda hs=hs: s.trace_ao(hs, TAU, BIAS, spin=S4)
calls["f4"] = lambda: s.light_filter(4, out=tmp)
calls["f4o"] = lambda: s.light_filter(4)
calls["p4"] = pipeline(h4, S4, 4)
calls["p8"] = pipeline(h8, S2, 2)
calls["s16"] = lambda: s.trace_ao_sum(h16, None, False, TAU, BIAS)
calls["s64"] = lambda: s.trace_ao_sum(h64, None, False, TAU, BIAS)
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
pairs = [(f"sp n={n}", f"ao n={n}") for n in SIZES] + [("p4", "s16"), ("p4", "s64"), ("p8", "s16"), ("p8", "s64")]
for mode in ("lone", "queued"):
    for a, b in pairs:
        ratios[f"{a} / {b} {mode}"] = round(med[f"{a} {mode}"] / med[f"{b} {mode}"], 3)
        ratio_rounds[f"{a} / {b} {mode}"] = [round(x / y, 3) for x, y in zip(res[f"{a} {mode}"], res[f"{b} {mode}"])]
floor_ms = FILTER_BYTES / HBM_ACHIEVABLE * 1e3
summary = {
    "device": torch.cuda.get_device_name(0), "build": sf.build_info()["source_sha256"],
    "clock_mhz_live_median": float(np.median(clocks)) if len(clocks) else None,
    "n": N, "reps": REPS, "size": [W, H], "K": K, "tau": TAU, "bias": BIAS,
    "ms_median": {k: round(v, 4) for k, v in med.items()}, "spread_of_median": spread, "ratio": ratios,
    "ratio_per_round": ratio_rounds,
    "rounds_ms": {k: [round(x, 4) for x in v] for k, v in res.items()},
    "filter_bytes": FILTER_BYTES, "filter_floor_ms_at_6.29_TBps": round(floor_ms, 4),
    "filter_floor_over_time_queued": round(floor_ms / med["f4 queued"], 3),
    "rms_error_against_unspun_n64": {k: round(v, 4) for k, v in quality.items()},
    "surface_pixels": int(surf.sum()), "bits_checked": True,
    "overflow_tiles_after_setup": overflow_setup, "overflow_tiles": int(s.stats().overflow_tiles),
}
print(json.dumps(summary))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
s.close()
