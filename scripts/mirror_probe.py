#!/usr/bin/env python3
"""Cost and quality of the sky-reflection traces (sf_trace_mirror, sf_trace_mirror_sum), one process, one GPU, at
1920 x 1080, K = 0.25 (the bench's camera), tau = 4, bias 2^-10, on the frame's own G-buffer (scripts/ao_spin_probe.py's
camera, rounds and settle):
  ao    trace_ao(ao_samples(n))                               n = 1, 4, 16
  mi    trace_mirror(lobe_samples(n, 8))                      the same n: a ray about the mirror axis against one about N
  aosp, misp   the same two with spin=ao_spins(4)
  ms    trace_mirror_sum(lobe_samples(n, 8), gradient)        the summing call against the mask call
  r     Render() of the frame itself, for scale
each queued back to back on the context's stream (and lone, synchronised each time). The bits are checked first: the
mask equals trace_ao on lights.mirror_axes' image (spun and unspun), and the sum equals lights.mirror_sum_model over
that mask. Then, per lobe exponent (8 and 64), the RMS error of the red channel (colours 1 / n, the gradient) against
the unspun n = 64 sum over the surface pixels: 4 rays spun 4 x 4 and filtered, 4 plain and filtered, 4 plain, 8 plain,
and the n = 64 answer filtered against itself. After a 300 ms settle under load the cases run interleaved, REPS rounds;
medians, the spread between rounds, ratios, the live shader clock and the build are printed, the last line as JSON.
Usage: mirror_probe.py [N=20] [REPS=5] [JSON path]"""
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
SIZES = (1, 4, 16)
SKY = dict(zenith=(0.25, 0.45, 1.0), horizon=(1.0, 0.8, 0.6), up=(0.0, 0.0, 1.0))

cam = sf.config_camera(W, H, K)
s = sf.Sphereflake(W, H)
s.SetCamera(cam)
s.Render()
s.PostProcess()
pos, nrm, _, _ = s.download()
surf = ~((pos[..., 0] == 0) & (pos[..., 1] == 0) & (pos[..., 2] == 0))
origin = np.asarray(cam.GetPosition(), np.float32)
S4 = lights.ao_spins(4)
same = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
even = lambda n: np.full((n, 3), np.float32(1.0) / np.float32(n), np.float32)

# the bits first
axes = lights.mirror_axes(pos, nrm)
pt = torch.from_numpy(np.ascontiguousarray(pos)).cuda()
at = torch.from_numpy(np.ascontiguousarray(axes)).cuda()
out = torch.zeros((H, W), dtype=torch.int64, device="cuda")
l4 = lights.lobe_samples(4, 8)
masks = {}
for key, spin in (("unspun", None), ("spun", S4)):
    s.trace_mirror(l4, TAU, BIAS, spin=spin)
    masks[key] = s.download_shadow_masks()
    s.trace_ao(l4, TAU, BIAS, pos=pt, nrm=at, out=out, spin=spin)
    s.Synchronize()
    assert np.array_equal(masks[key], out.cpu().numpy().view(np.uint64)), f"{key}: trace_mirror differs from trace_ao on the axes"
    s.trace_mirror_sum(l4, None, distance=TAU, bias=BIAS, spin=spin, **SKY)
    want = lights.mirror_sum_model(None, pos, nrm, origin, masks[key], l4, even(4), spin=spin, **SKY)
    assert same(s.download_light(), want), f"{key}: the sum differs from mirror_sum_model"
open_share = float(np.mean([((masks["unspun"][surf] >> np.uint64(i)) & np.uint64(1)).mean() for i in range(4)]))
del pt, at, out


def summed(samples, spin=None, size=0):
    s.trace_mirror_sum(samples, None, distance=TAU, bias=BIAS, spin=spin, **SKY)
    if size:
        s.light_filter(size)
    return s.download_light()


red = lambda b: b[..., 0].astype(np.float64)
quality = {}
for e in (8, 64):
    truth = summed(lights.lobe_samples(64, e))
    rms = lambda b: float(np.sqrt(np.mean((red(b) - red(truth))[surf] ** 2)))
    h4, h8 = lights.lobe_samples(4, e), lights.lobe_samples(8, e)
    quality[f"exponent {e}"] = {
        "4 spun + filtered": rms(summed(h4, S4, 4)), "4 plain + filtered": rms(summed(h4, None, 4)),
        "4 plain, unfiltered": rms(summed(h4)), "8 plain": rms(summed(h8)),
        "16 plain": rms(summed(lights.lobe_samples(16, e))),
        "64 filtered against itself": rms(summed(lights.lobe_samples(64, e), None, 4)),
    }
    for k, v in quality[f"exponent {e}"].items():
        print(f"RMS error against unspun n = 64, exponent {e:2d}  {k:28s}: {v:.4f}")
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


calls = {"r render": lambda: s.Render()}
for n in SIZES:
    ha, hl = lights.ao_samples(n), lights.lobe_samples(n, 8)
    calls[f"ao n={n}"] = lambda ha=ha: s.trace_ao(ha, TAU, BIAS)
    calls[f"mi n={n}"] = lambda hl=hl: s.trace_mirror(hl, TAU, BIAS)
    calls[f"aosp n={n}"] = lambda ha=ha: s.trace_ao(ha, TAU, BIAS, spin=S4)
    calls[f"misp n={n}"] = lambda hl=hl: s.trace_mirror(hl, TAU, BIAS, spin=S4)
    calls[f"ms n={n}"] = lambda hl=hl: s.trace_mirror_sum(hl, None, distance=TAU, bias=BIAS, **SKY)
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
pairs = [p for n in SIZES for p in ((f"mi n={n}", f"ao n={n}"), (f"misp n={n}", f"aosp n={n}"), (f"misp n={n}", f"mi n={n}"),
                                    (f"ms n={n}", f"mi n={n}"))]
for mode in ("lone", "queued"):
    for a, b in pairs:
        ratios[f"{a} / {b} {mode}"] = round(med[f"{a} {mode}"] / med[f"{b} {mode}"], 3)
        ratio_rounds[f"{a} / {b} {mode}"] = [round(x / y, 3) for x, y in zip(res[f"{a} {mode}"], res[f"{b} {mode}"])]
summary = {
    "device": torch.cuda.get_device_name(0), "build": sf.build_info()["source_sha256"],
    "clock_mhz_live_median": float(np.median(clocks)) if len(clocks) else None,
    "n": N, "reps": REPS, "size": [W, H], "K": K, "tau": TAU, "bias": BIAS,
    "ms_median": {k: round(v, 4) for k, v in med.items()}, "spread_of_median": spread, "ratio": ratios,
    "ratio_per_round": ratio_rounds,
    "rounds_ms": {k: [round(x, 4) for x in v] for k, v in res.items()},
    "rms_error_against_unspun_n64": {e: {k: round(v, 4) for k, v in q.items()} for e, q in quality.items()},
    "open_share_of_lobe4_bits": round(open_share, 4),
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
