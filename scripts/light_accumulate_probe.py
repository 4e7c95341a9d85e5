#!/usr/bin/env python3
"""Cost and quality of accumulating the light buffer over frames (sf_light_accumulate_to, sf_light_accumulate), one
process, one GPU, at 1920 x 1080, K = 0.25, tau = 4, bias 2^-10, on the bench's moving camera (bench.py: the config
camera with its yaw swept 1 mrad per frame; frames 0..15 of that path, the last one the frame measured):
  a_to   light_accumulate into a caller's buffer, frame 15 against frame 14's images   the kernel alone, against its
                                                         compulsory traffic (7 float4 per pixel, 112 B) at the
                                                         achievable 6.29 TB/s, and against light_filter(4)
  a_ctx  light_accumulate(), the context form            the kernel and its four copies; the view alternates between
                                                         frames 14 and 15 so that every call reprojects
  f4     light_filter(4) into a caller's buffer          the yardstick, measured again in this process
  p4     trace_ao_sum(h4, spin=ao_spins(4, phase)) + light_filter(4)                     last pull request's recipe
  p4a    trace_ao_sum(h4, spin=ao_spins(4, phase)) + light_accumulate() + light_filter(4)   this one's
  r      Render() of the frame itself, for scale
each queued back to back on the context's stream (and lone, synchronised each time). The bits are checked first: the
`_to` form of frame 1 against frame 0 equals lights.light_accumulate_model, and so does the context form's second
frame. Then 16 frames of the recipe: the RMS error of the open fraction against the unspun n = 64 sum at the last
frame, with and without accumulation, unfiltered and filtered, and the share of surface pixels that kept their history
at the last frame. After a 300 ms settle under load the cases run interleaved, REPS rounds; medians, the spread between
rounds and the build are printed, the last line as JSON.
Usage: light_accumulate_probe.py [N=20] [REPS=5] [JSON path]"""
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
FRAMES = 16
HBM_ACHIEVABLE = 6.29e12    # bytes / s, a float4 copy on this part
TO_BYTES = W * H * 112      # six float4 read, one written
COPY_BYTES = W * H * 32     # one float4 image read and written


def camera(frame):
    """Frame `frame` of bench.py's camera path: the config camera, yaw offset by a triangle wave of 1 mrad a frame."""
    cam = sf.config_camera(W, H, K)
    cam.SetYaw(np.float32(sf.DEFAULT_YAW + 1e-3 * (abs((frame + 10) % 40 - 20) - 10)))
    return cam


cams = [camera(k) for k in range(FRAMES)]
views = [tuple(np.asarray(v, np.float32) for v in c.corners()) for c in cams]
h4, h64 = lights.ao_samples(4), lights.ao_samples(64)
spin = lambda k: lights.ao_spins(4, lights.ao_phase(k))
same = lambda a, b: np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))
surface = lambda pos: ~((pos[..., 0] == 0) & (pos[..., 1] == 0) & (pos[..., 2] == 0))
s = sf.Sphereflake(W, H)

# the recipe over 16 frames, the bits of the first two checked against the model on the way
frames = []
for k in range(FRAMES):
    s.SetCamera(cams[k])
    s.Render()
    s.trace_ao_sum(h4, None, False, TAU, BIAS, spin=spin(k))
    if k < 2 or k >= FRAMES - 2:
        pos, nrm, _, _ = s.download()
        new = s.download_light()
    s.light_accumulate()
    if k < 2 or k >= FRAMES - 2:
        frames.append((k, pos, nrm, new, s.download_light()))
zero = np.zeros_like(frames[0][3])
want, _, _ = lights.light_accumulate_model(frames[0][3], frames[0][1], frames[0][2], views[0][0], zero, zero, zero, views[0])
assert same(frames[0][4], want), "the context form's first frame differs from the model"
want, acc1, _ = lights.light_accumulate_model(frames[1][3], frames[1][1], frames[1][2], views[1][0], frames[0][4],
                                              frames[0][1], frames[0][2], views[0])
assert same(frames[1][4], want), "the context form's second frame differs from the model"
got = s.light_accumulate(pos=frames[1][1], nrm=frames[1][2], buf=frames[1][3], hist_pos=frames[0][1],
                         hist_nrm=frames[0][2], hist=frames[0][4], hist_view=views[0], origin=views[1][0])
assert same(got, want), "light_accumulate_to differs from the model"
_, pos, nrm, single, accumulated = frames[-1]
surf = surface(pos)
kept = float(((accumulated[..., 3] >= 2) & surf).sum()) / float(surf.sum())
s.light_filter(4)
accumulated_f = s.download_light()
s.trace_ao_sum(h4, None, False, TAU, BIAS, spin=spin(FRAMES - 1))
s.light_filter(4)
single_f = s.download_light()
s.trace_ao_sum(h64, None, False, TAU, BIAS)
truth = s.download_light()
frac = lambda b: b[..., 0].astype(np.float64)
rms = lambda b: float(np.sqrt(np.mean((frac(b) - frac(truth))[surf] ** 2)))
quality = {"one frame, n=4 spun": rms(single), "one frame, then filter(4)": rms(single_f),
           "16 frames accumulated": rms(accumulated), "16 frames accumulated, then filter(4)": rms(accumulated_f)}
for k, v in quality.items():
    print(f"RMS error against unspun n = 64  {k:40s}: {v:.4f}")
print(f"surface pixels that kept their history at frame 15: {kept:.4f} (at frame 1: {acc1.sum() / surface(frames[1][1]).sum():.4f})")

# the timed cases
dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
_, hpos, hnrm, _, hbuf = frames[-2]
t_pos, t_nrm, t_new, t_hpos, t_hnrm, t_hist = (dev(a) for a in (pos, nrm, single, hpos, hnrm, hbuf))
tmp = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
torch.cuda.synchronize()
s.Synchronize()
flip = [0]


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


def a_to():
    s.light_accumulate(pos=t_pos, nrm=t_nrm, buf=t_new, hist_pos=t_hpos, hist_nrm=t_hnrm, hist=t_hist,
                       hist_view=views[-2], out=tmp, origin=views[-1][0])


def a_ctx():
    flip[0] ^= 1
    s.SetCamera(cams[FRAMES - 1 - flip[0]])
    s.light_accumulate()


def p4():
    s.trace_ao_sum(h4, None, False, TAU, BIAS, spin=spin(FRAMES - 1))
    s.light_filter(4)


def p4a():
    s.trace_ao_sum(h4, None, False, TAU, BIAS, spin=spin(FRAMES - 1))
    a_ctx()
    s.light_filter(4)


s.SetCamera(cams[-1])
s.Render()
calls = {"r render": lambda: s.Render(), "a_to": a_to, "a_ctx": a_ctx, "f4": lambda: s.light_filter(4, out=tmp),
         "p4": p4, "p4a": p4a}
cases = {}
for name, call in calls.items():
    for mode, how in (("lone", lone), ("queued", queued)):
        cases[f"{name} {mode}"] = (lambda call=call, how=how: how(call))
t0 = time.perf_counter()
while time.perf_counter() - t0 < 0.3:   # clock settle under load
    queued(lambda: s.Render())
res = {k: [] for k in cases}
for _ in range(REPS):
    for k, f in cases.items():
        res[k].append(f())
med = {k: float(np.median(v)) for k, v in res.items()}
for k, v in res.items():
    print(f"{k:24s}: ms {np.round(v, 4)} median {med[k]:.4f}")
floor_ms = TO_BYTES / HBM_ACHIEVABLE * 1e3
copies_ms = med["a_ctx queued"] - med["a_to queued"]
summary = {
    "device": torch.cuda.get_device_name(0), "build": sf.build_info()["source_sha256"],
    "n": N, "reps": REPS, "size": [W, H], "K": K, "tau": TAU, "bias": BIAS, "frames": FRAMES,
    "ms_median": {k: round(v, 4) for k, v in med.items()},
    "spread_of_median": {k: round((max(v) - min(v)) / med[k], 3) for k, v in res.items()},
    "rounds_ms": {k: [round(x, 4) for x in v] for k, v in res.items()},
    "to_bytes": TO_BYTES, "to_floor_ms_at_6.29_TBps": round(floor_ms, 4),
    "to_floor_over_time_queued": round(floor_ms / med["a_to queued"], 3),
    "to_over_filter_queued": round(med["a_to queued"] / med["f4 queued"], 3),
    "ctx_minus_to_ms_queued": round(copies_ms, 4),
    "four_copies_floor_ms_at_6.29_TBps": round(4 * COPY_BYTES / HBM_ACHIEVABLE * 1e3, 4),
    "copies_share_of_ctx_queued": round(copies_ms / med["a_ctx queued"], 3),
    "p4a_over_p4_queued": round(med["p4a queued"] / med["p4 queued"], 3),
    "rms_error_against_unspun_n64": {k: round(v, 4) for k, v in quality.items()},
    "kept_history_share_last_frame": round(kept, 4), "surface_pixels": int(surf.sum()), "bits_checked": True,
    "overflow_tiles": int(s.stats().overflow_tiles),
}
print(json.dumps(summary))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(summary, f, indent=1)
        f.write("\n")
s.close()
