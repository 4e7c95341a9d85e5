#!/usr/bin/env python3
"""Cost of tracing rays from caller-supplied origins (sf_trace_rays_to), one process, one GPU:
  a  trace_dirs of the 1080p K = 0.25 view's own pixel directions (dirs.pinhole) -- the yardstick; a12: the same
     with max_depth = 12, the levels trace_rays provisions by default (trace_dirs takes the view's geometric bound)
  b  trace_rays of the same rays with one origin for all of them (the same traversal; checked: the same bits)
  c  b with every group on the mixed-origin path (SF_FLAGS = SF_FLAG_FORCE_MIXED on a second context; the same bits)
  d  trace_rays of the mirror reflections off that frame (rays.reflect): one origin per ray, incoherent, deeper than
     the default 12 levels (most groups are re-traced); d20: the same with max_depth = 20 (no re-trace)
  e  a batch of 64 cameras along the config camera's path (K = 0.2 .. 0.6), a 240 x 135 image each, as one list;
     e0: what it replaces -- SetView + trace_dirs per camera, 64 launches on one context
each lone (synchronised each time) and queued back to back. After a 300 ms settle under load the cases run
interleaved, REPS rounds; medians, the spread between rounds, ratios, the live shader clock and the build are printed,
the last line as JSON.
Usage: rays_probe.py [N=50] [REPS=5]"""
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "sphereflake-raytracer_amd"))
import sphereflake_amd as sf  # noqa: E402
from sphereflake_amd import dirs, rays  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 50
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
W, H, K = 1920, 1080, 0.25
CW, CH, CAMS = 240, 135, 64
FORCE_MIXED = 0x8000

cam = sf.config_camera(W, H, K)
o, tl, tr, bl = cam.corners()
s = sf.Sphereflake(W, H)
s.SetCamera(cam)
old = os.environ.get("SF_FLAGS")
os.environ["SF_FLAGS"] = hex(FORCE_MIXED)   # (read when a context is created)
sm = sf.Sphereflake(W, H)
sm.SetCamera(cam)
if old is None:
    del os.environ["SF_FLAGS"]
else:
    os.environ["SF_FLAGS"] = old


def outputs(n):
    return (torch.empty((n, 4), dtype=torch.float32, device="cuda"), torch.empty((n, 4), dtype=torch.float32, device="cuda"),
            torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda"))


def bits(ts):
    return [t.cpu().numpy().reshape(-1).view(np.uint32) for t in ts]


pin_h = dirs.pinhole(o, tl, tr, bl, W, H)
pin = torch.from_numpy(pin_h).cuda()
org1 = torch.from_numpy(np.asarray(o, np.float32).reshape(1, 3)).cuda()
out_a, out_b, out_c = outputs(W * H), outputs(W * H), outputs(W * H)
torch.cuda.synchronize()
s.trace_dirs(pin, out=out_a)
s.trace_rays(org1, pin, rays_per_origin=W * H, out=out_b)
sm.trace_rays(org1, pin, rays_per_origin=W * H, out=out_c)
s.Synchronize()
sm.Synchronize()
same_b = all(np.array_equal(x, y) for x, y in zip(bits(out_a), bits(out_b)))
same_c = all(np.array_equal(x, y) for x, y in zip(bits(out_a), bits(out_c)))
assert same_b, "trace_rays (one origin) differs from trace_dirs"
assert same_c, "trace_rays (forced mixed) differs from trace_dirs"

# d: reflections off the frame
ro, rd, mask = rays.reflect(out_a[0].cpu().numpy().reshape(H, W, 4), out_a[1].cpu().numpy().reshape(H, W, 4), o, pin_h)
n_d = ro.shape[0]
ro_t, rd_t = torch.from_numpy(ro).cuda(), torch.from_numpy(rd).cuda()
out_d = outputs(n_d)

# e: the camera batch
co, cd, views = [], [], []
for k in np.linspace(0.2, 0.6, CAMS):
    c = sf.config_camera(CW, CH, float(k))
    oo, a, b, cc = c.corners()
    co.append(oo)
    views.append((oo, a, b, cc))
    cd.append(dirs.pinhole(oo, a, b, cc, CW, CH).reshape(-1, 3))
co_t = torch.from_numpy(np.ascontiguousarray(np.stack(co), np.float32)).cuda()
cd_t = torch.from_numpy(np.ascontiguousarray(np.concatenate(cd))).cuda()
n_e = CAMS * CW * CH
out_e = outputs(n_e)
s2 = sf.Sphereflake(CW, CH)
per = CW * CH
cam_dirs = [cd_t[k * per:(k + 1) * per] for k in range(CAMS)]
cam_outs = [tuple(t[k * per:(k + 1) * per] for t in out_e) for k in range(CAMS)]


def one_by_one():
    for k in range(CAMS):
        s2.SetView(*views[k])
        s2.trace_dirs(cam_dirs[k], out=cam_outs[k])


torch.cuda.synchronize()


def lone(call, ctx):
    ts = []
    for _ in range(N):
        t = time.perf_counter()
        call()
        ctx.Synchronize()
        ts.append(time.perf_counter() - t)
    return float(np.median(ts)) * 1e3


def queued(call, ctx):
    call()
    ctx.Synchronize()
    t = time.perf_counter()
    for _ in range(N):
        call()
    ctx.Synchronize()
    return (time.perf_counter() - t) / N * 1e3


calls = {
    "a dirs pinhole": (lambda: s.trace_dirs(pin, out=out_a), s),
    "a12 dirs pinhole 12 levels": (lambda: s.trace_dirs(pin, out=out_a, max_depth=12), s),
    "b rays one origin": (lambda: s.trace_rays(org1, pin, rays_per_origin=W * H, out=out_b), s),
    "c rays forced mixed": (lambda: sm.trace_rays(org1, pin, rays_per_origin=W * H, out=out_c), sm),
    "d rays reflect": (lambda: s.trace_rays(ro_t, rd_t, out=out_d), s),
    "d20 rays reflect 20 levels": (lambda: s.trace_rays(ro_t, rd_t, out=out_d, max_depth=20), s),
    "e rays 64 cameras": (lambda: s.trace_rays(co_t, cd_t, rays_per_origin=CW * CH, out=out_e), s),
    "e0 dirs 64 x SetView": (one_by_one, s2),
}
cases = {}
for name, (call, ctx) in calls.items():
    cases[name + " lone"] = (lambda call=call, ctx=ctx: lone(call, ctx))
    cases[name + " queued"] = (lambda call=call, ctx=ctx: queued(call, ctx))
t0 = time.perf_counter()
while time.perf_counter() - t0 < 0.3:   # clock settle under load
    queued(lambda: s.Render(), s)
s.reset_stats()
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
    print(f"{k:28s}: ms {np.round(v, 4)} median {med[k]:.4f}")
spread = {k: round((max(v) - min(v)) / med[k], 3) for k, v in res.items()}
ratio = lambda x, y: round(med[x] / med[y], 3)
summary = {
    "device": torch.cuda.get_device_name(0), "build": sf.build_info()["source_sha256"],
    "clock_mhz_live_median": float(np.median(clocks)) if len(clocks) else None,
    "n": N, "reps": REPS, "ms_median": {k: round(v, 4) for k, v in med.items()}, "spread_of_median": spread,
    "rays": {"a": W * H, "b": W * H, "c": W * H, "d": n_d, "e": n_e},
    "ratio": {
        "b / a lone": ratio("b rays one origin lone", "a dirs pinhole lone"),
        "b / a queued": ratio("b rays one origin queued", "a dirs pinhole queued"),
        "b / a12 lone": ratio("b rays one origin lone", "a12 dirs pinhole 12 levels lone"),
        "b / a12 queued": ratio("b rays one origin queued", "a12 dirs pinhole 12 levels queued"),
        "c / b lone": ratio("c rays forced mixed lone", "b rays one origin lone"),
        "c / b queued": ratio("c rays forced mixed queued", "b rays one origin queued"),
        "d / c queued, per ray": round(med["d rays reflect queued"] / med["c rays forced mixed queued"] * (W * H) / n_d, 3),
        "d20 / d queued": ratio("d20 rays reflect 20 levels queued", "d rays reflect queued"),
        "e / e0 lone": ratio("e rays 64 cameras lone", "e0 dirs 64 x SetView lone"),
        "e / e0 queued": ratio("e rays 64 cameras queued", "e0 dirs 64 x SetView queued"),
    },
    "reflect": {"hits": int((out_d[2] < sf.FLT_MAX).sum().item())},
    "overflow_groups": int(s.stats().overflow_tiles), "max_depth": int(s.stats().max_depth),
    "one_origin_equals_trace_dirs": bool(same_b), "forced_mixed_equals_trace_dirs": bool(same_c),
}
print(json.dumps(summary))
s2.close()
sm.close()
s.close()
