"""The inputs of the light traces' sweep over random views (tests/test_light_sweep_host.py on the CPU,
tests/test_gpu_light_sweep.py on the GPU), built once per (seed, variant) and shared, read-only.

Views: sweepviews.sweep_view(seed), seeds 0..63 -- the frames the render sweep proves equal to the oracle, 8 x 8 to
136 x 72 with the ragged sizes among them -- and the position and normal images of sweepviews.sweep_reference(seed,
variant) ("avx": LOD 70, "sse": LOD 60), the oracle's own.

Entries per view, sweep_entries(seed), from np.random.default_rng(11000 + seed), drawn in this order (float64, rounded
to float32 at the end):
  direction 0      normalize(o / |o| + 0.5 N(0, 1)^3), o the view's origin: roughly from the flake towards the camera,
                   so something is lit;
  directions 1..3  |N(0, 1)^3| + 0.05 with the signs of octant (3 seed + i) mod 8 -- bit k set: component k is
                   negative --, normalised: over the 64 seeds every octant gets 24 of the 192 forced directions;
  radii            uniform(2.5, 8.0, 4);
  the inside light normalize(N(0, 1)^3) uniform(0.2, 1.9): inside the flake's radius-2 ball, where the LOD
                   predicate's t < 0 arm is reached.
Point lights: dirs[i] radii[i] for i = 0..3, then the inside light as entry 4 (n = 5). Suns: lights.sun_direction(dirs[i])
(n = 4) at tau = 4. AO: lights.ao_samples(4) at tau = 4, once without a spin and once under lights.ao_spins(3), whose
period is no divisor of the 8-pixel tile. Shafts: the sun is direction 0, fractions lights.shaft_fractions(4), `dirs` the
view's pinhole directions divided by their float32 length, far = float32(|o| + 2), so the frame's misses are marched,
and tau = lights.shaft_distance(o, lights.shaft_ends(pos, dirs, far)).

Oracle masks: sweep_rays(seed, variant) traces, with the oracle's batch entry (pyoracle.trace_rays), the ray of every
entry at EVERY surface pixel -- for the shafts at every sample that is not (0, 0, 0), the marched misses included --
from the origins and directions that lights.shadow_model, sun_model, ao_model and shafts_model state on the host. The
oracle's min_t does not depend on the bias: it is computed once per case and oracle_mask() compares it with the
model's bound for either bias (0 and 2^-10). Each trace keeps its deepest node depth, anywhere along its rays, and
the deepest one a lit ray needs before its bound (deepest_needed: the overflow leg's two conditions).

The oracle's cost, measured on the CPU (x86-64, 8 hardware threads): pyoracle.trace_rays traces AO rays of seed 54 at
0.24 M rays / s on one thread (4.2 us per ray) and 1.2 M rays / s on eight, against the 4000 rays / s (0.25 ms per ray)
of dirscheck.oracle_rays. Seed 54, the largest case (136 x 72, 9208 surface pixels with 21 rays each and 4 per marched
miss: 195 704 rays), takes 1.1 CPU seconds, 0.4 s of wall time, per variant; all 128 cases take 13 CPU seconds, 6 s of
wall time. Under 3 s per case, so the cases are not split by trace kind. On the GPU side a case makes about 70 calls on
host arrays; measured on an MI355X (pytest --durations), the slowest case takes 0.34 s of wall time, the oracle's part
included (the first case of the run; seeds 4 and 54 follow with 0.19 s and 0.16 s), and the 128 cases 11 s."""
import functools

import numpy as np

from sphereflake_amd import dirs as sfdirs
from sphereflake_amd import lights
from maskcheck import bit, low, surface_of  # noqa: F401
from oracle import pyoracle
from sweepviews import LOD, SEEDS, sweep_reference, sweep_view  # noqa: F401

F = np.float32
FLT_MAX = F(np.finfo(np.float32).max)
TAU = 4.0
B10 = 2.0 ** -10
BIASES = (0.0, B10)
VARIANTS = ("avx", "sse")
TRACES = ("shadows", "suns", "ao", "ao_spin", "shafts")
COUNT = {"shadows": 5, "suns": 4, "ao": 4, "ao_spin": 4, "shafts": 4}
H4 = lights.ao_samples(4)
S3 = lights.ao_spins(3)
FRACTIONS = lights.shaft_fractions(4)
for _a in (H4, S3, FRACTIONS):
    _a.setflags(write=False)


def octant_of(v):
    """The sign octant of a vector: bit k set where component k is negative."""
    v = np.asarray(v).reshape(3)
    return int(sum((1 << k) for k in range(3) if np.signbit(v[k])))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def sweep_entries(seed):
    """The entries of view `seed`: dict of dirs [4, 3], radii [4], inside [3], lights [5, 3], suns [4, 3] (float32,
    read-only) and octants (the octants forced on directions 1..3)."""
    o = np.asarray(sweep_view(seed)[0][0], np.float64)
    rng = np.random.default_rng(11000 + seed)
    d = np.empty((4, 3), np.float64)
    d[0] = o / np.linalg.norm(o) + 0.5 * rng.normal(size=3)
    octants = []
    for i in (1, 2, 3):
        oc = (3 * seed + i) % 8
        v = np.abs(rng.normal(size=3)) + 0.05
        d[i] = np.where([(oc >> k) & 1 for k in range(3)], -v, v)
        octants.append(oc)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    radii = rng.uniform(2.5, 8.0, 4)
    v = rng.normal(size=3)
    inside = v / np.linalg.norm(v) * rng.uniform(0.2, 1.9)
    pts = np.concatenate([d * radii[:, None], inside[None, :]]).astype(F)
    suns = np.stack([lights.sun_direction(d[i]) for i in range(4)])
    d32, r32, in32 = d.astype(F), radii.astype(F), inside.astype(F)
    _frozen(d32, r32, in32, pts, suns)
    return {"dirs": d32, "radii": r32, "inside": in32, "lights": pts, "suns": suns, "octants": tuple(octants)}


@functools.lru_cache(maxsize=None)
def shaft_inputs(seed, variant="avx"):
    """(dirs [H, W, 3], far, tau) of the view's shafts trace (the march ends, and so tau, depend on the frame)."""
    (o, tl, tr, bl), _, _, (W, H) = sweep_view(seed)
    d = np.asarray(sfdirs.pinhole(o, tl, tr, bl, W, H), F)
    u = (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(F)
    far = F(np.linalg.norm(np.asarray(o, np.float64)) + 2.0)
    tau = lights.shaft_distance(o, lights.shaft_ends(sweep_reference(seed, variant)["pos4"], u, far))
    u.setflags(write=False)
    return u, far, tau


def model(seed, variant, trace, bias):
    """(F, d, bound, on) of the host model for the case's trace: the rays' origins F [n, H, W, 3] (shadows: [n, 3],
    the lights), unnormalised directions d [n, H, W, 3], bounds [n, H, W] and the pixels that have a ray [n, H, W]."""
    o = sweep_view(seed)[0][0]
    ref = sweep_reference(seed, variant)
    pos, nrm = ref["pos4"], ref["nrm4"]
    e = sweep_entries(seed)
    if trace == "shadows":
        parts = [lights.shadow_model(pos, o, l, bias) for l in e["lights"]]
        return e["lights"], np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]), \
            np.stack([p[2] for p in parts])
    if trace == "suns":
        Fo, d, bound, surf = lights.suns_model(pos, o, e["suns"], TAU, bias)
    elif trace in ("ao", "ao_spin"):
        Fo, d, bound, surf = lights.ao_model(pos, nrm, o, H4, TAU, bias, spin=S3 if trace == "ao_spin" else None)
    elif trace == "shafts":
        u, far, tau = shaft_inputs(seed, variant)
        return lights.shafts_model(pos, o, e["suns"][0], tau, bias, FRACTIONS, u, far)
    else:
        raise ValueError(trace)
    return Fo, d, bound, np.broadcast_to(surf, bound.shape)


@functools.lru_cache(maxsize=None)
def sweep_rays(seed, variant="avx"):
    """{trace: (min_t [n, H, W], deepest node, deepest needed node)} of the oracle for every ray of the case: FLT_MAX
    where there is no ray. min_t and the deepest node are independent of the bias. The deepest NEEDED node is the
    deepest one that a ray the oracle finds lit at bias 2^-10 expands with its bounding-sphere root under the ray's
    bound (pyoracle.trace_rays' near_depth): what an any-hit traversal must open, whatever it culls. Computed once,
    read-only."""
    children = sweep_view(seed)[1]["children"]
    out = {}
    for trace in TRACES:
        Fo, d, bound, on = model(seed, variant, trace, B10)   # (F and d do not depend on the bias)
        mint = np.full(on.shape, FLT_MAX, F)
        deepest, needed = 0, 0
        for i in range(on.shape[0]):
            if on[i].any():
                origins = Fo[i] if trace == "shadows" else Fo[i][on[i]]
                r = pyoracle.trace_rays(children, origins, d[i][on[i]], LOD[variant], bounds=bound[i][on[i]])
                mint[i][on[i]] = r["minT"]
                deepest = max(deepest, r["stats"]["max_depth"])
                with np.errstate(invalid="ignore"):
                    lit = ~(r["minT"] < bound[i][on[i]])
                if lit.any():
                    needed = max(needed, int(r["near_depth"][lit].max()))
        mint.setflags(write=False)
        out[trace] = (mint, deepest, needed)
    return out


@functools.lru_cache(maxsize=None)
def oracle_mask(seed, variant, trace, bias):
    """The oracle's mask words [H, W] uint64 of the case's trace at `bias`: bit i is 0 where entry i has a ray and the
    oracle's min_t is under the model's bound, else 1; bits n..63 are 0. Read-only."""
    mint = sweep_rays(seed, variant)[trace][0]
    _, _, bound, on = model(seed, variant, trace, bias)
    mask = np.zeros(on.shape[1:], np.uint64)
    with np.errstate(invalid="ignore"):
        for i in range(on.shape[0]):
            mask |= (~(on[i] & (mint[i] < bound[i]))).astype(np.uint64) << np.uint64(i)
    mask.setflags(write=False)
    return mask


def deepest(seed, variant, trace):
    """The deepest node any of the trace's oracle rays expands, anywhere along the ray."""
    return sweep_rays(seed, variant)[trace][1]


def deepest_needed(seed, variant, trace):
    """The deepest node a lit ray of the trace expands before its bound, at bias 2^-10 (sweep_rays)."""
    return sweep_rays(seed, variant)[trace][2]


def both_outcomes(mask, i, where, share=0.10):
    """Does bit i take either value on at least `share` of the pixels of `where`?"""
    total = int(where.sum())
    lit = int((where & bit(mask, i)).sum())
    return total > 0 and min(lit, total - lit) >= share * total


def entry_text(seed, variant, trace, i):
    """What entry i of the case's trace is, for a failure message: the light or direction and its sign octant."""
    e = sweep_entries(seed)
    if trace == "shadows":
        v = e["lights"][i]
        return f"light {i} {v.tolist()}" + (" (inside the ball)" if i == 4 else f" octant {octant_of(v)}")
    if trace == "suns":
        return f"sun {i} {e['suns'][i].tolist()} octant {octant_of(e['suns'][i])}"
    if trace == "shafts":
        return f"fraction {i} = {float(FRACTIONS[i])} under sun 0 {e['suns'][0].tolist()} octant {octant_of(e['suns'][0])}"
    return f"sample {i} {H4[i].tolist()}" + (" under ao_spins(3)" if trace == "ao_spin" else "")


def case_text(seed, variant):
    _, _, K, (W, H) = sweep_view(seed)
    return f"seed {seed} {variant} {W}x{H} K={K:.3f}"


def mask_difference(seed, variant, trace, bias, got, want):
    """'' if the two mask images are equal, else what a failure names: the case, the trace and the bias, the first
    differing pixel with its 8 x 8 tile, the differing bits with their entries and octants."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != np.uint64 or got.shape != want.shape:
        return f"{case_text(seed, variant)} {trace} bias {bias}: dtype / shape {got.dtype} {got.shape}"
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return ""
    y, x = (int(v) for v in bad[0])
    tiles_x = (got.shape[1] + 7) // 8
    g, w = int(got[y, x]), int(want[y, x])
    bits = [i for i in range(64) if ((g ^ w) >> i) & 1]
    named = "; ".join(f"bit {i}: {entry_text(seed, variant, trace, i) if i < COUNT[trace] else 'beyond n'}"
                      for i in bits[:6])
    return (f"{case_text(seed, variant)} {trace} bias {bias}: {len(bad)} pixels differ, the first at x {x} y {y}, tile "
            f"({x // 8}, {y // 8}) = {(y // 8) * tiles_x + x // 8}: got {g:#x} want {w:#x}; {named}")
