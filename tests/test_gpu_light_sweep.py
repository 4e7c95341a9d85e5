"""GPU sweep of the light traces over random views (tests/lightsweep.py: the 64 views of tests/sweepviews.py with five
point lights -- one inside the flake's ball --, four suns with forced sign octants, plain and spun AO and shafts per
view), in both reference variants: one case per (seed, variant), a fresh context with SetVariant and SetView, the
oracle's own position and normal images passed as pos= / nrm=. Every comparison covers the whole image and is bit
equality with the CPU oracle's masks, which cover every surface pixel and every marched miss
(tests/test_light_sweep_host.py shows that the inputs hold the cases; tests/test_oracle_batch_host.py that the batched
oracle is the per-ray one).

Leg A, the masks: trace_shadows (5 lights), trace_suns (4), trace_ao (4, plain), trace_ao(spin=ao_spins(3)) and
trace_shafts (4, with dirs and far), each at bias 0 and 2^-10: every word equals the oracle's, bits n..63 are 0, and a
miss of the frame has exactly its low n bits set unless the shafts march it. A view without a surface pixel comes out
all-lit with overflow_tiles unmoved.
Leg B, the hand-written n = 1 kernels: trace_shadow(lights[i]) and trace_sun(suns[i]) give 255 / 0 where the oracle's
mask has bit i set / clear, everywhere, at both biases.
Leg C, the sums: trace_shadows_sum, trace_suns_sum (the written-out copy of the entry loop) and trace_ao_sum plain and
spun with seeded random colours equal lights.sum_model / lights.ao_sum_model over the ORACLE's mask, bit for bit, as one
overwriting call and as an overwriting call with the first 2 entries followed by an accumulating call with the rest.
Leg D, overflow (AVX): for each trace whose deepest oracle node is >= 6 the same call with max_depth=4 gives the oracle's
words again; and where a ray that the oracle finds LIT expands a node of depth >= 6 BEFORE ITS BOUND
(lightsweep.deepest_needed), stats().overflow_tiles moves by at least 1: with 4 levels the kernels enter no child of a
depth-3 node (the rule sweepviews.OVERFLOW_LEVELS states for 5). The second condition is the first made sound for an
any-hit traversal: the oracle follows a ray through the whole flake, the kernels stop a lane at its first hit under the
bound and cull what lies wholly beyond the bound (sf_kernels.hip, occluded<ANYHIT>), so a deep node behind the surface
point, or on a stopped ray only, is one they need not open. Measured on the MI355X with the first condition alone: of
the 264 (seed, trace) pairs of depth >= 6 the counter stayed at 0 on 10 -- shafts of seeds 5, 38, 40, 50, 60, 61,
shadows of 27, 31, 57, suns of 39 --, all with the right words; their needed depths are 0..3, and the oracle puts 17 more
pairs under 6 (needed 0..5) whose counter moved all the same. 237 pairs on 56 views keep the counter's assertion.
Leg E, the context form: Render(), trace_suns(dirs) with pos=None, download_shadow_masks(): leg A's mask.

Left out, as tests/test_gpu_loop_sweep.py documents for the render sweep: SF_MAX_BLOCKS=1, the row-major schedule and 3
levels; no environment knob is set here.

A failure names the seed, variant, frame size and K, the trace and the bias, the first differing pixel with its 8 x 8
tile, and the differing bits with their entries and sign octants (lightsweep.mask_difference): the case replays on the
CPU through lightsweep.model / lights.*_model and pyoracle.trace_rays."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import sphereflake_amd as sf  # noqa: E402
from sphereflake_amd import lights  # noqa: E402
import lightsweep as ls  # noqa: E402
from lightsweep import B10, BIASES, COUNT, FRACTIONS, H4, S3, SEEDS, TAU, TRACES, sweep_entries, sweep_reference, sweep_view  # noqa: E402

F = np.float32
OVERFLOW_LEVELS = 4   # leg D's max_depth
DEEP = OVERFLOW_LEVELS + 2


@pytest.fixture(scope="module", autouse=True)
def device():
    sf.build()
    assert sf.device_count() >= 1, "no HIP device visible: GPU tests must run on an MI355X"


def mask_call(s, seed, variant, trace, bias, pos, nrm, **kw):
    """The mask trace of the case on host images."""
    e = sweep_entries(seed)
    if trace == "shadows":
        return s.trace_shadows(e["lights"], bias=bias, pos=pos, **kw)
    if trace == "suns":
        return s.trace_suns(e["suns"], TAU, bias=bias, pos=pos, **kw)
    if trace == "ao":
        return s.trace_ao(H4, TAU, bias, pos=pos, nrm=nrm, **kw)
    if trace == "ao_spin":
        return s.trace_ao(H4, TAU, bias, pos=pos, nrm=nrm, spin=S3, **kw)
    u, far, tau = ls.shaft_inputs(seed, variant)
    return s.trace_shafts(e["suns"][0], FRACTIONS, tau, bias, pos=pos, dirs=u, far=far, **kw)


def sum_difference(got, want, what):
    got = np.asarray(got)
    if got.dtype != np.float32 or got.shape != want.shape:
        return f"{what}: dtype / shape {got.dtype} {got.shape}"
    bad = np.argwhere((np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)).any(axis=-1))
    if bad.size == 0:
        return ""
    y, x = (int(v) for v in bad[0])
    return (f"{what}: {len(bad)} pixels differ, the first at x {x} y {y}, tile ({x // 8}, {y // 8}): got"
            f" {got[y, x].tolist()} want {want[y, x].tolist()}")


@pytest.mark.parametrize("variant", ls.VARIANTS)
@pytest.mark.parametrize("seed", SEEDS)
def test_light_sweep(seed, variant):
    view, _, _, (W, H) = sweep_view(seed)
    ref = sweep_reference(seed, variant)
    pos, nrm = ref["pos4"], ref["nrm4"]
    surf = ls.surface_of(pos)
    e = sweep_entries(seed)
    what = ls.case_text(seed, variant)
    colours = np.random.default_rng(12000 + seed).random((5, 3)).astype(F)
    with sf.Sphereflake(W, H) as s:
        s.SetVariant(variant)
        s.SetView(*view)

        # leg A: the masks against the oracle
        for trace in TRACES:
            n = COUNT[trace]
            for bias in BIASES:
                got = mask_call(s, seed, variant, trace, bias, pos, nrm)
                want = ls.oracle_mask(seed, variant, trace, bias)
                diff = ls.mask_difference(seed, variant, trace, bias, got, want)
                assert not diff, diff
                assert (got >> np.uint64(n) == 0).all(), f"{what} {trace} bias {bias}: a bit beyond n"
                marched = ls.model(seed, variant, trace, bias)[3].any(axis=0)
                assert (got[~surf & ~marched] == ls.low(n)).all(), f"{what} {trace} bias {bias}: a miss of the frame"
            if not surf.any() and trace != "shafts":
                assert (got == ls.low(n)).all() and s.stats().overflow_tiles == 0, f"{what} {trace}: no surface pixel"

        # leg B: the n = 1 kernels
        for bias in BIASES:
            for i in range(5):
                vis = s.trace_shadow(e["lights"][i], bias, pos=pos)
                want = np.where(ls.bit(ls.oracle_mask(seed, variant, "shadows", bias), i), 255, 0).astype(np.uint8)
                bad = np.argwhere(vis != want)
                assert vis.dtype == np.uint8 and bad.size == 0, \
                    f"{what} trace_shadow bias {bias} {ls.entry_text(seed, variant, 'shadows', i)}: {len(bad)} pixels" \
                    f" differ, the first (y, x) {bad[0].tolist()}, tile ({bad[0][1] // 8}, {bad[0][0] // 8})"
            for i in range(4):
                vis = s.trace_sun(e["suns"][i], TAU, bias, pos=pos)
                want = np.where(ls.bit(ls.oracle_mask(seed, variant, "suns", bias), i), 255, 0).astype(np.uint8)
                bad = np.argwhere(vis != want)
                assert vis.dtype == np.uint8 and bad.size == 0, \
                    f"{what} trace_sun bias {bias} {ls.entry_text(seed, variant, 'suns', i)}: {len(bad)} pixels" \
                    f" differ, the first (y, x) {bad[0].tolist()}, tile ({bad[0][1] // 8}, {bad[0][0] // 8})"

        # leg C: the sums over the oracle's masks, as one call and split 2 + the rest
        for bias in BIASES:
            masks = {t: ls.oracle_mask(seed, variant, t, bias) for t in TRACES}
            sums = (
                ("trace_shadows_sum", e["lights"], colours,
                 lambda pts, col, **kw: s.trace_shadows_sum(pts, col, bias=bias, pos=pos, nrm=nrm, **kw),
                 lights.sum_model(None, pos, nrm, [masks["shadows"]], e["lights"], colours, "shadows", view[0])),
                ("trace_suns_sum", e["suns"], colours[:4],
                 lambda pts, col, **kw: s.trace_suns_sum(pts, col, distance=TAU, bias=bias, pos=pos, nrm=nrm, **kw),
                 lights.sum_model(None, pos, nrm, [masks["suns"]], e["suns"], colours[:4], "suns")),
                ("trace_ao_sum", H4, colours[:4],
                 lambda pts, col, **kw: s.trace_ao_sum(pts, col, distance=TAU, bias=bias, pos=pos, nrm=nrm, **kw),
                 lights.ao_sum_model(None, pos, masks["ao"], colours[:4])),
                ("trace_ao_sum spun", H4, colours[:4],
                 lambda pts, col, **kw: s.trace_ao_sum(pts, col, distance=TAU, bias=bias, pos=pos, nrm=nrm, spin=S3, **kw),
                 lights.ao_sum_model(None, pos, masks["ao_spin"], colours[:4])),
            )
            for name, pts, col, call, want in sums:
                diff = sum_difference(call(pts, col), want, f"{what} {name} bias {bias}, one call")
                assert not diff, diff
                first = call(pts[:2], col[:2])
                both = call(pts[2:], col[2:], accumulate=True, out=first)
                diff = sum_difference(both, want, f"{what} {name} bias {bias}, 2 entries + the rest")
                assert not diff, diff

        # leg D: too few levels, the tiles re-traced
        if variant == "avx":
            for trace in TRACES:
                if ls.deepest(seed, variant, trace) < DEEP:
                    continue
                before = s.stats().overflow_tiles
                got = mask_call(s, seed, variant, trace, B10, pos, nrm, max_depth=OVERFLOW_LEVELS)
                moved = s.stats().overflow_tiles - before
                needed = ls.deepest_needed(seed, variant, trace)
                at = f"max_depth={OVERFLOW_LEVELS} (deepest oracle node {ls.deepest(seed, variant, trace)}, before a" \
                     f" lit ray's bound {needed})"
                diff = ls.mask_difference(seed, variant, trace, B10, got, ls.oracle_mask(seed, variant, trace, B10))
                assert not diff, f"{at}: {diff}"
                assert moved >= 1 or needed < DEEP, f"{what} {trace} {at}: overflow_tiles moved by {moved}"

        # leg E: the context's own G-buffer and mask buffer
        s.Render()
        assert s.trace_suns(e["suns"], TAU, bias=B10) is None
        got = s.download_shadow_masks()
        diff = ls.mask_difference(seed, variant, "suns", B10, got, ls.oracle_mask(seed, variant, "suns", B10))
        assert not diff, f"after Render(), pos=None: {diff}"
