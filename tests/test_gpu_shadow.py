"""Point-light shadows on the GPU (sf_trace_shadow_to / sf_trace_shadow / sf_light_image) against the CPU oracle:
the visibility byte of every pixel is bit-exact with tests/shadowcheck.py, which traces the light-side ray with the
reference's own arithmetic (oracle/) for the direction and bound of sphereflake_amd.lights.shadow_model."""
import ctypes

import numpy as np
import pytest

import sphereflake_amd as sf
from sphereflake_amd import lights
from conftest import load_frame
from dirscheck import same_bits
from oracle import pyoracle
from rayscheck import frame
from sfcheck import bad_rows, row_digests
import shadowcheck as sc

pytestmark = pytest.mark.gpu

BIASES = (0.0, 2.0 ** -11, 2.0 ** -7)
B9 = 2.0 ** -9
FIXUP_LOOP_COPIES = 40   # (t3 at 4 levels flags about 53 of a copy's 56.25 tiles: about 2130)


@pytest.fixture(scope="module", autouse=True)
def device():
    sf.build()
    assert sf.device_count() >= 1, "no HIP device visible: GPU tests must run on an MI355X"


def flake(name, variant="avx", size=None):
    S = pyoracle.load_setup(name)
    s = sf.Sphereflake(*(size or (S["W"], S["H"])))
    s.SetVariant(variant)
    s.SetView(S["origin"], S["tl"], S["tr"], S["bl"])
    return s


def light_of(light_name):
    return sc.INSIDE if light_name == "inside" else sc.LIGHTS[light_name]


def both_outcomes(vis, name):
    """A constant output cannot pass: at least 50 shadowed and 50 lit surface pixels."""
    surf = frame(name)["minT"] < np.finfo(np.float32).max
    assert int((vis == 0).sum()) >= 50 and int(((vis == 255) & surf).sum()) >= 50


# 1 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["avx", "sse"])
@pytest.mark.parametrize("name,light_name", sc.CASES)
def test_numpy_image_equals_the_oracle(name, light_name, variant):
    """The oracle's own frame, uploaded: every bias, both variants."""
    pos = frame(name, variant)["pos4"]
    with flake(name, variant) as s:
        for bias in BIASES:
            ref = sc.oracle_vis(name, light_name, bias, variant)
            if variant == "avx":
                both_outcomes(ref, name)
            got = s.trace_shadow(light_of(light_name), bias=bias, pos=pos)
            assert got.dtype == np.uint8 and got.shape == ref.shape
            bad = np.argwhere(got != ref)
            assert bad.size == 0, f"{name} {light_name} {variant} bias {bias}: {len(bad)} pixels differ, first {bad[:4]}"


@pytest.mark.parametrize("variant", ["avx", "sse"])
@pytest.mark.parametrize("name,light_name", sc.CASES)
def test_rendered_frame_equals_the_oracle(name, light_name, variant):
    """Render, trace_shadow() on the context's own G-buffer, download_shadow()."""
    with flake(name, variant) as s:
        s.Render()
        for bias in BIASES:
            assert s.trace_shadow(light_of(light_name), bias=bias) is None
            got = s.download_shadow()
            assert np.array_equal(got, sc.oracle_vis(name, light_name, bias, variant)), (name, light_name, bias)
        assert s.shadow_buffer() != 0


# 2 ---------------------------------------------------------------------------------------------------
def test_overflow_tiles_are_retraced():
    """max_depth = 4 provisions too few levels (the light-side traversals reach depth 6-7): same bits, and the
    re-trace counter moved."""
    pos = frame("t3")["pos4"]
    with flake("t3") as s:
        o0 = s.stats().overflow_tiles
        for light_name in ("side", "top"):
            got = s.trace_shadow(light_of(light_name), bias=B9, pos=pos, max_depth=4)
            assert np.array_equal(got, sc.oracle_vis("t3", light_name, B9)), light_name
        assert s.stats().overflow_tiles > o0


def test_more_flagged_tiles_than_fixup_blocks():
    """t3's position image stacked R times into one 80 x 45R image at max_depth = 4: more flagged tiles than the
    re-trace launch has blocks (1024 is the larger of the two fixup grids), so its blocks walk the list more than once.
    45 is no multiple of 8: the copies fall differently into tiles, the per-pixel bytes are the oracle's all the same."""
    R = FIXUP_LOOP_COPIES
    pos = np.concatenate([frame("t3")["pos4"]] * R)
    want = np.concatenate([sc.oracle_vis("t3", "side", B9)] * R)
    with flake("t3") as s:
        o0 = s.stats().overflow_tiles
        got = s.trace_shadow(light_of("side"), bias=B9, pos=pos, max_depth=4)
        moved = s.stats().overflow_tiles - o0
    print("flagged tiles", moved, "per copy", moved / R)
    assert moved > 1024
    assert np.array_equal(got, want)


# 3 ---------------------------------------------------------------------------------------------------
def test_partial_tiles():
    """A 13 x 11 crop (partial tiles in both directions, rows not 8-byte aligned) equals the crop of the whole."""
    import torch
    pos = frame("t3")["pos4"]
    ref = sc.oracle_vis("t3", "side", B9)
    y0, x0, h, w = 17, 30, 11, 13
    crop = np.ascontiguousarray(pos[y0:y0 + h, x0:x0 + w])
    with flake("t3") as s:
        got = s.trace_shadow(light_of("side"), bias=B9, pos=crop)
        assert np.array_equal(got, ref[y0:y0 + h, x0:x0 + w])
        # through device tensors, with a sentinel behind the last byte
        pt = torch.from_numpy(crop).cuda()
        out = torch.full((h * w + 64,), 0x5a, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        s.trace_shadow(light_of("side"), bias=B9, pos=pt, out=out)
        s.Synchronize()
        o = out.cpu().numpy()
        assert (o[h * w:] == 0x5a).all(), "wrote past the last pixel"
        assert np.array_equal(o[:h * w].reshape(h, w), ref[y0:y0 + h, x0:x0 + w])
    sub = ref[y0:y0 + h, x0:x0 + w]
    assert (sub == 0).any() and (sub == 255).any()


# 4 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,light_name", [("t3", "side"), ("t1", "low")])
def test_any_hit_equals_closest_hit(name, light_name):
    """trace_rays of the same d from the single origin `light`, then min_t < bound on the host: identical vis."""
    S = pyoracle.load_setup(name)
    pos = frame(name)["pos4"]
    light = np.asarray(light_of(light_name), np.float32)
    with flake(name) as s:
        for bias in (0.0, B9):
            d, bound, surf = lights.shadow_model(pos, S["origin"], light, bias)
            _, _, mint, _ = s.trace_rays(light.reshape(1, 3), d, rays_per_origin=d.shape[0] * d.shape[1])
            mint = mint.reshape(surf.shape)
            want = np.where(surf & (mint < bound), 0, 255).astype(np.uint8)
            got = s.trace_shadow(light, bias=bias, pos=pos)
            assert np.array_equal(got, want)
            assert np.array_equal(got, sc.oracle_vis(name, light_name, bias))


# 5 ---------------------------------------------------------------------------------------------------
def test_light_inside_the_ball_and_non_finite_light():
    fx = load_frame("t3")
    pos = frame("t3")["pos4"]
    with flake("t3") as s:
        got = s.trace_shadow(sc.INSIDE, bias=B9, pos=pos)
        assert np.array_equal(got, sc.oracle_vis("t3", "inside", B9))
        for light in ((np.nan, 0.0, 1.0), (np.inf, 0.0, 0.0), (0.0, -np.inf, 3.0)):
            got = s.trace_shadow(light, bias=B9, pos=pos)
            assert (got == 255).all(), light
        s.Render()
        p, n, _, _ = s.download()
        assert bad_rows(fx["row_digest_gbuf"], row_digests(p, n)) == []


# 6 ---------------------------------------------------------------------------------------------------
def test_callers_stream_between_renders_and_stats():
    """Render, shadows on a caller's torch stream, Render -- no host synchronisation in between; the statistics are
    what the renders alone leave, and the later render's bits are unchanged."""
    import torch
    S = pyoracle.load_setup("t3")
    W, H = S["W"], S["H"]
    ref = frame("t3")
    with flake("t3") as s:   # what two renders alone leave
        s.Render(emit_aux=True)
        s.Render(emit_aux=True)
        s.Synchronize()
        st0 = s.stats()
        want = (st0.max_depth, np.float32(st0.closest), st0.rays, st0.overflow_tiles)
    pt = torch.from_numpy(np.ascontiguousarray(ref["pos4"])).cuda()
    out = torch.full((H, W), 7, dtype=torch.uint8, device="cuda")
    ts = torch.cuda.Stream()
    torch.cuda.synchronize()
    with flake("t3") as s:
        s.Render(emit_aux=True)
        s.trace_shadow(sc.LIGHTS["side"], bias=B9, pos=pt, out=out, stream=ts.cuda_stream)
        s.trace_shadow(sc.LIGHTS["top"], bias=B9, stream=ts.cuda_stream)   # the context's frame, its own buffer
        s.Render(emit_aux=True)
        pos, nrm, mint, idx = s.download(aux=True)   # (synchronises the context, whatever stream its work ran on)
        st = s.stats()
        assert (st.max_depth, np.float32(st.closest), st.rays, st.overflow_tiles) == want
        assert np.array_equal(out.cpu().numpy(), sc.oracle_vis("t3", "side", B9))
        assert np.array_equal(s.download_shadow(), sc.oracle_vis("t3", "top", B9))
        for k, a in (("pos4", pos), ("nrm4", nrm), ("minT", mint), ("index", idx)):
            assert same_bits(a, ref[k]), f"Render after the shadow traces: {k} differs"


# 7 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ambient", [0.25, 0.0])
def test_light_image_equals_the_model(ambient):
    S = pyoracle.load_setup("t3")
    light = sc.LIGHTS["side"]
    with flake("t3") as s:
        s.Render()
        s.trace_shadow(light, bias=B9)
        p = sf.sf_shadow_params()
        assert sf.lib().sf_shadow_defaults(s.ctx, ctypes.byref(p)) == sf.SF_OK
        assert sf.lib().sf_light_image(s.ctx, ctypes.byref(p), 0.25, None, None, None, None) == sf.SF_ESTATE
        s.PostProcess()
        img = s.download_image()
        pos, nrm, _, _ = s.download()
        vis = s.download_shadow()
        s.light_image(light, ambient=ambient)
        got = s.download_image()
    assert np.array_equal(vis, sc.oracle_vis("t3", "side", B9))
    want = lights.light_model(img, pos, nrm, vis, S["origin"], light, ambient)
    assert np.array_equal(got[..., 3], img[..., 3])
    bad = np.argwhere((got != want).any(axis=-1))
    assert bad.size == 0, f"{len(bad)} pixels differ, first {bad[:4]}"
    assert (want != img).any() and len(np.unique(want[..., :3])) > 16   # the lighting did something


# 8 ---------------------------------------------------------------------------------------------------
def test_error_codes():
    import torch
    L = sf.lib()
    pos = torch.zeros((36, 64, 4), dtype=torch.float32, device="cuda")
    out = torch.full((36 * 64,), 9, dtype=torch.uint8, device="cuda")
    pp, op = ctypes.c_void_p(pos.data_ptr()), ctypes.c_void_p(out.data_ptr())

    def P(w=0, h=0, bias=B9, max_depth=0):
        p = sf.sf_shadow_params()
        p.light[:] = [-1.5, -2.5, 2.0]
        p.bias, p.width, p.height, p.max_depth = bias, w, h, max_depth
        return ctypes.byref(p)

    host = np.empty((36, 64), np.uint8)
    hp = host.ctypes.data_as(ctypes.c_void_p)
    with sf.Sphereflake(64, 36) as s:
        assert L.sf_trace_shadow_to(s.ctx, P(64, 36), pp, op) == sf.SF_ENOVIEW
        assert L.sf_trace_shadow(s.ctx, P()) == sf.SF_ENOVIEW
        S = pyoracle.load_setup("t1")
        s.SetView(S["origin"], S["tl"], S["tr"], S["bl"])
        assert L.sf_download_shadow(s.ctx, hp) == sf.SF_ESTATE
        assert L.sf_trace_shadow_to(s.ctx, P(64, 36), pp, None) == sf.SF_EINVAL
        for bias in (-0.25, 1.0, 2.0, float("nan")):
            assert L.sf_trace_shadow_to(s.ctx, P(64, 36, bias=bias), pp, op) == sf.SF_EINVAL
        assert L.sf_trace_shadow_to(s.ctx, P(64, 36, max_depth=32), pp, op) == sf.SF_EINVAL
        assert L.sf_trace_shadow_to(s.ctx, P(32, 16), None, op) == sf.SF_EINVAL   # sizes against a NULL pos4
        assert L.sf_trace_shadow_to(s.ctx, P(64, 0), pp, op) == sf.SF_EINVAL
        assert L.sf_trace_shadow(s.ctx, P(32, 16)) == sf.SF_EINVAL
        assert L.sf_trace_shadow_to(None, P(64, 36), pp, op) == sf.SF_EINVAL
        assert L.sf_trace_shadow_to(s.ctx, None, pp, op) == sf.SF_EINVAL
        s.Synchronize()
        assert (out == 9).all()   # none of them wrote
        # an all-miss position image: every byte 255, no ray
        assert L.sf_trace_shadow_to(s.ctx, P(64, 36), pp, op) == sf.SF_OK
        s.Synchronize()
        assert (out == 255).all()
        assert s.stats().rays == 0
