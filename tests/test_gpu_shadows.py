"""Many lights per pixel in one launch on the GPU (sf_trace_shadows_to / sf_trace_shadows / sf_light_image_many): bit i
of every pixel's mask word equals the visibility byte of light i -- the CPU oracle's (tests/shadowcheck.py) for the
named lights, the single-light kernel's (trace_shadow) for all 64 bits -- and the lighting pass equals
sphereflake_amd.lights.light_model_many bit for bit."""
import ctypes

import numpy as np
import pytest

import sphereflake_amd as sf
from sphereflake_amd import lights
from dirscheck import same_bits
from maskcheck import assert_mask
from oracle import pyoracle
from rayscheck import frame
import shadowcheck as sc

pytestmark = pytest.mark.gpu

BIASES = (0.0, 2.0 ** -11, 2.0 ** -7)
B9 = 2.0 ** -9
FIXUP_LOOP_COPIES = 38   # (t3 at 4 levels flags about 55.7 of a copy's 56.25 tiles: about 2115)
NAMED = {"t1": ("side", "low", "inside"), "t3": ("side", "top")}
U1 = np.uint64(1)


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


def points(names):
    return np.array([light_of(n) for n in names], np.float32)


def oracle_mask(name, names, bias, variant="avx"):
    return lights.masks_from_vis([sc.oracle_vis(name, n, bias, variant) for n in names])


def surface_of(name, variant="avx"):
    return frame(name, variant)["minT"] < np.finfo(np.float32).max


def popcount(a):
    return np.unpackbits(np.ascontiguousarray(a).view(np.uint8).reshape(a.shape + (-1,)), axis=-1).sum(axis=-1)


# 1 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["avx", "sse"])
@pytest.mark.parametrize("name", ["t1", "t3"])
def test_small_n_equals_the_oracle(name, variant):
    """The oracle's own frame, uploaded; the named lights (t1's include the one inside the radius-2 ball)."""
    names = NAMED[name]
    n = len(names)
    pos = frame(name, variant)["pos4"]
    surf = surface_of(name, variant)
    with flake(name, variant) as s:
        for bias in BIASES:
            if variant == "avx":   # a constant output cannot pass
                for ln in names:
                    v = sc.oracle_vis(name, ln, bias, variant)
                    assert int((v == 0).sum()) >= 50 and int(((v == 255) & surf).sum()) >= 50, (ln, bias)
            got = s.trace_shadows(points(names), bias=bias, pos=pos)
            assert_mask(got, oracle_mask(name, names, bias, variant), f"{name} {variant} bias {bias}")
            assert (got >> np.uint64(n) == 0).all()
            assert (got[~surf] == np.uint64((1 << n) - 1)).all()


# 2 ---------------------------------------------------------------------------------------------------
def test_all_64_bits_equal_the_single_light_kernel():
    """lights.disc(side, 0.25, 64) on t1: bit i is trace_shadow's byte for light i on the same image (the oracle
    gives, of 830 surface pixels, 262 shadowed for all 64 lights, 243 lit for all, 325 penumbra, and 303 whose upper
    32 bits carry what the lower do not). Prefixes of the list: n = 1, 32, 33."""
    pos = frame("t1")["pos4"]
    surf = surface_of("t1")
    L = lights.disc(sc.LIGHTS["side"], 0.25, 64)
    assert L.shape == (64, 3) and np.linalg.norm(L.astype(np.float64), axis=1).min() > 3.5
    with flake("t1") as s:
        vis = [s.trace_shadow(L[i], bias=B9, pos=pos) for i in range(64)]
        for n in (64, 1, 32, 33):
            got = s.trace_shadows(L[:n], bias=B9, pos=pos)
            assert_mask(got, lights.masks_from_vis(vis[:n]), f"n = {n}")
            if n < 64:
                assert (got >> np.uint64(n) == 0).all()
            if n == 64:
                m64 = got
    pc = popcount(m64)
    penumbra = surf & (pc > 0) & (pc < 64)
    lo, hi = popcount(m64 & np.uint64(0xffffffff)), popcount(m64 >> np.uint64(32))
    print("penumbra", int(penumbra.sum()), "halves differ", int((lo != hi).sum()), "all shadowed",
          int((surf & (pc == 0)).sum()), "all lit", int((surf & (pc == 64)).sum()))
    assert int(penumbra.sum()) >= 100
    assert int((lo != hi).sum()) >= 100
    assert (m64[~surf] == np.uint64(0xffffffffffffffff)).all()


# 3 ---------------------------------------------------------------------------------------------------
def test_overflow_tiles_are_retraced_for_every_light():
    """max_depth = 4 provisions too few levels: same bits, and the re-trace counter moved; auto levels: same bits."""
    pos = frame("t3")["pos4"]
    names = NAMED["t3"]
    want = oracle_mask("t3", names, B9)
    with flake("t3") as s:
        o0 = s.stats().overflow_tiles
        got = s.trace_shadows(points(names), bias=B9, pos=pos, max_depth=4)
        assert_mask(got, want, "max_depth = 4")
        assert s.stats().overflow_tiles > o0
        assert_mask(s.trace_shadows(points(names), bias=B9, pos=pos), want, "auto levels")


def test_more_flagged_tiles_than_fixup_blocks():
    """t3's position image stacked R times into one 80 x 45R image, three lights, max_depth = 4: more flagged tiles than
    the re-trace launch has blocks (1024 is the larger of the two fixup grids), so its blocks walk the list more than
    once. 45 is no multiple of 8: the copies fall differently into tiles, the per-pixel masks are the same."""
    R = FIXUP_LOOP_COPIES
    names = ("side", "top", "side")
    pos = np.concatenate([frame("t3")["pos4"]] * R)
    want = np.concatenate([oracle_mask("t3", names, B9)] * R)
    with flake("t3") as s:
        o0 = s.stats().overflow_tiles
        got = s.trace_shadows(points(names), bias=B9, pos=pos, max_depth=4)
        moved = s.stats().overflow_tiles - o0
    print("flagged tiles", moved, "per copy", moved / R)
    assert moved > 1024
    assert_mask(got, want, f"t3 x {R}, 4 levels")


# 4 ---------------------------------------------------------------------------------------------------
def test_partial_tiles():
    """A 13 x 11 crop (partial tiles in both directions) equals the crop of the whole; nothing is written past the
    last mask."""
    import torch
    pos = frame("t3")["pos4"]
    names = NAMED["t3"]
    ref = oracle_mask("t3", names, B9)
    y0, x0, h, w = 17, 30, 11, 13
    sub = ref[y0:y0 + h, x0:x0 + w]
    assert len(np.unique(sub)) >= 3
    crop = np.ascontiguousarray(pos[y0:y0 + h, x0:x0 + w])
    with flake("t3") as s:
        assert_mask(s.trace_shadows(points(names), bias=B9, pos=crop), sub, "numpy crop")
        pt = torch.from_numpy(crop).cuda()
        sentinel = 0x5a5a5a5a5a5a5a5a
        out = torch.full((h * w + 8,), sentinel, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        s.trace_shadows(points(names), bias=B9, pos=pt, out=out)
        s.Synchronize()
        o = out.cpu().numpy().view(np.uint64)
        assert (o[h * w:] == np.uint64(sentinel)).all(), "wrote past the last pixel"
        assert_mask(o[:h * w].reshape(h, w), sub, "torch crop")


# 5 ---------------------------------------------------------------------------------------------------
def test_non_finite_light_in_the_middle():
    pos = frame("t3")["pos4"]
    L = np.array([sc.LIGHTS["side"], (np.nan, 0.0, 0.0), sc.LIGHTS["top"]], np.float32)
    with flake("t3") as s:
        got = s.trace_shadows(L, bias=B9, pos=pos)
    assert ((got >> U1) & U1 == 1).all()
    assert np.array_equal(np.where(got & U1, 255, 0), sc.oracle_vis("t3", "side", B9))
    assert np.array_equal(np.where((got >> np.uint64(2)) & U1, 255, 0), sc.oracle_vis("t3", "top", B9))
    assert (got >> np.uint64(3) == 0).all()


# 6 ---------------------------------------------------------------------------------------------------
def test_statistics_and_render_state_untouched():
    ref = frame("t3")
    with flake("t3") as s:
        s.Render(emit_aux=True)
        s.Synchronize()
        st0 = s.stats()
        s.trace_shadows(points(NAMED["t3"]), bias=B9)
        s.trace_shadows(lights.sky(16), bias=B9, pos=ref["pos4"])
        s.Synchronize()
        st1 = s.stats()
        assert (st1.max_depth, np.float32(st1.closest), st1.rays) == (st0.max_depth, np.float32(st0.closest), st0.rays)
        s.Render(emit_aux=True)
        pos, nrm, mint, idx = s.download(aux=True)
        for k, a in (("pos4", pos), ("nrm4", nrm), ("minT", mint), ("index", idx)):
            assert same_bits(a, ref[k]), f"Render after trace_shadows: {k} differs"


# 7 ---------------------------------------------------------------------------------------------------
def test_rendered_frame_path():
    """Render, trace_shadows() on the context's own G-buffer, download_shadow_masks()."""
    names = NAMED["t3"]
    host = np.empty((45, 80), np.uint64)
    with flake("t3") as s:
        s.Render()
        assert s.shadow_mask_buffer() == 0
        assert sf.lib().sf_download_shadow_masks(s.ctx, host.ctypes.data_as(ctypes.c_void_p)) == sf.SF_ESTATE
        assert s.trace_shadows(points(names), bias=B9) is None
        assert_mask(s.download_shadow_masks(), oracle_mask("t3", names, B9), "rendered frame")
        assert s.shadow_mask_buffer() != 0


# 8 ---------------------------------------------------------------------------------------------------
def lit_image(s, L, weights, ambient, origin):
    """(image before, image after light_image_many, model's image) for the lights L on the context's frame."""
    s.Render()
    s.trace_shadows(L, bias=B9)
    s.PostProcess()
    img = s.download_image()
    pos, nrm, _, _ = s.download()
    mask = s.download_shadow_masks()
    s.light_image_many(L, weights, ambient=ambient)
    got = s.download_image()
    return img, got, lights.light_model_many(img, pos, nrm, mask, origin, L, weights, ambient), mask


@pytest.mark.parametrize("weights", [(0.75, 0.5), None])
def test_light_image_many_equals_the_model(weights):
    S = pyoracle.load_setup("t3")
    names = NAMED["t3"]
    with flake("t3") as s:
        p = sf.sf_shadows_params()
        assert sf.lib().sf_shadows_defaults(s.ctx, ctypes.byref(p)) == sf.SF_OK
        keep = points(names)
        p.lights, p.n = keep.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), 2
        s.Render()
        s.PostProcess()
        assert sf.lib().sf_light_image_many(s.ctx, ctypes.byref(p), 0.25, None, None, None, None) == sf.SF_ESTATE
        img, got, want, mask = lit_image(s, points(names), weights, 0.25, S["origin"])
    assert_mask(mask, oracle_mask("t3", names, B9), "mask")
    assert np.array_equal(got[..., 3], img[..., 3])
    bad = np.argwhere((got != want).any(axis=-1))
    assert bad.size == 0, f"{len(bad)} pixels differ, first {bad[:4]}"
    assert (want != img).any() and len(np.unique(want[..., :3])) > 16   # the lighting did something


def test_light_image_many_of_one_light_is_light_image():
    light = sc.LIGHTS["side"]
    with flake("t3") as s:
        s.Render()
        s.trace_shadow(light, bias=B9)
        s.trace_shadows([light], bias=B9)
        s.PostProcess()
        img = s.download_image()
        s.light_image(light, ambient=0.25)
        one = s.download_image()
        s.PostProcess()
        assert np.array_equal(s.download_image(), img)
        s.light_image_many([light], [1.0], ambient=0.25)
        many = s.download_image()
    assert np.array_equal(one, many) and (one != img).any()


def test_light_image_many_on_the_disc_sums_in_order():
    """64 lights: S is a 64-term float32 sum, formed in index order on both sides (bits >= 32 of the mask are read)."""
    S = pyoracle.load_setup("t3")
    L = lights.disc(sc.LIGHTS["side"], 0.25, 64)
    with flake("t3") as s:
        img, got, want, mask = lit_image(s, L, None, 0.25, S["origin"])
        pos, nrm, _, _ = s.download()
    bad = np.argwhere((got != want).any(axis=-1))
    assert bad.size == 0, f"{len(bad)} pixels differ, first {bad[:4]}"
    assert (want != img).any()
    # the upper half of the mask carries weight: the model without it gives another image
    low = lights.light_model_many(img, pos, nrm, mask & np.uint64(0xffffffff), S["origin"], L, None, 0.25)
    assert (low != want).any()


# 9 ---------------------------------------------------------------------------------------------------
def test_error_codes():
    import torch
    Lb = sf.lib()
    pos = torch.zeros((36, 64, 4), dtype=torch.float32, device="cuda")
    out = torch.full((36 * 64,), 9, dtype=torch.int64, device="cuda")
    img = torch.full((36 * 64 * 4,), 9, dtype=torch.uint8, device="cuda")
    pp, op, ip = (ctypes.c_void_p(t.data_ptr()) for t in (pos, out, img))
    two = np.array([sc.LIGHTS["side"], sc.LIGHTS["top"]], np.float32)
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    keep = []

    def P(w=0, h=0, bias=B9, max_depth=0, n=2, lights_=two, weights=None):
        p = sf.sf_shadows_params()
        if lights_ is not None:
            p.lights = fp(lights_)
        if weights is not None:
            wa = np.asarray(weights, np.float32)
            keep.append(wa)
            p.weights = fp(wa)
        p.n, p.bias, p.width, p.height, p.max_depth = n, bias, w, h, max_depth
        return ctypes.byref(p)

    many = np.zeros((65, 3), np.float32) + 3.0
    with sf.Sphereflake(64, 36) as s:
        assert Lb.sf_trace_shadows_to(s.ctx, P(64, 36), pp, op) == sf.SF_ENOVIEW
        assert Lb.sf_trace_shadows(s.ctx, P()) == sf.SF_ENOVIEW
        assert Lb.sf_light_image_many(s.ctx, P(), 0.25, pp, pp, op, ip) == sf.SF_ENOVIEW
        S = pyoracle.load_setup("t1")
        s.SetView(S["origin"], S["tl"], S["tr"], S["bl"])
        for call in (lambda p: Lb.sf_trace_shadows_to(s.ctx, p, pp, op),
                     lambda p: Lb.sf_light_image_many(s.ctx, p, 0.25, pp, pp, op, ip)):
            assert call(P(64, 36, n=0)) == sf.SF_EINVAL
            assert call(P(64, 36, n=65, lights_=many)) == sf.SF_EINVAL
            assert call(P(64, 36, lights_=None)) == sf.SF_EINVAL
        assert Lb.sf_trace_shadows_to(s.ctx, P(64, 36), pp, None) == sf.SF_EINVAL
        for bias in (-0.25, 1.0, 2.0, float("nan")):
            assert Lb.sf_trace_shadows_to(s.ctx, P(64, 36, bias=bias), pp, op) == sf.SF_EINVAL
        assert Lb.sf_trace_shadows_to(s.ctx, P(64, 36, max_depth=32), pp, op) == sf.SF_EINVAL
        assert Lb.sf_trace_shadows_to(s.ctx, P(32, 16), None, op) == sf.SF_EINVAL   # sizes against a NULL pos4
        assert Lb.sf_trace_shadows_to(s.ctx, P(64, 0), pp, op) == sf.SF_EINVAL
        assert Lb.sf_trace_shadows(s.ctx, P(32, 16)) == sf.SF_EINVAL
        assert Lb.sf_trace_shadows_to(None, P(64, 36), pp, op) == sf.SF_EINVAL
        assert Lb.sf_trace_shadows_to(s.ctx, None, pp, op) == sf.SF_EINVAL
        for wts in ((0.5, -0.5), (float("nan"), 1.0)):
            assert Lb.sf_light_image_many(s.ctx, P(weights=wts), 0.25, pp, pp, op, ip) == sf.SF_EINVAL
        for amb in (-0.1, 1.5, float("nan")):
            assert Lb.sf_light_image_many(s.ctx, P(), amb, pp, pp, op, ip) == sf.SF_EINVAL
        s.Synchronize()
        assert (out == 9).all() and (img == 9).all()   # none of them wrote
        # a negative weight does not bother the trace, which ignores the weights; an all-miss position image: every
        # mask has exactly its low n bits set, no ray
        assert Lb.sf_trace_shadows_to(s.ctx, P(64, 36, weights=(0.5, -0.5)), pp, op) == sf.SF_OK
        s.Synchronize()
        assert (out == 3).all()
        assert s.stats().rays == 0
        with pytest.raises(ValueError):
            s.trace_shadows(many, pos=(pos.data_ptr(), 64, 36), out=out)
        with pytest.raises(ValueError):
            s.trace_shadows(np.zeros((0, 3), np.float32), pos=(pos.data_ptr(), 64, 36), out=out)


# 10 --------------------------------------------------------------------------------------------------
def test_callers_stream_between_renders():
    """Render, masks on a caller's torch stream into caller-owned tensors, Render -- no host synchronisation in
    between; the statistics are what the renders alone leave, and the later render's bits are unchanged."""
    import torch
    S = pyoracle.load_setup("t3")
    W, H = S["W"], S["H"]
    ref = frame("t3")
    names = NAMED["t3"]
    with flake("t3") as s:   # what two renders alone leave
        s.Render(emit_aux=True)
        s.Render(emit_aux=True)
        s.Synchronize()
        st0 = s.stats()
        want = (st0.max_depth, np.float32(st0.closest), st0.rays, st0.overflow_tiles)
    pt = torch.from_numpy(np.ascontiguousarray(ref["pos4"])).cuda()
    out = torch.full((H, W), 7, dtype=torch.int64, device="cuda")
    ts = torch.cuda.Stream()
    torch.cuda.synchronize()
    with flake("t3") as s:
        s.Render(emit_aux=True)
        s.trace_shadows(points(names), bias=B9, pos=pt, out=out, stream=ts.cuda_stream)
        s.trace_shadows(points(names[::-1]), bias=B9, stream=ts.cuda_stream)   # the context's frame, its own buffer
        s.Render(emit_aux=True)
        pos, nrm, mint, idx = s.download(aux=True)   # (synchronises the context, whatever stream its work ran on)
        st = s.stats()
        assert (st.max_depth, np.float32(st.closest), st.rays, st.overflow_tiles) == want
        assert_mask(out.cpu().numpy().view(np.uint64), oracle_mask("t3", names, B9), "caller's tensors")
        assert_mask(s.download_shadow_masks(), oracle_mask("t3", names[::-1], B9), "context's buffer")
        for k, a in (("pos4", pos), ("nrm4", nrm), ("minT", mint), ("index", idx)):
            assert same_bits(a, ref[k]), f"Render after the shadow traces: {k} differs"
