"""Directional-light shadows on the GPU (sf_trace_sun_to / sf_trace_sun / sf_light_image_sun) against the CPU oracle:
the visibility byte of every pixel is bit-exact with tests/suncheck.py, which traces every pixel's ray from its own
origin with the reference's own arithmetic (oracle/), one call per surface pixel, for the origin, direction and bound
of sphereflake_amd.lights.sun_model."""
import ctypes

import numpy as np
import pytest

import sphereflake_amd as sf
from sphereflake_amd import lights
from conftest import load_frame
from dirscheck import same_bits
from oracle import pyoracle
from rayscheck import frame, oracle_multi
from sfcheck import bad_rows, row_digests
import suncheck as su

pytestmark = pytest.mark.gpu

BIASES = (0.0, su.B10)
FORCE_MIXED = "0x8000"   # SF_FLAG_FORCE_MIXED
FIXUP_LOOP_COPIES = 38   # (t3 at 4 levels flags about 55.8 of a copy's 56.25 tiles: about 2120)
# (fixture, direction, tau, variant): t1's 36 rows end in partial tiles
CASES = (("t1", "side", 4.0, "avx"), ("t3", "cam", 4.0, "avx"), ("t3", "cam", 8.0, "avx"), ("t1", "side", 4.0, "sse"))


@pytest.fixture(scope="module", autouse=True)
def device():
    sf.build()
    assert sf.device_count() >= 1, "no HIP device visible: GPU tests must run on an MI355X"


def flake(name, variant="avx"):
    S = pyoracle.load_setup(name)
    s = sf.Sphereflake(S["W"], S["H"])
    s.SetVariant(variant)
    s.SetView(S["origin"], S["tl"], S["tr"], S["bl"])
    return s


def both_outcomes(vis, name, variant="avx"):
    """A constant output cannot pass: at least 50 shadowed and 50 lit surface pixels."""
    surf = frame(name, variant)["minT"] < su.FLT_MAX
    assert int((vis == 0).sum()) >= 50 and int(((vis == 255) & surf).sum()) >= 50


# 1 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dir_name,tau,variant", CASES)
def test_numpy_image_equals_the_oracle(name, dir_name, tau, variant):
    """The oracle's own frame, uploaded: both biases."""
    pos = frame(name, variant)["pos4"]
    with flake(name, variant) as s:
        for bias in BIASES:
            ref = su.oracle_vis(name, dir_name, bias, tau, variant)
            both_outcomes(ref, name, variant)
            got = s.trace_sun(su.direction(dir_name), tau, bias=bias, pos=pos)
            assert got.dtype == np.uint8 and got.shape == ref.shape
            bad = np.argwhere(got != ref)
            assert bad.size == 0, f"{name} {dir_name} tau {tau} {variant} bias {bias}: {len(bad)} pixels differ, first {bad[:4]}"


def test_rendered_frame_equals_the_oracle():
    """Render, trace_sun() on the context's own G-buffer with the library's defaults (tau 4, bias 2^-10),
    download_shadow()."""
    with flake("t3") as s:
        s.Render()
        assert s.trace_sun(su.direction("cam")) is None
        assert np.array_equal(s.download_shadow(), su.oracle_vis("t3", "cam", su.B10))
        assert s.shadow_buffer() != 0
        p = s.sun_params((0.0, 0.0, 2.0))
        assert (p.distance, p.bias) == (4.0, 2.0 ** -10) and tuple(p.dir) == (0.0, 0.0, 2.0)


# 2 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("name,dir_name", su.CASES)
def test_any_hit_equals_closest_hit(name, dir_name, forced, monkeypatch):
    """trace_rays of the same per-pixel origins F and directions d through the closest-hit mixed traversal, then
    min_t < bound on the host: identical vis."""
    if forced:
        monkeypatch.setenv("SF_FLAGS", FORCE_MIXED)
    S = pyoracle.load_setup(name)
    pos = frame(name)["pos4"]
    s_dir = su.direction(dir_name)
    with flake(name) as s:
        for bias in BIASES:
            Fo, d, bound, surf = lights.sun_model(pos, S["origin"], s_dir, su.TAU, bias)
            _, _, mint, _ = s.trace_rays(Fo.reshape(-1, 3), d)
            mint = mint.reshape(surf.shape)
            want = np.where(surf & (mint < bound), 0, 255).astype(np.uint8)
            got = s.trace_sun(s_dir, su.TAU, bias=bias, pos=pos)
            assert np.array_equal(got, want)
            assert np.array_equal(got, su.oracle_vis(name, dir_name, bias))


# 3 ---------------------------------------------------------------------------------------------------
def test_overflow_tiles_are_retraced():
    """max_depth = 4 provisions too few levels (the sun rays reach depth 6-7): same bits, and the re-trace counter
    moved."""
    with flake("t3") as s:
        o0 = s.stats().overflow_tiles
        got = s.trace_sun(su.direction("cam"), su.TAU, bias=su.B10, pos=frame("t3")["pos4"], max_depth=4)
        assert np.array_equal(got, su.oracle_vis("t3", "cam", su.B10))
        assert s.stats().overflow_tiles > o0
    with flake("t1") as s:
        got = s.trace_sun(su.direction("side"), su.TAU, bias=su.B10, pos=frame("t1")["pos4"], max_depth=4)
        assert np.array_equal(got, su.oracle_vis("t1", "side", su.B10))


def test_more_flagged_tiles_than_fixup_blocks():
    """t3's position image stacked R times into one 80 x 45R image at max_depth = 4: more flagged tiles than the
    re-trace launch has blocks (1024), so its blocks walk the list more than once. 45 is no multiple of 8: the copies
    fall differently into tiles, the per-pixel bytes are the oracle's all the same."""
    R = FIXUP_LOOP_COPIES
    pos = np.concatenate([frame("t3")["pos4"]] * R)
    want = np.concatenate([su.oracle_vis("t3", "cam", su.B10)] * R)
    with flake("t3") as s:
        o0 = s.stats().overflow_tiles
        got = s.trace_sun(su.direction("cam"), su.TAU, bias=su.B10, pos=pos, max_depth=4)
        moved = s.stats().overflow_tiles - o0
    print("flagged tiles", moved, "per copy", moved / R)
    assert moved > 1024
    assert np.array_equal(got, want)


# 4 ---------------------------------------------------------------------------------------------------
def test_partial_tiles_and_unaligned_outputs():
    """A 13 x 11 crop (partial tiles in both directions, rows not 8-byte aligned) equals the crop of the whole; so does
    the whole image into an output pointer that is not 8-byte aligned (whole tiles, the per-byte store)."""
    import torch
    pos = frame("t3")["pos4"]
    ref = su.oracle_vis("t3", "cam", su.B10)
    s_dir = su.direction("cam")
    y0, x0, h, w = 5, 13, 11, 13
    crop = np.ascontiguousarray(pos[y0:y0 + h, x0:x0 + w])
    sub = ref[y0:y0 + h, x0:x0 + w]
    assert (sub == 0).sum() >= 30 and (sub == 255).sum() >= 30
    with flake("t3") as s:
        assert np.array_equal(s.trace_sun(s_dir, su.TAU, bias=su.B10, pos=crop), sub)
        for img, want, off in ((crop, sub, 3), (pos, ref, 1), (pos, ref, 0)):
            hh, ww = want.shape
            pt = torch.from_numpy(np.ascontiguousarray(img)).cuda()
            out = torch.full((off + hh * ww + 64,), 0x5a, dtype=torch.uint8, device="cuda")
            assert out.data_ptr() % 8 == 0
            torch.cuda.synchronize()
            s.trace_sun(s_dir, su.TAU, bias=su.B10, pos=pt, out=out.data_ptr() + off)
            s.Synchronize()
            o = out.cpu().numpy()
            assert (o[:off] == 0x5a).all() and (o[off + hh * ww:] == 0x5a).all(), "wrote outside the image"
            assert np.array_equal(o[off:off + hh * ww].reshape(hh, ww), want), (hh, ww, off)


# 5 ---------------------------------------------------------------------------------------------------
def test_directions_without_a_ray_and_use_origin():
    fx = load_frame("t3")
    S = pyoracle.load_setup("t3")
    pos = frame("t3")["pos4"]
    with flake("t3") as s:
        for direction in ((np.nan, 0.0, 1.0), (np.inf, 0.0, 0.0), (0.0, -np.inf, 3.0), (0.0, 0.0, 0.0)):
            got = s.trace_sun(direction, su.TAU, bias=su.B10, pos=pos)
            assert (got == 255).all(), direction
        s.Render()
        p, n, _, _ = s.download()
        assert bad_rows(fx["row_digest_gbuf"], row_digests(p, n)) == []
    # a context that looks from elsewhere, told the origin the position image is relative to
    with flake("t1") as s:
        got = s.trace_sun(su.direction("cam"), su.TAU, bias=su.B10, pos=pos, origin=S["origin"])
        assert np.array_equal(got, su.oracle_vis("t3", "cam", su.B10))
        assert not np.array_equal(s.trace_sun(su.direction("cam"), su.TAU, bias=su.B10, pos=pos), got)


# 6 ---------------------------------------------------------------------------------------------------
def test_callers_stream_between_renders_and_stats():
    """Render, sun shadows on a caller's torch stream, Render -- no host synchronisation in between; the statistics are
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
        s.trace_sun(su.direction("cam"), 8.0, bias=su.B10, pos=pt, out=out, stream=ts.cuda_stream)
        s.trace_sun(su.direction("cam"), su.TAU, bias=su.B10, stream=ts.cuda_stream)   # the context's frame and buffer
        s.Render(emit_aux=True)
        pos, nrm, mint, idx = s.download(aux=True)   # (synchronises the context, whatever stream its work ran on)
        st = s.stats()
        assert (st.max_depth, np.float32(st.closest), st.rays, st.overflow_tiles) == want
        assert np.array_equal(out.cpu().numpy(), su.oracle_vis("t3", "cam", su.B10, 8.0))
        assert np.array_equal(s.download_shadow(), su.oracle_vis("t3", "cam", su.B10))
        for k, a in (("pos4", pos), ("nrm4", nrm), ("minT", mint), ("index", idx)):
            assert same_bits(a, ref[k]), f"Render after the sun traces: {k} differs"


# 7 ---------------------------------------------------------------------------------------------------
def test_zero_sign_columns_do_not_reach_the_byte():
    """Caller-set child frames whose depth-1 axis column sum is an exact -0 -- what raises SF_STATUS_ZSIGN in the
    closest-hit mixed traversal and sends the group to its per-origin fallback. The any-hit mode ignores the flag
    (a zero's sign reaches no comparison); the oracle, which forms every column with the ray's own
    centre, pins that."""
    S = dict(pyoracle.load_setup("t1"))
    children = np.array(sf.child_transforms(), np.float32)
    children[8, 4:7] *= np.float32(-1.0)    # child 8 turned half round about its x axis: column 1 = (-0, -1/2, -0.866)
    children[8, 8:11] *= np.float32(-1.0)
    root = sf.root_transform(S["origin"])
    p0, p1, p2, b = root[0:3], root[4:7], root[8:11], children[8, 4:7]
    x = (p0[0] * b[0] + p1[0] * b[1]) + p2[0] * b[2]   # the x component of the column sum, as expand forms it
    assert x == 0 and np.signbit(x), "the setup no longer makes a -0 column sum"
    S["children"] = children
    S["root"] = root
    fr = pyoracle.render(S)
    surf = fr["minT"] < su.FLT_MAX
    assert surf.sum() > 500
    s_dir = su.direction("side")
    mint, pick, _ = su.oracle_sun_rays(children, fr["pos4"], S["origin"], s_dir, su.TAU, 70.0)
    ref = su.vis_of(fr["pos4"], S["origin"], s_dir, su.TAU, su.B10, mint)
    assert int((ref == 0).sum()) >= 50 and int(((ref == 255) & surf).sum()) >= 50
    with flake("t1") as s:
        s.SetSetup(children, root)
        got = s.trace_sun(s_dir, su.TAU, bias=su.B10, pos=fr["pos4"])
        bad = np.argwhere(got != ref)
        assert bad.size == 0, f"{len(bad)} pixels differ, first {bad[:4]}"
        # the closest-hit route (flag raised, per-origin fallback) agrees
        Fo, d, bound, sm = lights.sun_model(fr["pos4"], S["origin"], s_dir, su.TAU, su.B10)
        _, _, mt, _ = s.trace_rays(Fo.reshape(-1, 3), d)
        assert np.array_equal(np.where(sm & (mt.reshape(sm.shape) < bound), 0, 255).astype(np.uint8), ref)


# 8 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ambient", [0.25, 0.0])
def test_light_image_sun_equals_the_model(ambient):
    s_dir = su.direction("cam")
    with flake("t3") as s:
        s.Render()
        s.trace_sun(s_dir, su.TAU, bias=su.B10)
        p = s.sun_params(s_dir)
        assert sf.lib().sf_light_image_sun(s.ctx, ctypes.byref(p), 0.25, None, None, None, None) == sf.SF_ESTATE
        s.PostProcess()
        img = s.download_image()
        pos, nrm, _, _ = s.download()
        vis = s.download_shadow()
        s.light_image_sun(s_dir, ambient=ambient)
        got = s.download_image()
    assert np.array_equal(vis, su.oracle_vis("t3", "cam", su.B10))
    want = lights.light_model_sun(img, pos, nrm, vis, s_dir, ambient)
    assert np.array_equal(got[..., 3], img[..., 3])
    bad = np.argwhere((got != want).any(axis=-1))
    assert bad.size == 0, f"{len(bad)} pixels differ, first {bad[:4]}"
    assert (want != img).any() and len(np.unique(want[..., :3])) > 16   # the lighting did something


# 9 ---------------------------------------------------------------------------------------------------
def test_error_codes():
    import torch
    L = sf.lib()
    pos = torch.zeros((36, 64, 4), dtype=torch.float32, device="cuda")
    out = torch.full((36 * 64,), 9, dtype=torch.uint8, device="cuda")
    pp, op = ctypes.c_void_p(pos.data_ptr()), ctypes.c_void_p(out.data_ptr())

    def P(w=0, h=0, bias=su.B10, max_depth=0, distance=4.0):
        p = sf.sf_sun_params()
        p.dir[:] = [0.0, 0.6, 0.8]
        p.distance, p.bias, p.width, p.height, p.max_depth = distance, bias, w, h, max_depth
        return ctypes.byref(p)

    with sf.Sphereflake(64, 36) as s:
        d = sf.sf_sun_params()
        assert L.sf_sun_defaults(s.ctx, ctypes.byref(d)) == sf.SF_OK and L.sf_sun_defaults(s.ctx, None) == sf.SF_EINVAL
        assert (tuple(d.dir), d.distance, d.bias, d.use_origin, d.width, d.max_depth) == ((0.0, 0.0, 1.0), 4.0, 2.0 ** -10, 0, 0, 0)
        assert L.sf_trace_sun_to(s.ctx, P(64, 36), pp, op) == sf.SF_ENOVIEW
        assert L.sf_trace_sun(s.ctx, P()) == sf.SF_ENOVIEW
        S = pyoracle.load_setup("t1")
        s.SetView(S["origin"], S["tl"], S["tr"], S["bl"])
        assert L.sf_trace_sun_to(s.ctx, P(64, 36), pp, None) == sf.SF_EINVAL
        for bias in (-0.25, 1.0, 2.0, float("nan")):
            assert L.sf_trace_sun_to(s.ctx, P(64, 36, bias=bias), pp, op) == sf.SF_EINVAL
        for distance in (0.0, -4.0, float("inf"), float("nan")):
            assert L.sf_trace_sun_to(s.ctx, P(64, 36, distance=distance), pp, op) == sf.SF_EINVAL
            assert L.sf_trace_sun(s.ctx, P(distance=distance)) == sf.SF_EINVAL
        assert L.sf_trace_sun_to(s.ctx, P(64, 36, max_depth=32), pp, op) == sf.SF_EINVAL
        assert L.sf_trace_sun_to(s.ctx, P(32, 16), None, op) == sf.SF_EINVAL   # sizes against a NULL pos4
        assert L.sf_trace_sun_to(s.ctx, P(64, 0), pp, op) == sf.SF_EINVAL
        assert L.sf_trace_sun(s.ctx, P(32, 16)) == sf.SF_EINVAL
        assert L.sf_trace_sun_to(s.ctx, None, pp, op) == sf.SF_EINVAL
        for ambient in (-0.1, 1.5, float("nan")):
            assert L.sf_light_image_sun(s.ctx, P(), ambient, None, None, None, None) == sf.SF_EINVAL
        assert L.sf_light_image_sun(s.ctx, P(), 0.25, None, None, None, None) == sf.SF_ESTATE   # no image, no bytes yet
        assert L.sf_light_image_sun(s.ctx, None, 0.25, None, None, None, None) == sf.SF_EINVAL
        s.Synchronize()
        assert (out == 9).all()   # none of them wrote
        # an all-miss position image: every byte 255, no ray
        assert L.sf_trace_sun_to(s.ctx, P(64, 36), pp, op) == sf.SF_OK
        s.Synchronize()
        assert (out == 255).all()
        assert s.stats().rays == 0
