"""The colour light buffer on the GPU (sf_trace_suns_sum_to / sf_trace_shadows_sum_to / sf_light_fill /
sf_light_image_buffer): the summed buffer equals sphereflake_amd.lights.sum_model bit for bit -- fed the CPU oracle's
masks on its sampled pixels, the mask kernels' (trace_suns, trace_shadows) on whole images, per chunk of 64 beyond 64
entries -- a call equals its split into an overwriting and an accumulating call, and the resolve pass equals
light_model_buffer and, for grey colours, the older image passes with ambient 0."""
import ctypes

import numpy as np
import pytest

import sphereflake_amd as sf
from sphereflake_amd import lights
from dirscheck import same_bits
from lightsumcheck import BASE, CONE_COLOURS, assert_same, base_image, chunk_masks, colours, surface_of
from oracle import pyoracle
from rayscheck import frame
import shadowcheck as sc
import suncheck as su
import sunscheck as ss

pytestmark = pytest.mark.gpu

F = np.float32
B9 = 2.0 ** -9
NAMED = {"t1": ("side", "low", "inside"), "t3": ("side", "top")}   # (tests/test_gpu_shadows.py)
BIG = lights.SUM_MAX


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


def origin_of(name):
    return pyoracle.load_setup(name)["origin"]


def light_points(names):
    return np.array([sc.INSIDE if n == "inside" else sc.LIGHTS[n] for n in names], F)


def suns_model(s, base, pos, nrm, D, col, **kw):
    """sum_model over trace_suns' masks for consecutive chunks of 64."""
    masks = chunk_masks(s.trace_suns, D, distance=su.TAU, bias=su.B10, pos=pos, **kw)
    return lights.sum_model(base, pos, nrm, masks, D, col, "suns")


def lights_model(s, name, base, pos, nrm, L, col, **kw):
    masks = chunk_masks(s.trace_shadows, L, bias=B9, pos=pos, **kw)
    return lights.sum_model(base, pos, nrm, masks, L, col, "shadows", origin_of(name))


# 1 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", [("t1", "avx"), ("t3", "avx"), ("t1", "sse")])
def test_soft_sun_equals_the_model_over_the_oracle(name, variant):
    """The oracle's own frame, uploaded; the 8-direction cone with distinct RGB colours; both biases. Compared: the
    oracle's sampled pixels and every miss of the frame."""
    ref = frame(name, variant)
    pos, nrm = ref["pos4"], ref["nrm4"]
    D = ss.cone(name)
    with flake(name, variant) as s:
        for bias in (0.0, su.B10):
            mask, pick = ss.oracle_mask(name, D, su.TAU, bias, variant, None, ss.CONE_CASES[name][1])
            want = lights.sum_model(None, pos, nrm, [mask], D, CONE_COLOURS, "suns")
            got = s.trace_suns_sum(D, CONE_COLOURS, distance=su.TAU, bias=bias, pos=pos, nrm=nrm)
            assert_same(got, want, f"{name} {variant} bias {bias}", ss.compared(pos, pick))
            rgb = got[pick][:, :3]
            if variant == "avx":   # colour and visibility both show (tests/test_light_sum_host.py)
                assert int(((rgb[:, 0] != rgb[:, 1]) | (rgb[:, 1] != rgb[:, 2])).sum()) >= 100
            assert (got[~surface_of(pos)] == 0).all() and (got[..., 3] == 0).all()


# 2 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t1", "t3"])
def test_whole_images_equal_the_model_over_the_mask_kernel(name):
    ref = frame(name)
    pos, nrm = ref["pos4"], ref["nrm4"]
    D = lights.sky_dirs(64)
    with flake(name) as s:
        for n in (1, 33, 64):
            col = colours(n)
            want = suns_model(s, None, pos, nrm, D[:n], col)
            got = s.trace_suns_sum(D[:n], col, distance=su.TAU, bias=su.B10, pos=pos, nrm=nrm)
            assert_same(got, want, f"{name} n = {n}")
        # colours None: 1 / n per component
        assert_same(s.trace_suns_sum(D[:33], None, distance=su.TAU, bias=su.B10, pos=pos, nrm=nrm),
                    suns_model(s, None, pos, nrm, D[:33], None), f"{name} even colours")


# 3 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [100, 129])
def test_beyond_64_directions(n):
    """One call equals the model over the two or three chunk masks, and the call split at k with the second part
    accumulating."""
    ref = frame("t3")
    pos, nrm = ref["pos4"], ref["nrm4"]
    D = lights.sky_dirs(n, limit=BIG)
    col = colours(n)
    kw = dict(distance=su.TAU, bias=su.B10, pos=pos, nrm=nrm)
    with flake("t3") as s:
        want = suns_model(s, None, pos, nrm, D, col)
        got = s.trace_suns_sum(D, col, **kw)
        assert_same(got, want, f"n = {n}")
        assert len(np.unique(got[..., :3])) > 100
        for k in (1, 64, 65):
            first = s.trace_suns_sum(D[:k], col[:k], **kw)
            both = s.trace_suns_sum(D[k:], col[k:], accumulate=True, out=first, **kw)
            assert_same(both, got, f"n = {n} split at {k}")


# 4 ---------------------------------------------------------------------------------------------------
def test_accumulate_and_misses():
    ref = frame("t1")
    pos, nrm = ref["pos4"], ref["nrm4"]
    miss = ~surface_of(pos)
    assert int(miss.sum()) >= 100
    D = ss.cone("t1")
    base = base_image(pos.shape[:2])
    with flake("t1") as s:
        acc = s.trace_suns_sum(D, CONE_COLOURS, accumulate=True, out=base, distance=su.TAU, bias=su.B10, pos=pos, nrm=nrm)
        assert same_bits(acc[miss], base[miss]), "an accumulating call wrote a miss"
        assert (acc[..., 3] == F(BASE[3])).all(), ".w was not carried"
        assert_same(acc, suns_model(s, base, pos, nrm, D, CONE_COLOURS), "accumulating")
        assert (acc[~miss][:, :3] != base[~miss][:, :3]).any()
        import torch
        out = torch.from_numpy(base).cuda()   # an overwriting call into a buffer that holds the base
        pt, nt = torch.from_numpy(np.ascontiguousarray(pos)).cuda(), torch.from_numpy(np.ascontiguousarray(nrm)).cuda()
        s.trace_suns_sum(D, CONE_COLOURS, distance=su.TAU, bias=su.B10, pos=pt, nrm=nt, out=out)
        s.Synchronize()
        over = out.cpu().numpy()
        assert (over[miss] == 0).all() and (over[..., 3] == 0).all()
        assert_same(over, suns_model(s, None, pos, nrm, D, CONE_COLOURS), "overwriting")


# 5 ---------------------------------------------------------------------------------------------------
def overflow_case(s, call, tiles, chunks):
    """max_depth = 4 flags nearly every tile of t3: the accumulating call's bits equal the default depth's, and the
    re-trace counter moved by at least one tile and at most tiles x chunks."""
    want = call(0)
    o0 = s.stats().overflow_tiles
    got = call(4)
    moved = s.stats().overflow_tiles - o0
    print("flagged tiles", moved)
    assert_same(got, want, "max_depth = 4")   # (a chunk added twice shows here)
    assert 1 <= moved <= tiles * chunks
    return got


def test_overflow_with_an_accumulating_call():
    ref = frame("t3")
    pos, nrm = ref["pos4"], ref["nrm4"]
    D = lights.sky_dirs(100, limit=BIG)
    col = colours(100)
    base = base_image(pos.shape[:2])
    with flake("t3") as s:
        got = overflow_case(s, lambda depth: s.trace_suns_sum(D, col, accumulate=True, out=base, distance=su.TAU,
                                                              bias=su.B10, pos=pos, nrm=nrm, max_depth=depth), 60, 2)
        assert_same(got, suns_model(s, base, pos, nrm, D, col), "against the model")


# 6 ---------------------------------------------------------------------------------------------------
def test_partial_tiles():
    """A 13 x 11 crop (partial tiles in both directions), a caller's output with guard words before and after: the
    guards are intact and every pixel equals the model -- overwriting and accumulating, both traces."""
    import torch
    ref = frame("t3")
    y0, x0, h, w = 17, 30, 11, 13
    pos = np.ascontiguousarray(ref["pos4"][y0:y0 + h, x0:x0 + w])
    nrm = np.ascontiguousarray(ref["nrm4"][y0:y0 + h, x0:x0 + w])
    D = ss.cone("t3")
    L = light_points(NAMED["t3"])
    guard, sentinel = 16, -123.25
    pt, nt = torch.from_numpy(pos).cuda(), torch.from_numpy(nrm).cuda()
    with flake("t3") as s:
        want_s = suns_model(s, None, pos, nrm, D, CONE_COLOURS)
        want_l = lights_model(s, "t3", want_s, pos, nrm, L, CONE_COLOURS[:2])
        assert len(np.unique(want_s[..., 0])) >= 3
        out = torch.full((guard + h * w * 4 + guard,), sentinel, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        optr = out.data_ptr() + 4 * guard
        s.trace_suns_sum(D, CONE_COLOURS, distance=su.TAU, bias=su.B10, pos=pt, nrm=nt, out=optr)
        s.Synchronize()
        o = out.cpu().numpy()
        assert (o[:guard] == F(sentinel)).all() and (o[guard + h * w * 4:] == F(sentinel)).all(), "guards (suns)"
        assert_same(o[guard:guard + h * w * 4].reshape(h, w, 4), want_s, "suns crop")
        s.trace_shadows_sum(L, CONE_COLOURS[:2], accumulate=True, bias=B9, pos=(pt.data_ptr(), w, h),
                            nrm=(nt.data_ptr(), w, h), out=optr)
        s.Synchronize()
        o = out.cpu().numpy()
        assert (o[:guard] == F(sentinel)).all() and (o[guard + h * w * 4:] == F(sentinel)).all(), "guards (lights)"
        assert_same(o[guard:guard + h * w * 4].reshape(h, w, 4), want_l, "lights crop, accumulating")


# 7 ---------------------------------------------------------------------------------------------------
def test_entries_without_a_ray():
    """A NaN and a zero direction among good ones are lit with lam = 0: the sum is the good entries' alone, bit for
    bit. An infinite direction is lit with the lam the definition gives (the model's)."""
    ref = frame("t3")
    pos, nrm = ref["pos4"], ref["nrm4"]
    D = ss.cone("t3")
    kw = dict(distance=su.TAU, bias=su.B10, pos=pos, nrm=nrm)
    bad = np.array([D[0], (np.nan, 0.0, 1.0), D[1], (0.0, 0.0, 0.0), D[2], D[3]], F)
    col = CONE_COLOURS[:6]
    good = [0, 2, 4, 5]
    with flake("t3") as s:
        alone = s.trace_suns_sum(bad[good], col[good], **kw)
        got = s.trace_suns_sum(bad, col, **kw)
        assert_same(got, alone, "NaN and zero directions")
        assert_same(got, suns_model(s, None, pos, nrm, bad, col), "against the model")
        inf = np.array([D[0], (np.inf, 0.0, 0.0), D[1]], F)
        got = s.trace_suns_sum(inf, col[:3], **kw)
        want = suns_model(s, None, pos, nrm, inf, col[:3])
        assert_same(got, want, "an infinite direction")
        assert np.isinf(got[..., 0]).any() and np.isfinite(got[..., 0]).any()
        # the same for a light that is not finite
        L = np.array([sc.LIGHTS["side"], (np.nan, 0.0, 0.0), sc.LIGHTS["top"]], F)
        lkw = dict(bias=B9, pos=pos, nrm=nrm)
        assert_same(s.trace_shadows_sum(L, col[:3], **lkw), s.trace_shadows_sum(L[[0, 2]], col[[0, 2]], **lkw),
                    "a NaN light")


# 8 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", [("t1", "avx"), ("t3", "avx"), ("t1", "sse")])
def test_point_lights_equal_the_model_over_the_oracle(name, variant):
    ref = frame(name, variant)
    pos, nrm = ref["pos4"], ref["nrm4"]
    names = NAMED[name]
    L = light_points(names)
    col = CONE_COLOURS[:len(names)]
    with flake(name, variant) as s:
        for bias in (0.0, B9):
            mask = lights.masks_from_vis([sc.oracle_vis(name, n, bias, variant) for n in names])
            want = lights.sum_model(None, pos, nrm, [mask], L, col, "shadows", origin_of(name))
            got = s.trace_shadows_sum(L, col, bias=bias, pos=pos, nrm=nrm)
            assert_same(got, want, f"{name} {variant} bias {bias}")
            rgb = got[surface_of(pos)][:, :3]
            assert int(((rgb[:, 0] != rgb[:, 1]) | (rgb[:, 1] != rgb[:, 2])).sum()) >= 100


def test_point_lights_whole_image_against_the_mask_kernel():
    ref = frame("t1")
    pos, nrm = ref["pos4"], ref["nrm4"]
    L = lights.disc(sc.LIGHTS["side"], 0.25, 64)
    with flake("t1") as s:
        for n in (1, 33, 64):
            col = colours(n)
            got = s.trace_shadows_sum(L[:n], col, bias=B9, pos=pos, nrm=nrm)
            assert_same(got, lights_model(s, "t1", None, pos, nrm, L[:n], col), f"n = {n}")


@pytest.mark.parametrize("n", [100, 129])
def test_beyond_64_point_lights(n):
    ref = frame("t3")
    pos, nrm = ref["pos4"], ref["nrm4"]
    L = lights.sky(n, limit=BIG)
    col = colours(n)
    kw = dict(bias=B9, pos=pos, nrm=nrm)
    with flake("t3") as s:
        got = s.trace_shadows_sum(L, col, **kw)
        assert_same(got, lights_model(s, "t3", None, pos, nrm, L, col), f"n = {n}")
        for k in (1, 64, 65):
            first = s.trace_shadows_sum(L[:k], col[:k], **kw)
            assert_same(s.trace_shadows_sum(L[k:], col[k:], accumulate=True, out=first, **kw), got,
                        f"n = {n} split at {k}")


def test_point_lights_overflow_with_an_accumulating_call():
    ref = frame("t3")
    pos, nrm = ref["pos4"], ref["nrm4"]
    L = lights.sky(100, limit=BIG)
    col = colours(100)
    base = base_image(pos.shape[:2])
    with flake("t3") as s:
        got = overflow_case(s, lambda depth: s.trace_shadows_sum(L, col, accumulate=True, out=base, bias=B9, pos=pos,
                                                                 nrm=nrm, max_depth=depth), 60, 2)
        assert_same(got, lights_model(s, "t3", base, pos, nrm, L, col), "against the model")


# 9 ---------------------------------------------------------------------------------------------------
def test_resolve_equals_the_older_passes_for_grey_colours():
    """One overwriting sum with colours (w, w, w), then light_image_buffer: the image of light_image_suns /
    light_image_many with ambient 0, byte for byte."""
    D = lights.sun_cone(su.VECTORS["cam"], ss.HALF_ANGLE, 16)
    w = (np.arange(16, dtype=F) + F(1.0)) / F(160.0)
    L = lights.disc(sc.LIGHTS["side"], 0.25, 16)
    with flake("t3") as s:
        s.Render()
        s.PostProcess()
        img = s.download_image()
        s.trace_suns(D, su.TAU, bias=su.B10)
        s.light_image_suns(D, w, ambient=0.0)
        old = s.download_image()
        s.PostProcess()
        s.trace_suns_sum(D, np.repeat(w[:, None], 3, axis=1), distance=su.TAU, bias=su.B10)
        s.light_image_buffer()
        new = s.download_image()
        assert np.array_equal(new, old) and (new != img).any()
        s.PostProcess()
        s.trace_shadows(L, bias=B9)
        s.light_image_many(L, None, ambient=0.0)
        old = s.download_image()
        s.PostProcess()
        s.trace_shadows_sum(L, None, bias=B9)
        s.light_image_buffer()
        assert np.array_equal(s.download_image(), old) and (old != img).any()


def test_composed_scene():
    """The README's order on a small context after a real Render() + PostProcess(): fill, point lights, a sun cone, a
    sky of 100 -- the buffer equals the chain of host models over the mask kernels' masks, the image
    light_model_buffer's."""
    amb = (0.03125, 0.0625, 0.09375)
    L = lights.disc(sc.LIGHTS["side"], 0.25, 5)
    lc = colours(5, seed=9)
    D = lights.sun_cone(su.VECTORS["cam"], ss.HALF_ANGLE, 16)
    dc = np.tile(np.array([(1.0, 0.875, 0.625)], F) / F(32.0), (16, 1))
    Sky = lights.sky_dirs(100, limit=BIG)
    sk = lights.sky_colours(Sky)
    with flake("t3") as s:
        assert s.light_buffer() == 0
        s.Render()
        s.PostProcess()
        img = s.download_image()
        pos, nrm, _, _ = s.download()
        s.light_fill(amb)
        assert s.light_buffer() != 0
        filled = s.download_light()
        assert filled.shape == pos.shape and (filled == np.array(amb + (0.0,), F)).all()
        s.trace_shadows_sum(L, lc, accumulate=True, bias=B9)
        s.trace_suns_sum(D, dc, accumulate=True, distance=su.TAU, bias=su.B10)
        s.trace_suns_sum(Sky, sk, accumulate=True, distance=su.TAU, bias=su.B10)
        buf = s.download_light()
        s.light_image_buffer()
        got = s.download_image()
        want = lights_model(s, "t3", filled, pos, nrm, L, lc)
        want = suns_model(s, want, pos, nrm, D, dc)
        want = suns_model(s, want, pos, nrm, Sky, sk)
    assert_same(buf, want, "the composed buffer")
    model = lights.light_model_buffer(img, pos, buf)
    assert np.array_equal(got, model) and np.array_equal(got[..., 3], img[..., 3])
    assert (got != img).any() and len(np.unique(got[..., :3])) > 16
    rgb = buf[..., :3]
    assert int(((rgb[..., 0] != rgb[..., 1]) | (rgb[..., 1] != rgb[..., 2])).sum()) >= 100


# 10 --------------------------------------------------------------------------------------------------
def test_error_codes():
    import torch
    Lb = sf.lib()
    pos = torch.zeros((36, 64, 4), dtype=torch.float32, device="cuda")
    out = torch.full((36 * 64 * 4,), 9.0, dtype=torch.float32, device="cuda")
    img = torch.full((36 * 64 * 4,), 9, dtype=torch.uint8, device="cuda")
    pp, op, ip = (ctypes.c_void_p(t.data_ptr()) for t in (pos, out, img))
    three = lights.sun_cone((0.0, 0.6, 0.8), ss.HALF_ANGLE, 3)
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    keep = []

    def P(w=0, h=0, bias=su.B10, max_depth=0, n=3, points=three, cols=None, distance=4.0, accumulate=0):
        p = sf.sf_light_sum_params()
        if points is not None:
            p.points = fp(points)
        if cols is not None:
            ca = np.ascontiguousarray(cols, np.float32)
            keep.append(ca)
            p.colours = fp(ca)
        p.n, p.distance, p.bias, p.width, p.height, p.max_depth, p.accumulate = n, distance, bias, w, h, max_depth, accumulate
        return ctypes.byref(p)

    rgb = lambda *v: (ctypes.c_float * 3)(*v)
    many = np.tile(np.array([[0.0, 0.6, 0.8]], np.float32), (sf.SF_LIGHT_SUM_MAX + 1, 1))
    host = np.empty((36, 64, 4), np.float32)
    with sf.Sphereflake(64, 36) as s:
        d = sf.sf_light_sum_params()
        d.n = 5
        assert Lb.sf_light_sum_defaults(s.ctx, ctypes.byref(d)) == sf.SF_OK
        assert Lb.sf_light_sum_defaults(s.ctx, None) == sf.SF_EINVAL
        assert (bool(d.points), bool(d.colours), d.n, d.accumulate, d.distance, d.bias) == (False, False, 0, 0, 4.0, 2.0 ** -10)
        assert (d.use_origin, d.width, d.height, d.max_depth, d.stream) == (0, 0, 0, 0, None)
        suns_to = lambda p, a=pp, b=pp, c=op: Lb.sf_trace_suns_sum_to(s.ctx, p, a, b, c)
        lights_to = lambda p, a=pp, b=pp, c=op: Lb.sf_trace_shadows_sum_to(s.ctx, p, a, b, c)
        assert suns_to(P(64, 36)) == sf.SF_ENOVIEW and lights_to(P(64, 36)) == sf.SF_ENOVIEW
        assert Lb.sf_trace_suns_sum(s.ctx, P()) == sf.SF_ENOVIEW
        S = pyoracle.load_setup("t1")
        s.SetView(S["origin"], S["tl"], S["tr"], S["bl"])
        for call in (suns_to, lights_to):
            assert call(P(64, 36, n=0)) == sf.SF_EINVAL
            assert call(P(64, 36, n=sf.SF_LIGHT_SUM_MAX + 1, points=many)) == sf.SF_EINVAL
            assert call(P(64, 36, points=None)) == sf.SF_EINVAL
            for bad in (-0.5, float("nan"), float("inf")):
                assert call(P(64, 36, cols=[(0.5, 0.5, 0.5), (0.5, bad, 0.5), (0.5, 0.5, 0.5)])) == sf.SF_EINVAL
            for bias in (-0.25, 1.0, 2.0, float("nan")):
                assert call(P(64, 36, bias=bias)) == sf.SF_EINVAL
            assert call(P(64, 36, max_depth=32)) == sf.SF_EINVAL
            assert call(P(64, 0)) == sf.SF_EINVAL
            assert call(P(32, 16), None) == sf.SF_EINVAL        # sizes against a NULL pos4
            assert call(P(32, 16), pp, None) == sf.SF_EINVAL    # ... a NULL nrm4
            assert call(P(32, 16), pp, pp, None) == sf.SF_EINVAL   # ... a NULL out
            assert call(None) == sf.SF_EINVAL
            assert call(P(64, 36), pp, pp, None) == sf.SF_ESTATE   # the context's light buffer was never written
        for distance in (0.0, -4.0, float("inf"), float("nan")):
            assert suns_to(P(64, 36, distance=distance)) == sf.SF_EINVAL
            assert Lb.sf_trace_suns_sum(s.ctx, P(distance=distance)) == sf.SF_EINVAL
        # (the point lights have no distance; an accumulating call over an all-miss image writes nothing)
        assert lights_to(P(64, 36, distance=float("nan"), accumulate=1)) == sf.SF_OK
        assert Lb.sf_trace_suns_sum_to(None, P(64, 36), pp, pp, op) == sf.SF_EINVAL
        assert Lb.sf_trace_suns_sum(s.ctx, P(32, 16)) == sf.SF_EINVAL
        assert Lb.sf_trace_suns_sum(s.ctx, P(accumulate=1)) == sf.SF_ESTATE
        assert Lb.sf_trace_shadows_sum(s.ctx, P(accumulate=1)) == sf.SF_ESTATE
        assert Lb.sf_light_buffer(s.ctx, ctypes.byref(ctypes.c_void_p())) == sf.SF_ESTATE
        assert Lb.sf_download_light(s.ctx, host.ctypes.data_as(ctypes.c_void_p)) == sf.SF_ESTATE
        assert Lb.sf_light_image_buffer(s.ctx, None, pp, None, ip) == sf.SF_ESTATE   # no light buffer
        assert Lb.sf_light_image_buffer(s.ctx, None, pp, op, None) == sf.SF_ESTATE   # no image
        for bad in (-0.5, float("nan"), float("inf")):
            assert Lb.sf_light_fill(s.ctx, rgb(0.5, bad, 0.5), op, None) == sf.SF_EINVAL
            assert Lb.sf_light_fill(s.ctx, rgb(0.5, bad, 0.5), None, None) == sf.SF_EINVAL
        assert Lb.sf_light_fill(s.ctx, None, op, None) == sf.SF_EINVAL
        assert s.light_buffer() == 0   # (a refused fill made no buffer)
        s.Synchronize()
        assert (out == 9).all() and (img == 9).all()   # none of them wrote (but the one accepted call: all miss, below)
        # an all-miss position image: an overwriting call zeroes, an accumulating call leaves every pixel; no ray
        assert lights_to(P(64, 36, accumulate=1)) == sf.SF_OK
        s.Synchronize()
        assert (out == 9).all()
        assert suns_to(P(64, 36)) == sf.SF_OK
        s.Synchronize()
        assert (out == 0).all() and s.stats().rays == 0
        # a fill into the caller's buffer, and the context's own made by a fill
        assert Lb.sf_light_fill(s.ctx, rgb(0.25, 0.5, 0.75), op, None) == sf.SF_OK
        s.light_fill((0.5, 0.25, 0.125))
        assert (out.cpu().numpy().reshape(-1, 4) == np.array((0.25, 0.5, 0.75, 0.0), F)).all()
        assert (s.download_light() == np.array((0.5, 0.25, 0.125, 0.0), F)).all()
        with pytest.raises(ValueError):
            s.trace_suns_sum(many, pos=(pos.data_ptr(), 64, 36), nrm=(pos.data_ptr(), 64, 36), out=out)
        with pytest.raises(ValueError):
            s.trace_suns_sum(three, pos=(pos.data_ptr(), 64, 36), out=out)   # a device pos without a device nrm
        with pytest.raises(ValueError):
            s.trace_suns_sum(three, accumulate=True, pos=host, nrm=host)     # host images: the base goes in `out`


# 11 --------------------------------------------------------------------------------------------------
def test_callers_stream_between_renders():
    """Render, both summing traces and the resolve on a caller's torch stream (torch tensors, device addresses, the
    context's own buffers), Render -- no host synchronisation in between. The statistics are what two renders alone
    leave, and the later render's bits are the oracle frame's: nothing of the renders' state was touched."""
    import torch
    S = pyoracle.load_setup("t3")
    W, H = S["W"], S["H"]
    ref = frame("t3")
    D = ss.cone("t3")
    L = light_points(NAMED["t3"])
    with flake("t3") as s:   # what two renders alone leave
        s.Render(emit_aux=True)
        s.Render(emit_aux=True)
        s.Synchronize()
        st0 = s.stats()
        alone = (st0.max_depth, np.float32(st0.closest), st0.rays, st0.overflow_tiles)
    pt = torch.from_numpy(np.ascontiguousarray(ref["pos4"])).cuda()
    nt = torch.from_numpy(np.ascontiguousarray(ref["nrm4"])).cuda()
    out = torch.full((H, W, 4), 7.0, dtype=torch.float32, device="cuda")
    ts = torch.cuda.Stream()
    torch.cuda.synchronize()
    with flake("t3") as s:
        s.Render(emit_aux=True)
        s.PostProcess()
        s.trace_suns_sum(D, CONE_COLOURS, distance=su.TAU, bias=su.B10, pos=pt, nrm=nt, out=out, stream=ts.cuda_stream)
        s.trace_shadows_sum(L, CONE_COLOURS[:2], accumulate=True, bias=B9, pos=(pt.data_ptr(), W, H),
                            nrm=nt.data_ptr(), out=out.data_ptr(), stream=ts.cuda_stream)
        assert s.trace_suns_sum(D, CONE_COLOURS, distance=su.TAU, bias=su.B10, stream=ts.cuda_stream) is None
        s.trace_shadows_sum(L, CONE_COLOURS[:2], accumulate=True, bias=B9, stream=ts.cuda_stream)
        s.light_image_buffer(stream=ts.cuda_stream)
        s.Render(emit_aux=True)
        pos, nrm, mint, idx = s.download(aux=True)   # (synchronises the context, whatever stream its work ran on)
        st = s.stats()
        assert (st.max_depth, np.float32(st.closest), st.rays, st.overflow_tiles) == alone
        for k, a in (("pos4", pos), ("nrm4", nrm), ("minT", mint), ("index", idx)):
            assert same_bits(a, ref[k]), f"Render after the summing traces: {k} differs"
        theirs = out.cpu().numpy()
        own = s.download_light()
        want = suns_model(s, None, ref["pos4"], ref["nrm4"], D, CONE_COLOURS)
        want = lights_model(s, "t3", want, ref["pos4"], ref["nrm4"], L, CONE_COLOURS[:2])
        assert_same(theirs, want, "caller's tensors")
        assert_same(own, want, "the context's buffers")
        p, keep = s.light_sum_params(D, CONE_COLOURS)
        assert (p.n, p.accumulate, p.distance, p.bias) == (8, 0, 4.0, 2.0 ** -10)
