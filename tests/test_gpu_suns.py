"""Many sun directions per pixel in one launch on the GPU (sf_trace_suns_to / sf_trace_suns / sf_light_image_suns):
bit i of every pixel's mask word equals the visibility byte of direction i -- the CPU oracle's (tests/sunscheck.py) for
a soft sun of 8 directions and a sample of the sky dome, the single-direction kernel's (trace_sun) for all 64 bits --
and the lighting pass equals sphereflake_amd.lights.light_model_suns bit for bit."""
import ctypes

import numpy as np
import pytest

import sphereflake_amd as sf
from sphereflake_amd import lights
from dirscheck import same_bits
from maskcheck import assert_mask, assert_shape_of_mask, low, surface_of
from oracle import pyoracle
from rayscheck import frame
import suncheck as su
import sunscheck as ss

pytestmark = pytest.mark.gpu

BIASES = (0.0, su.B10)
FIXUP_LOOP_COPIES = 38   # (t3 at 4 levels flags nearly every tile of a copy's 56.25: as tests/test_gpu_sun.py)
U1 = np.uint64(1)


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


# 1 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", [("t1", "avx"), ("t3", "avx"), ("t1", "sse")])
def test_soft_sun_equals_the_oracle(name, variant):
    """The oracle's own frame, uploaded; 8 directions within 5 degrees of the fixture's sun; both biases. t1: all 830
    surface pixels; t3: every 3rd (1200). Compared: the traced pixels and every miss of the frame."""
    D = ss.cone(name)
    every = ss.CONE_CASES[name][1]
    pos = frame(name, variant)["pos4"]
    with flake(name, variant) as s:
        for bias in BIASES:
            want, pick = ss.oracle_mask(name, D, su.TAU, bias, variant, None, every)
            if variant == "avx":   # a constant mask cannot pass
                assert int(ss.mixed(want, 8, pick).sum()) >= 100
                for i in range(8):
                    assert int((pick & ~ss.bit(want, i)).sum()) >= 100 and int((pick & ss.bit(want, i)).sum()) >= 100
            got = s.trace_suns(D, su.TAU, bias=bias, pos=pos)
            where = ss.compared(pos, pick)
            assert (where | surface_of(pos)).all() and int(where.sum()) == int(pick.sum()) + int((~surface_of(pos)).sum())
            assert_mask(got, want, f"{name} {variant} bias {bias}", where)
            assert_shape_of_mask(got, 8, pos, f"{name} {variant} bias {bias}")


# 2 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t1", "t3"])
def test_all_64_bits_equal_the_single_direction_kernel(name):
    """lights.sky_dirs(64), whole images: bit i is trace_sun's byte for direction i on the same image. Prefixes of the
    list: n = 1 and 33. On t1 every 8th surface pixel also equals the oracle, where at least 8 directions of index
    >= 32 have both outcomes in quantity (tests/test_suns_host.py): a 32-bit shift cannot pass."""
    pos = frame(name)["pos4"]
    D = lights.sky_dirs(64)
    with flake(name) as s:
        vis = [s.trace_sun(D[i], su.TAU, bias=su.B10, pos=pos) for i in range(64)]
        for n in (64, 1, 33):
            got = s.trace_suns(D[:n], su.TAU, bias=su.B10, pos=pos)
            assert_mask(got, lights.masks_from_vis(vis[:n]), f"{name} n = {n}")
            assert_shape_of_mask(got, n, pos, f"{name} n = {n}")
            if n == 64:
                m64 = got
    print(name, "directions >= 32 with 20 shadowed pixels:", len([i for i in range(32, 64) if (vis[i] == 0).sum() >= 20]))
    if name == "t1":
        want, pick = ss.oracle_mask("t1", D, su.TAU, su.B10, "avx", None, ss.SKY_EVERY)
        both = [i for i in range(32, 64)
                if int((pick & ~ss.bit(want, i)).sum()) >= 20 and int((pick & ss.bit(want, i)).sum()) >= 20]
        assert len(both) >= 8
        assert_mask(m64, want, "t1 sky sample against the oracle", ss.compared(pos, pick))


# 3 ---------------------------------------------------------------------------------------------------
def test_order_and_directions_without_a_ray():
    """A permutation of the directions permutes the bits; a NaN, an infinite and a zero direction among good ones set
    their own bit everywhere and leave the others' alone."""
    pos = frame("t3")["pos4"]
    D = ss.cone("t3")
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    with flake("t3") as s:
        base = s.trace_suns(D, su.TAU, bias=su.B10, pos=pos)
        assert int(ss.mixed(base, 8, surface_of(pos)).sum()) >= 100   # the bits differ between directions
        got = s.trace_suns(D[perm], su.TAU, bias=su.B10, pos=pos)
        for j in range(8):
            assert np.array_equal(ss.bit(got, j), ss.bit(base, perm[j])), j
        bad = np.array([D[0], (np.nan, 0.0, 1.0), D[1], (np.inf, 0.0, 0.0), D[2], (0.0, 0.0, 0.0), D[3]], np.float32)
        got = s.trace_suns(bad, su.TAU, bias=su.B10, pos=pos)
        for j in (1, 3, 5):
            assert ss.bit(got, j).all(), j
        for j, i in ((0, 0), (2, 1), (4, 2), (6, 3)):
            assert np.array_equal(ss.bit(got, j), ss.bit(base, i)), j
        assert_shape_of_mask(got, 7, pos, "bad directions")
        only = s.trace_suns([(0.0, -np.inf, 3.0)], su.TAU, bias=su.B10, pos=pos)
        assert (only == U1).all()


# 4 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tiles", [("t3", 60), ("t1", 40)])
def test_overflow_tiles_are_retraced_once_for_all_directions(name, tiles):
    """max_depth = 4 provisions too few levels (the sun rays reach depth 6-7): same bits, the oracle's on its sample,
    and the re-trace counter moved by tiles, not by tiles x directions."""
    pos = frame(name)["pos4"]
    D = ss.cone(name)
    want, pick = ss.oracle_mask(name, D, su.TAU, su.B10, "avx", None, ss.CONE_CASES[name][1])
    with flake(name) as s:
        base = s.trace_suns(D, su.TAU, bias=su.B10, pos=pos)
        o0 = s.stats().overflow_tiles
        got = s.trace_suns(D, su.TAU, bias=su.B10, pos=pos, max_depth=4)
        moved = s.stats().overflow_tiles - o0
    print(name, "flagged tiles", moved)
    assert_mask(got, base, f"{name} max_depth = 4")
    assert_mask(got, want, f"{name} max_depth = 4 against the oracle", ss.compared(pos, pick))
    assert 1 <= moved <= tiles


def test_more_flagged_tiles_than_fixup_blocks():
    """t3's position image stacked R times into one 80 x 45R image, two directions, max_depth = 4: more flagged tiles
    than the re-trace launch has blocks (1024), so its blocks walk the list more than once. 45 is no multiple of 8: the
    copies fall differently into tiles, the per-pixel masks are the same."""
    R = FIXUP_LOOP_COPIES
    D = ss.cone("t3")[[0, 7]]
    one = frame("t3")["pos4"]
    pos = np.concatenate([one] * R)
    with flake("t3") as s:
        base = s.trace_suns(D, su.TAU, bias=su.B10, pos=one)
        o0 = s.stats().overflow_tiles
        got = s.trace_suns(D, su.TAU, bias=su.B10, pos=pos, max_depth=4)
        moved = s.stats().overflow_tiles - o0
    print("flagged tiles", moved, "per copy", moved / R)
    assert moved > 1024
    assert int(ss.mixed(base, 2, surface_of(one)).sum()) >= 20
    assert_mask(got, np.concatenate([base] * R), f"t3 x {R}, 4 levels")


# 5 ---------------------------------------------------------------------------------------------------
def test_partial_tiles():
    """A 13 x 11 crop (partial tiles in both directions) equals the crop of the whole; nothing is written before the
    first or past the last mask."""
    import torch
    pos = frame("t3")["pos4"]
    D = ss.cone("t3")
    y0, x0, h, w = 17, 30, 11, 13
    crop = np.ascontiguousarray(pos[y0:y0 + h, x0:x0 + w])
    guard, sentinel = 8, 0x5a5a5a5a5a5a5a5a
    with flake("t3") as s:
        sub = s.trace_suns(D, su.TAU, bias=su.B10, pos=pos)[y0:y0 + h, x0:x0 + w]
        assert len(np.unique(sub)) >= 3
        assert_mask(s.trace_suns(D, su.TAU, bias=su.B10, pos=crop), sub, "numpy crop")
        pt = torch.from_numpy(crop).cuda()
        out = torch.full((guard + h * w + guard,), sentinel, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        s.trace_suns(D, su.TAU, bias=su.B10, pos=pt, out=out.data_ptr() + 8 * guard)
        s.Synchronize()
        o = out.cpu().numpy().view(np.uint64)
        assert (o[:guard] == np.uint64(sentinel)).all(), "wrote before the first pixel"
        assert (o[guard + h * w:] == np.uint64(sentinel)).all(), "wrote past the last pixel"
        assert_mask(o[guard:guard + h * w].reshape(h, w), sub, "torch crop")


# 6 ---------------------------------------------------------------------------------------------------
def test_callers_stream_between_renders_and_the_shared_mask_buffer():
    """Render, trace_suns on a caller's torch stream twice (the caller's buffers, the context's), Render -- no host
    synchronisation in between; the statistics are what the renders alone leave and the later render's bits are the
    oracle frame's. download_shadow_masks() serves trace_suns, and a following trace_shadows overwrites the buffer."""
    import torch
    S = pyoracle.load_setup("t3")
    W, H = S["W"], S["H"]
    ref = frame("t3")
    D = ss.cone("t3")
    want, pick = ss.oracle_mask("t3", D, su.TAU, su.B10, "avx", None, ss.CONE_CASES["t3"][1])
    where = ss.compared(ref["pos4"], pick)
    with flake("t3") as s:   # what two renders alone leave
        s.Render(emit_aux=True)
        s.Render(emit_aux=True)
        s.Synchronize()
        st0 = s.stats()
        alone = (st0.max_depth, np.float32(st0.closest), st0.rays, st0.overflow_tiles)
    pt = torch.from_numpy(np.ascontiguousarray(ref["pos4"])).cuda()
    out = torch.full((H, W), 7, dtype=torch.int64, device="cuda")
    ts = torch.cuda.Stream()
    torch.cuda.synchronize()
    host = np.empty((H, W), np.uint64)
    with flake("t3") as s:
        s.Render(emit_aux=True)
        assert s.shadow_mask_buffer() == 0
        assert sf.lib().sf_download_shadow_masks(s.ctx, host.ctypes.data_as(ctypes.c_void_p)) == sf.SF_ESTATE
        s.trace_suns(D, su.TAU, bias=su.B10, pos=pt, out=out, stream=ts.cuda_stream)
        assert s.trace_suns(D[::-1], stream=ts.cuda_stream) is None   # the context's frame, its buffer, the defaults
        s.Render(emit_aux=True)
        pos, nrm, mint, idx = s.download(aux=True)   # (synchronises the context, whatever stream its work ran on)
        st = s.stats()
        assert (st.max_depth, np.float32(st.closest), st.rays, st.overflow_tiles) == alone
        for k, a in (("pos4", pos), ("nrm4", nrm), ("minT", mint), ("index", idx)):
            assert same_bits(a, ref[k]), f"Render after the sun traces: {k} differs"
        theirs = out.cpu().numpy().view(np.uint64)
        assert_mask(theirs, want, "caller's tensors", where)
        own = s.download_shadow_masks()
        assert s.shadow_mask_buffer() != 0
        for j in range(8):
            assert np.array_equal(ss.bit(own, j), ss.bit(theirs, 7 - j)), j
        p, keep = s.suns_params(D)
        assert (p.n, p.distance, p.bias) == (8, 4.0, 2.0 ** -10)
        # the buffer is trace_shadows' too
        L = lights.sky(3)
        s.trace_shadows(L, bias=su.B10)
        assert_mask(s.download_shadow_masks(), s.trace_shadows(L, bias=su.B10, pos=ref["pos4"]), "trace_shadows after")


# 7 ---------------------------------------------------------------------------------------------------
def test_zero_sign_columns_do_not_reach_the_bits():
    """The -0 column setup of tests/test_gpu_sun.py (test_zero_sign_columns_do_not_reach_the_byte), two directions,
    against the oracle, which forms every column with the ray's own centre."""
    S = dict(pyoracle.load_setup("t1"))
    children = np.array(sf.child_transforms(), np.float32)
    children[8, 4:7] *= np.float32(-1.0)
    children[8, 8:11] *= np.float32(-1.0)
    root = sf.root_transform(S["origin"])
    p0, p1, p2, b = root[0:3], root[4:7], root[8:11], children[8, 4:7]
    x = (p0[0] * b[0] + p1[0] * b[1]) + p2[0] * b[2]
    assert x == 0 and np.signbit(x), "the setup no longer makes a -0 column sum"
    S["children"] = children
    S["root"] = root
    fr = pyoracle.render(S)
    surf = fr["minT"] < su.FLT_MAX
    assert surf.sum() > 500
    D = ss.cone("t1")[[0, 7]]
    mints, pick, _ = ss.rays_for(children, fr["pos4"], S["origin"], D, su.TAU, 70.0)
    want = ss.mask_of(fr["pos4"], S["origin"], D, su.TAU, su.B10, mints, pick)
    for i in range(2):
        assert int((surf & ~ss.bit(want, i)).sum()) >= 50 and int((surf & ss.bit(want, i)).sum()) >= 50
    with flake("t1") as s:
        s.SetSetup(children, root)
        assert_mask(s.trace_suns(D, su.TAU, bias=su.B10, pos=fr["pos4"]), want, "-0 columns")


# 8 ---------------------------------------------------------------------------------------------------
def test_shadow_lod_constant():
    """set_shadow_lod(matched) (C about 394.7) on t3, four directions, every 3rd surface pixel, against the oracle at
    that constant; set_shadow_lod(0) restores the default's bits."""
    pos = frame("t3")["pos4"]
    D = ss.cone("t3")[[0, 3, 5, 7]]
    C = su.matched()
    want, pick = ss.oracle_mask("t3", D, su.TAU, su.B10, "avx", C, 3)
    where = ss.compared(pos, pick)
    with flake("t3") as s:
        base = s.trace_suns(D, su.TAU, bias=su.B10, pos=pos)
        s.set_shadow_lod(C)
        got = s.trace_suns(D, su.TAU, bias=su.B10, pos=pos)
        s.set_shadow_lod(0.0)
        again = s.trace_suns(D, su.TAU, bias=su.B10, pos=pos)
    assert_mask(got, want, f"C = {C}", where)
    assert (got != base).any()   # the constant changed bits
    assert_mask(again, base, "C = 0 again")


# 9 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ambient", [0.25, 0.0])
@pytest.mark.parametrize("explicit", [False, True])
def test_light_image_suns_equals_the_model(ambient, explicit):
    D = lights.sun_cone(su.VECTORS["cam"], ss.HALF_ANGLE, 16)
    weights = (np.arange(16, dtype=np.float32) + np.float32(1.0)) / np.float32(160.0) if explicit else None
    with flake("t3") as s:
        s.Render()
        s.PostProcess()
        p, keep = s.suns_params(D)
        assert sf.lib().sf_light_image_suns(s.ctx, ctypes.byref(p), 0.25, None, None, None, None) == sf.SF_ESTATE
        s.trace_suns(D, su.TAU, bias=su.B10)
        img = s.download_image()
        pos, nrm, _, _ = s.download()
        mask = s.download_shadow_masks()
        s.light_image_suns(D, weights, ambient=ambient)
        got = s.download_image()
    want = lights.light_model_suns(img, pos, nrm, mask, D, weights, ambient)
    assert np.array_equal(got[..., 3], img[..., 3])
    bad = np.argwhere((got != want).any(axis=-1))
    assert bad.size == 0, f"{len(bad)} pixels differ, first {bad[:4]}"
    assert (want != img).any() and len(np.unique(want[..., :3])) > 16   # the lighting did something
    assert int(ss.mixed(mask, 16, surface_of(pos)).sum()) >= 100          # ... over a penumbra


def test_light_image_suns_of_one_direction_is_light_image_sun():
    s_dir = su.direction("cam")
    with flake("t3") as s:
        s.Render()
        s.trace_sun(s_dir, su.TAU, bias=su.B10)
        s.trace_suns([s_dir], su.TAU, bias=su.B10)
        s.PostProcess()
        img = s.download_image()
        s.light_image_sun(s_dir, ambient=0.25)
        one = s.download_image()
        s.PostProcess()
        assert np.array_equal(s.download_image(), img)
        s.light_image_suns([s_dir], [1.0], ambient=0.25)
        many = s.download_image()
        assert np.array_equal(np.where(s.download_shadow_masks() & U1, 255, 0), s.download_shadow())
    assert np.array_equal(one, many) and (one != img).any()


# 10 --------------------------------------------------------------------------------------------------
def test_error_codes():
    import torch
    Lb = sf.lib()
    pos = torch.zeros((36, 64, 4), dtype=torch.float32, device="cuda")
    out = torch.full((36 * 64,), 9, dtype=torch.int64, device="cuda")
    img = torch.full((36 * 64 * 4,), 9, dtype=torch.uint8, device="cuda")
    pp, op, ip = (ctypes.c_void_p(t.data_ptr()) for t in (pos, out, img))
    three = lights.sun_cone((0.0, 0.6, 0.8), ss.HALF_ANGLE, 3)
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    keep = []

    def P(w=0, h=0, bias=su.B10, max_depth=0, n=3, dirs=three, weights=None, distance=4.0):
        p = sf.sf_suns_params()
        if dirs is not None:
            p.dirs = fp(dirs)
        if weights is not None:
            wa = np.asarray(weights, np.float32)
            keep.append(wa)
            p.weights = fp(wa)
        p.n, p.distance, p.bias, p.width, p.height, p.max_depth = n, distance, bias, w, h, max_depth
        return ctypes.byref(p)

    many = np.tile(np.array([[0.0, 0.6, 0.8]], np.float32), (65, 1))
    with sf.Sphereflake(64, 36) as s:
        d = sf.sf_suns_params()
        d.n = 5
        assert Lb.sf_suns_defaults(s.ctx, ctypes.byref(d)) == sf.SF_OK and Lb.sf_suns_defaults(s.ctx, None) == sf.SF_EINVAL
        assert (bool(d.dirs), bool(d.weights), d.n, d.distance, d.bias) == (False, False, 0, 4.0, 2.0 ** -10)
        assert (d.use_origin, d.width, d.height, d.max_depth, d.stream) == (0, 0, 0, 0, None)
        assert Lb.sf_trace_suns_to(s.ctx, P(64, 36), pp, op) == sf.SF_ENOVIEW
        assert Lb.sf_trace_suns(s.ctx, P()) == sf.SF_ENOVIEW
        S = pyoracle.load_setup("t1")
        s.SetView(S["origin"], S["tl"], S["tr"], S["bl"])
        for call in (lambda p: Lb.sf_trace_suns_to(s.ctx, p, pp, op),
                     lambda p: Lb.sf_light_image_suns(s.ctx, p, 0.25, pp, pp, op, ip)):
            assert call(P(64, 36, n=0)) == sf.SF_EINVAL
            assert call(P(64, 36, n=65, dirs=many)) == sf.SF_EINVAL
            assert call(P(64, 36, dirs=None)) == sf.SF_EINVAL
        assert Lb.sf_trace_suns_to(s.ctx, P(64, 36), pp, None) == sf.SF_EINVAL
        for bias in (-0.25, 1.0, 2.0, float("nan")):
            assert Lb.sf_trace_suns_to(s.ctx, P(64, 36, bias=bias), pp, op) == sf.SF_EINVAL
        for distance in (0.0, -4.0, float("inf"), float("nan")):
            assert Lb.sf_trace_suns_to(s.ctx, P(64, 36, distance=distance), pp, op) == sf.SF_EINVAL
            assert Lb.sf_trace_suns(s.ctx, P(distance=distance)) == sf.SF_EINVAL
        assert Lb.sf_trace_suns_to(s.ctx, P(64, 36, max_depth=32), pp, op) == sf.SF_EINVAL
        assert Lb.sf_trace_suns_to(s.ctx, P(32, 16), None, op) == sf.SF_EINVAL   # sizes against a NULL pos4
        assert Lb.sf_trace_suns_to(s.ctx, P(64, 0), pp, op) == sf.SF_EINVAL
        assert Lb.sf_trace_suns(s.ctx, P(32, 16)) == sf.SF_EINVAL
        assert Lb.sf_trace_suns_to(None, P(64, 36), pp, op) == sf.SF_EINVAL
        assert Lb.sf_trace_suns_to(s.ctx, None, pp, op) == sf.SF_EINVAL
        assert Lb.sf_light_image_suns(s.ctx, None, 0.25, pp, pp, op, ip) == sf.SF_EINVAL
        for wts in ((0.5, -0.5, 0.5), (float("nan"), 1.0, 1.0)):
            assert Lb.sf_light_image_suns(s.ctx, P(weights=wts), 0.25, pp, pp, op, ip) == sf.SF_EINVAL
        for amb in (-0.1, 1.5, float("nan")):
            assert Lb.sf_light_image_suns(s.ctx, P(), amb, pp, pp, op, ip) == sf.SF_EINVAL
        assert Lb.sf_light_image_suns(s.ctx, P(), 0.25, None, None, None, None) == sf.SF_ESTATE   # no image, no masks
        s.Synchronize()
        assert (out == 9).all() and (img == 9).all()   # none of them wrote
        # a negative weight does not bother the trace, which ignores the weights; an all-miss position image: every
        # mask has exactly its low n bits set, no ray
        assert Lb.sf_trace_suns_to(s.ctx, P(64, 36, weights=(0.5, -0.5, 0.5)), pp, op) == sf.SF_OK
        s.Synchronize()
        assert (out == 7).all()
        assert s.stats().rays == 0
        with pytest.raises(ValueError):
            s.trace_suns(many, pos=(pos.data_ptr(), 64, 36), out=out)
        with pytest.raises(ValueError):
            s.trace_suns(np.zeros((0, 3), np.float32), pos=(pos.data_ptr(), 64, 36), out=out)
