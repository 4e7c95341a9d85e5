"""Sky reflections on the GPU (sf_trace_mirror_to / sf_trace_mirror / sf_trace_mirror_sum_to / sf_trace_mirror_sum): a
lobe of rays about each pixel's mirror direction, formed on the device. Bit i of every surface pixel's word equals the
CPU oracle's answer for the ray lights.mirror_model states (tests/mirrorcheck.py); the mask equals trace_ao on the host's
image of mirror axes; the sum equals lights.mirror_sum_model. Everything is compared bit for bit."""
import ctypes

import numpy as np
import pytest

import sphereflake_amd as sf
from sphereflake_amd import lights
from dirscheck import same_bits
from lightsumcheck import BASE, assert_same, base_image, colours, surface_of
from oracle import pyoracle
from rayscheck import frame
import aocheck as ac
import mirrorcheck as mc
from aospincheck import assert_mask, assert_shape_of_mask, flake

pytestmark = pytest.mark.gpu

F = np.float32
KW = dict(distance=ac.TAU, bias=ac.B10)
SKY = dict(zenith=mc.ZENITH, horizon=mc.HORIZON, up=mc.UP)
S4, LOBE8, LOBE64 = mc.S4, mc.LOBE8, mc.LOBE64


@pytest.fixture(scope="module", autouse=True)
def device():
    sf.build()
    assert sf.device_count() >= 1, "no HIP device visible: GPU tests must run on an MI355X"


def even(n):
    return np.full((n, 3), F(1.0) / F(n), F)


# 1 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", [("t1", "avx"), ("t3", "avx"), ("t1", "sse"), ("t3", "sse")])
def test_masks_equal_the_oracle(name, variant):
    """The oracle's own frame uploaded; every surface pixel (830 on t1, 3600 on t3) and every miss of the frame: the
    mirror ray alone, lobe_samples(8, 8) spun 4 x 4, and 64 unspun samples (bit 63)."""
    ref = frame(name, variant)
    pos, nrm = ref["pos4"], ref["nrm4"]
    surf = surface_of(pos)
    with flake(name, variant) as s:
        for what, h, spin in (("mirror ray", mc.MIRROR, None), ("lobe 8 spun", LOBE8, S4), ("lobe 64", LOBE64, None)):
            want, _ = mc.oracle_mask(name, h, spin, variant=variant)
            got = s.trace_mirror(h, pos=pos, nrm=nrm, spin=spin, **KW)
            assert_mask(got, want, f"{name} {variant} {what}")
            assert_shape_of_mask(got, len(h), pos, f"{name} {variant} {what}")
            for i in {0, len(h) - 1}:   # both outcomes show, also in bit 63
                assert int((surf & ac.bit(got, i)).sum()) >= 100 and int((surf & ~ac.bit(got, i)).sum()) >= 100, (what, i)


# 2 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t1", "t3"])
@pytest.mark.parametrize("spin", [None, S4], ids=["unspun", "spun"])
def test_the_mask_is_trace_ao_on_the_axes_image(name, spin):
    ref = frame(name)
    pos, nrm = ref["pos4"], ref["nrm4"]
    axes = mc.axes(name)
    with flake(name) as s:
        got = s.trace_mirror(LOBE8, pos=pos, nrm=nrm, spin=spin, **KW)
        want = s.trace_ao(LOBE8, pos=pos, nrm=axes, spin=spin, **KW)
        about_n = s.trace_ao(LOBE8, pos=pos, nrm=nrm, spin=spin, **KW)
    assert_mask(got, want, f"{name} against trace_ao on mirror_axes")
    assert 2 * int((got != about_n).sum()) > int(surface_of(pos).sum())   # (not the normal's hemisphere)


# 3 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t1", "t3"])
def test_the_sum_equals_the_model(name):
    S = pyoracle.load_setup(name)
    ref = frame(name)
    pos, nrm = ref["pos4"], ref["nrm4"]
    surf = surface_of(pos)
    axes = mc.axes(name)
    with flake(name) as s:
        for n, h, spin in ((8, LOBE8, S4), (33, LOBE64[:33], None), (64, LOBE64, None)):
            col = colours(n)
            mask = s.trace_mirror(h, pos=pos, nrm=nrm, spin=spin, **KW)
            got = s.trace_mirror_sum(h, col, pos=pos, nrm=nrm, spin=spin, **SKY, **KW)
            want = lights.mirror_sum_model(None, pos, nrm, S["origin"], mask, h, col, spin=spin, **SKY)
            assert_same(got, want, f"{name} n = {n}, the gradient")
            assert (got[~surf] == 0).all() and (got[..., 3] == 0).all()
            # a white sky: trace_ao_sum on the axes image
            white = s.trace_mirror_sum(h, col, pos=pos, nrm=nrm, spin=spin, **KW)
            assert_same(white, s.trace_ao_sum(h, col, pos=pos, nrm=axes, spin=spin, **KW), f"{name} n = {n}, white")
            assert not same_bits(white[surf], got[surf])   # (the gradient shows)
        assert len(np.unique(got[surf][:, 0])) > 100
        # a call equals its split, also onto a seeded base that carries .w; misses are zeroed or left
        col = colours(8)
        kw = dict(pos=pos, nrm=nrm, spin=S4, **SKY, **KW)
        whole = s.trace_mirror_sum(LOBE8, col, **kw)
        for k in (1, 3, 7):
            first = s.trace_mirror_sum(LOBE8[:k], col[:k], **kw)
            both = s.trace_mirror_sum(LOBE8[k:], col[k:], accumulate=True, out=first, **kw)
            assert_same(both, whole, f"{name} split at {k}")
        base = base_image(pos.shape[:2])
        acc = s.trace_mirror_sum(LOBE8, col, accumulate=True, out=base, **kw)
        mask = s.trace_mirror(LOBE8, pos=pos, nrm=nrm, spin=S4, **KW)
    assert_same(acc, lights.mirror_sum_model(base, pos, nrm, S["origin"], mask, LOBE8, col, accumulate=True, spin=S4,
                                             **SKY), f"{name} accumulating")
    assert (acc[..., 3] == F(BASE[3])).all() and same_bits(acc[~surf], base[~surf])
    assert (whole[~surf] == 0).all() and (acc[surf][:, :3] != base[surf][:, :3]).any()


# 4 ---------------------------------------------------------------------------------------------------
def test_overflow_tiles_are_retraced_once():
    """max_depth = 4 on t3 provisions too few levels: overflow_tiles moves, the mask and the overwriting sum stay, and
    the accumulating sum is not added twice."""
    ref = frame("t3")
    pos, nrm = ref["pos4"], ref["nrm4"]
    col = colours(8)
    kw = dict(pos=pos, nrm=nrm, spin=S4, **KW)
    want, _ = mc.oracle_mask("t3", LOBE8, S4)
    with flake("t3") as s:
        mask = s.trace_mirror(LOBE8, **kw)
        whole = s.trace_mirror_sum(LOBE8, col, **SKY, **kw)
        base = base_image(pos.shape[:2])
        acc = s.trace_mirror_sum(LOBE8, col, accumulate=True, out=base, **SKY, **kw)
        o0 = s.stats().overflow_tiles
        shallow = s.trace_mirror(LOBE8, max_depth=4, **kw)
        o1 = s.stats().overflow_tiles
        shallow_sum = s.trace_mirror_sum(LOBE8, col, max_depth=4, **SKY, **kw)
        shallow_acc = s.trace_mirror_sum(LOBE8, col, accumulate=True, out=base, max_depth=4, **SKY, **kw)
        o2 = s.stats().overflow_tiles
    print("flagged tiles:", o1 - o0, "then", o2 - o1, "over two summing launches")
    assert 1 <= o1 - o0 <= 60 and o2 - o1 == 2 * (o1 - o0)
    assert_mask(mask, want, "max_depth = 0 against the oracle")
    assert_mask(shallow, mask, "max_depth = 4, the mask")
    assert_same(shallow_sum, whole, "max_depth = 4, the overwriting sum")
    assert_same(shallow_acc, acc, "max_depth = 4, the accumulating sum")
    assert (acc[surface_of(pos)][:, :3] != base[surface_of(pos)][:, :3]).any()


# 5 ---------------------------------------------------------------------------------------------------
def test_eye():
    """A displaced eye follows the model and the oracle; no eye is V = P, which is not the eye == origin form."""
    S = pyoracle.load_setup("t3")
    ref = frame("t3")
    pos, nrm = ref["pos4"], ref["nrm4"]
    surf = surface_of(pos)
    eye = mc.eye_of("t3")
    col = colours(8)
    o = np.asarray(S["origin"], F)
    with flake("t3") as s:
        plain = s.trace_mirror(LOBE8, pos=pos, nrm=nrm, spin=S4, **KW)
        moved = s.trace_mirror(LOBE8, pos=pos, nrm=nrm, spin=S4, eye=eye, **KW)
        moved_ao = s.trace_ao(LOBE8, pos=pos, nrm=mc.axes("t3", eye=eye), spin=S4, **KW)
        moved_sum = s.trace_mirror_sum(LOBE8, col, pos=pos, nrm=nrm, spin=S4, eye=eye, **SKY, **KW)
        # V = P or (o + P) - o: the mirror ray alone (s = A) with colour 1, horizon 0 and zenith 1 sums to
        # clamp(A . up, 0, 1) where the ray is open, so up = +-x, +-y, +-z read the device's axis out, bit for bit
        probe = np.array([[0.0, 0.0, 1.0]], F)
        one = np.ones((1, 3), F)
        axis_bits, open_ray = {}, {}
        for key, e in (("none", None), ("origin", o)):
            chans = [s.trace_mirror_sum(probe, one, zenith=(1, 1, 1), horizon=(0, 0, 0), up=up, pos=pos, nrm=nrm, eye=e,
                                        **KW)[..., 0] for up in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0),
                                                                 (0, 0, -1))]
            axis_bits[key] = np.stack(chans, -1)
            open_ray[key] = ac.bit(s.trace_mirror(probe, pos=pos, nrm=nrm, eye=e, **KW), 0)
    assert_mask(moved, mc.oracle_mask("t3", LOBE8, S4, eye)[0], "the displaced eye against the oracle")
    assert_mask(moved, moved_ao, "the displaced eye against trace_ao on its axes")
    assert int((surf & (moved != plain)).sum()) == 3020
    assert_same(moved_sum, lights.mirror_sum_model(None, pos, nrm, S["origin"], moved, LOBE8, col, spin=S4, eye=eye,
                                                   **SKY), "the displaced eye, summed")
    # the device's axis where the mirror ray is open: max(A, 0) and max(-A, 0) per component, bit for bit
    for key, e in (("none", None), ("origin", o)):
        A = lights.mirror_axes(pos, nrm, o, e)[..., :3]
        with np.errstate(invalid="ignore"):
            want = np.concatenate([np.where(A > 0, np.minimum(A, F(1)), F(0)), np.where(-A > 0, np.minimum(-A, F(1)), F(0))],
                                  -1).astype(F)
        pick = surf & open_ray[key]
        closed = surf & ~open_ray[key]
        print(key, "open", int(pick.sum()), "rows that differ", int((axis_bits[key][pick] != want[pick]).any(-1).sum()))
        assert int(pick.sum()) >= 1500
        assert same_bits(axis_bits[key][pick], want[pick]), key
        assert (axis_bits[key][closed] == 0).all()   # (a closed ray adds nothing)
    pick = surf & open_ray["none"] & open_ray["origin"]
    assert int((axis_bits["none"][pick] != axis_bits["origin"][pick]).any(-1).sum()) >= 1000   # other bits


# 6 ---------------------------------------------------------------------------------------------------
def test_crop():
    """A 13 x 11 crop of t3 at (32, 16) (partial tiles both ways, the corner at multiples of the 4 x 4 table) equals the
    crop of the whole; as numpy arrays, and as torch tensors with guard words before and after both outputs."""
    import torch
    S = pyoracle.load_setup("t3")
    ref = frame("t3")
    x0, y0, w, h = 32, 16, 13, 11
    pos = np.ascontiguousarray(ref["pos4"][y0:y0 + h, x0:x0 + w])
    nrm = np.ascontiguousarray(ref["nrm4"][y0:y0 + h, x0:x0 + w])
    col = colours(8)
    guard, sentinel, fsentinel = 8, 0x5a5a5a5a5a5a5a5a, -123.25
    with flake("t3") as s:
        sub = s.trace_mirror(LOBE8, pos=ref["pos4"], nrm=ref["nrm4"], spin=S4, **KW)[y0:y0 + h, x0:x0 + w]
        sub_sum = np.ascontiguousarray(
            s.trace_mirror_sum(LOBE8, col, pos=ref["pos4"], nrm=ref["nrm4"], spin=S4, **SKY, **KW)[y0:y0 + h, x0:x0 + w])
        assert len(np.unique(sub)) >= 3
        assert_mask(s.trace_mirror(LOBE8, pos=pos, nrm=nrm, spin=S4, **KW), sub, "numpy crop")
        assert_same(s.trace_mirror_sum(LOBE8, col, pos=pos, nrm=nrm, spin=S4, **SKY, **KW), sub_sum, "numpy crop, summed")
        pt, nt = torch.from_numpy(pos).cuda(), torch.from_numpy(nrm).cuda()
        out = torch.full((guard + h * w + guard,), sentinel, dtype=torch.int64, device="cuda")
        fout = torch.full((2 * guard + h * w * 4 + 2 * guard,), fsentinel, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        s.trace_mirror(LOBE8, pos=pt, nrm=nt, out=out.data_ptr() + 8 * guard, spin=S4, **KW)
        s.trace_mirror_sum(LOBE8, col, pos=pt, nrm=(nt.data_ptr(), w, h), out=fout.data_ptr() + 8 * guard, spin=S4,
                           **SKY, **KW)
        s.Synchronize()
        o = out.cpu().numpy().view(np.uint64)
        assert (o[:guard] == np.uint64(sentinel)).all(), "wrote before the first pixel"
        assert (o[guard + h * w:] == np.uint64(sentinel)).all(), "wrote past the last pixel"
        assert_mask(o[guard:guard + h * w].reshape(h, w), sub, "torch crop")
        fo = fout.cpu().numpy()
        assert (fo[:2 * guard] == F(fsentinel)).all() and (fo[2 * guard + h * w * 4:] == F(fsentinel)).all(), "guards"
        assert_same(fo[2 * guard:2 * guard + h * w * 4].reshape(h, w, 4), sub_sum, "torch crop, summed")


# 7 ---------------------------------------------------------------------------------------------------
def test_nan_normal():
    """A NaN normal sets all n bits of its pixel and touches no other; the sum there is the model's (every entry open,
    the sky's colour at t = 0: the horizon's)."""
    S = pyoracle.load_setup("t3")
    ref = frame("t3")
    pos = ref["pos4"]
    nrm = np.array(ref["nrm4"], F, copy=True)
    y, x = 22, 40
    assert surface_of(pos)[y, x]
    nrm[y, x, 1] = np.nan
    col = colours(8)
    with flake("t3") as s:
        clean = s.trace_mirror(LOBE8, pos=pos, nrm=ref["nrm4"], spin=S4, **KW)
        got = s.trace_mirror(LOBE8, pos=pos, nrm=nrm, spin=S4, **KW)
        summed = s.trace_mirror_sum(LOBE8, col, pos=pos, nrm=nrm, spin=S4, **SKY, **KW)
    assert got[y, x] == np.uint64(0xff) and clean[y, x] != np.uint64(0xff)
    other = np.ones(got.shape, bool)
    other[y, x] = False
    assert_mask(got, clean, "every other pixel", other)
    want = lights.mirror_sum_model(None, pos, nrm, S["origin"], got, LOBE8, col, spin=S4, **SKY)
    assert_same(summed, want, "the sum under a NaN normal")
    hz = np.zeros(3, F)
    for i in range(8):
        hz = hz + col[i] * np.array(mc.HORIZON, F)
    assert same_bits(summed[y, x, :3], hz)


# 8 ---------------------------------------------------------------------------------------------------
def test_context_form_and_error_codes():
    """Render -> trace_ao_sum -> trace_mirror_sum(accumulate=True) -> light_image_buffer on the context's own buffers:
    the buffer and the image are the models chained, the light buffer's pointer stays, no statistic moves; then the
    error codes, and a refused call wrote nothing."""
    import torch
    hs = lights.ao_samples(8)
    acol = lights.ao_colours(hs, (0.5, 0.75, 1.0))
    col = colours(8)
    with flake("t3") as s:
        s.Render()
        s.PostProcess()
        img = s.download_image()
        pos, nrm, _, _ = s.download()
        st0 = s.stats()
        before = (st0.max_depth, np.float32(st0.closest), st0.rays, st0.overflow_tiles)
        assert s.trace_ao_sum(hs, acol, spin=S4, **KW) is None
        ptr = s.light_buffer()
        diffuse = s.download_light()
        assert s.trace_mirror_sum(LOBE8, col, accumulate=True, spin=S4, **SKY, **KW) is None
        assert s.light_buffer() == ptr != 0
        buf = s.download_light()
        assert s.trace_mirror(LOBE8, spin=S4, **KW) is None
        mask = s.download_shadow_masks()
        s.light_image_buffer()
        got = s.download_image()
        st = s.stats()
        assert (st.max_depth, np.float32(st.closest), st.rays, st.overflow_tiles) == before
        origin = pyoracle.load_setup("t3")["origin"]
        assert_mask(mask, s.trace_mirror(LOBE8, pos=pos, nrm=nrm, spin=S4, **KW), "the context's mask buffer")
    assert_same(buf, lights.mirror_sum_model(diffuse, pos, nrm, origin, mask, LOBE8, col, accumulate=True, spin=S4,
                                             **SKY), "the buffer")
    assert (buf[surface_of(pos)][:, :3] != diffuse[surface_of(pos)][:, :3]).any()
    assert np.array_equal(got, lights.light_model_buffer(img, pos, buf)) and (got != img).any()

    Lb = sf.lib()
    dpos = torch.zeros((36, 64, 4), dtype=torch.float32, device="cuda")
    out = torch.full((36 * 64,), 9, dtype=torch.int64, device="cuda")
    fout = torch.full((36 * 64 * 4,), 9.0, dtype=torch.float32, device="cuda")
    pp, op, fp_ = (ctypes.c_void_p(t.data_ptr()) for t in (dpos, out, fout))
    three = lights.lobe_samples(3, 8)
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    keep = []

    def P(w=0, h=0, n=3, samples=three, cols=None, accumulate=0, **fields):
        p = sf.sf_mirror_params()
        assert Lb.sf_mirror_defaults(s2.ctx, ctypes.byref(p)) == sf.SF_OK
        assert (p.distance, p.bias, p.use_eye, p.n) == (4.0, 2.0 ** -10, 0, 0)
        assert (tuple(p.zenith), tuple(p.horizon), tuple(p.up)) == ((1, 1, 1), (1, 1, 1), (0, 0, 1))
        if samples is not None:
            p.samples = fp(samples)
        if cols is not None:
            ca = np.ascontiguousarray(cols, np.float32)
            keep.append(ca)
            p.colours = fp(ca)
        p.n, p.width, p.height, p.accumulate = n, w, h, accumulate
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(p, k)[:] = v
            else:
                setattr(p, k, v)
        return ctypes.byref(p)

    def T(size=4, table=S4, null=False):
        sp = sf.sf_ao_spin()
        if not null:
            t = np.ascontiguousarray(table, np.float32)
            keep.append(t)
            sp.cs = fp(t)
        sp.size = size
        keep.append(sp)
        return ctypes.byref(sp)

    many = np.tile(np.array([[0.0, 0.6, 0.8]], np.float32), (65, 1))
    nan, inf = float("nan"), float("inf")
    with sf.Sphereflake(64, 36) as s2:
        mask_to = lambda p, t=None, a=pp, b=pp, c=op: Lb.sf_trace_mirror_to(s2.ctx, p, t, a, b, c)
        sum_to = lambda p, t=None, a=pp, b=pp, c=fp_: Lb.sf_trace_mirror_sum_to(s2.ctx, p, t, a, b, c)
        own_mask = lambda p, t=None: Lb.sf_trace_mirror(s2.ctx, p, t)
        own_sum = lambda p, t=None: Lb.sf_trace_mirror_sum(s2.ctx, p, t)
        assert mask_to(P(64, 36)) == sf.SF_ENOVIEW and sum_to(P(64, 36)) == sf.SF_ENOVIEW
        assert own_mask(P()) == sf.SF_ENOVIEW and own_sum(P()) == sf.SF_ENOVIEW
        S = pyoracle.load_setup("t1")
        s2.SetView(S["origin"], S["tl"], S["tr"], S["bl"])
        for call, own in ((mask_to, own_mask), (sum_to, own_sum)):
            # everything the spun AO call rejects, but a null spin
            assert call(P(64, 36, n=0)) == sf.SF_EINVAL and own(P(n=0)) == sf.SF_EINVAL
            assert call(P(64, 36, n=65, samples=many)) == sf.SF_EINVAL and own(P(n=65, samples=many)) == sf.SF_EINVAL
            assert call(P(64, 36, samples=None)) == sf.SF_EINVAL and own(P(samples=None)) == sf.SF_EINVAL
            for bias in (-0.25, 1.0, 2.0, nan):
                assert call(P(64, 36, bias=bias)) == sf.SF_EINVAL
            for distance in (0.0, -4.0, inf, nan):
                assert call(P(64, 36, distance=distance)) == sf.SF_EINVAL and own(P(distance=distance)) == sf.SF_EINVAL
            assert call(P(64, 36, max_depth=32)) == sf.SF_EINVAL
            assert call(P(64, 0)) == sf.SF_EINVAL
            assert call(P(32, 16), None, None) == sf.SF_EINVAL        # sizes against a NULL pos4
            assert call(P(32, 16), None, pp, None) == sf.SF_EINVAL    # ... a NULL nrm4
            assert call(None) == sf.SF_EINVAL and own(None) == sf.SF_EINVAL
            assert own(P(32, 16)) == sf.SF_EINVAL
            assert call(P(64, 36), T(null=True)) == sf.SF_EINVAL and own(P(), T(null=True)) == sf.SF_EINVAL
            assert call(P(64, 36), T(size=0)) == sf.SF_EINVAL and own(P(), T(size=9)) == sf.SF_EINVAL
            t = np.array(S4, np.float32, copy=True)
            t[3, 2, 1] = nan
            assert call(P(64, 36), T(table=t)) == sf.SF_EINVAL and own(P(), T(table=t)) == sf.SF_EINVAL
            # the eye, under use_eye only
            for bad in (nan, inf, -inf):
                assert call(P(64, 36, eye=(0.0, bad, 0.0), use_eye=1)) == sf.SF_EINVAL
                assert own(P(eye=(0.0, bad, 0.0), use_eye=1)) == sf.SF_EINVAL
        assert mask_to(P(64, 36), None, pp, pp, None) == sf.SF_EINVAL          # a null mask
        assert sum_to(P(32, 16), None, pp, pp, None) == sf.SF_EINVAL           # sizes against a NULL out
        for bad in (-0.5, nan, inf):
            cols = [(0.5, 0.5, 0.5), (0.5, bad, 0.5), (0.5, 0.5, 0.5)]
            assert sum_to(P(64, 36, cols=cols)) == sf.SF_EINVAL and own_sum(P(cols=cols)) == sf.SF_EINVAL
            for field in ("zenith", "horizon"):
                assert sum_to(P(64, 36, **{field: (1.0, 1.0, bad)})) == sf.SF_EINVAL
                assert own_sum(P(**{field: (bad, 1.0, 1.0)})) == sf.SF_EINVAL
        for bad in (nan, inf, -inf):
            assert sum_to(P(64, 36, up=(0.0, bad, 1.0))) == sf.SF_EINVAL and own_sum(P(up=(bad, 0.0, 1.0))) == sf.SF_EINVAL
        # an accumulating call, or a null out, before the light buffer exists
        assert sum_to(P(64, 36), None, pp, pp, None) == sf.SF_ESTATE
        assert sum_to(P(64, 36, accumulate=1), None, pp, pp, None) == sf.SF_ESTATE
        assert own_sum(P(accumulate=1)) == sf.SF_ESTATE
        assert s2.light_buffer() == 0 and s2.shadow_mask_buffer() == 0   # (a refused call made no buffer)
        s2.Synchronize()
        assert (out == 9).all() and (fout == 9).all()   # none of them wrote
        # what the mask call does not read is not checked there: a NaN eye without use_eye, the gradient
        assert mask_to(P(64, 36, eye=(nan, nan, nan), zenith=(nan, -1.0, inf), up=(nan, 0.0, 0.0))) == sf.SF_OK
        assert sum_to(P(64, 36, accumulate=1, eye=(nan, nan, nan)), T()) == sf.SF_OK
        s2.Synchronize()
        assert (out == 7).all() and (fout == 9).all()   # an all-miss image: low n bits set; an accumulating sum leaves it
        assert sum_to(P(64, 36)) == sf.SF_OK
        s2.Synchronize()
        assert (fout == 0).all() and s2.stats().rays == 0
        dev = (dpos.data_ptr(), 64, 36)
        with pytest.raises(ValueError):
            s2.trace_mirror(three, pos=dev, nrm=dev, out=out, spin=np.zeros((9, 9, 2), np.float32))
        with pytest.raises(ValueError):
            s2.trace_mirror(three, pos=dev, out=out)   # a device pos without a device nrm


# 9 ---------------------------------------------------------------------------------------------------
def test_convergence():
    """t3, lobe exponent 8, the gradient, colours 1 / n, red channel, RMS against n = 64, all unspun: the error falls
    from n = 4 to 8 to 16 (the oracle gives 0.109 > 0.071 > 0.047)."""
    ref = frame("t3")
    pos, nrm = ref["pos4"], ref["nrm4"]
    surf = surface_of(pos)
    with flake("t3") as s:
        best = s.trace_mirror_sum(LOBE64, even(64), pos=pos, nrm=nrm, **SKY, **KW)
        err = [mc.red_rms(s.trace_mirror_sum(lights.lobe_samples(n, 8), even(n), pos=pos, nrm=nrm, **SKY, **KW), best, surf)
               for n in (16, 8, 4)]
    print("RMS against n = 64 at n = 16, 8, 4:", err)
    assert err[0] < err[1] < err[2]
