"""The edge-aware box filter of the light buffer on the GPU (sf_light_filter_to / sf_light_filter): it equals
sphereflake_amd.lights.light_filter_model bit for bit on the spun n = 4 sums of the fixtures, copies misses, carries
.w, follows the NaN rules of its definition, and -- what it is for -- four spun and filtered rays per pixel come closer to
64 rays than eight plain ones do."""
import ctypes

import numpy as np
import pytest

import sphereflake_amd as sf
from sphereflake_amd import lights
from lightsumcheck import BASE, assert_same, base_image, surface_of
from rayscheck import frame
import aocheck as ac
import aospincheck as sc
from aospincheck import flake

pytestmark = pytest.mark.gpu

F = np.float32
H4 = sc.H4
S4 = lights.ao_spins(4)
KW = dict(distance=ac.TAU, bias=ac.B10)
SIZES = (1, 2, 3, 4, 8)


@pytest.fixture(scope="module", autouse=True)
def device():
    sf.build()
    assert sf.device_count() >= 1, "no HIP device visible: GPU tests must run on an MI355X"


def spun_sum(s, name, base=None):
    """The spun n = 4 sum of fixture `name`'s own frame, colours 1 / n (onto `base` where given)."""
    ref = frame(name)
    if base is None:
        return s.trace_ao_sum(H4, None, pos=ref["pos4"], nrm=ref["nrm4"], spin=S4, **KW)
    return s.trace_ao_sum(H4, None, accumulate=True, out=base, pos=ref["pos4"], nrm=ref["nrm4"], spin=S4, **KW)


# 11 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t1", "t3"])
def test_the_filter_equals_the_model(name):
    """Sizes 1 (a copy), 2, 3, 4, 8 under the default thresholds and the two other candidates."""
    ref = frame(name)
    pos, nrm = ref["pos4"], ref["nrm4"]
    surf = surface_of(pos)
    if name == "t3":   # every window shape is exercised
        cnt = sc.accepted_counts(pos, nrm, 4)
        hist = [int(((cnt == k) & surf).sum()) for k in range(1, 17)]
        print("accepted-tap counts 1..16", hist)
        assert min(hist) >= 50
    with flake(name) as s:
        buf = spun_sum(s, name)
        assert 3 <= len(np.unique(buf[surf][:, 0])) <= 5   # (k / 4: the filter has something to average)
        for size in SIZES:
            for nmin, pmax in sc.THRESHOLDS:
                got = s.light_filter(size, nmin, pmax, pos=pos, nrm=nrm, buf=buf)
                assert_same(got, lights.light_filter_model(buf, pos, nrm, size, nmin, pmax), f"{name} {size} {nmin} {pmax}")
                if size == 1:
                    assert_same(got, buf, f"{name}: size 1 is a copy")
        got = s.light_filter(pos=pos, nrm=nrm, buf=buf)   # the defaults: 4, 0.9, 0.02
        assert_same(got, lights.light_filter_model(buf, pos, nrm, 4), f"{name} defaults")
        assert len(np.unique(got[surf][:, 0])) > 30 and (got[~surf] == 0).all()


# 12 --------------------------------------------------------------------------------------------------
def test_misses_w_crop_and_guards():
    """Misses are copied, .w is carried from a non-zero base, a 13 x 11 crop equals the model of the crop (its window
    is clipped at the crop's edge: it is not the crop of the whole), guard words around a torch output are intact."""
    import torch
    y0, x0, h, w = 17, 30, 11, 13
    guard, fsentinel = 8, -123.25
    one = frame("t1")   # (t1 has the misses: 830 of its 2304 pixels are surface; every pixel of t3 is)
    pos, nrm = one["pos4"], one["nrm4"]
    miss = ~surface_of(pos)
    with flake("t1") as s:
        base = base_image(pos.shape[:2])
        base[..., 3] += np.arange(base.shape[0] * base.shape[1], dtype=F).reshape(base.shape[:2])   # a .w per pixel
        buf = spun_sum(s, "t1", base)
        got = s.light_filter(4, pos=pos, nrm=nrm, buf=buf)
        assert_same(got, lights.light_filter_model(buf, pos, nrm, 4), "whole, on a base")
        assert int(miss.sum()) >= 100 and np.array_equal(got[miss].view(np.uint32), buf[miss].view(np.uint32))
        assert (got[miss][:, :3] == np.array(BASE[:3], F)).all()
        assert np.array_equal(got[..., 3], buf[..., 3]) and (got[..., 3] == base[..., 3]).all()
        assert (got[~miss][:, :3] != buf[~miss][:, :3]).any()
    ref = frame("t3")
    pos, nrm = ref["pos4"], ref["nrm4"]
    with flake("t3") as s:
        buf = spun_sum(s, "t3", base_image(pos.shape[:2]))
        got = s.light_filter(4, pos=pos, nrm=nrm, buf=buf)
        cp, cn, cb = (np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w]) for a in (pos, nrm, buf))
        want = lights.light_filter_model(cb, cp, cn, 4)
        assert_same(s.light_filter(4, pos=cp, nrm=cn, buf=cb), want, "numpy crop")
        assert not np.array_equal(want, got[y0:y0 + h, x0:x0 + w])   # (clipped: not the crop of the whole)
        pt, nt, bt = (torch.from_numpy(a).cuda() for a in (cp, cn, cb))
        fout = torch.full((2 * guard + h * w * 4 + 2 * guard,), fsentinel, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        s.light_filter(4, pos=pt, nrm=(nt.data_ptr(), w, h), buf=bt, out=fout.data_ptr() + 8 * guard)
        s.Synchronize()
        fo = fout.cpu().numpy()
        assert (fo[:2 * guard] == F(fsentinel)).all() and (fo[2 * guard + h * w * 4:] == F(fsentinel)).all(), "guards"
        assert_same(fo[2 * guard:2 * guard + h * w * 4].reshape(h, w, 4), want, "torch crop")
        assert np.array_equal(bt.cpu().numpy().view(np.uint32), cb.view(np.uint32))   # the input is not written


# 13 --------------------------------------------------------------------------------------------------
def test_nan_rules():
    """A NaN normal at q removes q from its neighbours' sums and leaves q averaging itself alone; a NaN light value
    spreads exactly to the pixels whose accepted window holds it."""
    ref = frame("t3")
    pos = ref["pos4"]
    cnt = sc.accepted_counts(pos, ref["nrm4"], 4)
    q = tuple(np.argwhere(cnt == 16)[60])   # a pixel inside a smooth patch
    nrm = np.array(ref["nrm4"], F, copy=True)
    nrm[q][1] = np.nan
    with flake("t3") as s:
        buf = spun_sum(s, "t3")
        clean = s.light_filter(4, pos=pos, nrm=ref["nrm4"], buf=buf)
        got = s.light_filter(4, pos=pos, nrm=nrm, buf=buf)
        assert_same(got, lights.light_filter_model(buf, pos, nrm, 4), "a NaN normal")
        assert np.array_equal(got[q].view(np.uint32), buf[q].view(np.uint32)) and np.isfinite(got).all()
        near = np.zeros(pos.shape[:2], bool)
        near[q[0] - 1:q[0] + 3, q[1] - 1:q[1] + 3] = True   # the pixels whose -2 .. +1 window holds q
        changed = (got.view(np.uint32) != clean.view(np.uint32)).any(-1)
        assert not (changed & ~near).any()
        # a value only q holds: its neighbours see it through the clean normals and not past the NaN one
        loud = np.array(buf, F, copy=True)
        loud[q][0] = 100.0
        seen = s.light_filter(4, pos=pos, nrm=ref["nrm4"], buf=loud)[..., 0] > 2
        assert seen[q] and 2 <= int(seen.sum()) <= 16 and not (seen & ~near).any()
        alone = s.light_filter(4, pos=pos, nrm=nrm, buf=loud)
        assert_same(alone, lights.light_filter_model(loud, pos, nrm, 4), "a NaN normal, a loud value")
        assert int((alone[..., 0] > 2).sum()) == 1 and alone[q][0] == 100.0
        hurt = np.array(buf, F, copy=True)
        hurt[q][2] = np.nan
        got = s.light_filter(4, pos=pos, nrm=ref["nrm4"], buf=hurt)
        want = lights.light_filter_model(hurt, pos, ref["nrm4"], 4)
        assert_same(got, want, "a NaN value")
        spread = np.isnan(got[..., 2])
        assert np.array_equal(spread, np.isnan(want[..., 2])) and 2 <= int(spread.sum()) <= 16 and spread[q]
        assert not (spread & ~near).any() and np.isfinite(got[..., :2]).all()


# 14 --------------------------------------------------------------------------------------------------
def test_context_form():
    """Render, a spun sum into the context's light buffer, sf_light_filter in place, light_image_buffer: the buffer and
    the image are the two models chained, and sf_light_buffer returns the same pointer before and after."""
    import torch
    Lb = sf.lib()
    with flake("t3") as s:
        s.Render()
        s.PostProcess()
        img = s.download_image()
        pos, nrm, _, _ = s.download()
        st0 = s.stats()
        alone = (st0.max_depth, np.float32(st0.closest), st0.rays, st0.overflow_tiles)
        p = s.light_filter_params(4)
        assert (p.size, p.normal_min, p.plane_max, p.width, p.height, p.stream) == (4, F(0.9), F(0.02), 0, 0, None)
        assert Lb.sf_light_filter(s.ctx, ctypes.byref(p)) == sf.SF_ESTATE        # before a buffer exists
        dev = torch.zeros((45, 80, 4), dtype=torch.float32, device="cuda")
        other = torch.full((45, 80, 4), 9.0, dtype=torch.float32, device="cuda")
        vp = lambda t: ctypes.c_void_p(t.data_ptr())
        assert Lb.sf_light_filter_to(s.ctx, ctypes.byref(p), None, None, None, vp(other)) == sf.SF_ESTATE
        assert Lb.sf_light_filter_to(s.ctx, ctypes.byref(p), None, None, vp(dev), vp(dev)) == sf.SF_EINVAL   # in == out
        assert Lb.sf_light_filter_to(s.ctx, ctypes.byref(p), None, None, vp(dev), None) == sf.SF_EINVAL
        for bad in (dict(size=0), dict(size=9), dict(normal_min=float("nan")), dict(plane_max=-0.5),
                    dict(plane_max=float("inf")), dict(plane_max=float("nan")), dict(width=80), dict(width=40, height=20)):
            b = s.light_filter_params(**{"size": 4, **bad})
            assert Lb.sf_light_filter_to(s.ctx, ctypes.byref(b), None, None, vp(dev), vp(other)) == sf.SF_EINVAL, bad
            assert Lb.sf_light_filter(s.ctx, ctypes.byref(b)) == sf.SF_EINVAL, bad
        assert s.light_buffer() == 0
        s.Synchronize()
        assert (other == 9).all()   # a refused call wrote nothing
        s.light_fill((0.0, 0.0, 0.0))
        s.trace_ao_sum(H4, None, accumulate=True, spin=S4, **KW)
        before = s.light_buffer()
        buf = s.download_light()
        assert Lb.sf_light_filter_to(s.ctx, ctypes.byref(p), None, None, None, ctypes.c_void_p(before)) == sf.SF_EINVAL
        assert s.light_filter(4) is None
        assert s.light_buffer() == before != 0
        filtered = s.download_light()
        s.light_image_buffer()
        got = s.download_image()
        again = s.light_filter(4, out=other)   # the context's images into a caller's buffer
        s.Synchronize()
        st = s.stats()
    want = lights.light_filter_model(buf, pos, nrm, 4)
    assert_same(filtered, want, "the context's light buffer, filtered in place")
    assert (filtered != buf).any()
    assert np.array_equal(got, lights.light_model_buffer(img, pos, want)) and (got != img).any()
    assert again is None
    assert_same(other.cpu().numpy(), lights.light_filter_model(want, pos, nrm, 4), "a second pass into a caller's buffer")
    # (one Render's: the filter and the traces touched no statistic)
    assert (st.max_depth, np.float32(st.closest), st.rays, st.overflow_tiles) == alone


# 15 --------------------------------------------------------------------------------------------------
def test_four_spun_filtered_rays_beat_eight_plain_ones():
    """t3, whole frame, cosine samples, colours 1 / n, tau = 4, bias 2^-10. RMS error of the open fraction against the
    unspun n = 64 sum over the 3600 surface pixels: n = 4 spun 4 x 4 then filtered is below n = 4 unspun then
    filtered, and below n = 8 unspun unfiltered. The CPU oracle gives 0.104, 0.134 and 0.113."""
    ref = frame("t3")
    pos, nrm = ref["pos4"], ref["nrm4"]
    surf = surface_of(pos)
    kw = dict(pos=pos, nrm=nrm, **KW)
    with flake("t3") as s:
        truth = s.trace_ao_sum(lights.ao_samples(64), None, **kw)
        spun = s.light_filter(4, pos=pos, nrm=nrm, buf=s.trace_ao_sum(H4, None, spin=S4, **kw))
        plain = s.light_filter(4, pos=pos, nrm=nrm, buf=s.trace_ao_sum(H4, None, **kw))
        eight = s.trace_ao_sum(sc.H8, None, **kw)
    e_spun, e_plain, e_eight = (sc.rms(a, truth, surf) for a in (spun, plain, eight))
    print("RMS error against n = 64: spun + filtered n = 4 %.4f, unspun + filtered n = 4 %.4f, unspun n = 8 %.4f"
          % (e_spun, e_plain, e_eight))
    assert int(surf.sum()) == 3600
    assert e_spun < e_plain and e_spun < e_eight
