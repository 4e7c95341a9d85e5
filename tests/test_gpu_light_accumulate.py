"""Temporal accumulation of the light buffer on the GPU (sf_light_accumulate_to / sf_light_accumulate /
sf_light_history_reset): the `_to` form equals sphereflake_amd.lights.light_accumulate_model bit for bit on frames the
library rendered from moved views, with a seeded history whose counts cover every case of the definition; the numpy,
torch and device-address forms agree; the context form is the chain of model calls, keeps the light buffer's address
and keeps its history apart from what is done to the light buffer afterwards; a still view leaves the running mean;
every error code, and a failing call writes nothing."""
import ctypes

import numpy as np
import pytest

import sphereflake_amd as sf
from sphereflake_amd import lights
from oracle import pyoracle
from lightsumcheck import assert_same, surface_of
import aocheck as ac
import aospincheck as sc
import accumcheck as ak
from aospincheck import flake

pytestmark = pytest.mark.gpu

F = np.float32
H4 = sc.H4
KW = dict(distance=ac.TAU, bias=ac.B10)
HISTORIES = (1, 4, 65535)


@pytest.fixture(scope="module", autouse=True)
def device():
    sf.build()
    assert sf.device_count() >= 1, "no HIP device visible: GPU tests must run on an MI355X"


def rendered(s, view):
    """The library's frame of `view` (origin, tl, tr, bl): (pos4, nrm4)."""
    s.SetView(*view)
    s.Render()
    pos, nrm, _, _ = s.download()
    return pos, nrm


def spun(s, k):
    """Frame k's input: the spun n = 4 sum of the context's own frame into the context's light buffer."""
    s.trace_ao_sum(H4, None, spin=lights.ao_spins(4, lights.ao_phase(k)), **KW)


# 1 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["avx", "sse"])
@pytest.mark.parametrize("pair", ak.PAIRS, ids=lambda p: "%s-%s-%g" % p)
def test_the_to_form_equals_the_model(pair, variant):
    """The five moved pairs, both frames rendered by the library; a seeded history light with .w drawn from
    {0, 1, 3, 16, 70000, NaN}; the three threshold pairs; max_history 1, 4 and 65535."""
    name = pair[0]
    S, hS = ak.moved_setup(name, ak.delta_of(*pair)), pyoracle.load_setup(name)
    with flake(name, variant) as s:
        hpos, hnrm = rendered(s, ak.view_of(hS))
        pos, nrm = rendered(s, ak.view_of(S))
        new = s.trace_ao_sum(H4, None, pos=pos, nrm=nrm, spin=lights.ao_spins(4), origin=S["origin"], **KW)
        hist = ak.seeded_history(pos.shape[:2], 7)
        surf = surface_of(pos)
        kw = dict(pos=pos, nrm=nrm, buf=new, hist_pos=hpos, hist_nrm=hnrm, hist=hist, hist_view=ak.view_of(hS))
        for nmin, pmax in sc.THRESHOLDS:
            for mh in HISTORIES:
                got = s.light_accumulate(mh, nmin, pmax, **kw)
                want, acc, taps = lights.light_accumulate_model(new, pos, nrm, S["origin"], hist, hpos, hnrm,
                                                                ak.view_of(hS), mh, nmin, pmax)
                assert_same(got, want, f"{pair} {variant} {nmin} {pmax} {mh}")
                assert (got[acc][:, 3] <= mh).all() and (got[surf & ~acc][:, 3] == 1).all()
                assert (got[~surf][:, 3] == 0).all()
        got = s.light_accumulate(**kw)   # the defaults: 16, 0.9, 0.02
        want, acc, taps = lights.light_accumulate_model(new, pos, nrm, S["origin"], hist, hpos, hnrm, ak.view_of(hS))
        assert_same(got, want, f"{pair} {variant} defaults")
        kept, n = int(acc.sum()), int(surf.sum())
        print(pair, variant, "accepted", kept, "/", n, "of them clamped at 16:", int((got[acc][:, 3] == 16).sum()))
        # (the seeded counts reject the third of the taps whose .w is 0 or NaN; the rest are as on the oracle's frames)
        assert 0.1 * n <= kept <= 0.85 * n and set(np.unique(got[acc][:, 3])) == {2.0, 4.0, 16.0}


# 2 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t4", "t5"])
def test_numpy_torch_and_address_forms_agree(name):
    """13 x 7 and 1 x 1, the history seen from the fixture's own view and, on t4, from a moved one: numpy images, torch
    tensors and device addresses give the same bits, and guard words around the output are intact."""
    import torch
    hS = pyoracle.load_setup(name)
    views = [ak.view_of(hS)] + ([ak.view_of(ak.moved_setup(name, ak.delta_of(name, "right", 0.01)))] if name == "t4"
                                else [])
    guard, sentinel = 8, -123.25
    with flake(name) as s:
        hpos, hnrm = rendered(s, ak.view_of(hS))
        h, w = hpos.shape[:2]
        rng = np.random.default_rng(4)
        new = rng.random((h, w, 4)).astype(F)
        hist = ak.seeded_history((h, w), 9)
        hist[0, 0, 3] = 3.0
        for view in views:
            pos, nrm = rendered(s, view)
            want, acc, _ = lights.light_accumulate_model(new, pos, nrm, view[0], hist, hpos, hnrm, ak.view_of(hS), 4)
            assert acc.any()
            host = s.light_accumulate(4, pos=pos, nrm=nrm, buf=new, hist_pos=hpos, hist_nrm=hnrm, hist=hist,
                                      hist_view=ak.view_of(hS), origin=view[0])
            assert_same(host, want, f"{name} numpy")
            ts = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (pos, nrm, new, hpos, hnrm, hist)]
            out = torch.full((h, w, 4), sentinel, dtype=torch.float32, device="cuda")
            s.light_accumulate(4, pos=ts[0], nrm=ts[1], buf=ts[2], hist_pos=ts[3], hist_nrm=ts[4], hist=ts[5],
                               hist_view=ak.view_of(hS), out=out, origin=view[0])
            s.Synchronize()
            assert_same(out.cpu().numpy(), want, f"{name} torch")
            flat = torch.full((2 * guard + h * w * 4 + 2 * guard,), sentinel, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            s.light_accumulate(4, pos=(ts[0].data_ptr(), w, h), nrm=ts[1].data_ptr(), buf=(ts[2].data_ptr(), w, h),
                               hist_pos=ts[3].data_ptr(), hist_nrm=ts[4], hist=ts[5].data_ptr(),
                               hist_view=np.concatenate(ak.view_of(hS)), out=flat.data_ptr() + 8 * guard,
                               origin=view[0])
            s.Synchronize()
            fo = flat.cpu().numpy()
            assert (fo[:2 * guard] == F(sentinel)).all() and (fo[2 * guard + h * w * 4:] == F(sentinel)).all(), "guards"
            assert_same(fo[2 * guard:2 * guard + h * w * 4].reshape(h, w, 4), want, f"{name} addresses")
            for t, a in zip(ts, (pos, nrm, new, hpos, hnrm, hist)):   # no input is written
                assert np.array_equal(t.cpu().numpy().view(np.uint32), np.ascontiguousarray(a).view(np.uint32))


# 3 ---------------------------------------------------------------------------------------------------
def test_context_form_is_the_chain_of_model_calls():
    """Three views of t3's path through the context form: each frame's light buffer equals the model applied to the
    frame before's result; the light buffer's address never changes; an in-place light_filter and an accumulating
    trace_suns_sum after light_accumulate do not reach the history; light_history_reset makes the next call a first
    call."""
    views = [ak.view_of(ak.moved_setup("t3", ak.delta_of("t3", *ak.path_view(k)))) for k in (13, 14, 15)]
    sun = lights.sun_direction((0.7, 0.7, 0.2)).reshape(1, 3)
    frames = []
    with flake("t3") as s:
        s.light_fill((0.0, 0.0, 0.0))
        address = s.light_buffer()
        assert address != 0
        for k, view in enumerate(views + views[-1:]):
            pos, nrm = rendered(s, view)
            spun(s, k)
            new = s.download_light()
            if k == 3:
                s.light_history_reset()
            assert s.light_accumulate() is None
            assert s.light_buffer() == address
            frames.append((view, pos, nrm, new, s.download_light()))
            # what the frame goes on to do with its light buffer: none of it may reach the next frame's history
            s.light_filter(4)
            s.trace_suns_sum(sun, np.array([[0.5, 0.4, 0.3]], F), accumulate=True, distance=4.0)
            assert s.light_buffer() == address
            assert (s.download_light() != frames[-1][4]).any()
    zero = np.zeros_like(frames[0][3])
    kept = []
    for k, (view, pos, nrm, new, got) in enumerate(frames):
        if k in (0, 3):   # the first call, and the first after a reset
            want, acc, _ = lights.light_accumulate_model(new, pos, nrm, view[0], zero, zero, zero, view)
            assert not acc.any()
        else:
            hview, hpos, hnrm, _, hbuf = frames[k - 1]
            want, acc, _ = lights.light_accumulate_model(new, pos, nrm, view[0], hbuf, hpos, hnrm, hview)
        assert_same(got, want, f"frame {k}")
        kept.append(int(acc.sum()))
    print("pixels that keep their history, frames 0..3:", kept, "of", int(surface_of(frames[0][1]).sum()))
    assert kept[1] >= 1800 and kept[2] >= 1800 and frames[2][4][..., 3].max() == 3.0


# 4 ---------------------------------------------------------------------------------------------------
def test_a_still_view_leaves_the_running_mean():
    """16 calls of the context form from t3's view with 16 differently spun inputs: the model's chain bit for bit, which
    is the running mean h + (in - h) / k, and .w = 16 on every surface pixel; a 17th call stays at 16."""
    S = pyoracle.load_setup("t3")
    view = ak.view_of(S)
    with flake("t3") as s:
        pos, nrm = rendered(s, view)
        surf = surface_of(pos)
        mean = None
        for k in range(17):
            spun(s, k)
            new = s.download_light()
            s.light_accumulate(16)
            got = s.download_light()
            if k == 0:
                mean = new[..., :3].copy()
            else:
                mean = mean + (new[..., :3] - mean) / F(min(k + 1, 16))
            assert_same(np.ascontiguousarray(got[..., :3]), mean, f"call {k}", surf)
            assert (got[surf][:, 3] == min(k + 1, 16)).all() and (got[~surf][:, 3] == 0).all()
        assert int(surf.sum()) == 3600


# 5 ---------------------------------------------------------------------------------------------------
def test_errors_and_a_failing_call_writes_nothing():
    import torch
    L = sf.lib()
    S = pyoracle.load_setup("t3")
    view = ak.view_of(S)
    with sf.Sphereflake(S["W"], S["H"]) as s:
        t = [torch.full((45, 80, 4), float(i + 1), dtype=torch.float32, device="cuda") for i in range(7)]
        vp = [ctypes.c_void_p(x.data_ptr()) for x in t]
        p = s.light_accumulate_params(hist_view=view)
        assert (p.max_history, p.normal_min, p.plane_max, p.use_origin, p.width, p.height, p.stream) \
            == (16, F(0.9), F(0.02), 0, 0, 0, None)
        call = lambda q, *a: L.sf_light_accumulate_to(s.ctx, ctypes.byref(q), *a)
        assert call(p, *vp) == sf.SF_ENOVIEW                      # use_origin == 0 before SetView
        assert L.sf_light_accumulate(s.ctx, ctypes.byref(p)) == sf.SF_ENOVIEW
        s.SetView(*view)
        assert L.sf_light_accumulate(s.ctx, ctypes.byref(p)) == sf.SF_ESTATE   # nothing has written the light buffer
        assert L.sf_light_accumulate_to(s.ctx, None, *vp) == sf.SF_EINVAL
        for k in range(7):                                         # a null image
            a = list(vp)
            a[k] = None
            assert call(p, *a) == sf.SF_EINVAL, k
        for k in range(6):                                         # out is one of the inputs
            a = list(vp)
            a[6] = vp[k]
            assert call(p, *a) == sf.SF_EINVAL, k
        bads = [dict(max_history=0), dict(max_history=65536), dict(normal_min=float("nan")), dict(plane_max=-0.5),
                dict(plane_max=float("inf")), dict(plane_max=float("nan")), dict(width=80), dict(height=45),
                dict(width=65536, height=65536)]
        for bad in bads:
            b = s.light_accumulate_params(**{"hist_view": view, **bad})
            assert call(b, *vp) == sf.SF_EINVAL, bad
        for field, n in (("hist_m", 9), ("hist_origin", 3)):
            for k in range(n):
                for v in (float("nan"), float("inf")):
                    b = s.light_accumulate_params(hist_view=view)
                    getattr(b, field)[k] = v
                    assert call(b, *vp) == sf.SF_EINVAL, (field, k)
        s.Synchronize()
        for i, x in enumerate(t):
            assert (x == float(i + 1)).all()                       # the refused calls wrote nothing
        # the context form: refused calls leave the light buffer and the history as they were
        s.Render()
        spun(s, 0)
        s.light_accumulate()
        first = s.download_light()
        for bad in bads[:7] + [dict(width=40, height=20)]:
            b = s.light_accumulate_params(**bad)
            assert L.sf_light_accumulate(s.ctx, ctypes.byref(b)) == sf.SF_EINVAL, bad
        assert_same(s.download_light(), first, "the light buffer after refused calls")
        pos, nrm, _, _ = s.download()
        spun(s, 1)
        new = s.download_light()
        s.light_accumulate()
        want, acc, _ = lights.light_accumulate_model(new, pos, nrm, view[0], first, pos, nrm, view)
        assert_same(s.download_light(), want, "the history after refused calls")
        assert np.array_equal(acc, surface_of(pos))
        flat = (view[0], view[1], view[2], view[2])               # a view that spans no volume
        s.SetView(*flat)
        assert L.sf_light_accumulate(s.ctx, ctypes.byref(p)) == sf.SF_EINVAL
        assert_same(s.download_light(), want, "the light buffer after a refused view")
        with pytest.raises(ValueError):
            s.light_accumulate(pos=pos)
        with pytest.raises(ValueError):
            s.light_accumulate(out=t[6])
        assert L.sf_light_history_reset(s.ctx) == sf.SF_OK
