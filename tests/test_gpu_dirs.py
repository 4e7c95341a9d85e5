"""GPU: caller-supplied directions (sf_trace_dirs_to / sf_trace_dirs / sf_probe_dirs) against the oracle. Every
comparison is of bit patterns, in all four channels (position, normal, t, heap hit index). Oracles: the oracle's
frame where the directions are a frame's own (dirs.pinhole), one-ray oracle calls (tests/dirscheck.py) elsewhere."""
import ctypes
import functools
import os

import numpy as np
import pytest

import sphereflake_amd as sf
from sphereflake_amd import dirs
from conftest import load_progressive
from dirscheck import FLT_MAX, oracle_rays, same_bits
from oracle import pyoracle
from sfcheck import bad_rows, row_digests
from test_gpu_random_views import random_view

pytestmark = pytest.mark.gpu

CHANNELS = ("pos4", "nrm4", "minT", "index")
LOD = {"avx": 70.0, "sse": 60.0}
SENTINEL = np.float32(-12345.5)
FIXUP_LOOP_COPIES = 38   # (t3 at 4 levels flags every group of the list, 56.25 a copy: about 2140)


@pytest.fixture(scope="module", autouse=True)
def device():
    sf.build()
    assert sf.device_count() >= 1, "no HIP device visible: GPU tests must run on an MI355X"


@functools.lru_cache(maxsize=None)
def view(name):
    """Setup of a named view: t1..t4 (reference dumps) or rv<seed> (test_gpu_random_views.random_view)."""
    if name.startswith("rv"):
        seed = int(name[2:])
        W, H, _, cam = random_view(np.random.default_rng(1000 + seed), seed)
        o, tl, tr, bl = cam.corners()
        return {"W": W, "H": H, "origin": o, "tl": tl, "tr": tr, "bl": bl, "root": sf.root_transform(o),
                "children": sf.child_transforms()}
    return pyoracle.load_setup(name)


@functools.lru_cache(maxsize=None)
def frame(name, variant="avx"):
    return pyoracle.render(view(name), lod=LOD[variant])


@functools.lru_cache(maxsize=None)
def pinhole(name):
    S = view(name)
    return dirs.pinhole(S["origin"], S["tl"], S["tr"], S["bl"], S["W"], S["H"])


def scattered():
    d = np.random.default_rng(7).normal(size=(512, 3)).astype(np.float32)
    assert not (d == 0.0).any()
    return d


@functools.lru_cache(maxsize=None)
def scattered_oracle(name):
    S = view(name)
    ref = oracle_rays(S["root"], S["children"], scattered())
    # the comparison below cannot pass on misses alone
    assert ref["stats"]["hits"] >= 50, ref["stats"]
    return ref


def flake(name, variant="avx", size=None):
    S = view(name)
    s = sf.Sphereflake(*(size or (S["W"], S["H"])))
    s.SetVariant(variant)
    s.SetView(S["origin"], S["tl"], S["tr"], S["bl"])
    return s


def trace(s, d, stride=3, pad=0, **kw):
    """d [H, W, 3] or [N, 3] through torch tensors (zero copy), outputs padded by `pad` sentinel elements behind
    the last ray. Returns the four channels as numpy arrays shaped like d's leading dimensions."""
    import torch
    lead = d.shape[:-1]
    n = int(np.prod(lead))
    if stride == 4:   # (the 4th float is ignored, whatever it holds)
        d = np.concatenate([d, np.full(lead + (1,), np.nan, np.float32)], axis=-1)
    dt = torch.from_numpy(np.ascontiguousarray(d)).cuda()
    pos = torch.full((n + pad, 4), float(SENTINEL), dtype=torch.float32, device="cuda")
    nrm = torch.full((n + pad, 4), float(SENTINEL), dtype=torch.float32, device="cuda")
    mint = torch.full((n + pad,), float(SENTINEL), dtype=torch.float32, device="cuda")
    idx = torch.full((n + pad,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s.trace_dirs(dt, out=(pos, nrm, mint, idx), **kw)
    s.Synchronize()
    got = {"pos4": pos.cpu().numpy(), "nrm4": nrm.cpu().numpy(), "minT": mint.cpu().numpy(),
           "index": idx.cpu().numpy().view(np.uint32)}
    for k, a in got.items():
        tail = a[n:]
        assert (tail == (np.uint32(0x5a5a5a5a) if k == "index" else SENTINEL)).all(), f"{k}: wrote past the last ray"
        got[k] = a[:n].reshape(lead + a.shape[1:])
    return got


def assert_same(got, ref, what, sel=None):
    for k in CHANNELS:
        a, b = got[k], ref[k]
        if sel is not None:
            a, b = a[sel], b[sel]
        assert same_bits(a, b), f"{what}: {k} differs"


# 1 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [3, 4])
@pytest.mark.parametrize("variant", ["avx", "sse"])
@pytest.mark.parametrize("name", ["t1", "t2", "t3", "t4", "rv1", "rv3", "rv6", "rv8"])
def test_pinhole_image_equals_the_frame(name, variant, stride):
    ref = frame(name, variant)
    S = view(name)
    with flake(name, variant) as s:
        got = trace(s, pinhole(name), stride=stride)
        st = s.stats()
    assert_same(got, ref, f"{name} {variant} stride {stride}")
    assert st.max_depth == ref["stats"]["max_depth"]
    assert np.float32(st.closest) == np.float32(ref["stats"]["closest"])
    assert st.rays == S["W"] * S["H"]


# 2 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t4", "t2"])
def test_list_mode_permuted_and_prefixes(name):
    """t4: 91 rays, one full and one partial wave; t2: 2304 rays. Any order, any prefix: the same per-ray bits, and
    nothing written behind the last ray."""
    ref = frame(name)
    flat = pinhole(name).reshape(-1, 3)
    n = flat.shape[0]
    perm = np.random.default_rng(11).permutation(n)
    want = {k: ref[k].reshape((n,) + ref[k].shape[2:])[perm] for k in CHANNELS}
    with flake(name) as s:
        got = trace(s, flat[perm], pad=70)
        assert_same(got, want, f"{name} list")
        for m in (1, 63, 64, 65):
            got = trace(s, flat[perm][:m], pad=70)
            assert_same(got, {k: want[k][:m] for k in CHANNELS}, f"{name} prefix {m}")
        assert s.stats().rays == n + 1 + 63 + 64 + 65


# 3 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(512,), (16, 32)])
@pytest.mark.parametrize("name", ["t2", "t3", "t4"])
def test_off_frustum_directions(name, shape):
    """Normally distributed directions -- all around the origin, nothing like a frame -- as a list and as a 32 x 16
    image (8 x 8 tiles of unrelated rays: the wave's cone switches itself off)."""
    ref = scattered_oracle(name)
    with flake(name) as s:
        got = trace(s, scattered().reshape(shape + (3,)))
        st = s.stats()
    assert_same({k: got[k].reshape((512,) + got[k].shape[len(shape):]) for k in CHANNELS}, ref, f"{name} {shape}")
    assert st.max_depth == ref["stats"]["max_depth"]
    assert np.float32(st.closest) == np.float32(ref["stats"]["closest"])


# 4 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [(5, 36, 63), (5, 32, 63), tuple(range(64))])
@pytest.mark.parametrize("shape", [(512,), (16, 32)])
def test_degenerate_directions_are_misses_and_harmless(shape, lanes):
    """Zero, NaN and infinite directions in lanes of the first wave -- the cone's axis lane among them (36 of a
    tile, 32 of a list), and a whole wave of them -- are misses and change no other ray."""
    ref = scattered_oracle("t3")
    d = scattered().reshape(shape + (3,)).copy()
    bad = [(0.0, 0.0, 0.0), (np.nan, 1.0, 1.0), (np.inf, 1.0, 1.0), (1e-30, 1e-30, 1e-30), (1.0, -np.inf, 1.0)]
    S = view("t3")
    assert oracle_rays(S["root"], S["children"], np.array(bad, np.float32))["stats"]["hits"] == 0
    # ray of lane l of the first wave: the l-th of a list, pixel (l % 8, l // 8) of an image's first tile
    rays = [l if len(shape) == 1 else (l // 8) * shape[1] + (l % 8) for l in lanes]
    for j, r in enumerate(rays):
        d.reshape(-1, 3)[r] = bad[j % len(bad)]
    with flake("t3") as s:
        got = trace(s, d)
    got = {k: got[k].reshape((512,) + got[k].shape[len(shape):]) for k in CHANNELS}
    keep = np.ones(512, bool)
    keep[rays] = False
    assert_same(got, ref, f"{shape} {lanes[:3]}", sel=keep)
    miss4 = np.array([0.0, 0.0, 0.0, 1.0], np.float32)
    for r in rays:
        assert same_bits(got["pos4"][r], miss4) and same_bits(got["nrm4"][r], miss4)
        assert got["minT"][r] == FLT_MAX and got["index"][r] == 0xffffffff


# 5 ---------------------------------------------------------------------------------------------------
def test_overflow_groups_are_retraced():
    """max_depth = 4 provisions too few levels for t3 (depth 9): the flagged groups are re-traced, results exact."""
    with flake("t3") as s:
        got = trace(s, pinhole("t3"), max_depth=4)
        assert_same(got, frame("t3"), "t3 pinhole, 4 levels")
        o1 = s.stats().overflow_tiles
        assert o1 > 0
        got = trace(s, scattered(), max_depth=4)
        assert_same(got, scattered_oracle("t3"), "t3 scattered, 4 levels")
        assert s.stats().overflow_tiles > o1
        s.Synchronize()   # clean: nothing left unresolved
        assert s.stats().max_depth == max(frame("t3")["stats"]["max_depth"], scattered_oracle("t3")["stats"]["max_depth"])
    with flake("t4") as s:   # depth 12 at the default provisioning
        got = trace(s, scattered())
        assert_same(got, scattered_oracle("t4"), "t4 scattered")
        s.Synchronize()
        assert s.stats().max_depth == scattered_oracle("t4")["stats"]["max_depth"]


def test_more_flagged_groups_than_fixup_blocks():
    """t3's pinhole directions R times over as one list at max_depth = 4: more flagged groups than the re-trace launch
    has blocks (1024 is the larger of the two fixup grids), so its blocks walk the list more than once. 3600 rays are
    56.25 groups: the copies are grouped differently, the per-ray results are the frame's all the same."""
    R = FIXUP_LOOP_COPIES
    ref = frame("t3")
    flat = pinhole("t3").reshape(-1, 3)
    n = flat.shape[0]
    want = {k: np.concatenate([ref[k].reshape((n,) + ref[k].shape[2:])] * R) for k in CHANNELS}
    with flake("t3") as s:
        o0 = s.stats().overflow_tiles
        got = trace(s, np.concatenate([flat] * R), max_depth=4)
        moved = s.stats().overflow_tiles - o0
    print("flagged groups", moved, "per copy", moved / R)
    assert moved > 1024
    assert_same(got, want, f"t3 pinhole x {R}, 4 levels")


# 6 ---------------------------------------------------------------------------------------------------
def test_context_buffers_and_bystanders(tmp_path):
    """A panorama traced into the context's own frame between renders: it is the one-ray oracle's, the
    post-process and the image dump take it, and the renders after it are what they were (heavy-first rebuilds
    included)."""
    S = view("t2")
    W, H = S["W"], S["H"]
    fwd = (S["tl"] + (S["tr"] - S["tl"]) * 0.5 + (S["bl"] - S["tl"]) * 0.5) - S["origin"]
    pano = dirs.equirect(W, H, fwd, (0.13, 0.21, 0.97))
    assert not (pano == 0.0).any()
    ref = oracle_rays(S["root"], S["children"], pano)
    assert ref["stats"]["hits"] >= 50
    with flake("t2") as s:
        s.Render(emit_aux=True)
        assert s.trace_dirs(pano) is None
        pos, nrm, mint, idx = s.download(aux=True)
        assert_same({"pos4": pos, "nrm4": nrm, "minT": mint, "index": idx}, ref, "t2 panorama")
        s.PostProcess()
        path = tmp_path / "pano.ppm"
        s.save_image(str(path), sf.SF_DUMP_IMAGE)
        assert os.path.getsize(path) == len(f"P6\n{W} {H}\n255\n") + W * H * 3
        for k in range(4):
            s.Render(emit_aux=True)
            pos, nrm, mint, idx = s.download(aux=True)
            assert_same({"pos4": pos, "nrm4": nrm, "minT": mint, "index": idx}, frame("t2"), f"render {k} after")
        # the numpy path returns the same panorama without touching the frame
        got = dict(zip(CHANNELS, s.trace_dirs(pano, out="host")))
        assert_same(got, ref, "t2 panorama (host arrays)")
        pos2, nrm2, _, _ = s.download()
        assert same_bits(pos2, pos) and same_bits(nrm2, nrm)


def test_progressive_after_directions():
    """The frame-less mode's p1 fixture on a context that traced directions first."""
    fx = load_progressive("p1")
    W, H, K = fx["W"], fx["H"], float.fromhex(fx["K"])
    with sf.Sphereflake(W, H) as s:
        s.SetCamera(sf.config_camera(W, H, K))
        s.trace_dirs(scattered())
        s.trace_dirs(scattered()[:100], max_depth=4)
        s.reset_stats()
        half = fx["packets"] // 3
        s.Progressive(fx["seed"], half, counter0=0)
        s.Progressive(fx["seed"], fx["packets"] - half)
        pos, nrm, _, _ = s.download()
        st = s.stats()
    assert bad_rows(fx["row_digest_gbuf"], row_digests(pos, nrm)) == []
    assert st.max_depth == fx["stats"]["max_depth"]
    assert np.float32(st.closest) == np.float32(float.fromhex(fx["stats"]["closest"]))
    assert st.rays == fx["stats"]["rays"]


# 7 ---------------------------------------------------------------------------------------------------
def test_callers_stream_between_renders():
    """Render, directions on a caller's torch stream, Render -- no host synchronisation in between."""
    import torch
    S = view("t3")
    W, H = S["W"], S["H"]
    ref = frame("t3")
    mk = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device="cuda")
    a = (mk(H, W, 4), mk(H, W, 4), mk(H, W), mk(H, W, dt=torch.int32))
    b = (mk(H, W, 4), mk(H, W, 4), mk(H, W), mk(H, W, dt=torch.int32))
    dt = torch.from_numpy(pinhole("t3")).cuda()
    ts = torch.cuda.Stream()
    torch.cuda.synchronize()
    with flake("t3") as s:
        s.render_to(a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), emit_aux=True)
        s.trace_dirs(dt, out=b, stream=ts.cuda_stream)
        s.Render(emit_aux=True)
        pos, nrm, mint, idx = s.download(aux=True)   # (synchronises the context, whatever stream its work ran on)
        assert s.stats().rays == 3 * W * H
        for what, t in (("render_to", a), ("trace_dirs", b)):
            got = {"pos4": t[0].cpu().numpy(), "nrm4": t[1].cpu().numpy(), "minT": t[2].cpu().numpy(),
                   "index": t[3].cpu().numpy().view(np.uint32)}
            assert_same(got, ref, what)
        assert_same({"pos4": pos, "nrm4": nrm, "minT": mint, "index": idx}, ref, "Render")


# 8 ---------------------------------------------------------------------------------------------------
def test_probe_move_axes_and_centre():
    S = view("t2")
    W, H = S["W"], S["H"]
    cam = sf.config_camera(W, H, S["K"])
    d = np.concatenate([dirs.move_axes(cam), pinhole("t2")[H // 2, W // 2].reshape(1, 3)])
    assert not np.signbit(d[d == 0.0]).any()   # (a +0 component is what the oracle's ray generation keeps)
    ref = oracle_rays(S["root"], S["children"], d)
    assert ref["minT"][6] < FLT_MAX   # the centre pixel sees the flake
    with flake("t2") as s:
        mint, idx, pos, nrm = s.probe(d)
        assert s.stats().rays == 7
    assert_same({"pos4": pos, "nrm4": nrm, "minT": mint, "index": idx}, ref, "probe")


# 9 ---------------------------------------------------------------------------------------------------
def test_error_codes():
    import torch
    L = sf.lib()
    d = torch.from_numpy(scattered()).cuda()
    o = torch.zeros(512 * 4, dtype=torch.float32, device="cuda")
    dp, op = ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(o.data_ptr())
    P = lambda w, h, stride=3: ctypes.byref(sf.sf_dirs_params(w, h, stride, 0, None))
    host = scattered()
    hp = host.ctypes.data_as(ctypes.c_void_p)
    hout = np.empty(512, np.float32)
    with sf.Sphereflake(64, 36) as s:
        assert L.sf_trace_dirs_to(s.ctx, P(512, 1), dp, op, None, None, None) == sf.SF_ENOVIEW
        assert L.sf_trace_dirs(s.ctx, P(64, 36), dp) == sf.SF_ENOVIEW
        assert L.sf_probe_dirs(s.ctx, hp, 7, hout.ctypes.data_as(ctypes.c_void_p), None, None, None) == sf.SF_ENOVIEW
        S = view("t2")
        s.SetView(S["origin"], S["tl"], S["tr"], S["bl"])
        assert L.sf_trace_dirs_to(s.ctx, P(512, 1, 2), dp, op, None, None, None) == sf.SF_EINVAL
        assert L.sf_trace_dirs_to(s.ctx, P(512, 1, 5), dp, op, None, None, None) == sf.SF_EINVAL
        assert L.sf_trace_dirs_to(s.ctx, P(512, 1), None, op, None, None, None) == sf.SF_EINVAL
        assert L.sf_trace_dirs_to(s.ctx, P(512, 1), dp, None, None, None, None) == sf.SF_EINVAL
        assert L.sf_trace_dirs(s.ctx, P(32, 16), dp) == sf.SF_EINVAL
        assert L.sf_probe_dirs(s.ctx, hp, 7, None, None, None, None) == sf.SF_EINVAL
        assert L.sf_trace_dirs_to(s.ctx, P(0, 1), dp, op, None, None, None) == sf.SF_OK
        assert L.sf_trace_dirs_to(s.ctx, P(64, 0), dp, op, None, None, None) == sf.SF_OK
        assert L.sf_probe_dirs(s.ctx, hp, 0, hout.ctypes.data_as(ctypes.c_void_p), None, None, None) == sf.SF_OK
        s.Synchronize()
        assert s.stats().rays == 0
        assert (o == 0).all()
        # one output alone is enough
        assert L.sf_trace_dirs_to(s.ctx, P(512, 1), dp, None, None, op, None) == sf.SF_OK
        s.Synchronize()
        assert same_bits(o[:512].cpu().numpy(), scattered_oracle("t2")["minT"])
