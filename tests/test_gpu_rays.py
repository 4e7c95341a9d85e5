"""GPU: rays from caller-supplied origins (sf_trace_rays_to / sf_probe_rays) against the oracle. Every comparison is
of bit patterns, in all four channels (position, normal, t, heap hit index). Oracles: the oracle's frame where the
rays are a frame's own, one-ray oracle calls under sf.root_transform(origin) (tests/rayscheck.py) elsewhere."""
import ctypes

import numpy as np
import pytest

import sphereflake_amd as sf
from sphereflake_amd import rays
from conftest import load_progressive
from dirscheck import FLT_MAX, same_bits
from oracle import pyoracle
from rayscheck import CHANNELS, frame, oracle_multi, pinhole, set_oracle
import rayscheck
from sfcheck import bad_rows, row_digests

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-12345.5)
FORCE_MIXED = "0x8000"   # SF_FLAG_FORCE_MIXED
MISS4 = np.array([0.0, 0.0, 0.0, 1.0], np.float32)
FIXUP_LOOP_COPIES = 132   # (the reflect set at 4 levels flags all 16 groups of a copy: 2112)


@pytest.fixture(scope="module", autouse=True)
def device():
    sf.build()
    assert sf.device_count() >= 1, "no HIP device visible: GPU tests must run on an MI355X"


def view(name):
    return pyoracle.load_setup(name)


def origin_of(name):
    return np.asarray(view(name)["origin"], np.float32)


def flake(name, variant="avx"):
    S = view(name)
    s = sf.Sphereflake(S["W"], S["H"])
    s.SetVariant(variant)
    s.SetView(S["origin"], S["tl"], S["tr"], S["bl"])
    return s


def trace(s, o, d, rpo=1, ostride=3, dstride=3, pad=70, **kw):
    """o [M, 3], d [H, W, 3] or [N, 3] through torch tensors (zero copy), outputs padded by `pad` sentinel elements
    behind the last ray. Returns the four channels as numpy arrays shaped like d's leading dimensions."""
    import torch
    lead = d.shape[:-1]
    n = int(np.prod(lead))
    if dstride == 4:   # (the 4th float is ignored, whatever it holds)
        d = np.concatenate([d, np.full(lead + (1,), np.nan, np.float32)], axis=-1)
    if ostride == 4:
        o = np.concatenate([o, np.full((o.shape[0], 1), np.nan, np.float32)], axis=-1)
    dt = torch.from_numpy(np.ascontiguousarray(d)).cuda()
    ot = torch.from_numpy(np.ascontiguousarray(o)).cuda()
    pos = torch.full((n + pad, 4), float(SENTINEL), dtype=torch.float32, device="cuda")
    nrm = torch.full((n + pad, 4), float(SENTINEL), dtype=torch.float32, device="cuda")
    mint = torch.full((n + pad,), float(SENTINEL), dtype=torch.float32, device="cuda")
    idx = torch.full((n + pad,), 0x5a5a5a5a, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s.trace_rays(ot, dt, rays_per_origin=rpo, out=(pos, nrm, mint, idx), **kw)
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
        if a.shape != b.shape:   # (an image against a list of the same rays)
            a = a.reshape(b.shape)
        if sel is not None:
            a, b = a[sel], b[sel]
        assert same_bits(a, b), f"{what}: {k} differs"


def flat(ref):
    return {k: ref[k].reshape((-1,) + ref[k].shape[2:]) for k in CHANNELS}


# 1, and 4 for it -------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("strides", [(3, 4), (4, 3)])
@pytest.mark.parametrize("variant", ["avx", "sse"])
@pytest.mark.parametrize("name", ["t1", "t2", "t3", "t4"])
def test_one_origin_equals_the_frame(name, variant, strides, forced, monkeypatch):
    """The frame's own rays from the frame's own origin: once as one origin for all rays, once with the origin
    repeated per ray -- the oracle's frame and its statistics, also with every group on the mixed path."""
    if forced:
        monkeypatch.setenv("SF_FLAGS", FORCE_MIXED)
    ref = frame(name, variant)
    S = view(name)
    n = S["W"] * S["H"]
    o = origin_of(name).reshape(1, 3)
    ostride, dstride = strides
    for k, (oo, rpo) in enumerate(((o, n), (np.repeat(o, n, axis=0), 1))):
        with flake(name, variant) as s:
            got = trace(s, oo, pinhole(name), rpo=rpo, ostride=ostride, dstride=dstride)
            st = s.stats()
        assert_same(got, ref, f"{name} {variant} strides {strides} run {k}")
        assert st.max_depth == ref["stats"]["max_depth"]
        assert np.float32(st.closest) == np.float32(ref["stats"]["closest"])
        assert st.rays == n


# 2, and 4 for it -------------------------------------------------------------------------------------
def camera_batch():
    o = np.stack([origin_of("t1"), origin_of("t2"), origin_of("t3"), origin_of("t4"),
                  (origin_of("t1") + origin_of("t2")) * np.float32(0.5)])
    d = np.tile(pinhole("t4").reshape(-1, 3), (5, 1))
    return o, d


@pytest.fixture(scope="module")
def camera_batch_oracle():
    o, d = camera_batch()
    ref = oracle_multi(view("t4")["children"], o, d, rays_per_origin=91)
    assert (ref["minT"][:91] < FLT_MAX).any()   # the t1-origin block sees the flake
    return ref


@pytest.mark.parametrize("forced", [False, True])
def test_camera_batch(camera_batch_oracle, forced, monkeypatch):
    """Five origins with t4's 13 x 7 image under each, a 455-ray list: groups 1, 2, 4 and 5 straddle two origins
    (mixed path), the others have one (the frame's traversal)."""
    if forced:
        monkeypatch.setenv("SF_FLAGS", FORCE_MIXED)
    o, d = camera_batch()
    assert d.shape == (455, 3)
    with flake("t4") as s:
        got = trace(s, o, d, rpo=91)
        assert s.stats().rays == 455
    assert_same(got, camera_batch_oracle, "camera batch")


# 3 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2304,), (36, 64)])
def test_jitter(shape):
    o, d = rayscheck.jitter()
    ref = set_oracle("jitter")
    with flake("t1") as s:
        got = trace(s, o, d.reshape(shape + (3,)))
        st = s.stats()
    assert_same(got, ref, f"jitter {shape}")
    assert st.max_depth == ref["stats"]["max_depth"]
    assert np.float32(st.closest) == np.float32(ref["stats"]["closest"])


@pytest.mark.parametrize("max_depth", [0, 4])
@pytest.mark.parametrize("name", ["reflect", "towards_in"])
def test_secondary_rays_overflow_and_are_retraced(name, max_depth):
    """Depth 16 against the default 12 levels (and against 4): groups overflow and are re-traced, results exact."""
    o, d = rayscheck.SETS[name][0]()
    ref = set_oracle(name)
    with flake("t3") as s:
        got = trace(s, o, d, max_depth=max_depth)
        st = s.stats()
    assert_same(got, ref, f"{name} max_depth {max_depth}")
    assert st.overflow_tiles > 0
    assert st.max_depth == ref["stats"]["max_depth"]
    assert np.float32(st.closest) == np.float32(ref["stats"]["closest"])


def test_more_flagged_groups_than_fixup_blocks():
    """The reflect set R times over as one list (an origin per ray: the mixed path) at max_depth = 4: more flagged
    groups than the re-trace launch has blocks (1024), so its blocks walk the list more than once, restaging the root
    image between groups."""
    R = FIXUP_LOOP_COPIES
    o, d = rayscheck.reflect()
    ref = set_oracle("reflect")
    want = {k: np.concatenate([ref[k]] * R) for k in CHANNELS}
    with flake("t3") as s:
        o0 = s.stats().overflow_tiles
        got = trace(s, np.concatenate([o] * R), np.concatenate([d] * R), max_depth=4)
        moved = s.stats().overflow_tiles - o0
    print("flagged groups", moved, "per copy", moved / R)
    assert moved > 1024
    assert_same(got, want, f"reflect x {R}, 4 levels")


def test_towards_out_sees_nothing():
    """The reference's quirk (tca >= 0 at the root's bounding ball): all misses, no node entered."""
    o, d = rayscheck.towards_out()
    assert set_oracle("towards_out")["stats"]["hits"] == 0
    with flake("t3") as s:
        before = s.stats()
        got = trace(s, o, d)
        st = s.stats()
    assert_same(got, set_oracle("towards_out"), "towards-out")
    assert (got["minT"] == FLT_MAX).all() and (got["index"] == 0xffffffff).all()
    assert st.max_depth == before.max_depth and np.float32(st.closest) == np.float32(before.closest)
    assert st.overflow_tiles == before.overflow_tiles and st.rays == before.rays + 64


# 4 (the rest) ----------------------------------------------------------------------------------------
def test_jitter_permuted_and_prefixes():
    o, d = rayscheck.jitter()
    ref = set_oracle("jitter")
    n = d.shape[0]
    perm = np.random.default_rng(13).permutation(n)
    want = {k: ref[k][perm] for k in CHANNELS}
    with flake("t1") as s:
        got = trace(s, o[perm], d[perm])
        assert_same(got, want, "jitter permuted")
        for m in (1, 63, 64, 65):
            got = trace(s, o[perm][:m], d[perm][:m])
            assert_same(got, {k: want[k][:m] for k in CHANNELS}, f"jitter prefix {m}")
        assert s.stats().rays == n + 1 + 63 + 64 + 65


# 5 ---------------------------------------------------------------------------------------------------
BAD_ORIGINS = np.array([(np.nan, 0.0, 0.0), (np.inf, 1.0, 1.0), (1.0, -np.inf, 1.0)], np.float32)
BAD_DIRS = np.array([(0.0, 0.0, 0.0), (np.nan, 1.0, 1.0), (np.inf, 1.0, 1.0), (1.0, -np.inf, 1.0)], np.float32)


@pytest.mark.parametrize("what", ["origins", "dirs"])
@pytest.mark.parametrize("pattern", ["lanes", "wave", "uniform"])
def test_non_finite_rays_are_misses_and_harmless(pattern, what):
    """Non-finite origins and directions in lanes 0, 32 and 63 of the first wave, in a whole wave, and in a group
    whose other rays share one origin: misses, as the oracle makes them, and no other ray changes."""
    children = view("t1")["children"]
    probe_d = pinhole("t1").reshape(-1, 3)[[0, 700, 1500, 2303]]
    for b in BAD_ORIGINS:   # (the oracle first: a non-finite origin is a miss whatever the direction)
        assert oracle_multi(children, b.reshape(1, 3), probe_d, rays_per_origin=4)["stats"]["hits"] == 0
    if pattern == "uniform":
        n = 128
        pix = np.random.default_rng(17).choice(64 * 36, size=n, replace=False)
        d = pinhole("t1").reshape(-1, 3)[pix].copy()
        o = np.repeat(origin_of("t1").reshape(1, 3), n, axis=0)
        f = frame("t1")
        ref = {k: flat(f)[k][pix] for k in CHANNELS}
        lanes = [0, 32, 63]
    else:
        # the jitter list with its hits first, so that the first wave's rays are hits to begin with
        full = set_oracle("jitter")
        order = np.argsort(~(full["minT"] < FLT_MAX), kind="stable")
        o, d = (a[order].copy() for a in rayscheck.jitter())
        ref = {k: full[k][order] for k in CHANNELS}
        lanes = [0, 32, 63] if pattern == "lanes" else list(range(64))
        assert (ref["minT"][:64] < FLT_MAX).all()
    assert (ref["minT"][lanes] < FLT_MAX).any()   # (the rays replaced were not misses anyway)
    for j, r in enumerate(lanes):
        if what == "origins":
            o[r] = BAD_ORIGINS[j % len(BAD_ORIGINS)]
        else:
            d[r] = BAD_DIRS[j % len(BAD_DIRS)]
    with flake("t1") as s:
        got = trace(s, o, d)
    keep = np.ones(d.shape[0], bool)
    keep[lanes] = False
    assert_same(got, ref, f"{pattern} {what}", sel=keep)
    for r in lanes:
        assert same_bits(got["pos4"][r], MISS4) and same_bits(got["nrm4"][r], MISS4)
        assert got["minT"][r] == FLT_MAX and got["index"][r] == 0xffffffff


# 6 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", [False, True])
def test_zero_signs(forced, monkeypatch):
    """Origins with exact +0 and -0 components and axis-aligned directions (zeros +0, the sign the oracle's ray
    generation keeps): as one group of several origins, and one origin at a time."""
    if forced:
        monkeypatch.setenv("SF_FLAGS", FORCE_MIXED)
    o = np.array([(0.0, 0.0, 3.0), (-0.0, 2.5, 0.0), (0.0, -3.0, -0.0), (2.75, 0.0, -0.0), (-0.0, -0.0, -4.0),
                  (0.0, 0.0, 0.0)], np.float32)
    axes = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.float32)
    assert not np.signbit(axes[axes == 0.0]).any()
    d = np.tile(axes, (o.shape[0], 1))
    ref = oracle_multi(view("t2")["children"], o, d, rays_per_origin=6)
    assert ref["stats"]["hits"] >= 5
    with flake("t2") as s:
        got = trace(s, o, d, rpo=6)
        assert_same(got, ref, "zero signs, one group")
        for k in range(o.shape[0]):
            got = trace(s, o[k:k + 1], axes, rpo=6)
            assert_same(got, {c: ref[c][6 * k:6 * k + 6] for c in CHANNELS}, f"zero signs, origin {k}")


# 7 ---------------------------------------------------------------------------------------------------
def test_callers_stream_between_renders():
    """Render, rays on a caller's torch stream into caller tensors, Render -- no host synchronisation in between."""
    import torch
    S = view("t3")
    W, H = S["W"], S["H"]
    ref = frame("t3")
    o, d = rayscheck.reflect()
    want = set_oracle("reflect")
    n = d.shape[0]
    mk = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device="cuda")
    a = (mk(H, W, 4), mk(H, W, 4), mk(H, W), mk(H, W, dt=torch.int32))
    b = (mk(n, 4), mk(n, 4), mk(n), mk(n, dt=torch.int32))
    ot, dt = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    ts = torch.cuda.Stream()
    torch.cuda.synchronize()
    with flake("t3") as s:
        s.render_to(a[0].data_ptr(), a[1].data_ptr(), a[2].data_ptr(), a[3].data_ptr(), emit_aux=True)
        s.trace_rays(ot, dt, out=b, stream=ts.cuda_stream)
        s.Render(emit_aux=True)
        pos, nrm, mint, idx = s.download(aux=True)   # (synchronises the context, whatever stream its work ran on)
        assert s.stats().rays == 2 * W * H + n
        for what, t, r in (("render_to", a, ref), ("trace_rays", b, want)):
            got = {"pos4": t[0].cpu().numpy(), "nrm4": t[1].cpu().numpy(), "minT": t[2].cpu().numpy(),
                   "index": t[3].cpu().numpy().view(np.uint32)}
            assert_same(got, r, what)
        assert_same({"pos4": pos, "nrm4": nrm, "minT": mint, "index": idx}, ref, "Render")


def test_progressive_after_rays():
    """The frame-less mode's p1 fixture on a context that traced rays first."""
    fx = load_progressive("p1")
    W, H, K = fx["W"], fx["H"], float.fromhex(fx["K"])
    o, d = rayscheck.jitter()
    with sf.Sphereflake(W, H) as s:
        s.SetCamera(sf.config_camera(W, H, K))
        s.trace_rays(o[:300], d[:300])
        s.trace_rays(o[:1], d[:100], rays_per_origin=100, max_depth=4)
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


# 8 ---------------------------------------------------------------------------------------------------
def test_probe_rays_look_ahead():
    S = view("t2")
    cam = sf.config_camera(S["W"], S["H"], S["K"])
    step = np.float32(0.25)
    o, d = rays.look_ahead(cam, 3, step)
    assert not np.signbit(d[d == 0.0]).any()
    ref = oracle_multi(S["children"], o, d, rays_per_origin=6)
    assert 0 < ref["stats"]["hits"] < d.shape[0]
    with flake("t2") as s:
        mint, idx, pos, nrm = s.probe_rays(o, d, rays_per_origin=6)
        assert s.stats().rays == d.shape[0]
        got = dict(zip(CHANNELS, s.trace_rays(o, d, rays_per_origin=6)))   # the numpy path
    assert_same({"pos4": pos, "nrm4": nrm, "minT": mint, "index": idx}, ref, "probe_rays")
    assert_same(got, ref, "trace_rays (host arrays)")


# 9 ---------------------------------------------------------------------------------------------------
def test_error_codes():
    import torch
    L = sf.lib()
    oj, dj = rayscheck.jitter()
    d = torch.from_numpy(dj[:512]).cuda()
    og = torch.from_numpy(oj[:512]).cuda()
    o = torch.zeros(512 * 4, dtype=torch.float32, device="cuda")
    dp, gp, op = ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(og.data_ptr()), ctypes.c_void_p(o.data_ptr())
    P = lambda w, h, ds=3, os_=3, rpo=1: ctypes.byref(sf.sf_rays_params(w, h, ds, os_, rpo, 0, None))
    hd, ho = np.ascontiguousarray(dj[:7]), np.ascontiguousarray(oj[:7])
    hp, hop = hd.ctypes.data_as(ctypes.c_void_p), ho.ctypes.data_as(ctypes.c_void_p)
    hout = np.empty(512, np.float32)
    houtp = hout.ctypes.data_as(ctypes.c_void_p)
    with sf.Sphereflake(64, 36) as s:
        assert L.sf_trace_rays_to(s.ctx, P(512, 1), gp, dp, op, None, None, None) == sf.SF_ENOVIEW
        assert L.sf_probe_rays(s.ctx, hop, hp, 7, 1, houtp, None, None, None) == sf.SF_ENOVIEW
        S = view("t1")
        s.SetView(S["origin"], S["tl"], S["tr"], S["bl"])
        for ds, os_ in ((2, 3), (5, 3), (3, 2), (3, 5), (0, 3), (3, 0)):
            assert L.sf_trace_rays_to(s.ctx, P(512, 1, ds, os_), gp, dp, op, None, None, None) == sf.SF_EINVAL
        assert L.sf_trace_rays_to(s.ctx, P(512, 1), None, dp, op, None, None, None) == sf.SF_EINVAL
        assert L.sf_trace_rays_to(s.ctx, P(512, 1), gp, None, op, None, None, None) == sf.SF_EINVAL
        assert L.sf_trace_rays_to(s.ctx, P(512, 1), gp, dp, None, None, None, None) == sf.SF_EINVAL
        assert L.sf_trace_rays_to(s.ctx, P(1 << 16, 1 << 15), gp, dp, op, None, None, None) == sf.SF_EINVAL   # 2^31 rays
        assert L.sf_probe_rays(s.ctx, hop, hp, 7, 1, None, None, None, None) == sf.SF_EINVAL
        assert L.sf_probe_rays(s.ctx, None, hp, 7, 1, houtp, None, None, None) == sf.SF_EINVAL
        assert L.sf_trace_rays_to(s.ctx, P(0, 1), gp, dp, op, None, None, None) == sf.SF_OK
        assert L.sf_trace_rays_to(s.ctx, P(64, 0), gp, dp, op, None, None, None) == sf.SF_OK
        assert L.sf_probe_rays(s.ctx, hop, hp, 0, 1, houtp, None, None, None) == sf.SF_OK
        s.Synchronize()
        assert s.stats().rays == 0
        assert (o == 0).all()
        # one output alone is enough
        assert L.sf_trace_rays_to(s.ctx, P(512, 1), gp, dp, None, None, op, None) == sf.SF_OK
        s.Synchronize()
        assert same_bits(o[:512].cpu().numpy(), set_oracle("jitter")["minT"][:512])
