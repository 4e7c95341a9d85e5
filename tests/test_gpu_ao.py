"""Ray-traced ambient occlusion about each pixel's normal on the GPU (sf_trace_ao_to / sf_trace_ao /
sf_trace_ao_sum_to / sf_trace_ao_sum): bit i of every pixel's mask word equals the CPU oracle's answer for the ray of
sample i turned about that pixel's own normal (tests/aocheck.py), a constant normal image gives trace_suns' bits for
lights.ao_directions of that normal, and the summing call equals sphereflake_amd.lights.ao_sum_model over trace_ao's
mask. Everything is compared bit for bit."""
import ctypes

import numpy as np
import pytest

import sphereflake_amd as sf
from sphereflake_amd import lights
from dirscheck import same_bits
from lightsumcheck import BASE, CONE_COLOURS, assert_same, base_image, colours
from maskcheck import assert_mask, assert_shape_of_mask, low, surface_of
from oracle import pyoracle
from rayscheck import frame
import aocheck as ac
import suncheck as su

pytestmark = pytest.mark.gpu

F = np.float32
BIASES = (0.0, ac.B10)
FIXUP_LOOP_COPIES = 38   # (t3 at 4 levels flags nearly every tile of a copy's 56.25: as tests/test_gpu_suns.py)
H8 = lights.ao_samples(8)
KW = dict(distance=ac.TAU, bias=ac.B10)


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


def constant_image(shape, N0):
    nrm = np.empty(tuple(shape) + (4,), F)
    nrm[...] = np.array(tuple(N0) + (0.0,), F)
    return nrm


# 1 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", [("t1", "avx"), ("t3", "avx"), ("t1", "sse")])
def test_eight_samples_equal_the_oracle(name, variant):
    """The oracle's own frame -- positions and normals -- uploaded; ao_samples(8), tau = 4, both biases. t1: all 830
    surface pixels; t3: every 3rd (1200). Compared: the traced pixels and every miss of the frame."""
    every = ac.EVERY[name]
    ref = frame(name, variant)
    pos, nrm = ref["pos4"], ref["nrm4"]
    with flake(name, variant) as s:
        for bias in BIASES:
            want, pick = ac.oracle_mask(name, H8, ac.TAU, bias, variant, None, every)
            if variant == "avx" and bias == ac.B10:   # a constant mask cannot pass
                c = ac.counts(want, 8, pick)
                print(name, "lit / occluded per sample", c)
                assert min(x[0] for x in c) >= 100 and min(x[1] for x in c) >= 100
            got = s.trace_ao(H8, ac.TAU, bias, pos=pos, nrm=nrm)
            where = ac.compared(pos, pick)
            assert (where | surface_of(pos)).all() and int(where.sum()) == int(pick.sum()) + int((~surface_of(pos)).sum())
            assert_mask(got, want, f"{name} {variant} bias {bias}", where)
            assert_shape_of_mask(got, 8, pos, f"{name} {variant} bias {bias}")


# 2 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t1", "t3"])
def test_all_64_bits(name):
    """ao_samples(64), whole images: the prefixes n = 1 and 33 equal the low bits of n = 64. On t1 every 8th surface
    pixel (104) also equals the oracle, where at least 8 samples of index >= 32 have at least 20 pixels of each outcome
    (tests/test_ao_host.py): a 32-bit shift cannot pass."""
    ref = frame(name)
    pos, nrm = ref["pos4"], ref["nrm4"]
    h = lights.ao_samples(64)
    with flake(name) as s:
        m64 = s.trace_ao(h, pos=pos, nrm=nrm, **KW)
        assert_shape_of_mask(m64, 64, pos, f"{name} n = 64")
        for n in (1, 33):
            got = s.trace_ao(h[:n], pos=pos, nrm=nrm, **KW)
            assert_mask(got, m64 & low(n), f"{name} n = {n}")
            assert_shape_of_mask(got, n, pos, f"{name} n = {n}")
    surf = surface_of(pos)
    assert int(ac.mixed(m64 >> np.uint64(32), 32, surf).sum()) >= 100   # the high word is alive
    if name == "t1":
        want, pick = ac.oracle_mask("t1", h, ac.TAU, ac.B10, "avx", None, ac.SKY_EVERY)
        c = ac.counts(want, 64, pick)
        both = [i for i in range(32, 64) if c[i][0] >= 20 and c[i][1] >= 20]
        print("samples >= 32 with both outcomes", len(both))
        assert len(both) >= 8
        assert_mask(m64, want, "t1, 64 samples, against the oracle", ac.compared(pos, pick))


# 3 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N0", ac.CONSTANT_NORMALS)
def test_constant_normal_is_trace_suns(N0):
    """t3's positions under one constant normal: trace_ao equals trace_suns of lights.ao_directions(N0, samples), whole
    image -- the product s tau is formed on the host there and on the device here."""
    pos = frame("t3")["pos4"]
    nrm = constant_image(pos.shape[:2], N0)
    h = lights.ao_samples(16)
    D = lights.ao_directions(np.array(N0, F), h)
    assert D.shape == (16, 3) and np.isfinite(D).all()
    with flake("t3") as s:
        want = s.trace_suns(D, ac.TAU, bias=ac.B10, pos=pos)
        got = s.trace_ao(h, pos=pos, nrm=nrm, **KW)
    assert_mask(got, want, f"N0 = {N0}")
    assert_shape_of_mask(got, 16, pos, f"N0 = {N0}")
    c = ac.counts(got, 16, surface_of(pos))
    assert max(min(x) for x in c) >= 100   # some sample has both outcomes in quantity


# 4 ---------------------------------------------------------------------------------------------------
def test_order_and_rays_that_are_not_traced():
    """A permutation of the samples permutes the bits; a NaN, an infinite and a zero sample among good ones set their
    own bit everywhere and leave the others' alone; a caller's NaN normal at some surface pixels sets those pixels' low
    n bits and changes no other pixel."""
    ref = frame("t3")
    pos, nrm = ref["pos4"], ref["nrm4"]
    surf = surface_of(pos)
    perm = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    with flake("t3") as s:
        base = s.trace_ao(H8, pos=pos, nrm=nrm, **KW)
        assert int(ac.mixed(base, 8, surf).sum()) >= 100   # the bits differ between samples
        got = s.trace_ao(H8[perm], pos=pos, nrm=nrm, **KW)
        for j in range(8):
            assert np.array_equal(ac.bit(got, j), ac.bit(base, perm[j])), j
        bad = np.array([H8[0], (np.nan, 0.0, 1.0), H8[1], (np.inf, 0.0, 0.0), H8[2], (0.0, 0.0, 0.0), H8[3]], F)
        got = s.trace_ao(bad, pos=pos, nrm=nrm, **KW)
        for j in (1, 3, 5):
            assert ac.bit(got, j).all(), j
        for j, i in ((0, 0), (2, 1), (4, 2), (6, 3)):
            assert np.array_equal(ac.bit(got, j), ac.bit(base, i)), j
        assert_shape_of_mask(got, 7, pos, "bad samples")
        only = s.trace_ao([(0.0, -np.inf, 3.0)], pos=pos, nrm=nrm, **KW)
        assert (only == np.uint64(1)).all()
        # NaN normals: every 5th surface pixel, one component each in turn; an infinite one among them
        hurt = np.zeros(surf.shape, bool).reshape(-1)
        idx = np.nonzero(surf.reshape(-1))[0][::5]
        hurt[idx] = True
        hurt = hurt.reshape(surf.shape)
        bad_n = np.array(nrm, F, copy=True).reshape(-1, 4)
        for k, p in enumerate(idx):
            bad_n[p, k % 3] = np.inf if k % 7 == 3 else np.nan
        got = s.trace_ao(H8, pos=pos, nrm=bad_n.reshape(nrm.shape), **KW)
    assert int(hurt.sum()) >= 500 and int((hurt & (base != low(8))).sum()) >= 100   # (the NaN changed something)
    assert (got[hurt] == low(8)).all(), "a NaN normal traced a ray"
    assert_mask(got, base, "the other pixels", ~hurt)


# 5 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tiles", [("t3", 60), ("t1", 40)])
def test_overflow_tiles_are_retraced_once_for_all_samples(name, tiles):
    """max_depth = 4 provisions too few levels (the rays reach depth 7): same bits, the oracle's on its sample, and the
    re-trace counter moved by tiles, not by tiles x samples."""
    ref = frame(name)
    pos, nrm = ref["pos4"], ref["nrm4"]
    want, pick = ac.oracle_mask(name, H8, ac.TAU, ac.B10, "avx", None, ac.EVERY[name])
    with flake(name) as s:
        base = s.trace_ao(H8, pos=pos, nrm=nrm, **KW)
        o0 = s.stats().overflow_tiles
        got = s.trace_ao(H8, pos=pos, nrm=nrm, max_depth=4, **KW)
        moved = s.stats().overflow_tiles - o0
    print(name, "flagged tiles", moved)
    assert_mask(got, base, f"{name} max_depth = 4")
    assert_mask(got, want, f"{name} max_depth = 4 against the oracle", ac.compared(pos, pick))
    assert 1 <= moved <= tiles


def test_more_flagged_tiles_than_fixup_blocks():
    """t3's frame stacked R times into one 80 x 45R image, two samples, max_depth = 4: more flagged tiles than the
    re-trace launch has blocks (1024), so its blocks walk the list more than once. 45 is no multiple of 8: the copies
    fall differently into tiles, the per-pixel masks are the same."""
    R = FIXUP_LOOP_COPIES
    h = H8[[1, 6]]
    ref = frame("t3")
    one_p, one_n = ref["pos4"], ref["nrm4"]
    pos, nrm = np.concatenate([one_p] * R), np.concatenate([one_n] * R)
    with flake("t3") as s:
        base = s.trace_ao(h, pos=one_p, nrm=one_n, **KW)
        o0 = s.stats().overflow_tiles
        got = s.trace_ao(h, pos=pos, nrm=nrm, max_depth=4, **KW)
        moved = s.stats().overflow_tiles - o0
    print("flagged tiles", moved, "per copy", moved / R)
    assert moved > 1024
    assert int(ac.mixed(base, 2, surface_of(one_p)).sum()) >= 20
    assert_mask(got, np.concatenate([base] * R), f"t3 x {R}, 4 levels")


# 6 ---------------------------------------------------------------------------------------------------
def test_partial_tiles():
    """A 13 x 11 crop (partial tiles in both directions), as numpy arrays and as torch tensors with guard words before
    and after the output, for the mask and for the light buffer: it equals the crop of the whole and the guards are
    intact."""
    import torch
    ref = frame("t3")
    y0, x0, h, w = 17, 30, 11, 13
    pos = np.ascontiguousarray(ref["pos4"][y0:y0 + h, x0:x0 + w])
    nrm = np.ascontiguousarray(ref["nrm4"][y0:y0 + h, x0:x0 + w])
    guard, sentinel, fsentinel = 8, 0x5a5a5a5a5a5a5a5a, -123.25
    col = CONE_COLOURS
    with flake("t3") as s:
        sub = s.trace_ao(H8, pos=ref["pos4"], nrm=ref["nrm4"], **KW)[y0:y0 + h, x0:x0 + w]
        sub_sum = s.trace_ao_sum(H8, col, pos=ref["pos4"], nrm=ref["nrm4"], **KW)[y0:y0 + h, x0:x0 + w]
        assert len(np.unique(sub)) >= 3
        assert_mask(s.trace_ao(H8, pos=pos, nrm=nrm, **KW), sub, "numpy crop")
        assert_same(s.trace_ao_sum(H8, col, pos=pos, nrm=nrm, **KW), np.ascontiguousarray(sub_sum), "numpy crop, summed")
        pt, nt = torch.from_numpy(pos).cuda(), torch.from_numpy(nrm).cuda()
        out = torch.full((guard + h * w + guard,), sentinel, dtype=torch.int64, device="cuda")
        fout = torch.full((2 * guard + h * w * 4 + 2 * guard,), fsentinel, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        s.trace_ao(H8, pos=pt, nrm=nt, out=out.data_ptr() + 8 * guard, **KW)
        s.trace_ao_sum(H8, col, pos=pt, nrm=(nt.data_ptr(), w, h), out=fout.data_ptr() + 8 * guard, **KW)
        s.Synchronize()
        o = out.cpu().numpy().view(np.uint64)
        assert (o[:guard] == np.uint64(sentinel)).all(), "wrote before the first pixel"
        assert (o[guard + h * w:] == np.uint64(sentinel)).all(), "wrote past the last pixel"
        assert_mask(o[guard:guard + h * w].reshape(h, w), sub, "torch crop")
        fo = fout.cpu().numpy()
        assert (fo[:2 * guard] == F(fsentinel)).all() and (fo[2 * guard + h * w * 4:] == F(fsentinel)).all(), "guards"
        assert_same(fo[2 * guard:2 * guard + h * w * 4].reshape(h, w, 4), np.ascontiguousarray(sub_sum), "torch crop, summed")


# 7 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t1", "t3"])
def test_the_sum_equals_the_model_over_the_mask(name):
    ref = frame(name)
    pos, nrm = ref["pos4"], ref["nrm4"]
    h = lights.ao_samples(64)
    with flake(name) as s:
        for n in (8, 33, 64):
            col = colours(n)
            mask = s.trace_ao(h[:n], pos=pos, nrm=nrm, **KW)
            got = s.trace_ao_sum(h[:n], col, pos=pos, nrm=nrm, **KW)
            assert_same(got, lights.ao_sum_model(None, pos, mask, col), f"{name} n = {n}")
            assert (got[~surface_of(pos)] == 0).all() and (got[..., 3] == 0).all()
        rgb = got[surface_of(pos)][:, :3]
        assert len(np.unique(rgb[:, 0])) > 100   # visibility shows
        # colours None: 1 / n per component
        mask = s.trace_ao(h[:33], pos=pos, nrm=nrm, **KW)
        assert_same(s.trace_ao_sum(h[:33], None, pos=pos, nrm=nrm, **KW),
                    lights.ao_sum_model(None, pos, mask, np.full((33, 3), F(1.0) / F(33), F)), f"{name} even colours")


@pytest.mark.parametrize("depth", [0, 4])
def test_a_call_equals_its_split(depth):
    """One call of 8 equals an overwriting call of k and an accumulating call of 8 - k, for k = 1 and 5 -- also at
    max_depth = 4, where a flagged tile must not add its chunk twice."""
    ref = frame("t3")
    pos, nrm = ref["pos4"], ref["nrm4"]
    col = colours(8)
    kw = dict(pos=pos, nrm=nrm, max_depth=depth, **KW)
    with flake("t3") as s:
        whole = s.trace_ao_sum(H8, col, pos=pos, nrm=nrm, **KW)
        o0 = s.stats().overflow_tiles
        assert_same(s.trace_ao_sum(H8, col, **kw), whole, f"one call at max_depth = {depth}")
        for k in (1, 5):
            first = s.trace_ao_sum(H8[:k], col[:k], **kw)
            both = s.trace_ao_sum(H8[k:], col[k:], accumulate=True, out=first, **kw)
            assert_same(both, whole, f"split at {k}, max_depth = {depth}")
        moved = s.stats().overflow_tiles - o0
        # an accumulating call on a non-zero base (a .w the trace must carry): a chunk added twice shows here
        base = base_image(pos.shape[:2])
        acc = s.trace_ao_sum(H8, col, accumulate=True, out=base, **kw)
        mask = s.trace_ao(H8, pos=pos, nrm=nrm, **KW)
    print("flagged tiles over five launches", moved)
    if depth:   # (every one of the five launches re-traced at least a tile: the flagged-tile rule was exercised)
        assert moved >= 5
    assert_same(acc, lights.ao_sum_model(base, pos, mask, col, True), f"accumulating, max_depth = {depth}")


def test_accumulate_and_misses():
    """Misses are zeroed by an overwriting call and left alone by an accumulating one; .w is carried."""
    import torch
    ref = frame("t1")
    pos, nrm = ref["pos4"], ref["nrm4"]
    miss = ~surface_of(pos)
    assert int(miss.sum()) >= 100
    base = base_image(pos.shape[:2])
    col = CONE_COLOURS
    with flake("t1") as s:
        mask = s.trace_ao(H8, pos=pos, nrm=nrm, **KW)
        acc = s.trace_ao_sum(H8, col, accumulate=True, out=base, pos=pos, nrm=nrm, **KW)
        assert same_bits(acc[miss], base[miss]), "an accumulating call wrote a miss"
        assert (acc[..., 3] == F(BASE[3])).all(), ".w was not carried"
        assert_same(acc, lights.ao_sum_model(base, pos, mask, col, True), "accumulating")
        assert (acc[~miss][:, :3] != base[~miss][:, :3]).any()
        out = torch.from_numpy(base).cuda()   # an overwriting call into a buffer that holds the base
        pt, nt = torch.from_numpy(np.ascontiguousarray(pos)).cuda(), torch.from_numpy(np.ascontiguousarray(nrm)).cuda()
        s.trace_ao_sum(H8, col, pos=pt, nrm=nt, out=out, **KW)
        s.Synchronize()
        over = out.cpu().numpy()
        assert (over[miss] == 0).all() and (over[..., 3] == 0).all()
        assert_same(over, lights.ao_sum_model(None, pos, mask, col), "overwriting")


def test_fill_then_ao_then_resolve():
    """The README's order on a real Render() + PostProcess(): light_fill(0), trace_ao_sum(accumulate=True) with a sky
    colour, light_image_buffer -- the buffer is ao_sum_model over trace_ao's mask, the image light_model_buffer's."""
    h = lights.ao_samples(32)
    col = lights.ao_colours(h, (0.5, 0.75, 1.0))
    with flake("t3") as s:
        s.Render()
        s.PostProcess()
        img = s.download_image()
        pos, nrm, _, _ = s.download()
        s.light_fill((0.0, 0.0, 0.0))
        filled = s.download_light()
        s.trace_ao_sum(h, col, accumulate=True, **KW)
        buf = s.download_light()
        s.trace_ao(h, **KW)
        mask = s.download_shadow_masks()
        s.light_image_buffer()
        got = s.download_image()
    assert_same(buf, lights.ao_sum_model(filled, pos, mask, col, True), "the buffer")
    assert np.array_equal(got, lights.light_model_buffer(img, pos, buf)) and np.array_equal(got[..., 3], img[..., 3])
    assert (got != img).any() and len(np.unique(got[..., :3])) > 16
    assert int(ac.mixed(mask, 32, surface_of(pos)).sum()) >= 100


# 8 ---------------------------------------------------------------------------------------------------
def test_shadow_lod_constant():
    """set_shadow_lod(matched_lod(4, 0.1258)) (C about 394.7) on t3, every 3rd surface pixel, against the oracle at
    that constant; it differs from the default's bits; set_shadow_lod(0) restores them."""
    ref = frame("t3")
    pos, nrm = ref["pos4"], ref["nrm4"]
    C = float(lights.matched_lod(4, 0.1258))
    assert C == su.matched()
    want, pick = ac.oracle_mask("t3", H8, ac.TAU, ac.B10, "avx", C, 3)
    where = ac.compared(pos, pick)
    with flake("t3") as s:
        base = s.trace_ao(H8, pos=pos, nrm=nrm, **KW)
        s.set_shadow_lod(C)
        got = s.trace_ao(H8, pos=pos, nrm=nrm, **KW)
        s.set_shadow_lod(0.0)
        again = s.trace_ao(H8, pos=pos, nrm=nrm, **KW)
    assert_mask(got, want, f"C = {C}", where)
    differ = sum(int((pick & (ac.bit(got, i) != ac.bit(base, i))).sum()) for i in range(8))
    print("sampled bits that differ from the default's", differ)
    assert differ >= 20
    assert_mask(again, base, "C = 0 again")


# 9 ---------------------------------------------------------------------------------------------------
def test_callers_stream_between_renders_and_the_shared_buffers():
    """Render, the two traces on a caller's torch stream (the caller's tensors, the context's own buffers), Render -- no
    host synchronisation in between. The statistics are what two renders alone leave and the later render's bits are
    the oracle frame's; the mask buffer is the one trace_suns writes."""
    import torch
    S = pyoracle.load_setup("t3")
    W, H = S["W"], S["H"]
    ref = frame("t3")
    col = CONE_COLOURS
    want, pick = ac.oracle_mask("t3", H8, ac.TAU, ac.B10, "avx", None, ac.EVERY["t3"])
    where = ac.compared(ref["pos4"], pick)
    with flake("t3") as s:   # what two renders alone leave
        s.Render(emit_aux=True)
        s.Render(emit_aux=True)
        s.Synchronize()
        st0 = s.stats()
        alone = (st0.max_depth, np.float32(st0.closest), st0.rays, st0.overflow_tiles)
    pt = torch.from_numpy(np.ascontiguousarray(ref["pos4"])).cuda()
    nt = torch.from_numpy(np.ascontiguousarray(ref["nrm4"])).cuda()
    out = torch.full((H, W), 7, dtype=torch.int64, device="cuda")
    fout = torch.full((H, W, 4), 7.0, dtype=torch.float32, device="cuda")
    ts = torch.cuda.Stream()
    torch.cuda.synchronize()
    host = np.empty((H, W), np.uint64)
    with flake("t3") as s:
        s.Render(emit_aux=True)
        assert s.shadow_mask_buffer() == 0 and s.light_buffer() == 0
        assert sf.lib().sf_download_shadow_masks(s.ctx, host.ctypes.data_as(ctypes.c_void_p)) == sf.SF_ESTATE
        s.trace_ao(H8, pos=pt, nrm=nt, out=out, stream=ts.cuda_stream, **KW)
        s.trace_ao_sum(H8, col, pos=pt, nrm=nt, out=fout, stream=ts.cuda_stream, **KW)
        assert s.trace_ao(H8[::-1], stream=ts.cuda_stream) is None   # the context's frame, its buffer, the defaults
        assert s.trace_ao_sum(H8, col, stream=ts.cuda_stream) is None
        s.Render(emit_aux=True)
        pos, nrm, mint, idx = s.download(aux=True)   # (synchronises the context, whatever stream its work ran on)
        st = s.stats()
        assert (st.max_depth, np.float32(st.closest), st.rays, st.overflow_tiles) == alone
        for k, a in (("pos4", pos), ("nrm4", nrm), ("minT", mint), ("index", idx)):
            assert same_bits(a, ref[k]), f"Render after the occlusion traces: {k} differs"
        theirs = out.cpu().numpy().view(np.uint64)
        assert_mask(theirs, want, "caller's tensors", where)
        own = s.download_shadow_masks()
        assert s.shadow_mask_buffer() != 0 and s.light_buffer() != 0
        for j in range(8):
            assert np.array_equal(ac.bit(own, j), ac.bit(theirs, 7 - j)), j
        summed = lights.ao_sum_model(None, ref["pos4"], theirs, col)
        assert_same(fout.cpu().numpy(), summed, "caller's light buffer")
        assert_same(s.download_light(), summed, "the context's light buffer")
        p, keep = s.ao_params(H8)
        assert (p.n, p.accumulate, p.distance, p.bias) == (8, 0, 4.0, 2.0 ** -10)
        # the mask buffer is trace_suns' too
        D = lights.sky_dirs(3)
        s.trace_suns(D, ac.TAU, bias=ac.B10)
        assert_mask(s.download_shadow_masks(), s.trace_suns(D, ac.TAU, bias=ac.B10, pos=ref["pos4"]), "trace_suns after")


# 10 --------------------------------------------------------------------------------------------------
def test_error_codes():
    import torch
    Lb = sf.lib()
    pos = torch.zeros((36, 64, 4), dtype=torch.float32, device="cuda")
    out = torch.full((36 * 64,), 9, dtype=torch.int64, device="cuda")
    fout = torch.full((36 * 64 * 4,), 9.0, dtype=torch.float32, device="cuda")
    pp, op, fp_ = (ctypes.c_void_p(t.data_ptr()) for t in (pos, out, fout))
    three = lights.ao_samples(3)
    fp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    keep = []

    def P(w=0, h=0, bias=ac.B10, max_depth=0, n=3, samples=three, cols=None, distance=4.0, accumulate=0):
        p = sf.sf_ao_params()
        if samples is not None:
            p.samples = fp(samples)
        if cols is not None:
            ca = np.ascontiguousarray(cols, np.float32)
            keep.append(ca)
            p.colours = fp(ca)
        p.n, p.distance, p.bias, p.width, p.height, p.max_depth, p.accumulate = n, distance, bias, w, h, max_depth, accumulate
        return ctypes.byref(p)

    many = np.tile(np.array([[0.0, 0.6, 0.8]], np.float32), (65, 1))
    with sf.Sphereflake(64, 36) as s:
        d = sf.sf_ao_params()
        d.n = 5
        assert Lb.sf_ao_defaults(s.ctx, ctypes.byref(d)) == sf.SF_OK and Lb.sf_ao_defaults(s.ctx, None) == sf.SF_EINVAL
        assert (bool(d.samples), bool(d.colours), d.n, d.accumulate, d.distance, d.bias) == (False, False, 0, 0, 4.0, 2.0 ** -10)
        assert (d.use_origin, d.width, d.height, d.max_depth, d.stream) == (0, 0, 0, 0, None)
        mask_to = lambda p, a=pp, b=pp, c=op: Lb.sf_trace_ao_to(s.ctx, p, a, b, c)
        sum_to = lambda p, a=pp, b=pp, c=fp_: Lb.sf_trace_ao_sum_to(s.ctx, p, a, b, c)
        assert mask_to(P(64, 36)) == sf.SF_ENOVIEW and sum_to(P(64, 36)) == sf.SF_ENOVIEW
        assert Lb.sf_trace_ao(s.ctx, P()) == sf.SF_ENOVIEW and Lb.sf_trace_ao_sum(s.ctx, P()) == sf.SF_ENOVIEW
        S = pyoracle.load_setup("t1")
        s.SetView(S["origin"], S["tl"], S["tr"], S["bl"])
        for call, own in ((mask_to, Lb.sf_trace_ao), (sum_to, Lb.sf_trace_ao_sum)):
            assert call(P(64, 36, n=0)) == sf.SF_EINVAL and own(s.ctx, P(n=0)) == sf.SF_EINVAL
            assert call(P(64, 36, n=65, samples=many)) == sf.SF_EINVAL and own(s.ctx, P(n=65, samples=many)) == sf.SF_EINVAL
            assert call(P(64, 36, samples=None)) == sf.SF_EINVAL and own(s.ctx, P(samples=None)) == sf.SF_EINVAL
            for bias in (-0.25, 1.0, 2.0, float("nan")):
                assert call(P(64, 36, bias=bias)) == sf.SF_EINVAL
            for distance in (0.0, -4.0, float("inf"), float("nan")):
                assert call(P(64, 36, distance=distance)) == sf.SF_EINVAL
                assert own(s.ctx, P(distance=distance)) == sf.SF_EINVAL
            assert call(P(64, 36, max_depth=32)) == sf.SF_EINVAL
            assert call(P(64, 0)) == sf.SF_EINVAL
            assert call(P(32, 16), None) == sf.SF_EINVAL        # sizes against a NULL pos4
            assert call(P(32, 16), pp, None) == sf.SF_EINVAL    # ... a NULL nrm4
            assert call(None) == sf.SF_EINVAL
            assert own(s.ctx, P(32, 16)) == sf.SF_EINVAL
            assert own(s.ctx, None) == sf.SF_EINVAL
        assert mask_to(P(64, 36), pp, pp, None) == sf.SF_EINVAL          # a null mask
        assert sum_to(P(32, 16), pp, pp, None) == sf.SF_EINVAL           # sizes against a NULL out
        for bad in (-0.5, float("nan"), float("inf")):
            cols = [(0.5, 0.5, 0.5), (0.5, bad, 0.5), (0.5, 0.5, 0.5)]
            assert sum_to(P(64, 36, cols=cols)) == sf.SF_EINVAL
            assert Lb.sf_trace_ao_sum(s.ctx, P(cols=cols)) == sf.SF_EINVAL
        # an accumulating call before the light buffer exists
        assert sum_to(P(64, 36), pp, pp, None) == sf.SF_ESTATE
        assert sum_to(P(64, 36, accumulate=1), pp, pp, None) == sf.SF_ESTATE
        assert Lb.sf_trace_ao_sum(s.ctx, P(accumulate=1)) == sf.SF_ESTATE
        assert s.light_buffer() == 0 and s.shadow_mask_buffer() == 0   # (a refused call made no buffer)
        s.Synchronize()
        assert (out == 9).all() and (fout == 9).all()   # none of them wrote
        # a negative colour does not bother the mask trace, which ignores the colours; an all-miss position image:
        # every mask has exactly its low n bits set, an accumulating sum leaves every pixel, an overwriting one zeroes
        assert mask_to(P(64, 36, cols=[(0.5, -0.5, 0.5)] * 3)) == sf.SF_OK
        assert sum_to(P(64, 36, accumulate=1)) == sf.SF_OK
        s.Synchronize()
        assert (out == 7).all() and (fout == 9).all()
        assert sum_to(P(64, 36)) == sf.SF_OK
        s.Synchronize()
        assert (fout == 0).all() and s.stats().rays == 0
        dev = (pos.data_ptr(), 64, 36)
        with pytest.raises(ValueError):
            s.trace_ao(many, pos=dev, nrm=dev, out=out)
        with pytest.raises(ValueError):
            s.trace_ao(np.zeros((0, 3), np.float32), pos=dev, nrm=dev, out=out)
        with pytest.raises(ValueError):
            s.trace_ao(three, pos=dev, out=out)   # a device pos without a device nrm
        with pytest.raises(ValueError):
            s.trace_ao(three, pos=np.zeros((36, 64, 4), np.float32))   # a host pos without a host nrm
        with pytest.raises(ValueError):
            s.trace_ao_sum(three, accumulate=True, pos=np.zeros((36, 64, 4), F), nrm=np.zeros((36, 64, 4), F))
