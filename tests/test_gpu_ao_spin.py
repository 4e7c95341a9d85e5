"""Ambient occlusion with a per-pixel spin on the GPU (sf_trace_ao_spin_to / sf_trace_ao_spin / sf_trace_ao_spin_sum_to /
sf_trace_ao_spin_sum): every pixel turns its frame by its own table entry before the samples are laid out. Bit i of
every pixel's word equals the CPU oracle's answer for the spun ray (tests/aospincheck.py); the identity table, a uniform
table, a constant normal and a crop reduce to calls that are pinned elsewhere. Everything is compared bit for bit."""
import ctypes

import numpy as np
import pytest

import sphereflake_amd as sf
from sphereflake_amd import lights
from dirscheck import same_bits
from lightsumcheck import BASE, CONE_COLOURS, assert_same, base_image, colours, surface_of
from oracle import pyoracle
from rayscheck import frame
import aocheck as ac
import aospincheck as sc
from aospincheck import assert_mask, assert_shape_of_mask, constant_image, flake

pytestmark = pytest.mark.gpu

F = np.float32
BIASES = (0.0, ac.B10)
H8 = sc.H8
S4 = lights.ao_spins(4)
KW = dict(distance=ac.TAU, bias=ac.B10)


@pytest.fixture(scope="module", autouse=True)
def device():
    sf.build()
    assert sf.device_count() >= 1, "no HIP device visible: GPU tests must run on an MI355X"


# 1 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,variant", [("t1", "avx"), ("t3", "avx"), ("t1", "sse")])
def test_eight_spun_samples_equal_the_oracle(name, variant):
    """The oracle's own frame uploaded; ao_samples(8) under ao_spins(4), tau = 4, both biases. t1: all 830 surface
    pixels; t3: every 3rd (1200). Compared: the traced pixels and every miss of the frame."""
    every = ac.EVERY[name]
    ref = frame(name, variant)
    pos, nrm = ref["pos4"], ref["nrm4"]
    ent = sc.entry_of(pos.shape[:2], 4)
    with flake(name, variant) as s:
        for bias in BIASES:
            want, pick = sc.oracle_mask(name, H8, S4, ac.TAU, bias, variant, every)
            if variant == "avx" and bias == ac.B10:   # neither an ignored table nor a constant mask can pass
                plain, _ = ac.oracle_mask(name, H8, ac.TAU, bias, variant, None, every)
                differ = [int((pick & (ent == k) & (want != plain)).sum()) for k in range(16)]
                lit = [sum(int((pick & (ent == k) & ac.bit(want, i)).sum()) for i in range(8)) for k in range(16)]
                occ = [sum(int((pick & (ent == k) & ~ac.bit(want, i)).sum()) for i in range(8)) for k in range(16)]
                print(name, "per entry: differ", min(differ), "lit", min(lit), "occluded", min(occ))
                assert min(differ) >= 20 and min(lit) >= 100 and min(occ) >= 100
            got = s.trace_ao(H8, ac.TAU, bias, pos=pos, nrm=nrm, spin=S4)
            where = ac.compared(pos, pick)
            assert int(where.sum()) == int(pick.sum()) + int((~surface_of(pos)).sum())
            assert_mask(got, want, f"{name} {variant} bias {bias}", where)
            assert_shape_of_mask(got, 8, pos, f"{name} {variant} bias {bias}")


# 2 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [3, 8])
def test_other_table_sizes(size):
    """ao_spins(3) does not divide the 8 x 8 tile and ao_spins(8) equals it: t3, every 3rd surface pixel, against the
    oracle."""
    ref = frame("t3")
    pos, nrm = ref["pos4"], ref["nrm4"]
    tab = lights.ao_spins(size)
    want, pick = sc.oracle_mask("t3", H8, tab, ac.TAU, ac.B10, "avx", 3)
    with flake("t3") as s:
        got = s.trace_ao(H8, pos=pos, nrm=nrm, spin=tab, **KW)
        other = s.trace_ao(H8, pos=pos, nrm=nrm, spin=S4, **KW)
    assert_mask(got, want, f"size {size}", ac.compared(pos, pick))
    assert_shape_of_mask(got, 8, pos, f"size {size}")
    assert int((got != other).sum()) >= 500   # (the table's size shows)


# 3 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t1", "t3"])
def test_identity_table_is_the_unspun_call(name):
    """{(1, 0)} equals trace_ao and trace_ao_sum: whole images, n = 64, the mask and the sum."""
    ref = frame(name)
    pos, nrm = ref["pos4"], ref["nrm4"]
    h = lights.ao_samples(64)
    col = colours(64)
    with flake(name) as s:
        assert_mask(s.trace_ao(h, pos=pos, nrm=nrm, spin=sc.IDENTITY, **KW), s.trace_ao(h, pos=pos, nrm=nrm, **KW),
                    f"{name} mask")
        plain = s.trace_ao_sum(h, col, pos=pos, nrm=nrm, **KW)
        assert_same(s.trace_ao_sum(h, col, pos=pos, nrm=nrm, spin=sc.IDENTITY, **KW), plain, f"{name} sum")
        assert_same(s.trace_ao_sum(h, col, pos=pos, nrm=nrm, spin=(1.0, 0.0), **KW), plain, f"{name} sum, a pair")
    assert len(np.unique(plain[surface_of(pos)][:, 0])) > 100


# 4 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N0", ac.CONSTANT_NORMALS)
def test_constant_normal_is_trace_suns(N0):
    """t3's positions under one constant normal and the 1 x 1 table (0.6, 0.8): trace_ao equals trace_suns of
    lights.ao_directions(N0, samples, spin=(0.6, 0.8)), whole image."""
    pos = frame("t3")["pos4"]
    nrm = constant_image(pos.shape[:2], N0)
    h = lights.ao_samples(16)
    D = lights.ao_directions(np.array(N0, F), h, spin=sc.PAIR)
    assert D.shape == (16, 3) and np.isfinite(D).all()
    assert not same_bits(D, lights.ao_directions(np.array(N0, F), h))
    with flake("t3") as s:
        want = s.trace_suns(D, ac.TAU, bias=ac.B10, pos=pos)
        got = s.trace_ao(h, pos=pos, nrm=nrm, spin=np.array(sc.PAIR, F).reshape(1, 1, 2), **KW)
        plain = s.trace_ao(h, pos=pos, nrm=nrm, **KW)
    assert_mask(got, want, f"N0 = {N0}")
    assert_shape_of_mask(got, 16, pos, f"N0 = {N0}")
    assert int((got != plain).sum()) >= 100   # (the turn shows)


# 5 ---------------------------------------------------------------------------------------------------
def test_uniform_table_is_its_one_entry():
    ref = frame("t3")
    pos, nrm = ref["pos4"], ref["nrm4"]
    uniform = np.empty((4, 4, 2), F)
    uniform[...] = np.array(sc.PAIR, F)
    col = CONE_COLOURS
    with flake("t3") as s:
        one = s.trace_ao(H8, pos=pos, nrm=nrm, spin=sc.PAIR, **KW)
        assert_mask(s.trace_ao(H8, pos=pos, nrm=nrm, spin=uniform, **KW), one, "uniform 4 x 4")
        assert_same(s.trace_ao_sum(H8, col, pos=pos, nrm=nrm, spin=uniform, **KW),
                    s.trace_ao_sum(H8, col, pos=pos, nrm=nrm, spin=sc.PAIR, **KW), "uniform 4 x 4, summed")
        plain = s.trace_ao(H8, pos=pos, nrm=nrm, **KW)
    assert int((one != plain).sum()) >= 500


# 6 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("x0,y0", [(28, 16), (30, 17)])
def test_crops(x0, y0):
    """A 13 x 11 crop of t3 (partial tiles in both directions): at multiples of the table's size it equals the crop of
    the whole; elsewhere it does when its table is the whole's rolled by (x0 mod 4, y0 mod 4). As numpy arrays and as
    torch tensors with guard words before and after the mask and the sum outputs."""
    import torch
    ref = frame("t3")
    h, w = 11, 13
    pos = np.ascontiguousarray(ref["pos4"][y0:y0 + h, x0:x0 + w])
    nrm = np.ascontiguousarray(ref["nrm4"][y0:y0 + h, x0:x0 + w])
    tab = np.ascontiguousarray(np.roll(S4, (-(y0 % 4), -(x0 % 4)), axis=(0, 1)))   # tab[y, x] = S4[y + y0, x + x0]
    assert same_bits(tab[0, 0], S4[y0 % 4, x0 % 4]) and (same_bits(tab, S4) == (x0 % 4 == 0 and y0 % 4 == 0))
    guard, sentinel, fsentinel = 8, 0x5a5a5a5a5a5a5a5a, -123.25
    col = CONE_COLOURS
    with flake("t3") as s:
        sub = s.trace_ao(H8, pos=ref["pos4"], nrm=ref["nrm4"], spin=S4, **KW)[y0:y0 + h, x0:x0 + w]
        sub_sum = np.ascontiguousarray(
            s.trace_ao_sum(H8, col, pos=ref["pos4"], nrm=ref["nrm4"], spin=S4, **KW)[y0:y0 + h, x0:x0 + w])
        assert len(np.unique(sub)) >= 3
        assert_mask(s.trace_ao(H8, pos=pos, nrm=nrm, spin=tab, **KW), sub, "numpy crop")
        assert_same(s.trace_ao_sum(H8, col, pos=pos, nrm=nrm, spin=tab, **KW), sub_sum, "numpy crop, summed")
        if x0 % 4 or y0 % 4:   # (the unrolled table is another image there: the roll is needed)
            assert int((s.trace_ao(H8, pos=pos, nrm=nrm, spin=S4, **KW) != sub).sum()) >= 10
        pt, nt = torch.from_numpy(pos).cuda(), torch.from_numpy(nrm).cuda()
        out = torch.full((guard + h * w + guard,), sentinel, dtype=torch.int64, device="cuda")
        fout = torch.full((2 * guard + h * w * 4 + 2 * guard,), fsentinel, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        s.trace_ao(H8, pos=pt, nrm=nt, out=out.data_ptr() + 8 * guard, spin=tab, **KW)
        s.trace_ao_sum(H8, col, pos=pt, nrm=(nt.data_ptr(), w, h), out=fout.data_ptr() + 8 * guard, spin=tab, **KW)
        s.Synchronize()
        o = out.cpu().numpy().view(np.uint64)
        assert (o[:guard] == np.uint64(sentinel)).all(), "wrote before the first pixel"
        assert (o[guard + h * w:] == np.uint64(sentinel)).all(), "wrote past the last pixel"
        assert_mask(o[guard:guard + h * w].reshape(h, w), sub, "torch crop")
        fo = fout.cpu().numpy()
        assert (fo[:2 * guard] == F(fsentinel)).all() and (fo[2 * guard + h * w * 4:] == F(fsentinel)).all(), "guards"
        assert_same(fo[2 * guard:2 * guard + h * w * 4].reshape(h, w, 4), sub_sum, "torch crop, summed")


# 7 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,tiles", [("t3", 60), ("t1", 40)])
def test_overflow_tiles_are_retraced_once_for_all_samples(name, tiles):
    """max_depth = 4 provisions too few levels: the same bits, the oracle's on its sample, and the re-trace counter
    moved by tiles, not by tiles x samples."""
    ref = frame(name)
    pos, nrm = ref["pos4"], ref["nrm4"]
    want, pick = sc.oracle_mask(name, H8, S4, ac.TAU, ac.B10, "avx", ac.EVERY[name])
    with flake(name) as s:
        base = s.trace_ao(H8, pos=pos, nrm=nrm, spin=S4, **KW)
        o0 = s.stats().overflow_tiles
        got = s.trace_ao(H8, pos=pos, nrm=nrm, max_depth=4, spin=S4, **KW)
        moved = s.stats().overflow_tiles - o0
    print(name, "flagged tiles", moved)
    assert_mask(got, base, f"{name} max_depth = 4")
    assert_mask(got, want, f"{name} max_depth = 4 against the oracle", ac.compared(pos, pick))
    assert 1 <= moved <= tiles


# 8 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t1", "t3"])
def test_the_sum_equals_the_model_over_the_spun_mask(name):
    ref = frame(name)
    pos, nrm = ref["pos4"], ref["nrm4"]
    h = lights.ao_samples(64)
    with flake(name) as s:
        for n in (8, 33, 64):
            col = colours(n)
            mask = s.trace_ao(h[:n], pos=pos, nrm=nrm, spin=S4, **KW)
            got = s.trace_ao_sum(h[:n], col, pos=pos, nrm=nrm, spin=S4, **KW)
            assert_same(got, lights.ao_sum_model(None, pos, mask, col), f"{name} n = {n}")
            assert (got[~surface_of(pos)] == 0).all() and (got[..., 3] == 0).all()
        assert len(np.unique(got[surface_of(pos)][:, 0])) > 100   # visibility shows


@pytest.mark.parametrize("depth", [0, 4])
def test_a_call_equals_its_split(depth):
    """One call of 8 equals an overwriting call of k and an accumulating call of 8 - k, for k = 1 and 5 -- also at
    max_depth = 4, where a flagged tile must not add its chunk twice, also onto a non-zero base that carries .w."""
    ref = frame("t3")
    pos, nrm = ref["pos4"], ref["nrm4"]
    col = colours(8)
    kw = dict(pos=pos, nrm=nrm, max_depth=depth, spin=S4, **KW)
    with flake("t3") as s:
        whole = s.trace_ao_sum(H8, col, pos=pos, nrm=nrm, spin=S4, **KW)
        o0 = s.stats().overflow_tiles
        assert_same(s.trace_ao_sum(H8, col, **kw), whole, f"one call at max_depth = {depth}")
        for k in (1, 5):
            first = s.trace_ao_sum(H8[:k], col[:k], **kw)
            both = s.trace_ao_sum(H8[k:], col[k:], accumulate=True, out=first, **kw)
            assert_same(both, whole, f"split at {k}, max_depth = {depth}")
        moved = s.stats().overflow_tiles - o0
        base = base_image(pos.shape[:2])
        acc = s.trace_ao_sum(H8, col, accumulate=True, out=base, **kw)
        mask = s.trace_ao(H8, pos=pos, nrm=nrm, spin=S4, **KW)
    print("flagged tiles over five launches", moved)
    if depth:
        assert moved >= 5
    want = lights.ao_sum_model(base, pos, mask, col, True)
    assert_same(acc, want, f"accumulating, max_depth = {depth}")
    assert (acc[..., 3] == F(BASE[3])).all() and same_bits(acc[~surface_of(pos)], base[~surface_of(pos)])


# 9 ---------------------------------------------------------------------------------------------------
def test_callers_stream_between_renders_and_the_shared_buffers():
    """Render, the spun traces on a caller's torch stream (the caller's tensors, the context's own buffers), Render -- no
    host synchronisation in between. The statistics are what two renders alone leave, the later render's bits are the
    oracle frame's, and the context forms write the mask buffer trace_suns writes and the light buffer."""
    import torch
    S = pyoracle.load_setup("t3")
    W, H = S["W"], S["H"]
    ref = frame("t3")
    col = CONE_COLOURS
    want, pick = sc.oracle_mask("t3", H8, S4, ac.TAU, ac.B10, "avx", ac.EVERY["t3"])
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
    with flake("t3") as s:
        s.Render(emit_aux=True)
        assert s.shadow_mask_buffer() == 0 and s.light_buffer() == 0
        s.trace_ao(H8, pos=pt, nrm=nt, out=out, stream=ts.cuda_stream, spin=S4, **KW)
        s.trace_ao_sum(H8, col, pos=pt, nrm=nt, out=fout, stream=ts.cuda_stream, spin=S4, **KW)
        assert s.trace_ao(H8, stream=ts.cuda_stream, spin=S4) is None   # the context's frame, its buffer, the defaults
        assert s.trace_ao_sum(H8, col, stream=ts.cuda_stream, spin=S4) is None
        s.Render(emit_aux=True)
        pos, nrm, mint, idx = s.download(aux=True)   # (synchronises the context, whatever stream its work ran on)
        st = s.stats()
        assert (st.max_depth, np.float32(st.closest), st.rays, st.overflow_tiles) == alone
        for k, a in (("pos4", pos), ("nrm4", nrm), ("minT", mint), ("index", idx)):
            assert same_bits(a, ref[k]), f"Render after the spun traces: {k} differs"
        theirs = out.cpu().numpy().view(np.uint64)
        assert_mask(theirs, want, "caller's tensors", where)
        assert s.shadow_mask_buffer() != 0 and s.light_buffer() != 0
        assert_mask(s.download_shadow_masks(), theirs, "the context's mask buffer")
        summed = lights.ao_sum_model(None, ref["pos4"], theirs, col)
        assert_same(fout.cpu().numpy(), summed, "caller's light buffer")
        assert_same(s.download_light(), summed, "the context's light buffer")
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
    big = np.zeros((9, 9, 2), np.float32)
    big[..., 0] = 1.0
    with sf.Sphereflake(64, 36) as s:
        NULL = object()   # (a null spin pointer; None: the good 4 x 4 table)
        spin = lambda t: T() if t is None else None if t is NULL else t
        mask_to = lambda p, t=None, a=pp, b=pp, c=op: Lb.sf_trace_ao_spin_to(s.ctx, p, spin(t), a, b, c)
        sum_to = lambda p, t=None, a=pp, b=pp, c=fp_: Lb.sf_trace_ao_spin_sum_to(s.ctx, p, spin(t), a, b, c)
        own_mask = lambda p, t=None: Lb.sf_trace_ao_spin(s.ctx, p, spin(t))
        own_sum = lambda p, t=None: Lb.sf_trace_ao_spin_sum(s.ctx, p, spin(t))
        assert mask_to(P(64, 36)) == sf.SF_ENOVIEW and sum_to(P(64, 36)) == sf.SF_ENOVIEW
        assert own_mask(P()) == sf.SF_ENOVIEW and own_sum(P()) == sf.SF_ENOVIEW
        S = pyoracle.load_setup("t1")
        s.SetView(S["origin"], S["tl"], S["tr"], S["bl"])
        for call, own in ((mask_to, own_mask), (sum_to, own_sum)):
            # everything the unspun call rejects
            assert call(P(64, 36, n=0)) == sf.SF_EINVAL and own(P(n=0)) == sf.SF_EINVAL
            assert call(P(64, 36, n=65, samples=many)) == sf.SF_EINVAL and own(P(n=65, samples=many)) == sf.SF_EINVAL
            assert call(P(64, 36, samples=None)) == sf.SF_EINVAL and own(P(samples=None)) == sf.SF_EINVAL
            for bias in (-0.25, 1.0, 2.0, float("nan")):
                assert call(P(64, 36, bias=bias)) == sf.SF_EINVAL
            for distance in (0.0, -4.0, float("inf"), float("nan")):
                assert call(P(64, 36, distance=distance)) == sf.SF_EINVAL and own(P(distance=distance)) == sf.SF_EINVAL
            assert call(P(64, 36, max_depth=32)) == sf.SF_EINVAL
            assert call(P(64, 0)) == sf.SF_EINVAL
            assert call(P(32, 16), None, None) == sf.SF_EINVAL        # sizes against a NULL pos4
            assert call(P(32, 16), None, pp, None) == sf.SF_EINVAL    # ... a NULL nrm4
            assert call(None) == sf.SF_EINVAL and own(None) == sf.SF_EINVAL
            assert own(P(32, 16)) == sf.SF_EINVAL
            # the spin's own
            assert call(P(64, 36), NULL) == sf.SF_EINVAL and own(P(), NULL) == sf.SF_EINVAL
            assert call(P(64, 36), T(null=True)) == sf.SF_EINVAL and own(P(), T(null=True)) == sf.SF_EINVAL
            assert call(P(64, 36), T(size=0)) == sf.SF_EINVAL and own(P(), T(size=0)) == sf.SF_EINVAL
            assert call(P(64, 36), T(size=9, table=big)) == sf.SF_EINVAL and own(P(), T(size=9, table=big)) == sf.SF_EINVAL
            for bad in (float("nan"), float("inf"), -float("inf")):
                t = np.array(S4, np.float32, copy=True)
                t[3, 2, 1] = bad
                assert call(P(64, 36), T(table=t)) == sf.SF_EINVAL and own(P(), T(table=t)) == sf.SF_EINVAL
        assert mask_to(P(64, 36), None, pp, pp, None) == sf.SF_EINVAL          # a null mask
        assert sum_to(P(32, 16), None, pp, pp, None) == sf.SF_EINVAL           # sizes against a NULL out
        for bad in (-0.5, float("nan"), float("inf")):
            cols = [(0.5, 0.5, 0.5), (0.5, bad, 0.5), (0.5, 0.5, 0.5)]
            assert sum_to(P(64, 36, cols=cols)) == sf.SF_EINVAL and own_sum(P(cols=cols)) == sf.SF_EINVAL
        # an accumulating call before the light buffer exists
        assert sum_to(P(64, 36), None, pp, pp, None) == sf.SF_ESTATE
        assert sum_to(P(64, 36, accumulate=1), None, pp, pp, None) == sf.SF_ESTATE
        assert own_sum(P(accumulate=1)) == sf.SF_ESTATE
        assert s.light_buffer() == 0 and s.shadow_mask_buffer() == 0   # (a refused call made no buffer)
        s.Synchronize()
        assert (out == 9).all() and (fout == 9).all()   # none of them wrote
        # an all-miss position image: every mask has exactly its low n bits set, an accumulating sum leaves every pixel,
        # an overwriting one zeroes; a table value beyond the size's entries is not read
        t = np.full((8, 8, 2), np.nan, np.float32)
        t.reshape(-1, 2)[:4] = np.array([(1, 0), (0, 1), (-1, 0), (0, -1)], np.float32)
        assert mask_to(P(64, 36), T(size=2, table=t)) == sf.SF_OK
        assert sum_to(P(64, 36, accumulate=1)) == sf.SF_OK
        s.Synchronize()
        assert (out == 7).all() and (fout == 9).all()
        assert sum_to(P(64, 36)) == sf.SF_OK
        s.Synchronize()
        assert (fout == 0).all() and s.stats().rays == 0
        dev = (pos.data_ptr(), 64, 36)
        for bad in (np.zeros((9, 9, 2), np.float32), np.zeros((4, 4, 3), np.float32), np.zeros((3, 4, 2), np.float32)):
            with pytest.raises(ValueError):
                s.trace_ao(three, pos=dev, nrm=dev, out=out, spin=bad)
        with pytest.raises(ValueError):
            s.trace_ao(three, pos=dev, out=out, spin=S4)   # a device pos without a device nrm
