"""Sky reflections without a GPU: the host models operation by operation, lobe_samples and sky_gradient, the oracle
conditions tests/test_gpu_mirror.py relies on (measured on the CPU oracle at every surface pixel of t1 and t3), the
header, the exports, the struct layout, the error codes with a null context and the inline C++ members. Everything
that is a bit pattern is compared bit for bit."""
import ctypes
import pathlib
import shutil

import numpy as np
import pytest

import sphereflake_amd as sf
from sphereflake_amd import lights
from abicheck import compile_class_user, defined_symbols, undefined_symbols
from dirscheck import same_bits
from oracle import pyoracle
from rayscheck import frame
import aocheck as ac
import aospincheck as sc
import mirrorcheck as mc

F = np.float32
SYMBOLS = ("sf_mirror_defaults", "sf_trace_mirror_to", "sf_trace_mirror", "sf_trace_mirror_sum_to",
           "sf_trace_mirror_sum")
PIXELS = {"t1": ((18, 32), (10, 30), (25, 40), (17, 20)), "t3": ((22, 40), (10, 41), (30, 30), (20, 60), (40, 45))}


@pytest.fixture(scope="module", autouse=True)
def built():
    sf.build()


def dot3(a, b):
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


def axis_at(P, N, o, eye):
    """Steps 2 and 3 of the definition at one pixel, one numpy float32 scalar operation at a time."""
    P, N = [F(x) for x in P[:3]], [F(x) for x in N[:3]]
    V = P if eye is None else [F(F(F(o[k]) + P[k]) - F(eye[k])) for k in range(3)]
    nv = dot3(N, V)
    k = F(nv + nv)
    R = [F(V[c] - F(k * N[c])) for c in range(3)]
    ln = np.sqrt(dot3(R, R))
    assert ln.dtype == F
    return np.array([F(R[c] / ln) for c in range(3)], F), nv


# ---- the models ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t1", "t3"])
def test_mirror_axes_operation_by_operation(name):
    S = pyoracle.load_setup(name)
    f = frame(name)
    o = np.asarray(S["origin"], F).reshape(3)
    for eye in (None, o, mc.eye_of(name)):
        A = lights.mirror_axes(f["pos4"], f["nrm4"], o, eye)
        assert A.shape == f["pos4"].shape and A.dtype == F and (A[..., 3] == 0).all()
        seen = 0
        for y, x in PIXELS[name]:
            if not sc.surface_of(f["pos4"])[y, x]:
                continue
            want, _ = axis_at(f["pos4"][y, x], f["nrm4"][y, x], o, eye)
            assert same_bits(A[y, x, :3], want), (name, y, x)
            seen += 1
        assert seen >= 3
    with pytest.raises(ValueError):
        lights.mirror_axes(f["pos4"], f["nrm4"], None, o)        # an eye needs the origin
    with pytest.raises(ValueError):
        lights.mirror_axes(f["pos4"], f["nrm4"][:-1])


def test_view_vector_is_the_position_not_the_eye_form():
    """use_eye == 0 takes V = P; eye == origin is other bits: 3022 of t3's 3600 axes change (35 of t1's 830)."""
    for name, changed in (("t3", 3022), ("t1", 35)):
        S = pyoracle.load_setup(name)
        f = frame(name)
        surf = sc.surface_of(f["pos4"])
        plain = lights.mirror_axes(f["pos4"], f["nrm4"])
        same_eye = lights.mirror_axes(f["pos4"], f["nrm4"], S["origin"], S["origin"])
        assert same_bits(plain, lights.mirror_axes(f["pos4"], f["nrm4"], S["origin"], None))   # (the origin is not read)
        n = int((plain[surf][:, :3] != same_eye[surf][:, :3]).any(-1).sum())
        print(name, "axes changed by eye == origin:", n)
        assert n == changed
        assert np.abs(plain[surf] - same_eye[surf]).max() < 1e-6


@pytest.mark.parametrize("spin", [None, mc.S4])
def test_mirror_model_is_ao_model_on_the_axes(spin):
    S = pyoracle.load_setup("t3")
    f = frame("t3")
    eye = mc.eye_of("t3")
    A = lights.mirror_axes(f["pos4"], f["nrm4"], S["origin"], eye)
    got = lights.mirror_model(f["pos4"], f["nrm4"], S["origin"], mc.LOBE8, 4.0, ac.B10, spin=spin, eye=eye)
    want = lights.ao_model(f["pos4"], A, S["origin"], mc.LOBE8, 4.0, ac.B10, spin=spin)
    surf = want[3]
    assert np.array_equal(got[3], surf) and int(surf.sum()) == 3600
    for a, b, what in zip(got[:3], want[:3], ("F", "d", "bound")):
        assert same_bits(a[:, surf], b[:, surf]), what
    # one pixel by hand: s, f, F, d, bound
    y, x = PIXELS["t3"][0]
    T, B, N = lights.ao_basis(A, spin=spin)
    h = mc.LOBE8[5]
    o = np.asarray(S["origin"], F)
    w = o + f["pos4"][y, x, :3]
    s = np.array([F(F(F(T[y, x, c] * h[0]) + F(B[y, x, c] * h[1])) + F(A[y, x, c] * h[2])) for c in range(3)], F)
    Fo = w + s * F(4.0)
    d = (w - Fo) + F(0.0)
    assert same_bits(got[0][5, y, x], Fo) and same_bits(got[1][5, y, x], d)
    assert got[2][5, y, x] == F(np.sqrt(dot3(d, d)) * F(F(1.0) - F(ac.B10)))


@pytest.mark.parametrize("spin", [None, mc.S4, (0.6, 0.8)])
def test_the_mirror_ray_is_the_axis_itself(spin):
    """h = (0, 0, 1) gives s = A exactly; the spin does not matter for it."""
    f = frame("t3")
    A = lights.mirror_axes(f["pos4"], f["nrm4"])
    surf = sc.surface_of(f["pos4"])
    s = lights.ao_directions(A, mc.MIRROR, spin)
    assert same_bits(s[0][surf], A[surf][:, :3])


def test_lobe_samples():
    for n, e in ((1, 8), (8, 8), (64, 64), (5, 0), (16, 1)):
        h = lights.lobe_samples(n, e)
        assert h.shape == (n, 3) and h.dtype == F
        assert np.abs((h.astype(np.float64) ** 2).sum(-1) - 1).max() < 1e-6 and (h[:, 2] > 0).all()
        for i in {0, n // 2, n - 1}:
            u, th = (i + 0.5) / n, i * np.pi * (3.0 - np.sqrt(5.0))
            z = (1.0 - u) ** (1.0 / (e + 1.0))
            r = np.sqrt(1.0 - z * z)
            assert same_bits(h[i], np.array([r * np.cos(th), r * np.sin(th), z], np.float64).astype(F))
    # exponent 1 is ao_samples' cosine distribution (the radius is formed another way: to rounding)
    for n in (4, 8, 64):
        assert np.abs(lights.lobe_samples(n, 1).astype(np.float64) - lights.ao_samples(n).astype(np.float64)).max() < 2e-7
    # a larger exponent is a narrower lobe
    assert lights.lobe_samples(8, 64)[:, 2].min() > lights.lobe_samples(8, 8)[:, 2].min() > lights.ao_samples(8)[:, 2].min()
    for bad in ((0, 8), (65, 8), (8, -1.0), (8, float("nan")), (8, float("inf"))):
        with pytest.raises(ValueError):
            lights.lobe_samples(*bad)


def test_sky_gradient():
    s = lights.ao_directions(lights.mirror_axes(frame("t3")["pos4"], frame("t3")["nrm4"]), mc.LOBE8, mc.S4)
    ones = lights.sky_gradient(s, (1, 1, 1), (1, 1, 1), mc.UP)
    assert ones.dtype == F and (ones[:, sc.surface_of(frame("t3")["pos4"])] == 1).all()   # exactly 1
    E = lights.sky_gradient(s, mc.ZENITH, mc.HORIZON, mc.UP)
    z, h = np.array(mc.ZENITH, F), np.array(mc.HORIZON, F)
    for i, y, x in ((0, 22, 40), (7, 10, 41), (3, 30, 30)):
        v = s[i, y, x]
        u = dot3(v, np.array(mc.UP, F))
        t = F(min(max(u, F(0)), F(1)))
        assert same_bits(E[i, y, x], np.array([F(h[c] + F(F(z[c] - h[c]) * t)) for c in range(3)], F))
    # the clamp's ends, -0 and NaN; `up` is not normalised
    d = np.array([(0, 0, 1), (0, 0, -1), (1, 0, 0), (0, 0, -0.0), (np.nan, 0, 0), (0, 0, 0.25)], F)
    E = lights.sky_gradient(d, mc.ZENITH, mc.HORIZON, (0, 0, 2))
    assert same_bits(E[0], h + (z - h) * F(1)) and same_bits(E[1], h) and same_bits(E[2], h)
    assert same_bits(E[3], h) and same_bits(E[4], h)
    assert same_bits(E[5], h + (z - h) * F(0.5))
    assert same_bits(lights.sky_gradient(d[3], (1, 1, 1), (0, 0, 0), (0, 0, 1)), np.zeros(3, F))   # +0, not -0
    for bad in (dict(zenith=(1, -1, 1)), dict(horizon=(np.nan, 0, 0)), dict(up=(0, np.inf, 1))):
        with pytest.raises(ValueError):
            lights.sky_gradient(d, **bad)


def test_mirror_sum_model():
    """The sum at a few pixels by hand; with a white sky it is ao_sum_model on the same mask; the split at k."""
    S = pyoracle.load_setup("t3")
    f = frame("t3")
    pos, nrm = f["pos4"], f["nrm4"]
    mask, _ = mc.oracle_mask("t3", mc.LOBE8, mc.S4)
    col = np.linspace(0.05, 0.3, 24, dtype=F).reshape(8, 3)
    kw = dict(zenith=mc.ZENITH, horizon=mc.HORIZON, up=mc.UP, spin=mc.S4)
    got = lights.mirror_sum_model(None, pos, nrm, S["origin"], mask, mc.LOBE8, col, **kw)
    s = lights.ao_directions(lights.mirror_axes(pos, nrm), mc.LOBE8, mc.S4)
    for y, x in PIXELS["t3"]:
        acc = np.zeros(3, F)
        for i in range(8):
            E = lights.sky_gradient(s[i, y, x], mc.ZENITH, mc.HORIZON, mc.UP)
            k = E if (int(mask[y, x]) >> i) & 1 else np.zeros(3, F)
            acc = acc + col[i] * k
        assert same_bits(got[y, x, :3], acc) and got[y, x, 3] == 0
    assert (got[~sc.surface_of(pos)] == 0).all()
    white = lights.mirror_sum_model(None, pos, nrm, S["origin"], mask, mc.LOBE8, col, spin=mc.S4)
    assert same_bits(white, lights.ao_sum_model(None, pos, mask, col))
    base = np.full(pos.shape, F(0.125), F)
    base[..., 3] = F(7.0)
    for k in (1, 3, 7):
        first = lights.mirror_sum_model(None, pos, nrm, S["origin"], mask, mc.LOBE8[:k], col[:k], **kw)
        both = lights.mirror_sum_model(first, pos, nrm, S["origin"], mask >> np.uint64(k), mc.LOBE8[k:], col[k:],
                                       accumulate=True, **kw)
        assert same_bits(both, got), k
    acc = lights.mirror_sum_model(base, pos, nrm, S["origin"], mask, mc.LOBE8, col, accumulate=True, **kw)
    assert (acc[..., 3] == 7).all() and same_bits(acc[~sc.surface_of(pos)], base[~sc.surface_of(pos)])
    with pytest.raises(ValueError):
        lights.mirror_sum_model(None, pos, nrm, S["origin"], mask, mc.LOBE8, col, accumulate=True, **kw)
    with pytest.raises(ValueError):
        lights.mirror_sum_model(None, pos, nrm, S["origin"], mask, mc.LOBE8, col[:7], **kw)


# ---- the oracle conditions of the GPU tests -------------------------------------------------------------
@pytest.mark.parametrize("name", ["t1", "t3"])
def test_oracle_facts(name):
    """avx, tau = 4, bias 2^-10, every surface pixel (830 on t1, 3600 on t3)."""
    S = pyoracle.load_setup(name)
    f = frame(name)
    pos, nrm = f["pos4"], f["nrm4"]
    surf = sc.surface_of(pos)
    ns = int(surf.sum())
    assert ns == {"t1": 830, "t3": 3600}[name]
    # the axis: finite, unit to rounding, and the viewer is in front of every surface pixel
    A = mc.axes(name)[..., :3]
    P, N = pos[..., :3], nrm[..., :3]
    nv = (N[..., 0] * P[..., 0] + N[..., 1] * P[..., 1]) + N[..., 2] * P[..., 2]
    off = float(np.abs(np.linalg.norm(A[surf].astype(np.float64), axis=-1) - 1).max())
    print(name, "||A| - 1| <=", off)
    assert np.isfinite(A[surf]).all() and off <= 1.4e-7 and (nv[surf] < 0).all()
    # lobe_samples(8, 8) under ao_spins(4): both outcomes per bit, and not AO about N
    m8, deepest = mc.oracle_mask(name, mc.LOBE8, mc.S4)
    opened = [int((surf & ac.bit(m8, i)).sum()) for i in range(8)]
    closed = [int((surf & ~ac.bit(m8, i)).sum()) for i in range(8)]
    print(name, "open", min(opened), "closed", min(closed), "deepest", deepest)
    assert min(opened) >= 200 and min(closed) >= 200
    assert (min(opened), min(closed)) == {"t1": (309, 474), "t3": (1386, 2002)}[name]
    about_n, pick = sc.oracle_mask(name, mc.LOBE8, mc.S4, ac.TAU, ac.B10, "avx", 1)
    differ = int((surf & (about_n != m8)).sum())
    print(name, "words that differ from trace_ao_spin about N:", differ)
    assert np.array_equal(pick, surf) and 2 * differ > ns and differ == {"t1": 726, "t3": 3075}[name]
    # the mirror ray alone
    m1, _ = mc.oracle_mask(name, mc.MIRROR)
    assert int((surf & ac.bit(m1, 0)).sum()) == {"t1": 356, "t3": 1609}[name]
    # the rays go deep enough for max_depth = 4 to flag tiles
    assert deepest == 8 and mc.oracle_mask(name, mc.LOBE8, mc.S4, variant="sse")[1] == 7
    # every origin is outside the radius-2 ball
    for h, spin in ((mc.LOBE64, None), (mc.LOBE8, mc.S4)):
        Fo = lights.mirror_model(pos, nrm, S["origin"], h, 4.0, ac.B10, spin=spin)[0]
        near = float(np.linalg.norm(Fo[:, surf].astype(np.float64), axis=-1).min())
        assert 2.12 < near < 2.2, near
    assert (mc.oracle_mask(name, mc.LOBE64)[0][~surf] == np.uint64(2 ** 64 - 1)).all()


def test_oracle_facts_of_the_eye_and_of_convergence():
    S = pyoracle.load_setup("t3")
    f = frame("t3")
    pos, nrm = f["pos4"], f["nrm4"]
    surf = sc.surface_of(pos)
    m8, _ = mc.oracle_mask("t3", mc.LOBE8, mc.S4)
    moved, _ = mc.oracle_mask("t3", mc.LOBE8, mc.S4, mc.eye_of("t3"))
    assert int((surf & (moved != m8)).sum()) == 3020
    col = lambda n: np.full((n, 3), F(1.0) / F(n), F)
    sky = dict(zenith=mc.ZENITH, horizon=mc.HORIZON, up=mc.UP)
    m64, _ = mc.oracle_mask("t3", mc.LOBE64)
    ref = lights.mirror_sum_model(None, pos, nrm, S["origin"], m64, mc.LOBE64, col(64), **sky)
    err = []
    for n in (16, 8, 4):
        h = lights.lobe_samples(n, 8)
        m, _ = mc.oracle_mask("t3", h)
        err.append(mc.red_rms(lights.mirror_sum_model(None, pos, nrm, S["origin"], m, h, col(n), **sky), ref, surf))
    print("RMS against n = 64 at n = 16, 8, 4:", err)
    assert err[0] < err[1] < err[2]
    assert [round(e, 3) for e in err] == [0.047, 0.071, 0.109]


# ---- the header, the library, the class -----------------------------------------------------------------
def test_header_states_the_definition():
    text = " ".join(pathlib.Path(sf.HEADER_PATH).read_text().split())
    for sym in SYMBOLS + ("sf_mirror_params",):
        assert sym in text, sym
    for sentence in (
            "with use_eye == 0, V = P",
            "V = (o + P) - eye per component",
            "THESE ARE DIFFERENT BITS",
            "it changes 3022 of 3600 axes in their last bits",
            "nv = ((N.x V.x) + (N.y V.y)) + (N.z V.z); k = nv + nv; R.c = V.c - (k N.c);",
            "len = sqrtf(rr), correctly rounded; A.c = R.c / len, a correctly rounded division.",
            "u_i = ((s_i.x up.x) + (s_i.y up.y)) + (s_i.z up.z)",
            "t_i = min(max(u_i, 0), 1), and +0 where u_i is -0 or NaN",
            "E_i.c = horizon.c + ((zenith.c - horizon.c) t_i)",
            "S.c = S.c + (colours[i].c (open_i ? E_i.c : 0.0f))",
            "`up` is used as given, not normalised.",
            "The mask equals sf_trace_ao_spin_to's mask (sf_trace_ao_to's without a spin) on a normal image that holds A",
            "E is exactly 1, and a closed entry adds colours 0, as there.",
            "h = (0, 0, 1) gives s = A exactly, with or without a spin.",
            "A call equals its split into an overwriting call with the first k entries and an accumulating call",
            "A flagged tile stores nothing in its first pass.",
            "top-left corner is at multiples of the spin's `size`",
            "tau >= 4 keeps every ray's origin outside the flake's radius-2 ball",
            "the flake does not reflect itself, there is no Fresnel term",
            "spin NULL means unspun"):
        assert sentence in text, sentence
    assert "#define SF_ABI_VERSION 1" in text and sf.lib().sf_abi_version() == 1


def test_symbols_are_exported():
    if shutil.which("nm") is None:
        pytest.skip("binutils not available")
    have = defined_symbols(sf.LIB_PATH)
    assert set(SYMBOLS) <= have
    assert set(SYMBOLS) <= set(sf.SIGNATURES)
    for k in ("wave", "fixup", "sum_wave", "sum_fixup"):
        assert "sf_trace_mirror_" + k in have


def test_struct_layout_matches_the_header():
    P, A = sf.sf_mirror_params, sf.sf_ao_params
    for name, _ in A._fields_:   # sf_ao_params' fields first, where they are there
        assert getattr(P, name).offset == getattr(A, name).offset, name
    assert (P.stream.offset, P.eye.offset, P.use_eye.offset, P.zenith.offset, P.horizon.offset, P.up.offset) == \
        (64, 72, 84, 88, 100, 112)
    assert ctypes.sizeof(P) == 128


def test_defaults_and_error_codes_without_a_device():
    L = sf.lib()
    p = sf.sf_mirror_params()
    assert L.sf_mirror_defaults(None, ctypes.byref(p)) == sf.SF_EINVAL
    buf = (ctypes.c_float * 64)()
    vp = ctypes.cast(buf, ctypes.c_void_p)
    p.samples, p.n, p.distance = ctypes.cast(buf, ctypes.POINTER(ctypes.c_float)), 1, 4.0
    sp = sf.sf_ao_spin()
    sp.cs, sp.size = ctypes.cast(buf, ctypes.POINTER(ctypes.c_float)), 1
    for spin in (ctypes.byref(sp), None):
        assert L.sf_trace_mirror_to(None, ctypes.byref(p), spin, vp, vp, vp) == sf.SF_EINVAL
        assert L.sf_trace_mirror(None, ctypes.byref(p), spin) == sf.SF_EINVAL
        assert L.sf_trace_mirror_sum_to(None, ctypes.byref(p), spin, vp, vp, vp) == sf.SF_EINVAL
        assert L.sf_trace_mirror_sum(None, ctypes.byref(p), spin) == sf.SF_EINVAL


def test_cpp_members_are_inline_over_the_c_abi(tmp_path):
    """TraceMirror / TraceMirrorSum compile for an application in both forms, stay inline, and need only sf_* symbols
    the library has."""
    if shutil.which("g++") is None or shutil.which("nm") is None:
        pytest.skip("binutils / g++ not available")
    source = ('#include "Sphereflake.hpp"\n'
              "using namespace SphereflakeRaytracer;\n"
              "void reflect(Sphereflake& s, const float* pdev, const float* ndev, uint64_t* mdev, float* ldev) {\n"
              "    static const float h[6] = { 0.0f, 0.0f, 1.0f, 0.6f, 0.0f, 0.8f };\n"
              "    static const float cs[8] = { 1.0f, 0.0f, 0.0f, 1.0f, -1.0f, 0.0f, 0.0f, -1.0f };\n"
              "    sf_mirror_params p;\n"
              "    sf_mirror_defaults(s.Context(), &p);\n"
              "    p.samples = h; p.n = 2;\n"
              "    p.zenith[0] = 0.25f; p.eye[2] = 3.0f; p.use_eye = 1;\n"
              "    sf_ao_spin spin = { cs, 2 };\n"
              "    s.TraceMirror(p);\n"
              "    s.TraceMirror(p, &spin);\n"
              "    s.TraceMirrorSum(p);\n"
              "    p.accumulate = 1;\n"
              "    s.TraceMirrorSum(p, &spin);\n"
              "    p.width = 64; p.height = 36;\n"
              "    s.TraceMirror(p, &spin, pdev, ndev, mdev);\n"
              "    s.TraceMirrorSum(p, nullptr, pdev, ndev, ldev);\n}\n")
    obj = compile_class_user(tmp_path, "mirror", source)
    need, have = undefined_symbols(obj), defined_symbols(sf.LIB_PATH)
    assert set(SYMBOLS) <= need
    assert not [n for n in need if "TraceMirror" in n]
    assert not [n for n in need if (n.startswith("sf_") or "SphereflakeRaytracer" in n) and n not in have]
