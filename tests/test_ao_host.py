"""Host side of the ambient-occlusion traces (sf_trace_ao_to, sf_trace_ao_sum_to): the sample generators and the host
statement of the definition (sphereflake_amd.lights) against suns_model and a scalar restatement, the oracle facts the
GPU tests stand on, the header and the library's exports, and the error codes that need no device. No GPU needed."""
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

F = np.float32
SYMBOLS = ("sf_ao_defaults", "sf_trace_ao_to", "sf_trace_ao", "sf_trace_ao_sum_to", "sf_trace_ao_sum")


def unit_normals(name):
    f = frame(name)
    surf = f["minT"] < ac.FLT_MAX
    return f["nrm4"][surf][:, :3]


# ---- the samples and their colours ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cosine", "uniform"])
def test_ao_samples(kind):
    for n in (1, 8, 33, 64):
        h = lights.ao_samples(n, kind)
        assert h.dtype == F and h.shape == (n, 3)
        assert np.abs(np.linalg.norm(h.astype(np.float64), axis=1) - 1.0).max() < 1e-7   # unit, to float32 rounding
        assert (h[:, 2] > 0).all()
        assert same_bits(h, lights.ao_samples(n, kind))   # deterministic
        assert len(np.unique(h, axis=0)) == n
        u = (np.arange(n) + 0.5) / n
        assert np.abs(h[:, 2] - (np.sqrt(1.0 - u) if kind == "cosine" else u)).max() < 1e-7
        # the golden-angle spiral: sample i at angle i pi (3 - sqrt 5)
        th = np.arange(n) * np.pi * (3.0 - np.sqrt(5.0))
        r = np.hypot(h[:, 0].astype(np.float64), h[:, 1].astype(np.float64))
        assert np.abs(h[:, 0] - r * np.cos(th)).max() < 1e-6 and np.abs(h[:, 1] - r * np.sin(th)).max() < 1e-6
    z = lights.ao_samples(64, kind)[:, 2].astype(np.float64).mean()
    # the mean of cos(theta): 2/3 under the cosine density (the midpoint rule's error on sqrt(1 - u) at n = 64 is under
    # 0.002), 1/2 under the uniform one (exact for midpoints)
    assert abs(z - (2.0 / 3.0 if kind == "cosine" else 0.5)) < 2e-3
    assert same_bits(lights.ao_samples(8), lights.ao_samples(8, "cosine"))
    for n in (0, 65):
        with pytest.raises(ValueError):
            lights.ao_samples(n, kind)
    with pytest.raises(ValueError):
        lights.ao_samples(8, "stratified")


def test_ao_colours():
    sky = (0.25, 0.5, 1.0)
    hc, hu = lights.ao_samples(32), lights.ao_samples(32, "uniform")
    cc, cu = lights.ao_colours(hc, sky), lights.ao_colours(hu, sky, "uniform")
    assert cc.dtype == cu.dtype == F and cc.shape == cu.shape == (32, 3)
    assert same_bits(cc, np.tile((np.array(sky) / 32).astype(F), (32, 1)))
    assert np.abs(cu - (2.0 * hu[:, 2:3].astype(np.float64) / 32) * np.array(sky)).max() < 1e-8
    # an open hemisphere sums to one sky either way (the uniform set's mean h.z is 1/2)
    assert np.abs(cc.astype(np.float64).sum(axis=0) - sky).max() < 1e-6
    assert np.abs(cu.astype(np.float64).sum(axis=0) - sky).max() < 1e-6
    assert same_bits(lights.ao_colours(hc), np.full((32, 3), F(1.0 / 32), F))
    for bad in ((-0.1, 0, 0), (np.nan, 1, 1), (np.inf, 1, 1)):
        with pytest.raises(ValueError):
            lights.ao_colours(hc, bad)
    with pytest.raises(ValueError):
        lights.ao_colours(hc, sky, "other")
    with pytest.raises(ValueError):
        lights.ao_colours(np.zeros((65, 3), F), sky)


# ---- the frame ----------------------------------------------------------------------------------------
def scalar_basis(N):
    """sf.h's step 2 for one normal, one float32 operation at a time."""
    x, y, z = F(N[0]), F(N[1]), F(N[2])
    sg = np.copysign(F(1.0), z)
    a = F(-1.0) / (sg + z)
    b = (x * y) * a
    T = (F(1.0) + sg * ((x * x) * a), sg * b, -(sg * x))
    B = (b, sg + (y * y) * a, -y)
    return np.array(T, F), np.array(B, F)


def test_ao_basis_special_normals():
    """N = (0, 0, +-1), (0, 0, -0.0) and (1, 0, 0): no division by zero, no NaN, and the vectors sf.h's formulas give."""
    cases = {(0.0, 0.0, 1.0): ((1, 0, 0), (0, 1, 0)),
             (0.0, 0.0, -1.0): ((1, 0, 0), (0, -1, 0)),
             (0.0, 0.0, -0.0): ((1, 0, 0), (0, -1, 0)),     # sg = -1: a = -1 / (-1 + -0) = 1
             (1.0, 0.0, 0.0): ((0, 0, -1), (0, 1, 0))}      # sg = +1, a = -1: T = (1 - 1, 0, -1)
    for N, (Tw, Bw) in cases.items():
        T, B, Nn = lights.ao_basis(np.array(N, F))
        assert T.dtype == B.dtype == Nn.dtype == F and T.shape == B.shape == (3,)
        assert np.isfinite(T).all() and np.isfinite(B).all()
        assert np.array_equal(T, np.array(Tw, F)) and np.array_equal(B, np.array(Bw, F)), (N, T, B)
        assert same_bits(Nn, np.array(N, F))   # N as given, its zero's sign too
        Ts, Bs = scalar_basis(N)
        assert same_bits(T, Ts) and same_bits(B, Bs)
        # h = (0, 0, 1) gives s = N exactly; h = (1, 0, 0) gives T, (0, 1, 0) gives B (as values: 0 + -0 is +0)
        s = lights.ao_directions(np.array(N, F), [(0, 0, 1), (1, 0, 0), (0, 1, 0)])
        assert np.array_equal(s[0], np.array(N, F)) and np.array_equal(s[1], T) and np.array_equal(s[2], B)


def test_ao_basis_equals_the_scalar_statement_and_is_orthonormal():
    rng = np.random.default_rng(331)
    N = rng.normal(size=(6, 7, 4)).astype(F)
    N[..., :3] /= np.linalg.norm(N[..., :3].astype(np.float64), axis=-1, keepdims=True).astype(F)
    N[0, 0, :3] = (np.nan, 0.0, 1.0)
    N[0, 1, :3] = (3.0, -4.0, 12.0)   # not a unit vector: used as given
    T, B, Nn = lights.ao_basis(N)
    assert T.shape == B.shape == Nn.shape == (6, 7, 3)
    for y in range(6):
        for x in range(7):
            Ts, Bs = scalar_basis(N[y, x])
            assert same_bits(T[y, x], Ts) and same_bits(B[y, x], Bs), (y, x)
    assert np.isnan(T[0, 0]).any()
    # orthonormal to 1e-6 absolute on unit normals: the fixtures' own (measured: 3.3e-7 at worst)
    worst = 0.0
    for name in ("t1", "t3"):
        U = unit_normals(name)
        assert np.abs(np.linalg.norm(U.astype(np.float64), axis=1) - 1.0).max() < 1e-6
        T, B, Nn = (v.astype(np.float64) for v in lights.ao_basis(U))
        M = np.stack([T, B, Nn], axis=1)                      # [npx, 3, 3], rows T, B, N
        err = np.abs(M @ M.transpose(0, 2, 1) - np.eye(3)).max()
        worst = max(worst, err)
        assert (np.linalg.det(M) > 0.999).all()               # right-handed: T x B = N
    print("orthonormality error", worst)
    assert worst <= 1e-6


def test_ao_directions_scalar_and_shapes():
    rng = np.random.default_rng(337)
    N = rng.normal(size=(4, 5, 3)).astype(F)
    h = np.concatenate([lights.ao_samples(5), [[0, 0, 0], [np.nan, 0, 1], [np.inf, 0, 0]]]).astype(F)
    s = lights.ao_directions(N, h)
    assert s.dtype == F and s.shape == (8, 4, 5, 3)
    for i in range(8):
        for y in range(4):
            for x in range(5):
                T, B = scalar_basis(N[y, x])
                with np.errstate(invalid="ignore"):
                    want = np.array([((T[c] * h[i][0]) + (B[c] * h[i][1])) + (N[y, x][c] * h[i][2]) for c in range(3)], F)
                assert same_bits(s[i, y, x], want), (i, y, x)
    assert (s[5] == 0).all() and np.isnan(s[6]).any() and not np.isfinite(s[7]).all()
    assert lights.ao_directions(N[0, 0], h[:5]).shape == (5, 3)
    with pytest.raises(ValueError):
        lights.ao_directions(N, np.zeros((65, 3), F))


# ---- the model ----------------------------------------------------------------------------------------
def test_ao_model_with_a_constant_normal_is_suns_model():
    rng = np.random.default_rng(347)
    pos = rng.normal(scale=1.5, size=(5, 8, 4)).astype(F)
    pos[0, 3, :3] = 0.0
    pos[1, 2, :3] = (np.inf, 1.0, 1.0)
    o = np.array([1.25, -2.5, 0.75], F)
    h = np.concatenate([lights.ao_samples(6), [[0, 0, 0], [np.nan, 0, 1]]]).astype(F)
    for N0 in ac.CONSTANT_NORMALS + ((0.0, 0.0, -0.0), (3.0, -4.0, 12.0)):
        nrm = np.empty((5, 8, 4), F)
        nrm[...] = np.array(N0 + (0.0,), F)
        Fo, d, bound, surf = lights.ao_model(pos, nrm, o, h, 4.0, ac.B10)
        assert Fo.shape == d.shape == (8, 5, 8, 3) and bound.shape == (8, 5, 8) and surf.shape == (5, 8)
        D = lights.ao_directions(np.array(N0, F), h)
        F1, d1, b1, s1 = lights.suns_model(pos, o, D, 4.0, ac.B10)
        assert same_bits(Fo, F1) and same_bits(d, d1) and same_bits(bound, b1) and np.array_equal(surf, s1), N0
    assert not surf[0, 3] and surf.sum() == 39
    with pytest.raises(ValueError):
        lights.ao_model(pos, nrm, o, h, 0.0, 0.0)
    with pytest.raises(ValueError):
        lights.ao_model(pos, nrm, o, h, 4.0, 1.0)
    with pytest.raises(ValueError):
        lights.ao_model(pos, nrm[:4], o, h, 4.0, 0.0)


def test_ao_model_per_pixel():
    """A normal per pixel: slice (i, p) is sun_model of pixel p alone with the direction ao_directions gives there."""
    rng = np.random.default_rng(349)
    pos = rng.normal(size=(3, 4, 4)).astype(F)
    nrm = rng.normal(size=(3, 4, 4)).astype(F)
    o = np.array([0.5, 0.25, -3.0], F)
    h = lights.ao_samples(4, "uniform")
    Fo, d, bound, surf = lights.ao_model(pos, nrm, o, h, 4.5, 0.0)
    s = lights.ao_directions(nrm, h)
    for i in range(4):
        for y in range(3):
            for x in range(4):
                F1, d1, b1, _ = lights.sun_model(pos[y, x], o, s[i, y, x], 4.5, 0.0)
                assert same_bits(Fo[i, y, x], F1) and same_bits(d[i, y, x], d1) and same_bits(bound[i, y, x], b1)
    assert surf.all()


def test_ao_sum_model():
    rng = np.random.default_rng(353)
    npx = 40
    pos = rng.normal(size=(npx, 4)).astype(F)
    pos[7, :3] = 0.0
    mask = rng.integers(0, 2 ** 63, size=npx, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=npx).astype(np.uint64)
    col = (rng.uniform(0.5, 1.0, (64, 3)) * 2.0 ** rng.integers(-8, 1, (64, 1)) / 64).astype(F)
    base = rng.random((npx, 4)).astype(F)
    for accumulate in (False, True):
        out = lights.ao_sum_model(base, pos, mask, col, accumulate)
        assert out.dtype == F and out.shape == (npx, 4)
        for p in range(npx):
            if p == 7:
                want = base[p] if accumulate else np.zeros(4, F)
            else:
                S = base[p, :3].copy() if accumulate else np.zeros(3, F)
                for i in range(64):
                    k = F(1.0) if (int(mask[p]) >> i) & 1 else F(0.0)
                    S = S + col[i] * k
                want = np.concatenate([S, [base[p, 3] if accumulate else F(0.0)]]).astype(F)
            assert same_bits(out[p], want), (accumulate, p)
        # a call equals its split, and bits >= 32 are live
        for k in (1, 33):
            first = lights.ao_sum_model(base, pos, mask & np.uint64((1 << k) - 1), col[:k], accumulate)
            assert same_bits(lights.ao_sum_model(first, pos, mask >> np.uint64(k), col[k:], True), out)
        assert (lights.ao_sum_model(base, pos, mask & np.uint64(0xffffffff), col, accumulate) != out).any()
    # it is sum_model with a Lambert term of one: unit normals along the one direction
    up = np.tile(np.array([[0, 0, 1]], F), (64, 1))
    nz = np.tile(np.array([[0, 0, 1, 0]], F), (npx, 1))
    assert same_bits(lights.ao_sum_model(None, pos, mask, col), lights.sum_model(None, pos, nz, [mask], up, col))
    with pytest.raises(ValueError):
        lights.ao_sum_model(None, pos, mask, col, True)
    with pytest.raises(ValueError):
        lights.ao_sum_model(None, pos, mask, -col)
    with pytest.raises(ValueError):
        lights.ao_sum_model(None, pos, mask[:5], col)


# ---- the oracle facts the GPU tests stand on ------------------------------------------------------------
@pytest.mark.parametrize("name,traced", [("t1", 830), ("t3", 1200)])
def test_oracle_facts_of_the_eight_sample_cases(name, traced):
    """ao_samples(8), tau = 4, bias 2^-10: every sample has at least 100 traced pixels lit and 100 occluded, so a
    constant mask cannot pass. Measured: t1 at least 325 lit and 322 occluded per sample, t3 395 and 221; the rays
    reach depth 7."""
    h = lights.ao_samples(8)
    every = ac.EVERY[name]
    m, pick = ac.oracle_mask(name, h, every=every)
    c = ac.counts(m, 8, pick)
    deepest = ac.frame_rays(name, h, every=every)[2]
    print(name, int(pick.sum()), "lit / occluded", c, "mixed", int(ac.mixed(m, 8, pick).sum()), "deepest", deepest)
    assert int(pick.sum()) == traced
    assert min(x[0] for x in c) >= 100 and min(x[1] for x in c) >= 100
    assert (m >> np.uint64(8) == 0).all() and (m[~pick] == np.uint64(255)).all()
    assert deepest > 4   # max_depth = 4 provisions too few levels: the re-trace test has tiles to flag
    # every ray starts outside the radius-2 ball
    f = frame(name)
    Fo, _, _, _ = lights.ao_model(f["pos4"], f["nrm4"], pyoracle.load_setup(name)["origin"], h, ac.TAU, 0.0)
    assert np.linalg.norm(Fo[:, pick].astype(np.float64), axis=-1).min() >= 2.0


def test_oracle_facts_of_the_64_sample_case():
    """t1 under ao_samples(64), every 8th surface pixel (104): at least 8 samples of index >= 32 have at least 20 pixels
    of each outcome, so a 32-bit shift cannot pass. Measured: all 32 of them do; all 104 pixels are mixed."""
    h = lights.ao_samples(64)
    m, pick = ac.oracle_mask("t1", h, every=ac.SKY_EVERY)
    assert int(pick.sum()) == 104
    c = ac.counts(m, 64, pick)
    both = [i for i in range(32, 64) if c[i][0] >= 20 and c[i][1] >= 20]
    print("samples >= 32 with both outcomes", len(both), "mixed pixels", int(ac.mixed(m, 64, pick).sum()))
    assert len(both) >= 8


def test_oracle_facts_of_the_lod_case():
    """t3 at the matched constant (about 394.7), every 3rd surface pixel: the oracle's bits differ from the default
    constant's. Measured: 214 of 9600."""
    import suncheck as su
    h = lights.ao_samples(8)
    base, pick = ac.oracle_mask("t3", h, every=3)
    fine, pick2 = ac.oracle_mask("t3", h, lod=su.matched(), every=3)
    assert np.array_equal(pick, pick2)
    differ = sum(int((pick & (ac.bit(base, i) != ac.bit(fine, i))).sum()) for i in range(8))
    print("bits that differ", differ, "of", 8 * int(pick.sum()))
    assert differ >= 20


# ---- the header, the library, the class ---------------------------------------------------------------
def test_header_states_the_definition():
    text = " ".join(pathlib.Path(sf.HEADER_PATH).read_text().split())
    for sym in SYMBOLS + ("sf_ao_params",):
        assert sym in text, sym
    assert "#define SF_AO_SAMPLES_MAX 64" in text and sf.SF_AO_SAMPLES_MAX == 64 and lights.AO_SAMPLES_MAX == 64
    assert "sg = copysignf(1, N.z); a = -1 / (sg + N.z), a correctly rounded division; b = (N.x N.y) a;" in text
    assert "T = (1 + sg ((N.x N.x) a), sg b, -sg N.x); B = (b, sg + (N.y N.y) a, -N.y)." in text
    assert "s_i.c = ((T.c h_i.x) + (B.c h_i.y)) + (N.c h_i.z); per component, f_i.c = s_i.c tau." in text
    assert "h = (0, 0, 1) gives s = N exactly." in text
    assert "bit for bit, sf_trace_suns_to with dirs[i] = s_i(N0)" in text
    assert "S.c = S.c + colours[i].c (lit_i ? 1.0f : 0.0f) in index order" in text
    assert "#define SF_ABI_VERSION 1" in text and sf.lib().sf_abi_version() == 1


def test_symbols_are_exported():
    if shutil.which("nm") is None:
        pytest.skip("binutils not available")
    have = defined_symbols(sf.LIB_PATH)
    assert set(SYMBOLS) <= have
    assert set(SYMBOLS) <= set(sf.SIGNATURES)


def test_struct_layout_matches_the_header():
    P = sf.sf_ao_params
    assert ctypes.sizeof(P) == 72
    assert (P.samples.offset, P.colours.offset, P.n.offset, P.accumulate.offset, P.distance.offset) == (0, 8, 16, 20, 24)
    assert (P.bias.offset, P.origin.offset, P.use_origin.offset, P.width.offset, P.height.offset) == (28, 32, 44, 48, 52)
    assert (P.max_depth.offset, P.stream.offset) == (56, 64)


def test_error_codes_without_a_device():
    L = sf.lib()
    p = sf.sf_ao_params()
    buf = (ctypes.c_float * 64)()
    vp = ctypes.cast(buf, ctypes.c_void_p)
    p.samples, p.n, p.distance = ctypes.cast(buf, ctypes.POINTER(ctypes.c_float)), 1, 4.0
    assert L.sf_ao_defaults(None, ctypes.byref(p)) == sf.SF_EINVAL
    assert p.n == 1   # (a refused sf_ao_defaults wrote nothing)
    assert L.sf_trace_ao_to(None, ctypes.byref(p), vp, vp, vp) == sf.SF_EINVAL
    assert L.sf_trace_ao(None, ctypes.byref(p)) == sf.SF_EINVAL
    assert L.sf_trace_ao_sum_to(None, ctypes.byref(p), vp, vp, vp) == sf.SF_EINVAL
    assert L.sf_trace_ao_sum(None, ctypes.byref(p)) == sf.SF_EINVAL


def test_cpp_members_are_inline_over_the_c_abi(tmp_path):
    """Sphereflake::TraceAO / TraceAOSum compile for an application, stay inline, and need only sf_* symbols the
    library has."""
    if shutil.which("g++") is None or shutil.which("nm") is None:
        pytest.skip("binutils / g++ not available")
    source = ('#include "Sphereflake.hpp"\n'
              "using namespace SphereflakeRaytracer;\n"
              "void occlude(Sphereflake& s, const float* pdev, const float* ndev, uint64_t* mdev, float* ldev) {\n"
              "    static const float h[6] = { 0.0f, 0.0f, 1.0f, 0.6f, 0.0f, 0.8f };\n"
              "    sf_ao_params p;\n"
              "    sf_ao_defaults(s.Context(), &p);\n"
              "    p.samples = h; p.n = 2;\n"
              "    s.TraceAO(p);\n"
              "    s.TraceAOSum(p);\n"
              "    p.width = 64; p.height = 36; p.accumulate = 1;\n"
              "    s.TraceAO(p, pdev, ndev, mdev);\n"
              "    s.TraceAOSum(p, pdev, ndev, ldev);\n}\n")
    obj = compile_class_user(tmp_path, "ao", source)
    need, have = undefined_symbols(obj), defined_symbols(sf.LIB_PATH)
    assert {"sf_trace_ao_to", "sf_trace_ao", "sf_trace_ao_sum_to", "sf_trace_ao_sum"} <= need
    assert not [n for n in need if "TraceAO" in n]
    assert not [n for n in need if (n.startswith("sf_") or "SphereflakeRaytracer" in n) and n not in have]
