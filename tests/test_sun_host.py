"""Host side of the directional-light shadows and of the shadow traces' LOD constant (sf_trace_sun_to,
sf_light_image_sun, sf_set_shadow_lod): the host statement of the definition (sphereflake_amd.lights) against a scalar
restatement, the oracle facts the GPU tests stand on, the header and the library's exports, and the error codes that
need no device. No GPU needed."""
import ctypes
import math
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
import suncheck as su

F = np.float32
SYMBOLS = ("sf_set_shadow_lod", "sf_get_shadow_lod", "sf_sun_defaults", "sf_trace_sun_to", "sf_trace_sun",
           "sf_light_image_sun")


def scalar_sun(P, o, s, tau, b):
    """Steps 1-3 of sf.h's definition for one pixel, one float32 operation at a time."""
    P, o, s, tau = [F(v) for v in P], [F(v) for v in o], [F(v) for v in s], F(tau)
    surface = not (P[0] == 0 and P[1] == 0 and P[2] == 0)
    with np.errstate(all="ignore"):
        w = [o[k] + P[k] for k in range(3)]
        f = [s[k] * tau for k in range(3)]
        Fo = [w[k] + f[k] for k in range(3)]
        d = [(w[k] - Fo[k]) + F(0.0) for k in range(3)]
        length = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        bound = length * (F(1.0) - F(b))
    return np.array(Fo, F), np.array(d, F), F(bound), surface


def test_sun_model_equals_the_scalar_restatement():
    rng = np.random.default_rng(223)
    pos = rng.normal(scale=1.5, size=(40, 4)).astype(F)
    pos[3, :3] = 0.0                       # a miss of the frame
    pos[4, :3] = (-0.0, 0.0, -0.0)         # ... whatever the zeros' signs
    pos[5, :3] = (0.0, 0.0, 1e-30)         # no miss
    pos[8, :3] = (np.inf, 1.0, 1.0)
    pos[9, :3] = (np.nan, 1.0, 1.0)
    o = np.array([1.25, -2.5, 0.75], F)
    s = su.direction("side")
    for tau in (4.0, 8.0, 0.5):
        for b in (0.0, 2.0 ** -10, 0.5):
            Fo, d, bound, surf = lights.sun_model(pos, o, s, tau, b)
            assert Fo.dtype == d.dtype == bound.dtype == F
            assert Fo.shape == d.shape == (40, 3) and bound.shape == surf.shape == (40,)
            for i in range(40):
                sF, sd, sb, ss = scalar_sun(pos[i, :3], o, s, tau, b)
                assert same_bits(Fo[i], sF) and same_bits(d[i], sd) and same_bits(bound[i], sb), (i, tau, b)
                assert bool(surf[i]) == ss
            assert not np.signbit(d[d == 0]).any()
    Fo, d, bound, surf = lights.sun_model(pos, o, s, 4.0, 0.0)
    assert not surf[3] and not surf[4] and surf[5]
    # the rounding order matters: d is (w - (w + f)) + 0, not -f
    assert (d[10:] != -(s * F(4.0))).any()
    # a sun along an axis: the other components of w - F are w - w = +0, and stay +0
    Fz, dz, bz, _ = lights.sun_model(np.array([[0.5, -0.25, 1.0, 1.0]], F), np.zeros(3, F), (0.0, 0.0, 1.0), 4.0, 0.0)
    assert same_bits(dz[0], np.array([0.0, 0.0, -4.0], F)) and same_bits(Fz[0], np.array([0.5, -0.25, 5.0], F))
    assert bz[0] == 4.0
    # -0 is removed from d: w.x = -0 and F.x = -0 + +0 = +0 give w - F = -0 without the + 0.0f
    _, dm, _, _ = lights.sun_model(np.array([[-0.0, 1.0, 1.0, 1.0]], F), np.array([-0.0, 0.0, 0.0], F),
                                   (0.0, 0.0, 1.0), 4.0, 0.0)
    assert same_bits(dm[0, 0], F(0.0))
    # an image keeps its shape
    F2, d2, b2, s2 = lights.sun_model(pos.reshape(5, 8, 4), o, s, 4.0, 0.0)
    assert F2.shape == d2.shape == (5, 8, 3) and same_bits(d2.reshape(40, 3), d) and same_bits(b2.reshape(40), bound)
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            lights.sun_model(pos, o, s, 4.0, bad)
    for bad in (0.0, -4.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            lights.sun_model(pos, o, s, bad, 0.0)


def test_light_model_sun_on_a_few_pixels():
    pos = np.array([[0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 0, 1], [0, 0, 1, 1], [0, 0, 1, 1]], F)
    nrm = np.array([[0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 1, 1], [0, 0, -1, 1], [0.6, 0, 0.8, 1]], F)
    vis = np.array([255, 0, 255, 255, 255], np.uint8)
    rgba = np.full((5, 4), 200, np.uint8)
    out = lights.light_model_sun(rgba, pos, nrm, vis, (0.0, 0.0, 1.0), 0.25)
    assert out.dtype == np.uint8 and (out[:, 3] == 200).all()
    assert (out[0, :3] == 200).all()        # lit, facing the sun: k = 1
    assert (out[1, :3] == 50).all()         # shadowed: k = ambient, 200 * 0.25 + 0.5 -> 50
    assert (out[2] == 200).all()            # a miss of the frame stays
    assert (out[3, :3] == 50).all()         # facing away: the Lambert term clamps to 0
    # by hand: lam = (0.6 * 0 + 0 * 0) + 0.8 * 1 = 0.8f, k = 0.25 + 0.75 * 0.8f, c = uint8(200 k + 0.5)
    k = F(0.25) + F(0.75) * F(0.8)
    assert (out[4, :3] == np.uint8(F(200) * k + F(0.5))).all() and out[4, 0] == 170
    assert (rgba == 200).all()              # not in place
    with pytest.raises(ValueError):
        lights.light_model_sun(rgba, pos, nrm, vis, (0.0, 0.0, 1.0), 1.5)


def test_sun_direction_and_matched_lod():
    s = lights.sun_direction((0.7, 0.7, 0.2))   # the reference's lightDir
    assert s.dtype == F and abs(float(np.linalg.norm(s.astype(np.float64))) - 1.0) < 1e-7
    assert np.allclose(s, np.array([0.7, 0.7, 0.2]) / math.sqrt(1.02), rtol=0, atol=1e-7)
    for bad in ((0, 0, 0), (np.nan, 0, 1), (np.inf, 0, 0)):
        with pytest.raises(ValueError):
            lights.sun_direction(bad)
    assert lights.matched_lod(4.0, 4.0) == F(70.0) and lights.matched_lod(4.0, 1.0) == F(140.0)
    assert lights.matched_lod(4.0, 1.0, 60.0) == F(120.0)
    assert lights.matched_lod(4.0, su.T3_CLOSEST) == F(70.0 * math.sqrt(4.0 / 0.1258))
    assert 394.6 < su.matched() < 394.8
    for bad in ((0.0, 1.0), (4.0, 0.0), (4.0, -1.0), (float("nan"), 1.0), (4.0, float("inf"))):
        with pytest.raises(ValueError):
            lights.matched_lod(*bad)
    assert lights.DEFAULT_SUN_DISTANCE == 4.0


def test_oracle_facts_of_the_gpu_cases():
    """The figures the GPU tests stand on, at tau = 4 and bias 2^-10: both outcomes occur in quantity, every ray starts
    outside the radius-2 ball, and the matched LOD constant changes bits."""
    want = {("t1", "side", None): (830, 285, 545, 7), ("t3", "cam", None): (1200, 217, 983, 6),
            ("t3", "cam", su.matched()): (1200, 230, 970, 9)}
    vis = {}
    for (name, dn, lod), figures in want.items():
        S = pyoracle.load_setup(name)
        pos = frame(name)["pos4"]
        mint, pick, deepest = su.frame_rays(name, dn, su.TAU, "avx", lod, 1 if name == "t1" else 3)
        v = su.vis_of(pos, S["origin"], su.direction(dn), su.TAU, su.B10, mint, pick)
        got = (int(pick.sum()), int((v[pick] == 0).sum()), int((v[pick] == 255).sum()), deepest)
        print(name, dn, lod, got)
        assert got == figures
        assert (v[~pick] == 255).all()
        Fo, _, _, _ = lights.sun_model(pos, S["origin"], su.direction(dn), su.TAU, 0.0)
        assert np.linalg.norm(Fo[pick].astype(np.float64), axis=-1).min() >= 2.32
        vis[lod] = v
    assert int((vis[None] != vis[su.matched()]).sum()) == 13
    assert abs(float(frame("t3")["stats"]["closest"]) - su.T3_CLOSEST) < 1e-4


def test_header_documents_the_consequences():
    text = " ".join(pathlib.Path(sf.HEADER_PATH).read_text().split())
    for sym in SYMBOLS + ("sf_sun_params",):
        assert sym in text, sym
    assert "THE LEVEL OF DETAIL IS THAT OF A VIEWER AT DISTANCE tau" in text
    assert "tau >= 4 puts every F outside" in text
    assert "matched_lod" in text
    assert "#define SF_ABI_VERSION 1" in text


def test_symbols_are_exported():
    if shutil.which("nm") is None:
        pytest.skip("binutils not available")
    have = defined_symbols(sf.LIB_PATH)
    assert set(SYMBOLS) <= have
    assert set(SYMBOLS) <= set(sf.SIGNATURES)


def test_struct_layout_matches_the_header():
    assert ctypes.sizeof(sf.sf_sun_params) == 56
    assert sf.sf_sun_params.distance.offset == 12 and sf.sf_sun_params.bias.offset == 16
    assert sf.sf_sun_params.origin.offset == 20 and sf.sf_sun_params.use_origin.offset == 32
    assert sf.sf_sun_params.max_depth.offset == 44 and sf.sf_sun_params.stream.offset == 48


def test_null_context_is_einval():
    L = sf.lib()
    p = sf.sf_sun_params()
    buf = (ctypes.c_float * 64)()
    vp = ctypes.cast(buf, ctypes.c_void_p)
    assert L.sf_sun_defaults(None, ctypes.byref(p)) == sf.SF_EINVAL
    assert L.sf_trace_sun_to(None, ctypes.byref(p), vp, vp) == sf.SF_EINVAL
    assert L.sf_trace_sun(None, ctypes.byref(p)) == sf.SF_EINVAL
    assert L.sf_light_image_sun(None, ctypes.byref(p), 0.25, vp, vp, vp, vp) == sf.SF_EINVAL
    assert L.sf_set_shadow_lod(None, 70.0) == sf.SF_EINVAL
    assert math.isnan(L.sf_get_shadow_lod(None))


def test_cpp_members_are_inline_over_the_c_abi(tmp_path):
    """Sphereflake::SetShadowLod / TraceSun / LightImageSun compile for an application, stay inline, and need only
    sf_* symbols the library has."""
    if shutil.which("g++") is None or shutil.which("nm") is None:
        pytest.skip("binutils / g++ not available")
    source = ('#include "Sphereflake.hpp"\n'
              "using namespace SphereflakeRaytracer;\n"
              "void light(Sphereflake& s, const float* pdev, uint8_t* vdev) {\n"
              "    sf_sun_params p;\n"
              "    sf_sun_defaults(s.Context(), &p);\n"
              "    p.dir[0] = 0.6f; p.dir[1] = 0.0f; p.dir[2] = 0.8f;\n"
              "    s.SetShadowLod(140.0f);\n"
              "    s.TraceSun(p);\n"
              "    s.LightImageSun(p, 0.25f);\n"
              "    p.width = 64; p.height = 36;\n"
              "    s.TraceSun(p, pdev, vdev);\n}\n")
    obj = compile_class_user(tmp_path, "sun", source)
    need, have = undefined_symbols(obj), defined_symbols(sf.LIB_PATH)
    assert {"sf_set_shadow_lod", "sf_trace_sun_to", "sf_trace_sun", "sf_light_image_sun"} <= need
    assert not [n for n in need if "TraceSun" in n or "LightImageSun" in n or "SetShadowLod" in n]
    assert not [n for n in need if (n.startswith("sf_") or "SphereflakeRaytracer" in n) and n not in have]
