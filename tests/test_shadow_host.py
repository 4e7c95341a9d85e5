"""Host side of the point-light shadows (sf_trace_shadow_to, sf_light_image): the host statement of the definition
(sphereflake_amd.lights) against a scalar restatement, the oracle helper's counts, the header and the library's
exports, and the error codes that need no device. No GPU needed."""
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
import shadowcheck as sc

F = np.float32
SYMBOLS = ("sf_shadow_defaults", "sf_trace_shadow_to", "sf_trace_shadow", "sf_download_shadow", "sf_shadow_buffer",
           "sf_light_image")


def scalar_shadow(P, o, l, b):
    """Steps 1-3 of sf.h's definition for one pixel, one float32 operation at a time."""
    P, o, l = [F(v) for v in P], [F(v) for v in o], [F(v) for v in l]
    surface = not (P[0] == 0 and P[1] == 0 and P[2] == 0)
    with np.errstate(all="ignore"):
        w = [o[k] + P[k] for k in range(3)]
        d = [(w[k] - l[k]) + F(0.0) for k in range(3)]
        length = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        bound = length * (F(1.0) - F(b))
    return np.array(d, F), F(bound), surface


def test_shadow_model_equals_the_scalar_restatement():
    rng = np.random.default_rng(211)
    pos = rng.normal(scale=3.0, size=(40, 4)).astype(F)
    pos[3, :3] = 0.0                       # a miss of the frame
    pos[4, :3] = (-0.0, 0.0, -0.0)         # ... whatever the zeros' signs
    pos[5, :3] = (0.0, 0.0, 1e-30)         # no miss
    o = np.array([1.25, -2.5, 0.75], F)
    l = np.array([-1.5, -2.5, 2.0], F)
    pos[6, :3] = l - o                     # the light itself: d = +0 (never -0), bound 0
    pos[7, 1] = 0.0                        # w.y - l.y = -2.5 - -2.5: +0 after the + 0.0f
    pos[8, :3] = (np.inf, 1.0, 1.0)
    pos[9, :3] = (np.nan, 1.0, 1.0)
    for b in (0.0, 2.0 ** -11, 2.0 ** -9, 2.0 ** -7, 0.5):
        d, bound, surf = lights.shadow_model(pos, o, l, b)
        assert d.dtype == F and bound.dtype == F and d.shape == (40, 3) and bound.shape == surf.shape == (40,)
        for i in range(40):
            sd, sb, ss = scalar_shadow(pos[i, :3], o, l, b)
            assert same_bits(d[i], sd) and same_bits(bound[i], sb) and bool(surf[i]) == ss, (i, b)
        assert not np.signbit(d[d == 0]).any()
    d, bound, surf = lights.shadow_model(pos, o, l, 0.0)
    assert not surf[3] and not surf[4] and surf[5] and surf[6]
    assert same_bits(d[6], np.zeros(3, F)) and bound[6] == 0
    assert same_bits(d[7, 1], F(0.0))
    # -0 - +0 = -0 without the + 0.0f
    d3, _, s3 = lights.shadow_model(np.array([[-0.0, 1.0, 1.0, 1.0]], F), np.array([-0.0, 1.0, 1.0], F), np.zeros(3, F), 0.0)
    assert s3[0] and same_bits(d3[0], np.array([0.0, 2.0, 2.0], F))
    # an image keeps its shape
    img = pos.reshape(5, 8, 4)
    d2, b2, s2 = lights.shadow_model(img, o, l, 0.0)
    assert d2.shape == (5, 8, 3) and same_bits(d2.reshape(40, 3), d) and same_bits(b2.reshape(40), bound)
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError):
            lights.shadow_model(pos, o, l, bad)


def test_light_model_on_a_few_pixels():
    o = np.zeros(3, F)
    l = np.array([0.0, 0.0, 4.0], F)
    pos = np.array([[0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 0, 1], [0, 0, 1, 1]], F)
    nrm = np.array([[0, 0, 1, 1], [0, 0, 1, 1], [0, 0, 1, 1], [0, 0, -1, 1]], F)
    vis = np.array([255, 0, 255, 255], np.uint8)
    rgba = np.full((4, 4), 200, np.uint8)
    out = lights.light_model(rgba, pos, nrm, vis, o, l, 0.25)
    assert out.dtype == np.uint8 and (out[:, 3] == 200).all()
    assert (out[0, :3] == 200).all()        # lit, facing the light: k = 1
    assert (out[1, :3] == 50).all()         # shadowed: k = ambient, 200 * 0.25 + 0.5 -> 50
    assert (out[2] == 200).all()            # a miss of the frame stays
    assert (out[3, :3] == 50).all()         # facing away: the Lambert term clamps to 0
    assert (rgba == 200).all()              # not in place


def test_oracle_counts_of_the_gpu_cases():
    """The figures the GPU tests stand on, at bias 2^-9: both outcomes occur, so a constant output cannot pass."""
    want = {("t1", "side"): (454, 376, 1474), ("t3", "side"): (2505, 1095, 0), ("t3", "top"): (3358, 242, 0),
            ("t1", "low"): (618, 212, 1474)}
    for name, light_name in sc.CASES:
        vis = sc.oracle_vis(name, light_name, 2.0 ** -9)
        surf = frame(name)["minT"] < np.finfo(F).max
        got = (int((vis == 0).sum()), int(((vis == 255) & surf).sum()), int((~surf).sum()))
        print(name, light_name, got)
        assert got == want[(name, light_name)]
        assert (vis[~surf] == 255).all()
    # the bias only ever removes shadow
    a, b = sc.oracle_vis("t3", "side", 0.0), sc.oracle_vis("t3", "side", 2.0 ** -7)
    assert ((a == 0) | (b == 255)).all() and (a != b).any()


def test_header_documents_the_consequences():
    text = " ".join(pathlib.Path(sf.HEADER_PATH).read_text().split())
    for sym in SYMBOLS + ("sf_shadow_params",):
        assert sym in text, sym
    assert "THE LEVEL OF DETAIL IS THE LIGHT'S" in text
    assert "A LIGHT INSIDE THE RADIUS-2 BALL" in text
    assert "#define SF_ABI_VERSION 1" in text


def test_symbols_are_exported():
    if shutil.which("nm") is None:
        pytest.skip("binutils not available")
    have = defined_symbols(sf.LIB_PATH)
    assert set(SYMBOLS) <= have
    assert set(SYMBOLS) <= set(sf.SIGNATURES)


def test_struct_layout_matches_the_header():
    assert ctypes.sizeof(sf.sf_shadow_params) == 56
    assert sf.sf_shadow_params.bias.offset == 12 and sf.sf_shadow_params.origin.offset == 16
    assert sf.sf_shadow_params.use_origin.offset == 28 and sf.sf_shadow_params.stream.offset == 48


def test_null_context_is_einval():
    L = sf.lib()
    p = sf.sf_shadow_params()
    buf = (ctypes.c_float * 64)()
    vp = ctypes.cast(buf, ctypes.c_void_p)
    assert L.sf_shadow_defaults(None, ctypes.byref(p)) == sf.SF_EINVAL
    assert L.sf_trace_shadow_to(None, ctypes.byref(p), vp, vp) == sf.SF_EINVAL
    assert L.sf_trace_shadow(None, ctypes.byref(p)) == sf.SF_EINVAL
    assert L.sf_download_shadow(None, vp) == sf.SF_EINVAL
    assert L.sf_shadow_buffer(None, ctypes.byref(ctypes.c_void_p())) == sf.SF_EINVAL
    assert L.sf_light_image(None, ctypes.byref(p), 0.25, vp, vp, vp, vp) == sf.SF_EINVAL


def test_cpp_members_are_inline_over_the_c_abi(tmp_path):
    """Sphereflake::TraceShadow / LightImage compile for an application, stay inline, and need only sf_* symbols the
    library has."""
    if shutil.which("g++") is None or shutil.which("nm") is None:
        pytest.skip("binutils / g++ not available")
    source = ('#include "Sphereflake.hpp"\n'
              "using namespace SphereflakeRaytracer;\n"
              "void light(Sphereflake& s, const float* pdev, uint8_t* vdev) {\n"
              "    sf_shadow_params p;\n"
              "    sf_shadow_defaults(s.Context(), &p);\n"
              "    p.light[0] = -1.5f; p.light[1] = -2.5f; p.light[2] = 2.0f;\n"
              "    s.TraceShadow(p);\n"
              "    s.LightImage(p, 0.25f);\n"
              "    p.width = 64; p.height = 36;\n"
              "    s.TraceShadow(p, pdev, vdev);\n}\n")
    obj = compile_class_user(tmp_path, "shadow", source)
    need, have = undefined_symbols(obj), defined_symbols(sf.LIB_PATH)
    assert {"sf_trace_shadow_to", "sf_trace_shadow", "sf_light_image"} <= need
    assert not [n for n in need if "TraceShadow" in n or "LightImage" in n]
    assert not [n for n in need if (n.startswith("sf_") or "SphereflakeRaytracer" in n) and n not in have]
