"""Host side of the many-light shadows (sf_trace_shadows_to, sf_light_image_many): the library's exports and the
header, the error codes that need no device, the light generators and the host statement of the lighting
(sphereflake_amd.lights). No GPU needed."""
import ctypes
import pathlib
import shutil

import numpy as np
import pytest

import sphereflake_amd as sf
from sphereflake_amd import lights
from abicheck import compile_class_user, defined_symbols, undefined_symbols
from oracle import pyoracle
from rayscheck import frame
import shadowcheck as sc

F = np.float32
SYMBOLS = ("sf_shadows_defaults", "sf_trace_shadows_to", "sf_trace_shadows", "sf_download_shadow_masks",
           "sf_shadow_mask_buffer", "sf_light_image_many")


def test_symbols_are_exported():
    if shutil.which("nm") is None:
        pytest.skip("binutils not available")
    have = defined_symbols(sf.LIB_PATH)
    assert set(SYMBOLS) <= have
    assert set(SYMBOLS) <= set(sf.SIGNATURES)


def test_header_carries_the_definition():
    text = " ".join(pathlib.Path(sf.HEADER_PATH).read_text().split())
    for sym in SYMBOLS + ("sf_shadows_params",):
        assert sym in text, sym
    assert "#define SF_SHADOW_LIGHTS_MAX 64" in text and sf.SF_SHADOW_LIGHTS_MAX == 64 == lights.LIGHTS_MAX
    assert "DEFINITION OF THE MASK" in text and "Bits n..63 are 0" in text
    assert "THE LEVEL OF DETAIL IS EACH LIGHT'S OWN" in text
    assert "#define SF_ABI_VERSION 1" in text


def test_struct_layout_matches_the_header():
    P = sf.sf_shadows_params
    assert ctypes.sizeof(P) == 64
    assert (P.lights.offset, P.weights.offset, P.n.offset, P.bias.offset) == (0, 8, 16, 20)
    assert (P.origin.offset, P.use_origin.offset, P.width.offset, P.height.offset) == (24, 36, 40, 44)
    assert (P.max_depth.offset, P.stream.offset) == (48, 56)


def test_errors_that_need_no_device():
    L = sf.lib()
    p = sf.sf_shadows_params()
    p.n = 7
    buf = (ctypes.c_float * 64)()
    vp = ctypes.cast(buf, ctypes.c_void_p)
    assert L.sf_shadows_defaults(None, ctypes.byref(p)) == sf.SF_EINVAL
    assert p.n == 7   # (untouched)
    assert L.sf_trace_shadows_to(None, ctypes.byref(p), vp, vp) == sf.SF_EINVAL
    assert L.sf_trace_shadows(None, ctypes.byref(p)) == sf.SF_EINVAL
    assert L.sf_download_shadow_masks(None, vp) == sf.SF_EINVAL
    assert L.sf_shadow_mask_buffer(None, ctypes.byref(ctypes.c_void_p())) == sf.SF_EINVAL
    assert L.sf_light_image_many(None, ctypes.byref(p), 0.25, vp, vp, vp, vp) == sf.SF_EINVAL


@pytest.mark.parametrize("n", [0, 65, -1])
def test_generators_refuse_a_count_out_of_range(n):
    with pytest.raises(ValueError):
        lights.disc(sc.LIGHTS["side"], 0.25, n)
    with pytest.raises(ValueError):
        lights.sky(n)


def test_model_and_helper_refuse_a_count_out_of_range():
    with pytest.raises(ValueError):
        lights.masks_from_vis([])
    with pytest.raises(ValueError):
        lights.masks_from_vis([np.zeros((2, 2), np.uint8)] * 65)
    rgba, g, m = np.zeros((2, 2, 4), np.uint8), np.ones((2, 2, 4), F), np.zeros((2, 2), np.uint64)
    for L in (np.zeros((0, 3), F), np.ones((65, 3), F)):
        with pytest.raises(ValueError):
            lights.light_model_many(rgba, g, g, m, np.zeros(3, F), L)
    for w in ((0.5, -0.5), (np.nan, 1.0), (1.0,)):
        with pytest.raises(ValueError):
            lights.light_model_many(rgba, g, g, m, np.zeros(3, F), np.ones((2, 3), F), w)


def test_disc():
    c = np.asarray(sc.LIGHTS["side"], np.float64)
    for n in (1, 16, 64):
        d = lights.disc(sc.LIGHTS["side"], 0.25, n)
        assert d.dtype == F and d.shape == (n, 3)
        assert np.array_equal(d, lights.disc(sc.LIGHTS["side"], 0.25, n))   # deterministic
        off = d.astype(np.float64) - c
        assert (np.linalg.norm(off, axis=1) <= 0.25 + 1e-6).all()
        assert np.abs(off @ (c / np.linalg.norm(c))).max() < 1e-6           # in the plane that faces the centre
        assert (np.linalg.norm(d.astype(np.float64), axis=1) > 2.0).all()   # outside the flake's bounding ball
        assert len(np.unique(d, axis=0)) == n
    d = lights.disc(sc.LIGHTS["side"], 0.25, 64).astype(np.float64)
    assert np.linalg.norm(d, axis=1).min() > 3.53
    # the stated construction, point 5 of 16
    a = -c / np.linalg.norm(c)
    u = np.cross(a, (0, 0, 1.0))
    u /= np.linalg.norm(u)
    v = np.cross(a, u)
    r, th = 0.25 * np.sqrt(5.5 / 16), 5 * np.pi * (3 - np.sqrt(5))
    assert np.array_equal(lights.disc(sc.LIGHTS["side"], 0.25, 16)[5], (c + r * np.cos(th) * u + r * np.sin(th) * v).astype(F))


def test_sky():
    for n in (1, 16, 64):
        s = lights.sky(n)
        assert s.dtype == F and s.shape == (n, 3)
        assert np.array_equal(s, lights.sky(n))
        s64 = s.astype(np.float64)
        assert np.allclose(np.linalg.norm(s64, axis=1), 4.0, atol=1e-5) and (np.linalg.norm(s64, axis=1) > 2.0).all()
        assert np.allclose(s64[:, 2], 4.0 * (np.arange(n) + 0.5) / n, atol=1e-5)   # z_i = (i + 0.5) / n along up
        assert len(np.unique(s, axis=0)) == n
    t = lights.sky(16, radius=3.0, up=(0, 2.0, 0)).astype(np.float64)
    assert np.allclose(t[:, 1], 3.0 * (np.arange(16) + 0.5) / 16, atol=1e-5)
    assert np.allclose(np.linalg.norm(t, axis=1), 3.0, atol=1e-5)


def test_masks_from_vis_round_trips():
    rng = np.random.default_rng(64)
    for n in (1, 2, 33, 64):
        vis = [np.where(rng.random((5, 7)) < 0.5, 255, 0).astype(np.uint8) for _ in range(n)]
        m = lights.masks_from_vis(vis)
        assert m.dtype == np.uint64 and m.shape == (5, 7)
        if n < 64:
            assert (m >> np.uint64(n) == 0).all()
        back = lights.vis_from_masks(m, n)
        assert all(np.array_equal(a, b) for a, b in zip(vis, back))
    m = lights.masks_from_vis([np.full((1, 1), 255, np.uint8)] * 64)
    assert int(m[0, 0]) == 0xffffffffffffffff


def test_one_light_of_weight_one_is_light_model():
    """light_model_many with n = 1 and weight 1 equals light_model byte for byte on the t1 oracle frame."""
    S = pyoracle.load_setup("t1")
    fr = frame("t1")
    vis = sc.oracle_vis("t1", "side", 2.0 ** -9)
    rng = np.random.default_rng(5)
    rgba = rng.integers(0, 256, size=vis.shape + (4,), dtype=np.uint8)
    light = sc.LIGHTS["side"]
    for ambient in (0.25, 0.0):
        one = lights.light_model(rgba, fr["pos4"], fr["nrm4"], vis, S["origin"], light, ambient)
        many = lights.light_model_many(rgba, fr["pos4"], fr["nrm4"], lights.masks_from_vis([vis]), S["origin"],
                                       [light], [1.0], ambient)
        assert np.array_equal(one, many) and (one != rgba).any()
    # the sum is a sum: two copies of the light at weight 1/2 each give the same image (x/2 + x/2 is exact)
    m2 = lights.masks_from_vis([vis, vis])
    two = lights.light_model_many(rgba, fr["pos4"], fr["nrm4"], m2, S["origin"], [light, light], None, 0.25)
    assert np.array_equal(two, lights.light_model(rgba, fr["pos4"], fr["nrm4"], vis, S["origin"], light, 0.25))
    # ... and no clamp on S: two copies at weight 1 each brighten beyond one light
    over = lights.light_model_many(rgba, fr["pos4"], fr["nrm4"], m2, S["origin"], [light, light], [1.0, 1.0], 0.25)
    assert (over.astype(int) >= two.astype(int)).all() and (over != two).any()


def test_cpp_members_are_inline_over_the_c_abi(tmp_path):
    """Sphereflake::TraceShadows / LightImageMany compile for an application, stay inline, and need only sf_* symbols
    the library has."""
    if shutil.which("g++") is None or shutil.which("nm") is None:
        pytest.skip("binutils / g++ not available")
    source = ('#include "Sphereflake.hpp"\n'
              "using namespace SphereflakeRaytracer;\n"
              "void light(Sphereflake& s, const float* pdev, uint64_t* mdev) {\n"
              "    static const float l[6] = { -1.5f, -2.5f, 2.0f, 0.0f, 0.0f, 6.0f };\n"
              "    sf_shadows_params p;\n"
              "    sf_shadows_defaults(s.Context(), &p);\n"
              "    p.lights = l; p.n = 2;\n"
              "    s.TraceShadows(p);\n"
              "    s.LightImageMany(p, 0.25f);\n"
              "    p.width = 64; p.height = 36;\n"
              "    s.TraceShadows(p, pdev, mdev);\n}\n")
    obj = compile_class_user(tmp_path, "shadows", source)
    need, have = undefined_symbols(obj), defined_symbols(sf.LIB_PATH)
    assert {"sf_trace_shadows_to", "sf_trace_shadows", "sf_light_image_many"} <= need
    assert not [n for n in need if "TraceShadows" in n or "LightImageMany" in n]
    assert not [n for n in need if (n.startswith("sf_") or "SphereflakeRaytracer" in n) and n not in have]
