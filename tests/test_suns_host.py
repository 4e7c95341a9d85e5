"""Host side of the many-sun-directions traces (sf_trace_suns_to, sf_light_image_suns): the direction generators and
the host statement of the definition (sphereflake_amd.lights) against sun_model / light_model_sun and a scalar
restatement, the oracle facts the GPU tests stand on, the header and the library's exports, and the error codes that
need no device. No GPU needed."""
import ctypes
import pathlib
import shutil

import numpy as np
import pytest

import sphereflake_amd as sf
from sphereflake_amd import lights
from abicheck import compile_class_user, defined_symbols, undefined_symbols
from dirscheck import same_bits
import suncheck as su
import sunscheck as ss

F = np.float32
SYMBOLS = ("sf_suns_defaults", "sf_trace_suns_to", "sf_trace_suns", "sf_light_image_suns")


def angles(dirs, axis):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.arccos(np.clip(dirs.astype(np.float64) @ a, -1.0, 1.0))


def test_sun_cone():
    for axis in (su.VECTORS["side"], su.VECTORS["cam"], (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (-0.95, 0.2, 0.1)):
        for half in (np.radians(0.25), np.radians(5.0), np.radians(30.0)):
            for n in (1, 8, 16, 64):
                D = lights.sun_cone(axis, half, n)
                assert D.dtype == F and D.shape == (n, 3)
                assert np.abs(np.linalg.norm(D.astype(np.float64), axis=1) - 1.0).max() < 1e-7
                ang = angles(D, axis)
                assert ang.max() < half + 1e-6                 # all inside the cone
                assert ang[0] == ang.min() and (np.diff(ang) > -1e-6).all()   # the first ring nearest the axis
                mean = D.astype(np.float64).mean(axis=0)
                # the mean direction: one sample sits at half sqrt(1 / 2), the disc's median radius; n of them turned
                # by the golden angle cancel at least as well as n random ones would (1 / sqrt(n))
                assert angles(mean[None] / np.linalg.norm(mean), axis)[0] < half / np.sqrt(2.0 * n) + 1e-6
                assert same_bits(D, lights.sun_cone(axis, half, n))   # deterministic
                if n >= 8:   # the samples fill the cone: the outermost reaches most of the half angle
                    assert ang.max() > 0.9 * half
                    assert len(np.unique(D, axis=0)) == n
    assert same_bits(lights.sun_cone((0.7, 0.7, 0.2), 0.0, 3), np.tile(lights.sun_direction((0.7, 0.7, 0.2)), (3, 1)))
    for bad in ((0, 0, 0), (np.nan, 0, 1)):
        with pytest.raises(ValueError):
            lights.sun_cone(bad, 0.1, 4)
    for half in (-0.1, np.pi / 2, float("nan")):
        with pytest.raises(ValueError):
            lights.sun_cone((0, 0, 1), half, 4)
    for n in (0, 65):
        with pytest.raises(ValueError):
            lights.sun_cone((0, 0, 1), 0.1, n)


def test_sky_dirs():
    for up in ((0.0, 0.0, 1.0), (1.0, 2.0, -3.0)):
        for n in (1, 16, 64):
            D = lights.sky_dirs(n, up)
            assert D.dtype == F and D.shape == (n, 3)
            assert np.abs(np.linalg.norm(D.astype(np.float64), axis=1) - 1.0).max() < 1e-7
            assert (D.astype(np.float64) @ np.asarray(up) > 0).all()
            assert same_bits(D, lights.sky_dirs(n, up))
            # sky()'s points, normalised
            P = lights.sky(n, 4.0, up).astype(np.float64)
            assert np.abs(D - P / np.linalg.norm(P, axis=1, keepdims=True)).max() < 1e-6
    with pytest.raises(ValueError):
        lights.sky_dirs(65)
    with pytest.raises(ValueError):
        lights.sky_dirs(4, (0, 0, 0))


def test_suns_model_is_sun_model_per_direction():
    rng = np.random.default_rng(229)
    pos = rng.normal(scale=1.5, size=(5, 8, 4)).astype(F)
    pos[0, 3, :3] = 0.0
    pos[1, 2, :3] = (np.inf, 1.0, 1.0)
    o = np.array([1.25, -2.5, 0.75], F)
    D = np.concatenate([lights.sun_cone(su.VECTORS["side"], ss.HALF_ANGLE, 5), [[0, 0, 0], [np.nan, 0, 1]]]).astype(F)
    Fo, d, bound, surf = lights.suns_model(pos, o, D, 4.0, su.B10)
    assert Fo.shape == d.shape == (7, 5, 8, 3) and bound.shape == (7, 5, 8) and surf.shape == (5, 8)
    assert Fo.dtype == d.dtype == bound.dtype == F
    for i in range(7):
        F1, d1, b1, s1 = lights.sun_model(pos, o, D[i], 4.0, su.B10)
        assert same_bits(Fo[i], F1) and same_bits(d[i], d1) and same_bits(bound[i], b1) and np.array_equal(surf, s1)
    with pytest.raises(ValueError):
        lights.suns_model(pos, o, np.zeros((65, 3), F), 4.0, 0.0)
    with pytest.raises(ValueError):
        lights.suns_model(pos, o, D, 0.0, 0.0)


def scalar_suns_pixel(c, nrm, m, D, w, ambient):
    """sf.h's statement of sf_light_image_suns for one surface pixel's colour byte, one float32 operation at a time."""
    S = F(0.0)
    for i in range(len(D)):
        dot = (F(nrm[0]) * D[i][0] + F(nrm[1]) * D[i][1]) + F(nrm[2]) * D[i][2]
        lam = np.fmax(F(0.0), dot)
        S = S + w[i] * (lam if (int(m) >> i) & 1 else F(0.0))
    k = F(ambient) + (F(1.0) - F(ambient)) * S
    return np.uint8(np.fmin(F(c) * k + F(0.5), F(255.0)))


def test_light_model_suns():
    rng = np.random.default_rng(233)
    npx = 48
    pos = rng.normal(size=(npx, 4)).astype(F)
    pos[5, :3] = 0.0
    nrm = rng.normal(size=(npx, 4)).astype(F)
    nrm[:, :3] /= np.linalg.norm(nrm[:, :3], axis=1, keepdims=True)
    rgba = rng.integers(0, 256, size=(npx, 4)).astype(np.uint8)
    # n = 1 and weight 1: light_model_sun, byte for byte
    s = su.direction("side")
    vis = np.where(rng.random(npx) < 0.5, 255, 0).astype(np.uint8)
    one = lights.light_model_suns(rgba, pos, nrm, lights.masks_from_vis([vis]), [s], [1.0], 0.25)
    assert np.array_equal(one, lights.light_model_sun(rgba, pos, nrm, vis, s, 0.25)) and (one != rgba).any()
    # 64 directions against the scalar restatement, bits >= 32 live, default and explicit weights
    D = lights.sky_dirs(64)
    mask = rng.integers(0, 2 ** 63, size=npx, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=npx).astype(np.uint64)
    for weights in (None, rng.random(64).astype(F) * F(0.05)):
        w = np.full(64, F(1.0) / F(64), F) if weights is None else weights
        for ambient in (0.25, 0.0):
            out = lights.light_model_suns(rgba, pos, nrm, mask, D, weights, ambient)
            assert out.dtype == np.uint8 and np.array_equal(out[:, 3], rgba[:, 3]) and np.array_equal(out[5], rgba[5])
            for p in range(npx):
                if p != 5:
                    for ch in range(3):
                        assert out[p, ch] == scalar_suns_pixel(rgba[p, ch], nrm[p], mask[p], D, w, ambient), (p, ch)
        low = lights.light_model_suns(rgba, pos, nrm, mask & np.uint64(0xffffffff), D, weights, 0.25)
        assert (low != lights.light_model_suns(rgba, pos, nrm, mask, D, weights, 0.25)).any()
    # the sum runs in index order, and a byte tells: with x the float32 below 1/2 and e = 2^-27 (under half an ulp of
    # x), ((x + e) + e) + e = x and 3 x + 1/2 < 2: byte 1; ((e + e) + e) + x = 1/2 and 3 / 2 + 1/2 = 2: byte 2
    up = np.array([[0, 0, 1]] * 4, F)
    pz, nz = np.array([[0, 0, 1, 1]], F), np.array([[0, 0, 1, 1]], F)
    img = np.full((1, 4), 3, np.uint8)
    x, e = np.nextafter(F(0.5), F(0.0)), F(2.0 ** -27)
    assert ((x + e) + e) + e == x and ((e + e) + e) + x == F(0.5)
    big_first = lights.light_model_suns(img, pz, nz, [15], up, [x, e, e, e], 0.0)
    big_last = lights.light_model_suns(img, pz, nz, [15], up, [e, e, e, x], 0.0)
    assert tuple(big_first[0]) == (1, 1, 1, 3) and tuple(big_last[0]) == (2, 2, 2, 3)
    assert tuple(lights.light_model_suns(img, pz, nz, [7], up, [e, e, e, x], 0.0)[0]) == (0, 0, 0, 3)   # bit 3 clear
    with pytest.raises(ValueError):
        lights.light_model_suns(img, pz, nz, [15], up, [x, e, e, -e], 0.0)   # no negative weights
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            lights.light_model_suns(img, pz, nz, [1], up, None, bad)
    with pytest.raises(ValueError):
        lights.light_model_suns(img, pz, nz, [1], up, [1.0, 1.0], 0.25)


@pytest.mark.parametrize("name,traced", [("t1", 830), ("t3", 1200)])
def test_oracle_facts_of_the_cone_cases(name, traced):
    """The conditions the GPU tests stand on, at tau = 4 and bias 2^-10. Measured: t1 220 mixed, at least 250 shadowed
    and 517 lit per direction, deepest node 7; t3 295 mixed, 181 / 890, deepest 6."""
    D = ss.cone(name)
    every = ss.CONE_CASES[name][1]
    m, pick = ss.oracle_mask(name, D, every=every)
    shadowed = [int((pick & ~ss.bit(m, i)).sum()) for i in range(8)]
    lit = [int((pick & ss.bit(m, i)).sum()) for i in range(8)]
    nmixed = int(ss.mixed(m, 8, pick).sum())
    print(name, int(pick.sum()), "mixed", nmixed, "shadowed", shadowed, "lit", lit, ss.frame_rays(name, D, every=every)[2])
    assert int(pick.sum()) == traced
    assert nmixed >= 100 and min(shadowed) >= 100 and min(lit) >= 100
    assert (m >> np.uint64(8) == 0).all() and (m[~pick] == np.uint64(255)).all()
    # every ray starts outside the radius-2 ball
    Fo, _, _, _ = lights.suns_model(ss.frame(name)["pos4"], ss.pyoracle.load_setup(name)["origin"], D, su.TAU, 0.0)
    assert np.linalg.norm(Fo[:, pick].astype(np.float64), axis=-1).min() >= 2.0


def test_oracle_facts_of_the_sky_case():
    """t1 under sky_dirs(64), every 8th surface pixel. Measured: 31 directions with at least 20 shadowed and 20 lit
    pixels of the sample, 16 of them with index >= 32; deepest node 8."""
    D = lights.sky_dirs(64)
    m, pick = ss.oracle_mask("t1", D, every=ss.SKY_EVERY)
    assert int(pick.sum()) == 104
    both = [i for i in range(64) if int((pick & ~ss.bit(m, i)).sum()) >= 20 and int((pick & ss.bit(m, i)).sum()) >= 20]
    print("sky", both)
    assert len([i for i in both if i >= 32]) >= 8   # (a 32-bit shift cannot pass)


def test_header_declares_the_entries():
    text = " ".join(pathlib.Path(sf.HEADER_PATH).read_text().split())
    for sym in SYMBOLS + ("sf_suns_params",):
        assert sym in text, sym
    assert "#define SF_SUN_DIRS_MAX 64" in text and sf.SF_SUN_DIRS_MAX == 64
    assert "DEFINITION OF THE MASK (exact). Bit i (i < n) of mask[p] is 1 iff sf_trace_sun_to with dir = dirs[i]" in text
    assert "#define SF_ABI_VERSION 1" in text


def test_symbols_are_exported():
    if shutil.which("nm") is None:
        pytest.skip("binutils not available")
    have = defined_symbols(sf.LIB_PATH)
    assert set(SYMBOLS) <= have
    assert set(SYMBOLS) <= set(sf.SIGNATURES)


def test_struct_layout_matches_the_header():
    P = sf.sf_suns_params
    assert ctypes.sizeof(P) == 64
    assert (P.dirs.offset, P.weights.offset, P.n.offset, P.distance.offset, P.bias.offset) == (0, 8, 16, 20, 24)
    assert (P.origin.offset, P.use_origin.offset, P.width.offset, P.height.offset) == (28, 40, 44, 48)
    assert (P.max_depth.offset, P.stream.offset) == (52, 56)


def test_null_context_is_einval():
    L = sf.lib()
    p = sf.sf_suns_params()
    buf = (ctypes.c_float * 64)()
    vp = ctypes.cast(buf, ctypes.c_void_p)
    p.dirs, p.n, p.distance = ctypes.cast(buf, ctypes.POINTER(ctypes.c_float)), 1, 4.0
    assert L.sf_suns_defaults(None, ctypes.byref(p)) == sf.SF_EINVAL
    assert L.sf_trace_suns_to(None, ctypes.byref(p), vp, vp) == sf.SF_EINVAL
    assert L.sf_trace_suns(None, ctypes.byref(p)) == sf.SF_EINVAL
    assert L.sf_light_image_suns(None, ctypes.byref(p), 0.25, vp, vp, vp, vp) == sf.SF_EINVAL
    assert p.n == 1   # (a refused sf_suns_defaults wrote nothing)


def test_cpp_members_are_inline_over_the_c_abi(tmp_path):
    """Sphereflake::TraceSuns / LightImageSuns compile for an application, stay inline, and need only sf_* symbols the
    library has."""
    if shutil.which("g++") is None or shutil.which("nm") is None:
        pytest.skip("binutils / g++ not available")
    source = ('#include "Sphereflake.hpp"\n'
              "using namespace SphereflakeRaytracer;\n"
              "void light(Sphereflake& s, const float* pdev, uint64_t* mdev) {\n"
              "    static const float dirs[6] = { 0.6f, 0.0f, 0.8f, 0.0f, 0.6f, 0.8f };\n"
              "    sf_suns_params p;\n"
              "    sf_suns_defaults(s.Context(), &p);\n"
              "    p.dirs = dirs; p.n = 2;\n"
              "    s.TraceSuns(p);\n"
              "    s.LightImageSuns(p, 0.25f);\n"
              "    p.width = 64; p.height = 36;\n"
              "    s.TraceSuns(p, pdev, mdev);\n}\n")
    obj = compile_class_user(tmp_path, "suns", source)
    need, have = undefined_symbols(obj), defined_symbols(sf.LIB_PATH)
    assert {"sf_trace_suns_to", "sf_trace_suns", "sf_light_image_suns"} <= need
    assert not [n for n in need if "TraceSuns" in n or "LightImageSuns" in n]
    assert not [n for n in need if (n.startswith("sf_") or "SphereflakeRaytracer" in n) and n not in have]
