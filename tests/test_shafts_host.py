"""Host side of the light shafts (sf_trace_shafts_to, sf_light_image_shafts): the host statement of the definition
(sphereflake_amd.lights) against sun_model and a scalar restatement, the oracle facts the GPU tests stand on, the
header and the library's exports, and the error codes that need no device. No GPU needed."""
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
import shaftscheck as sc
import suncheck as su

F = np.float32
SYMBOLS = ("sf_shafts_defaults", "sf_trace_shafts_to", "sf_trace_shafts", "sf_light_image_shafts")


def test_shaft_fractions():
    for n in (1, 2, 8, 33, 64):
        f = lights.shaft_fractions(n)
        assert f.dtype == F and f.shape == (n,)
        assert same_bits(f, np.array([F((i + 0.5) / n) for i in range(n)], F))
        assert (f > 0).all() and (f < 1).all() and (np.diff(f) > 0).all()
    for n in (0, 65):
        with pytest.raises(ValueError):
            lights.shaft_fractions(n)


def test_shaft_ends():
    pos = frame("t1")["pos4"]
    surf = sc.surface_of(pos)
    D = sc.unit_dirs("t1")
    assert D.dtype == F and np.abs(np.linalg.norm(D.astype(np.float64), axis=-1) - 1.0).max() < 1e-6
    E = lights.shaft_ends(pos, D, 13.0)
    assert E.dtype == F and E.shape == pos.shape[:2] + (3,)
    assert same_bits(E[surf], pos[surf][:, :3])
    assert same_bits(E[~surf], D[~surf] * F(13.0))
    assert sc.surface_of(E).all()
    # a 4-float direction image is read the same; no image or far = 0 leaves the misses at 0
    D4 = np.concatenate([D, np.full(D.shape[:2] + (1,), 7.0, F)], axis=-1)
    assert same_bits(lights.shaft_ends(pos, D4, 13.0), E)
    for d, far in ((None, 13.0), (D, 0.0), (None, 0.0)):
        E0 = lights.shaft_ends(pos, d, far)
        assert same_bits(E0, pos[..., :3])
    # a zero direction at a miss stays unmarched; one rounding per component
    one = np.zeros((1, 2, 4), F)
    d2 = np.array([[[0.0, 0.0, 0.0], [0.1, -0.3, 0.7]]], F)
    E2 = lights.shaft_ends(one, d2, 3.3)
    assert not sc.surface_of(E2)[0, 0]
    assert same_bits(E2[0, 1], np.array([F(0.1) * F(3.3), F(-0.3) * F(3.3), F(0.7) * F(3.3)], F))
    for far in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            lights.shaft_ends(pos, D, far)
    with pytest.raises(ValueError):
        lights.shaft_ends(pos, D[:-1], 13.0)


@pytest.mark.parametrize("name", ["t1", "t3"])
def test_shafts_model_is_sun_model_on_the_scaled_images(name):
    S = pyoracle.load_setup(name)
    pos = frame(name)["pos4"]
    s, tau, far = sc.sun(name), sc.CASES[name][1], sc.CASES[name][2]
    fr = lights.shaft_fractions(8)
    E = lights.shaft_ends(pos, sc.dirs_of(name), far)
    Q = lights.shaft_samples(E, fr)
    assert Q.dtype == F and Q.shape == (8,) + E.shape
    got = lights.shafts_model(pos, S["origin"], s, tau, su.B10, fr, sc.dirs_of(name), far)
    for i in range(8):
        scaled = np.stack([E[..., 0] * fr[i], E[..., 1] * fr[i], E[..., 2] * fr[i]], axis=-1)
        assert same_bits(Q[i], scaled)
        want = lights.sun_model(scaled, S["origin"], s, tau, su.B10)
        for k in range(4):
            assert same_bits(np.asarray(got[k][i]), np.asarray(want[k])), (i, k)
    # a scalar restatement of one pixel, one sample
    y, x = np.argwhere(sc.surface_of(pos))[37]
    o = np.asarray(S["origin"], F)
    q = [F(E[y, x, k]) * fr[5] for k in range(3)]
    w = [o[k] + q[k] for k in range(3)]
    Fo = [w[k] + s[k] * F(tau) for k in range(3)]
    d = [(w[k] - Fo[k]) + F(0.0) for k in range(3)]
    bound = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) * (F(1.0) - F(su.B10))
    assert same_bits(got[0][5, y, x], np.array(Fo, F)) and same_bits(got[1][5, y, x], np.array(d, F))
    assert same_bits(got[2][5, y, x], F(bound)) and got[3][5, y, x]
    # a product that underflows is a sample without a ray
    tiny = np.zeros((1, 1, 4), F)
    tiny[0, 0, :3] = 1e-45   # (the least denormal: a quarter of it rounds to 0)
    assert not lights.shafts_model(tiny, o, s, tau, 0.0, [0.25])[3].any()
    for bad in ([], [0.0, 0.5], [-0.5], [float("nan")], [float("inf")], np.full(65, 0.5)):
        with pytest.raises(ValueError):
            lights.shaft_samples(E, bad)


def test_shaft_distance():
    for name in ("t1", "t3"):
        S = pyoracle.load_setup(name)
        o = np.asarray(S["origin"], np.float64)
        E = lights.shaft_ends(frame(name)["pos4"], sc.unit_dirs(name), 13.0)
        tau = lights.shaft_distance(S["origin"], E)
        assert isinstance(tau, F)
        r = np.linalg.norm(o + E.astype(np.float64), axis=-1).max()
        exact = 2.0 + max(r, np.linalg.norm(o))
        assert float(tau) >= exact and float(np.nextafter(tau, F(0.0))) < exact   # rounded up, no further
        # every ray of every sample then starts outside the radius-2 ball
        Fo = lights.shafts_model(frame(name)["pos4"], S["origin"], sc.sun(name), tau, 0.0, lights.shaft_fractions(8),
                                 sc.unit_dirs(name), 13.0)[0]
        assert np.linalg.norm(Fo.astype(np.float64), axis=-1).min() >= 2.0
    ends = np.array([[3.0, 0.0, 0.0], [np.nan, 0.0, 0.0]], F)
    assert float(lights.shaft_distance((0.0, 4.0, 0.0), ends)) == 7.0


def test_mask_packing():
    """The mask word of the samples' visibility bytes: masks_from_vis / vis_from_masks over all 64 bits."""
    rng = np.random.default_rng(7)
    vis = [np.where(rng.random((5, 7)) < 0.5, 255, 0).astype(np.uint8) for _ in range(64)]
    for n in (1, 33, 64):
        m = lights.masks_from_vis(vis[:n])
        assert m.dtype == np.uint64
        for i in range(n):
            assert np.array_equal(sc.bit(m, i), vis[i] != 0)
        if n < 64:
            assert (m >> np.uint64(n) == 0).all()
        assert (m <= sc.low(n)).all()
        back = lights.vis_from_masks(m, n)
        assert all(np.array_equal(back[i], vis[i]) for i in range(n))
    assert sc.low(64) == np.uint64(2 ** 64 - 1) and sc.low(8) == np.uint64(255)


def scalar_pixel(c, E, m, w, gain, col):
    """light_model_shafts' pixel in scalar float32 arithmetic."""
    if E[0] == 0 and E[1] == 0 and E[2] == 0:
        return list(c[:3])
    length = np.sqrt((E[0] * E[0] + E[1] * E[1]) + E[2] * E[2])
    S = F(0.0)
    for i in range(len(w)):
        S = S + (w[i] if (int(m) >> i) & 1 else F(0.0))
    t = (F(gain) * length) * S
    a = F(0.0) if np.isnan(t) else min(t, F(1.0))
    return [int(min((F(c[k]) + (F(col[k]) - F(c[k])) * a) + F(0.5), F(255.0))) for k in range(3)]


def test_light_model_shafts_properties():
    rng = np.random.default_rng(11)
    pos = frame("t1")["pos4"]
    D = sc.unit_dirs("t1")
    fr = lights.shaft_fractions(8)
    img = rng.integers(0, 256, pos.shape[:2] + (4,), dtype=np.uint8)
    mask = rng.integers(0, 256, pos.shape[:2], dtype=np.uint64)
    col = (255.0, 240.0, 200.0)
    w = (np.arange(8, dtype=F) + F(1.0)) / F(36.0)
    E = lights.shaft_ends(pos, D, 13.0)
    with np.errstate(all="ignore"):
        for weights, gain in ((None, 0.05), (w, 0.125), (w, 50.0)):
            out = lights.light_model_shafts(img, pos, mask, fr, weights, gain, col, D, 13.0)
            assert out.dtype == np.uint8 and np.array_equal(out[..., 3], img[..., 3])
            ww = np.full(8, F(1.0) / F(8), F) if weights is None else weights
            for y, x in ((0, 0), (5, 9), (17, 30), (18, 33), (35, 63), (20, 28)):
                assert list(out[y, x, :3]) == scalar_pixel(img[y, x], E[y, x], mask[y, x], ww, gain, col), (y, x)
            # every channel moves towards the colour, never past it
            lo = np.minimum(img[..., :3], np.array(col, F)).astype(F)
            hi = np.maximum(img[..., :3], np.array(col, F)).astype(F)
            assert (out[..., :3] >= np.floor(lo)).all() and (out[..., :3] <= np.ceil(hi)).all()
        assert (lights.light_model_shafts(img, pos, mask, fr, w, 50.0, col, D, 13.0)[mask != 0][:, :3]
                == np.array(col, np.uint8)).all()   # saturated
    # no lit sample, a zero gain: unchanged; misses are touched only where they were marched
    assert np.array_equal(lights.light_model_shafts(img, pos, np.zeros_like(mask), fr, w, 1.0, col, D, 13.0), img)
    assert np.array_equal(lights.light_model_shafts(img, pos, mask, fr, w, 0.0, col, D, 13.0), img)
    surf = sc.surface_of(pos)
    plain = lights.light_model_shafts(img, pos, mask, fr, w, 0.125, col)
    marched = lights.light_model_shafts(img, pos, mask, fr, w, 0.125, col, D, 13.0)
    assert np.array_equal(plain[~surf], img[~surf]) and np.array_equal(plain[surf], marched[surf])
    assert (marched[~surf] != img[~surf]).any()
    # a NaN blend factor (an infinite length, no lit sample) leaves the pixel; the sum runs in index order
    inf = np.zeros((1, 1, 4), F)
    inf[0, 0, 0] = 3e38
    px = np.array([[[10, 20, 30, 40]]], np.uint8)
    assert np.array_equal(lights.light_model_shafts(px, inf, np.zeros((1, 1), np.uint64), fr, w, 1.0, col), px)
    big = np.array([1.0, 2.0 ** -24, 2.0 ** -24], F)
    one = np.zeros((1, 1, 4), F)
    one[0, 0, 2] = 0.5
    up = lights.light_model_shafts(px, one, np.array([[7]], np.uint64), fr[:3], big, 1.0, col)
    down = lights.light_model_shafts(px, one, np.array([[7]], np.uint64), fr[:3], big[::-1], 1.0, col)
    assert list(up[0, 0, :3]) == scalar_pixel(px[0, 0], one[0, 0], 7, big, 1.0, col)
    assert list(down[0, 0, :3]) == scalar_pixel(px[0, 0], one[0, 0], 7, big[::-1], 1.0, col)
    for kw in ({"gain": -1.0}, {"gain": float("inf")}, {"gain": float("nan")}, {"colour": (256.0, 0.0, 0.0)},
               {"colour": (0.0, -1.0, 0.0)}, {"colour": (0.0, 0.0, float("nan"))}, {"weights": -w},
               {"weights": w[:3]}):
        with pytest.raises(ValueError):
            lights.light_model_shafts(img, pos, mask, fr, **kw)


@pytest.mark.parametrize("name", ["t1", "t3"])
def test_oracle_facts_of_the_parity_cases(name):
    """The conditions the GPU tests stand on (avx): each stated bit has both outcomes in quantity among the traced
    pixels, so a constant mask cannot pass; both biases."""
    fr = lights.shaft_fractions(8)
    for part, every, traced in sc.PARITY[name]:
        bits, count = sc.BOTH[(name, part)]
        assert count >= 20
        for bias in (0.0, su.B10):
            m, pick = sc.oracle_mask(name, fr, bias, "avx", every, part)
            print(name, part, bias, [sc.outcomes(m, pick, i) for i in range(8)])
            assert int(pick.sum()) == traced and (pick <= sc.part_of(name, part)).all()
            for i in bits:
                assert min(sc.outcomes(m, pick, i)) >= count, i
            assert (m >> np.uint64(8) == 0).all() and (m[~pick] == np.uint64(255)).all()
    # every traced ray starts outside the radius-2 ball
    S = pyoracle.load_setup(name)
    Fo = lights.shafts_model(frame(name)["pos4"], S["origin"], sc.sun(name), sc.CASES[name][1], 0.0, fr,
                             sc.dirs_of(name), sc.CASES[name][2])[0]
    assert np.linalg.norm(Fo.astype(np.float64), axis=-1).min() >= 2.0


def test_oracle_facts_of_the_64_sample_case():
    """t1, n = 64, every 8th surface pixel (104): bits 32..55 each have at least 20 pixels of either outcome (the
    minimum is 21), so a 32-bit shift cannot pass."""
    m, pick = sc.oracle_mask("t1", lights.shaft_fractions(64), su.B10, "avx", sc.ALL64_EVERY, "surface")
    assert int(pick.sum()) == 104
    least = [min(sc.outcomes(m, pick, i)) for i in range(64)]
    print(least)
    assert min(least[32:56]) >= 20


def test_header_declares_the_entries():
    text = " ".join(pathlib.Path(sf.HEADER_PATH).read_text().split())
    for sym in SYMBOLS + ("sf_shafts_params",):
        assert sym in text, sym
    assert "#define SF_SHAFT_SAMPLES_MAX 64" in text and sf.SF_SHAFT_SAMPLES_MAX == 64
    assert lights.SHAFT_SAMPLES_MAX == 64
    assert "Bit i of mask[p] is 1 iff sf_trace_sun_to with the same dir, distance, bias, origin and shadow LOD " \
           "constant writes 255 at a pixel whose position is Q_i" in text
    for consequence in ("A sample with sigma_i == 1 is the surface point itself", "tau >= 2 + max |o + E|",
                        "so a larger tau is coarser"):
        assert consequence in text, consequence
    assert "#define SF_ABI_VERSION 1" in text


def test_symbols_are_exported():
    L = sf.lib()
    for sym in SYMBOLS:
        assert sym in sf.SIGNATURES and getattr(L, sym) is not None, sym
    if shutil.which("nm") is None:
        return
    have = defined_symbols(sf.LIB_PATH)
    assert set(SYMBOLS) <= have


def test_struct_layout_matches_the_header():
    P = sf.sf_shafts_params
    assert ctypes.sizeof(P) == 104
    assert (P.dir.offset, P.distance.offset, P.bias.offset, P.fractions.offset, P.weights.offset) == (0, 12, 16, 24, 32)
    assert (P.n.offset, P.dirs.offset, P.dirs_stride.offset, P.far.offset, P.origin.offset) == (40, 48, 56, 60, 64)
    assert (P.use_origin.offset, P.width.offset, P.height.offset, P.max_depth.offset, P.stream.offset) \
        == (76, 80, 84, 88, 96)


def test_null_context_is_einval():
    L = sf.lib()
    p = sf.sf_shafts_params()
    buf = (ctypes.c_float * 64)(*([0.5] * 64))
    vp = ctypes.cast(buf, ctypes.c_void_p)
    p.fractions, p.n, p.distance = ctypes.cast(buf, ctypes.POINTER(ctypes.c_float)), 1, 4.0
    assert L.sf_shafts_defaults(None, ctypes.byref(p)) == sf.SF_EINVAL
    assert L.sf_trace_shafts_to(None, ctypes.byref(p), vp, vp) == sf.SF_EINVAL
    assert L.sf_trace_shafts(None, ctypes.byref(p)) == sf.SF_EINVAL
    assert L.sf_light_image_shafts(None, ctypes.byref(p), 0.25, buf, vp, vp, vp) == sf.SF_EINVAL
    assert p.n == 1   # (a refused sf_shafts_defaults wrote nothing)


def test_cpp_members_are_inline_over_the_c_abi(tmp_path):
    """Sphereflake::TraceShafts / LightImageShafts compile for an application, stay inline, and need only sf_* symbols
    the library has."""
    if shutil.which("g++") is None or shutil.which("nm") is None:
        pytest.skip("binutils / g++ not available")
    source = ('#include "Sphereflake.hpp"\n'
              "using namespace SphereflakeRaytracer;\n"
              "void light(Sphereflake& s, const float* pdev, const float* ddev, uint64_t* mdev) {\n"
              "    static const float fractions[2] = { 0.25f, 0.75f };\n"
              "    static const float colour[3] = { 255.0f, 240.0f, 200.0f };\n"
              "    sf_shafts_params p;\n"
              "    sf_shafts_defaults(s.Context(), &p);\n"
              "    p.fractions = fractions; p.n = 2;\n"
              "    p.dirs = ddev; p.dirs_stride = 3; p.far = 13.0f;\n"
              "    s.TraceShafts(p);\n"
              "    s.LightImageShafts(p, 0.05f, colour);\n"
              "    p.width = 64; p.height = 36;\n"
              "    s.TraceShafts(p, pdev, mdev);\n}\n")
    obj = compile_class_user(tmp_path, "shafts", source)
    need, have = undefined_symbols(obj), defined_symbols(sf.LIB_PATH)
    assert {"sf_trace_shafts_to", "sf_trace_shafts", "sf_light_image_shafts"} <= need
    assert not [n for n in need if "TraceShafts" in n or "LightImageShafts" in n]
    assert not [n for n in need if (n.startswith("sf_") or "SphereflakeRaytracer" in n) and n not in have]
