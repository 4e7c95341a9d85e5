"""CPU: the host statement of the colour light buffer (sphereflake_amd.lights.sum_model, light_model_buffer,
sky_colours; sf_trace_suns_sum_to / sf_trace_shadows_sum_to / sf_light_image_buffer in sf.h), its header and its
exports. The GPU side is tests/test_gpu_light_sum.py."""
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
from lightsumcheck import CONE_COLOURS, pack
import shadowcheck as sc
import suncheck as su
import sunscheck as ss

F = np.float32
SYMBOLS = ("sf_light_sum_defaults", "sf_trace_suns_sum_to", "sf_trace_suns_sum", "sf_trace_shadows_sum_to",
           "sf_trace_shadows_sum", "sf_light_fill", "sf_light_buffer", "sf_download_light", "sf_light_image_buffer")


@pytest.fixture(scope="module", autouse=True)
def built():
    sf.build()
    return sf.lib()


def synthetic(n, shape=(6, 7), seed=3):
    """A small frame with two misses, unit normals, n entries, random chunk masks and per-entry colours whose float
    sums depend on the order (magnitudes from 2^-12 to 1)."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-1.0, 1.0, shape + (4,)).astype(F)
    pos[0, 0, :3] = 0.0
    pos[3, 4, :3] = 0.0
    nrm = rng.normal(size=shape + (4,)).astype(F)
    nrm[..., :3] /= np.linalg.norm(nrm[..., :3], axis=-1, keepdims=True)
    pts = rng.normal(size=(n, 3)).astype(F)
    pts /= np.linalg.norm(pts, axis=-1, keepdims=True)
    col = (rng.uniform(0.5, 1.0, (n, 3)) * 2.0 ** rng.integers(-12, 1, (n, 1))).astype(F)
    masks = [rng.integers(0, 2 ** 63, shape, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, shape, dtype=np.uint64)
             for _ in range((n + 63) // 64)]
    base = rng.uniform(0.0, 1.0, shape + (4,)).astype(F)
    return pos, nrm, pts, col, masks, base


@pytest.mark.parametrize("kind", ["suns", "shadows"])
@pytest.mark.parametrize("k", [1, 63, 64, 65])
def test_split_invariance(kind, k):
    """n entries at once equal the first k overwriting, then the rest accumulating -- with the second call's masks
    re-chunked from its own entry 0, as a second device call would produce them."""
    n = 150
    pos, nrm, pts, col, masks, base = synthetic(n)
    bits = np.stack([ss.bit(masks[i // 64], i % 64) for i in range(n)])
    o = (0.25, -0.5, 0.125)
    for start in (None, base):
        whole = lights.sum_model(start, pos, nrm, masks, pts, col, kind, o)
        first = lights.sum_model(start, pos, nrm, pack(bits[:k]), pts[:k], col[:k], kind, o)
        both = lights.sum_model(first, pos, nrm, pack(bits[k:]), pts[k:], col[k:], kind, o)
        assert same_bits(whole, both), (kind, k, start is None)


def test_the_order_is_pinned():
    """Reversing the entries (and their bits) changes some float sum: an implementation that sums in another order
    cannot equal the model."""
    n = 100
    pos, nrm, pts, col, masks, _ = synthetic(n)
    rev = pack(np.stack([ss.bit(masks[i // 64], i % 64) for i in range(n)])[::-1])
    a = lights.sum_model(None, pos, nrm, masks, pts, col)
    b = lights.sum_model(None, pos, nrm, rev, pts[::-1], col[::-1])
    assert np.allclose(a, b, rtol=1e-5, atol=1e-7)
    assert int((a.view(np.uint32) != b.view(np.uint32)).sum()) >= 10


def test_misses_and_w():
    pos, nrm, pts, col, masks, base = synthetic(70)
    miss = np.zeros(pos.shape[:2], bool)
    miss[0, 0] = miss[3, 4] = True
    over = lights.sum_model(None, pos, nrm, masks, pts, col)
    assert over.dtype == F and over.shape == pos.shape
    assert (over[miss] == 0).all() and (over[..., 3] == 0).all()
    assert (over[~miss][:, :3] > 0).any()
    acc = lights.sum_model(base, pos, nrm, masks, pts, col)
    assert same_bits(acc[miss], base[miss]) and same_bits(acc[..., 3], base[..., 3])
    assert (acc[~miss][:, :3] >= base[~miss][:, :3]).all() and (acc[~miss][:, :3] > base[~miss][:, :3]).any()
    assert same_bits(base, synthetic(70)[5])   # the base was not changed in place
    # colours None: float32(1) / float32(n) per component
    even = lights.sum_model(None, pos, nrm, masks, pts, None)
    assert same_bits(even, lights.sum_model(None, pos, nrm, masks, pts, np.full((70, 3), F(1.0) / F(70.0), F)))
    for bad in (dict(colours=-col), dict(colours=col[:5]), dict(kind="moon")):
        with pytest.raises(ValueError):
            lights.sum_model(None, pos, nrm, masks, pts, **{"colours": col, **bad})
    with pytest.raises(ValueError):
        lights.sum_model(None, pos, nrm, masks[:1], pts, col)


def grey_image(shape):
    rng = np.random.default_rng(11)
    return rng.integers(0, 256, shape + (4,), dtype=np.uint8)


def test_grey_suns_equal_light_model_suns():
    """Ambient 0, colours (w, w, w): the resolve of the sum is light_model_suns' image, byte for byte, on t1's oracle
    frame under the oracle's cone mask."""
    ref = frame("t1")
    D = ss.cone("t1")
    mask, _ = ss.oracle_mask("t1", D)
    w = (np.arange(8, dtype=F) + F(1.0)) / F(40.0)
    img = grey_image(mask.shape)
    for weights in (None, w):
        col = None if weights is None else np.repeat(weights[:, None], 3, axis=1)
        buf = lights.sum_model(None, ref["pos4"], ref["nrm4"], [mask], D, col, "suns")
        got = lights.light_model_buffer(img, ref["pos4"], buf)
        want = lights.light_model_suns(img, ref["pos4"], ref["nrm4"], mask, D, weights, ambient=0.0)
        assert np.array_equal(got, want)
        assert (got != img).any()


def test_grey_lights_equal_light_model_many():
    ref = frame("t1")
    S = pyoracle.load_setup("t1")
    names = ("side", "low")
    L = np.array([sc.LIGHTS[n] for n in names], F)
    mask = lights.masks_from_vis([sc.oracle_vis("t1", n, 2.0 ** -9) for n in names])
    img = grey_image(mask.shape)
    w = np.array([0.75, 0.5], F)
    buf = lights.sum_model(None, ref["pos4"], ref["nrm4"], [mask], L, np.repeat(w[:, None], 3, axis=1), "shadows",
                           S["origin"])
    got = lights.light_model_buffer(img, ref["pos4"], buf)
    want = lights.light_model_many(img, ref["pos4"], ref["nrm4"], mask, S["origin"], L, w, ambient=0.0)
    assert np.array_equal(got, want) and (got != img).any()
    assert np.array_equal(got[..., 3], img[..., 3])
    surf = ref["minT"] < su.FLT_MAX
    assert np.array_equal(got[~surf], img[~surf])   # a miss of the frame stays


def test_sky_colours():
    for n in (1, 16, 256):
        D = lights.sky_dirs(n, limit=lights.SUM_MAX)
        C = lights.sky_colours(D, zenith=(0.25, 0.5, 1.0), horizon=(1.0, 0.75, 0.5))
        assert C.shape == (n, 3) and C.dtype == F and (C >= 0).all()
        z = D.astype(np.float64)[:, 2]
        want = (np.array((1.0, 0.75, 0.5)) + (np.array((0.25, 0.5, 1.0)) - np.array((1.0, 0.75, 0.5))) * z[:, None]) / n
        assert np.allclose(C, want, rtol=1e-6, atol=0)
    # the two ends of the gradient, and the 1 / n scale
    ends = lights.sky_colours(np.array([(0, 0, 1), (1, 0, 0), (0, 3, 0), (0, 0, -1)], F), (0.25, 0.5, 1.0), (1.0, 0.75, 0.5))
    assert np.array_equal(ends[0], np.array((0.25, 0.5, 1.0), F) / F(4.0))
    for i in (1, 2, 3):   # (below the horizon clamps to the horizon colour)
        assert np.array_equal(ends[i], np.array((1.0, 0.75, 0.5), F) / F(4.0))
    up = lights.sky_colours(np.array([(0, 1, 0)], F), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), up=(0, 2, 0))
    assert np.array_equal(up, np.array([(0.0, 0.0, 1.0)], F))
    for bad in (np.zeros((1, 3), F), np.array([(np.nan, 0, 1)], F)):
        with pytest.raises(ValueError):
            lights.sky_colours(bad)
    with pytest.raises(ValueError):
        lights.sky_colours(np.ones((2, 3), F), zenith=(-1.0, 0.0, 0.0))


def test_generators_take_a_limit():
    assert lights.sky_dirs(129, limit=lights.SUM_MAX).shape == (129, 3)
    assert same_bits(lights.sky_dirs(64, limit=lights.SUM_MAX), lights.sky_dirs(64))
    assert lights.sky(100, limit=lights.SUM_MAX).shape == (100, 3)
    assert lights.sun_cone((0, 0, 1), 0.1, 70, limit=128).shape == (70, 3)
    assert lights.disc((3, 0, 1), 0.25, 70, limit=128).shape == (70, 3)
    with pytest.raises(ValueError):
        lights.sky_dirs(129, limit=128)
    assert lights.SUM_MAX == sf.SF_LIGHT_SUM_MAX == 65536


def test_the_oracle_sample_is_coloured():
    """t1's cone under per-direction colours: at least 100 pixels of the summed buffer have three channels that are
    not all equal, and at least 100 differ from the buffer with every direction lit -- a device buffer that ignores
    colour or visibility cannot equal it."""
    ref = frame("t1")
    D = ss.cone("t1")
    mask, pick = ss.oracle_mask("t1", D)
    col = CONE_COLOURS
    buf = lights.sum_model(None, ref["pos4"], ref["nrm4"], [mask], D, col)
    rgb = buf[pick][:, :3]
    assert int(((rgb[:, 0] != rgb[:, 1]) | (rgb[:, 1] != rgb[:, 2])).sum()) >= 100
    lit = lights.sum_model(None, ref["pos4"], ref["nrm4"], [np.full(mask.shape, 255, np.uint64)], D, col)
    assert int((buf[pick] != lit[pick]).any(axis=-1).sum()) >= 100


def test_header_and_abi():
    text = " ".join(pathlib.Path(sf.HEADER_PATH).read_text().split())
    for sym in SYMBOLS + ("sf_light_sum_params",):
        assert sym in text, sym
    assert "#define SF_LIGHT_SUM_MAX 65536" in text
    assert "DEFINITION OF THE SUM (exact; binary32, round to nearest" in text
    assert "#define SF_ABI_VERSION 1" in text
    assert sf.lib().sf_abi_version() == 1
    assert set(SYMBOLS) <= set(sf.SIGNATURES)
    L = sf.lib()
    for sym in SYMBOLS:
        assert getattr(L, sym) is not None, sym
    if shutil.which("nm") is not None:
        assert set(SYMBOLS) <= defined_symbols(sf.LIB_PATH)


def test_struct_layout_matches_the_header():
    P = sf.sf_light_sum_params
    assert ctypes.sizeof(P) == 72
    assert (P.points.offset, P.colours.offset, P.n.offset, P.accumulate.offset) == (0, 8, 16, 20)
    assert (P.distance.offset, P.bias.offset, P.origin.offset, P.use_origin.offset) == (24, 28, 32, 44)
    assert (P.width.offset, P.height.offset, P.max_depth.offset, P.stream.offset) == (48, 52, 56, 64)


def test_null_context_is_einval():
    L = sf.lib()
    p = sf.sf_light_sum_params()
    buf = (ctypes.c_float * 64)()
    vp = ctypes.cast(buf, ctypes.c_void_p)
    p.points, p.n, p.distance = ctypes.cast(buf, ctypes.POINTER(ctypes.c_float)), 1, 4.0
    assert L.sf_light_sum_defaults(None, ctypes.byref(p)) == sf.SF_EINVAL
    assert p.n == 1   # (a refused sf_light_sum_defaults wrote nothing)
    for name in ("sf_trace_suns_sum", "sf_trace_shadows_sum"):
        assert getattr(L, name + "_to")(None, ctypes.byref(p), vp, vp, vp) == sf.SF_EINVAL
        assert getattr(L, name)(None, ctypes.byref(p)) == sf.SF_EINVAL
    assert L.sf_light_fill(None, ctypes.cast(buf, ctypes.POINTER(ctypes.c_float)), vp, None) == sf.SF_EINVAL
    assert L.sf_light_buffer(None, ctypes.byref(ctypes.c_void_p())) == sf.SF_EINVAL
    assert L.sf_download_light(None, vp) == sf.SF_EINVAL
    assert L.sf_light_image_buffer(None, None, vp, vp, vp) == sf.SF_EINVAL


def test_cpp_members_are_inline_over_the_c_abi(tmp_path):
    """Sphereflake::TraceSunsSum / TraceShadowsSum / LightFill / LightImageBuffer compile for an application, stay
    inline, and need only sf_* symbols the library has."""
    if shutil.which("g++") is None or shutil.which("nm") is None:
        pytest.skip("binutils / g++ not available")
    source = ('#include "Sphereflake.hpp"\n'
              "using namespace SphereflakeRaytracer;\n"
              "void light(Sphereflake& s, const float* pdev, const float* ndev, float* ldev) {\n"
              "    static const float dirs[6] = { 0.6f, 0.0f, 0.8f, 0.0f, 0.6f, 0.8f };\n"
              "    static const float amb[3] = { 0.1f, 0.1f, 0.2f };\n"
              "    sf_light_sum_params p;\n"
              "    sf_light_sum_defaults(s.Context(), &p);\n"
              "    p.points = dirs; p.n = 2; p.accumulate = 1;\n"
              "    s.LightFill(amb);\n"
              "    s.TraceSunsSum(p);\n"
              "    s.TraceShadowsSum(p);\n"
              "    s.LightImageBuffer();\n"
              "    p.width = 64; p.height = 36;\n"
              "    s.TraceSunsSum(p, pdev, ndev, ldev);\n"
              "    s.TraceShadowsSum(p, pdev, ndev, ldev);\n}\n")
    obj = compile_class_user(tmp_path, "sum", source)
    need, have = undefined_symbols(obj), defined_symbols(sf.LIB_PATH)
    assert {"sf_trace_suns_sum_to", "sf_trace_suns_sum", "sf_trace_shadows_sum_to", "sf_trace_shadows_sum",
            "sf_light_fill", "sf_light_image_buffer"} <= need
    assert not [n for n in need if "Sum" in n or "LightFill" in n or "LightImageBuffer" in n]
    assert not [n for n in need if (n.startswith("sf_") or "SphereflakeRaytracer" in n) and n not in have]
