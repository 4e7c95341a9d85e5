"""Host side of ray tracing from caller-supplied origins (sf_trace_rays_to): what the definition stands on (the
root transform's columns), the seeded ray sets of the GPU tests on the oracle, the generators of
sphereflake_amd.rays, and the entry points' null-context answers. No GPU needed."""
import ctypes
import shutil

import numpy as np
import pytest

import sphereflake_amd as sf
from sphereflake_amd import dirs, rays
from abicheck import compile_class_user, defined_symbols, undefined_symbols
from dirscheck import FLT_MAX, same_bits
from oracle import pyoracle
import rayscheck


def test_root_columns_do_not_depend_on_the_origin():
    """Columns 0..2 of sf.root_transform(o) are the same bits for every finite origin, and column 3 is
    float32(0) - o: the origin enters the reference's ray through that column only (Sphereflake.cpp:83)."""
    origins = [np.asarray(pyoracle.load_setup(n)["origin"], np.float32) for n in ("t1", "t2", "t3", "t4")]
    rng = np.random.default_rng(5)
    origins += [v.astype(np.float32) for v in rng.normal(scale=4.0, size=(6, 3))]
    origins += [np.array([0.0, -0.0, 1e-30], np.float32), np.array([-3e5, 2.5, 0.0], np.float32)]
    base = sf.root_transform(origins[0]).reshape(16)
    for n in ("t1", "t2", "t3", "t4"):
        assert same_bits(np.asarray(pyoracle.load_setup(n)["root"], np.float32).reshape(16)[:12], base[:12])
    for o in origins:
        r = sf.root_transform(o).reshape(16)
        assert same_bits(r[:12], base[:12])
        assert same_bits(r[12:15], np.float32(0.0) - o)
        assert r[15] == 1.0


def counts(name):
    ref = rayscheck.set_oracle(name)
    hits = int((ref["minT"] < FLT_MAX).sum())
    n = ref["minT"].size
    print(name, "hits", hits, "misses", n - hits, "negative", int((ref["minT"] < 0).sum()), "depth",
          ref["stats"]["max_depth"])
    return ref, hits, n - hits


def test_ray_set_jitter():
    o, d = rayscheck.jitter()
    S = pyoracle.load_setup("t1")
    assert o.shape == d.shape == (64 * 36, 3) and o.dtype == d.dtype == np.float32
    assert np.linalg.norm(o.astype(np.float64) - np.asarray(S["origin"], np.float64), axis=1).max() < 0.5 + 1e-5
    _, hits, misses = counts("jitter")
    assert hits >= 400 and misses >= 400


def test_ray_set_reflect():
    ref, hits, misses = counts("reflect")
    assert ref["minT"].size == 1024
    assert hits >= 200 and misses >= 200
    assert 12 <= ref["stats"]["max_depth"] <= 20


def test_ray_set_towards_in():
    ref, hits, misses = counts("towards_in")
    assert ref["minT"].size == 1024
    assert hits >= 500 and misses >= 5
    assert (ref["minT"] < 0).any()
    assert 12 <= ref["stats"]["max_depth"] <= 20


def test_ray_set_towards_out_pins_the_quirk():
    """Feelers from the flake's surface towards a light outside it: every sphere's centre is behind the ray, the
    root's bounding ball included (tca >= 0, SIMD_AVX.h:247-258) -- the reference sees nothing."""
    ref, hits, _ = counts("towards_out")
    assert ref["minT"].size == 64
    assert hits == 0


def test_reflect_and_towards_geometry():
    pos, nrm, d, o = rayscheck._t3_hits()
    ro, rd, mask = rays.reflect(pos, nrm, o, d, 1e-3)
    assert ro.dtype == rd.dtype == np.float32 and ro.shape == rd.shape == (1024, 3) and mask.shape == (1024,)
    n = nrm[:, :3].astype(np.float64)
    dn = d.astype(np.float64)
    dn /= np.linalg.norm(dn, axis=1, keepdims=True)
    # the world hit point origin + pos (magnitude < 8: 2^-21 absolute in float32), offset by eps n; 1e-5 is 20x that
    assert np.abs(ro - (o.astype(np.float64) + pos[:, :3] + 1e-3 * n)).max() < 1e-5
    # a mirror: the reflected direction keeps the tangential part and flips the normal part; unit vectors stored
    # in float32 (2^-24 relative), the normals themselves unit to the rsqrt's 2^-22: 1e-5 is 40x that
    assert np.abs((rd * n).sum(1) + (dn * n).sum(1)).max() < 1e-5
    assert np.abs(np.cross(rd, n) - np.cross(dn, n)).max() < 1e-5
    assert not np.signbit(rd[rd == 0.0]).any()
    to, td, _ = rays.towards(pos, nrm, o, (0.0, 0.0, 3.0), 1e-3)
    assert same_bits(to, ro)
    assert same_bits(td, (np.array([0.0, 0.0, 3.0], np.float32) - to) + np.float32(0.0))
    # misses are masked out
    pos2, nrm2 = pos.copy(), nrm.copy()
    pos2[5], nrm2[5] = (0, 0, 0, 1), (0, 0, 0, 1)
    ro2, rd2, mask2 = rays.reflect(pos2, nrm2, o, d, 1e-3)
    assert not mask2[5] and mask2.sum() == 1023 and ro2.shape == (1023, 3)
    assert same_bits(ro2[5:], ro[6:]) and same_bits(rd2[:5], rd[:5])


def test_look_ahead_geometry():
    cam = sf.config_camera(64, 36, 0.5)
    steps, step = 3, 0.125
    o, d = rays.look_ahead(cam, steps, step)
    axes = dirs.move_axes(cam)
    assert o.dtype == d.dtype == np.float32 and o.shape == (6 * steps, 3) and d.shape == (36 * steps, 3)
    assert same_bits(d.reshape(6 * steps, 6, 3), np.broadcast_to(axes, (6 * steps, 6, 3)))
    p = cam.GetPosition()
    for a in range(6):
        for k in range(1, steps + 1):
            # float32: position + axis * (k step); k step is exact here (a power of two times a small integer)
            assert same_bits(o[a * steps + k - 1], p + axes[a] * np.float32(k * step))
    with pytest.raises(ValueError):
        rays.look_ahead(cam, 0, step)


def test_null_context_is_einval():
    L = sf.lib()
    p = sf.sf_rays_params(4, 1, 3, 3, 1, 0, None)
    buf = (ctypes.c_float * 64)()
    vp = ctypes.cast(buf, ctypes.c_void_p)
    assert L.sf_trace_rays_to(None, ctypes.byref(p), vp, vp, vp, vp, None, None) == sf.SF_EINVAL
    assert L.sf_probe_rays(None, vp, vp, 4, 1, vp, None, None, None) == sf.SF_EINVAL


def test_cpp_members_are_inline_over_the_c_abi(tmp_path):
    """Sphereflake::TraceRays / ProbeRays compile for an application, stay inline (no new exported class member),
    and need only sf_* symbols the library has."""
    if shutil.which("g++") is None or shutil.which("nm") is None:
        pytest.skip("binutils / g++ not available")
    source = ('#include "Sphereflake.hpp"\n'
              "using namespace SphereflakeRaytracer;\n"
              "float brake(Sphereflake& s, const float* org, const float* axes, const float* odev,\n"
              "            const float* ddev, float* pdev, sf_vec4* pos) {\n"
              "    float t[36]; uint32_t idx[36];\n"
              "    s.ProbeRays(org, axes, 36, 6, t, idx, pos);\n"
              "    sf_rays_params p = {}; p.width = 64; p.height = 1; p.dir_stride = 3; p.origin_stride = 4;\n"
              "    p.rays_per_origin = 8;\n"
              "    s.TraceRays(p, odev, ddev, pdev, nullptr);\n"
              "    return t[0];\n}\n")
    obj = compile_class_user(tmp_path, "probe", source)
    need, have = undefined_symbols(obj), defined_symbols(sf.LIB_PATH)
    assert {"sf_probe_rays", "sf_trace_rays_to"} <= need
    assert not [n for n in need if "TraceRays" in n or "ProbeRays" in n]
    assert not [n for n in need if (n.startswith("sf_") or "SphereflakeRaytracer" in n) and n not in have]
