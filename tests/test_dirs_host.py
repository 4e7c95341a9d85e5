"""Host side of direction tracing (sf_trace_dirs_to): the direction generators of sphereflake_amd.dirs against
the oracle and against their own geometry, and the entry points' null-context answers. No GPU needed."""
import ctypes
import shutil

import numpy as np
import pytest

import sphereflake_amd as sf
from sphereflake_amd import dirs
from abicheck import compile_class_user, defined_symbols, undefined_symbols
from dirscheck import oracle_rays, same_bits
from oracle import pyoracle


@pytest.mark.parametrize("name", ["t1", "t2", "t3", "t4"])
def test_pinhole_is_the_frames_ray_generation(name):
    """dirs.pinhole gives the frame's own pre-normalised pixel vectors: traced one ray at a time (a 1 x 1 oracle
    frame whose corners are the vector), 200 seeded pixels get the bits the oracle's frame gives them."""
    S = pyoracle.load_setup(name)
    W, H = S["W"], S["H"]
    d = dirs.pinhole(S["origin"], S["tl"], S["tr"], S["bl"], W, H)
    assert d.dtype == np.float32 and d.shape == (H, W, 3) and d.flags.c_contiguous
    frame = pyoracle.render(S)
    rng = np.random.default_rng(20 + int(name[1]))
    pix = rng.choice(W * H, size=min(200, W * H), replace=False)
    y, x = pix // W, pix % W
    one = oracle_rays(S["root"], S["children"], d[y, x])
    assert one["stats"]["hits"] > 0
    for k in ("pos4", "nrm4", "minT", "index"):
        assert same_bits(one[k], frame[k][y, x]), (name, k)


def test_equirect_geometry():
    W, H = 64, 32
    f = np.array([0.3, -0.5, 0.8])
    up = np.array([0.1, 1.0, 0.2])
    d = dirs.equirect(W, H, f, up)
    assert d.dtype == np.float32 and d.shape == (H, W, 3)
    assert np.isfinite(d).all()
    assert not np.signbit(d[d == 0.0]).any()
    fu = f / np.linalg.norm(f)
    uu = up - fu * np.dot(up, fu)
    uu /= np.linalg.norm(uu)
    # float32 storage of unit vectors computed in float64: 2^-24 relative per component, 1e-6 is 16x that
    tol = 1e-6
    assert np.abs(np.linalg.norm(d.astype(np.float64), axis=-1) - 1.0).max() < tol
    assert np.abs(d[H // 2, W // 2] - fu).max() < tol            # the centre looks along forward
    assert np.abs(d[H // 2, 0] + fu).max() < tol                 # the left edge looks backwards
    # ... and so does the right edge, one pixel (2 pi / W of longitude) short of it
    assert np.arccos(np.clip(np.dot(d[H // 2, W - 1], -fu), -1, 1)) < 2 * np.pi / W + tol
    assert np.abs(d[0] - uu).max() < tol                         # the top row points along up
    # longitude grows to the right of forward (right = forward x up), latitude falls down the image
    r = np.cross(fu, uu)
    assert np.dot(d[H // 2, W // 2 + 1], r) > 0 and np.dot(d[H // 2 + 1, W // 2], uu) < 0


def _glm_basis(yaw, pitch, roll):
    """Columns of the rotation of glm::quat(vec3(yaw, pitch, roll)) (camera.h:65-68), in float64."""
    e = np.array([yaw, pitch, roll], np.float64) * 0.5
    c, s = np.cos(e), np.sin(e)
    w = c[0] * c[1] * c[2] + s[0] * s[1] * s[2]
    x = s[0] * c[1] * c[2] - c[0] * s[1] * s[2]
    y = c[0] * s[1] * c[2] + s[0] * c[1] * s[2]
    z = c[0] * c[1] * s[2] - s[0] * s[1] * c[2]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


@pytest.mark.parametrize("angles", [(sf.DEFAULT_YAW, sf.DEFAULT_PITCH, 0.0), (0.3, -0.2, 0.25), (-2.0, 1.1, -0.4)])
def test_move_axes_are_the_cameras_basis(angles):
    """+- orientation * x, z, y in the key order of main.cpp:214-242 (D, A, S, W, Q, E)."""
    yaw, pitch, roll = angles
    cam = sf.config_camera(64, 36, 0.5)
    cam.SetYaw(np.float32(yaw))
    cam.SetPitch(np.float32(pitch))
    cam.SetRoll(np.float32(roll))
    m = dirs.move_axes(cam)
    assert m.dtype == np.float32 and m.shape == (6, 3)
    R = _glm_basis(float(np.float32(yaw)), float(np.float32(pitch)), float(np.float32(roll)))
    want = np.stack([R[:, 0], -R[:, 0], R[:, 2], -R[:, 2], R[:, 1], -R[:, 1]])
    # the corners are float32 sums of a position of magnitude ~5 and an offset of magnitude ~1: differences of
    # corners carry ~5 x 2^-23 = 6e-7 absolute error on lengths of ~1; 2e-5 is 30x that
    assert np.abs(m - want).max() < 2e-5
    assert np.array_equal(m[0::2], -m[1::2])


def test_cpp_members_are_inline_over_the_c_abi(tmp_path):
    """Sphereflake::TraceDirections / ProbeDirections compile for an application, stay inline (no new exported
    class member to keep in step with the application's vector types), and need only sf_* symbols the library has."""
    if shutil.which("g++") is None or shutil.which("nm") is None:
        pytest.skip("binutils / g++ not available")
    source = ('#include "Sphereflake.hpp"\n'
              "using namespace SphereflakeRaytracer;\n"
              "float brake(Sphereflake& s, const float* axes6, const float* ddev, float* pdev, sf_vec4* pos) {\n"
              "    float t[6]; uint32_t idx[6];\n"
              "    s.ProbeDirections(axes6, 6, t, idx, pos);\n"
              "    sf_dirs_params p = {}; p.width = 64; p.height = 1; p.stride = 3;\n"
              "    s.TraceDirections(p, ddev, pdev, nullptr);\n"
              "    p.width = (uint32_t)s.Width(); p.height = (uint32_t)s.Height();\n"
              "    s.TraceDirections(p, ddev);\n"
              "    return t[0];\n}\n")
    obj = compile_class_user(tmp_path, "probe", source)
    need, have = undefined_symbols(obj), defined_symbols(sf.LIB_PATH)
    assert {"sf_probe_dirs", "sf_trace_dirs_to", "sf_trace_dirs"} <= need
    assert not [n for n in need if "TraceDirections" in n or "ProbeDirections" in n]
    assert not [n for n in need if (n.startswith("sf_") or "SphereflakeRaytracer" in n) and n not in have]


def test_null_context_is_einval():
    L = sf.lib()
    p = sf.sf_dirs_params(4, 1, 3, 0, None)
    buf = (ctypes.c_float * 64)()
    vp = ctypes.cast(buf, ctypes.c_void_p)
    assert L.sf_trace_dirs_to(None, ctypes.byref(p), vp, vp, vp, None, None) == sf.SF_EINVAL
    assert L.sf_trace_dirs(None, ctypes.byref(p), vp) == sf.SF_EINVAL
    assert L.sf_probe_dirs(None, vp, 4, vp, None, None, None) == sf.SF_EINVAL
