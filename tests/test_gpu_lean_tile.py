"""GPU tests of the lean tile loop (sf_kernels.hip: trace_queue_body<LEAN>, kernel sf_trace_queue1) against the general
one (sf_trace_queue1g, forced by SF_LEAN=0) and the oracle, and of what came with it: the wave's cone maximum by DPP
row operations (wave_max_pos) and the root's LOD decided like a child's (traverse_ray).

The host takes the lean loop exactly when a launch asks for nothing it leaves out: no aux channels, no part units in
the unit order, no tile costs recorded. At these small frame sizes the default schedule is the heavy-first order with
split tiles, which records costs every render, so beside the default the cases run under
  rowmajor: SF_ORDER=0 -- every render takes the lean loop, row-major units
  ordered:  SF_ORDER=1 SF_SPLIT_BUCKETS=0 SF_ORDER_RECORD=0 -- the 1080p product launch's schedule: the render that
            rebuilds the order records costs (general loop), the renders after it read the ordered units with their
            priority levels in the lean loop
and assert from sf_lean_launches which loop ran."""
import functools

import numpy as np
import pytest

from conftest import load_frame
from sfcheck import bad_rows, frame_digest, row_digests

pytestmark = pytest.mark.gpu

import sphereflake_amd as sf  # noqa: E402
from test_gpu_depth_seed import CATCH, camera_view, seeded_view  # noqa: E402

SCHEDULES = {
    "default": {},
    "rowmajor": {"SF_ORDER": "0"},
    "ordered": {"SF_ORDER": "1", "SF_SPLIT_BUCKETS": "0", "SF_ORDER_RECORD": "0"},
}
MISS = np.array([0.0, 0.0, 0.0, 1.0], np.float32)


@pytest.fixture(scope="module", autouse=True)
def device():
    sf.build()
    assert sf.device_count() >= 1, "no HIP device visible: GPU tests must run on an MI355X"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def away_camera(w, h):
    """The config camera turned half a turn about its yaw axis: no ray meets the root's bounding sphere."""
    cam = sf.config_camera(w, h, 1.0)
    cam.SetYaw(np.float32(sf.DEFAULT_YAW + np.pi))
    return cam


FAR_W, FAR_H, FAR_HALF = 64, 64, 2.2   # the far view's frame, and half its extent at the flake (units)


def far_view():
    """A view from T_0 + 1.9 r_0 away (T_0 = 4900 r_0: the root's LOD threshold), the image plane through the flake's
    centre: the bounding sphere's near root t = tca - sqrt(4 r^2 - d^2) lies between T_0 - 0.1 r_0 and T_0 + 1.9 r_0,
    on both sides of the threshold and inside the band where neither tca < T nor tca (1 - 2^-8) >= Tfar decides."""
    r0, t0 = sf.depth_constants(0)
    c = sf.root_transform(np.zeros(3, np.float32))[12:15].astype(np.float64)
    f = -np.asarray(sf.DEFAULT_CAMERA_POSITION, np.float64)
    f /= np.linalg.norm(f)
    right = np.cross(f, [0.0, 0.0, 1.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, f)
    o = c - f * (t0 + 1.9 * r0)
    s = FAR_HALF * r0
    tl, tr, bl = c + s * (up - right), c + s * (up + right), c + s * (-up - right)
    view = tuple(np.asarray(v, np.float32) for v in (o, tl, tr, bl))
    setup = {"W": FAR_W, "H": FAR_H, "origin": view[0], "tl": view[1], "tr": view[2], "bl": view[3],
             "root": sf.root_transform(view[0]), "children": sf.child_transforms()}
    return view, setup


def far_root_counts():
    """(rays that expand the root, rays that hit its bounding sphere and fail its LOD) in the oracle's frame of the far
    view. The oracle counts the nodes expanded (`interior`); at this distance no child passes its LOD (T_1 = T_0 / 3),
    so that is the root's expansions. With the LOD constant 71 instead of 70 (T_0 = 5041 r_0, beyond every bounding
    hit here; T_1 still far too small) every ray that hits the root's bounding sphere expands it: the difference is
    the rays whose bounding hit fails the root's LOD. (In float32 d^2 = |c|^2 - tca^2 cancels to within a few units
    at |c| = 4900, so which rays hit the bounding sphere is the reference's own arithmetic, not geometry.)"""
    from oracle import pyoracle
    _, setup = far_view()
    wide = pyoracle.render(setup, threads=8, lod=71.0)["stats"]
    ref = reference(("far", None))[2]["stats"]
    assert wide["max_depth"] == 0 and ref["max_depth"] == 0
    return ref["interior"], wide["interior"] - ref["interior"]


@functools.lru_cache(maxsize=None)
def reference(key):
    """(view, (W, H), oracle frame), computed once and read-only: ("seed", k): seeded_view(k) of
    test_gpu_depth_seed.py at 256 x 144; ("config", (w, h)): the config camera at w x h; ("away", (w, h)): the same
    looking away from the flake; ("far", None): far_view()."""
    from oracle import pyoracle
    kind, v = key
    if kind == "seed":
        view, setup, _ = seeded_view(v)
    elif kind == "config":
        view, setup = camera_view(sf.config_camera(v[0], v[1], 1.0))
    elif kind == "away":
        view, setup = camera_view(away_camera(*v))
    else:
        view, setup = far_view()
    ref = pyoracle.render(setup, threads=8)
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return view, (setup["W"], setup["H"]), ref


def render_frames(view, size, env, monkeypatch, n, lean=None):
    """n renders after a reset (no aux channels: the launch the lean loop serves) in a fresh context under `env`
    (and SF_LEAN=`lean` where given): [((pos, nrm), stats)], and how many launches took the lean loop."""
    for k in SCHEDULES["rowmajor"].keys() | SCHEDULES["ordered"].keys() | {"SF_LEAN", "SF_FLAGS"}:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if lean is not None:
        monkeypatch.setenv("SF_LEAN", lean)
    frames = []
    with sf.Sphereflake(*size) as s:
        s.SetView(*view)
        s.reset_stats()
        for _ in range(n):
            s.Render()
            pos, nrm, _, _ = s.download()
            frames.append(((pos, nrm), s.stats()))
        return frames, s.lean_launches()


def assert_oracle(got, st, ref, what):
    pos, nrm = got
    assert np.array_equal(bits(pos), bits(ref["pos4"])), what
    assert np.array_equal(bits(nrm), bits(ref["nrm4"])), what
    assert st.max_depth == ref["stats"]["max_depth"], what
    assert np.float32(st.closest) == np.float32(ref["stats"]["closest"]), what
    assert st.overflow_tiles == 0, what


def assert_golden(fx, got, st, what):
    pos, nrm = got
    assert bad_rows(fx["row_digest_gbuf"], row_digests(pos, nrm)) == [], what
    assert frame_digest(pos, nrm) == fx["frame_digest"], what
    assert st.max_depth == fx["stats"]["max_depth"], what
    assert np.float32(st.closest) == np.float32(float.fromhex(fx["stats"]["closest"])), what
    assert st.overflow_tiles == 0, what


def lean_and_general(view, size, schedule, monkeypatch):
    """The default (lean where the launch allows) and SF_LEAN=0 under one schedule: the frames of both after asserting
    that they agree bit for bit and in max_depth, closest, rays and overflow_tiles, render by render, and that the loop
    that ran is the one the schedule calls for."""
    n = 3 if schedule == "ordered" else 2   # (the render after the reset, and the next; ordered: the rebuild first)
    general, ng = render_frames(view, size, SCHEDULES[schedule], monkeypatch, n, lean="0")
    lean, nl = render_frames(view, size, SCHEDULES[schedule], monkeypatch, n)
    assert ng == 0, schedule
    if schedule == "rowmajor":
        assert nl == n
    elif schedule == "ordered":
        assert nl == n - 1   # (every render but the one that rebuilds the order)
    for k, ((a, sa), (b, sb)) in enumerate(zip(general, lean)):
        for x, y in zip(a, b):
            assert np.array_equal(bits(x), bits(y)), (schedule, k)
        assert (sa.max_depth, sa.closest, sa.rays, sa.overflow_tiles) == \
               (sb.max_depth, sb.closest, sb.rays, sb.overflow_tiles), (schedule, k)
        assert sb.rays == (k + 1) * size[0] * size[1], (schedule, k)
    return lean


@pytest.mark.parametrize("schedule", list(SCHEDULES))
def test_lean_equals_general_c1_golden(schedule, monkeypatch):
    """c1 (640 x 360): the default against SF_LEAN=0, and the golden digests."""
    fx = load_frame("c1")
    view, _ = camera_view(sf.config_camera(fx["W"], fx["H"], float.fromhex(fx["K"])))
    for k, (got, st) in enumerate(lean_and_general(view, (fx["W"], fx["H"]), schedule, monkeypatch)):
        assert_golden(fx, got, st, (schedule, k))


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("seed", CATCH)
def test_lean_equals_general_occluded_deepest_node(seed, schedule, monkeypatch):
    """The seeded 256 x 144 views whose deepest node is occluded: the default against SF_LEAN=0, and the oracle."""
    view, size, ref = reference(("seed", seed))
    for k, (got, st) in enumerate(lean_and_general(view, size, schedule, monkeypatch)):
        assert_oracle(got, st, ref, (seed, schedule, k))


@pytest.mark.parametrize("schedule", ["rowmajor", "ordered"])
def test_edge_tiles_70x44(schedule, monkeypatch):
    """70 x 44: neither side is a multiple of 8, so the edge tiles have invalid lanes in x and in y, which take part
    in the cone maximum."""
    view, size, ref = reference(("config", (70, 44)))
    for k, (got, st) in enumerate(lean_and_general(view, size, schedule, monkeypatch)):
        assert_oracle(got, st, ref, (schedule, k))


def test_view_away_from_the_flake(monkeypatch):
    """Every tile leaves at the root: every pixel is (0, 0, 0, 1), max_depth is the oracle's, the rays are counted."""
    view, size, ref = reference(("away", (136, 72)))
    assert ref["stats"]["hits"] == 0
    frames, n = render_frames(view, size, SCHEDULES["rowmajor"], monkeypatch, 2)
    assert n == 2
    for k, ((pos, nrm), st) in enumerate(frames):
        assert np.array_equal(bits(pos), bits(np.broadcast_to(MISS, pos.shape))), k
        assert np.array_equal(bits(nrm), bits(np.broadcast_to(MISS, nrm.shape))), k
        assert_oracle((pos, nrm), st, ref, k)
        assert st.rays == (k + 1) * size[0] * size[1]


@pytest.mark.parametrize("schedule", ["rowmajor", "ordered"])
def test_far_view_straddles_root_lod(schedule, monkeypatch):
    """About 4 900 units away, narrow field of view: some rays that hit the root's bounding sphere pass the root's LOD
    and some fail it, both counted from the oracle's output (far_root_counts)."""
    view, size, ref = reference(("far", None))
    passed, failed = far_root_counts()
    print(f"far view: {passed} rays expand the root, {failed} hit its bounding sphere and fail its LOD")
    assert passed > 0 and failed > 0
    for k, (got, st) in enumerate(lean_and_general(view, size, schedule, monkeypatch)):
        assert_oracle(got, st, ref, (schedule, k))


def test_three_frames_in_flight_dist(monkeypatch):
    """Three frames on a 3-slot sf_dist at 256 x 144 (the bench's own path: the lean loop under frames in flight),
    each against the oracle."""
    monkeypatch.setenv("SF_ORDER", "0")
    monkeypatch.delenv("SF_LEAN", raising=False)
    keys = [("seed", CATCH[0]), ("seed", CATCH[1]), ("seed", CATCH[2])]
    with sf.SphereflakeDist(0, 256, 144, slots=3) as d:
        slots = []
        for key in keys:
            d.SetView(*reference(key)[0])
            d.RenderBands()
            slots.append(d.last_slot())
        assert sorted(slots) == [0, 1, 2]
        for key, slot in zip(keys, slots):
            ref = reference(key)[2]
            pos, nrm = d.download_slot(slot)
            assert np.array_equal(bits(pos), bits(ref["pos4"])), key
            assert np.array_equal(bits(nrm), bits(ref["nrm4"])), key
        st = d.stats()
        assert st.max_depth == max(reference(k)[2]["stats"]["max_depth"] for k in keys)
        assert st.overflow_tiles == 0
        assert sum(sf.lib().sf_lean_launches(d.context(k)) for k in range(3)) == 3


def test_general_loop_serves_forced_retrace(monkeypatch):
    """SF_FLAGS=0x400 (every tile through the index-order re-trace) under the default SF_LEAN: a mode the lean loop
    leaves out, so the general loop runs; the golden c1."""
    fx = load_frame("c1")
    view, _ = camera_view(sf.config_camera(fx["W"], fx["H"], float.fromhex(fx["K"])))
    frames, n = render_frames(view, (fx["W"], fx["H"]), {"SF_FLAGS": "0x400", "SF_ORDER": "0"}, monkeypatch, 2)
    assert n == 0
    for k, (got, st) in enumerate(frames):
        assert_golden(fx, got, st, k)
