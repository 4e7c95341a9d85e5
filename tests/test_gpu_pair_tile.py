"""GPU tests of the pair-unit tile loop (sf_kernels.hip: traverse_pair / trace_pair, kernels sf_trace_queue1 and
sf_trace_queue1c): two horizontally adjacent 8 x 8 tiles traced by one wave, ray A and ray B per lane, sharing the
traversal's upper levels; a subtree entered by lanes of one ray only runs the one-ray loop.

Every case renders with SF_PAIR=1 (pair units wherever the lean loop may run, whatever the frame size) and with
SF_PAIR=0 (no pair units) in fresh contexts and requires bit-equal position and normal, equal max_depth, closest, rays
and overflow_tiles, and equality with the oracle or the golden digests; sf_pair_launches says which loop ran. The
schedules are test_gpu_lean_tile.py's `rowmajor` and `ordered`: under `ordered` the render that rebuilds the order is
the cost-recording pair loop (sf_trace_queue1c) and the renders after it read ordered pair units."""
import functools

import numpy as np
import pytest

from conftest import load_frame

pytestmark = pytest.mark.gpu

import sphereflake_amd as sf  # noqa: E402
from test_gpu_depth_seed import CATCH, camera_view  # noqa: E402
from test_gpu_lean_tile import (MISS, SCHEDULES, assert_golden, assert_oracle, away_camera, bits,  # noqa: E402
                                far_root_counts, reference)

PAIR_SCHEDULES = ["rowmajor", "ordered"]
ENV_KEYS = SCHEDULES["rowmajor"].keys() | SCHEDULES["ordered"].keys() | {"SF_LEAN", "SF_FLAGS", "SF_PAIR", "SF_LEVELS",
                                                                        "SF_TIE_INLINE", "SF_MAX_BLOCKS"}
EDGE_W, EDGE_H, EDGE_YAW = 128, 72, 0.2   # the view whose flake ends inside the frame (edge_view)


@pytest.fixture(scope="module", autouse=True)
def device():
    sf.build()
    assert sf.device_count() >= 1, "no HIP device visible: GPU tests must run on an MI355X"


def render_frames(view, size, env, monkeypatch, n, pair, variant=None, **kw):
    """n renders after a reset (no aux channels) in a fresh context under `env` and SF_PAIR=`pair` (in the reference
    variant `variant` where given): [((pos, nrm), stats)], the launches that took the pair loop, and those that took
    a lean loop."""
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("SF_PAIR", pair)
    frames = []
    with sf.Sphereflake(*size) as s:
        if variant is not None:
            s.SetVariant(variant)
        s.SetView(*view)
        s.reset_stats()
        for _ in range(n):
            s.Render(**kw)
            pos, nrm, _, _ = s.download()
            frames.append(((pos, nrm), s.stats()))
        return frames, s.pair_launches(), s.lean_launches()


def pair_and_single(view, size, schedule, monkeypatch, extra=None, **kw):
    """SF_PAIR=1 and SF_PAIR=0 under one schedule: the pair frames, after asserting that the two agree bit for bit and
    in max_depth, closest, rays and overflow_tiles, render by render, that every SF_PAIR=1 launch took the pair loop
    and that no SF_PAIR=0 launch did."""
    n = 3 if schedule == "ordered" else 2   # (the render after the reset, and the next; ordered: the rebuild first)
    env = dict(SCHEDULES[schedule], **(extra or {}))
    single, ps, _ = render_frames(view, size, env, monkeypatch, n, "0", **kw)
    paired, pp, lp = render_frames(view, size, env, monkeypatch, n, "1", **kw)
    assert ps == 0, schedule
    assert pp == n and lp == n, (schedule, pp, lp)   # (the lean count includes the pair launches)
    for k, ((a, sa), (b, sb)) in enumerate(zip(single, paired)):
        for x, y in zip(a, b):
            assert np.array_equal(bits(x), bits(y)), (schedule, k)
        assert (sa.max_depth, sa.closest, sa.rays, sa.overflow_tiles) == \
               (sb.max_depth, sb.closest, sb.rays, sb.overflow_tiles), (schedule, k)
        assert sb.rays == (k + 1) * size[0] * size[1], (schedule, k)
    return paired


def c1_view():
    fx = load_frame("c1")
    view, _ = camera_view(sf.config_camera(fx["W"], fx["H"], float.fromhex(fx["K"])))
    return fx, view


@functools.lru_cache(maxsize=None)
def edge_view():
    """(view, size, oracle frame): the config camera at 128 x 72 turned 0.2 rad, so that the flake leaves the frame on
    one side and ends inside it on the other (the yaw chosen on the CPU from the oracle's frame)."""
    from oracle import pyoracle
    cam = sf.config_camera(EDGE_W, EDGE_H, 1.0)
    cam.SetYaw(np.float32(sf.DEFAULT_YAW + EDGE_YAW))
    view, setup = camera_view(cam)
    ref = pyoracle.render(setup, threads=8)
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return view, (EDGE_W, EDGE_H), ref


def pair_hit_classes(index, w, h):
    """Pairs of the frame with hits only in their A tile, only in their B tile, in neither, in both."""
    hit = np.asarray(index).reshape(h, w) != 0xffffffff
    only_a = only_b = neither = both = 0
    for ty in range((h + 7) // 8):
        for px in range(((w + 7) // 8 + 1) // 2):
            a = bool(hit[8 * ty:8 * ty + 8, 16 * px:16 * px + 8].any())
            b = bool(hit[8 * ty:8 * ty + 8, 16 * px + 8:16 * px + 16].any())
            only_a += a and not b
            only_b += b and not a
            neither += not a and not b
            both += a and b
    return only_a, only_b, neither, both


@pytest.mark.parametrize("schedule", PAIR_SCHEDULES)
def test_pair_equals_single_c1_golden(schedule, monkeypatch):
    """c1 (640 x 360, 80 tile columns): SF_PAIR=1 against SF_PAIR=0, and the golden digests."""
    fx, view = c1_view()
    for k, (got, st) in enumerate(pair_and_single(view, (fx["W"], fx["H"]), schedule, monkeypatch)):
        assert_golden(fx, got, st, (schedule, k))


@pytest.mark.parametrize("schedule", PAIR_SCHEDULES)
@pytest.mark.parametrize("size", [(72, 40), (70, 44), (136, 72), (8, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_odd_tile_columns_and_edge_lanes(size, schedule, monkeypatch):
    """72 x 40: 9 tile columns, the last pair of each row has an empty B; 70 x 44: its last A tile has 6 valid columns
    and the bottom row 4 valid rows; 136 x 72: 17 columns; 8 x 8: one tile, one pair. Against the oracle."""
    view, size, ref = reference(("config", size))
    for k, (got, st) in enumerate(pair_and_single(view, size, schedule, monkeypatch)):
        assert_oracle(got, st, ref, (size, schedule, k))


@pytest.mark.parametrize("schedule", PAIR_SCHEDULES)
@pytest.mark.parametrize("seed", CATCH)
def test_pair_occluded_deepest_node(seed, schedule, monkeypatch):
    """The seeded 256 x 144 views whose deepest node is occluded: the depth seed and the cull's depth bound are shared
    by the two tiles of a pair, and max_depth must still be the oracle's."""
    view, size, ref = reference(("seed", seed))
    for k, (got, st) in enumerate(pair_and_single(view, size, schedule, monkeypatch)):
        assert_oracle(got, st, ref, (seed, schedule, k))


@pytest.mark.parametrize("schedule", PAIR_SCHEDULES)
def test_one_half_leaves_at_the_root(schedule, monkeypatch):
    """The flake ends inside the frame: pairs with hits only in the A tile, only in the B tile, and in neither."""
    view, size, ref = edge_view()
    only_a, only_b, neither, both = pair_hit_classes(ref["index"], *size)
    print(f"edge view: {only_a} pairs hit in A only, {only_b} in B only, {neither} in neither, {both} in both")
    assert only_a > 0 and only_b > 0 and neither > 0
    for k, (got, st) in enumerate(pair_and_single(view, size, schedule, monkeypatch)):
        assert_oracle(got, st, ref, (schedule, k))


def test_view_away_from_the_flake(monkeypatch):
    """Every pair leaves at the root: every pixel is (0, 0, 0, 1), the rays are counted."""
    view, size, ref = reference(("away", (136, 72)))
    assert ref["stats"]["hits"] == 0
    for k, ((pos, nrm), st) in enumerate(pair_and_single(view, size, "rowmajor", monkeypatch)):
        assert np.array_equal(bits(pos), bits(np.broadcast_to(MISS, pos.shape))), k
        assert np.array_equal(bits(nrm), bits(np.broadcast_to(MISS, nrm.shape))), k
        assert_oracle((pos, nrm), st, ref, k)


@pytest.mark.parametrize("schedule", PAIR_SCHEDULES)
def test_far_view_straddles_root_lod(schedule, monkeypatch):
    """far_view() of the lean tests at 64 x 64: rays on both sides of the root's LOD threshold within a pair."""
    view, size, ref = reference(("far", None))
    passed, failed = far_root_counts()
    assert passed > 0 and failed > 0
    for k, (got, st) in enumerate(pair_and_single(view, size, schedule, monkeypatch)):
        assert_oracle(got, st, ref, (schedule, k))


@pytest.mark.parametrize("schedule", PAIR_SCHEDULES)
def test_forced_retrace_of_pairs_c1(schedule, monkeypatch):
    """SF_FLAGS=0x400: every pair through the index-order re-trace by its own wave -- the pair loop serves the flag
    itself (pair_and_single asserts that it ran); the golden c1."""
    fx, view = c1_view()
    for k, (got, st) in enumerate(pair_and_single(view, (fx["W"], fx["H"]), schedule, monkeypatch,
                                                  extra={"SF_FLAGS": "0x400"})):
        assert_golden(fx, got, st, (schedule, k))


@pytest.mark.parametrize("schedule", PAIR_SCHEDULES)
def test_forced_retrace_of_pairs_72x40(schedule, monkeypatch):
    """The same at 72 x 40 (pairs with an empty B), against the oracle."""
    view, size, ref = reference(("config", (72, 40)))
    for k, (got, st) in enumerate(pair_and_single(view, size, schedule, monkeypatch, extra={"SF_FLAGS": "0x400"})):
        assert_oracle(got, st, ref, (schedule, k))


@pytest.mark.parametrize("schedule", PAIR_SCHEDULES)
def test_overflow_of_pairs_72x40(schedule, monkeypatch):
    """max_depth = 3 levels, below the view's depth: the levels are not proven, pairs overflow, both tiles of each go
    to the overflow list and sf_fixup_wave re-traces them: the oracle's frame, overflow_tiles as with SF_PAIR=0."""
    view, size, ref = reference(("config", (72, 40)))
    assert ref["stats"]["max_depth"] > 3
    for k, (got, st) in enumerate(pair_and_single(view, size, schedule, monkeypatch, max_depth=3)):
        assert_oracle(got, st, ref, (schedule, k))


def test_three_frames_in_flight_dist(monkeypatch):
    """Three views on a 3-slot sf_dist at 256 x 144 with SF_PAIR=1 (the bench's own path), each slot against the
    oracle."""
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SF_PAIR", "1")
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
        assert sum(sf.lib().sf_pair_launches(d.context(k)) for k in range(3)) == 3
