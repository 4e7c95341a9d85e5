"""GPU tests of the lean loops' fixed path around the traversal (sf_kernels.hip: frame_consts by a scalar load,
ray_dir_pair / normalize3_fast2 in the pair unit's head, write_pair in its tail, the one-ray forms in the single-tile
lean loop): both table gathers of a stage in flight behind one wait, rsqrtps_pos where every live lane's squared
length is a positive normal and rsqrtps_x86 for the whole wave otherwise, the misses' zeros selected after shading.

Every case renders with SF_PAIR=1 (sf_trace_queue1 / 1c) and SF_PAIR=0 (sf_trace_queue1t) in fresh contexts and
requires bit-equal position and normal and equal stats against the golden digests or the oracle, and against
SF_LEAN=0 of the same library (the general loop, whose ray generation and shading are unchanged: normalize3 with
rsqrtps_x86 per lane). pair_launches / lean_launches say which loop ran."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import sphereflake_amd as sf  # noqa: E402
from test_gpu_depth_seed import camera_view  # noqa: E402
from test_gpu_lean_tile import MISS, SCHEDULES, assert_golden, assert_oracle, bits, reference  # noqa: E402
from test_gpu_leaf_nodes import render, same_frames  # noqa: E402
from test_gpu_pair_fold import fixture_view  # noqa: E402
from test_gpu_pair_tile import ENV_KEYS, pair_and_single  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def device():
    sf.build()
    assert sf.device_count() >= 1, "no HIP device visible: GPU tests must run on an MI355X"


def three_loops(view, size, schedule, monkeypatch):
    """The pair loop's frames under `schedule`, after asserting that the single-tile lean loop (pair_and_single) and
    the general loop (SF_LEAN=0) give the same frames and stats, render by render, and that each loop ran."""
    paired = pair_and_single(view, size, schedule, monkeypatch)
    general, pp, lp = render(view, size, dict(SCHEDULES[schedule], SF_LEAN="0"), monkeypatch, "r" + "R" * len(paired))
    assert (pp, lp) == (0, 0), schedule
    same_frames(paired, general, ("SF_LEAN=0", schedule))
    return paired


def test_one_pair_partial_in_both_directions_t4(monkeypatch):
    """t4 (13 x 7): one pair unit; tile A full width and 7 rows, tile B 5 columns: invalid lanes in both rays."""
    fx, view, size = fixture_view("t4")
    assert size == (13, 7)
    for k, (got, st) in enumerate(three_loops(view, size, "rowmajor", monkeypatch)):
        assert_golden(fx, got, st, k)


@pytest.mark.parametrize("schedule", ["rowmajor", "ordered"])
def test_hits_and_misses_in_one_tile_t1(schedule, monkeypatch):
    """t1 (64 x 36): tiles with hits and misses side by side, so the zeros are selected lane by lane."""
    fx, view, size = fixture_view("t1")
    frames = three_loops(view, size, schedule, monkeypatch)
    pos = frames[0][0][0].reshape(size[1], size[0], 4)
    miss = (bits(pos) == bits(MISS)).all(axis=-1)
    mixed = sum(0 < int(miss[y:y + 8, x:x + 8].sum()) < miss[y:y + 8, x:x + 8].size
                for y in range(0, size[1], 8) for x in range(0, size[0], 8))
    assert mixed > 0
    for k, (got, st) in enumerate(frames):
        assert_golden(fx, got, st, (schedule, k))


def test_last_pair_without_b_tile_24x16(monkeypatch):
    """24 x 16 on the flake: 3 tile columns, so the last pair of each row has no B tile and its ray B no live lane."""
    view, size, ref = reference(("config", (24, 16)))
    assert ref["stats"]["hits"] > 0
    for k, (got, st) in enumerate(three_loops(view, size, "rowmajor", monkeypatch)):
        assert_oracle(got, st, ref, k)


def test_no_live_lane_at_shading_40x20(monkeypatch):
    """40 x 20 looking away from the flake: every ray misses, no lane is live when the units shade."""
    view, size, ref = reference(("away", (40, 20)))
    assert ref["stats"]["hits"] == 0
    for k, ((pos, nrm), st) in enumerate(three_loops(view, size, "rowmajor", monkeypatch)):
        assert np.array_equal(bits(pos), bits(np.broadcast_to(MISS, pos.shape))), k
        assert np.array_equal(bits(nrm), bits(np.broadcast_to(MISS, nrm.shape))), k
        assert_oracle((pos, nrm), st, ref, k)


def test_twice_in_one_context_and_after_a_reset_t3(monkeypatch):
    """t3 (80 x 45) twice in one context and once more after a stats reset, in the three loops."""
    fx, view, size = fixture_view("t3")
    runs = []
    for env, want in (({"SF_PAIR": "1"}, (3, 3)), ({"SF_PAIR": "0"}, (0, 3)), ({"SF_LEAN": "0"}, (0, 0))):
        frames, pp, lp = render(view, size, dict(SCHEDULES["rowmajor"], **env), monkeypatch, "rRRrR")
        assert (pp, lp) == want, env
        for k, (got, st) in enumerate(frames):
            assert_golden(fx, got, st, (env, k))
        runs.append(frames)
    same_frames(runs[0], runs[1], "SF_PAIR=0")
    same_frames(runs[0], runs[2], "SF_LEAN=0")


ORIGIN = np.zeros(3, np.float32)
HUGE = np.full(3, 1e20, np.float32)


@pytest.mark.parametrize("corner", [ORIGIN, HUGE], ids=["length0", "lengthinf"])
def test_fallback_for_the_whole_wave(corner, monkeypatch):
    """16 x 8, all four view corners equal: every ray's squared length is 0 (corners at the origin) or +inf (1e20),
    so every live lane fails the predicate and both rays take rsqrtps_x86. The directions are NaN (0 x inf): every
    pixel is a miss. Against SF_LEAN=0 only (x86's NaN payloads are not the oracle's concern here)."""
    view, size = (ORIGIN, corner, corner, corner), (16, 8)
    runs = []
    for env, want in (({"SF_PAIR": "1"}, (2, 2)), ({"SF_PAIR": "0"}, (0, 2)), ({"SF_LEAN": "0"}, (0, 0))):
        for k in ENV_KEYS:
            monkeypatch.delenv(k, raising=False)
        for k, v in dict(SCHEDULES["rowmajor"], **env).items():
            monkeypatch.setenv(k, v)
        frames = []
        with sf.Sphereflake(*size) as s:
            s.SetView(*view)
            s.reset_stats()
            for _ in range(2):
                s.Render()
                s.Synchronize()   # (raises on a device error)
                pos, nrm, _, _ = s.download()
                frames.append(((pos, nrm), s.stats()))
            assert (s.pair_launches(), s.lean_launches()) == want, env
        for k, ((pos, nrm), st) in enumerate(frames):
            assert np.array_equal(bits(pos), bits(np.broadcast_to(MISS, pos.shape))), (env, k)
            assert np.array_equal(bits(nrm), bits(np.broadcast_to(MISS, nrm.shape))), (env, k)
            assert st.rays == (k + 1) * size[0] * size[1] and st.overflow_tiles == 0, (env, k)
        runs.append(frames)
    same_frames(runs[0], runs[2], "SF_PAIR=1 / SF_LEAN=0")
    same_frames(runs[1], runs[2], "SF_PAIR=0 / SF_LEAN=0")


@pytest.mark.parametrize("pair", ["1", "0"])
def test_three_frames_in_flight_dist(pair, monkeypatch):
    """Three views on a 3-slot sf_dist at 80 x 45: t3's (golden) and the config camera at two scales (oracle)."""
    from oracle import pyoracle
    from sfcheck import bad_rows, frame_digest, row_digests
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SF_PAIR", pair)
    fx, view3, size = fixture_view("t3")
    assert size == (80, 45)
    view1, _, ref1 = reference(("config", size))
    view2, setup2 = camera_view(sf.config_camera(size[0], size[1], 0.5))
    ref2 = pyoracle.render(setup2, threads=8)
    with sf.SphereflakeDist(0, size[0], size[1], slots=3) as d:
        slots = []
        for v in (view3, view1, view2):
            d.SetView(*v)
            d.RenderBands()
            slots.append(d.last_slot())
        assert sorted(slots) == [0, 1, 2]
        st = d.stats()
        pos, nrm = d.download_slot(slots[0])
        assert bad_rows(fx["row_digest_gbuf"], row_digests(pos, nrm)) == []
        assert frame_digest(pos, nrm) == fx["frame_digest"]
        for slot, ref in ((slots[1], ref1), (slots[2], ref2)):
            pos, nrm = d.download_slot(slot)
            assert np.array_equal(bits(pos), bits(ref["pos4"])), slot
            assert np.array_equal(bits(nrm), bits(ref["nrm4"])), slot
        assert st.max_depth == max(fx["stats"]["max_depth"], ref1["stats"]["max_depth"], ref2["stats"]["max_depth"])
        assert st.overflow_tiles == 0
        assert sum(sf.lib().sf_pair_launches(d.context(k)) for k in range(3)) == (3 if pair == "1" else 0)
