"""GPU tests of the leaf-level loop (sf_kernels.hip: leaf_children): a node whose children are all inline leaves is
not opened -- its children are tested from the parent's loop, own sphere first, with no push and no pop -- in
traverse_ray, in the pair loop's one-ray loop and for the disjoint-lane nodes of its two-ray loop.

Every case renders with SF_PAIR=1 and with SF_PAIR=0 in fresh contexts and requires bit-equal position and normal, equal
stats (max_depth, closest, rays, overflow tiles) and the golden digests (or the oracle's frame). The frames are the
golden t4 (13 x 7), t1 and t2 (64 x 36) and t3 (80 x 45, depth 9): tests/test_leaf_nodes_host.py shows with the CPU
model that each holds leaf-level nodes the loop takes, leaf children whose bounding sphere is hit and whose own sphere
is not, and -- with the depth seed off -- leaf-level nodes that keep the child loop (the GPU cannot see which ran)."""
import numpy as np
import pytest

from sfcheck import bad_rows, frame_digest, row_digests

pytestmark = pytest.mark.gpu

import sphereflake_amd as sf  # noqa: E402
from test_gpu_depth_seed import CATCH, camera_view  # noqa: E402
from test_gpu_lean_tile import SCHEDULES, assert_golden, assert_oracle, bits, reference  # noqa: E402
from test_gpu_pair_fold import fixture_view  # noqa: E402
from test_gpu_pair_tile import ENV_KEYS, PAIR_SCHEDULES, pair_and_single  # noqa: E402

FIXTURES = ["t4", "t1", "t2", "t3"]


@pytest.fixture(scope="module", autouse=True)
def device():
    sf.build()
    assert sf.device_count() >= 1, "no HIP device visible: GPU tests must run on an MI355X"


def same_frames(a, b, what):
    """Two lists of ((pos, nrm), stats): bit-equal frames, equal stats."""
    for k, (((pa, na), sa), ((pb, nb), sb)) in enumerate(zip(a, b)):
        assert np.array_equal(bits(pa), bits(pb)) and np.array_equal(bits(na), bits(nb)), (what, k)
        assert (sa.max_depth, sa.closest, sa.rays, sa.overflow_tiles) == \
               (sb.max_depth, sb.closest, sb.rays, sb.overflow_tiles), (what, k)


@pytest.mark.parametrize("schedule", PAIR_SCHEDULES)
@pytest.mark.parametrize("name", FIXTURES)
def test_leaf_fixtures_golden(name, schedule, monkeypatch):
    fx, view, size = fixture_view(name)
    for k, (got, st) in enumerate(pair_and_single(view, size, schedule, monkeypatch)):
        assert_golden(fx, got, st, (name, schedule, k))


@pytest.mark.parametrize("flags", ["0x10", "0x100", "0x400"])
@pytest.mark.parametrize("name", ["t2", "t3"])
def test_leaf_flags(name, flags, monkeypatch):
    """0x10: no depth seed -- the first leaf-level nodes of every unit keep the child loop (their children's depth is
    not counted yet), the later ones take leaf_children; 0x100: no occlusion cull (no seed either, index order);
    0x400: every unit re-traced in index order."""
    fx, view, size = fixture_view(name)
    for k, (got, st) in enumerate(pair_and_single(view, size, "rowmajor", monkeypatch, extra={"SF_FLAGS": flags})):
        assert_golden(fx, got, st, (name, flags, k))


def test_leaf_nodes_at_the_deepest_provisioned_level(monkeypatch):
    """t3 with 3 provisioned levels: a leaf-level node whose level has no table keeps the overflow test, the tiles go to
    the fixup's deeper re-trace, and the frame is the golden one."""
    fx, view, size = fixture_view("t3")
    assert fx["stats"]["max_depth"] > 3
    for k, (got, st) in enumerate(pair_and_single(view, size, "rowmajor", monkeypatch, max_depth=3)):
        assert_golden(fx, got, st, k)


def render(view, size, env, monkeypatch, plan):
    """A fresh context under `env`; plan: a string of 'r' (reset the stats) and 'R' (render, download): the frames."""
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    frames = []
    with sf.Sphereflake(*size) as s:
        s.SetView(*view)
        for step in plan:
            if step == "r":
                s.reset_stats()
                continue
            s.Render()
            pos, nrm, _, _ = s.download()
            frames.append(((pos, nrm), s.stats()))
        return frames, s.pair_launches(), s.lean_launches()


def test_leaf_general_loop(monkeypatch):
    """t2 with SF_LEAN=0: the general tile loop (trace_tile's traverse_ray) whatever SF_PAIR says."""
    fx, view, size = fixture_view("t2")
    runs = []
    for pair in ("1", "0"):
        frames, pp, lp = render(view, size, dict(SCHEDULES["rowmajor"], SF_LEAN="0", SF_PAIR=pair), monkeypatch, "rRR")
        assert (pp, lp) == (0, 0), pair
        for k, (got, st) in enumerate(frames):
            assert_golden(fx, got, st, (pair, k))
        runs.append(frames)
    same_frames(runs[0], runs[1], "SF_LEAN=0")


def test_leaf_cold_warm_and_reset(monkeypatch):
    """One context, t3 twice and, after a stats reset, once more: the first frame starts with no depth seed (the first
    leaf-level nodes keep the child loop until the units' own depth covers them), the second with the seed at the
    frame's depth (every leaf-level node takes leaf_children), the third cold again."""
    fx, view, size = fixture_view("t3")
    runs = []
    for pair in ("1", "0"):
        frames, pp, lp = render(view, size, dict(SCHEDULES["rowmajor"], SF_PAIR=pair), monkeypatch, "rRRrR")
        assert (pp, lp) == ((3, 3) if pair == "1" else (0, 3)), pair
        for k, (got, st) in enumerate(frames):
            pos, nrm = got
            assert bad_rows(fx["row_digest_gbuf"], row_digests(pos, nrm)) == [], (pair, k)
            assert frame_digest(pos, nrm) == fx["frame_digest"], (pair, k)
            assert st.max_depth == fx["stats"]["max_depth"], (pair, k)
            assert np.float32(st.closest) == np.float32(float.fromhex(fx["stats"]["closest"])), (pair, k)
            assert st.overflow_tiles == 0, (pair, k)
        runs.append(frames)
    same_frames(runs[0], runs[1], "cold / warm / reset")


def test_leaf_occluded_deepest_node(monkeypatch):
    """A 256 x 144 view whose deepest node is occluded (test_gpu_depth_seed.py's CATCH): a loop that skipped children
    the child loop counts would report a smaller max depth than the oracle."""
    view, size, ref = reference(("seed", CATCH[0]))
    for k, (got, st) in enumerate(pair_and_single(view, size, "rowmajor", monkeypatch)):
        assert_oracle(got, st, ref, k)


@pytest.mark.parametrize("pair", ["1", "0"])
def test_leaf_three_frames_in_flight_dist(pair, monkeypatch):
    """Three views on a 3-slot sf_dist at 80 x 45: t3's (golden) and the config camera at two scales (oracle)."""
    from oracle import pyoracle
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
