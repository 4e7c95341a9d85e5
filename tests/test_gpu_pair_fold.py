"""GPU tests of the pair loop's folded subtrees (sf_kernels.hip: traverse_pair / one_ray_subtree): a node that no
hardware lane visits with both its rays -- a node of one tile only, or one that straddles the tiles' boundary on
disjoint lanes -- runs the one-ray loop, the lanes that visit with ray B exchanged into ray A's registers around it.

Every case renders with SF_PAIR=1 and with SF_PAIR=0 in fresh contexts (test_gpu_pair_tile.py's pair_and_single) and
requires bit-equal position and normal, equal stats, and the golden digests. The frames are the golden t1-t4: the
smallest that hold A-only, B-only and disjoint-lane subtree roots and one-sided iterations of the two-ray loop, which
tests/test_pair_fold_host.py counts with the CPU model (the GPU cannot see which loop ran inside a unit):

  t4 13 x 7 (one pair, B tile 5 columns wide), t1 64 x 36, t2 64 x 36 (depth 8), t3 80 x 45 (depth 9, partial bottom
  row)."""
import functools

import numpy as np
import pytest

from conftest import load_frame
from sfcheck import bad_rows, frame_digest, row_digests

pytestmark = pytest.mark.gpu

import sphereflake_amd as sf  # noqa: E402
from test_gpu_depth_seed import camera_view  # noqa: E402
from test_gpu_lean_tile import assert_golden, bits, reference  # noqa: E402
from test_gpu_pair_tile import ENV_KEYS, PAIR_SCHEDULES, pair_and_single  # noqa: E402

FIXTURES = ["t4", "t1", "t2", "t3"]


@pytest.fixture(scope="module", autouse=True)
def device():
    sf.build()
    assert sf.device_count() >= 1, "no HIP device visible: GPU tests must run on an MI355X"


@functools.lru_cache(maxsize=None)
def fixture_view(name):
    """(golden frame, view, (W, H)) of a golden fixture: the view of its committed setup."""
    from oracle import pyoracle
    fx, S = load_frame(name), pyoracle.load_setup(name)
    assert (int(S["W"]), int(S["H"])) == (fx["W"], fx["H"])
    view = tuple(np.asarray(S[k], np.float32) for k in ("origin", "tl", "tr", "bl"))
    return fx, view, (fx["W"], fx["H"])


@pytest.mark.parametrize("schedule", PAIR_SCHEDULES)
@pytest.mark.parametrize("name", FIXTURES)
def test_fold_fixtures_golden(name, schedule, monkeypatch):
    """Each fixture under both schedules (`ordered`: the cost-recording pair kernel rebuilds the order)."""
    fx, view, size = fixture_view(name)
    for k, (got, st) in enumerate(pair_and_single(view, size, schedule, monkeypatch)):
        assert_golden(fx, got, st, (name, schedule, k))


@pytest.mark.parametrize("name", ["t2", "t3"])
def test_fold_forced_index_order_retrace(name, monkeypatch):
    """SF_FLAGS=0x400: every pair re-traced in index order -- the exchange of the ancestor masks under the other
    child order."""
    fx, view, size = fixture_view(name)
    for k, (got, st) in enumerate(pair_and_single(view, size, "rowmajor", monkeypatch, extra={"SF_FLAGS": "0x400"})):
        assert_golden(fx, got, st, (name, k))


def test_fold_overflow_inside_exchanged_subtrees(monkeypatch):
    """t3 with 3 provisioned levels: the overflow is flagged inside exchanged subtrees (the deepest level's test reads
    both register sets), both tiles of the pair go to the fixup, and the frame is the golden one."""
    fx, view, size = fixture_view("t3")
    assert fx["stats"]["max_depth"] > 3
    for k, (got, st) in enumerate(pair_and_single(view, size, "rowmajor", monkeypatch, max_depth=3)):
        assert_golden(fx, got, st, k)


def test_fold_without_depth_seed(monkeypatch):
    """t2 with SF_FLAGS=0x10: the occlusion cull's depth bound starts from nothing in every unit."""
    fx, view, size = fixture_view("t2")
    for k, (got, st) in enumerate(pair_and_single(view, size, "rowmajor", monkeypatch, extra={"SF_FLAGS": "0x10"})):
        assert_golden(fx, got, st, k)


def test_fold_three_frames_in_flight_dist(monkeypatch):
    """Three views on a 3-slot sf_dist at 80 x 45 with SF_PAIR=1: t3's (golden) and the config camera at two scales
    (oracle)."""
    from oracle import pyoracle
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SF_PAIR", "1")
    fx, view3, size = fixture_view("t3")
    assert size == (80, 45)
    view1, _, ref1 = reference(("config", size))
    view2, setup2 = camera_view(sf.config_camera(size[0], size[1], 0.5))
    ref2 = pyoracle.render(setup2, threads=8)
    views = [view3, view1, view2]
    with sf.SphereflakeDist(0, size[0], size[1], slots=3) as d:
        slots = []
        for v in views:
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
        assert sum(sf.lib().sf_pair_launches(d.context(k)) for k in range(3)) == 3
