"""GPU tests of the traversal's near root in its select-free form (sf_rootforms.h: sqrt_fix, near_root_of; used by
sf_kernels.hip's near_root_big in the own-sphere accept of every tile loop), beside the LOD band's exact root, which
keeps the general form.

Every case renders with SF_PAIR=1 (sf_trace_queue1 / 1c: traverse_pair, leaf_children_pair, dfs_one), SF_PAIR=0
(sf_trace_queue1t: the single-tile lean loop) and SF_LEAN=0 (the general loop) in fresh contexts, asserts from
pair_launches / lean_launches which loop ran, and compares position, normal, max_depth, closest and rays with the
oracle, bit for bit. The oracle frames are test_gpu_lean_tile.reference's (computed once per process, read-only)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import sphereflake_amd as sf  # noqa: E402
from test_gpu_depth_seed import camera_view  # noqa: E402
from test_gpu_lean_tile import SCHEDULES, assert_oracle, bits, far_root_counts, reference  # noqa: E402
from test_gpu_leaf_nodes import render, same_frames  # noqa: E402
from test_gpu_pair_tile import ENV_KEYS, edge_view, pair_and_single, pair_hit_classes  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def device():
    sf.build()
    assert sf.device_count() >= 1, "no HIP device visible: GPU tests must run on an MI355X"


def three_loops(view, size, ref, monkeypatch, extra=None):
    """Two renders in each of the three loops under the row-major schedule (and `extra`), each against the oracle frame
    `ref`; pair_and_single asserts that every SF_PAIR=1 launch took the pair loop, that no SF_PAIR=0 launch did, and
    the rays counted; SF_LEAN=0 must take neither lean loop."""
    extra = extra or {}
    paired = pair_and_single(view, size, "rowmajor", monkeypatch, extra=extra)
    general, pp, lp = render(view, size, dict(SCHEDULES["rowmajor"], SF_LEAN="0", **extra), monkeypatch, "rRR")
    assert (pp, lp) == (0, 0)
    same_frames(paired, general, "SF_LEAN=0")
    for k, (got, st) in enumerate(paired):
        assert_oracle(got, st, ref, k)
        assert st.rays == (k + 1) * size[0] * size[1], k


def test_one_pair_16x8(monkeypatch):
    """16 x 8 on the flake: one pair unit, both tiles whole."""
    view, size, ref = reference(("config", (16, 8)))
    assert ref["stats"]["hits"] > 0
    three_loops(view, size, ref, monkeypatch)


def test_last_pair_without_b_tile_24x16(monkeypatch):
    """24 x 16: the last pair of each row has no B tile, so its hit path runs for ray A alone."""
    view, size, ref = reference(("config", (24, 16)))
    assert ref["stats"]["hits"] > 0
    three_loops(view, size, ref, monkeypatch)


def test_far_view_band_roots(monkeypatch):
    """far_view() of the lean tests (from T_0 + 1.9 r_0 away): every bounding hit of the root lies in the band that
    neither tca < T nor tca (1 - 2^-8) >= Tfar decides, on both sides of the threshold, in both rays of the pairs: the
    bracket, and for its undecided lanes the exact root, decide every one of them."""
    view, size, ref = reference(("far", None))
    passed, failed = far_root_counts()
    assert passed > 0 and failed > 0
    three_loops(view, size, ref, monkeypatch)


def test_one_sided_pairs(monkeypatch):
    """edge_view() of the pair tests (128 x 72, the flake ends inside the frame): pairs with hits in one tile only, so
    the one-ray forms run on exchanged registers."""
    view, size, ref = edge_view()
    only_a, only_b, _, both = pair_hit_classes(ref["index"], *size)
    assert only_a + only_b > 0 and both > 0
    three_loops(view, size, ref, monkeypatch)


def test_forced_retrace_72x40(monkeypatch):
    """SF_FLAGS=0x400 at 72 x 40: every unit re-traced in index order (the accept's tie rule without a branch)."""
    view, size, ref = reference(("config", (72, 40)))
    three_loops(view, size, ref, monkeypatch, extra={"SF_FLAGS": "0x400"})


@pytest.mark.parametrize("env", [{"SF_PAIR": "1"}, {"SF_PAIR": "0"}, {"SF_LEAN": "0"}], ids=["pair", "single", "general"])
def test_three_frames_in_flight_dist(env, monkeypatch):
    """Three views on a 3-slot SphereflakeDist at 80 x 45 (the config camera at three scales; row-major units, so that
    the lean loops take every launch that SF_LEAN allows), each slot against the oracle."""
    from oracle import pyoracle
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(SCHEDULES["rowmajor"], **env).items():
        monkeypatch.setenv(k, v)
    size = (80, 45)
    view1, _, ref1 = reference(("config", size))
    refs = [(view1, ref1)]
    for scale in (0.5, 0.25):
        view, setup = camera_view(sf.config_camera(size[0], size[1], scale))
        refs.append((view, pyoracle.render(setup, threads=8)))
    with sf.SphereflakeDist(0, size[0], size[1], slots=3) as d:
        slots = []
        for view, _ in refs:
            d.SetView(*view)
            d.RenderBands()
            slots.append(d.last_slot())
        assert sorted(slots) == [0, 1, 2]
        st = d.stats()
        for slot, (_, ref) in zip(slots, refs):
            pos, nrm = d.download_slot(slot)
            assert np.array_equal(bits(pos), bits(ref["pos4"])), slot
            assert np.array_equal(bits(nrm), bits(ref["nrm4"])), slot
        assert st.max_depth == max(ref["stats"]["max_depth"] for _, ref in refs)
        assert np.float32(st.closest) == min(np.float32(ref["stats"]["closest"]) for _, ref in refs)
        assert st.rays == 3 * size[0] * size[1]
        assert st.overflow_tiles == 0
        # (pair launches, lean launches -- which include the pair launches)
        want = (3, 3) if env == {"SF_PAIR": "1"} else (0, 3) if env == {"SF_PAIR": "0"} else (0, 0)
        got = (sum(sf.lib().sf_pair_launches(d.context(k)) for k in range(3)),
               sum(sf.lib().sf_lean_launches(d.context(k)) for k in range(3)))
        assert got == want, env
