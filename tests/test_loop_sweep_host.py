"""CPU test that the views of tests/test_gpu_loop_sweep.py (tests/sweepviews.py, seeds 0..63) hold the cases of the
lean and pair tile loops: the wave model (scripts/experiments/wave_sim.c, a 16 x 8 unit, AVX variant) traces every view,
agrees with the oracle in every pixel, and counts what the GPU cannot report from inside a unit -- the subtree roots
the pair loop's one_ray_subtree takes (entered by tile B only: every entering lane exchanged; by both tiles on disjoint
hardware lanes: some exchanged), the two-ray iterations whose bounding hits lie in one tile, the leaf-level nodes and
those of them that keep the child loop. The oracle's frames give the rest: deep views, views where no ray hits, views
from inside a sphere (every ray hits at depth 0, with a negative min_t: the reference's quirk), the four classes of
pairs by which of their tiles are hit, and views that the SSE variant (LOD 60) renders differently from the AVX one.

Every floor below is a condition on the sweep's inputs, well under what this generator gives (64 views, CPU):
  views with a B-only root below depth 0            42   (1825 roots)      floor 20
  views with a disjoint-lane root below depth 0     39   (936 roots)       floor 20
  one-sided two-ray iterations                      4310                   floor 1000
  leaf-level nodes                                  33 568                 floor 10 000
  leaf-level nodes that keep the child loop         1338                   floor 300
  views of max depth >= 9                           5    (three at 10)     floor 3
  views where no ray hits                           8                      floor 5
  views where every ray hits at max depth 0         3    (seeds 31, 38, 57) floor 3
  views with a negative min_t                       10                     (printed)
  pairs hit in A only / B only / neither / both     154 / 32 / 637 / 689   each at least once
  views of depth >= 7 (the GPU sweep's overflow leg) 26                    floor 20
  views whose LOD-60 frame differs from LOD-70      25                     floor 1
If the generator changes, the counts are measured again and stated here; a floor is never lowered to fit."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import REPO
from sweepviews import DEEP, OVERFLOW_LEVELS, SEEDS, sweep_reference, sweep_view
from test_gpu_pair_tile import pair_hit_classes

import sphereflake_amd as sf


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    """The model built for the pair unit, and its totals per view (each traced once)."""
    sf.build()
    mp = pytest.MonkeyPatch()
    mp.setenv("WAVE_UNIT", "16x8")
    mp.setenv("WAVE_SIM_DIR", str(tmp_path_factory.mktemp("wave_sim_sweep")))
    mp.delenv("LEVELS", raising=False)
    try:
        spec = importlib.util.spec_from_file_location(
            "wave_sim_sweep", os.path.join(REPO, "scripts", "experiments", "wave_sim.py"))
        ws = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ws)
    finally:
        mp.undo()
    assert (ws.TW, ws.TH) == (16, 8)
    return {seed: ws.run(sweep_view(seed)[1]) for seed in SEEDS}


@pytest.fixture(scope="module")
def frames():
    sf.build()
    return {seed: sweep_reference(seed, "avx") for seed in SEEDS}


def test_model_agrees_with_the_oracle_on_every_view(model, frames):
    for seed in SEEDS:
        t, (W, H) = model[seed], sweep_view(seed)[3]
        what = (seed, (W, H), sweep_view(seed)[2])
        assert t["tiles"] == ((W + 15) // 16) * ((H + 7) // 8), what
        assert t["mismatch"] == 0, what
        assert t["ties"] == 0, what   # (a tie takes the index-order re-trace: the SF_FLAGS=0x400 tests' ground)
        assert t["maxd"] == frames[seed]["stats"]["max_depth"], what


def test_sweep_reaches_the_folded_subtrees(model):
    b_views = [s for s in SEEDS if model[s]["root_b"][1:].sum() > 0]
    d_views = [s for s in SEEDS if model[s]["root_d"][1:].sum() > 0]
    b_roots = sum(int(model[s]["root_b"][1:].sum()) for s in SEEDS)
    d_roots = sum(int(model[s]["root_d"][1:].sum()) for s in SEEDS)
    side = sum(int(model[s]["side_iter"].sum()) for s in SEEDS)
    print(f"B-only roots below depth 0: {b_roots} on {len(b_views)} views; disjoint-lane roots: {d_roots} on"
          f" {len(d_views)} views; one-sided two-ray iterations {side}")
    assert len(b_views) >= 20
    assert len(d_views) >= 20
    assert side >= 1000


def test_sweep_reaches_the_leaf_level_loop(model):
    nodes = sum(int(model[s]["lf_node"].sum()) for s in SEEDS)
    old = sum(int(model[s]["lf_old"].sum()) for s in SEEDS)
    print(f"leaf-level nodes {nodes}, keeping the child loop {old}")
    assert nodes >= 10000
    assert old >= 300


def test_sweep_has_deep_empty_and_inside_views(frames):
    st = {s: frames[s]["stats"] for s in SEEDS}
    deep = [s for s in SEEDS if st[s]["max_depth"] >= 9]
    empty = [s for s in SEEDS if st[s]["hits"] == 0]
    inside = [s for s in SEEDS if st[s]["hits"] == st[s]["rays"] and st[s]["max_depth"] == 0]
    print(f"max depth >= 9: seeds {deep} (depths {[st[s]['max_depth'] for s in deep]}); no ray hits: {empty};"
          f" every ray hits at depth 0: {inside}; depth >= 7 (the overflow leg): {sum(st[s]['max_depth'] >= 7 for s in SEEDS)}")
    assert len(deep) >= 3
    assert len(empty) >= 5
    assert len(inside) >= 3
    # (a camera inside the sphere it sees: the reference reports the negative root)
    print(f"views with a negative min_t: {[s for s in SEEDS if (frames[s]['minT'] < 0).any()]}")


def test_deep_views_overflow_the_levels_of_the_overflow_leg(model, frames):
    """The renderer's overflow_tiles counts the tiles that sf_fixup_wave could not resolve, 0 in every correct frame,
    so the GPU cannot say that a unit overflowed. The inputs can: on every view of depth >= DEEP the model enters
    children that are no leaves from nodes of depth levels - 1 (`push`), which the kernels flag instead."""
    deep = [s for s in SEEDS if frames[s]["stats"]["max_depth"] >= DEEP]
    assert len(deep) >= 20   # (26 here)
    for s in deep:
        lv = OVERFLOW_LEVELS
        assert lv + 2 <= DEEP
        assert model[s]["push"][lv - 1] > 0 and model[s]["exp"][lv] > 0, (s, lv)
    print(f"{len(deep)} views of depth >= {DEEP}, children entered from depth {OVERFLOW_LEVELS - 1}: " + ", ".join(
        f"{s}: {int(model[s]['push'][OVERFLOW_LEVELS - 1])}" for s in deep))


def test_sweep_has_the_four_pair_classes(frames):
    total = np.zeros(4, np.int64)
    for s in SEEDS:
        total += pair_hit_classes(frames[s]["index"], *sweep_view(s)[3])
    print("pairs hit in A only {}, in B only {}, in neither {}, in both {}".format(*total))
    assert (total > 0).all()


def test_sse_variant_differs_from_avx(frames):
    differ = []
    for s in SEEDS:
        a, b = frames[s], sweep_reference(s, "sse")
        if not (np.array_equal(a["index"], b["index"]) and np.array_equal(a["minT"].view(np.uint32), b["minT"].view(np.uint32))):
            differ.append(s)
    print(f"LOD 60 frame differs from LOD 70 on {len(differ)} of {len(SEEDS)} views: {differ}")
    assert len(differ) >= 1
