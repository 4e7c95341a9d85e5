"""CPU test that the frames of tests/test_gpu_pair_fold.py reach the pair loop's folded subtrees: the wave model
(scripts/experiments/wave_sim.c, a 16 x 8 unit) traces each fixture, agrees with the oracle in every pixel, and counts
the subtree roots that the kernel's one_ray_subtree takes -- entered by tile B only (every entering lane exchanged)
and by both tiles on disjoint hardware lanes (some lanes exchanged) -- and the two-ray iterations whose bounding hits
lie in one tile. The GPU test cannot see which loop ran inside a unit; this shows that its frames hold the cases."""
import importlib.util
import os

import pytest

from conftest import REPO

FIXTURES = ["t4", "t1", "t2", "t3"]


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    """The model built for the pair unit, and its totals per fixture (each traced once)."""
    mp = pytest.MonkeyPatch()
    mp.setenv("WAVE_UNIT", "16x8")
    mp.setenv("WAVE_SIM_DIR", str(tmp_path_factory.mktemp("wave_sim")))
    try:
        spec = importlib.util.spec_from_file_location(
            "wave_sim_pair", os.path.join(REPO, "scripts", "experiments", "wave_sim.py"))
        ws = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ws)
    finally:
        mp.undo()
    assert (ws.TW, ws.TH) == (16, 8)
    return {name: ws.run(name) for name in FIXTURES}


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_has_exchanged_and_disjoint_roots(model, name):
    t = model[name]
    assert t["mismatch"] == 0 and t["ties"] == 0
    b_only, disjoint = int(t["root_b"][1:].sum()), int(t["root_d"][1:].sum())
    print(f"{name}: roots entered from a two-ray node: A-only {int(t['root_a'][1:].sum())} B-only {b_only}"
          f" disjoint {disjoint}; one-sided two-ray iterations {int(t['side_iter'].sum())}")
    assert b_only >= 1 and disjoint >= 1
    # a folded subtree is at least the one-tile subtree the kernel ran on its one-ray loop before
    assert (t["fold_iter"] >= t["half_iter"]).all() and (t["fold_exp"] >= t["half_exp"]).all()
    assert t["fold_iter"].sum() > t["half_iter"].sum()


@pytest.mark.parametrize("name", ["t2", "t3"])
def test_fixture_has_one_sided_iterations(model, name):
    t = model[name]
    assert int(t["side_iter"].sum()) >= 1
    assert (t["side_lod"] <= t["side_iter"]).all()
    assert (t["side_iter"] <= t["iter"] - t["fold_iter"]).all()
