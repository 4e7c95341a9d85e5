"""CPU test that the frames of tests/test_gpu_leaf_nodes.py hold the cases of the leaf-level loop (sf_kernels.hip:
leaf_children): the wave model (scripts/experiments/wave_sim.c, a 16 x 8 unit, no depth seed: the kernel under
SF_FLAGS=0x10) traces each fixture, agrees with the oracle in every pixel, and counts per depth the leaf-level nodes --
every child the cone cull kept is an inline leaf --, those that take the loop, those that must keep the child loop
because their children's depth is not yet counted in the unit's max depth, and the child iterations whose bounding
sphere some visiting lane hits while no visiting lane hits the child's own sphere (the iterations the loop ends at its
first compare). The GPU test cannot see which path ran inside a unit; this shows that its frames hold the cases."""
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
    mp.setenv("WAVE_SIM_DIR", str(tmp_path_factory.mktemp("wave_sim_leaf")))
    mp.delenv("LEVELS", raising=False)
    try:
        spec = importlib.util.spec_from_file_location(
            "wave_sim_leaf", os.path.join(REPO, "scripts", "experiments", "wave_sim.py"))
        ws = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ws)
    finally:
        mp.undo()
    assert (ws.TW, ws.TH) == (16, 8)
    return {name: ws.run(name) for name in FIXTURES}


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_has_leaf_level_cases(model, name):
    t = model[name]
    assert t["mismatch"] == 0 and t["ties"] == 0
    nodes, old, empty = int(t["lf_node"].sum()), int(t["lf_old"].sum()), int(t["lf_empty"].sum())
    taken = nodes - old
    hit, own = int(t["lf_hit"].sum()), int(t["lf_own"].sum())
    print(f"{name}: leaf-level nodes {nodes} (no child kept {empty}), taking the loop {taken}, keeping the child loop"
          f" {old}; their iterations {int(t['lf_iter'].sum())}: bounding sphere hit {hit}, own sphere hit {own},"
          f" entered {int(t['lf_ent'].sum())}, entered with an own hit {int(t['lf_ent_own'].sum())}")
    # leaf-level nodes with children to test, taken by the loop
    assert taken - empty >= 1 and int(t["lf_iter"].sum()) >= 1
    # leaf children whose bounding sphere is hit and whose own sphere is not
    assert hit - own >= 1
    # with the seed off: leaf-level nodes that must keep the child loop
    assert old >= 1
    # an own hit is a bounding hit; an entry is a bounding hit
    assert (t["lf_own"] <= t["lf_hit"]).all() and (t["lf_ent"] <= t["lf_hit"]).all()
    assert (t["lf_ent_own"] <= t["lf_own"]).all() and (t["lf_ent_own"] <= t["lf_ent"]).all()
    assert (t["lf_hit"] <= t["lf_iter"]).all() and (t["lf_iter"] <= t["iter"]).all()
    assert (t["lf_node"] <= t["exp"]).all()

