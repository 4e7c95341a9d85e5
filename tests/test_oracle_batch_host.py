"""CPU test of the oracle's batched ray entry (oracle/sf_oracle.c sfo_trace_rays, pyoracle.trace_rays): it is the
per-ray path -- rayscheck.oracle_multi, one pyoracle.render call of a 1 x 1 frame per ray -- bit for bit in position,
normal, min_t and hit index and in max_depth / closest / hits, on the seeded ray sets of tests/rayscheck.py and on
directions with a -0, a zero and a NaN component, at both LOD constants. tests/lightsweep.py builds its oracle masks
on the batch; this file is what lets it."""
import numpy as np
import pytest

import sphereflake_amd as sf
from dirscheck import same_bits
from oracle import pyoracle
from rayscheck import CHANNELS, SETS, oracle_multi, set_oracle


@pytest.fixture(scope="module", autouse=True)
def built():
    sf.build()


def assert_equal(got, want, what):
    for c in CHANNELS:
        assert got[c].dtype == want[c].dtype and same_bits(got[c], want[c]), f"{what}: {c} differs"
    for k in ("max_depth", "hits"):
        assert got["stats"][k] == want["stats"][k], (what, k)
    assert same_bits(np.float32(got["stats"]["closest"]), np.float32(want["stats"]["closest"])), (what, "closest")


def test_root_columns_are_the_root_transforms():
    """The rotation the batch takes from the golden setup is sf.root_transform's at any origin, and the translation
    it forms, 0 - origin, is root_transform's too."""
    cols = pyoracle.root_columns()
    for o in ((0.0, 0.0, 0.0), (-5.4098, -7.2139, 1.19006), (0.3, -0.0, 1e-30)):
        root = sf.root_transform(np.array(o, np.float32))
        assert same_bits(root[:12], cols), o
        assert same_bits(root[12:], np.append(np.float32(0.0) - np.array(o, np.float32), np.float32(1.0))), o


@pytest.mark.parametrize("threads", [1, 8])
@pytest.mark.parametrize("name", sorted(SETS))
def test_batch_equals_the_per_ray_path_on_the_seeded_sets(name, threads):
    gen, setup = SETS[name]
    o, d = gen()
    got = pyoracle.trace_rays(pyoracle.load_setup(setup)["children"], o, d, 70.0, threads=threads)
    assert_equal(got, set_oracle(name), f"{name}, {threads} threads")
    assert (got["stats"]["hits"] > 0) == (name != "towards_out")   # (that set's rays leave the flake)


def special_directions():
    """256 directions from the origin (-5.4098, -7.2139, 1.19006) (t3's camera): seeded normals about the direction
    to the flake, and among them components that are -0, +0 and NaN, whole -0 / 0 / NaN directions, an infinity and
    a denormal."""
    rng = np.random.default_rng(107)
    o = np.array((-5.4098, -7.2139, 1.19006), np.float32)
    d = (-o / np.linalg.norm(o) + rng.normal(0.0, 0.12, (256, 3))).astype(np.float32)
    for k in range(3):
        d[10 + k, k] = -0.0
        d[20 + k, k] = 0.0
        d[30 + k, k] = np.nan
        d[40 + k, (k + 1) % 3] = -0.0
        d[40 + k, (k + 2) % 3] = -0.0
    d[50] = (-0.0, -0.0, -0.0)
    d[51] = (0.0, 0.0, 0.0)
    d[52] = (np.nan, np.nan, np.nan)
    d[53, 1] = np.inf
    d[54, 2] = 1e-42
    d[55] = (-0.0, 0.0, np.nan)
    # axis-aligned rays at the flake's centre from an origin of their own are below (one -0 among two exact zeros)
    return o, d


@pytest.mark.parametrize("lod", [70.0, 60.0])
def test_batch_equals_the_per_ray_path_on_special_directions(lod):
    children = pyoracle.load_setup("t3")["children"]
    o, d = special_directions()
    assert np.signbit(d[d == 0]).any() and (d == 0).any() and np.isnan(d).any()
    want = oracle_multi(children, o.reshape(1, 3), d, rays_per_origin=256, lod=lod)
    got = pyoracle.trace_rays(children, o, d, lod)
    assert_equal(got, want, f"LOD {lod}")
    assert 100 <= got["stats"]["hits"] < 256
    # a ray down an axis, its direction's other components -0 and +0: the hit is the centre sphere's, and the
    # direction's -0 comes out as +0 (the position's component is +0, not -0)
    o2 = np.array([(0.0, -6.0, 0.0), (5.0, 0.0, 0.0), (0.0, 0.0, 7.0)], np.float32)
    d2 = np.array([(-0.0, 1.0, 0.0), (-1.0, -0.0, 0.0), (0.0, -0.0, -1.0)], np.float32)
    want2 = oracle_multi(children, o2, d2, lod=lod)
    got2 = pyoracle.trace_rays(children, o2, d2, lod)
    assert_equal(got2, want2, f"LOD {lod}, axes")
    assert got2["stats"]["hits"] == 3
    assert not np.signbit(got2["pos4"][0, 0]) and not np.signbit(got2["pos4"][1, 1]) and not np.signbit(got2["pos4"][2, 1])


def test_lod_constant_is_set_per_call():
    """The constant is the library's global: a call at 60 after one at 70 traces at 60, and the other way round."""
    children = pyoracle.load_setup("t3")["children"]
    o, d = SETS["towards_in"][0]()
    a70 = pyoracle.trace_rays(children, o, d, 70.0)
    a60 = pyoracle.trace_rays(children, o, d, 60.0)
    b70 = pyoracle.trace_rays(children, o, d, 70.0)
    assert_equal(b70, a70, "70 again")
    assert not same_bits(a60["minT"], a70["minT"])
    assert_equal(a60, oracle_multi(children, o, d, lod=60.0), "60")


def test_near_depth_is_a_statistic_only():
    """With bounds the batch returns the same rays, and per ray the deepest node expanded before the bound: under an
    infinite bound the largest is max_depth, under bound 0 only the nodes whose bounding sphere holds the origin count
    (negative roots: these rays start on the flake), under -inf none, and the depth grows with the bound."""
    children = pyoracle.load_setup("t3")["children"]
    o, d = SETS["towards_in"][0]()
    plain = pyoracle.trace_rays(children, o, d, 70.0)
    inf = pyoracle.trace_rays(children, o, d, 70.0, bounds=np.full(len(d), np.inf, np.float32))
    assert_equal(inf, plain, "with bounds")
    assert inf["near_depth"].dtype == np.int8 and int(inf["near_depth"].max()) == plain["stats"]["max_depth"] >= 5
    zero = pyoracle.trace_rays(children, o, d, 70.0, bounds=np.zeros(len(d), np.float32))
    assert (zero["near_depth"] <= inf["near_depth"]).all() and (zero["near_depth"] < inf["near_depth"]).any()
    none = pyoracle.trace_rays(children, o, d, 70.0, bounds=np.full(len(d), -np.inf, np.float32))
    assert (none["near_depth"] == -1).all()
    hit = plain["minT"] < np.finfo(np.float32).max
    at_hit = pyoracle.trace_rays(children, o, d, 70.0, bounds=np.where(hit, plain["minT"], 0).astype(np.float32))
    assert (at_hit["near_depth"] <= inf["near_depth"]).all() and (at_hit["near_depth"][hit] >= 0).all()
    assert (at_hit["near_depth"] < inf["near_depth"]).any()   # (something deeper lies behind the hit)
    assert_equal(pyoracle.trace_rays(children, o, d, 70.0), plain, "after a bounded call")


def test_empty_batch():
    children = pyoracle.load_setup("t1")["children"]
    r = pyoracle.trace_rays(children, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 70.0)
    assert r["minT"].shape == (0,) and r["pos4"].shape == (0, 4)
    assert r["stats"] == {"max_depth": 0, "closest": float(np.finfo(np.float32).max), "hits": 0}
