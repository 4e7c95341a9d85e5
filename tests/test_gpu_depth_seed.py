"""GPU tests of the occlusion cull's depth seed (sf_kernels.hip: DepthSeed). The cull's depth bound -- the
condition that keeps the max-depth statistic what the reference reports -- starts from the depth the context's
max-depth word already holds and this wave's earlier tiles reached, not from 0 per tile. That may change neither a
pixel nor a statistic: cold (after a reset) and warm (the word holds the frame's depth), against the seed switched off
(SF_FLAGS=0x10, SF_FLAG_NO_DEPTH_SEED), across views of different depth under one word, per slot of sf_dist, and
through the index-order re-trace and sf_fixup_wave.

CATCH: views whose deepest node is occluded -- found on the CPU by scripts/experiments/depth_seed_view_search.py
among seeded_view(0..199): a cull without the depth condition reports a smaller max depth than the reference there
(occl_sim.c, mode + 128), so they tell a correct seed from a cull that ignores the statistic."""
import functools

import numpy as np
import pytest

from conftest import load_frame
from sfcheck import aux_digests, bad_rows, frame_digest, row_digests

pytestmark = pytest.mark.gpu

import sphereflake_amd as sf  # noqa: E402

NO_SEED = 0x10   # SF_FLAG_NO_DEPTH_SEED
W, H = 256, 144
CATCH = [6, 160, 169]   # seeds of seeded_view (see the module docstring): 36 of the 200 views searched are such views


def seeded_view(seed):
    """Random view `seed` at 256 x 144: ((origin, tl, tr, bl), the oracle's setup, camera scale); camera scale
    log-uniform over [0.05, 2.5], the rest as tests/test_gpu_random_views.py."""
    rng = np.random.default_rng(7000 + seed)
    cam = sf.Camera(W, H)
    K = float(np.exp(rng.uniform(np.log(0.05), np.log(2.5))))
    cam.SetPosition(np.asarray(sf.DEFAULT_CAMERA_POSITION, np.float32) * np.float32(K)
                    + rng.normal(0.0, 0.15 * K, 3).astype(np.float32))
    cam.SetPitch(np.float32(sf.DEFAULT_PITCH + rng.uniform(-0.4, 0.4)))
    cam.SetYaw(np.float32(sf.DEFAULT_YAW + rng.uniform(-0.6, 0.6)))
    cam.SetRoll(np.float32(rng.uniform(-0.3, 0.3)))
    cam.SetFOV(float(rng.choice([45.0, 60.0, 90.0])))
    return camera_view(cam) + (K,)


def camera_view(cam):
    o, tl, tr, bl = cam.corners()
    setup = {"W": cam.width, "H": cam.height, "origin": o, "tl": tl, "tr": tr, "bl": bl,
             "root": sf.root_transform(o), "children": sf.child_transforms()}
    return (o, tl, tr, bl), setup


@functools.lru_cache(maxsize=None)
def reference(key):
    """(view, oracle frame) of a view, computed once: ("seed", k): seeded_view(k); ("config", name): the BASELINE
    config view of that golden frame; ("scale", K): the config camera at scale K, 256 x 144."""
    from oracle import pyoracle
    kind, v = key
    if kind == "seed":
        view, setup, _ = seeded_view(v)
    elif kind == "config":
        fx = load_frame(v)
        view, setup = camera_view(sf.config_camera(fx["W"], fx["H"], float.fromhex(fx["K"])))
    else:
        view, setup = camera_view(sf.config_camera(W, H, v))
    ref = pyoracle.render(setup, threads=8)
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return view, (setup["W"], setup["H"]), ref


@pytest.fixture(scope="module", autouse=True)
def device():
    sf.build()
    assert sf.device_count() >= 1, "no HIP device visible: GPU tests must run on an MI355X"


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_oracle(got, st, ref, what, max_depth=None):
    pos, nrm, mint, idx = got
    assert np.array_equal(idx, ref["index"]), what
    assert np.array_equal(bits(pos), bits(ref["pos4"])), what
    assert np.array_equal(bits(nrm), bits(ref["nrm4"])), what
    assert np.array_equal(bits(mint), bits(ref["minT"])), what
    assert st.max_depth == (ref["stats"]["max_depth"] if max_depth is None else max_depth), what
    assert st.overflow_tiles == 0, what


def assert_golden(fx, got, st, what):
    pos, nrm, mint, idx = got
    assert bad_rows(fx["row_digest_gbuf"], row_digests(pos, nrm)) == [], what
    assert bad_rows(fx["row_digest_aux"], aux_digests(mint, idx)) == [], what
    assert frame_digest(pos, nrm) == fx["frame_digest"], what
    assert st.max_depth == fx["stats"]["max_depth"], what
    assert np.float32(st.closest) == np.float32(float.fromhex(fx["stats"]["closest"])), what
    assert st.overflow_tiles == 0, what


@pytest.mark.parametrize("name", ["c1", "c2"])
def test_cold_and_warm_seed_golden(name):
    """After a reset (the word at -1: the seed only grows within the frame) and again without one (the word holds
    the frame's depth from the start): the reference's frame and stats both times."""
    fx = load_frame(name)
    with sf.Sphereflake(fx["W"], fx["H"]) as s:
        s.SetCamera(sf.config_camera(fx["W"], fx["H"], float.fromhex(fx["K"])))
        s.reset_stats()
        for what in ("cold", "warm"):
            s.Render(emit_aux=True)
            assert_golden(fx, s.download(aux=True), s.stats(), (name, what))


@pytest.mark.parametrize("seed", CATCH)
def test_cold_and_warm_seed_occluded_deepest_node(seed):
    """The same on the views whose deepest node is occluded (CATCH), against the oracle."""
    view, (w, h), ref = reference(("seed", seed))
    with sf.Sphereflake(w, h) as s:
        s.SetView(*view)
        s.reset_stats()
        for what in ("cold", "warm"):
            s.Render(emit_aux=True)
            st = s.stats()
            assert_oracle(s.download(aux=True), st, ref, (seed, what))
            assert np.float32(st.closest) == np.float32(ref["stats"]["closest"])


@pytest.mark.parametrize("key", [("config", "c1"), ("config", "c2")] + [("seed", k) for k in sorted(set(range(8)) | set(CATCH))])
def test_seed_on_off_identical(key, monkeypatch):
    """The seed switched off (SF_FLAGS=0x10: every tile's depth bound from 0, as before the seed) and on: the same
    G-buffer, minT, hit index, max depth, closest and rays, bit for bit, on the render after a reset and on the next;
    and, seed on, the oracle's."""
    view, (w, h), ref = reference(key)
    out = {}
    for flags in (NO_SEED, 0):
        monkeypatch.setenv("SF_FLAGS", hex(flags))
        with sf.Sphereflake(w, h) as s:
            s.SetView(*view)
            s.reset_stats()
            frames = []
            for _ in range(2):
                s.Render(emit_aux=True)
                frames.append((s.download(aux=True), s.stats()))
            out[flags] = frames
    for k, ((a, sa), (b, sb)) in enumerate(zip(out[NO_SEED], out[0])):
        for x, y in zip(a, b):
            assert np.array_equal(bits(x), bits(y)), (key, k)
        assert (sa.max_depth, sa.closest, sa.rays) == (sb.max_depth, sb.closest, sb.rays), (key, k)
        assert_oracle(b, sb, ref, (key, k))
        assert np.float32(sb.closest) == np.float32(ref["stats"]["closest"]), (key, k)
        assert sb.rays == (k + 1) * w * h


DEEP, SHALLOW = 0.22, 2.0   # camera scales: close to the flake (depth 9 at 256 x 144), and far outside it (depth 5)


def test_word_is_cumulative_until_reset():
    """A deep view, then a shallow one under the same word: the shallow frame is the oracle's and max_depth stays the
    deep view's (the seed then lies above everything the shallow frame reaches). After a reset the shallow view
    reports its own depth: the seed was cleared with the word."""
    vd, _, rd = reference(("scale", DEEP))
    vs, _, rs = reference(("scale", SHALLOW))
    deep, shallow = rd["stats"]["max_depth"], rs["stats"]["max_depth"]
    assert deep >= shallow + 2
    with sf.Sphereflake(W, H) as s:
        s.SetView(*vd)
        s.Render(emit_aux=True)
        assert_oracle(s.download(aux=True), s.stats(), rd, "deep")
        s.SetView(*vs)
        s.Render(emit_aux=True)
        assert_oracle(s.download(aux=True), s.stats(), rs, "shallow after deep", max_depth=deep)
        s.reset_stats()
        s.Render(emit_aux=True)
        st = s.stats()
        assert_oracle(s.download(aux=True), st, rs, "shallow after reset")
        assert np.float32(st.closest) == np.float32(rs["stats"]["closest"])


def test_word_per_slot_of_dist():
    """sf_dist with 3 slots, 6 frames: every slot context has a word of its own. Deep frames on slot 0 only: every
    frame is the oracle's, the combined stats hold the deep view's depth; after a reset, three shallow frames (one per
    slot) report the shallow view's."""
    vd, _, rd = reference(("scale", DEEP))
    vs, _, rs = reference(("scale", SHALLOW))
    with sf.SphereflakeDist(0, W, H, slots=3) as d:
        for k, (v, r) in enumerate([(vd, rd), (vs, rs), (vs, rs), (vd, rd), (vs, rs), (vs, rs)]):
            d.SetView(*v)
            d.RenderBands()
            pos, nrm = d.download_slot(d.last_slot())
            assert np.array_equal(bits(pos), bits(r["pos4"])), k
            assert np.array_equal(bits(nrm), bits(r["nrm4"])), k
        st = d.stats()
        assert st.max_depth == rd["stats"]["max_depth"]
        assert np.float32(st.closest) == np.float32(min(rd["stats"]["closest"], rs["stats"]["closest"]))
        assert st.overflow_tiles == 0
        d.reset_stats()
        for k in range(3):
            d.SetView(*vs)
            d.RenderBands()
            pos, nrm = d.download_slot(d.last_slot())
            assert np.array_equal(bits(pos), bits(rs["pos4"])), k
        st = d.stats()
        assert st.max_depth == rs["stats"]["max_depth"]
        assert np.float32(st.closest) == np.float32(rs["stats"]["closest"])


@pytest.mark.parametrize("env", [{"SF_FLAGS": "0x400"}, {"SF_FLAGS": "0x400", "SF_TIE_INLINE": "0"},
                                 {"SF_FLAGS": "0x400", "SF_LEVELS": "3"}],
                         ids=["inline", "fixup", "low_levels"])
def test_seed_through_retrace_and_fixup(env, monkeypatch):
    """Every tile of c1 through the index-order re-trace (SF_FLAGS=0x400) -- by its own wave, by sf_fixup_wave
    (SF_TIE_INLINE=0), and with the levels forced below the frame's depth so that tiles overflow into sf_fixup_wave's
    deeper re-trace -- with the seed on: the reference's frame and stats, cold, warm and with the heavy-first order."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fx = load_frame("c1")
    with sf.Sphereflake(fx["W"], fx["H"]) as s:
        s.SetCamera(sf.config_camera(fx["W"], fx["H"], float.fromhex(fx["K"])))
        s.reset_stats()
        for k in range(3):
            s.Render(emit_aux=True)
            assert_golden(fx, s.download(aux=True), s.stats(), (env, k))
