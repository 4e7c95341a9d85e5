"""The LOD constant of the shadow traces on the GPU (sf_set_shadow_lod): trace_sun, trace_shadow and trace_shadows
follow it bit for bit with the oracle at the same constant, and nothing else does -- renders, their statistics and the
closest-hit ray traces keep the variant's own."""
import math

import numpy as np
import pytest

import sphereflake_amd as sf
from sphereflake_amd import lights
from conftest import load_frame
from dirscheck import oracle_rays, same_bits
from oracle import pyoracle
from rayscheck import frame
from sfcheck import bad_rows, row_digests
import shadowcheck as sc
import suncheck as su

pytestmark = pytest.mark.gpu

C = su.matched()   # ~394.7: the camera's detail at t3's closest distance, for rays that start 4 away


@pytest.fixture(scope="module", autouse=True)
def device():
    sf.build()
    assert sf.device_count() >= 1, "no HIP device visible: GPU tests must run on an MI355X"


def flake(name, variant="avx"):
    S = pyoracle.load_setup(name)
    s = sf.Sphereflake(S["W"], S["H"])
    s.SetVariant(variant)
    s.SetView(S["origin"], S["tl"], S["tr"], S["bl"])
    return s


def oracle_shadow_vis(name, light, bias, lod):
    """shadowcheck.oracle_vis at another LOD constant: the light-side rays of the fixture's own frame."""
    S = pyoracle.load_setup(name)
    pos = frame(name)["pos4"]
    d, _, surf = lights.shadow_model(pos, S["origin"], light, 0.0)
    mint = np.full(surf.shape, su.FLT_MAX, np.float32)
    mint[surf] = oracle_rays(sf.root_transform(np.asarray(light, np.float32)), S["children"], d[surf], lod=lod)["minT"]
    return sc.vis_of(pos, S["origin"], light, bias, mint)


def test_sun_follows_the_constant_and_zero_restores_it():
    pos = frame("t3")["pos4"]
    s_dir = su.direction("cam")
    base, fine = su.oracle_vis("t3", "cam", su.B10), su.oracle_vis("t3", "cam", su.B10, lod=C)
    assert (base != fine).any() and (fine == 0).sum() >= 50 and (fine == 255).sum() >= 50
    with flake("t3") as s:
        assert s.get_shadow_lod() == 0.0
        assert np.array_equal(s.trace_sun(s_dir, su.TAU, bias=su.B10, pos=pos), base)
        s.set_shadow_lod(C)
        assert s.get_shadow_lod() == np.float32(C)
        got = s.trace_sun(s_dir, su.TAU, bias=su.B10, pos=pos)
        bad = np.argwhere(got != fine)
        assert bad.size == 0, f"{len(bad)} pixels differ from the oracle at lod {C}, first {bad[:4]}"
        assert (got != base).any()
        s.set_shadow_lod(0.0)
        assert np.array_equal(s.trace_sun(s_dir, su.TAU, bias=su.B10, pos=pos), base)
        s.set_shadow_lod(70.0)   # the variant's own, spelt out
        assert np.array_equal(s.trace_sun(s_dir, su.TAU, bias=su.B10, pos=pos), base)


def test_point_lights_follow_the_constant():
    """trace_shadow against the oracle at the constant; bit i of trace_shadows is trace_shadow(lights[i]) there too."""
    pos = frame("t3")["pos4"]
    names = ("side", "top", "low")
    L = np.array([sc.LIGHTS[n] for n in names], np.float32)
    with flake("t3") as s:
        s.set_shadow_lod(C)
        vis = [s.trace_shadow(L[i], bias=su.B10, pos=pos) for i in range(3)]
        mask = s.trace_shadows(L, bias=su.B10, pos=pos)
        s.set_shadow_lod(0.0)
        side0 = s.trace_shadow(L[0], bias=su.B10, pos=pos)
    fine = oracle_shadow_vis("t3", sc.LIGHTS["side"], su.B10, C)
    bad = np.argwhere(vis[0] != fine)
    assert bad.size == 0, f"{len(bad)} pixels differ from the oracle at lod {C}, first {bad[:4]}"
    assert np.array_equal(side0, sc.oracle_vis("t3", "side", su.B10)) and (side0 != fine).any()
    assert np.array_equal(mask, lights.masks_from_vis(vis))


def test_the_variant_keeps_its_own_default():
    """With the constant at 0 the SSE variant's shadow traces use 60; a set constant survives SetVariant."""
    pos = frame("t1", "sse")["pos4"]
    s_dir = su.direction("side")
    with flake("t1", "sse") as s:
        assert np.array_equal(s.trace_sun(s_dir, su.TAU, bias=su.B10, pos=pos),
                              su.oracle_vis("t1", "side", su.B10, variant="sse"))
        s.set_shadow_lod(C)
        s.SetVariant("avx")
        s.SetVariant("sse")
        assert s.get_shadow_lod() == np.float32(C)
        assert np.array_equal(s.trace_sun(s_dir, su.TAU, bias=su.B10, pos=pos),
                              su.oracle_vis("t1", "side", su.B10, variant="sse", lod=C))


def test_renders_and_ray_traces_do_not_see_it():
    """Render() before and after is the golden frame, the statistics are what two renders alone leave, and trace_rays
    (closest hit, the variant's constant) returns the same bits."""
    fx = load_frame("t3")
    ref = frame("t3")
    S = pyoracle.load_setup("t3")
    Fo, d, _, _ = lights.sun_model(ref["pos4"], S["origin"], su.direction("cam"), su.TAU, 0.0)
    with flake("t3") as s:   # what two renders alone leave
        s.Render(emit_aux=True)
        s.Render(emit_aux=True)
        s.Synchronize()
        st0 = s.stats()
        want = (st0.max_depth, np.float32(st0.closest), st0.rays, st0.overflow_tiles)
    with flake("t3") as s:
        s.Render(emit_aux=True)
        p, n, _, _ = s.download()
        assert bad_rows(fx["row_digest_gbuf"], row_digests(p, n)) == []
        s.set_shadow_lod(C)
        s.trace_sun(su.direction("cam"), su.TAU, bias=su.B10)
        s.Render(emit_aux=True)
        pos, nrm, mint, idx = s.download(aux=True)
        st = s.stats()
        assert (st.max_depth, np.float32(st.closest), st.rays, st.overflow_tiles) == want
        assert bad_rows(fx["row_digest_gbuf"], row_digests(pos, nrm)) == []
        for k, a in (("pos4", pos), ("nrm4", nrm), ("minT", mint), ("index", idx)):
            assert same_bits(a, ref[k]), f"Render under a shadow LOD constant: {k} differs"
        assert np.array_equal(s.download_shadow(), su.oracle_vis("t3", "cam", su.B10, lod=C))
        rays_fine = s.trace_rays(Fo.reshape(-1, 3), d)[2]
        s.set_shadow_lod(0.0)
        assert same_bits(s.trace_rays(Fo.reshape(-1, 3), d)[2], rays_fine)


def test_error_codes():
    L = sf.lib()
    with sf.Sphereflake(64, 36) as s:
        for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
            assert L.sf_set_shadow_lod(s.ctx, bad) == sf.SF_EINVAL
            with pytest.raises(Exception):
                s.set_shadow_lod(bad)
        assert s.get_shadow_lod() == 0.0
        assert L.sf_set_shadow_lod(s.ctx, 123.5) == sf.SF_OK and s.get_shadow_lod() == 123.5
        assert L.sf_set_shadow_lod(s.ctx, -0.0) == sf.SF_OK and s.get_shadow_lod() == 0.0
        assert L.sf_set_shadow_lod(None, 70.0) == sf.SF_EINVAL and math.isnan(L.sf_get_shadow_lod(None))
