"""CPU test that the inputs of tests/test_gpu_light_sweep.py (tests/lightsweep.py: the views of tests/sweepviews.py,
seeds 0..63, with five point lights, four suns, plain and spun AO and shafts per view) hold the cases the light traces
can go wrong on: lights and suns in every sign octant, entries with both outcomes on a real share of the surface, a
light inside the flake's ball (the t < 0 arm of the LOD predicate), views the two variants shadow differently, deep
traces (the overflow leg's), marched misses, views from inside a sphere. The oracle's masks cover every surface pixel
(and every marched miss), traced with the batch entry that tests/test_oracle_batch_host.py proves equal to the per-ray
path.

Every floor below is a condition on the sweep's inputs, not a measurement of the code under test, and lies well under
what this generator gives. Counted on whole frames by the oracle, AVX variant, bias 2^-10 (64 views); "both outcomes"
means the bit is set on at least 10 % and clear on at least 10 % of the view's surface pixels:
  views with at least 50 surface pixels (the views the next five rows count)       49            floor 40
  views where one of the four outside lights has both outcomes                      46 (98 of 196 entries)  floor 30
  the same for the four suns                                                        42 (113 of 196)         floor 30
  views where the inside light has both outcomes                                    13            floor 8
  views where a plain AO sample has both outcomes / a spun one                      49 (172) / 49 (192)     floor 40 each
  views where a shaft sample has both outcomes on the surface                       12 (20 entries)         floor 8
  views where a shaft sample has both outcomes (5 % each) on >= 50 marched misses   13 (21 entries)         floor 8
  views whose spun AO mask differs from the plain one                               56            floor 45
  views where light 0's bits at LOD 60 differ from those at LOD 70                  31            floor 8
  views whose masks differ between bias 0 and 2^-10: lights / suns / AO / shafts    55 / 53 / 56 / 3        (printed)
  deepest node of a point-light ray / a sun ray / an AO ray / a shaft ray           10 / 8 / 8 / 7          >= 6 each
  views with a trace whose deepest node is >= 6 (the GPU sweep's overflow leg)      56 (264 traces)         floor 45
  of those traces, the ones where a LIT ray expands a node of depth >= 6 before its
  bound (what an any-hit traversal must open: the leg's counter assertion)          237 on 56 views         floor 45 views
  views without a surface pixel (every mask all-lit)                                8             floor 5
  views where every ray hits at depth 0, the camera inside a sphere                 3 (seeds 31, 38, 57)    floor 3
  views with a negative min_t (surface points behind the camera)                    10            floor 6
  forced directions per sign octant                                                 24 each       24 each
(The generator was first counted on a 150-pixel sample per view: 49, 43 (99), 45 (117), 13, 17 and 7 / 8 for rows 1-4,
9 and 11; the whole frames give the numbers above.) If the generator changes, the counts are measured again and stated
here; a floor is never lowered to fit."""
import numpy as np
import pytest

import sphereflake_amd as sf
from sphereflake_amd import lights
import lightsweep as ls
from lightsweep import B10, COUNT, SEEDS, TRACES, sweep_entries, sweep_reference, sweep_view
from dirscheck import same_bits
from rayscheck import oracle_multi


@pytest.fixture(scope="module", autouse=True)
def built():
    sf.build()


@pytest.fixture(scope="module")
def surface():
    return {s: ls.surface_of(sweep_reference(s, "avx")["pos4"]) for s in SEEDS}


@pytest.fixture(scope="module")
def big(surface):
    return [s for s in SEEDS if int(surface[s].sum()) >= 50]


def views_with_both(trace, entries, seeds, where, variant="avx", share=0.10):
    """(views, entries) that have both outcomes on `share` of where(seed, i)."""
    views, total = 0, 0
    for s in seeds:
        m = ls.oracle_mask(s, variant, trace, B10)
        k = sum(ls.both_outcomes(m, i, where(s, i), share) for i in entries)
        views += k > 0
        total += k
    return views, total


def test_entries_are_what_the_generator_states():
    octants = np.zeros(8, int)
    for s in SEEDS:
        e = sweep_entries(s)
        o = np.asarray(sweep_view(s)[0][0], np.float64)
        assert e["lights"].shape == (5, 3) and e["suns"].shape == (4, 3) and e["lights"].dtype == np.float32
        norm = np.linalg.norm(e["lights"].astype(np.float64), axis=1)
        assert (norm[:4] > 2.49).all() and (norm[:4] < 8.01).all(), s     # outside the radius-2 ball
        assert 0.19 < norm[4] < 1.91, s                                       # inside it
        assert np.allclose(np.linalg.norm(e["suns"].astype(np.float64), axis=1), 1.0, atol=1e-6)
        assert np.allclose(e["lights"][:4] / norm[:4, None], e["suns"], atol=1e-6)
        assert np.dot(e["dirs"][0], o / np.linalg.norm(o)) > -0.5, s         # roughly towards the camera
        for i in (1, 2, 3):
            oc = (3 * s + i) % 8
            assert e["octants"][i - 1] == oc
            assert ls.octant_of(e["dirs"][i]) == ls.octant_of(e["suns"][i]) == ls.octant_of(e["lights"][i]) == oc
            assert (np.abs(e["suns"][i]) > 0.005).all()                      # no component near an octant's face
            octants[oc] += 1
        again = np.random.default_rng(11000 + s)   # the draws, in the stated order
        first = again.normal(size=3)
        assert same_bits(e["dirs"][0], ((o / np.linalg.norm(o) + 0.5 * first)
                                        / np.linalg.norm(o / np.linalg.norm(o) + 0.5 * first)).astype(np.float32))
    print("forced directions per octant", octants)
    assert (octants == 24).all()
    assert lights.ao_spins(3).shape[0] == 3 and 8 % 3 != 0


def test_batch_masks_equal_the_per_ray_oracle_on_a_view():
    """The masks are the per-ray oracle's (rayscheck.oracle_multi) on one small view, every trace: the sweep's
    gathering of rays, its scatter of min_t and its packing of bits, beside the batch entry's own test."""
    small = [s for s in SEEDS if sweep_view(s)[3] == (24, 16)]
    seed = max(small, key=lambda s: len(np.unique(ls.oracle_mask(s, "avx", "shadows", B10))))   # the most varied one
    children = sweep_view(seed)[1]["children"]
    for trace in TRACES:
        Fo, d, bound, on = ls.model(seed, "avx", trace, B10)
        want = np.zeros(on.shape[1:], np.uint64)
        for i in range(COUNT[trace]):
            origins = np.broadcast_to(Fo[i], d[i].shape)[on[i]]
            r = oracle_multi(children, origins, d[i][on[i]], lod=70.0)
            lit = np.ones(on.shape[1:], bool)
            with np.errstate(invalid="ignore"):
                lit[on[i]] = ~(r["minT"] < bound[i][on[i]])
            want |= lit.astype(np.uint64) << np.uint64(i)
        got = ls.oracle_mask(seed, "avx", trace, B10)
        assert not ls.mask_difference(seed, "avx", trace, B10, got, want)
        assert len(np.unique(got)) >= (3 if trace == "shadows" else 2), trace   # (no constant image)


def test_masks_have_the_shape_the_traces_promise():
    """Bits n..63 are 0; a pixel without a ray has exactly its low n bits set (for the shafts: per sample)."""
    for s in SEEDS:
        for v in ls.VARIANTS:
            surf = ls.surface_of(sweep_reference(s, v)["pos4"])
            for trace in TRACES:
                m = ls.oracle_mask(s, v, trace, B10)
                n = COUNT[trace]
                assert m.shape == surf.shape and (m >> np.uint64(n) == 0).all()
                if trace != "shafts":
                    assert (m[~surf] == ls.low(n)).all()
            _, far, tau = ls.shaft_inputs(s, v)
            assert far > 0 and tau > 2.0   # (lights.shaft_distance: every sample's ray starts outside the ball)


def test_sweep_has_lights_and_suns_with_both_outcomes(surface, big):
    where = lambda s, i: surface[s]
    lv, le = views_with_both("shadows", range(4), big, where)
    sv, se = views_with_both("suns", range(4), big, where)
    iv, _ = views_with_both("shadows", [4], big, where)
    print(f"views with >= 50 surface pixels {len(big)}; an outside light with both outcomes: {lv} views, {le} of"
          f" {4 * len(big)} entries; a sun: {sv} views, {se} entries; the inside light: {iv} views")
    assert len(big) >= 40
    assert lv >= 30
    assert sv >= 30
    assert iv >= 8


def test_sweep_has_ao_and_shafts_with_both_outcomes(surface, big):
    where = lambda s, i: surface[s]
    av, ae = views_with_both("ao", range(4), big, where)
    pv, pe = views_with_both("ao_spin", range(4), big, where)
    fv, fe = views_with_both("shafts", range(4), big, where)

    def marched(s, i):
        on = ls.model(s, "avx", "shafts", B10)[3][i]
        w = on & ~surface[s]
        return w if int(w.sum()) >= 50 else np.zeros_like(w)
    mv, me = views_with_both("shafts", range(4), SEEDS, marched, share=0.05)
    differ = [s for s in SEEDS if (ls.oracle_mask(s, "avx", "ao", B10) != ls.oracle_mask(s, "avx", "ao_spin", B10)).any()]
    print(f"AO with both outcomes: plain {av} views ({ae} entries), spun {pv} ({pe}); shafts on the surface {fv} ({fe}),"
          f" on marched misses {mv} ({me}); spun mask differs from the plain one on {len(differ)} views")
    assert av >= 40 and pv >= 40
    assert fv >= 8
    assert mv >= 8
    assert len(differ) >= 45


def test_variants_and_biases_shadow_differently():
    lod = [s for s in SEEDS if (ls.bit(ls.oracle_mask(s, "avx", "shadows", B10), 0)
                                != ls.bit(ls.oracle_mask(s, "sse", "shadows", B10), 0)).any()]
    print(f"light 0's bits at LOD 60 differ from LOD 70 on {len(lod)} views: {lod}")
    assert len(lod) >= 8
    for trace in TRACES:
        n = sum(bool((ls.oracle_mask(s, "avx", trace, 0.0) != ls.oracle_mask(s, "avx", trace, B10)).any()) for s in SEEDS)
        print(f"{trace}: the masks at bias 0 and 2^-10 differ on {n} views")


def test_sweep_has_deep_traces_for_the_overflow_leg():
    deep = {t: max(ls.deepest(s, "avx", t) for s in SEEDS) for t in TRACES}
    views = [s for s in SEEDS if any(ls.deepest(s, "avx", t) >= 6 for t in TRACES)]
    traces = [(s, t) for s in SEEDS for t in TRACES if ls.deepest(s, "avx", t) >= 6]
    needed = [(s, t) for s, t in traces if ls.deepest_needed(s, "avx", t) >= 6]
    print(f"deepest node per trace {deep}; views with a trace of depth >= 6: {len(views)} ({len(traces)} traces); with a"
          f" lit ray that needs depth >= 6 before its bound: {len(needed)} traces on {len({s for s, _ in needed})} views")
    assert all(d >= 6 for d in deep.values())
    assert len(views) >= 45
    assert len({s for s, _ in needed}) >= 45
    assert {t for _, t in needed} == set(TRACES)
    for s in SEEDS:
        for t in TRACES:
            assert ls.deepest_needed(s, "avx", t) <= ls.deepest(s, "avx", t)


def test_sweep_has_empty_and_inside_views(surface):
    frames = {s: sweep_reference(s, "avx") for s in SEEDS}
    empty = [s for s in SEEDS if not surface[s].any()]
    inside = [s for s in SEEDS if frames[s]["stats"]["hits"] == frames[s]["stats"]["rays"]
              and frames[s]["stats"]["max_depth"] == 0]
    negative = [s for s in SEEDS if (frames[s]["minT"] < 0).any()]
    print(f"no surface pixel: {empty}; every ray hits at depth 0: {inside}; a negative min_t: {negative}")
    assert len(empty) >= 5
    assert len(inside) >= 3
    assert len(negative) >= 6
    for s in empty:   # every mask all-lit
        for trace in ("shadows", "suns", "ao", "ao_spin"):
            assert (ls.oracle_mask(s, "avx", trace, B10) == ls.low(COUNT[trace])).all()
