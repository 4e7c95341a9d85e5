"""Temporal accumulation of the light buffer without a GPU: sf_reproject_matrix against lights.reproject_matrix, the
reprojection on the oracle's frames (same view: every tap is the pixel itself; moved views: taps accepted, rejected and
off the image), lights.light_accumulate_model's edge cases by hand, the quality claim on the oracle, the spin table's
phase, the header, the exports and the struct layout."""
import ctypes
import pathlib
import shutil

import numpy as np
import pytest

import sphereflake_amd as sf
from sphereflake_amd import lights
from abicheck import defined_symbols
from oracle import pyoracle
from dirscheck import same_bits
from rayscheck import frame
from sweepviews import SEEDS, sweep_view
import aospincheck as sc
import accumcheck as ak

F = np.float32
SYMBOLS = ("sf_reproject_matrix", "sf_light_accumulate_defaults", "sf_light_accumulate_to", "sf_light_accumulate",
           "sf_light_history_reset")
SETUPS = ("t1", "t2", "t3", "t4", "t5", "s1", "s2", "s3", "s4", "c1", "c2", "c3", "c4", "c5")


@pytest.fixture(scope="module", autouse=True)
def built():
    sf.build()


def c_matrix(view):
    v = np.ascontiguousarray(view, F).reshape(12)
    m = np.full(9, 7.0, F)
    fp = ctypes.POINTER(ctypes.c_float)
    rc = sf.lib().sf_reproject_matrix(v.ctypes.data_as(fp), m.ctypes.data_as(fp))
    return rc, m


# ---- the matrix ---------------------------------------------------------------------------------------
def test_reproject_matrix_equals_the_host_statement():
    """The 14 golden setups and the loop sweep's 64 seeded views: the library's matrix is lights.reproject_matrix's bit
    for bit, and m [a b c] is the identity within 1e-5."""
    views = [np.concatenate(ak.view_of(pyoracle.load_setup(n))) for n in SETUPS]
    views += [np.concatenate([np.asarray(x, F).reshape(3) for x in sweep_view(seed)[0]]) for seed in SEEDS]
    assert len(views) == 14 + 64
    worst = 0.0
    for v in views:
        rc, m = c_matrix(v)
        assert rc == sf.SF_OK
        assert same_bits(m, lights.reproject_matrix(v)) and same_bits(m, sf.reproject_matrix(v))
        o, tl, tr, bl = v[0:3], v[3:6], v[6:9], v[9:12]
        cols = np.stack([tr - tl, bl - tl, tl - o], axis=-1).astype(np.float64)
        err = float(np.abs(m.reshape(3, 3).astype(np.float64) @ cols - np.eye(3)).max())
        worst = max(worst, err)
        assert err <= 1e-5, (v, err)
    print("largest |m [a b c] - I| entry over the 78 views: %.3g" % worst)


def test_reproject_matrix_errors():
    """A null pointer, an input that is not finite and a view that spans no volume: SF_EINVAL, m not written."""
    v = np.concatenate(ak.view_of(pyoracle.load_setup("t3")))
    L = sf.lib()
    fp = ctypes.POINTER(ctypes.c_float)
    m = np.zeros(9, F)
    assert L.sf_reproject_matrix(None, m.ctypes.data_as(fp)) == sf.SF_EINVAL
    assert L.sf_reproject_matrix(v.ctypes.data_as(fp), None) == sf.SF_EINVAL
    for k in (0, 5, 11):
        for bad in (np.nan, np.inf, -np.inf):
            w = v.copy()
            w[k] = bad
            rc, m = c_matrix(w)
            assert rc == sf.SF_EINVAL and (m == 7).all()
            with pytest.raises(ValueError):
                lights.reproject_matrix(w)
    flat = v.copy()
    flat[9:12] = flat[6:9]          # bl == tr: a and b are parallel, the determinant is 0
    rc, m = c_matrix(flat)
    assert rc == sf.SF_EINVAL and (m == 7).all()
    eye = v.copy()
    eye[0:3] = eye[3:6]             # the origin on the top-left corner: c == 0
    assert c_matrix(eye)[0] == sf.SF_EINVAL
    with pytest.raises(ValueError):
        lights.reproject_matrix(flat)
    with pytest.raises(ValueError):
        lights.reproject_matrix(v[:11])


# ---- the reprojection on the oracle's frames --------------------------------------------------------------
@pytest.mark.parametrize("name", ["t1", "t2", "t3", "t4", "t5"])
def test_same_view_taps_the_pixel_itself(name):
    """The history's view equal to the current one: t = p on every surface pixel, no tap at a miss; with a history
    of .w = 1 every surface pixel is accepted and becomes h + (in - h) / 2."""
    S, f = pyoracle.load_setup(name), frame(name)
    pos, nrm = f["pos4"], f["nrm4"]
    surf = sc.surface_of(pos)
    H, W = surf.shape
    rng = np.random.default_rng(5)
    new, old = rng.random((H, W, 4)).astype(F), rng.random((H, W, 4)).astype(F)
    old[..., 3] = 1.0
    out, acc, taps = lights.light_accumulate_model(new, pos, nrm, S["origin"], old, pos, nrm, ak.view_of(S))
    yy, xx = np.mgrid[0:H, 0:W]
    assert ((taps[..., 0] == xx) & (taps[..., 1] == yy))[surf].all() and (taps[~surf] == -1).all()
    assert np.array_equal(acc, surf)
    want = old[..., :3] + (new[..., :3] - old[..., :3]) / F(2.0)
    assert same_bits(out[surf][:, :3], want[surf]) and (out[surf][:, 3] == 2).all()
    assert same_bits(out[~surf][:, :3], new[~surf][:, :3]) and (out[~surf][:, 3] == 0).all()


# (accepted, surface pixels, surface pixels whose tap is off the image), measured on the oracle at the defaults
MEASURED = {("t1", "right", 0.01): (536, 836, 0), ("t1", "fwd", 0.03): (632, 841, 0),
            ("t3", "right", 0.01): (2131, 3600, 215), ("t3", "fwd", 0.03): (2187, 3600, 0),
            ("t3", "right", 0.03): (1737, 3600, 670)}


def pair_model(name, direction, distance, hist=None):
    S, f = ak.moved_frame(name, direction, distance)
    hS, hf = pyoracle.load_setup(name), frame(name)
    if hist is None:
        hist = np.ones(hf["pos4"].shape, F)
    new = np.full(f["pos4"].shape, 3.0, F)
    return (f, hf) + lights.light_accumulate_model(new, f["pos4"], f["nrm4"], S["origin"], hist, hf["pos4"], hf["nrm4"],
                                                   ak.view_of(hS))


@pytest.mark.parametrize("pair", ak.PAIRS, ids=lambda p: "%s-%s-%g" % p)
def test_moved_views_accept_and_reject(pair):
    """The current frame is the moved view, the history the fixture's: at the default thresholds at least 25 % of the
    surface pixels keep their history and at least 15 % lose it; t3 moved right by 0.03 has at least 100 taps off the
    image. Measured on the oracle (accepted / surface, off the image): t1 right 0.01 536 / 836, t1 fwd 0.03 632 / 841,
    t3 right 0.01 2131 / 3600 (215 off), t3 fwd 0.03 2187 / 3600, t3 right 0.03 1737 / 3600 (670 off)."""
    f, hf, out, acc, taps = pair_model(*pair)
    surf = sc.surface_of(f["pos4"])
    n, kept = int(surf.sum()), int(acc.sum())
    off = int((surf & (taps[..., 0] < 0)).sum())
    print(pair, "accepted", kept, "/", n, "taps off the image", off)
    assert not acc[~surf].any()
    assert kept >= 0.25 * n and n - kept >= 0.15 * n
    if pair == ("t3", "right", 0.03):
        assert off >= 100
    assert (kept, n, off) == MEASURED[pair]
    # the two endings: (1 + (3 - 1) / 2, 2) where accepted, (3, 1) elsewhere on the surface, (3, 0) at a miss
    assert (out[acc] == np.array([2, 2, 2, 2], F)).all() and (out[surf & ~acc] == np.array([3, 3, 3, 1], F)).all()
    assert (out[~surf] == np.array([3, 3, 3, 0], F)).all()


def test_every_branch_is_exercised_by_the_pairs():
    """Over the five pairs each way a surface pixel can lose its history occurs: no tap (off the image), a tap that is
    a miss of the history's frame, a history count below 1, a normal too far off, a point off the tangent plane."""
    seen = dict(off=0, miss=0, count=0, normal=0, plane=0, kept=0)
    for pair in ak.PAIRS:
        name = pair[0]
        hist = ak.seeded_history(frame(name)["pos4"].shape[:2], 3)
        f, hf, out, acc, taps = pair_model(*pair, hist=hist)
        S, hS = ak.moved_frame(*pair)[0], pyoracle.load_setup(name)
        surf = sc.surface_of(f["pos4"])
        has = surf & (taps[..., 0] >= 0)
        x, y = np.where(has, taps[..., 0], 0), np.where(has, taps[..., 1], 0)
        Pq, Nq, h = hf["pos4"][y, x, :3], hf["nrm4"][y, x, :3], hist[y, x]
        N, P = f["nrm4"][..., :3], f["pos4"][..., :3]
        there = sc.surface_of(hf["pos4"])[y, x]
        with np.errstate(invalid="ignore"):
            counted = h[..., 3] >= 1
            nn = (N[..., 0] * Nq[..., 0] + N[..., 1] * Nq[..., 1]) + N[..., 2] * Nq[..., 2]
            E = (hS["origin"] + Pq) - (S["origin"] + P)
            e = (N[..., 0] * E[..., 0] + N[..., 1] * E[..., 1]) + N[..., 2] * E[..., 2]
            pp = (P[..., 0] * P[..., 0] + P[..., 1] * P[..., 1]) + P[..., 2] * P[..., 2]
            near = nn >= F(0.9)
            flat = (e * e) <= (F(0.02) * F(0.02)) * pp
        assert np.array_equal(acc, has & there & counted & near & flat)   # the rule, restated on its own
        seen["off"] += int((surf & ~has).sum())
        seen["miss"] += int((has & ~there).sum())
        seen["count"] += int((has & there & ~counted).sum())
        seen["normal"] += int((has & there & counted & ~near).sum())
        seen["plane"] += int((has & there & counted & near & ~flat).sum())
        seen["kept"] += int(acc.sum())
        # .w of the seeded history: min(h.w + 1, 16) where kept
        assert (out[acc][:, 3] == np.minimum(h[acc][:, 3] + F(1.0), F(16.0))).all()
    print(seen)
    assert min(seen.values()) >= 20, seen


# ---- the model by hand -----------------------------------------------------------------------------------
def wall(h=4, w=6, z=4.0):
    """A view looking down +z from the origin onto a wall at depth z that fills the image exactly: pixel (x, y)'s
    ray is a u + b v + c with u = x / w, v = y / h, so its wall point reprojects to itself."""
    view = (np.zeros(3, F), np.array([-1, -1, 1], F), np.array([1, -1, 1], F), np.array([-1, 1, 1], F))
    u = (np.arange(w, dtype=F) / F(w))[None, :]
    v = (np.arange(h, dtype=F) / F(h))[:, None]
    pos = np.zeros((h, w, 4), F)
    pos[..., 0] = (F(-1.0) + F(2.0) * u) * F(z)
    pos[..., 1] = (F(-1.0) + F(2.0) * v) * F(z)
    pos[..., 2] = F(z)
    nrm = np.zeros((h, w, 4), F)
    nrm[..., 2] = F(-1.0)
    return view, pos, nrm


def test_model_by_hand_and_its_edge_cases():
    """The blend and its count by hand; a history count of 0, of NaN and above max_history; a miss in either frame;
    NaN positions and normals; q.z <= 0; max_history = 1 is h + (in - h), not `in`."""
    view, pos, nrm = wall()
    assert np.array_equal(lights.reproject_matrix(view), np.array([0.5, 0, 0.5, 0, 0.5, 0.5, 0, 0, 1], F))
    rng = np.random.default_rng(2)
    new, old = rng.random((4, 6, 4)).astype(F), rng.random((4, 6, 4)).astype(F)
    old[..., 3] = 3.0
    old[0, 1, 3] = 0.0          # never written: rejected
    old[0, 2, 3] = np.nan       # a NaN count: rejected
    old[0, 3, 3] = 70000.0      # above max_history: clamped
    old[0, 4, 3] = 0.5          # below 1: rejected
    old[0, 5, 3] = 16.0         # at max_history: stays there
    hp, hn, p2, n2 = pos.copy(), nrm.copy(), pos.copy(), nrm.copy()
    hp[1, 0, :3] = 0.0          # a miss of the history's frame
    p2[1, 1, :3] = 0.0          # a miss of the current frame
    p2[1, 2, 0] = np.nan        # a NaN position: no tap
    n2[1, 3, 1] = np.nan        # a NaN normal: rejected
    hn[1, 4, 2] = np.nan        # a NaN normal in the history: rejected
    hp[1, 5, 1] = np.nan        # a NaN position in the history: rejected by the plane test
    p2[2, 0, 2] = F(-4.0)       # behind the history's viewer: q.z <= 0, no tap
    out, acc, taps = lights.light_accumulate_model(new, p2, n2, view[0], old, hp, hn, view)
    blend = lambda y, x, m: np.append(old[y, x, :3] + (new[y, x, :3] - old[y, x, :3]) / F(m), F(m))
    fresh = lambda y, x: np.append(new[y, x, :3], F(1.0))
    assert same_bits(out[0, 0], blend(0, 0, 4)) and acc[0, 0] and tuple(taps[0, 0]) == (0, 0)
    assert same_bits(out[3, 5], blend(3, 5, 4)) and tuple(taps[3, 5]) == (5, 3)
    for x in (1, 2, 4):
        assert same_bits(out[0, x], fresh(0, x)) and not acc[0, x] and tuple(taps[0, x]) == (x, 0)
    assert same_bits(out[0, 3], blend(0, 3, 16)) and same_bits(out[0, 5], blend(0, 5, 16))
    assert same_bits(out[1, 0], fresh(1, 0)) and tuple(taps[1, 0]) == (0, 1)
    assert same_bits(out[1, 1], np.append(new[1, 1, :3], F(0.0))) and tuple(taps[1, 1]) == (-1, -1)
    assert same_bits(out[1, 2], fresh(1, 2)) and tuple(taps[1, 2]) == (-1, -1)
    for x in (3, 4, 5):
        assert same_bits(out[1, x], fresh(1, x)) and not acc[1, x] and tuple(taps[1, x]) == (x, 1)
    assert same_bits(out[2, 0], fresh(2, 0)) and tuple(taps[2, 0]) == (-1, -1)
    assert int(acc.sum()) == 24 - 10
    # max_history = 1: h + (in - h) / 1, which is not `in` to the last bit everywhere
    one = lights.light_accumulate_model(new, pos, nrm, view[0], old, pos, nrm, view, 1)[0]
    assert same_bits(one[2, 2, :3], old[2, 2, :3] + (new[2, 2, :3] - old[2, 2, :3])) and (one[..., 3] == 1).all()
    small, unit = np.full((4, 6, 4), F(2.0 ** -30), F), np.ones((4, 6, 4), F)
    one = lights.light_accumulate_model(small, pos, nrm, view[0], unit, pos, nrm, view, 1)[0]
    assert (one[..., :3] == 0).all()   # 1 + (2^-30 - 1) = 1 + -1
    # a history of .w = 0 everywhere: the first frame needs no special case
    first = lights.light_accumulate_model(new, pos, nrm, view[0], np.zeros_like(old), pos, nrm, view)
    assert same_bits(first[0][..., :3], new[..., :3]) and (first[0][..., 3] == 1).all() and not first[1].any()
    # a tap off the image: the same wall seen from a history view turned to the side
    side = (view[0], view[1] + F(3.0) * np.array([1, 0, 0], F), view[2] + F(3.0) * np.array([1, 0, 0], F),
            view[3] + F(3.0) * np.array([1, 0, 0], F))
    out, acc, taps = lights.light_accumulate_model(new, pos, nrm, view[0], old, pos, nrm, side)
    assert not acc.any() and (taps == -1).all() and same_bits(out[..., :3], new[..., :3]) and (out[..., 3] == 1).all()
    for bad in (dict(max_history=0), dict(max_history=65536), dict(normal_min=np.nan), dict(plane_max=-1.0),
                dict(plane_max=np.inf)):
        with pytest.raises(ValueError):
            lights.light_accumulate_model(new, pos, nrm, view[0], old, pos, nrm, view, **bad)


def test_still_view_is_the_running_mean():
    """K calls from a still view with max_history >= K: .w = K and the mean of the K inputs, rounded in step 5's order;
    past max_history an exponential average with weight 1 / max_history."""
    view, pos, nrm = wall()
    rng = np.random.default_rng(8)
    frames = rng.random((20, 4, 6, 4)).astype(F)
    hist = np.zeros((4, 6, 4), F)
    mean = np.zeros((4, 6, 3), F)
    for k in range(16):
        hist = lights.light_accumulate_model(frames[k], pos, nrm, view[0], hist, pos, nrm, view, 16)[0]
        mean = mean + (frames[k][..., :3] - mean) / F(k + 1) if k else frames[k][..., :3].copy()
        assert same_bits(hist[..., :3], mean) and (hist[..., 3] == k + 1).all()
    # (at most three roundings of 2^-24 per step on values below 1, 16 steps)
    assert np.abs(hist[..., :3].astype(np.float64) - frames[:16, ..., :3].astype(np.float64).mean(0)).max() < 3e-6
    for k in range(16, 20):
        nxt = lights.light_accumulate_model(frames[k], pos, nrm, view[0], hist, pos, nrm, view, 16)[0]
        assert same_bits(nxt[..., :3], hist[..., :3] + (frames[k][..., :3] - hist[..., :3]) / F(16.0))
        assert (nxt[..., 3] == 16).all()
        hist = nxt


# ---- the quality claim, on the oracle ------------------------------------------------------------------------
def test_sixteen_accumulated_frames_beat_one():
    """t3 (80 x 45, 3600 surface pixels), ao_samples(4) under ao_spins(4, ao_phase(k)), colours 1 / n, tau = 4, bias
    2^-10, max_history 16, default thresholds; RMS error of the open fraction against the unspun n = 64 sum at the
    last view, unfiltered / after light_filter_model(4). Measured on the oracle:
        single frame, phase 0 (ao_spins(4))           0.1697 / 0.1043
        single frame, frame 15's phase                0.1682 / 0.1058
        16 frames, camera moving 0.0005 per frame     0.1059 / 0.0928   (2619 of 3600 pixels keep their history)
        16 frames, still camera                       0.0492 / 0.0538
    The issue's figures for the moving camera are 0.1061 / 0.0929: the directions fwd and right are formed here in
    float64 and rounded once with the distance, which moves the views in their last bits; the still figures agree."""
    f = frame("t3")
    pos, nrm = f["pos4"], f["nrm4"]
    surf = sc.surface_of(pos)
    truth = ak.truth64("t3")
    filt = lambda b: lights.light_filter_model(b, pos, nrm, 4)
    err = lambda b: (sc.rms(b, truth, surf), sc.rms(filt(b), truth, surf))
    single0 = err(ak.oracle_sum(pyoracle.load_setup("t3"), f, ak.H4, lights.ao_spins(4)))
    single = err(ak.spun_sum("t3", "path", 0.0, 15))
    moving_buf, kept = ak.accumulate_path([ak.path_view(k) for k in range(ak.PATH_FRAMES)])
    still_buf, kept_still = ak.accumulate_path([("path", 0.0)] * ak.PATH_FRAMES)
    moving, still = err(moving_buf), err(still_buf)
    print("RMS error against n = 64, unfiltered / filtered: single (phase 0) %.4f / %.4f, single (frame 15) %.4f / %.4f,"
          " moving %.4f / %.4f (%d of %d keep their history), still %.4f / %.4f"
          % (single0 + single + moving + (int(kept.sum()), int(surf.sum())) + still))
    assert int(surf.sum()) == 3600 and ak.path_view(15) == ("path", 0.0)
    assert np.array_equal(kept_still, surf) and (still_buf[surf][:, 3] == 16).all()
    for one in (single0, single):
        assert moving[0] < one[0] and moving[1] < one[1]
        assert still[0] < one[0] and still[1] < one[1]
    assert still[0] < moving[0] and still[1] < moving[1]


# ---- the spin table's phase --------------------------------------------------------------------------------
def test_spin_phase():
    """phase 0 is today's table bit for bit, sizes 1..8; a phase turns every entry by 2 pi phase; ao_phase steps by the
    plastic number's reciprocal and not by the golden ratio."""
    for size in range(1, 9):
        base = lights.ao_spins(size)
        assert same_bits(lights.ao_spins(size, 0.0), base) and same_bits(lights.ao_spins(size, phase=0), base)
        turned = lights.ao_spins(size, 0.25).astype(np.float64)   # a quarter turn: (c, s) -> (-s, c)
        assert np.abs(turned[..., 0] + base[..., 1]).max() < 1e-6 and np.abs(turned[..., 1] - base[..., 0]).max() < 1e-6
    assert lights.ao_phase(0) == 0.0
    assert lights.ao_phase(1) == 0.7548776662466927
    assert abs(lights.ao_phase(2) - 0.5097553324933854) < 1e-15
    assert all(0.0 <= lights.ao_phase(k) < 1.0 for k in range(64))
    assert abs(lights.AO_PHASE_STEP - (np.sqrt(5.0) - 1.0) / 2.0) > 0.1
    assert "golden" in lights.ao_phase.__doc__.lower()
    with pytest.raises(ValueError):
        lights.ao_spins(4, np.nan)


# ---- the header, the library ---------------------------------------------------------------------------
def test_header_states_the_definition():
    text = " ".join(pathlib.Path(sf.HEADER_PATH).read_text().split())
    for sym in SYMBOLS + ("sf_light_accumulate_params",):
        assert sym in text, sym
    assert "#define SF_ABI_VERSION 1" in text
    assert "q.k = ((m[3k] D.x) + (m[3k+1] D.y)) + (m[3k+2] D.z)" in text
    assert "fx = (u (float)W) + 0.5f, fy = (v (float)H) + 0.5f" in text
    assert "nn = ((N.x N'.x) + (N.y N'.y)) + (N.z N'.z)" in text
    assert "E = (o' + P') - w per component, e = ((N.x E.x) + (N.y E.y)) + (N.z E.z)" in text
    assert "m = min(h.w + 1.0f, (float)max_history); per channel out.c = h.c + ((in.c - h.c) / m)" in text
    assert "Otherwise out[p] = (in[p].xyz, 1)" in text
    assert "det = ((a.x bc.x) + (a.y bc.y)) + (a.z bc.z)" in text
    assert "WHICH IS NOT `in` TO THE LAST BIT" in text


def test_symbols_are_exported():
    if shutil.which("nm") is None:
        pytest.skip("binutils not available")
    have = defined_symbols(sf.LIB_PATH)
    assert set(SYMBOLS) <= have and set(SYMBOLS) <= set(sf.SIGNATURES)


def test_struct_layout_and_errors_without_a_device():
    P = sf.sf_light_accumulate_params
    assert ctypes.sizeof(P) == 96
    assert (P.max_history.offset, P.normal_min.offset, P.plane_max.offset, P.origin.offset, P.use_origin.offset,
            P.hist_origin.offset, P.hist_m.offset, P.width.offset, P.height.offset, P.stream.offset) \
        == (0, 4, 8, 12, 24, 28, 40, 76, 80, 88)
    L = sf.lib()
    p = P()
    p.max_history = 7
    buf = (ctypes.c_float * 64)()
    vp = ctypes.cast(buf, ctypes.c_void_p)
    assert L.sf_light_accumulate_defaults(None, ctypes.byref(p)) == sf.SF_EINVAL and p.max_history == 7
    assert L.sf_light_accumulate_to(None, ctypes.byref(p), vp, vp, vp, vp, vp, vp, vp) == sf.SF_EINVAL
    assert L.sf_light_accumulate(None, ctypes.byref(p)) == sf.SF_EINVAL
    assert L.sf_light_history_reset(None) == sf.SF_EINVAL
    assert sf.lib().sf_abi_version() == 1
