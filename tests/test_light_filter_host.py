"""The edge-aware box filter of the light buffer without a GPU: lights.light_filter_model by hand on a 5 x 5 image, its
window, its NaN rules, the oracle condition tests/test_gpu_light_filter.py relies on, the header, the exports and the
struct layout."""
import ctypes
import pathlib
import shutil

import numpy as np
import pytest

import sphereflake_amd as sf
from sphereflake_amd import lights
from abicheck import defined_symbols
from dirscheck import same_bits
from rayscheck import frame
import aospincheck as sc

F = np.float32
SYMBOLS = ("sf_light_filter_defaults", "sf_light_filter_to", "sf_light_filter")


@pytest.fixture(scope="module", autouse=True)
def built():
    sf.build()


def plane(h=5, w=5, z=4.0):
    """A flat wall facing the viewer at depth z, one unit per 100 pixels: every tap passes both tests."""
    pos = np.zeros((h, w, 4), F)
    pos[..., 0] = (np.arange(w, dtype=F) * F(0.01))[None, :]
    pos[..., 1] = (np.arange(h, dtype=F) * F(0.01))[:, None]
    pos[..., 2] = F(z)
    nrm = np.zeros((h, w, 4), F)
    nrm[..., 2] = F(-1.0)
    return pos, nrm


def values(h=5, w=5):
    rng = np.random.default_rng(11)
    buf = (rng.uniform(0.0, 1.0, (h, w, 4)) * 2.0 ** rng.integers(-6, 1, (h, w, 1))).astype(F)
    buf[..., 3] = np.arange(h * w, dtype=F).reshape(h, w) + F(0.5)
    return buf


def by_hand(buf, taps):
    """The mean of the taps [(y, x), ...] in the order given, one rounding per operation."""
    S = np.zeros(3, F)
    for y, x in taps:
        S = S + buf[y, x, :3]
    return S / F(len(taps))


def test_window_order_and_mean_by_hand():
    """Every tap accepted: the window is -(R // 2) .. R - 1 - R // 2 in both directions, clipped at the image, summed
    dy outer and dx inner, divided once; .w is the pixel's own. R = 1 is a copy."""
    pos, nrm = plane()
    buf = values()
    assert same_bits(lights.light_filter_model(buf, pos, nrm, 1), buf)
    for R in (2, 3, 4, 8):
        out = lights.light_filter_model(buf, pos, nrm, R)
        lo, hi = -(R // 2), R - 1 - R // 2
        for y in range(5):
            for x in range(5):
                taps = [(y + dy, x + dx) for dy in range(lo, hi + 1) for dx in range(lo, hi + 1)
                        if 0 <= y + dy < 5 and 0 <= x + dx < 5]
                assert same_bits(out[y, x, :3], by_hand(buf, taps)), (R, y, x)
        assert same_bits(out[..., 3], buf[..., 3])
    # the order matters in binary32: the reversed sum differs somewhere, so the test above pins the order
    out = lights.light_filter_model(buf, pos, nrm, 4)
    rev = np.array([[by_hand(buf, [(y + dy, x + dx) for dy in range(1, -3, -1) for dx in range(1, -3, -1)
                                   if 0 <= y + dy < 5 and 0 <= x + dx < 5]) for x in range(5)] for y in range(5)])
    assert not same_bits(out[..., :3], rev)
    assert (-2, 1) == (-(4 // 2), 4 - 1 - 4 // 2)


def test_acceptance_by_hand():
    """A miss is copied and skipped as a tap; a tilted normal fails normal_min exactly at the threshold; a pixel off the
    tangent plane fails plane_max; the tests are one-sided (p's plane and p's |P|)."""
    pos, nrm = plane()
    buf = values()
    pos[1, 1, :3] = 0.0                                        # a miss of the frame
    nrm[2, 3, :3] = np.array([0.6, 0.0, -0.8], F)              # N_p . N_q = 0.8 against its neighbours
    pos[3, 1, 2] = F(4.5)                                      # half a unit behind the wall
    out = lights.light_filter_model(buf, pos, nrm, 3, 0.9, 0.02)
    assert same_bits(out[1, 1], buf[1, 1])
    taps = lambda y, x, skip: [(y + dy, x + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
                               if 0 <= y + dy < 5 and 0 <= x + dx < 5 and (y + dy, x + dx) not in skip]
    assert same_bits(out[0, 0, :3], by_hand(buf, taps(0, 0, {(1, 1)})))
    assert same_bits(out[2, 2, :3], by_hand(buf, taps(2, 2, {(1, 1), (2, 3), (3, 1)})))
    assert same_bits(out[2, 3, :3], buf[2, 3, :3])             # the tilted pixel keeps only itself (count 1: S / 1)
    assert same_bits(out[3, 1, :3], buf[3, 1, :3])             # and so does the one behind the wall
    assert same_bits(out[0, 4, :3], by_hand(buf, taps(0, 4, set())))
    # normal_min = 0.8 lets the tilted tap in where the plane test agrees: e = N_p . D is 0 for p on the wall
    out = lights.light_filter_model(buf, pos, nrm, 3, F(0.8), 0.02)
    assert same_bits(out[2, 2, :3], by_hand(buf, taps(2, 2, {(1, 1), (3, 1)})))
    # seen from the tilted pixel its neighbours leave its plane: e = 0.6 D.x, e e = 3.6e-5 > k2 pp only for a small k2
    k2pp = F(F(0.0001) * F(0.0001)) * F(F(F(0.03) * F(0.03) + F(0.02) * F(0.02)) + F(16.0))
    assert F(F(0.6) * F(0.01)) ** 2 > k2pp
    out = lights.light_filter_model(buf, pos, nrm, 3, F(0.8), 0.0001)
    assert same_bits(out[2, 3, :3], by_hand(buf, [(1, 3), (2, 3), (3, 3)]))   # only dx = 0 stays in its plane
    # a wider plane_max takes the pixel behind the wall back in: 0.5^2 <= (0.2^2) pp
    out = lights.light_filter_model(buf, pos, nrm, 3, 0.9, 0.2)
    assert same_bits(out[2, 2, :3], by_hand(buf, taps(2, 2, {(1, 1), (2, 3)})))
    for bad in (dict(size=0), dict(size=9), dict(size=4, normal_min=np.nan), dict(size=4, plane_max=-1.0),
                dict(size=4, plane_max=np.inf)):
        with pytest.raises(ValueError):
            lights.light_filter_model(buf, pos, nrm, **bad)


def test_nan_rules():
    """A NaN normal at q removes q from its neighbours' sums and leaves q averaging itself alone; a NaN light value
    spreads exactly to the pixels whose accepted window holds it."""
    pos, nrm = plane()
    buf = values()
    clean = lights.light_filter_model(buf, pos, nrm, 3)
    nrm2 = nrm.copy()
    nrm2[2, 2, 1] = np.nan
    out = lights.light_filter_model(buf, pos, nrm2, 3)
    assert same_bits(out[2, 2, :3], buf[2, 2, :3])
    taps = [(1 + dy, 1 + dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (1 + dy, 1 + dx) != (2, 2)]
    assert same_bits(out[1, 1, :3], by_hand(buf, taps))
    assert same_bits(out[0, 0], clean[0, 0]) and same_bits(out[4, 4], clean[4, 4]) and np.isfinite(out).all()
    buf2 = buf.copy()
    buf2[2, 2, 1] = np.nan
    out = lights.light_filter_model(buf2, pos, nrm, 3)
    hit = np.isnan(out[..., 1])
    want = np.zeros((5, 5), bool)
    want[1:4, 1:4] = True
    assert np.array_equal(hit, want) and np.isfinite(out[..., 0]).all() and np.isfinite(out[..., 2]).all()
    assert same_bits(out[..., 0], clean[..., 0])
    out = lights.light_filter_model(buf2, pos, nrm2, 3)   # the NaN value behind a NaN normal stays at home
    assert np.array_equal(np.isnan(out[..., 1]), (np.arange(25).reshape(5, 5) == 12))


def test_counts_helper_agrees_with_the_model():
    """aospincheck.accepted_counts restates the acceptance rule; a buffer of ones with one 2 in it moves exactly the
    pixels whose window accepts that pixel, by 1 / count."""
    f = frame("t3")
    pos, nrm = f["pos4"], f["nrm4"]
    cnt = sc.accepted_counts(pos, nrm, 4)
    surf = sc.surface_of(pos)
    ones = np.ones(pos.shape[:2] + (4,), F)
    base = lights.light_filter_model(ones, pos, nrm, 4)
    assert (base[..., 0] == 1).all()
    y, x = np.argwhere(cnt == 16)[40]
    ones[y, x, 0] = 2.0
    out = lights.light_filter_model(ones, pos, nrm, 4)
    moved = out[..., 0] != 1
    assert moved[y, x] and 2 <= int(moved.sum()) <= 16
    for yy, xx in np.argwhere(moved):
        if (yy, xx) != (y, x):
            assert out[yy, xx, 0] == F(F(cnt[yy, xx] + 1) / F(cnt[yy, xx])), (yy, xx)
    assert (cnt[~surf] == 0).all() and (cnt[surf] >= 1).all()


def test_oracle_facts_of_the_filter_case():
    """t3 at size 4 with the defaults: every accepted-tap count from 1 to 16 occurs on at least 50 surface pixels
    (observed minimum 91; 649 pixels keep only themselves, 588 all sixteen), so every window shape is exercised."""
    f = frame("t3")
    cnt = sc.accepted_counts(f["pos4"], f["nrm4"], 4)
    surf = sc.surface_of(f["pos4"])
    hist = [int(((cnt == k) & surf).sum()) for k in range(1, 17)]
    print("accepted-tap counts 1..16", hist)
    assert sum(hist) == int(surf.sum()) == 3600 and min(hist) >= 50
    assert (hist[0], hist[15]) == (649, 588)


# ---- the header, the library ---------------------------------------------------------------------------
def test_header_states_the_definition():
    text = " ".join(pathlib.Path(sf.HEADER_PATH).read_text().split())
    for sym in SYMBOLS + ("sf_light_filter_params",):
        assert sym in text, sym
    assert "nn = ((N_p.x N_q.x) + (N_p.y N_q.y)) + (N_p.z N_q.z)" in text
    assert "e = ((N_p.x D.x) + (N_p.y D.y)) + (N_p.z D.z)" in text
    assert "k2 = plane_max plane_max formed on the host in binary32" in text
    assert "out[p].xyz = S / (float)count, a correctly rounded division; out[p].w = in[p].w." in text
    assert "NOT TUNED AT 1920 x 1080" in text


def test_symbols_are_exported():
    if shutil.which("nm") is None:
        pytest.skip("binutils not available")
    have = defined_symbols(sf.LIB_PATH)
    assert set(SYMBOLS) <= have and set(SYMBOLS) <= set(sf.SIGNATURES)


def test_struct_layout_and_errors_without_a_device():
    P = sf.sf_light_filter_params
    assert ctypes.sizeof(P) == 32
    assert (P.size.offset, P.normal_min.offset, P.plane_max.offset, P.width.offset, P.height.offset,
            P.stream.offset) == (0, 4, 8, 12, 16, 24)
    L = sf.lib()
    p = P()
    p.size = 7
    buf = (ctypes.c_float * 64)()
    vp = ctypes.cast(buf, ctypes.c_void_p)
    assert L.sf_light_filter_defaults(None, ctypes.byref(p)) == sf.SF_EINVAL and p.size == 7
    assert L.sf_light_filter_to(None, ctypes.byref(p), vp, vp, vp, vp) == sf.SF_EINVAL
    assert L.sf_light_filter(None, ctypes.byref(p)) == sf.SF_EINVAL
