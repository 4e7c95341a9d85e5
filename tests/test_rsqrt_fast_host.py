"""CPU restatement of the lean loops' fast table normalisation (sf_kernels.hip: rsqrtps_pos, and the wave-uniform
predicate of normalize3_fast / normalize3_fast2 that chooses between it and rsqrtps_x86), compared with the oracle's
rsqrtps on the golden table.

rsqrtps_pos reads the table at bits 13..23 of the argument (mantissa >> 13 with the exponent's parity above it: an
11-bit key, whatever the argument) and subtracts the exponent's half, (E + (E & 1) - 128) << 22. It is the x86
instruction's value for every positive normal finite argument, and the predicate `bits - 0x00800000 < 0x7f000000`
(unsigned) is true exactly for those; for anything else a live lane sends the whole wave down rsqrtps_x86."""
import ctypes

import numpy as np

from oracle import pyoracle


def rsqrtps_pos(bits, lut):
    """sf_kernels.hip rsqrtps_pos on uint32 bit patterns (uint32 arithmetic, wrapping as on the device)."""
    b = np.asarray(bits, np.uint32)
    E = b >> np.uint32(23)
    key = (b >> np.uint32(13)) & np.uint32(0x7ff)
    assert key.max() < lut.size
    with np.errstate(over="ignore"):
        return lut[key] - ((E + (E & np.uint32(1)) - np.uint32(128)) << np.uint32(22))


def plain(bits):
    """normalize3_fast's predicate: the argument is positive, normal and finite (rsqrtps_pos applies)."""
    b = np.asarray(bits, np.uint32)
    with np.errstate(over="ignore"):
        return (b - np.uint32(0x00800000)) < np.uint32(0x7f000000)


def oracle_bits(bits, lut):
    f = pyoracle.lib().sfo_rsqrtps
    p = lut.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    x = np.asarray(bits, np.uint32).view(np.float32)
    return np.array([f(float(v), p) for v in x], np.float32).view(np.uint32)


def test_rsqrtps_pos_equals_oracle_on_every_exponent_and_key(lut):
    lut = np.ascontiguousarray(lut, np.uint32)
    assert lut.size == 2048
    E = np.arange(1, 255, dtype=np.uint32)[:, None, None]
    # (a key's top bit is the exponent's parity, E's own: per exponent the 1024 mantissa prefixes, 2048 keys in all)
    top = np.arange(1024, dtype=np.uint32)[None, :, None]
    low = np.array([0, 0x1fff], np.uint32)[None, None, :]
    bits = ((E << np.uint32(23)) | (top << np.uint32(13)) | low).reshape(-1)
    assert bits.size == 254 * 1024 * 2
    assert plain(bits).all()
    got = rsqrtps_pos(bits, lut)
    ref = oracle_bits(bits, lut)
    bad = np.nonzero(got != ref)[0]
    assert bad.size == 0, [(hex(bits[i]), hex(got[i]), hex(ref[i])) for i in bad[:8]]
    # every 11-bit key was read: both parities of the exponent times every 10-bit mantissa prefix
    assert np.unique((bits >> np.uint32(13)) & np.uint32(0x7ff)).size == 2048


def test_predicate_boundaries(lut):
    cases = {
        0x00000000: False,   # +0
        0x007fffff: False,   # the largest denormal
        0x00800000: True,    # the smallest normal
        0x7f7fffff: True,    # FLT_MAX
        0x7f800000: False,   # +inf
        0x7fc00000: False,   # NaN
        0x80000000: False,   # -0
        0xbf800000: False,   # -1
    }
    bits = np.array(list(cases), np.uint32)
    assert plain(bits).tolist() == list(cases.values())
    # where the predicate holds rsqrtps_pos is the oracle's value; where it does not, the kernels take rsqrtps_x86
    ok = bits[plain(bits)]
    assert np.array_equal(rsqrtps_pos(ok, np.ascontiguousarray(lut, np.uint32)), oracle_bits(ok, lut))


def test_predicate_false_exactly_outside_the_positive_normals():
    """By class, on each class's ends and a sample inside: +-0, denormals, negatives, +inf, NaNs fail; normals pass."""
    rng = np.random.default_rng(11)
    def span(lo, hi):
        return np.concatenate([np.array([lo, hi], np.uint32), rng.integers(lo, hi + 1, 1000, dtype=np.uint64).astype(np.uint32)])
    assert plain(span(0x00800000, 0x7f7fffff)).all()            # positive normals
    assert not plain(span(0x00000000, 0x007fffff)).any()        # +0 and the positive denormals
    assert not plain(span(0x7f800000, 0x7fffffff)).any()        # +inf and the positive NaNs
    assert not plain(span(0x80000000, 0xffffffff)).any()        # -0, every negative, -inf, the negative NaNs
    # a key is inside the table whatever the argument (a lane that is not live still reads inside it)
    any_bits = rng.integers(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32)
    assert (((any_bits >> np.uint32(13)) & np.uint32(0x7ff)) < 2048).all()
