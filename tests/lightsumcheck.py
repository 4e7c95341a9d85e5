"""Shared pieces of the colour-light-buffer tests (tests/test_light_sum_host.py, tests/test_gpu_light_sum.py)."""
import numpy as np

from maskcheck import surface_of  # noqa: F401

F = np.float32

# distinct RGB colours for the 8-direction cones and the named lights
CONE_COLOURS = np.array([(0.5, 0.25, 0.125), (0.125, 0.5, 0.25), (0.25, 0.125, 0.5), (0.375, 0.375, 0.0625),
                         (0.0625, 0.1875, 0.4375), (0.3125, 0.0625, 0.25), (0.1875, 0.4375, 0.3125),
                         (0.21875, 0.28125, 0.09375)], F) / F(3.0)

# the non-zero base of the accumulate tests (a .w the traces must carry)
BASE = (0.125, 0.25, 0.5, 7.5)


def colours(n, seed=5):
    """n RGB colours whose magnitudes spread over 2^-8 .. 1 / n: float sums that depend on the order."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.5, 1.0, (n, 3)) * 2.0 ** rng.integers(-8, 1, (n, 1)) / n).astype(F)


def pack(bits):
    """Chunk masks (a list of uint64 images) from bits [n, ...] (bool): entry i is bit i % 64 of chunk i // 64."""
    bits = np.asarray(bits, bool)
    out = []
    for j in range(0, len(bits), 64):
        m = np.zeros(bits.shape[1:], np.uint64)
        for i in range(min(64, len(bits) - j)):
            m |= bits[j + i].astype(np.uint64) << np.uint64(i)
        out.append(m)
    return out


def chunk_masks(trace, points, **kw):
    """The masks of trace (trace_suns or trace_shadows) for consecutive chunks of 64 of the points."""
    return [trace(points[j:j + 64], **kw) for j in range(0, len(points), 64)]


def base_image(shape):
    b = np.empty(tuple(shape) + (4,), F)
    b[...] = np.asarray(BASE, F)
    return b


def assert_same(got, want, what, where=None):
    """Bitwise equality of two float32 [H, W, 4] images (where `where` holds)."""
    assert got.dtype == np.float32 and got.shape == want.shape, what
    differ = (np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(want).view(np.uint32)).any(axis=-1)
    if where is not None:
        differ &= where
    bad = np.argwhere(differ)
    assert bad.size == 0, f"{what}: {len(bad)} pixels differ, first {bad[:3].tolist()}: " \
                          f"{[got[tuple(b)].tolist() for b in bad[:3]]} != {[want[tuple(b)].tolist() for b in bad[:3]]}"
