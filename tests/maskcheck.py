"""What the tests of the mask traces (trace_shadows, trace_suns, trace_shafts, trace_ao, trace_mirror) say about a
uint64 mask image and the position image it belongs to: one definition each."""
import numpy as np


def bit(mask, i):
    """Bit i of every word, as bool."""
    return ((np.asarray(mask, np.uint64) >> np.uint64(i)) & np.uint64(1)) != 0


def low(n):
    """The word with its low n bits set, n = 0..64."""
    return np.uint64((1 << n) - 1)


def surface_of(pos4):
    """The surface pixels of a position image: a miss of the frame is (0, 0, 0)."""
    P = np.asarray(pos4)[..., :3]
    return ~((P[..., 0] == 0) & (P[..., 1] == 0) & (P[..., 2] == 0))


def assert_mask(got, want, what, where=None):
    """Equal words (where `where` holds)."""
    assert got.dtype == np.uint64 and got.shape == want.shape, what
    differ = got != want
    if where is not None:
        differ &= where
    bad = np.argwhere(differ)
    assert bad.size == 0, f"{what}: {len(bad)} pixels differ, first {bad[:4]}: " \
                          f"{[hex(int(got[tuple(b)])) for b in bad[:4]]} != {[hex(int(want[tuple(b)])) for b in bad[:4]]}"


def assert_shape_of_mask(got, n, pos, what):
    """Bits n..63 are zero everywhere, and a miss of the frame has exactly its low n bits set."""
    if n < 64:
        assert (got >> np.uint64(n) == 0).all(), what
    assert (got[~surface_of(pos)] == low(n)).all(), what
