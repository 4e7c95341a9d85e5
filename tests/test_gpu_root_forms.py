"""GPU test of sf_rootforms.h on the device: sqrt_fix on the hardware's own v_sqrt_f32 estimate against
__builtin_sqrtf, and near_root_of against the reference's select between tca + thc and tca - thc, for every float x of
the forms' domain 2^-96 <= x < inf -- all 2^32 patterns swept by tests/hip/root_forms_check.hip, in the style of
test_gpu_post.py::test_fastmath_matches_ieee_on_every_float."""
import ctypes
import os

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

# +-0, denormals, the smallest normal, ordinary traversal values, values far above every thc, FLT_MAX, +-inf; the
# kernel adds -thc and thc * +-2^24, +-2^25 per argument (tca +- thc round together, or differ by one ulp)
TCAS = np.array([0.0, -0.0, 2.0 ** -149, -2.0 ** -149, 2.0 ** -126 - 2.0 ** -149, 2.0 ** -126, 1.0, -1.0, 3.7,
                 2.0 ** -30, 1000.0, 2.0 ** 40, 2.0 ** 100, -2.0 ** 100, np.finfo(np.float32).max, np.inf, -np.inf],
                np.float32)


def test_root_forms_match_ieee_on_every_float():
    path = os.path.join(REPO, "tests", "hip", "build", "libsf_root_forms_check.so")
    assert os.path.exists(path), "build the test kernels first (__graft_entry__.build())"
    fn = ctypes.CDLL(path).sf_root_forms_check
    fn.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.POINTER(ctypes.c_float), ctypes.c_int]
    c = (ctypes.c_ulonglong * 6)()
    assert fn(c, TCAS.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(TCAS)) == 0
    n_x, bad_sqrt, n_roots, bad_roots, took_t0, bare_sqrt = list(c)
    print(f"{n_x} arguments, {bad_sqrt} sqrt_fix mismatches ({bare_sqrt} of the bare v_sqrt), {n_roots} near roots, "
          f"{bad_roots} mismatches, {took_t0} where the reference took t0")
    assert n_x == 224 << 23                      # every float of [2^-96, FLT_MAX]
    assert n_roots == n_x * (len(TCAS) + 5)
    assert bad_sqrt == 0 and bad_roots == 0
    assert bare_sqrt > 0                         # (the correction is needed)
    assert took_t0 > 0                           # (the t0 == t1 case is among the arguments)
