"""Host test of sf_rootforms.h (the traversal's near root without compare -> select pairs): tests/cpp/root_forms_host.c,
a stand-alone C program holding the header's own text, compiled with -ffp-contract=off (every fused operation an
explicit fmaf) and run over all 2^32 float patterns x on every CPU.

  - sqrt_fix(s0, x) for each estimate s0 within 1 ulp of sqrt_rn(x) -- the root and both neighbours; the device's
    v_sqrt_f32 result is one of them -- against the two selects it replaces, and against the correctly rounded sqrtf.
  - near_root_of(tca, thc) with thc = sqrtf(x) against (t0 <= t1) ? t0 : t1 for a fixed set of tca: +-0, denormals,
    ordinary values, values where tca + thc and tca - thc round together, FLT_MAX, +-inf; and per x the tca = -thc
    (t0 = 0) and thc * +-2^24, +-2^25 (the last place where the two roots still differ).

Patterns outside the forms' domain 2^-96 <= x <= FLT_MAX are counted out: the callers' wave-uniform tiny-argument test
sends those to the general form."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, REPO

NTCA = 17 + 5   # the program's fixed set and its five per-argument values


def test_root_forms_on_every_float(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler for tests/cpp/root_forms_host.c")
    exe = str(tmp_path / "root_forms_host")
    # (-fno-math-errno / -fno-trapping-math let sqrtf and the compares vectorise; neither changes a result)
    subprocess.check_call([cc, "-O3", "-march=native", "-ffp-contract=off", "-fno-math-errno", "-fno-trapping-math",
                           "-I", os.path.join(PKG, "csrc"), "-o", exe,
                           os.path.join(REPO, "tests", "cpp", "root_forms_host.c"), "-lpthread", "-lm"])
    threads = min(64, len(os.sched_getaffinity(0)))
    out = subprocess.check_output([exe, str(threads)], text=True)
    n_dom, bad_sel, bad_rn, n_roots, bad_roots, took_t0 = map(int, out.split())
    print(f"{n_dom} arguments x 3 estimates: {bad_sel} differ from the selects, {bad_rn} from sqrtf; {n_roots} near "
          f"roots: {bad_roots} differ, {took_t0} where the reference took t0")
    assert n_dom == 224 << 23                  # every float of [2^-96, FLT_MAX]
    assert n_roots == n_dom * NTCA
    assert bad_sel == 0 and bad_rn == 0 and bad_roots == 0
    assert took_t0 > 0                         # (t0 == t1 after rounding is among the cases)
