// sf_rootforms.h -- the traversal's near root t = fl(tca - sqrt_rn(x)), x = R2 - d2 >= 2^-96 (finite), in a form whose
// selects read no mask that the VALU instruction before them wrote (on gfx950 a v_cmp -> v_cndmask pair costs two
// wait states; the compiler fills them with s_nop where it has nothing independent to issue, and in the DFS's hit
// path it has nothing). Bit for bit the reference's
//     thc = sqrt_rn(x); t0 = tca + thc; t1 = tca - thc; t = (t0 <= t1) ? t0 : t1          (SIMD_AVX.h:260-267)
// on that domain; the proofs are below and in DESIGN.md §6.1. Checked for every float x
// (tests/test_root_forms_host.py on the host with every estimate within 1 ulp; tests/hip/root_forms_check.hip on the
// device with the hardware's).
//
// One text for the device and for a plain C host program: the host program defines SF_ROOTFORMS_HOST and supplies the
// estimate itself (sqrt_fix takes it as an argument), since only the device has v_sqrt_f32.
#pragma once

#include <stdint.h>

#if defined(SF_ROOTFORMS_HOST)
#include <math.h>
#include <string.h>
#define SF_RF_FN static inline
#define SF_RF_FMA(a, b, c) fmaf((a), (b), (c))
SF_RF_FN uint32_t sf_rf_bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    return u;
}
SF_RF_FN float sf_rf_float(uint32_t u)
{
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}
#else
#include <hip/hip_runtime.h>
#define SF_RF_FN __device__ __forceinline__
#define SF_RF_FMA(a, b, c) __builtin_fmaf((a), (b), (c))
SF_RF_FN uint32_t sf_rf_bits(float f) { return __float_as_uint(f); }
SF_RF_FN float sf_rf_float(uint32_t u) { return __uint_as_float(u); }
#endif

// domain of the short forms (as SF_SQRT_MID_LO in sf_fastmath.h: below it the IEEE sequence scales its argument)
#define SF_ROOT_BIG_LO 0x1p-96f

// sqrt_rn(x) from an estimate s0 within 1 ulp of it, 2^-96 <= x < inf: the IEEE sequence's two neighbour tests,
//     thc = (rdn <= 0) ? sdn : s0;  thc = (rup > 0) ? sup : thc,   rdn = fma(-sdn, s0, x), rup = fma(-sup, s0, x)
// (sdn / sup: s0's neighbours, bits - 1 / + 1), as integer arithmetic on the residuals' sign bits:
//     thc = bits(sdn) + sign(-rdn) + sign(-rup),   -rdn = fma(sdn, s0, -x), -rup = fma(sup, s0, -x).
//  - fma(a, b, -c) = -fma(-a, b, c) exactly: round-to-nearest-even is symmetric in the sign, except that an exact zero
//    sum is +0 for both. So sign(-rdn) = 1 exactly when rdn > 0, and sign(-rup) = 1 exactly when rup > 0 -- zero
//    residuals (a neighbour whose product with s0 is x itself) included: both forms see +0, "rdn <= 0" and "not
//    rup > 0", sign 0.
//  - No residual rounds to zero from a non-zero value: s0 >= 2^-48 (1 - 2^-23), so the exact residual is a multiple
//    of ulp(s0)^2 >= 2^-142, above the smallest denormal (denormals are kept). None is NaN or inf: x and s0 are
//    finite and positive, sdn >= 2^-49.
//  - rup <= rdn (sup > sdn, s0 > 0, rounding is monotone), so sign(-rup) = 1 implies sign(-rdn) = 1. The three cases:
//    rdn <= 0: both signs 0, thc = sdn; rdn > 0 >= rup: thc = sdn + 1 = s0; rup > 0: thc = sdn + 2 = sup -- the
//    selects' results. (bits + 1 is the next float up: s0 is positive, finite and below FLT_MAX.)
// x = 0 and x < 2^-96 are outside the domain (sdn of s0 = 0 is a NaN pattern); the callers' uniform tiny-argument
// test sends a wave with such a lane among its hits to the general form.
SF_RF_FN float sqrt_fix(float s0, float x)
{
    const float sdn = sf_rf_float(sf_rf_bits(s0) - 1u);
    const float sup = sf_rf_float(sf_rf_bits(s0) + 1u);
    const float ndn = SF_RF_FMA(sdn, s0, -x);
    const float nup = SF_RF_FMA(sup, s0, -x);
    return sf_rf_float(sf_rf_bits(sdn) + (sf_rf_bits(ndn) >> 31) + (sf_rf_bits(nup) >> 31));
}

// (t0 <= t1) ? t0 : t1 with t0 = fl(tca + thc), t1 = fl(tca - thc), for thc > 0 (not NaN) and any tca: t1 itself.
//  - tca - thc < tca + thc exactly, and rounding is monotone, so t1 <= t0: the compare holds only when t0 == t1.
//  - Equal floats have equal bits unless both are zero. t0 = 0 needs tca = -thc exactly (a sum of two floats rounds
//    to zero only when it is zero), and then t1 = fl(-2 thc) != 0. So where the reference takes t0, t0 and t1 are
//    the same non-zero value (thc below half an ulp of tca; +-inf for tca = +-inf), the same bits.
//  - tca NaN: the compare fails, the reference takes t1 too.
// thc = 0 would differ (tca = -0: t0 = +0, t1 = -0); the domain x >= 2^-96 keeps thc >= 2^-48.
SF_RF_FN float near_root_of(float tca, float thc)
{
    return tca - thc;
}
