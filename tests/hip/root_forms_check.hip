// Test kernel (not product code): sf_rootforms.h's near root against the reference's form on the IEEE square root, for
// every float x of the short forms' domain with the hardware's own estimate. Built by __graft_entry__.build() into
// tests/hip/build/libsf_root_forms_check.so; called by tests/test_gpu_root_forms.py.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "sf_rootforms.h"

namespace {

// Near root of RaySphereIntersection on the correctly rounded root (sf_kernels.hip's near_root on x = R2 - d2)
__device__ __forceinline__ float near_root_ref(float tca, float thc)
{
    const float t0 = tca + thc;
    const float t1 = tca - thc;
    return (t0 <= t1) ? t0 : t1;
}

// out[0]: arguments of the domain 2^-96 <= x < inf, out[1]: sqrt_fix mismatches, out[2]: near roots compared,
// out[3]: near-root mismatches, out[4]: near roots where the reference took t0 (t0 == t1 after rounding),
// out[5]: mismatches of the bare v_sqrt (what the correction is for). Every 32-bit pattern once (grid-stride over 2^32).
// tcas: n fixed values; per x also tca = -thc (t0 = 0), thc * 2^24 and thc * 2^25 (tca +- thc round together), and
// their negatives.
__global__ void __launch_bounds__(256) check_all(unsigned long long* out, const float* tcas, int n)
{
    unsigned long long n_x = 0, bad_s = 0, n_t = 0, bad_t = 0, n_t0 = 0, bad_hw = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (1ull << 32); i += stride) {
        const float x = __uint_as_float((uint32_t)i);
        if (!(x >= SF_ROOT_BIG_LO && x <= 3.402823466e38f)) continue;
        ++n_x;
        const float ref = __builtin_sqrtf(x);
        const float s0 = __builtin_amdgcn_sqrtf(x);
        const float thc = sqrt_fix(s0, x);
        bad_s += __float_as_uint(thc) != __float_as_uint(ref);
        bad_hw += __float_as_uint(s0) != __float_as_uint(ref);
        auto one = [&](float tca) {
            const float want = near_root_ref(tca, ref);
            ++n_t;
            bad_t += __float_as_uint(near_root_of(tca, thc)) != __float_as_uint(want);
            n_t0 += (tca + ref) <= (tca - ref);
        };
        for (int k = 0; k < n; ++k) one(tcas[k]);
        one(-ref);
        one(ref * 0x1p24f);
        one(ref * 0x1p25f);
        one(ref * -0x1p24f);
        one(ref * -0x1p25f);
    }
    atomicAdd(&out[0], n_x);
    atomicAdd(&out[1], bad_s);
    atomicAdd(&out[2], n_t);
    atomicAdd(&out[3], bad_t);
    atomicAdd(&out[4], n_t0);
    atomicAdd(&out[5], bad_hw);
}

}  // namespace

// tcas: n <= 32 host floats. Returns 0 and the six counts, or a negative step number.
extern "C" int sf_root_forms_check(unsigned long long* counts, const float* tcas, int n)
{
    if (n < 0 || n > 32) return -5;
    unsigned long long* d = nullptr;
    float* dt = nullptr;
    if (hipMalloc(&d, 6 * sizeof *d) != hipSuccess) return -1;
    if (hipMalloc(&dt, 32 * sizeof *dt) != hipSuccess) {
        (void)hipFree(d);
        return -1;
    }
    int rc = 0;
    if (hipMemset(d, 0, 6 * sizeof *d) != hipSuccess) rc = -2;
    if (!rc && n > 0 && hipMemcpy(dt, tcas, n * sizeof *dt, hipMemcpyHostToDevice) != hipSuccess) rc = -2;
    if (!rc) {
        hipLaunchKernelGGL(check_all, dim3(8192), dim3(256), 0, 0, d, dt, n);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = -3;
    }
    if (!rc && hipMemcpy(counts, d, 6 * sizeof *d, hipMemcpyDeviceToHost) != hipSuccess) rc = -4;
    (void)hipFree(d);
    (void)hipFree(dt);
    return rc;
}
