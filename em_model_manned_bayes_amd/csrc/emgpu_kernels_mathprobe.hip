// emgpu_kernels_mathprobe.hip -- k_math_probe: one hand-written device math function evaluated on n arguments, one lane per element, for
// emgpu_debug_device_math (tests/test_gpu_device_math.py compares the results with long-double values of the exact arguments).  Every
// instance calls the function the product kernels call (emgpu_device.h, emgpu_device_math.h), never a copy.  Not a product kernel.
#include <hip/hip_runtime.h>

#include "emgpu_device.h"
#include "emgpu_device_math.h"
#include "emgpu_mathprobe.h"

namespace emgpu {

template <int FN>
__global__ void __launch_bounds__(256) k_math_probe(int64_t n, const double *__restrict__ x, double *__restrict__ out0, double *__restrict__ out1) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    double a = 0.0, b = 0.0;
    if constexpr (FN == EMGPU_MATH_SINCOS_SMALL) sincos_small<false>(v, a, b);
    else if constexpr (FN == EMGPU_MATH_SINCOS_SMALL_SK) sincos_small<true>(v, a, b);
    else if constexpr (FN == EMGPU_MATH_SINCOSD_SMALL) sincosd_small(v, a, b);
    else if constexpr (FN == EMGPU_MATH_T_SINCOSD) t_sincosd(v, a, b);
    else if constexpr (FN == EMGPU_MATH_F_SINCOSD) f_sincosd(v, a, b);
    else if constexpr (FN == EMGPU_MATH_UT_SINCOS) ut_sincos<false>(v, a, b);
    else if constexpr (FN == EMGPU_MATH_UT_SINCOS_SK) ut_sincos<true>(v, a, b);
    else if constexpr (FN == EMGPU_MATH_UT_ATAN) a = ut_atan<false>(v);
    else if constexpr (FN == EMGPU_MATH_UT_ATAN_SK) a = ut_atan<true>(v);
    else if constexpr (FN == EMGPU_MATH_UT_ASIN_SMALL) a = ut_asin_small<false>(v);
    else if constexpr (FN == EMGPU_MATH_UT_ASIN_SMALL_SK) a = ut_asin_small<true>(v);
    else if constexpr (FN == EMGPU_MATH_UT_RCP) a = ut_rcp(v);
    else a = round500(v);
    out0[i] = a;
    if (FN <= EMGPU_MATH_UT_SINCOS_SK && out1) out1[i] = b;
}

template <int FN>
static void probe(int64_t n, const double *x, double *out0, double *out1, hipStream_t s) {
    hipLaunchKernelGGL(k_math_probe<FN>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, x, out0, out1);
}

hipError_t launch_math_probe(int32_t fn, int64_t n, const double *x, double *out0, double *out1, hipStream_t s) {
    switch (fn) {
    case EMGPU_MATH_SINCOS_SMALL: probe<EMGPU_MATH_SINCOS_SMALL>(n, x, out0, out1, s); break;
    case EMGPU_MATH_SINCOS_SMALL_SK: probe<EMGPU_MATH_SINCOS_SMALL_SK>(n, x, out0, out1, s); break;
    case EMGPU_MATH_SINCOSD_SMALL: probe<EMGPU_MATH_SINCOSD_SMALL>(n, x, out0, out1, s); break;
    case EMGPU_MATH_T_SINCOSD: probe<EMGPU_MATH_T_SINCOSD>(n, x, out0, out1, s); break;
    case EMGPU_MATH_F_SINCOSD: probe<EMGPU_MATH_F_SINCOSD>(n, x, out0, out1, s); break;
    case EMGPU_MATH_UT_SINCOS: probe<EMGPU_MATH_UT_SINCOS>(n, x, out0, out1, s); break;
    case EMGPU_MATH_UT_SINCOS_SK: probe<EMGPU_MATH_UT_SINCOS_SK>(n, x, out0, out1, s); break;
    case EMGPU_MATH_UT_ATAN: probe<EMGPU_MATH_UT_ATAN>(n, x, out0, out1, s); break;
    case EMGPU_MATH_UT_ATAN_SK: probe<EMGPU_MATH_UT_ATAN_SK>(n, x, out0, out1, s); break;
    case EMGPU_MATH_UT_ASIN_SMALL: probe<EMGPU_MATH_UT_ASIN_SMALL>(n, x, out0, out1, s); break;
    case EMGPU_MATH_UT_ASIN_SMALL_SK: probe<EMGPU_MATH_UT_ASIN_SMALL_SK>(n, x, out0, out1, s); break;
    case EMGPU_MATH_UT_RCP: probe<EMGPU_MATH_UT_RCP>(n, x, out0, out1, s); break;
    case EMGPU_MATH_ROUND500: probe<EMGPU_MATH_ROUND500>(n, x, out0, out1, s); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace emgpu
