// emgpu_mathprobe.h -- the launcher of k_math_probe (emgpu_kernels_mathprobe.hip): function fn (EMGPU_MATH_*, include/emgpu.h) of x[0..n)
// into out0 and, for the sin/cos pairs, out1 (or null).  Device pointers; the caller (emgpu_debug_device_math) has checked fn, n > 0, the
// pointers and their alignment.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/emgpu.h"

namespace emgpu {
hipError_t launch_math_probe(int32_t fn, int64_t n, const double *x, double *out0, double *out1, hipStream_t s);
}
