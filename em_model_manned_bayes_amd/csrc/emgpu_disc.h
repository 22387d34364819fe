// emgpu_disc.h -- the unit-disc point of section 13 of the RNG slot map, once: what k_encounter_pose (streams a = 0 and 1) and k_cpa_pose
// (stream a = 3) draw a heading from.  Device code only.
#pragma once
#include "emgpu_device.h"
#include "emgpu_encounter.h"

// 2 u(x) - 1: a coordinate in (-1, 1)
__device__ __forceinline__ double centred(uint32_t x) { return 2.0 * emgpu::uniform32(x) - 1.0; }

// The unit-disc point of stream a: attempt j takes words 2 (j & 1) and 2 (j & 1) + 1 of block j >> 1; the first attempt with
// 0 < p * p + q * q <= 1 is taken.  false: none was (p = 1, q = 0).
__device__ __forceinline__ bool disc_point(uint32_t g_lo, uint32_t g_hi, uint32_t k0, uint32_t k1, uint32_t a, int max_attempts, double &p,
                                           double &q) {
    bool got = false;
    p = 1.0; q = 0.0;
    for (int j = 0; j < max_attempts && !got; j += 2) {
        const uint4 v = emgpu::philox4x32(g_lo, g_hi, 0u, (EMGPU_SEC_ENCOUNTER << 28) | (a << 20) | (uint32_t)(j >> 1), k0, k1);
        const double p0 = centred(v.x), q0 = centred(v.y), p1 = centred(v.z), q1 = centred(v.w);
        const double d0 = p0 * p0 + q0 * q0, d1 = p1 * p1 + q1 * q1;
        const bool ok0 = d0 > 0.0 && d0 <= 1.0, ok1 = j + 1 < max_attempts && d1 > 0.0 && d1 <= 1.0;
        p = ok0 ? p0 : (ok1 ? p1 : p);
        q = ok0 ? q0 : (ok1 ? q1 : q);
        got = ok0 || ok1;
    }
    return got;
}
