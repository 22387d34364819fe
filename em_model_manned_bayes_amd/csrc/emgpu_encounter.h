// emgpu_encounter.h -- the argument block and the launcher of k_encounter_pose (emgpu_kernels_encounter.hip): per pair of 1 Hz tracks a
// random heading of the intruder, its entry point on the encounter cylinder around the ownship and the volume the cylinder sweeps per
// second relative to it.  Built on the host by emgpu_pairs.cpp; no model, no context, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/emgpu.h"
#include "emgpu_pairs.h"

// section 13 of the RNG slot map: counter = {g_lo, g_hi, 0, 13 << 28 | a << 20 | block}
#define EMGPU_SEC_ENCOUNTER 13u

// The definition (DESIGN.md "Intruders on the encounter cylinder"; include/emgpu.h).  Pair i takes column ia of set A and column ib of set
// B (the pairing: emgpu_pairs.h), reads points 0 and 1 of both, and writes the pose {c, s, ox, oy, oz} that kernel reads:
//   heading   (p, q) the a = 0 disc point, r = sqrt(p * p + q * q), c = p / r, s = q / r
//   relative  rx = (c * bx - s * by) - ax, ry = (s * bx + c * by) - ay, wr = bz - az, g = sqrt(rx * rx + ry * ry)
//   rate      Q = ks * g + ke * |wr|; side entry iff u1 * Q < ks * g, end cap otherwise
//   pose      ox = (A0x + relx) - (c * B0x - s * B0y), oy = (A0y + rely) - (s * B0x + c * B0y), oz = (A0z + dz) - B0z
// Every product, sum, quotient and root is one IEEE double operation; nothing is contracted.
struct EmgpuEncounterRun {
    EmgpuPairDims dim;
    uint64_t seed, first_index;
    int32_t max_attempts, _pad;
    double R, H, ks, ke, rate_scale;   // ks = (4 * R) * H, ke = (pi * R) * R
    EmgpuPairCols col;
    const uint32_t *weights_in;        // [n_pairs] or null (1)
    double *pose;                      // [5][n_pairs] or null
    double *rate;                      // [n_pairs] or null
    uint8_t *flags;
    uint32_t *weights_out;
};

namespace emgpu {
hipError_t launch_encounter_pose(const EmgpuEncounterRun &A, hipStream_t s, const char **name);
}
