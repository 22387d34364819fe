// emgpu_cpa.h -- the argument block and the launcher of k_cpa_pose (emgpu_kernels_cpa.hip): per pair of 1 Hz tracks a random heading of
// the intruder, a drawn second tc at which the two aircraft pass, a signed lateral miss and a vertical offset there, the pose that makes
// the pass happen so, and the flux through the miss plane.  Built on the host by emgpu_pairs.cpp; no model, no context, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/emgpu.h"
#include "emgpu_encounter.h"
#include "emgpu_pairs.h"

// The definition (DESIGN.md "Intruders at a drawn closest approach"; include/emgpu.h).  Section 13 of the RNG slot map, streams a = 3 (the
// heading's disc point, as a = 0 of k_encounter_pose) and a = 4 (block 0: u1 lateral, u2 vertical, x the second).  Pair i reads points tc
// and tc + 1 of column ia of set A and of column ib of set B (the pairing: emgpu_pairs.h):
//   second    tc = t_lo + ((uint64)x * span >> 32), span = t_hi - t_lo + 1
//   heading   (p, q) the a = 3 disc point, r = sqrt(p * p + q * q), c = p / r, s = q / r
//   relative  rx = (c * bx - s * by) - ax, ry = (s * bx + c * by) - ay, g = sqrt(rx * rx + ry * ry)
//   rate      Q = kc * g
//   offsets   l = Hm * (2 * u1 - 1), relx = (-l) * (ry / g), rely = l * (rx / g), dz = Vm * (2 * u2 - 1)
//   pose      ox = (Atx + relx) - (c * Btx - s * Bty), oy = (Aty + rely) - (s * Btx + c * Bty), oz = (Atz + dz) - Btz
// Every product, sum, quotient and root is one IEEE double operation; nothing is contracted.
struct EmgpuCpaRun {
    EmgpuPairDims dim;
    uint64_t seed, first_index;
    int32_t max_attempts, t_lo;
    uint32_t span, _pad;               // t_hi - t_lo + 1: 1 .. 65536
    double Hm, Vm, kc, rate_scale;     // kc = (4 * Hm) * Vm
    EmgpuPairCols col;
    const uint32_t *weights_in;        // [n_pairs] or null (1)
    double *pose;                      // [5][n_pairs] or null
    double *rate;                      // [n_pairs] or null
    int32_t *t_cpa;
    uint8_t *flags;
    uint32_t *weights_out;
};

namespace emgpu {
hipError_t launch_cpa_pose(const EmgpuCpaRun &A, hipStream_t s, const char **name);
}
