// emgpu_avoid.h -- the argument block and the launcher of k_avoid (emgpu_kernels_avoid.hip): the ownship's vertical avoidance manoeuvre on
// paired 1 Hz tracks -- the alert second, the sense, the mitigated vertical miss and the NMAC with and without the manoeuvre, whose
// weighted ratio is the risk ratio.  Built on the host by emgpu_pairs.cpp; no model, no context, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/emgpu.h"
#include "emgpu_pairs.h"

// The definition (include/emgpu.h).  The pairing, the pose and the per-point dx, dy, dz, d are k_miss_distance's
// (emgpu_miss.h); the relative velocity (ux, uy) at point p and the predicate lost[p] are k_well_clear's (emgpu_well_clear.h), here with
// the four ALERT thresholds: alert[p] = lost[p], on the unmitigated state.  Added: wz = dz[q+1] - dz[q] with the same q = min(p, P-2)
// (P = 1: 0).
//   t_alert = the first p with alert[p] (-1: none); only it acts.  There, with (x, y, z) = (dx, dy, dz)[t_alert] and well clear's clamped tc:
//     zp = z + tc * wz;  descend = zp > 0 || (!(zp < 0) && z > 0);  climb = !descend
//   t0 = t_alert + delay.  For a point p with k = p - t0 >= 1, kd = (double)k:
//     g = kd < tr ? half_a * (kd * kd) : rate * (kd - half_tr);  g = g < dz_max ? g : dz_max
//     dz'[p] = climb ? dz[p] - g : dz[p] + g
//   and dz'[p] = dz[p] otherwise (k <= 0, or no alert).  tr = rate / accel, half_tr = 0.5 * tr, half_a = 0.5 * accel come from the host.
//   hmd, vmd, t_cpa: k_miss_distance's, bit for bit; vmd_mit = dz'[t_cpa].
//   NMAC_UNMIT  some p with d[p] < nmac_h && |dz[p]| < nmac_v;  NMAC_MIT  the same with dz'[p]
//   LATE        alerted && t0 >= P-1: no point was moved
// Every product, sum, quotient and root is one IEEE double operation; nothing is contracted; a NaN compares false.
struct EmgpuAvoidRun {
    EmgpuPairDims dim;
    int32_t P, delay;               // delay: delay_s, at most 65537 (more changes nothing: P <= 65537)
    double tau_s, D2, H2, h;        // the alert volume
    double nmac_h, nmac_v;
    double rate, tr, half_tr, half_a, dz_max;
    EmgpuPairCols col;
    const double *pose;             // [5][n_pairs] or null
    const uint32_t *weights;        // [n_pairs] or null (1)
    double *hmd, *vmd, *vmd_mit;    // [n_pairs] each, or null
    int32_t *t_cpa, *t_alert;
    uint8_t *flags;
    unsigned long long *totals;     // [12], added to; or null
};

namespace emgpu {
hipError_t launch_avoid(const EmgpuAvoidRun &A, hipStream_t s, const char **name);
}
