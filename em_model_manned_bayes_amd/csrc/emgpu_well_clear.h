// emgpu_well_clear.h -- the argument block and the launcher of k_well_clear (emgpu_kernels_well_clear.hip): loss of DAA well clear of paired
// 1 Hz tracks, evaluated at every whole second on the relative state k_miss_distance forms.  Built on the host by emgpu_pairs.cpp; no
// model, no context, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/emgpu.h"
#include "emgpu_pairs.h"

// The definition (include/emgpu.h).  The pairing, the pose and the per-point dx, dy, dz are k_miss_distance's
// (emgpu_miss.h).  The relative velocity at point p is the forward difference of the segment that starts there, the last point taking the
// last segment's: q = min(p, P-2), ux = dx[q+1] - dx[q], uy = dy[q+1] - dy[q]; P = 1: ux = uy = 0.  Per point (x, y, z) = (dx, dy, dz)[p],
// with D2 = dmod * dmod and H2 = hmd * hmd from the host:
//   rr = x * x + y * y, rv = x * ux + y * uy, vv = ux * ux + uy * uy
//   valid   = rr, rv, vv and z all finite
//   inside  = rr <= D2;  closing = rv < 0
//   tau     = inside ? 0 : (closing ? (D2 - rr) / rv : +inf)
//   tc      = vv > 0 ? (-rv) / vv : 0;  tc = tc > 0 ? tc : 0
//   px = x + tc * ux, py = y + tc * uy, hp2 = px * px + py * py
//   by_tau  = !inside && closing && tau <= tau_s && hp2 <= H2
//   lost[p] = valid && fabs(z) <= h && (inside || by_tau)
// The comparisons are <= (the NMAC test of the miss kernels is <).  t_first is the first p with lost[p] (-1: none), n_lost their number,
// tau_min the smallest tau over the valid points (NaN: no valid point).  Every product, sum and quotient is one IEEE double operation;
// nothing is contracted; no root enters.
struct EmgpuWellClearRun {
    EmgpuPairDims dim;
    int32_t P, _pad;
    double tau_s, D2, H2, h;
    EmgpuPairCols col;
    const double *pose;             // [5][n_pairs] or null
    const uint32_t *weights;        // [n_pairs] or null (1)
    const uint8_t *miss_flags;      // [n_pairs] or null: a miss kernel's flags, EMGPU_MISS_NMAC_ANY is read
    int32_t *t_first, *n_lost;      // [n_pairs] each, or null
    double *tau_min;
    uint8_t *flags;
    unsigned long long *totals;     // [10], added to; or null
};

namespace emgpu {
hipError_t launch_well_clear(const EmgpuWellClearRun &A, hipStream_t s, const char **name);
}
