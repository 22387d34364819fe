// emgpu_miss_seg.h -- the argument block and the launcher of k_miss_segments (emgpu_kernels_miss_seg.hip): miss distance, time of closest
// approach and NMAC flags of paired 1 Hz tracks ON THE SEGMENTS between the seconds, the tracks read as piecewise linear.  Built on the host
// by emgpu_pairs.cpp; no model, no context, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/emgpu.h"
#include "emgpu_pairs.h"

// The definition (include/emgpu.h).  The pairing, the pose and the per-point dx, dy, dz, d are k_miss_distance's
// (emgpu_miss.h).  Per segment p = 1 .. P-1 between points p-1 and p, (x0, y0, z0) = (dx, dy, dz)[p-1], z1 = dz[p]:
//   ex = dx[p] - x0, ey = dy[p] - y0, ez = z1 - z0, ee = ex * ex + ey * ey, re = x0 * ex + y0 * ey
//   valid = ee, re, z0 and ez all finite; ts = ee > 0 ? (-re) / ee : 0
//   interior candidate iff valid && ts > 0 && ts < 1: ds = sqrt(px * px + py * py) at px = x0 + ts * ex, py = y0 + ts * ey; zs = z0 + ts * ez
//   near = min(z0, z1) < V && max(z0, z1) > -V
//   ez != 0: t0 = (-V - z0) / ez, t1 = (V - z0) / ez, lo = max(min(t0, t1), 0), hi = min(max(t0, t1), 1); else lo = 0, hi = 1
//   tc = ts clamped to [lo, hi] (tc > lo ? tc : lo, then tc < hi ? tc : hi), dc = sqrt(qx * qx + qy * qy) at qx = x0 + tc * ex, qy = y0 + tc * ey
//   between = valid && near && lo < hi && dc < H
// The CPA is the first of the smallest candidates in time order: point 0, interior 1, point 1, interior 2, ...  Every product, sum, quotient
// and root is one IEEE double operation; nothing is contracted.
struct EmgpuMissSegRun {
    EmgpuPairDims dim;
    int32_t P, _pad;
    double nmac_h, nmac_v;
    EmgpuPairCols col;
    const double *pose;             // [5][n_pairs] or null
    const uint32_t *weights;        // [n_pairs] or null (1)
    double *hmd, *vmd, *t_cpa_s;    // [n_pairs] each, or null
    uint8_t *flags;
    unsigned long long *totals;     // [10], added to; or null
};

namespace emgpu {
hipError_t launch_miss_segments(const EmgpuMissSegRun &A, hipStream_t s, const char **name);
}
