// emgpu_miss.h -- the argument block and the launcher of k_miss_distance (emgpu_kernels_miss.hip): the horizontal and vertical miss
// distance, the time of closest approach and the NMAC flags of paired 1 Hz tracks.  Built on the host by emgpu_pairs.cpp; no model, no
// context, no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/emgpu.h"
#include "emgpu_pairs.h"

// The definition (DESIGN.md "Miss distance of paired tracks"; include/emgpu.h).  Pair i takes column ia of set A and column ib of set B
// (the pairing: emgpu_pairs.h), both xyz f64 [P][3][ld_x] in feet.  With a pose {c, s, ox, oy, oz} of pair i, B's
// point is x' = (c * x - s * y) + ox, y' = (s * x + c * y) + oy, z' = z + oz; without one it is read as it lies.  Per second p:
//   dx = xa - xb', dy = ya - yb', d[p] = sqrt(dx * dx + dy * dy), dz[p] = zb' - za           CorTerminalModel.m:122-125
//   t_cpa = the first p with the smallest d[p], NaNs skipped; hmd = d[t_cpa], vmd = dz[t_cpa]  :127-128
//   NMAC_CPA  hmd < nmac_h && |vmd| < nmac_v                                                  track.m:175
//   NMAC_ANY  some p with d[p] < nmac_h && |dz[p]| < nmac_v
// Every product, sum and root is one IEEE double operation; nothing is contracted.  The minimum is over the ROOTS: two different sums of
// squares can round to one root, and then the earlier second is the CPA.
struct EmgpuMissRun {
    EmgpuPairDims dim;
    int32_t P, _pad;
    double nmac_h, nmac_v;
    EmgpuPairCols col;
    const double *pose;             // [5][n_pairs] or null
    const uint32_t *weights;        // [n_pairs] or null (1)
    double *hmd, *vmd;              // [n_pairs] each, or null
    int32_t *t_cpa;
    uint8_t *flags;
    unsigned long long *totals;     // [8], added to; or null
};

namespace emgpu {
hipError_t launch_miss_distance(const EmgpuMissRun &A, hipStream_t s, const char **name);
}
