// emgpu_trackval.h -- the argument block and the launcher of k_track_values (emgpu_kernels_trackval.hip): 1 Hz TRACKS into the VALUES of a
// trace, in the layout k_discretize_dbn reads.  The inverse of k_sample2track (emgpu_kernels_track.hip), as k_count_dbn is the sampler's.
// Built on the host by emgpu_trackval.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/emgpu.h"

// The definition (DESIGN.md "Values from tracks"; include/emgpu.h).  One track is P >= 3 points (x, y, z) in feet, one second apart, f64;
// it yields T = P - 2 seconds of values.  All arithmetic is f64 and not contracted.
//   displacement  t = 0 .. P-2:  dx = x[t+1] - x[t], dy = y[t+1] - y[t], dz = z[t+1] - z[t]               sample2track.m:211-212, :201
//   speed         s[t] = sqrt(dx * dx + dy * dy): two multiplies, one add, an IEEE square root              :211-212 (|speed * (cosd, sind)|)
//   heading       h[t] = atan2(dy, dx) * 57.29577951308232; where s[t] == 0: h[t] = h[t-1], h[-1] = 0       :211-212 (the angle), :189
//   values        t = 0 .. T-1:
//     vertical rate  dz[t] / ur_vertrate                                                                    :201 with :131
//     acceleration   (s[t+1] - s[t]) / ur_speed                                                             :204 with :132
//     turn rate      w / ur_heading, d = h[t+1] - h[t], w = d - 360 * floor((d + 180) / 360) in [-180, 180)  :207 with :133
//   initial rows  altitude z[0] (:186), speed s[0] / ur_speed (:188 with :126), the three rates their value at t = 0
// Non-finite coordinates flow through this arithmetic; nothing is reported (k_discretize_dbn reports a NaN).
#define EMGPU_TV_BLOCK 256     // lanes = tracks of one workgroup
#define EMGPU_TV_TILE 8        // ROWS: points of one LDS tile
#define EMGPU_TV_STRIDE (3 * EMGPU_TV_TILE + 1)   // doubles between two tracks of the tile: odd, so that 32 lanes' 8-byte reads hit 64 banks
struct EmgpuTrackValuesRun {
    int64_t n;
    int64_t ld;                  // track dimension of init_val and dyn_val
    int32_t P, nd;               // points per track; rows per group of four seconds in dyn_val
    int32_t row[5];              // init_val rows of altitude, speed, vertical rate, acceleration, turn rate; -1: not written
    int32_t slot[3];             // dyn_val rows of vertical rate, acceleration, turn rate
    double ur_speed, ur_vertrate, ur_heading;
    const double *xyz;           // PLANAR [P][3][n]; ROWS [n][P][3]
    void *init_val;              // V [..][ld], already at the call's first column; null: no initial half
    void *dyn_val;               // V [ceil(T/4)][nd][ld][4]; null: no dynamic half
};

namespace emgpu {
// rows: xyz is [n][P][3], else [P][3][n]; f64: the values are doubles (EMGPU_VALUE_F64), else floats
hipError_t launch_track_values(const EmgpuTrackValuesRun &A, bool rows, bool f64, hipStream_t s, const char **name);
}
