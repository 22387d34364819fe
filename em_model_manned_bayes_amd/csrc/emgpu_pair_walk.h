// emgpu_pair_walk.h -- what the four kernels that walk the seconds of paired 1 Hz tracks share: k_miss_distance (emgpu_kernels_miss.hip),
// k_miss_segments (emgpu_kernels_miss_seg.hip), k_well_clear (emgpu_kernels_well_clear.hip) and k_avoid (emgpu_kernels_avoid.hip).  One
// lane per pair, 256-lane workgroups that walk the tiles of emgpu_pairs.h, sequential in time.  Device-only but for launch_pair_walk, and
// kept out of emgpu_pairs.h so that the host unit and the two placement kernels do not include it.
//
// The walk: per lane the pose's five doubles once (pair_pose), then per second six 8-byte loads, three of each set (pair_point), coalesced
// along the pair index where the indices are the identity; with one column in a set (n_x == 1) the 64 lanes of a wave name one address
// per coordinate; through arbitrary indices a lane's load is alone in its 64-byte sector.
//
// The totals are integers, so the order of the adds does not matter; they are reduced in three stages:
//   1. registers per lane over the workgroup's tiles: u32 for a count (a lane takes at most 2^32 / 256 / 2048 = 8192 pairs of a call),
//      u64 for a sum of weights (8192 * (2^32 - 1) < 2^45);
//   2. a shuffle reduction per wave on 64-bit values, one 64-bit LDS slot per (wave, counter);
//   3. one 64-bit vector atomic without return (global_atomic_add_x2, relaxed, agent scope) per (workgroup, touched counter).
// Every partial from stage 2 on is 64-bit, so none can wrap and the grid needs no cap on the tiles of a workgroup: it is
// min(tiles, 2048) workgroups, so the atomics of stage 3 are paid 2048 times per counter at most.  No float atomic, no scratch.
// Stages 2 and 3 are EMGPU_PAIR_TOTALS, text and not a function template: as a function (one call, or a wave sum and an add) the register
// allocation of every kernel moved, while the text compiles to what the four written-out copies did (HISTORY.md section 42).
#pragma once
#include "emgpu_pairs.h"

constexpr int kBlock = 256, kWaves = kBlock / 64;

__device__ __forceinline__ bool finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }   // a NaN compares false

// The pose of pair i as the declarations of c, s, ox, oy, oz: B is turned by (c, s) about its own origin, then moved by (ox, oy, oz);
// without POSE it stays where it is.  Text, as EMGPU_PAIR_POINT below: as functions (the pose as a struct or as five references, the point
// taking either) the two leave k_miss_segments as it was and move the registers of the other three kernels (HISTORY.md section 42).
#define EMGPU_PAIR_POSE(pose, n_pairs, i)                                                                                            \
    double c = 1.0, s = 0.0, ox = 0.0, oy = 0.0, oz = 0.0;                                                                           \
    if (POSE) {                                                                                                                      \
        const double *q = pose + (size_t)i;                                                                                          \
        const size_t np = (size_t)n_pairs;                                                                                           \
        c = q[0]; s = q[np]; ox = q[2 * np]; oy = q[3 * np]; oz = q[4 * np];                                                         \
    }

// A point of the pair as the declarations of dx, dy, dz: a and b at its second in columns of pitch lda and ldb, B posed by q, then
// (dx, dy) = A - B and dz = B - A.
#define EMGPU_PAIR_POINT(a, b, lda, ldb)                                                                                             \
    const double xa = a[0], ya = a[lda], za = a[2 * lda];                                                                            \
    double xb = b[0], yb = b[ldb], zb = b[2 * ldb];                                                                                  \
    if (POSE) {                                                                                                                      \
        const double xr = (c * xb - s * yb) + ox, yr = (s * xb + c * yb) + oy;                                                       \
        xb = xr; yb = yr; zb = zb + oz;                                                                                              \
    }                                                                                                                                \
    const double dx = xa - xb, dy = ya - yb, dz = zb - za;

// The alerting volume of k_well_clear and k_avoid at a point (x, y, z) of relative velocity (ux, uy), as declarations: modified tau
// against A.D2 = DMOD^2 (0 inside DMOD, infinite when not closing), the time tc to the horizontal closest approach, never negative, and
// the predicted miss there against A.H2 = HMD^2; `in_volume` names the result, a valid point within A.h vertically that is inside DMOD
// or caught by tau.  Text: as a function returning a struct it costs k_avoid six registers and a wave per SIMD, and with out-parameters
// either that or other code in both kernels (HISTORY.md section 42).
#define EMGPU_TAU_POINT(A, x, y, z, ux, uy, in_volume)                                                                               \
    const double rr = x * x + y * y, rv = x * ux + y * uy, vv = ux * ux + uy * uy;                                                   \
    const bool valid = finite(rr) && finite(rv) && finite(vv) && finite(z);                                                          \
    const bool inside = rr <= A.D2, closing = rv < 0.0;                                                                              \
    const double tau = inside ? 0.0 : (closing ? (A.D2 - rr) / rv : __builtin_inf());                                                \
    double tc = vv > 0.0 ? (-rv) / vv : 0.0;                                                                                         \
    tc = tc > 0.0 ? tc : 0.0;                                                                                                        \
    const double px = x + tc * ux, py = y + tc * uy, hp2 = px * px + py * py;                                                        \
    const bool by_tau = !inside && closing && tau <= A.tau_s && hp2 <= A.H2;                                                         \
    const bool in_volume = valid && __builtin_fabs(z) <= A.h && (inside || by_tau);

// Stages 2 and 3 on the lane's counters `...` (N of them, in the order of the entry point's totals), through part[kWaves][N] in LDS.
// Every lane of the workgroup comes here or none.
#define EMGPU_PAIR_TOTALS(N, part, totals, ...)                                                                                      \
    {                                                                                                                                \
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;                                                                  \
        unsigned long long v[N] = {__VA_ARGS__};                                                                                     \
        _Pragma("unroll") for (int k = 0; k < N; k++) {                                                                              \
            unsigned long long x = v[k];                                                                                             \
            _Pragma("unroll") for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);                                            \
            if (lane == 0) part[wave][k] = x;                                                                                        \
        }                                                                                                                            \
        __syncthreads();                                                                                                             \
        if (threadIdx.x < N) {                                                                                                       \
            unsigned long long x = 0ull;                                                                                             \
            _Pragma("unroll") for (int w = 0; w < kWaves; w++) x += part[w][threadIdx.x];                                            \
            if (x) (void)__hip_atomic_fetch_add(totals + threadIdx.x, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);                \
        }                                                                                                                            \
    }

// The launch of a walking kernel on A's pairs: the instance with a pose where A carries one; its name for the caller that asks.
template <class Run>
hipError_t launch_pair_walk(const Run &A, hipStream_t s, const char **name, void (*posed)(const Run), const char *posed_name,
                            void (*plain)(const Run), const char *plain_name) {
    if (name) *name = A.pose ? posed_name : plain_name;
    if (A.dim.n_pairs <= 0) return hipSuccess;
    hipLaunchKernelGGL(A.pose ? posed : plain, pair_grid(A.dim.n_pairs, kBlock), dim3(kBlock), 0, s, A);
    return hipGetLastError();
}
