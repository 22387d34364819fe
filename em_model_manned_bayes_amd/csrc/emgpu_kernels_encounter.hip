// emgpu_kernels_encounter.hip -- k_encounter_pose: per pair of 1 Hz tracks a random heading of the intruder, its entry point on the
// encounter cylinder around the ownship, the pose {c, s, ox, oy, oz} k_miss_distance reads, the swept volume per second and integer weights
// with that rate folded in; one lane per pair, 256-lane workgroups.  The definition is in emgpu_encounter.h.
//
// Memory: per lane twelve 8-byte loads, points 0 and 1 of both sets, coalesced along the pair index where the indices are the identity
// (with n_x == 1 the wave names one address per coordinate; through arbitrary indices a lane's load is alone in its sector), and up to
// 8 + 8 + 1 + 4 bytes of index, weight and outputs per pair, all plain vector loads and stores, coalesced.  Nothing is shared between
// lanes: no LDS, no atomics.
// Draws: Philox blocks of section 13.  The heading's disc point costs one block per two attempts (1.27 attempts on average: one block
// for 95 % of the lanes), the surface / offset / height draws one block, an end-cap position one more per two attempts -- only for the
// lanes that enter through an end.  The rejection loops run on lane predicates, bounded by max_attempts; no lane leaves before the stores.
// A pair with an index outside its set loads nothing and draws nothing.
// The grid is min(tiles, 2048) workgroups that walk the 256-pair tiles, as k_miss_distance's.
// The compiler's figures (registers, LDS, scratch) are in DESIGN.md section 33.
#include <hip/hip_runtime.h>

#include "emgpu_device.h"
#include "emgpu_disc.h"
#include "emgpu_encounter.h"

namespace {
constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void k_encounter_pose(const EmgpuEncounterRun A) {
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    const uint32_t k0 = (uint32_t)A.seed, k1 = (uint32_t)(A.seed >> 32);
    const size_t np = (size_t)A.dim.n_pairs, la = (size_t)A.dim.ld_a, lb = (size_t)A.dim.ld_b;
    // tile j of this workgroup: pairs (blockIdx.x + j * gridDim.x) * 256 ...
    for (int64_t tile = blockIdx.x; tile * kBlock < A.dim.n_pairs; tile += gridDim.x) {
        const int64_t i = tile * kBlock + threadIdx.x;
        if (i >= A.dim.n_pairs) continue;
        const int64_t ia = pair_column(A.col.idx_a, A.dim.n_a, i), ib = pair_column(A.col.idx_b, A.dim.n_b, i);
        const bool bad = ia < 0 || ia >= A.dim.n_a || ib < 0 || ib >= A.dim.n_b;   // (spelled here: in a shared helper it moves registers)
        double c = nan, s = nan, ox = nan, oy = nan, oz = nan, rate = 0.0;
        uint32_t fl = EMGPU_ENC_BAD_INDEX, wout = 0u;
        if (!bad) {
            const uint64_t g = A.first_index + (uint64_t)i;
            const uint32_t g_lo = (uint32_t)g, g_hi = (uint32_t)(g >> 32);
            const double *a = A.col.xyz_a + (size_t)ia, *b = A.col.xyz_b + (size_t)ib;
            const double a0x = a[0], a0y = a[la], a0z = a[2 * la], a1x = a[3 * la], a1y = a[4 * la], a1z = a[5 * la];
            const double b0x = b[0], b0y = b[lb], b0z = b[2 * lb], b1x = b[3 * lb], b1y = b[4 * lb], b1z = b[5 * lb];
            // 1. the displacements of the first second
            const double ax = a1x - a0x, ay = a1y - a0y, az = a1z - a0z;
            const double bx = b1x - b0x, by = b1y - b0y, bz = b1z - b0z;
            // 2. the heading
            double p, q;
            fl = disc_point(g_lo, g_hi, k0, k1, 0u, A.max_attempts, p, q) ? 0u : EMGPU_ENC_FALLBACK;
            const double r = __builtin_sqrt(p * p + q * q);
            c = p / r; s = q / r;
            const double vx = c * bx - s * by, vy = s * bx + c * by;
            // 3. the intruder's velocity relative to the ownship
            const double rx = vx - ax, ry = vy - ay, wr = bz - az;
            const double gh = __builtin_sqrt(rx * rx + ry * ry);
            // 4. the volume swept per second, through the side and through the ends
            const double Qs = A.ks * gh, Qe = A.ke * __builtin_fabs(wr);
            const double Q = Qs + Qe;
            if (Q > 0.0 && Q < inf) {
                // 5. the entry point
                const uint4 v = emgpu::philox4x32(g_lo, g_hi, 0u, (EMGPU_SEC_ENCOUNTER << 28) | (2u << 20), k0, k1);
                double relx, rely, dz;
                if (emgpu::uniform32(v.x) * Q < Qs) {
                    const double ex = rx / gh, ey = ry / gh;
                    const double m = centred(v.y);
                    const double l = A.R * m, h = A.R * __builtin_sqrt(1.0 - m * m);
                    relx = (-h) * ex - l * ey; rely = l * ex - h * ey;
                    dz = A.H * centred(v.z);
                } else {
                    double pe, qe;
                    fl |= EMGPU_ENC_END | (disc_point(g_lo, g_hi, k0, k1, 1u, A.max_attempts, pe, qe) ? 0u : EMGPU_ENC_FALLBACK);
                    relx = A.R * pe; rely = A.R * qe;
                    dz = wr < 0.0 ? A.H : -A.H;
                }
                // 6. the pose that puts B's point 0 there
                ox = (a0x + relx) - (c * b0x - s * b0y);
                oy = (a0y + rely) - (s * b0x + c * b0y);
                oz = (a0z + dz) - b0z;
                rate = Q;
                if (A.weights_out) {
                    const double w = A.weights_in ? (double)A.weights_in[i] : 1.0;
                    const double f = __builtin_floor(w * (Q / A.rate_scale) + 0.5);
                    const bool fits = f <= 4294967295.0;      // (false for a NaN: 0 * inf)
                    wout = fits ? (uint32_t)f : 0xFFFFFFFFu;
                    fl |= fits ? 0u : EMGPU_ENC_SATURATED;
                }
            } else {
                fl |= EMGPU_ENC_NO_ENTRY;
            }
        }
        if (A.pose) {
            double *o = A.pose + (size_t)i;
            o[0] = c; o[np] = s; o[2 * np] = ox; o[3 * np] = oy; o[4 * np] = oz;
        }
        if (A.rate) A.rate[i] = rate;
        if (A.flags) A.flags[i] = (uint8_t)fl;
        if (A.weights_out) A.weights_out[i] = wout;
    }
}
} // namespace

namespace emgpu {
hipError_t launch_encounter_pose(const EmgpuEncounterRun &A, hipStream_t s, const char **name) {
    if (name) *name = "k_encounter_pose";
    if (A.dim.n_pairs <= 0) return hipSuccess;
    const dim3 grid = pair_grid(A.dim.n_pairs, kBlock);
    hipLaunchKernelGGL(k_encounter_pose, grid, dim3(kBlock), 0, s, A);
    return hipGetLastError();
}
} // namespace emgpu
