// emgpu_kernels_cpa.hip -- k_cpa_pose: per pair of 1 Hz tracks a random heading of the intruder, a drawn second tc, a lateral miss and a
// vertical offset at that second, the pose {c, s, ox, oy, oz} k_miss_distance reads that makes the two aircraft, flying on as they do at tc,
// pass exactly so, the flux through the miss plane and integer weights with that rate folded in; one lane per pair, 256-lane workgroups.
// The definition is in emgpu_cpa.h.
//
// Memory: per lane ten 8-byte loads, points tc and tc + 1 of both sets (the definition's az and bz enter nothing: z of point tc + 1 is not
// loaded).  With t_lo == t_hi every lane reads the same two rows and the loads are coalesced along the pair index as k_encounter_pose's
// are; with a drawn second the lanes of a wave read up to `span` different rows and most loads are alone in their 64-byte sector.  Up to
// 8 + 8 + 4 bytes of index and weight in and 40 + 8 + 4 + 1 + 4 bytes out per pair, all plain vector loads and stores, coalesced.
// Nothing is shared between lanes: no LDS, no atomics.
// Draws: Philox blocks of section 13.  One block of stream a = 4 (u1, u2 and the second), then the heading's disc point of stream a = 3,
// one block per two attempts (emgpu_disc.h).  The rejection loop runs on lane predicates, bounded by max_attempts; no lane leaves before
// the stores.  A pair with an index outside its set loads nothing and draws nothing.
// The grid is min(tiles, 2048) workgroups that walk the 256-pair tiles, as k_miss_distance's.
// The compiler's figures (registers, LDS, scratch) are in DESIGN.md section 37.
#include <hip/hip_runtime.h>

#include "emgpu_cpa.h"
#include "emgpu_device.h"
#include "emgpu_disc.h"

namespace {
constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void k_cpa_pose(const EmgpuCpaRun A) {
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    const uint32_t k0 = (uint32_t)A.seed, k1 = (uint32_t)(A.seed >> 32);
    const size_t np = (size_t)A.dim.n_pairs, la = (size_t)A.dim.ld_a, lb = (size_t)A.dim.ld_b;
    // tile j of this workgroup: pairs (blockIdx.x + j * gridDim.x) * 256 ...
    for (int64_t tile = blockIdx.x; tile * kBlock < A.dim.n_pairs; tile += gridDim.x) {
        const int64_t i = tile * kBlock + threadIdx.x;
        if (i >= A.dim.n_pairs) continue;
        const int64_t ia = pair_column(A.col.idx_a, A.dim.n_a, i), ib = pair_column(A.col.idx_b, A.dim.n_b, i);
        const bool bad = ia < 0 || ia >= A.dim.n_a || ib < 0 || ib >= A.dim.n_b;
        double c = nan, s = nan, ox = nan, oy = nan, oz = nan, rate = 0.0;
        int32_t tc = -1;
        uint32_t fl = EMGPU_CPA_BAD_INDEX, wout = 0u;
        if (!bad) {
            const uint64_t g = A.first_index + (uint64_t)i;
            const uint32_t g_lo = (uint32_t)g, g_hi = (uint32_t)(g >> 32);
            // 0. the second: below t_lo + span, so points tc and tc + 1 lie inside the tracks (t_hi <= points - 2)
            const uint4 v = emgpu::philox4x32(g_lo, g_hi, 0u, (EMGPU_SEC_ENCOUNTER << 28) | (4u << 20), k0, k1);
            tc = A.t_lo + (int32_t)(((uint64_t)v.z * A.span) >> 32);
            const double *a = A.col.xyz_a + ((size_t)tc * 3 * la + (size_t)ia), *b = A.col.xyz_b + ((size_t)tc * 3 * lb + (size_t)ib);
            const double a0x = a[0], a0y = a[la], a0z = a[2 * la], a1x = a[3 * la], a1y = a[4 * la];
            const double b0x = b[0], b0y = b[lb], b0z = b[2 * lb], b1x = b[3 * lb], b1y = b[4 * lb];
            // 1. the horizontal displacements of second tc (az and bz enter nothing)
            const double ax = a1x - a0x, ay = a1y - a0y;
            const double bx = b1x - b0x, by = b1y - b0y;
            // 2. the heading
            double p, q;
            fl = disc_point(g_lo, g_hi, k0, k1, 3u, A.max_attempts, p, q) ? 0u : EMGPU_CPA_FALLBACK;
            const double r = __builtin_sqrt(p * p + q * q);
            c = p / r; s = q / r;
            const double vx = c * bx - s * by, vy = s * bx + c * by;
            // 3. the intruder's horizontal velocity relative to the ownship
            const double rx = vx - ax, ry = vy - ay;
            const double gh = __builtin_sqrt(rx * rx + ry * ry);
            // 4. the flux through the miss plane, 2 Hm x 2 Vm
            const double Q = A.kc * gh;
            if (Q > 0.0 && Q < inf) {
                // 5. the offsets at the pass: lateral, perpendicular to the relative velocity, and vertical
                const double ex = rx / gh, ey = ry / gh;
                const double l = A.Hm * centred(v.x);
                const double relx = (-l) * ey, rely = l * ex;
                const double dz = A.Vm * centred(v.y);
                // 6. the pose that puts B's point tc there
                ox = (a0x + relx) - (c * b0x - s * b0y);
                oy = (a0y + rely) - (s * b0x + c * b0y);
                oz = (a0z + dz) - b0z;
                rate = Q;
                if (A.weights_out) {
                    const double w = A.weights_in ? (double)A.weights_in[i] : 1.0;
                    const double f = __builtin_floor(w * (Q / A.rate_scale) + 0.5);
                    const bool fits = f <= 4294967295.0;      // (false for a NaN: 0 * inf)
                    wout = fits ? (uint32_t)f : 0xFFFFFFFFu;
                    fl |= fits ? 0u : EMGPU_CPA_SATURATED;
                }
            } else {
                fl |= EMGPU_CPA_NO_PASS;
            }
        }
        if (A.pose) {
            double *o = A.pose + (size_t)i;
            o[0] = c; o[np] = s; o[2 * np] = ox; o[3 * np] = oy; o[4 * np] = oz;
        }
        if (A.rate) A.rate[i] = rate;
        if (A.t_cpa) A.t_cpa[i] = tc;
        if (A.flags) A.flags[i] = (uint8_t)fl;
        if (A.weights_out) A.weights_out[i] = wout;
    }
}
} // namespace

namespace emgpu {
hipError_t launch_cpa_pose(const EmgpuCpaRun &A, hipStream_t s, const char **name) {
    if (name) *name = "k_cpa_pose";
    if (A.dim.n_pairs <= 0) return hipSuccess;
    const dim3 grid = pair_grid(A.dim.n_pairs, kBlock);
    hipLaunchKernelGGL(k_cpa_pose, grid, dim3(kBlock), 0, s, A);
    return hipGetLastError();
}
} // namespace emgpu
