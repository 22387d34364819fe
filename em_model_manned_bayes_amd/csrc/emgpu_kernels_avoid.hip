// emgpu_kernels_avoid.hip -- k_avoid<POSE>: the ownship's vertical avoidance manoeuvre on paired 1 Hz tracks.  Per pair the second of the
// first alert (k_well_clear's predicate with the alert thresholds), the sense fixed there, and the NMAC and the vertical miss with and
// without the manoeuvre that follows.  One lane per pair, 256-lane workgroups, sequential in time: k_well_clear's shape
// (emgpu_kernels_well_clear.hip).  The definition is in emgpu_avoid.h.
//
// Memory: k_miss_distance's six 8-byte loads per (second, lane), and nothing more.  The manoeuvre is a closed form of the seconds since
// the alert, so no mitigated track is ever written or read: dz'[p] is formed in a register when point p arrives.  The previous point's
// dx, dy, dz stay in three registers; when point p arrives the alert of point p-1 is evaluated with the forward difference as its velocity
// (if no alert has fired), then dz'[p] is formed, then the two NMAC tests and the CPA see the point.  The last point's alert is evaluated
// behind the loop; it can only be LATE.  Everything that depends on a coordinate is a select: no lane branches on data.  (A wave-uniform
// skip of the alert's two divisions once every lane of a wave has alerted was tried and left out: the vote keeps the compiler from
// unrolling the loop over the seconds, which is what keeps twelve loads in flight per lane.)
// The totals are reduced in the sibling kernels' three stages, twelve counters wide: u32 / u64 registers per lane, a shuffle reduction per
// wave into one 64-bit LDS slot per (wave, counter), one relaxed agent-scope 64-bit vector atomic without return per (workgroup, touched
// counter).  The per-pair outputs are plain vector stores, coalesced.  No float atomic, no scratch.
// Compiler's figures (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): <no pose> 81 VGPRs, <pose> 91 VGPRs; 106 SGPRs, 384 bytes
// of LDS, no scratch, 5 waves per SIMD for both.
#include <hip/hip_runtime.h>

#include "emgpu_avoid.h"

namespace {
constexpr int kBlock = 256, kWaves = kBlock / 64, kTotals = 12;

__device__ __forceinline__ bool finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }   // a NaN compares false

// the alert of point p of the pair: (x, y, z) = (dx, dy, dz)[p] and its relative velocity (ux, uy, wz); the first one sets t_alert and the sense
__device__ __forceinline__ void alert_point(const EmgpuAvoidRun &A, int p, double x, double y, double z, double ux, double uy, double wz,
                                            int32_t &t_alert, bool &climb) {
    const double rr = x * x + y * y, rv = x * ux + y * uy, vv = ux * ux + uy * uy;
    const bool valid = finite(rr) && finite(rv) && finite(vv) && finite(z);
    const bool inside = rr <= A.D2, closing = rv < 0.0;
    const double tau = inside ? 0.0 : (closing ? (A.D2 - rr) / rv : __builtin_inf());
    double tc = vv > 0.0 ? (-rv) / vv : 0.0;
    tc = tc > 0.0 ? tc : 0.0;
    const double px = x + tc * ux, py = y + tc * uy, hp2 = px * px + py * py;
    const bool by_tau = !inside && closing && tau <= A.tau_s && hp2 <= A.H2;
    const bool alert = valid && __builtin_fabs(z) <= A.h && (inside || by_tau);
    const double zp = z + tc * wz;   // the intruder's vertical offset at the horizontal closest approach
    const bool descend = zp > 0.0 || (!(zp < 0.0) && z > 0.0);
    const bool fire = alert && t_alert < 0;
    t_alert = fire ? p : t_alert;
    climb = fire ? !descend : climb;
}

template <bool POSE>
__global__ __launch_bounds__(kBlock) void k_avoid(const EmgpuAvoidRun A) {
    __shared__ unsigned long long part[kWaves][kTotals];
    const double nan = __builtin_nan("");
    uint32_t n_eval = 0u, n_alert = 0u, n_unmit = 0u, n_mit = 0u, n_ind = 0u, n_none = 0u, n_bad = 0u;
    unsigned long long w_eval = 0ull, w_alert = 0ull, w_unmit = 0ull, w_mit = 0ull, w_ind = 0ull;
    const size_t lda = (size_t)A.dim.ld_a, ldb = (size_t)A.dim.ld_b, step_a = 3 * lda, step_b = 3 * ldb;
    // tile j of this workgroup: pairs (blockIdx.x + j * gridDim.x) * 256 ...
    for (int64_t tile = blockIdx.x; tile * kBlock < A.dim.n_pairs; tile += gridDim.x) {
        const int64_t i = tile * kBlock + threadIdx.x;
        if (i >= A.dim.n_pairs) continue;
        const int64_t ia = pair_column(A.col.idx_a, A.dim.n_a, i), ib = pair_column(A.col.idx_b, A.dim.n_b, i);
        const bool bad = ia < 0 || ia >= A.dim.n_a || ib < 0 || ib >= A.dim.n_b;
        double best = nan, vmd = nan, vmit = nan;
        int32_t t = -1, t_alert = -1;
        uint32_t fl = EMGPU_AVOID_BAD_INDEX;
        if (!bad) {
            double c = 1.0, s = 0.0, ox = 0.0, oy = 0.0, oz = 0.0;
            if (POSE) {
                const double *q = A.pose + (size_t)i;
                const size_t np = (size_t)A.dim.n_pairs;
                c = q[0]; s = q[np]; ox = q[2 * np]; oy = q[3 * np]; oz = q[4 * np];
            }
            const double *a = A.col.xyz_a + (size_t)ia, *b = A.col.xyz_b + (size_t)ib;
            double x0 = 0.0, y0 = 0.0, z0 = 0.0, ux = 0.0, uy = 0.0, wz = 0.0;
            bool climb = false, unmit = false, mit = false;
#pragma unroll 2
            for (int p = 0; p < A.P; p++, a += step_a, b += step_b) {
                const double xa = a[0], ya = a[lda], za = a[2 * lda];
                double xb = b[0], yb = b[ldb], zb = b[2 * ldb];
                if (POSE) {
                    const double xr = (c * xb - s * yb) + ox, yr = (s * xb + c * yb) + oy;
                    xb = xr; yb = yr; zb = zb + oz;
                }
                const double dx = xa - xb, dy = ya - yb, dz = zb - za;
                if (p > 0) {   // (uniform) the alert of the second before, now that its forward difference is known
                    ux = dx - x0; uy = dy - y0; wz = dz - z0;
                    alert_point(A, p - 1, x0, y0, z0, ux, uy, wz, t_alert, climb);
                }
                // dz'[p]: the ownship has moved g feet k = p - t0 seconds after the response began
                const int32_t k = p - (t_alert + A.delay);
                const double kd = (double)k;
                double g = kd < A.tr ? A.half_a * (kd * kd) : A.rate * (kd - A.half_tr);
                g = g < A.dz_max ? g : A.dz_max;
                const double zg = climb ? dz - g : dz + g, zm = (t_alert >= 0 && k >= 1) ? zg : dz;
                const double d = __builtin_sqrt(dx * dx + dy * dy);
                const bool take = d == d && (t < 0 || d < best);   // the first of equal roots stays; a NaN never enters
                best = take ? d : best;
                vmd = take ? dz : vmd;
                vmit = take ? zm : vmit;
                t = take ? p : t;
                unmit = unmit || (d < A.nmac_h && __builtin_fabs(dz) < A.nmac_v);
                mit = mit || (d < A.nmac_h && __builtin_fabs(zm) < A.nmac_v);
                x0 = dx; y0 = dy; z0 = dz;
            }
            alert_point(A, A.P - 1, x0, y0, z0, ux, uy, wz, t_alert, climb);   // the last point, with the last segment's velocity (P = 1: none, 0)
            const bool alerted = t_alert >= 0, late = alerted && t_alert + A.delay >= A.P - 1, ind = mit && !unmit;
            fl = (alerted ? EMGPU_AVOID_ALERTED : 0u) | (climb ? EMGPU_AVOID_CLIMB : 0u) | (unmit ? EMGPU_AVOID_NMAC_UNMIT : 0u) |
                 (mit ? EMGPU_AVOID_NMAC_MIT : 0u) | (late ? EMGPU_AVOID_LATE : 0u) | (t < 0 ? EMGPU_AVOID_NO_CPA : 0u);
            const unsigned long long w = A.weights ? (unsigned long long)A.weights[i] : 1ull;
            n_eval += 1u; n_alert += alerted ? 1u : 0u; n_unmit += unmit ? 1u : 0u; n_mit += mit ? 1u : 0u; n_ind += ind ? 1u : 0u;
            n_none += t < 0 ? 1u : 0u;
            w_eval += w; w_alert += alerted ? w : 0ull; w_unmit += unmit ? w : 0ull; w_mit += mit ? w : 0ull; w_ind += ind ? w : 0ull;
        } else {
            n_bad += 1u;
        }
        if (A.hmd) A.hmd[i] = best;
        if (A.vmd) A.vmd[i] = vmd;
        if (A.vmd_mit) A.vmd_mit[i] = vmit;
        if (A.t_cpa) A.t_cpa[i] = t;
        if (A.t_alert) A.t_alert[i] = t_alert;
        if (A.flags) A.flags[i] = (uint8_t)fl;
    }
    if (!A.totals) return;   // (uniform: every lane of the workgroup returns or none)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long v[kTotals] = {n_eval, n_alert, n_unmit, n_mit, n_ind, n_none, n_bad, w_eval, w_alert, w_unmit, w_mit, w_ind};
#pragma unroll
    for (int k = 0; k < kTotals; k++) {
        unsigned long long x = v[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
        if (lane == 0) part[wave][k] = x;
    }
    __syncthreads();
    if (threadIdx.x < kTotals) {
        unsigned long long x = 0ull;
#pragma unroll
        for (int w = 0; w < kWaves; w++) x += part[w][threadIdx.x];
        if (x) (void)__hip_atomic_fetch_add(A.totals + threadIdx.x, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
} // namespace

namespace emgpu {
hipError_t launch_avoid(const EmgpuAvoidRun &A, hipStream_t s, const char **name) {
    if (name) *name = A.pose ? "k_avoid[pose]" : "k_avoid";
    if (A.dim.n_pairs <= 0) return hipSuccess;
    const dim3 grid = pair_grid(A.dim.n_pairs, kBlock);   // the atomics of stage 3 are paid 2048 times at most
    if (A.pose) hipLaunchKernelGGL(k_avoid<true>, grid, dim3(kBlock), 0, s, A);
    else hipLaunchKernelGGL(k_avoid<false>, grid, dim3(kBlock), 0, s, A);
    return hipGetLastError();
}
} // namespace emgpu
