// emgpu_kernels_avoid.hip -- k_avoid<POSE>: the ownship's vertical avoidance manoeuvre on paired 1 Hz tracks.  Per pair the second of the
// first alert (k_well_clear's predicate, EMGPU_TAU_POINT, with the alert thresholds), the sense fixed there, and the NMAC and the vertical
// miss with and without the manoeuvre that follows.  One lane per pair, 256-lane workgroups, sequential in time: k_well_clear's shape
// (emgpu_kernels_well_clear.hip).  The definition is in emgpu_avoid.h.
//
// Memory: the walk's six 8-byte loads per (second, lane) (emgpu_pair_walk.h), and nothing more.  The manoeuvre is a closed form of the
// seconds since the alert, so no mitigated track is ever written or read: dz'[p] is formed in a register when point p arrives.  The previous
// point's dx, dy, dz stay in three registers; when point p arrives the alert of point p-1 is evaluated with the forward difference as its velocity
// (if no alert has fired), then dz'[p] is formed, then the two NMAC tests and the CPA see the point.  The last point's alert is evaluated
// behind the loop; it can only be LATE.  Everything that depends on a coordinate is a select: no lane branches on data.  (A wave-uniform
// skip of the alert's two divisions once every lane of a wave has alerted was tried and left out: the vote keeps the compiler from
// unrolling the loop over the seconds, which is what keeps twelve loads in flight per lane.)
// The twelve totals are reduced in the three stages of emgpu_pair_walk.h.  The per-pair outputs are plain vector stores, coalesced.
// Compiler's figures (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): <no pose> 81 VGPRs, <pose> 91 VGPRs; 106 SGPRs, 384 bytes
// of LDS, no scratch, 5 waves per SIMD for both.
#include <hip/hip_runtime.h>

#include "emgpu_avoid.h"
#include "emgpu_pair_walk.h"

namespace {
constexpr int kTotals = 12;

// the alert of point p of the pair: (x, y, z) = (dx, dy, dz)[p] and its relative velocity (ux, uy, wz); the first one sets t_alert and the sense
__device__ __forceinline__ void alert_point(const EmgpuAvoidRun &A, int p, double x, double y, double z, double ux, double uy, double wz,
                                            int32_t &t_alert, bool &climb) {
    EMGPU_TAU_POINT(A, x, y, z, ux, uy, alert)
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
            EMGPU_PAIR_POSE(A.pose, A.dim.n_pairs, i)
            const double *a = A.col.xyz_a + (size_t)ia, *b = A.col.xyz_b + (size_t)ib;
            double x0 = 0.0, y0 = 0.0, z0 = 0.0, ux = 0.0, uy = 0.0, wz = 0.0;
            bool climb = false, unmit = false, mit = false;
#pragma unroll 2
            for (int p = 0; p < A.P; p++, a += step_a, b += step_b) {
                EMGPU_PAIR_POINT(a, b, lda, ldb)
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
    EMGPU_PAIR_TOTALS(kTotals, part, A.totals, n_eval, n_alert, n_unmit, n_mit, n_ind, n_none, n_bad, w_eval, w_alert, w_unmit, w_mit, w_ind);
}
} // namespace

namespace emgpu {
hipError_t launch_avoid(const EmgpuAvoidRun &A, hipStream_t s, const char **name) {
    return launch_pair_walk(A, s, name, k_avoid<true>, "k_avoid[pose]", k_avoid<false>, "k_avoid");
}
} // namespace emgpu
