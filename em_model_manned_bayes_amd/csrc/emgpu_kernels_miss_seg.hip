// emgpu_kernels_miss_seg.hip -- k_miss_segments<POSE>: paired 1 Hz tracks read as piecewise linear into horizontal / vertical miss distance,
// a real-valued time of closest approach and NMAC flags that see what happens between two seconds.  One lane per pair, 256-lane workgroups,
// sequential in time: k_miss_distance's shape (emgpu_kernels_miss.hip).  The definition is in emgpu_miss_seg.h.
//
// Memory: the walk's six 8-byte loads per (second, lane) (emgpu_pair_walk.h), and nothing more: the previous second's dx, dy, dz stay in
// three registers, so a segment costs no load.  The running minimum, its time and dz there, and the NMAC bits stay in registers; the four
// per-pair outputs are plain vector stores, coalesced.  The minimum and the flags are selects in the source.  The arithmetic behind `near`
// (two divisions, a root) sits behind a lane branch: measured against the all-select form the two are within each other's spread,
// since the compiler guards the expensive operands of a select with an EXEC branch of its own either way.
// The totals are k_miss_distance's eight and two more, reduced in the three stages of emgpu_pair_walk.h.
// Compiler's figures (hipcc -O3, gfx950): <no pose> 79 VGPRs, 6 waves per SIMD; <pose> 89 VGPRs, 5 waves per SIMD; 106 SGPRs, 320 bytes of
// LDS, no scratch.
#include <hip/hip_runtime.h>

#include "emgpu_miss_seg.h"
#include "emgpu_pair_walk.h"

namespace {
constexpr int kTotals = 10;

template <bool POSE>
__global__ __launch_bounds__(kBlock) void k_miss_segments(const EmgpuMissSegRun A) {
    __shared__ unsigned long long part[kWaves][kTotals];
    const double nan = __builtin_nan("");
    const double H = A.nmac_h, V = A.nmac_v;
    uint32_t n_eval = 0u, n_cpa = 0u, n_any = 0u, n_none = 0u, n_bad = 0u, n_btw = 0u;
    unsigned long long w_eval = 0ull, w_cpa = 0ull, w_any = 0ull, w_btw = 0ull;
    const size_t lda = (size_t)A.dim.ld_a, ldb = (size_t)A.dim.ld_b, step_a = 3 * lda, step_b = 3 * ldb;
    // tile j of this workgroup: pairs (blockIdx.x + j * gridDim.x) * 256 ...
    for (int64_t tile = blockIdx.x; tile * kBlock < A.dim.n_pairs; tile += gridDim.x) {
        const int64_t i = tile * kBlock + threadIdx.x;
        if (i >= A.dim.n_pairs) continue;
        const int64_t ia = pair_column(A.col.idx_a, A.dim.n_a, i), ib = pair_column(A.col.idx_b, A.dim.n_b, i);
        const bool bad = ia < 0 || ia >= A.dim.n_a || ib < 0 || ib >= A.dim.n_b;
        double best = nan, vmd = nan, t = -1.0;
        uint32_t fl = EMGPU_MISS_BAD_INDEX;
        if (!bad) {
            EMGPU_PAIR_POSE(A.pose, A.dim.n_pairs, i)
            const double *a = A.col.xyz_a + (size_t)ia, *b = A.col.xyz_b + (size_t)ib;
            bool at_point = false, on_segment = false, inside = false;   // NMAC at some point; on some segment; the CPA is an interior one
            double x0 = 0.0, y0 = 0.0, z0 = 0.0;
#pragma unroll 2
            for (int p = 0; p < A.P; p++, a += step_a, b += step_b) {
                EMGPU_PAIR_POINT(a, b, lda, ldb)
                const double d = __builtin_sqrt(dx * dx + dy * dy);
                if (p > 0) {   // (uniform) the segment from the second before: its interior comes before this point
                    const double ex = dx - x0, ey = dy - y0, ez = dz - z0;
                    const double ee = ex * ex + ey * ey, re = x0 * ex + y0 * ey;
                    const bool valid = finite(ee) && finite(re) && finite(z0) && finite(ez);
                    const double ts = ee > 0.0 ? (-re) / ee : 0.0;
                    const double px = x0 + ts * ex, py = y0 + ts * ey;
                    const double ds = __builtin_sqrt(px * px + py * py), zs = z0 + ts * ez;
                    const bool take = valid && ts > 0.0 && ts < 1.0 && ds == ds && (t < 0.0 || ds < best);
                    best = take ? ds : best;
                    vmd = take ? zs : vmd;
                    t = take ? (double)(p - 1) + ts : t;
                    inside = take ? true : inside;
                    const bool near = valid && (z0 < dz ? z0 : dz) < V && (z0 < dz ? dz : z0) > -V;
                    if (near) {   // a lane branch: the two divisions and the root behind it are skipped by a wave with no lane in the band
                        const double t0 = (-V - z0) / ez, t1 = (V - z0) / ez;
                        const double mn = t0 < t1 ? t0 : t1, mx = t0 < t1 ? t1 : t0;
                        const double lo = ez != 0.0 ? (mn > 0.0 ? mn : 0.0) : 0.0, hi = ez != 0.0 ? (mx < 1.0 ? mx : 1.0) : 1.0;
                        double tc = ts;
                        tc = tc > lo ? tc : lo;
                        tc = tc < hi ? tc : hi;
                        const double qx = x0 + tc * ex, qy = y0 + tc * ey;
                        const double dc = __builtin_sqrt(qx * qx + qy * qy);
                        on_segment = on_segment || (lo < hi && dc < H);
                    }
                }
                const bool take = d == d && (t < 0.0 || d < best);   // the first of equal minima stays; a NaN never enters
                best = take ? d : best;
                vmd = take ? dz : vmd;
                t = take ? (double)p : t;
                inside = take ? false : inside;
                at_point = at_point || (d < H && __builtin_fabs(dz) < V);
                x0 = dx; y0 = dy; z0 = dz;
            }
            const bool cpa = best < H && __builtin_fabs(vmd) < V, any = at_point || on_segment, btw = on_segment && !at_point;
            fl = (cpa ? EMGPU_MISS_NMAC_CPA : 0u) | (any ? EMGPU_MISS_NMAC_ANY : 0u) | (t < 0.0 ? EMGPU_MISS_NO_CPA : 0u) |
                 (inside ? EMGPU_MISS_CPA_BETWEEN : 0u) | (btw ? EMGPU_MISS_NMAC_BETWEEN : 0u);
            const unsigned long long w = A.weights ? (unsigned long long)A.weights[i] : 1ull;
            n_eval += 1u; n_cpa += cpa ? 1u : 0u; n_any += any ? 1u : 0u; n_none += t < 0.0 ? 1u : 0u; n_btw += btw ? 1u : 0u;
            w_eval += w; w_cpa += cpa ? w : 0ull; w_any += any ? w : 0ull; w_btw += btw ? w : 0ull;
        } else {
            n_bad += 1u;
        }
        if (A.hmd) A.hmd[i] = best;
        if (A.vmd) A.vmd[i] = vmd;
        if (A.t_cpa_s) A.t_cpa_s[i] = t;
        if (A.flags) A.flags[i] = (uint8_t)fl;
    }
    if (!A.totals) return;   // (uniform: every lane of the workgroup returns or none)
    EMGPU_PAIR_TOTALS(kTotals, part, A.totals, n_eval, n_cpa, n_any, n_none, n_bad, w_eval, w_cpa, w_any, n_btw, w_btw);
}
} // namespace

namespace emgpu {
hipError_t launch_miss_segments(const EmgpuMissSegRun &A, hipStream_t s, const char **name) {
    return launch_pair_walk(A, s, name, k_miss_segments<true>, "k_miss_segments[pose]", k_miss_segments<false>, "k_miss_segments");
}
} // namespace emgpu
