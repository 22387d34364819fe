// emgpu_kernels_miss.hip -- k_miss_distance<POSE>: paired 1 Hz tracks into horizontal / vertical miss distance, time of closest approach
// and NMAC flags, one lane per pair, 256-lane workgroups, sequential in time.  The definition is in emgpu_miss.h.
//
// Memory: the walk of emgpu_pair_walk.h, six 8-byte loads per (second, lane) and the pose once.  The running minimum, its second and dz
// there, and the two NMAC bits stay in registers; the four per-pair outputs are plain vector stores, coalesced.  No lane branches on a
// coordinate: the minimum and the flags are selects.  A pair with an index outside its set loads nothing.
// The totals, five counts and three weighted sums, are reduced in the three stages of emgpu_pair_walk.h.
// Compiler's figures (hipcc -O3, gfx950): <no pose> 64 VGPRs, <pose> 79 VGPRs, 256 bytes of LDS, no scratch.
#include <hip/hip_runtime.h>

#include "emgpu_miss.h"
#include "emgpu_pair_walk.h"

namespace {
constexpr int kTotals = 8;

template <bool POSE>
__global__ __launch_bounds__(kBlock) void k_miss_distance(const EmgpuMissRun A) {
    __shared__ unsigned long long part[kWaves][kTotals];
    const double nan = __builtin_nan("");
    uint32_t n_eval = 0u, n_cpa = 0u, n_any = 0u, n_none = 0u, n_bad = 0u;
    unsigned long long w_eval = 0ull, w_cpa = 0ull, w_any = 0ull;
    const size_t step_a = 3 * (size_t)A.dim.ld_a, step_b = 3 * (size_t)A.dim.ld_b;
    // tile j of this workgroup: pairs (blockIdx.x + j * gridDim.x) * 256 ...
    for (int64_t tile = blockIdx.x; tile * kBlock < A.dim.n_pairs; tile += gridDim.x) {
        const int64_t i = tile * kBlock + threadIdx.x;
        if (i >= A.dim.n_pairs) continue;
        const int64_t ia = pair_column(A.col.idx_a, A.dim.n_a, i), ib = pair_column(A.col.idx_b, A.dim.n_b, i);
        const bool bad = ia < 0 || ia >= A.dim.n_a || ib < 0 || ib >= A.dim.n_b;   // (spelled here: in a shared helper it moves registers)
        double best = nan, vmd = nan;
        int32_t t = -1;
        uint32_t fl = EMGPU_MISS_BAD_INDEX;
        if (!bad) {
            EMGPU_PAIR_POSE(A.pose, A.dim.n_pairs, i)
            const double *a = A.col.xyz_a + (size_t)ia, *b = A.col.xyz_b + (size_t)ib;
            bool any = false;
#pragma unroll 4
            for (int p = 0; p < A.P; p++, a += step_a, b += step_b) {
                EMGPU_PAIR_POINT(a, b, (size_t)A.dim.ld_a, (size_t)A.dim.ld_b)
                const double d = __builtin_sqrt(dx * dx + dy * dy);
                const bool take = d == d && (t < 0 || d < best);   // the first of equal roots stays; a NaN never enters
                best = take ? d : best;
                vmd = take ? dz : vmd;
                t = take ? p : t;
                any = any || (d < A.nmac_h && __builtin_fabs(dz) < A.nmac_v);
            }
            const bool cpa = best < A.nmac_h && __builtin_fabs(vmd) < A.nmac_v;
            fl = (cpa ? EMGPU_MISS_NMAC_CPA : 0u) | (any ? EMGPU_MISS_NMAC_ANY : 0u) | (t < 0 ? EMGPU_MISS_NO_CPA : 0u);
            const unsigned long long w = A.weights ? (unsigned long long)A.weights[i] : 1ull;
            n_eval += 1u; n_cpa += cpa ? 1u : 0u; n_any += any ? 1u : 0u; n_none += t < 0 ? 1u : 0u;
            w_eval += w; w_cpa += cpa ? w : 0ull; w_any += any ? w : 0ull;
        } else {
            n_bad += 1u;
        }
        if (A.hmd) A.hmd[i] = best;
        if (A.vmd) A.vmd[i] = vmd;
        if (A.t_cpa) A.t_cpa[i] = t;
        if (A.flags) A.flags[i] = (uint8_t)fl;
    }
    if (!A.totals) return;   // (uniform: every lane of the workgroup returns or none)
    EMGPU_PAIR_TOTALS(kTotals, part, A.totals, n_eval, n_cpa, n_any, n_none, n_bad, w_eval, w_cpa, w_any);
}
} // namespace

namespace emgpu {
hipError_t launch_miss_distance(const EmgpuMissRun &A, hipStream_t s, const char **name) {
    return launch_pair_walk(A, s, name, k_miss_distance<true>, "k_miss_distance[pose]", k_miss_distance<false>, "k_miss_distance");
}
} // namespace emgpu
