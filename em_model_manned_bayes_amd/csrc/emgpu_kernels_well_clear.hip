// emgpu_kernels_well_clear.hip -- k_well_clear<POSE>: loss of DAA well clear of paired 1 Hz tracks (modified tau, DMOD, predicted horizontal
// miss, vertical separation) at every whole second.  One lane per pair, 256-lane workgroups, sequential in time: k_miss_distance's shape
// (emgpu_kernels_miss.hip).  The definition is in emgpu_well_clear.h.
//
// Memory: the walk's six 8-byte loads per (second, lane) (emgpu_pair_walk.h), and nothing more: the previous second's dx, dy, dz stay in
// three registers as in k_miss_segments, and point p-1 is evaluated when point p arrives, with the forward difference as its velocity.  The
// last point is evaluated behind the loop with the last velocity; both go through wc_point, the per-point text once.  The predicate (EMGPU_TAU_POINT,
// shared with k_avoid) is selects; its two divisions are the only expensive operands, and no root enters.  The per-pair outputs are plain
// vector stores, coalesced.  The ten totals are reduced in the three stages of emgpu_pair_walk.h.
// Compiler's figures (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): <no pose> 73 VGPRs, 6 waves per SIMD; <pose> 83 VGPRs,
// 5 waves per SIMD; 106 SGPRs, 320 bytes of LDS, no scratch, for both.
#include <hip/hip_runtime.h>

#include "emgpu_well_clear.h"
#include "emgpu_pair_walk.h"

namespace {
constexpr int kTotals = 10;

// what a lane keeps of its pair while it walks the seconds
struct WcState {
    double tau_min;
    int32_t t_first, n_lost;
    bool have, by_inside, by_tau;   // a valid point was seen; some lost point had `inside`; some had `by_tau`
};

// point p of the pair: (x, y, z) = (dx, dy, dz)[p] and its relative velocity (ux, uy), into st
__device__ __forceinline__ void wc_point(const EmgpuWellClearRun &A, int p, double x, double y, double z, double ux, double uy, WcState &st) {
    EMGPU_TAU_POINT(A, x, y, z, ux, uy, lost)
    const bool take = valid && (!st.have || tau < st.tau_min);
    st.tau_min = take ? tau : st.tau_min;
    st.have = st.have || valid;
    st.t_first = lost && st.t_first < 0 ? p : st.t_first;
    st.n_lost += lost ? 1 : 0;
    st.by_inside = st.by_inside || (lost && inside);
    st.by_tau = st.by_tau || (lost && by_tau);
}

template <bool POSE>
__global__ __launch_bounds__(kBlock) void k_well_clear(const EmgpuWellClearRun A) {
    __shared__ unsigned long long part[kWaves][kTotals];
    uint32_t n_eval = 0u, n_lost = 0u, n_start = 0u, n_none = 0u, n_bad = 0u, n_nmac = 0u;
    unsigned long long w_eval = 0ull, w_lost = 0ull, w_start = 0ull, w_nmac = 0ull;
    const size_t lda = (size_t)A.dim.ld_a, ldb = (size_t)A.dim.ld_b, step_a = 3 * lda, step_b = 3 * ldb;
    // tile j of this workgroup: pairs (blockIdx.x + j * gridDim.x) * 256 ...
    for (int64_t tile = blockIdx.x; tile * kBlock < A.dim.n_pairs; tile += gridDim.x) {
        const int64_t i = tile * kBlock + threadIdx.x;
        if (i >= A.dim.n_pairs) continue;
        const int64_t ia = pair_column(A.col.idx_a, A.dim.n_a, i), ib = pair_column(A.col.idx_b, A.dim.n_b, i);
        const bool bad = ia < 0 || ia >= A.dim.n_a || ib < 0 || ib >= A.dim.n_b;
        WcState st{__builtin_nan(""), -1, 0, false, false, false};
        uint32_t fl = EMGPU_WC_BAD_INDEX;
        if (!bad) {
            EMGPU_PAIR_POSE(A.pose, A.dim.n_pairs, i)
            const double *a = A.col.xyz_a + (size_t)ia, *b = A.col.xyz_b + (size_t)ib;
            double x0 = 0.0, y0 = 0.0, z0 = 0.0, ux = 0.0, uy = 0.0;
#pragma unroll 2
            for (int p = 0; p < A.P; p++, a += step_a, b += step_b) {
                EMGPU_PAIR_POINT(a, b, lda, ldb)
                if (p > 0) {   // (uniform) the second before, now that its forward difference is known
                    ux = dx - x0; uy = dy - y0;
                    wc_point(A, p - 1, x0, y0, z0, ux, uy, st);
                }
                x0 = dx; y0 = dy; z0 = dz;
            }
            wc_point(A, A.P - 1, x0, y0, z0, ux, uy, st);   // the last point, with the last segment's velocity (P = 1: none, 0)
            const bool lost = st.n_lost > 0, start = st.t_first == 0, none = !st.have;
            fl = (lost ? EMGPU_WC_LOST : 0u) | (start ? EMGPU_WC_AT_START : 0u) | (none ? EMGPU_WC_NO_DATA : 0u) |
                 (st.by_inside ? EMGPU_WC_INSIDE_DMOD : 0u) | (st.by_tau ? EMGPU_WC_BY_TAU : 0u);
            const unsigned long long w = A.weights ? (unsigned long long)A.weights[i] : 1ull;
            const bool nmac = lost && A.miss_flags && (A.miss_flags[i] & EMGPU_MISS_NMAC_ANY) != 0u;
            n_eval += 1u; n_lost += lost ? 1u : 0u; n_start += start ? 1u : 0u; n_none += none ? 1u : 0u; n_nmac += nmac ? 1u : 0u;
            w_eval += w; w_lost += lost ? w : 0ull; w_start += start ? w : 0ull; w_nmac += nmac ? w : 0ull;
        } else {
            n_bad += 1u;
        }
        if (A.t_first) A.t_first[i] = st.t_first;
        if (A.n_lost) A.n_lost[i] = st.n_lost;
        if (A.tau_min) A.tau_min[i] = st.tau_min;
        if (A.flags) A.flags[i] = (uint8_t)fl;
    }
    if (!A.totals) return;   // (uniform: every lane of the workgroup returns or none)
    EMGPU_PAIR_TOTALS(kTotals, part, A.totals, n_eval, n_lost, n_start, n_none, n_bad, w_eval, w_lost, w_start, n_nmac, w_nmac);
}
} // namespace

namespace emgpu {
hipError_t launch_well_clear(const EmgpuWellClearRun &A, hipStream_t s, const char **name) {
    return launch_pair_walk(A, s, name, k_well_clear<true>, "k_well_clear[pose]", k_well_clear<false>, "k_well_clear");
}
} // namespace emgpu
