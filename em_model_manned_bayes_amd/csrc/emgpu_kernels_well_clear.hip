// emgpu_kernels_well_clear.hip -- k_well_clear<POSE>: loss of DAA well clear of paired 1 Hz tracks (modified tau, DMOD, predicted horizontal
// miss, vertical separation) at every whole second.  One lane per pair, 256-lane workgroups, sequential in time: k_miss_distance's shape
// (emgpu_kernels_miss.hip).  The definition is in emgpu_well_clear.h.
//
// Memory: k_miss_distance's six 8-byte loads per (second, lane), and nothing more: the previous second's dx, dy, dz stay in three registers
// as in k_miss_segments, and point p-1 is evaluated when point p arrives, with the forward difference as its velocity.  The last point is
// evaluated behind the loop with the last velocity; both go through wc_point, the per-point text once.  The predicate is selects; its two
// divisions are the only expensive operands, and no root enters.  The per-pair outputs are plain vector stores, coalesced.
// The totals are reduced in the sibling kernels' three stages, ten counters wide: u32 / u64 registers per lane, a shuffle reduction per
// wave into one 64-bit LDS slot per (wave, counter), one relaxed agent-scope 64-bit vector atomic without return per (workgroup, touched
// counter).  No float atomic, no scratch.
// Compiler's figures (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): <no pose> 73 VGPRs, 6 waves per SIMD; <pose> 83 VGPRs,
// 5 waves per SIMD; 106 SGPRs, 320 bytes of LDS, no scratch, for both.
#include <hip/hip_runtime.h>

#include "emgpu_well_clear.h"

namespace {
constexpr int kBlock = 256, kWaves = kBlock / 64, kTotals = 10;

__device__ __forceinline__ bool finite(double x) { return __builtin_fabs(x) < __builtin_inf(); }   // a NaN compares false

// what a lane keeps of its pair while it walks the seconds
struct WcState {
    double tau_min;
    int32_t t_first, n_lost;
    bool have, by_inside, by_tau;   // a valid point was seen; some lost point had `inside`; some had `by_tau`
};

// point p of the pair: (x, y, z) = (dx, dy, dz)[p] and its relative velocity (ux, uy), into st
__device__ __forceinline__ void wc_point(const EmgpuWellClearRun &A, int p, double x, double y, double z, double ux, double uy, WcState &st) {
    const double rr = x * x + y * y, rv = x * ux + y * uy, vv = ux * ux + uy * uy;
    const bool valid = finite(rr) && finite(rv) && finite(vv) && finite(z);
    const bool inside = rr <= A.D2, closing = rv < 0.0;
    const double tau = inside ? 0.0 : (closing ? (A.D2 - rr) / rv : __builtin_inf());
    double tc = vv > 0.0 ? (-rv) / vv : 0.0;
    tc = tc > 0.0 ? tc : 0.0;
    const double px = x + tc * ux, py = y + tc * uy, hp2 = px * px + py * py;
    const bool by_tau = !inside && closing && tau <= A.tau_s && hp2 <= A.H2;
    const bool lost = valid && __builtin_fabs(z) <= A.h && (inside || by_tau);
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
            double c = 1.0, s = 0.0, ox = 0.0, oy = 0.0, oz = 0.0;
            if (POSE) {
                const double *q = A.pose + (size_t)i;
                const size_t np = (size_t)A.dim.n_pairs;
                c = q[0]; s = q[np]; ox = q[2 * np]; oy = q[3 * np]; oz = q[4 * np];
            }
            const double *a = A.col.xyz_a + (size_t)ia, *b = A.col.xyz_b + (size_t)ib;
            double x0 = 0.0, y0 = 0.0, z0 = 0.0, ux = 0.0, uy = 0.0;
#pragma unroll 2
            for (int p = 0; p < A.P; p++, a += step_a, b += step_b) {
                const double xa = a[0], ya = a[lda], za = a[2 * lda];
                double xb = b[0], yb = b[ldb], zb = b[2 * ldb];
                if (POSE) {
                    const double xr = (c * xb - s * yb) + ox, yr = (s * xb + c * yb) + oy;
                    xb = xr; yb = yr; zb = zb + oz;
                }
                const double dx = xa - xb, dy = ya - yb, dz = zb - za;
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
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long v[kTotals] = {n_eval, n_lost, n_start, n_none, n_bad, w_eval, w_lost, w_start, n_nmac, w_nmac};
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
hipError_t launch_well_clear(const EmgpuWellClearRun &A, hipStream_t s, const char **name) {
    if (name) *name = A.pose ? "k_well_clear[pose]" : "k_well_clear";
    if (A.dim.n_pairs <= 0) return hipSuccess;
    const dim3 grid = pair_grid(A.dim.n_pairs, kBlock);   // the atomics of stage 3 are paid 2048 times at most
    if (A.pose) hipLaunchKernelGGL(k_well_clear<true>, grid, dim3(kBlock), 0, s, A);
    else hipLaunchKernelGGL(k_well_clear<false>, grid, dim3(kBlock), 0, s, A);
    return hipGetLastError();
}
} // namespace emgpu
