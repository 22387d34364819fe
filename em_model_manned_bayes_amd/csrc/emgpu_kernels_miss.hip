// emgpu_kernels_miss.hip -- k_miss_distance<POSE>: paired 1 Hz tracks into horizontal / vertical miss distance, time of closest approach
// and NMAC flags, one lane per pair, 256-lane workgroups, sequential in time.  The definition is in emgpu_miss.h.
//
// Memory: per (second, lane) six 8-byte loads, three of each set, coalesced along the pair index where the indices are the identity; with
// one column in a set (n_x == 1) the 64 lanes of a wave name one address per coordinate; through arbitrary indices a lane's load is alone
// in its 64-byte sector.  The pose's five doubles are read once per lane.  The running minimum, its second and dz there, and the two NMAC
// bits stay in registers; the four per-pair outputs are plain vector stores, coalesced.  No lane branches on a coordinate: the minimum and
// the flags are selects.  A pair with an index outside its set loads nothing.
// The totals are integers, so the order of the adds does not matter; they are reduced in three stages:
//   1. registers per lane over the workgroup's tiles: u32 for the five counts (a lane takes at most 2^32 / 256 / 2048 = 8192 pairs of a
//      call), u64 for the three weighted sums (8192 * (2^32 - 1) < 2^45);
//   2. a shuffle reduction per wave on 64-bit values, one 64-bit LDS slot per (wave, counter);
//   3. one 64-bit vector atomic without return (global_atomic_add_x2, relaxed, agent scope) per (workgroup, touched counter).
// Every partial from stage 2 on is 64-bit, so none can wrap and the grid needs no cap on the tiles of a workgroup: it is
// min(tiles, 2048) workgroups that walk the tiles.
// Compiler's figures (hipcc -O3, gfx950): <no pose> 64 VGPRs, <pose> 79 VGPRs, 256 bytes of LDS, no scratch.
#include <hip/hip_runtime.h>

#include "emgpu_miss.h"

namespace {
constexpr int kBlock = 256, kWaves = kBlock / 64, kTotals = 8;

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
            double c = 1.0, s = 0.0, ox = 0.0, oy = 0.0, oz = 0.0;
            if (POSE) {
                const double *q = A.pose + (size_t)i;
                const size_t np = (size_t)A.dim.n_pairs;
                c = q[0]; s = q[np]; ox = q[2 * np]; oy = q[3 * np]; oz = q[4 * np];
            }
            const double *a = A.col.xyz_a + (size_t)ia, *b = A.col.xyz_b + (size_t)ib;
            bool any = false;
#pragma unroll 4
            for (int p = 0; p < A.P; p++, a += step_a, b += step_b) {
                const double xa = a[0], ya = a[(size_t)A.dim.ld_a], za = a[2 * (size_t)A.dim.ld_a];
                double xb = b[0], yb = b[(size_t)A.dim.ld_b], zb = b[2 * (size_t)A.dim.ld_b];
                if (POSE) {
                    const double xr = (c * xb - s * yb) + ox, yr = (s * xb + c * yb) + oy;
                    xb = xr; yb = yr; zb = zb + oz;
                }
                const double dx = xa - xb, dy = ya - yb;
                const double d = __builtin_sqrt(dx * dx + dy * dy), dz = zb - za;
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
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long v[kTotals] = {n_eval, n_cpa, n_any, n_none, n_bad, w_eval, w_cpa, w_any};
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
hipError_t launch_miss_distance(const EmgpuMissRun &A, hipStream_t s, const char **name) {
    if (name) *name = A.pose ? "k_miss_distance[pose]" : "k_miss_distance";
    if (A.dim.n_pairs <= 0) return hipSuccess;
    const dim3 grid = pair_grid(A.dim.n_pairs, kBlock);   // the atomics of stage 3 are paid 2048 times at most
    if (A.pose) hipLaunchKernelGGL(k_miss_distance<true>, grid, dim3(kBlock), 0, s, A);
    else hipLaunchKernelGGL(k_miss_distance<false>, grid, dim3(kBlock), 0, s, A);
    return hipGetLastError();
}
} // namespace emgpu
