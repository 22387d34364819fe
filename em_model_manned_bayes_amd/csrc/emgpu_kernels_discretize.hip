// emgpu_kernels_discretize.hip -- k_discretize_dbn<float | double>: a device-resident trace of values into the trace of bins k_score_dbn and
// k_count_dbn read, one lane per trajectory, 256-lane workgroups.  The definition is in emgpu_discretize.h.
//
// Memory: per (group of four seconds, temporal-map row, lane) one 16-byte load of dyn_val (two for doubles) and one dword store of dyn_bin,
// both coalesced along the trajectory index; init_val / init_bin one element and one byte per (variable, lane).  Every variable's boundaries
// b[0..r] and fine steps h[d] = (b[d] - b[d-1]) / n_fine sit in LDS (2 * 16 * 65 doubles, filled once per workgroup from the plan's table):
// a cut point is read once per row at one address for the whole wave (a broadcast) and serves the row's four values.
// The coarse and the fine bin are sums of compares: no lane branches on its value, only on what the workgroup shares (the row's variable).
// repeat / change are integers, so the order of the adds does not matter; they are reduced in three stages:
//   1. u32 registers per lane and row, over the workgroup's tiles;
//   2. a shuffle reduction per wave, one LDS slot per (wave, row, kind);
//   3. one 64-bit vector atomic without return (global_atomic_add_x2, relaxed, agent scope) per (workgroup, row, kind).
// No u32 partial can wrap: T - 1 <= 65534 per trajectory and at most EMGPU_DISC_WG_TRAJ trajectories per workgroup (emgpu_discretize.h).
// A lane that met a bad value stores the constant 1 to *bad with a plain vector store.
// Compiler's figures (hipcc -O3, gfx950): <float> 112 VGPRs, <double> 116 VGPRs, 16 768 bytes of LDS, no scratch.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "emgpu_discretize.h"

namespace {
constexpr int kBlock = 256, kWaves = kBlock / 64;

__device__ __forceinline__ void load4(const float *p, double x[4]) {
    const float4 v = *reinterpret_cast<const float4 *>(p);
    x[0] = (double)v.x; x[1] = (double)v.y; x[2] = (double)v.z; x[3] = (double)v.w;
}
__device__ __forceinline__ void load4(const double *p, double x[4]) {
    const double2 a = *reinterpret_cast<const double2 *>(p), b = *reinterpret_cast<const double2 *>(p + 2);
    x[0] = a.x; x[1] = a.y; x[2] = b.x; x[3] = b.y;
}

// W values of one variable: d (0 for a bad value) and, for n_fine > 0 and a variable with boundaries, f
template <int W>
__device__ __forceinline__ void bins(const double *x, const double *cut, const double *step, uint32_t r, bool cont, bool wrap, int n_fine,
                                     uint32_t *d, uint32_t *f) {
    if (!cont) {   // categorical: the value is the bin
#pragma unroll
        for (int s = 0; s < W; s++) {
            const bool good = x[s] >= 1.0 && x[s] <= (double)r && x[s] == __builtin_floor(x[s]);
            d[s] = (uint32_t)(good ? x[s] : 0.0);
            f[s] = 0u;
        }
        return;
    }
#pragma unroll
    for (int s = 0; s < W; s++) d[s] = 1u;
    for (uint32_t q = 1; q < r; q++) {
        const double c = cut[q];
#pragma unroll
        for (int s = 0; s < W; s++) d[s] += x[s] >= c ? 1u : 0u;
    }
    double a[W], h[W];
#pragma unroll
    for (int s = 0; s < W; s++) {
        if (wrap) d[s] = d[s] == r ? 1u : d[s];   // 1 + mod(d - 1, r - 1) for d in 1..r
        f[s] = 1u;
        a[s] = cut[d[s] - 1u];
        h[s] = step[d[s] - 1u];
    }
    for (int k = 1; k < n_fine; k++) {
        const double kk = (double)k;
#pragma unroll
        for (int s = 0; s < W; s++) f[s] += x[s] >= a[s] + kk * h[s] ? 1u : 0u;
    }
#pragma unroll
    for (int s = 0; s < W; s++) d[s] = x[s] != x[s] ? 0u : d[s];   // NaN
}

template <typename V>
__global__ __launch_bounds__(kBlock) void k_discretize_dbn(const EmgpuDiscretizeRun A) {
    __shared__ double cut[EMGPU_MAX_NI][EMGPU_DISC_NB];
    __shared__ double step[EMGPU_MAX_NI][EMGPU_DISC_NB];
    __shared__ uint32_t part[kWaves][2 * EMGPU_MAX_ND];
    const double nf = (double)(A.n_fine > 0 ? A.n_fine : 1);
    for (int e = threadIdx.x; e < EMGPU_MAX_NI * EMGPU_DISC_NB; e += kBlock) {
        const int v = e / EMGPU_DISC_NB, j = e % EMGPU_DISC_NB;
        double b = 0.0, h = 0.0;
        if (v < A.ni && A.v_cont[v] && j <= (int)A.v_r[v]) {
            b = A.bnd[(int)A.v_boff[v] + j];
            if (j < (int)A.v_r[v]) h = (A.bnd[(int)A.v_boff[v] + j + 1] - b) / nf;
        }
        cut[v][j] = b; step[v][j] = h;
    }
    __syncthreads();
    const bool pairs = A.n_fine > 0 && A.repeat && A.change;
    const int G4 = (A.T + 3) >> 2;
    uint32_t rep[EMGPU_MAX_ND], chg[EMGPU_MAX_ND];
#pragma unroll
    for (int k = 0; k < EMGPU_MAX_ND; k++) rep[k] = chg[k] = 0u;
    bool bad = false;
    // tile j of this workgroup: trajectories (blockIdx.x + j * gridDim.x) * 256 ...; at most EMGPU_DISC_WG_TRAJ / 256 tiles (the launcher)
    for (int64_t tile = blockIdx.x; tile * kBlock < A.n; tile += gridDim.x) {
        const int64_t i = tile * kBlock + threadIdx.x;
        if (i >= A.n) continue;
        if (A.init_val) {
            const V *iv = (const V *)A.init_val + (size_t)i;
            for (int v = 0; v < A.ni; v++) {
                const double x = (double)iv[(size_t)v * (size_t)A.ld];
                uint32_t d, f;
                bins<1>(&x, cut[v], step[v], A.v_r[v], A.v_cont[v] != 0, (A.wrap_mask >> v) & 1u, 0, &d, &f);
                bad = bad || d == 0u;
                A.init_bin[(size_t)v * (size_t)A.ld + (size_t)i] = (uint8_t)d;
            }
        }
        if (!A.dyn_val) continue;
        uint32_t pd[EMGPU_MAX_ND], pf[EMGPU_MAX_ND];   // the previous column's d (0: none, or bad) and f
#pragma unroll
        for (int k = 0; k < EMGPU_MAX_ND; k++) pd[k] = pf[k] = 0u;
        const V *dv = (const V *)A.dyn_val + 4 * (size_t)i;
        for (int g = 0; g < G4; g++) {
#pragma unroll
            for (int k = 0; k < EMGPU_MAX_ND; k++) {
                if (k >= A.nd) continue;
                const size_t row = (size_t)g * (size_t)A.nd + (size_t)k;
                const int v = A.d_var[k];
                const bool cont = A.v_cont[v] != 0;
                double x[4];
                uint32_t d[4], f[4];
                load4(dv + 4 * row * (size_t)A.ld, x);
                bins<4>(x, cut[v], step[v], A.v_r[v], cont, (A.wrap_mask >> v) & 1u, A.n_fine, d, f);
                const uint32_t zero = A.v_zero[v];
                uint32_t word = 0u;
#pragma unroll
                for (int s = 0; s < 4; s++) {
                    const bool live = 4 * g + s < A.T;      // columns >= T are the last word's padding: written 0, never reported
                    const uint32_t ds = live ? d[s] : 0u;
                    bad = bad || (live && ds == 0u);
                    word |= ds << (8 * s);
                    // (pd is 0 before column 0 and after a bad value, and ds is 0 for a bad or padding value: no such pair passes)
                    const bool pair = pairs && cont && ds != 0u && ds == pd[k] && ds != zero;
                    rep[k] += pair && f[s] == pf[k] ? 1u : 0u;
                    chg[k] += pair && f[s] != pf[k] ? 1u : 0u;
                    pd[k] = ds; pf[k] = f[s];
                }
                A.dyn_bin[row * (size_t)A.ld + (size_t)i] = word;
            }
        }
    }
    if (bad) *A.bad = 1u;
    if (!pairs || !A.dyn_val) return;   // (uniform: every lane of the workgroup returns or none)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < EMGPU_MAX_ND; k++) {
        uint32_t a = rep[k], b = chg[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); b += __shfl_xor(b, o, 64); }
        if (lane == 0) { part[wave][2 * k] = a; part[wave][2 * k + 1] = b; }
    }
    __syncthreads();
    if (threadIdx.x < 2 * A.nd) {
        uint32_t x = 0u;
#pragma unroll
        for (int w = 0; w < kWaves; w++) x += part[w][threadIdx.x];
        unsigned long long *dst = (threadIdx.x & 1 ? A.change : A.repeat) + A.d_var[threadIdx.x >> 1];
        if (x) (void)__hip_atomic_fetch_add(dst, (unsigned long long)x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
} // namespace

namespace emgpu {
hipError_t launch_discretize_dbn(const EmgpuDiscretizeRun &A, bool f64, hipStream_t s, const char **name) {
    if (name) *name = f64 ? "k_discretize_dbn[f64]" : "k_discretize_dbn[f32]";
    if (A.n <= 0 || (!A.init_val && !A.dyn_val)) return hipSuccess;
    // enough workgroups to fill the chip, few enough that the atomics of stage 3 are paid 2048 times at most; and never more than
    // EMGPU_DISC_WG_TRAJ trajectories per workgroup (the bound on a u32 partial)
    const int64_t tiles = (A.n + kBlock - 1) / kBlock, per_wg = EMGPU_DISC_WG_TRAJ / kBlock;
    const int64_t blocks = std::max<int64_t>(std::min<int64_t>(tiles, 2048), (tiles + per_wg - 1) / per_wg);
    const dim3 grid((unsigned)blocks);
    if (f64) hipLaunchKernelGGL(k_discretize_dbn<double>, grid, dim3(kBlock), 0, s, A);
    else hipLaunchKernelGGL(k_discretize_dbn<float>, grid, dim3(kBlock), 0, s, A);
    return hipGetLastError();
}
} // namespace emgpu
