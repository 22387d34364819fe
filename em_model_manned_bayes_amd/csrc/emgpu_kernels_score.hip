// emgpu_kernels_score.hip -- k_score_dbn: log P(trajectory | model) of every trajectory of a device-resident trace, one lane per trajectory.
// The sum and its order are defined in emgpu_score.h; every addition is a plain f64 add (the build has -ffp-contract=off).
//
// Memory: a lane reads its ni bytes of init_bin and one u32 (four seconds) per dynamic variable and group of dyn_bin, both coalesced along the
// trajectory index, and gathers one 8-byte table entry per node.  The tables (tens to a few hundred KB) stay in L2.  The gather form serves
// both transition modes: the frozen branch only computes its column numbers once per lane instead of once per second.
// No atomics, no shared state: lane i writes log_lik[i] / initial[i], and a lane that met a bin outside 1..r stores the constant 1 to *bad.
#include <hip/hip_runtime.h>

#include <cmath>

#include "emgpu_score.h"

namespace {
constexpr int kBlock = 256;

// Positions p >= ni and rows k >= nd are PADDING the host filled with node 0's / row 0's shape and zero strides (emgpu_score.cpp): their loads
// stay inside the trace and the tables, and a select keeps their entries out of the sum -- the body has no branch per node, so the bins stay
// scalars in registers.  The same select skips column 0 (no transition into it) and the padding columns >= T of the last packed word.
template <bool PER_STEP>
__global__ __launch_bounds__(kBlock) void k_score_dbn(const EmgpuScoreRun A) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= A.n) return;
    uint32_t bin[EMGPU_MAX_NI];   // 0-based, clamped into 0 .. r-1, by topological position
    bool bad = false;
    double acc = 0.0;
#pragma unroll
    for (int p = 0; p < EMGPU_MAX_NI; p++) {
        const uint32_t r = A.i_r[p];
        uint32_t z = (uint32_t)A.init_bin[(size_t)A.i_var[p] * (size_t)A.ld + (size_t)i] - 1u;
        bad |= z >= r;
        z = z >= r ? 0u : z;
        bin[p] = z;
        uint32_t col = 0u;
#pragma unroll
        for (int q = 0; q < p; q++) col += A.i_stride[p][q] * bin[q];
        const double x = A.logp_i[(size_t)A.i_off[p] + (size_t)(col * r + z)];
        acc = p < A.ni ? acc + x : acc;
    }
    const double nan = __builtin_nan("");
    if (A.initial) A.initial[i] = bad ? nan : acc;

    if (A.dyn_bin && A.nd > 0) {
        uint32_t base[EMGPU_MAX_ND], prev[EMGPU_MAX_ND], cur[EMGPU_MAX_ND], w[EMGPU_MAX_ND];
        const uint32_t *col_i = A.dyn_bin + (size_t)i;
#pragma unroll
        for (int k = 0; k < EMGPU_MAX_ND; k++) {
            base[k] = 0u;
#pragma unroll
            for (int p = 0; p < EMGPU_MAX_NI; p++) base[k] += A.d_static[k][p] * bin[p];
            const uint32_t z = (col_i[(size_t)(k < A.nd ? k : 0) * (size_t)A.ld] & 0xFFu) - 1u;   // column 0 (checked with its word below)
            prev[k] = z >= (uint32_t)A.d_r[k] ? 0u : z;
        }
        if constexpr (!PER_STEP) {   // frozen: one column for every second, from init_bin and column 0
#pragma unroll
            for (int k = 0; k < EMGPU_MAX_ND; k++)
#pragma unroll
                for (int kp = 0; kp < EMGPU_MAX_ND; kp++) base[k] += A.d_cur[k][kp] * prev[kp];
        }
        const int G4 = (A.T + 3) >> 2;
        for (int g = 0; g < G4; g++) {
#pragma unroll
            for (int k = 0; k < EMGPU_MAX_ND; k++) w[k] = col_i[((size_t)g * (size_t)A.nd + (size_t)(k < A.nd ? k : 0)) * (size_t)A.ld];
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const int c = 4 * g + s;
#pragma unroll
                for (int k = 0; k < EMGPU_MAX_ND; k++) {
                    const uint32_t z = ((w[k] >> (8 * s)) & 0xFFu) - 1u, r = A.d_r[k];
                    bad |= c < A.T && z >= r;
                    cur[k] = z >= r ? 0u : z;
                }
#pragma unroll
                for (int k = 0; k < EMGPU_MAX_ND; k++) {
                    uint32_t col = base[k];
                    if constexpr (PER_STEP) {
#pragma unroll
                        for (int kp = 0; kp < EMGPU_MAX_ND; kp++) col += A.d_cur[k][kp] * prev[kp] + A.d_new[k][kp] * cur[kp];
                    }
                    const double x = A.logp_t[(size_t)A.d_off[k] + (size_t)(col * (uint32_t)A.d_r[k] + cur[k])];
                    acc = (k < A.nd && c > 0 && c < A.T) ? acc + x : acc;
                }
#pragma unroll
                for (int k = 0; k < EMGPU_MAX_ND; k++) prev[k] = cur[k];
            }
        }
    }
    A.log_lik[i] = bad ? nan : acc;
    if (bad) *A.bad = 1u;
}
} // namespace

namespace emgpu {
hipError_t launch_score_dbn(const EmgpuScoreRun &A, bool per_step, hipStream_t s, const char **name) {
    if (name) *name = per_step ? "k_score_dbn[per-step]" : "k_score_dbn[frozen]";
    if (A.n <= 0) return hipSuccess;
    const dim3 grid((unsigned)((A.n + kBlock - 1) / kBlock));
    if (per_step) hipLaunchKernelGGL(k_score_dbn<true>, grid, dim3(kBlock), 0, s, A);
    else hipLaunchKernelGGL(k_score_dbn<false>, grid, dim3(kBlock), 0, s, A);
    return hipGetLastError();
}
} // namespace emgpu
