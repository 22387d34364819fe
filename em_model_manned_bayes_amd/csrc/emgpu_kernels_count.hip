// emgpu_kernels_count.hip -- k_count_dbn: the sufficient statistics of a device-resident trace, one lane per trajectory, unweighted (every
// observation adds 1) or WEIGHTED (every observation of trajectory i adds weights[i]).  The definition is in emgpu_count.h.  Counts are
// integers: the result does not depend on the order of the adds, whatever the scheme below does.
//
// Memory: the bins are read as k_score_dbn reads them (ni bytes of init_bin, one u32 = four seconds per dynamic variable and group, coalesced
// along the trajectory index); a weighted lane reads its weight first, and a lane of weight 0 reads no bin, does no add and sets no report.
// What is new is the adds, reduced twice before they reach global memory:
//   1. RUN LENGTH, per lane and temporal-map row: the lane keeps (cell, pending count) and flushes only when the next second's cell differs,
//      and once at its end.  Frozen: the column never changes, so a flush follows a change of the variable's own bin; per step: an event of
//      the variable or of a parent.  nd * (T-1) adds per trajectory become about nd * (events + 1).  The pending count is a u32 count of
//      seconds in both forms; the flush adds count * weight (weighted: a 64-bit product, < 2^16 * 2^32).
//   2. LDS PARTIALS, per workgroup, for the tables small enough to share the partials' cells (EMGPU_COUNT_LDS_CELLS u32, or
//      EMGPU_WCOUNT_LDS_CELLS u64 when weighted: the same bytes; the host assigns them, smallest first: the initial network's roots and
//      low-arity nodes, which every lane of the grid hits, and small transition tables): ds_add_u32 / ds_add_u64 without return, and ONE
//      global add per touched cell when the workgroup ends.  A workgroup takes at most EMGPU_COUNT_WG_TRAJ trajectories (the launcher's
//      grid), which is what keeps a partial of either width from wrapping (emgpu_count.h).
// Tables too large for the partials (the headline model's transition tables: 74 480 cells) take their run-length flushes as global adds:
// their column is a function of many parent bins, so the lanes of a wave spread over the table instead of meeting in one cell.
// Global adds are 64-bit vector atomics without return (global_atomic_add_x2), relaxed, agent scope.  A lane that skipped an observation
// stores the constant 1 to *bad with a plain vector store.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "emgpu_count.h"

namespace {
constexpr int kBlock = 256;
typedef unsigned long long u64;

__device__ __forceinline__ void add_global(u64 *p, u64 x) {
    (void)__hip_atomic_fetch_add(p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

#ifdef EMGPU_COUNT_NAIVE   // tools/count_time.py --naive builds this variant for the record in HISTORY.md: one global add per observation
constexpr bool kNaive = true;
#else
constexpr bool kNaive = false;
#endif

// `x` (observations, times the weight) into cell `cell` (an index into the network's counts array) of a node whose first cell is `off`
template <typename P> __device__ __forceinline__ void add_cell(u64 *counts, P *part, uint32_t lds, uint32_t off, uint32_t cell, P x) {
    if (!kNaive && lds != EMGPU_COUNT_NO_LDS) (void)__hip_atomic_fetch_add(&part[lds + (cell - off)], x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else add_global(counts + cell, x);
}

// `weights`: [n], one per trajectory of the window (not offset by col_offset); read only when WEIGHTED
template <bool PER_STEP, bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void k_count_dbn(const EmgpuCountRun A, const uint32_t *weights) {
    typedef std::conditional_t<WEIGHTED, u64, uint32_t> P;   // a partial, a weight, a flush
    __shared__ P part[WEIGHTED ? EMGPU_WCOUNT_LDS_CELLS : EMGPU_COUNT_LDS_CELLS];
    const EmgpuScoreRun &G = A.G;
    for (uint32_t c = threadIdx.x; c < A.lds_used; c += kBlock) part[c] = 0;
    __syncthreads();
    const bool want_t = A.counts_t && G.dyn_bin && G.nd > 0 && G.T > 1;
    bool skipped = false;
    // tile j of this workgroup: trajectories (blockIdx.x + j * gridDim.x) * 256 ...; at most EMGPU_COUNT_WG_TRAJ / 256 tiles (launch_count_dbn)
    for (int64_t tile = blockIdx.x; tile * kBlock < G.n; tile += gridDim.x) {
        const int64_t i = tile * kBlock + threadIdx.x;
        if (i >= G.n) continue;
        P wt = 1;
        if constexpr (WEIGHTED) {
            wt = weights[(size_t)i];
            if (wt == 0) continue;    // left out: whatever its bins hold, nothing is added and nothing reported
        }
        uint32_t bin[EMGPU_MAX_NI];   // 0-based, clamped into 0 .. r-1, by topological position
        uint32_t ibad = 0u;           // bit p: the bin at position p is outside 1..r
#pragma unroll
        for (int p = 0; p < EMGPU_MAX_NI; p++) {   // positions >= ni are padding: node 0 again, zero strides (emgpu_score.cpp)
            const uint32_t r = G.i_r[p];
            uint32_t z = (uint32_t)G.init_bin[(size_t)G.i_var[p] * (size_t)G.ld + (size_t)i] - 1u;
            ibad |= (z >= r && p < G.ni) ? 1u << p : 0u;
            z = z >= r ? 0u : z;
            bin[p] = z;
            uint32_t col = 0u;
#pragma unroll
            for (int q = 0; q < p; q++) col += G.i_stride[p][q] * bin[q];
            if (A.counts_i && p < G.ni) {
                if (ibad & A.i_mask[p]) skipped = true;
                else add_cell(A.counts_i, part, A.i_lds[p], G.i_off[p], G.i_off[p] + col * r + z, wt);
            }
        }
        if (!want_t) continue;

        uint32_t base[EMGPU_MAX_ND], prev[EMGPU_MAX_ND], cur[EMGPU_MAX_ND], w[EMGPU_MAX_ND];
        uint32_t pend_cell[EMGPU_MAX_ND], pend[EMGPU_MAX_ND];   // the run: `pend` observations of pend_cell, not yet added
        uint32_t fixed_bad = 0u;      // bit k: a bin row k reads for every second (static parents; frozen: column 0) is bad
        uint32_t prev_bad = 0u;       // bit k: row k's bin in the previous column is bad
        const uint32_t *col_i = G.dyn_bin + (size_t)i;
#pragma unroll
        for (int k = 0; k < EMGPU_MAX_ND; k++) {
            base[k] = 0u;
#pragma unroll
            for (int p = 0; p < EMGPU_MAX_NI; p++) base[k] += G.d_static[k][p] * bin[p];
            const uint32_t z = (col_i[(size_t)(k < G.nd ? k : 0) * (size_t)G.ld] & 0xFFu) - 1u;   // column 0
            prev_bad |= (z >= (uint32_t)G.d_r[k] && k < G.nd) ? 1u << k : 0u;
            prev[k] = z >= (uint32_t)G.d_r[k] ? 0u : z;
            pend_cell[k] = 0u; pend[k] = 0u;
        }
#pragma unroll
        for (int k = 0; k < EMGPU_MAX_ND; k++) {
            if (ibad & A.d_smask[k]) fixed_bad |= 1u << k;
            if constexpr (!PER_STEP) {   // frozen: one column for every second, from init_bin and column 0
                if (prev_bad & A.d_cmask[k]) fixed_bad |= 1u << k;
#pragma unroll
                for (int kp = 0; kp < EMGPU_MAX_ND; kp++) base[k] += G.d_cur[k][kp] * prev[kp];
            }
        }
        const int G4 = (G.T + 3) >> 2;
        for (int g = 0; g < G4; g++) {
#pragma unroll
            for (int k = 0; k < EMGPU_MAX_ND; k++) w[k] = col_i[((size_t)g * (size_t)G.nd + (size_t)(k < G.nd ? k : 0)) * (size_t)G.ld];
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const int c = 4 * g + s;
                uint32_t cur_bad = 0u;
#pragma unroll
                for (int k = 0; k < EMGPU_MAX_ND; k++) {
                    const uint32_t z = ((w[k] >> (8 * s)) & 0xFFu) - 1u, r = G.d_r[k];
                    cur_bad |= (z >= r && k < G.nd) ? 1u << k : 0u;
                    cur[k] = z >= r ? 0u : z;
                }
                const bool live = c > 0 && c < G.T;   // column 0 has no transition into it; columns >= T are the last word's padding
#pragma unroll
                for (int k = 0; k < EMGPU_MAX_ND; k++) {
                    uint32_t col = base[k];
                    bool skip = ((fixed_bad >> k) & 1u) != 0u;
                    if constexpr (PER_STEP) {
#pragma unroll
                        for (int kp = 0; kp < EMGPU_MAX_ND; kp++) col += G.d_cur[k][kp] * prev[kp] + G.d_new[k][kp] * cur[kp];
                        skip = skip || (prev_bad & A.d_cmask[k]) || (cur_bad & A.d_nmask[k]);
                    } else {
                        skip = skip || ((cur_bad >> k) & 1u);
                    }
                    if (k < G.nd && live) {
                        const uint32_t cell = G.d_off[k] + col * (uint32_t)G.d_r[k] + cur[k];
                        if (skip) {
                            skipped = true;
                        } else if (!kNaive && pend[k] != 0u && cell == pend_cell[k]) {
                            pend[k]++;
                        } else {
                            if (pend[k] != 0u) add_cell(A.counts_t, part, A.d_lds[k], G.d_off[k], pend_cell[k], (P)pend[k] * wt);
                            pend_cell[k] = cell; pend[k] = 1u;
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < EMGPU_MAX_ND; k++) prev[k] = cur[k];
                prev_bad = cur_bad;
            }
        }
#pragma unroll
        for (int k = 0; k < EMGPU_MAX_ND; k++)
            if (k < G.nd && pend[k] != 0u) add_cell(A.counts_t, part, A.d_lds[k], G.d_off[k], pend_cell[k], (P)pend[k] * wt);
    }
    if (skipped) *G.bad = 1u;
    if (kNaive) return;
    // the workgroup's partials: one global add per touched cell
    __syncthreads();
    for (int p = 0; p < G.ni; p++) {
        if (!A.counts_i || A.i_lds[p] == EMGPU_COUNT_NO_LDS) continue;
        for (uint32_t c = threadIdx.x; c < A.i_cells[p]; c += kBlock) {
            const P x = part[A.i_lds[p] + c];
            if (x) add_global(A.counts_i + G.i_off[p] + c, x);
        }
    }
    for (int k = 0; k < G.nd; k++) {
        if (!want_t || A.d_lds[k] == EMGPU_COUNT_NO_LDS) continue;
        for (uint32_t c = threadIdx.x; c < A.d_cells[k]; c += kBlock) {
            const P x = part[A.d_lds[k] + c];
            if (x) add_global(A.counts_t + G.d_off[k] + c, x);
        }
    }
}
} // namespace

namespace emgpu {
hipError_t launch_count_dbn(const EmgpuCountRun &A, const uint32_t *weights, bool per_step, hipStream_t s, const char **name) {
    const bool weighted = weights != nullptr;
    if (name) *name = weighted ? (per_step ? "k_count_dbn[per-step,weighted]" : "k_count_dbn[frozen,weighted]")
                               : (per_step ? "k_count_dbn[per-step]" : "k_count_dbn[frozen]");
    if (A.G.n <= 0 || (!A.counts_i && !A.counts_t)) return hipSuccess;
    if (A.lds_used > (uint32_t)(weighted ? EMGPU_WCOUNT_LDS_CELLS : EMGPU_COUNT_LDS_CELLS)) return hipErrorInvalidValue;
    // enough workgroups to fill the chip, few enough that the flush of the partials is paid 2048 times at most; and never more than
    // EMGPU_COUNT_WG_TRAJ trajectories per workgroup (the bound on a partial)
    const int64_t tiles = (A.G.n + kBlock - 1) / kBlock, per_wg = EMGPU_COUNT_WG_TRAJ / kBlock;
    const int64_t blocks = std::max<int64_t>(std::min<int64_t>(tiles, 2048), (tiles + per_wg - 1) / per_wg);
    const auto k = weighted ? (per_step ? k_count_dbn<true, true> : k_count_dbn<false, true>)
                            : (per_step ? k_count_dbn<true, false> : k_count_dbn<false, false>);
    hipLaunchKernelGGL(k, dim3((unsigned)blocks), dim3(kBlock), 0, s, A, weights);
    return hipGetLastError();
}
} // namespace emgpu
