// emgpu_count.h -- the argument block and the launcher of k_count_dbn (emgpu_kernels_count.hip): the sufficient statistics of a trace, i.e.
// how often every cell of the model's N_initial / N_transition tables was observed.  Built on the host by emgpu_count.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "emgpu_score.h"

// The definition (DESIGN.md "Counting a trace"; include/emgpu.h).  An OBSERVATION is
//   (a) an initial node v of a trajectory: cell (bin of v, column its parents' bins select) of N_initial{v};
//   (b) for t = 1 .. T-1 and every temporal-map row k, the (t+1) node of row k at column t: a cell of that node's N_transition, parent bins
//       read exactly as k_score_dbn reads them (emgpu_score.h): per step, or frozen at column 0.
// Every observation adds exactly 1 to its cell, or, in a WEIGHTED count, the u32 weights[i] of its trajectory i: an exact u64
// addition.  An observation whose own bin, or any parent bin it reads, is outside 1..r is SKIPPED (it adds nothing and sets *bad); every other
// observation of the trajectory still counts.  A trajectory of weight 0 is left out before anything is looked at: it reads nothing, adds
// nothing and reports nothing, whatever its bins hold.
//
// The graph part G is the block k_score_dbn takes (filled by emgpu::fill_trace_graph, the one owner of that derivation); here G.i_off / G.d_off
// are the nodes' first cells in counts_i / counts_t (emgpu_count_layout) and G.log_lik / initial / logp_* are unused (null).
// The workgroup's LDS partials (32 KB: five workgroups of 256 per CU): u32 cells, or u64 cells in a weighted count, so the same bytes hold
// half the cells; i_lds / d_lds / lds_used are assigned under the cap of the call's form (fill_count).
#define EMGPU_COUNT_LDS_CELLS 8192
#ifndef EMGPU_WCOUNT_LDS_CELLS
#define EMGPU_WCOUNT_LDS_CELLS 4096   // tools/count_time.py --weighted --lds 8192 times the -DEMGPU_WCOUNT_LDS_CELLS=8192 variant against it
#endif
#define EMGPU_COUNT_NO_LDS 0xFFFFFFFFu
// Why neither partial can wrap: a workgroup feeds at most EMGPU_COUNT_WG_TRAJ trajectories into its partials before it flushes them, and a
// trajectory adds at most max(1, T-1) <= 65534 (sample_time <= 65535) observations to one cell.  u32: 65536 * 65534 = 4 294 836 224 < 2^32.
// u64: 65536 * 65534 * (2^32 - 1) < 2^64.  Nor can a cell of the caller's tables within one weighted call: the entry points refuse more than
// n * max(1, T-1) = 2^32 observations per cell, and 2^32 * (2^32 - 1) < 2^64.
#define EMGPU_COUNT_WG_TRAJ 65536
struct EmgpuCountRun {
    EmgpuScoreRun G;
    unsigned long long *counts_i;    // null: the initial network is not counted
    unsigned long long *counts_t;    // null: the transition network is not counted
    // a node's cells in the workgroup's LDS partials (EMGPU_COUNT_NO_LDS: the table is too large, its adds go to global memory), and its size
    uint32_t i_lds[EMGPU_MAX_NI], i_cells[EMGPU_MAX_NI];   // by topological position
    uint32_t d_lds[EMGPU_MAX_ND], d_cells[EMGPU_MAX_ND];   // by temporal-map row
    uint32_t lds_used;                                     // cells of the partials in use (<= the form's cap)
    // whose bins an observation reads, as bit masks: a set bit that meets a bad bin skips the observation
    uint32_t i_mask[EMGPU_MAX_NI];   // positions q <= p: the node itself and its parents
    uint32_t d_smask[EMGPU_MAX_ND];  // positions of row k's static parents
    uint32_t d_cmask[EMGPU_MAX_ND];  // rows whose time-t node is a parent of row k
    uint32_t d_nmask[EMGPU_MAX_ND];  // rows whose (t+1) node is a parent of row k, and k itself
};

namespace emgpu {
// weights: null for the unweighted instances; else [n], one per trajectory of the window (not offset by col_offset).  Sets *name to the
// instance it chose (also when there is nothing to launch); hipErrorInvalidValue when lds_used exceeds the form's cap.
hipError_t launch_count_dbn(const EmgpuCountRun &A, const uint32_t *weights, bool per_step, hipStream_t s, const char **name);
}
