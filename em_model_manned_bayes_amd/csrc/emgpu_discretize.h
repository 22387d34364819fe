// emgpu_discretize.h -- the argument block and the launcher of k_discretize_dbn (emgpu_kernels_discretize.hip): a trace of VALUES into the
// trace of BINS that k_score_dbn and k_count_dbn read, and the repeat / change counts behind a model's resample rates.  Built on the host by
// emgpu_discretize.cpp from the model's plan (the boundaries are the plan's own device table).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/emgpu.h"
#include "emgpu_plan.h"

// The definition (DESIGN.md "Discretizing a trace"; include/emgpu.h).  For one value x, promoted exactly to f64, of variable v with r bins
// and boundaries b[0..r]:
//   coarse  d = 1 + #{q in 1..r-1 : x >= b[q]}                                   discretize_bayes.m:14-22
//   wrap    where bit v of wrap_mask is set: d = 1 + mod(d - 1, r - 1)            hierarchical_discretize.m:29  (d == r becomes 1)
//   fine    a = b[d-1], h = (b[d] - a) / n_fine, f = 1 + #{k in 1..n_fine-1 : x >= a + k * h}     hierarchical_cutpoints.m:14,
//           hierarchical_discretize.m:37-41; one f64 multiply and one f64 add per cut, not contracted
//   a variable without boundaries ('*') is categorical: d = x when x is an integer in 1..r; it is never wrapped and has no fine bin
//   BAD: NaN, or a categorical value that is no integer in 1..r: the bin written is 0, *bad is set, and no pair holds the value
//   pairs   temporal-map row k of variable v, columns c = 1..T-1: both values good, d[c] == d[c-1], d[c] not v's zero bin:
//           repeat[v] += 1 when f[c] == f[c-1], else change[v] += 1               hierarchical_discretize.m:43-49
// The compiled caps are those of every model the library loads: EMGPU_MAX_NI variables of at most EMGPU_MAX_R bins (emgpu_plan.h;
// compile_plan refuses larger models with EMGPU_ERR_UNSUPPORTED), so the workgroup's two LDS tables below always fit.
//
// Why no u32 partial of repeat / change can wrap: a trajectory adds at most T - 1 <= 65534 (sample_time <= 65535) to one (row, kind), and a
// workgroup takes at most EMGPU_DISC_WG_TRAJ = 65536 trajectories (the launcher's grid): a lane's register holds at most 256 tiles * 65534,
// a wave's sum 64 times that, the workgroup's sum 65536 * 65534 = 4 294 836 224 < 2^32.
#define EMGPU_DISC_WG_TRAJ 65536
#define EMGPU_DISC_NB (EMGPU_MAX_R + 1)   // boundaries of one variable in the LDS table
struct EmgpuDiscretizeRun {
    int64_t n;
    int64_t ld;                  // trajectory dimension of all four arrays
    int32_t T, ni, nd, n_fine;   // n_fine 0: bins only
    uint32_t wrap_mask, _pad;
    const void *init_val;        // V [ni][ld] by variable id, already at the call's first column; null with init_bin: no initial half
    const void *dyn_val;         // V [ceil(T/4)][nd][ld][4]; null with dyn_bin: no dynamic half
    uint8_t *init_bin;           // [ni][ld]
    uint32_t *dyn_bin;           // [ceil(T/4)][nd][ld], byte c % 4 of word c / 4 = column c; the last word's padding bytes are written 0
    unsigned long long *repeat;  // [ni] by variable id, added to; null with n_fine 0
    unsigned long long *change;
    uint32_t *bad;               // device word: a lane that met a bad value stores 1
    const double *bnd;           // the plan's boundary table
    // ---- by variable id
    uint8_t v_r[EMGPU_MAX_NI];       // bins
    uint8_t v_cont[EMGPU_MAX_NI];    // 1: has boundaries b[0..r] at bnd[v_boff]; 0: categorical
    uint8_t v_zero[EMGPU_MAX_NI];    // zero bin (0 = none)
    uint16_t v_boff[EMGPU_MAX_NI];
    uint8_t d_var[EMGPU_MAX_ND];     // the variable id of temporal-map row k
};

namespace emgpu {
// f64: the values are doubles (EMGPU_VALUE_F64), else floats
hipError_t launch_discretize_dbn(const EmgpuDiscretizeRun &A, bool f64, hipStream_t s, const char **name);
}
