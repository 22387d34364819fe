// emgpu_score.h -- the argument block and the launcher of k_score_dbn (emgpu_kernels_score.hip): the log-likelihood of a trace under a model.
// Built on the host by emgpu_score.cpp from the model's plan and its two log tables (emgpu::initial_log_prob, emgpu::transition_log_prob).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/emgpu.h"
#include "emgpu_plan.h"

// The definition (DESIGN.md "Scoring a trace"): acc starts at +0.0 and receives one IEEE double addition per node, in this order:
//   1. the initial nodes by topological position p: the entry at the node's bin in the column its parents' bins select;
//   2. for t = 1 .. T-1, and within t for the temporal-map rows k = 0 .. nd-1: the entry of row k's (t+1) node at its bin in column t.
// Parent bins, per step (dbn_sample.m:65-93): a static parent's bin in init_bin, a time-t node's bin in column t-1, a (t+1) node's bin in
// column t.  Frozen (dbn_sample.m:97-135): the column number is computed once, from init_bin and column 0.
// Every bin read (init_bin, columns 0 .. T-1 of dyn_bin) outside 1..r makes the trajectory's log_lik NaN and sets *bad; the index is clamped
// into the table before the load.  `initial` (acc after step 1) is NaN when a bin of init_bin is outside 1..r.
// NOT part of the number: the normalisation by the rejection loop of UncorEncounterModel.sample (altitude / speed / layers).
struct EmgpuScoreRun {
    int64_t n;
    int64_t ld;                 // trajectory dimension of init_bin / dyn_bin
    int32_t T, ni, nd, _pad;
    const uint8_t *init_bin;    // [ni][ld] by variable id, already at the call's first column
    const uint32_t *dyn_bin;    // [ceil(T/4)][nd][ld], byte c % 4 of word c / 4 = column c; null: no transitions are scored
    double *log_lik;            // [n]
    double *initial;            // [n] or null
    uint32_t *bad;              // device word: a lane that met a bin outside 1..r stores 1
    const double *logp_i;       // initial_log_prob
    const double *logp_t;       // transition_log_prob
    // ---- initial network by topological position (EmgpuPlan's numbering)
    uint8_t i_var[EMGPU_MAX_NI], i_r[EMGPU_MAX_NI];
    uint32_t i_off[EMGPU_MAX_NI];
    uint32_t i_stride[EMGPU_MAX_NI][EMGPU_MAX_NI];   // [p][q < p]
    // ---- transition network by temporal-map row k
    uint8_t d_r[EMGPU_MAX_ND];
    uint32_t d_off[EMGPU_MAX_ND];
    uint32_t d_static[EMGPU_MAX_ND][EMGPU_MAX_NI];   // static parents, by topological position
    uint32_t d_cur[EMGPU_MAX_ND][EMGPU_MAX_ND];      // the time-t node of row k'
    uint32_t d_new[EMGPU_MAX_ND][EMGPU_MAX_ND];      // the (t+1) node of row k'
};

struct emgpu_model;
namespace emgpu {
// What can be said about a trace call (emgpu_score_dbn_*, emgpu_count_dbn_*) without a device: EMGPU_OK, or the error (recorded).  `have_out`:
// the call's required output is there (`outputs` names it in the message); `transitions`: the call reads dyn_bin when the trace has any.
int check_trace_args(const emgpu_model *h, const emgpu_score_params *p, const void *init_bin, const void *dyn_bin, bool have_out,
                     const char *outputs, bool transitions);
// The graph part of the argument block from the model's plan -- topological positions, strides by temporal-map row, padding positions and
// rows -- with i_off / d_off [by temporal-map row] as the caller's tables are laid out; the buffers stay null.  The one owner of this
// derivation: k_score_dbn and k_count_dbn (emgpu_count.h) index with it.  Returns whether the parents are read per step (dbn_sample.m:55).
bool fill_trace_graph(const EmgpuPlan &P, const emgpu_score_params *p, const uint32_t *i_off, const uint32_t *d_off, EmgpuScoreRun &A);
hipError_t launch_score_dbn(const EmgpuScoreRun &A, bool per_step, hipStream_t s, const char **name);
}
