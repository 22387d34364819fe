// emgpu_debug.cpp -- the emgpu_debug_* getters that need no device: what the plan compiler made of a model, read back by the tests; and
// emgpu_debug_device_math, which needs one and no context: a probe kernel over the track kernels' device math (emgpu_mathprobe.h).
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>

#include "emgpu_internal.hpp"
#include "emgpu_mathprobe.h"

// The model's plan for a getter of dynamic variable k, or null after fail(): k must be one (`padded`: one with a padded table; the getter
// says which in its own words, no_k), and col, where the getter has the helper check it, a column of its transition table.
static std::shared_ptr<const emgpu::CompiledPlan> dynamic_plan(const emgpu_model *m, int32_t k, const int64_t *col,
                                                               const char *no_k = "no such dynamic variable", bool padded = false) {
    std::shared_ptr<const emgpu::CompiledPlan> cp = emgpu::plan_of(m->m);
    const EmgpuPlan &P = cp->plan;
    if (k < 0 || k >= P.nd || (padded && P.d_pw[k] == 0)) { fail(EMGPU_ERR_ARG, no_k); return nullptr; }
    if (col && (*col < 0 || *col >= m->m.q_transition[P.d_tvar[k]])) { fail(EMGPU_ERR_ARG, "no such column"); return nullptr; }
    return cp;
}

extern "C" {

int emgpu_debug_column_thresholds(const double *weights, int32_t r, uint32_t *out) {
    if (!weights || !out || r < 1 || r > EMGPU_MAX_R) return fail(EMGPU_ERR_ARG, "bad arguments");
    if (r > 1) emgpu::column_thresholds(weights, r, out);
    return EMGPU_OK;
}

uint32_t emgpu_debug_bernoulli_threshold(double rate) { return emgpu::bernoulli_threshold(rate); }

int emgpu_debug_dynamic_column(const emgpu_model *m, int32_t k, int64_t col, int32_t *tvar, int32_t *r, int64_t *q,
                               uint32_t *thr, int32_t *meff, uint32_t *cthr, uint32_t *map) {
    EMGPU_TRY
    if (!m || !tvar || !r || !q || !thr || !meff || !cthr || !map) return fail(EMGPU_ERR_ARG, "null argument");
    const std::shared_ptr<const emgpu::CompiledPlan> cp_keep = dynamic_plan(m, k, nullptr);   // (the column: behind tvar, r and q, which a bad column still gets)
    if (!cp_keep) return EMGPU_ERR_ARG;
    const emgpu::CompiledPlan &cp = *cp_keep;
    const EmgpuPlan &P = cp.plan;
    *tvar = (int32_t)P.d_tvar[k] + 1;
    *r = (int32_t)P.d_r[k];
    *q = m->m.q_transition[P.d_tvar[k]];
    if (col < 0 || col >= *q) return fail(EMGPU_ERR_ARG, "no such column");
    const int rm1 = *r - 1;
    for (int t = 0; t < rm1 && t < 15; t++) thr[t] = cp.thr[P.d_off[k] + (size_t)col * rm1 + t];
    *meff = (int32_t)P.d_meff[k];
    *map = 0u;
    if (*meff > 0) {
        const uint32_t *c = cp.cthr.data() + P.d_coff[k] + (size_t)col * (*meff + 1);
        for (int t = 0; t < *meff; t++) cthr[t] = c[t];
        *map = c[*meff];
    }
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_debug_parent_masks(const emgpu_model *m, uint32_t *cur_mask, uint32_t *new_mask) {
    EMGPU_TRY
    if (!m || !cur_mask || !new_mask) return fail(EMGPU_ERR_ARG, "null argument");
    const std::shared_ptr<const emgpu::CompiledPlan> cp_keep = emgpu::plan_of(m->m); const emgpu::CompiledPlan &cp = *cp_keep;
    emgpu::step_parent_masks(cp.plan, cur_mask, new_mask);
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_debug_kernel_choice(const emgpu_model *m, const emgpu_sample_params *p, const emgpu_sample_out *out, char *name, int32_t cap) {
    EMGPU_TRY
    if (!m || !p || !out || !name) return fail(EMGPU_ERR_ARG, "null argument");
    const std::shared_ptr<const emgpu::CompiledPlan> cp_keep = emgpu::plan_of(m->m);
    EmgpuRun A;   // what choose_dbn reads of fill_run's and bind_outputs' run: which outputs are asked for, never where they are
    memset(&A, 0, sizeof A);
    A.n = p->n; A.per_step = p->transition_mode == EMGPU_TRANSITION_PER_STEP; A.flags = p->flags; A.event_cap = p->event_cap;
    A.indices = p->indices;
    A.dyn_bin = out->dyn_bin; A.dyn_val = out->dyn_val; A.ev_count = out->ev_count;
    A.events = reinterpret_cast<uint64_t *>(out->events);
    const emgpu::DbnChoice c = emgpu::choose_dbn(cp_keep->plan, A, p->start != nullptr || out->log_weight != nullptr);
    if (cap < 1 || strlen(c.name) >= (size_t)cap) return fail(EMGPU_ERR_ARG, "name does not fit cap");
    strcpy(name, c.name);
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_debug_padded_column(const emgpu_model *m, int32_t k, int64_t col, int32_t *width, uint32_t *words) {
    EMGPU_TRY
    if (!m || !width || !words) return fail(EMGPU_ERR_ARG, "null argument");
    const std::shared_ptr<const emgpu::CompiledPlan> cp_keep = dynamic_plan(m, k, &col);
    if (!cp_keep) return EMGPU_ERR_ARG;
    const emgpu::CompiledPlan &cp = *cp_keep;
    const EmgpuPlan &P = cp.plan;
    *width = (int32_t)P.d_pw[k];
    for (int t = 0; t < *width; t++) words[t] = cp.pthr[P.d_poff[k] + (size_t)col * (size_t)*width + t];
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_debug_pk_column(const emgpu_model *m, int32_t k, int64_t col, uint32_t *words) {
    EMGPU_TRY
    if (!m || !words) return fail(EMGPU_ERR_ARG, "null argument");
    const std::shared_ptr<const emgpu::CompiledPlan> cp_keep = dynamic_plan(m, k, &col, "no such padded dynamic variable", true);
    if (!cp_keep) return EMGPU_ERR_ARG;
    const emgpu::CompiledPlan &cp = *cp_keep;
    const EmgpuPlan &P = cp.plan;
    for (int t = 0; t < 4; t++) words[t] = cp.pthr[P.d_poffpk[k] + (size_t)col * 4 + t];
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_debug_device_math(void *hip_stream, int32_t fn, int64_t n, const double *x, double *out0, double *out1) {
    EMGPU_TRY
    if (fn < EMGPU_MATH_SINCOS_SMALL || fn > EMGPU_MATH_ROUND500) return fail(EMGPU_ERR_ARG, "no such function: fn outside 0..12");
    if (n < 0 || n > ((int64_t)1 << 32)) return fail(EMGPU_ERR_ARG, "n outside 0..2^32");
    if (!x) return fail(EMGPU_ERR_ARG, "null argument: x");
    if (!out0) return fail(EMGPU_ERR_ARG, "null argument: out0");
    if (((uintptr_t)x | (uintptr_t)out0 | (uintptr_t)out1) & 7u) return fail(EMGPU_ERR_ARG, "x, out0 and out1 must be 8-byte aligned");
    if (n == 0) return EMGPU_OK;
    launch_ok(emgpu::launch_math_probe(fn, n, x, out0, out1, (hipStream_t)hip_stream));
    return EMGPU_OK;
    EMGPU_CATCH
}

} // extern "C"
