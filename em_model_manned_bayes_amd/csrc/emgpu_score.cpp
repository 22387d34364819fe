// emgpu_score.cpp -- emgpu_score_dbn_device / emgpu_score_dbn_host: the log-likelihood of a trace under a model (k_score_dbn,
// emgpu_kernels_score.hip; the definition is in emgpu_score.h and DESIGN.md).  The host entry point uploads, scores and downloads chunk by chunk
// (emgpu_tracechunk.hpp).
#include <cstring>
#include <string>

#include "emgpu_score.h"
#include "emgpu_tracechunk.hpp"

using namespace emgpu_detail;

namespace {
// both networks' log tables on the device, with the model version get_uploaded holds (it frees them when the model changes): the initial
// network's is the one the start grids' log-weights read (ensure_logp), the transition network's is uploaded here
void ensure_score_tables(emgpu_ctx *ctx, Uploaded &u, const Model &m) {
    ensure_logp(ctx, u, m);
    if (u.d_logpt) return;
    std::vector<double> lp;
    if (m.n_dyn() > 0) lp = emgpu::transition_log_prob(m, u.lpt_off);
    if (lp.size() > 0xFFFFFFF0ull) throw Error(EMGPU_ERR_UNSUPPORTED, "log table too large (the kernel indexes it with 32 bits)");
    HIP_OK(hipMalloc((void **)&u.d_logpt, (lp.size() + 1) * sizeof(double)));
    HIP_OK(hipMemcpyAsync(u.d_logpt, lp.data(), lp.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_OK(hipStreamSynchronize(ctx->stream));   // lp is a local
}

// the kernel's argument block but its buffers, the model's tables on the device
bool fill_score(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_score_params *p, EmgpuScoreRun &A) {
    Uploaded &u = get_uploaded(ctx, h);
    ensure_score_tables(ctx, u, h->m);
    const bool per_step = emgpu::fill_trace_graph(u.cp.plan, p, u.lp_off, u.lpt_off, A);
    A.logp_i = u.d_logp; A.logp_t = u.d_logpt;
    return per_step;
}

int check_args(const emgpu_model *h, const emgpu_score_params *p, const void *init_bin, const void *dyn_bin, const void *log_lik) {
    return emgpu::check_trace_args(h, p, init_bin, dyn_bin, log_lik != nullptr, "log_lik", true);
}

} // namespace

namespace emgpu {
int check_trace_args(const emgpu_model *h, const emgpu_score_params *p, const void *init_bin, const void *dyn_bin, bool have_out,
                     const char *outputs, bool transitions) {
    if (!h || !p) return fail(EMGPU_ERR_ARG, "null argument");
    if (p->n < 0 || p->sample_time < 1 || p->sample_time > 65535) return fail(EMGPU_ERR_ARG, "n < 0 or sample_time outside 1..65535");
    if (p->transition_mode != EMGPU_TRANSITION_REFERENCE_AUTO && p->transition_mode != EMGPU_TRANSITION_PER_STEP)
        return fail(EMGPU_ERR_ARG, "unknown transition_mode");
    const int64_t ld = p->ld ? p->ld : p->n;
    if (ld < 0 || p->col_offset < 0 || p->col_offset + p->n > ld) return fail(EMGPU_ERR_ARG, "col_offset + n exceeds ld");
    if (h->m.n_initial > EMGPU_MAX_NI || h->m.n_dyn() > EMGPU_MAX_ND) return fail(EMGPU_ERR_UNSUPPORTED, "more variables than EMGPU_MAX_NI / EMGPU_MAX_ND");
    if (p->n > 0 && (!init_bin || !have_out)) return fail(EMGPU_ERR_ARG, std::string("null init_bin or ") + outputs);
    if (p->n > 0 && !dyn_bin && transitions && p->sample_time > 1 && h->m.n_dyn() > 0)
        return fail(EMGPU_ERR_ARG, "null dyn_bin: only a call with sample_time 1, or a model without a transition network, has no transitions to score");
    return EMGPU_OK;
}

bool fill_trace_graph(const EmgpuPlan &P, const emgpu_score_params *p, const uint32_t *i_off, const uint32_t *d_off, EmgpuScoreRun &A) {
    memset(&A, 0, sizeof A);
    A.T = p->sample_time; A.ni = P.ni; A.nd = P.nd;
    memcpy(A.i_var, P.i_var, sizeof A.i_var);
    memcpy(A.i_r, P.i_r, sizeof A.i_r);
    memcpy(A.i_off, i_off, sizeof A.i_off);
    memcpy(A.i_stride, P.i_stride, sizeof A.i_stride);
    for (int k = 0; k < P.nd; k++) {   // the plan numbers the dynamic variables in sampling order, the trace and the sum by temporal-map row
        const int row = P.d_row[k];
        A.d_r[row] = P.d_r[k];
        A.d_off[row] = d_off[row];
        memcpy(A.d_static[row], P.d_stride_static[k], sizeof A.d_static[row]);
        for (int kp = 0; kp < P.nd; kp++) {
            A.d_cur[row][P.d_row[kp]] = P.d_stride_cur[k][kp];
            A.d_new[row][P.d_row[kp]] = P.d_stride_new[k][kp];
        }
    }
    // padding: positions >= ni and rows >= nd repeat node 0 / row 0 with zero strides (the kernels load them and keep them out of the result)
    for (int q = P.ni; q < EMGPU_MAX_NI; q++) {
        A.i_var[q] = A.i_var[0]; A.i_r[q] = A.i_r[0]; A.i_off[q] = A.i_off[0];
        memset(A.i_stride[q], 0, sizeof A.i_stride[q]);
    }
    for (int k = P.nd; k < EMGPU_MAX_ND && P.nd > 0; k++) { A.d_r[k] = A.d_r[0]; A.d_off[k] = A.d_off[0]; }
    return p->transition_mode == EMGPU_TRANSITION_PER_STEP || P.depend != 0;   // dbn_sample.m:55
}
} // namespace emgpu

extern "C" {

int emgpu_score_dbn_device(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_score_params *p, const uint8_t *init_bin, const uint32_t *dyn_bin,
                           double *log_lik, double *initial) {
    EMGPU_TRY
    if (const int rc = check_args(h, p, init_bin, dyn_bin, log_lik)) return rc;
    CTX_ENTER(ctx);
    EmgpuScoreRun A;
    const bool per_step = fill_score(ctx, h, p, A);
    const size_t off = (size_t)p->col_offset;
    A.n = p->n; A.ld = p->ld ? p->ld : p->n;
    A.init_bin = init_bin ? init_bin + off : nullptr;
    A.dyn_bin = dyn_bin && p->sample_time > 1 ? dyn_bin + off : nullptr;
    A.log_lik = log_lik; A.initial = initial;
    A.bad = ctx->d_bad();
    ctx->last_launches = 0;
    launch_recorded(ctx, emgpu::launch_score_dbn, A, per_step);
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_score_dbn_host(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_score_params *p, const uint8_t *init_bin, const uint32_t *dyn_bin,
                         double *log_lik, double *initial) {
    EMGPU_TRY
    if (const int rc = check_args(h, p, init_bin, dyn_bin, log_lik)) return rc;
    CTX_ENTER(ctx);
    EmgpuScoreRun A;
    const bool per_step = fill_score(ctx, h, p, A);
    ctx->last_launches = 0;
    ctx->last_kernel = per_step ? "k_score_dbn[per-step]" : "k_score_dbn[frozen]";
    if (p->n == 0) return EMGPU_OK;
    const int64_t ld = p->ld ? p->ld : p->n;
    const size_t ni = (size_t)A.ni, rows_d = dyn_bin && p->sample_time > 1 ? (size_t)((p->sample_time + 3) / 4) * (size_t)A.nd : 0;
    CallBuffers B(ctx);
    enum { INIT, DYN, LL, INITIAL };   // the chunk's arrays: the bins as the kernel reads them, a double per lane for each output
    ChunkBlock blk(ctx, "emgpu_score_dbn_host", p->n, {{1, ni}, {4, rows_d}, {8, 1}, {8, 1}});
    const size_t c = (size_t)blk.c();
    A.ld = blk.c();
    A.init_bin = (const uint8_t *)blk.at(INIT);
    A.dyn_bin = rows_d ? (const uint32_t *)blk.at(DYN) : nullptr;
    A.log_lik = (double *)blk.at(LL);
    A.initial = initial ? (double *)blk.at(INITIAL) : nullptr;
    A.bad = ctx->d_bad();
    BadWordScope bad(ctx);
    blk.each([&](int64_t c0, int64_t cn) {
        const size_t src = (size_t)(p->col_offset + c0);
        HIP_OK(hipMemcpy2DAsync(blk.at(INIT), c, init_bin + src, (size_t)ld, (size_t)cn, ni, hipMemcpyHostToDevice, ctx->stream));
        if (rows_d) HIP_OK(hipMemcpy2DAsync(blk.at(DYN), 4 * c, dyn_bin + src, 4 * (size_t)ld, 4 * (size_t)cn, rows_d, hipMemcpyHostToDevice, ctx->stream));
        A.n = cn;
        launch_recorded(ctx, emgpu::launch_score_dbn, A, per_step);
        B.down(log_lik + c0, A.log_lik, 8 * (size_t)cn);
        if (initial) B.down(initial + c0, A.initial, 8 * (size_t)cn);
    });
    if (bad.finish()) return fail(EMGPU_ERR_ARG, kScoreBadBin);
    return EMGPU_OK;
    EMGPU_CATCH
}

} // extern "C"
