// emgpu_score.cpp -- emgpu_score_dbn_device / emgpu_score_dbn_host: the log-likelihood of a trace under a model (k_score_dbn,
// emgpu_kernels_score.hip; the definition is in emgpu_score.h and DESIGN.md).  The host entry point uploads, scores and downloads in chunks of
// EMGPU_HOST_CHUNK_MB device bytes: it never holds device memory proportional to n.
#include <algorithm>
#include <cstring>
#include <string>

#include "emgpu_hostmem.hpp"
#include "emgpu_score.h"

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

// the kernel's argument block but its buffers
bool fill_score(const Uploaded &u, const emgpu_score_params *p, EmgpuScoreRun &A) {
    const bool per_step = emgpu::fill_trace_graph(u.cp.plan, p, u.lp_off, u.lpt_off, A);
    A.logp_i = u.d_logp; A.logp_t = u.d_logpt;
    return per_step;
}

int check_args(const emgpu_model *h, const emgpu_score_params *p, const void *init_bin, const void *dyn_bin, const void *log_lik) {
    return emgpu::check_trace_args(h, p, init_bin, dyn_bin, log_lik != nullptr, "log_lik", true);
}

void launch(emgpu_ctx *ctx, const EmgpuScoreRun &A, bool per_step) {
    const char *name = "";
    launch_ok(emgpu::launch_score_dbn(A, per_step, ctx->stream, &name));
    ctx->last_kernel = name;
    ctx->last_launches++;
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
    if (!ctx) return fail(EMGPU_ERR_ARG, "null ctx");
    CTX_LOCK(ctx);
    HIP_OK(hipSetDevice(ctx->device));
    Uploaded &u = get_uploaded(ctx, h);
    ensure_score_tables(ctx, u, h->m);
    EmgpuScoreRun A;
    const bool per_step = fill_score(u, p, A);
    const size_t off = (size_t)p->col_offset;
    A.n = p->n; A.ld = p->ld ? p->ld : p->n;
    A.init_bin = init_bin ? init_bin + off : nullptr;
    A.dyn_bin = dyn_bin && p->sample_time > 1 ? dyn_bin + off : nullptr;
    A.log_lik = log_lik; A.initial = initial;
    A.bad = ctx->d_status + 1;
    ctx->last_launches = 0;
    launch(ctx, A, per_step);
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_score_dbn_host(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_score_params *p, const uint8_t *init_bin, const uint32_t *dyn_bin,
                         double *log_lik, double *initial) {
    EMGPU_TRY
    if (const int rc = check_args(h, p, init_bin, dyn_bin, log_lik)) return rc;
    if (!ctx) return fail(EMGPU_ERR_ARG, "null ctx");
    CTX_LOCK(ctx);
    HIP_OK(hipSetDevice(ctx->device));
    Uploaded &u = get_uploaded(ctx, h);
    ensure_score_tables(ctx, u, h->m);
    EmgpuScoreRun A;
    const bool per_step = fill_score(u, p, A);
    ctx->last_launches = 0;
    ctx->last_kernel = per_step ? "k_score_dbn[per-step]" : "k_score_dbn[frozen]";
    if (p->n == 0) return EMGPU_OK;
    const int64_t ld = p->ld ? p->ld : p->n;
    const size_t ni = (size_t)A.ni, rows_d = dyn_bin && p->sample_time > 1 ? (size_t)((p->sample_time + 3) / 4) * (size_t)A.nd : 0;
    // a chunk: c trajectories, c a multiple of 256 (the device arrays' trajectory dimension), of about host_chunk_target device bytes
    const size_t per_lane = ni + 4 * rows_d + 16;
    const size_t target = host_chunk_target((size_t)256 << 20);
    const int64_t c = (int64_t)std::min<size_t>(round_up((size_t)p->n, 256), std::max<size_t>(target / per_lane / 256 * 256, 256));
    const size_t o_dyn = round_up(ni * (size_t)c, 256), o_ll = o_dyn + round_up(4 * rows_d * (size_t)c, 256), o_in = o_ll + 8 * (size_t)c;
    CallBuffers B(ctx);
    char *dev = (char *)device_block_or_trim(ctx, o_in + 8 * (size_t)c, true);
    if (!dev) return fail(EMGPU_ERR_HIP, "emgpu_score_dbn_host: out of device memory for one chunk");
    struct Release { emgpu_ctx *ctx; void *p; ~Release() { (void)hipStreamSynchronize(ctx->stream); device_release(p); } } release{ctx, dev};
    A.ld = c;
    A.init_bin = (const uint8_t *)dev;
    A.dyn_bin = rows_d ? (const uint32_t *)(dev + o_dyn) : nullptr;
    A.log_lik = (double *)(dev + o_ll);
    A.initial = initial ? (double *)(dev + o_in) : nullptr;
    A.bad = ctx->d_status + 1;
    // the word may hold the report of an earlier _device call nobody has synchronized on yet: that one is not this call's.  Take it out
    // before the first chunk and put it back behind the last, for the emgpu_ctx_sync it belongs to.
    HIP_OK(hipMemcpyAsync(ctx->h_status + 1, ctx->d_status + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(hipMemsetAsync(ctx->d_status + 1, 0, sizeof(uint32_t), ctx->stream));
    HIP_OK(hipStreamSynchronize(ctx->stream));
    const bool pending = ctx->h_status[1] != 0;
    for (int64_t c0 = 0; c0 < p->n; c0 += c) {
        const int64_t cn = std::min<int64_t>(c, p->n - c0);
        const size_t src = (size_t)(p->col_offset + c0);
        HIP_OK(hipMemcpy2DAsync(dev, (size_t)c, init_bin + src, (size_t)ld, (size_t)cn, ni, hipMemcpyHostToDevice, ctx->stream));
        if (rows_d) HIP_OK(hipMemcpy2DAsync(dev + o_dyn, 4 * (size_t)c, dyn_bin + src, 4 * (size_t)ld, 4 * (size_t)cn, rows_d, hipMemcpyHostToDevice, ctx->stream));
        A.n = cn;
        launch(ctx, A, per_step);
        B.down(log_lik + c0, A.log_lik, 8 * (size_t)cn);
        if (initial) B.down(initial + c0, A.initial, 8 * (size_t)cn);
        HIP_OK(hipStreamSynchronize(ctx->stream));   // the next chunk overwrites the buffer; the caller's arrays are pageable
    }
    HIP_OK(hipMemcpyAsync(ctx->h_status + 1, ctx->d_status + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(hipMemsetAsync(ctx->d_status + 1, pending ? 1 : 0, sizeof(uint32_t), ctx->stream));   // (any non-zero word is a report)
    HIP_OK(hipStreamSynchronize(ctx->stream));
    if (ctx->h_status[1]) return fail(EMGPU_ERR_ARG, kScoreBadBin);
    return EMGPU_OK;
    EMGPU_CATCH
}

} // extern "C"
