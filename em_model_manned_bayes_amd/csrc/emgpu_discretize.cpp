// emgpu_discretize.cpp -- emgpu_discretize_dbn_device / emgpu_discretize_dbn_host: a trace of values into a trace of bins, and the repeat /
// change counts of its fine bins (k_discretize_dbn, emgpu_kernels_discretize.hip; the definition is in emgpu_discretize.h and DESIGN.md).
// The host entry point uploads, discretizes and downloads chunk by chunk (emgpu_tracechunk.hpp), into two device vectors it keeps across
// the chunks and adds to the caller's once, at the end.
#include <cstring>

#include "emgpu_discretize.h"
#include "emgpu_score.h"
#include "emgpu_tracechunk.hpp"

using namespace emgpu_detail;

namespace {
constexpr const char *kBadValue = "discretize: a NaN, or a categorical value that is no integer in 1..r, in the trace (its bin is 0; no pair holds it)";

// what can be said without a device: EMGPU_OK, or the error (recorded)
int check_args(const emgpu_model *h, const emgpu_discretize_params *p, const void *init_val, const void *dyn_val, const void *init_bin,
               const void *dyn_bin, const void *repeat, const void *change) {
    if (!h || !p) return fail(EMGPU_ERR_ARG, "null argument");
    // n, sample_time, ld / col_offset and the compiled maxima: the rules of every trace call (the pointers are this call's own business)
    const emgpu_score_params sp = {p->n, p->sample_time, EMGPU_TRANSITION_REFERENCE_AUTO, p->ld, p->col_offset};
    if (const int rc = emgpu::check_trace_args(h, &sp, p, p, true, "", false)) return rc;
    if (p->n_fine != 0 && (p->n_fine < 2 || p->n_fine > 255)) return fail(EMGPU_ERR_ARG, "n_fine must be 0 (bins only) or 2..255");
    if (p->value_type != EMGPU_VALUE_F32 && p->value_type != EMGPU_VALUE_F64) return fail(EMGPU_ERR_ARG, "unknown value_type");
    if (h->m.n_initial < 32 && (p->wrap_mask >> h->m.n_initial)) return fail(EMGPU_ERR_ARG, "wrap_mask names a variable the model does not have");
    if ((init_val == nullptr) != (init_bin == nullptr)) return fail(EMGPU_ERR_ARG, "init_val and init_bin come as a pair: one of them is null");
    if ((dyn_val == nullptr) != (dyn_bin == nullptr)) return fail(EMGPU_ERR_ARG, "dyn_val and dyn_bin come as a pair: one of them is null");
    if (p->n > 0 && !init_val && !dyn_val) return fail(EMGPU_ERR_ARG, "null init and dyn halves: nothing to discretize");
    if (p->n_fine > 0 && (!repeat || !change)) return fail(EMGPU_ERR_ARG, "n_fine > 0 needs both the repeat and the change vector");
    return EMGPU_OK;
}

// the kernel's argument block but its trace buffers
void fill(const Model &m, const Uploaded &u, const emgpu_discretize_params *p, EmgpuDiscretizeRun &A) {
    const EmgpuPlan &P = u.cp.plan;
    memset(&A, 0, sizeof A);
    A.T = p->sample_time; A.ni = m.n_initial; A.nd = m.n_dyn(); A.n_fine = p->n_fine; A.wrap_mask = p->wrap_mask;
    A.bnd = u.d_bnd;
    for (int v = 0; v < m.n_initial; v++) {
        const int pos = u.cp.pos_of_var[(size_t)v];
        A.v_r[v] = (uint8_t)m.r_initial[(size_t)v];
        A.v_cont[v] = m.boundaries[(size_t)v].empty() ? 0 : 1;   // (compile_plan: a variable with boundaries has at least r + 1)
        A.v_zero[v] = (size_t)v < m.zero_bins.size() ? (uint8_t)m.zero_bins[(size_t)v] : 0;
        A.v_boff[v] = P.i_boff[pos];
    }
    for (int k = 0; k < A.nd; k++) {
        const int v = m.temporal_map[(size_t)k][0] - 1;
        if (v < 0 || v >= m.n_initial) throw Error(EMGPU_ERR_ARG, "temporal map row without an initial variable");
        A.d_var[k] = (uint8_t)v;
    }
}

} // namespace

extern "C" {

int emgpu_discretize_dbn_device(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_discretize_params *p, const void *init_val, const void *dyn_val,
                                uint8_t *init_bin, uint32_t *dyn_bin, uint64_t *repeat, uint64_t *change) {
    EMGPU_TRY
    if (const int rc = check_args(h, p, init_val, dyn_val, init_bin, dyn_bin, repeat, change)) return rc;
    if (((uintptr_t)dyn_val & 15u) || ((uintptr_t)dyn_bin & 3u)) return fail(EMGPU_ERR_ARG, "dyn_val must be 16-byte aligned and dyn_bin 4-byte aligned");
    CTX_ENTER(ctx);
    Uploaded &u = get_uploaded(ctx, h);
    EmgpuDiscretizeRun A;
    fill(h->m, u, p, A);
    const bool f64 = p->value_type == EMGPU_VALUE_F64;
    const size_t es = f64 ? 8 : 4, off = (size_t)p->col_offset;
    const bool dyn = dyn_val && A.nd > 0;
    A.n = p->n; A.ld = p->ld ? p->ld : p->n;
    A.init_val = init_val ? (const char *)init_val + es * off : nullptr;
    A.init_bin = init_bin ? init_bin + off : nullptr;
    A.dyn_val = dyn ? (const char *)dyn_val + 4 * es * off : nullptr;
    A.dyn_bin = dyn ? dyn_bin + off : nullptr;
    A.repeat = p->n_fine > 0 ? (unsigned long long *)repeat : nullptr;
    A.change = p->n_fine > 0 ? (unsigned long long *)change : nullptr;
    A.bad = ctx->d_bad();
    ctx->last_launches = 0;
    launch_recorded(ctx, emgpu::launch_discretize_dbn, A, f64);
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_discretize_dbn_host(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_discretize_params *p, const void *init_val, const void *dyn_val,
                              uint8_t *init_bin, uint32_t *dyn_bin, uint64_t *repeat, uint64_t *change) {
    EMGPU_TRY
    if (const int rc = check_args(h, p, init_val, dyn_val, init_bin, dyn_bin, repeat, change)) return rc;
    CTX_ENTER(ctx);
    Uploaded &u = get_uploaded(ctx, h);
    EmgpuDiscretizeRun A;
    fill(h->m, u, p, A);
    const bool f64 = p->value_type == EMGPU_VALUE_F64;
    ctx->last_launches = 0;
    ctx->last_kernel = f64 ? "k_discretize_dbn[f64]" : "k_discretize_dbn[f32]";
    if (p->n == 0) return EMGPU_OK;
    const int64_t ld = p->ld ? p->ld : p->n;
    const size_t es = f64 ? 8 : 4;
    const size_t ni = init_val ? (size_t)A.ni : 0, rows_d = dyn_val ? (size_t)((p->sample_time + 3) / 4) * (size_t)A.nd : 0;
    const bool pairs = p->n_fine > 0;
    if (!ni && !rows_d) return EMGPU_OK;   // (a dynamic half alone, of a model without dynamic variables)
    // the two device vectors of this call: the model's size, whatever n is
    CallBuffers B(ctx);
    uint64_t *d_rc = B.alloc<uint64_t>(2 * EMGPU_MAX_NI * sizeof(uint64_t));
    HIP_OK(hipMemsetAsync(d_rc, 0, 2 * EMGPU_MAX_NI * sizeof(uint64_t), ctx->stream));
    A.repeat = pairs ? (unsigned long long *)d_rc : nullptr;
    A.change = pairs ? (unsigned long long *)(d_rc + EMGPU_MAX_NI) : nullptr;
    enum { INIT_VAL, DYN_VAL, INIT_BIN, DYN_BIN };   // the chunk's arrays: the values as the kernel reads them, the bins as it writes them
    ChunkBlock blk(ctx, "emgpu_discretize_dbn_host", p->n, {{es, ni}, {4 * es, rows_d}, {1, ni}, {4, rows_d}});
    const size_t c = (size_t)blk.c();
    A.ld = blk.c();
    A.init_val = ni ? blk.at(INIT_VAL) : nullptr;
    A.dyn_val = rows_d ? blk.at(DYN_VAL) : nullptr;
    A.init_bin = ni ? (uint8_t *)blk.at(INIT_BIN) : nullptr;
    A.dyn_bin = rows_d ? (uint32_t *)blk.at(DYN_BIN) : nullptr;
    A.bad = ctx->d_bad();
    BadWordScope bad(ctx);
    blk.each([&](int64_t c0, int64_t cn) {
        const size_t src = (size_t)(p->col_offset + c0);
        if (ni) HIP_OK(hipMemcpy2DAsync(blk.at(INIT_VAL), es * c, (const char *)init_val + es * src, es * (size_t)ld, es * (size_t)cn, ni, hipMemcpyHostToDevice, ctx->stream));
        if (rows_d) HIP_OK(hipMemcpy2DAsync(blk.at(DYN_VAL), 4 * es * c, (const char *)dyn_val + 4 * es * src, 4 * es * (size_t)ld, 4 * es * (size_t)cn, rows_d, hipMemcpyHostToDevice, ctx->stream));
        A.n = cn;
        launch_recorded(ctx, emgpu::launch_discretize_dbn, A, f64);
        if (ni) HIP_OK(hipMemcpy2DAsync(init_bin + src, (size_t)ld, blk.at(INIT_BIN), c, (size_t)cn, ni, hipMemcpyDeviceToHost, ctx->stream));
        if (rows_d) HIP_OK(hipMemcpy2DAsync(dyn_bin + src, 4 * (size_t)ld, blk.at(DYN_BIN), 4 * c, 4 * (size_t)cn, rows_d, hipMemcpyDeviceToHost, ctx->stream));
    });
    uint64_t got[2 * EMGPU_MAX_NI] = {0};
    if (pairs) B.down(got, d_rc, sizeof got);
    const bool reported = bad.finish();
    for (int v = 0; pairs && v < A.ni; v++) { repeat[v] += got[v]; change[v] += got[EMGPU_MAX_NI + v]; }
    if (reported) return fail(EMGPU_ERR_ARG, kBadValue);
    return EMGPU_OK;
    EMGPU_CATCH
}

} // extern "C"
