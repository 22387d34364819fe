// emgpu_count.cpp -- emgpu_count_layout / emgpu_count_dbn_device / emgpu_count_dbn_host: the sufficient statistics of a trace (k_count_dbn,
// emgpu_kernels_count.hip; the definition is in emgpu_count.h and DESIGN.md), and emgpu_count_dbn_weighted_device / _host: the same with a
// u32 weight per trajectory (emgpu_kernels_wcount.hip).  The host entry points upload and count chunk by chunk
// (emgpu_tracechunk.hpp) into device tables they keep across the chunks, and add them to the caller's once, at the end.
#include <algorithm>
#include <cstring>
#include <utility>

#include "emgpu_count.h"
#include "emgpu_tracechunk.hpp"

using namespace emgpu_detail;

namespace {
constexpr const char *kCountBadBin = "count: a bin outside 1..r in the trace (the observations that read it were skipped)";

// the first element of every node's table in a network's counts array, and the total behind the last: the element order and count of
// emgpu_model_get_f64(EMGPU_F_N_INITIAL / EMGPU_F_N_TRANSITION, node), node after node
std::vector<int64_t> layout(const Model &m, int network) {
    const auto &N = network == 0 ? m.N_initial : m.N_transition;
    std::vector<int64_t> off(N.size() + 1, 0);
    for (size_t v = 0; v < N.size(); v++) off[v + 1] = off[v] + (int64_t)N[v].size();
    return off;
}

// `weighted`: the call takes weights, which must be there, and one call's n * max(1, T-1) observations per cell stay within 2^32
int check_args(const emgpu_model *h, const emgpu_score_params *p, const void *init_bin, const void *dyn_bin, const void *ci, const void *ct,
               bool weighted, const void *weights) {
    if (const int rc = emgpu::check_trace_args(h, p, init_bin, dyn_bin, ci || ct, "both counts arrays", ct != nullptr)) return rc;
    if (!weighted) return EMGPU_OK;
    if (!weights) return fail(EMGPU_ERR_ARG, "null weights (emgpu_count_dbn_* counts without weights)");
    if ((uint64_t)p->n * (uint64_t)std::max(1, p->sample_time - 1) > (1ull << 32))
        return fail(EMGPU_ERR_ARG, "weighted count: n * max(1, sample_time - 1) exceeds 2^32, a cell could wrap within the call: split the call");
    return EMGPU_OK;
}

// the kernel's argument block but its buffers; want_i / want_t: the networks the call counts; lds_cells: the partials the kernel keeps
bool fill_count(const Model &m, const EmgpuPlan &P, const emgpu_score_params *p, bool want_i, bool want_t, uint32_t lds_cells, EmgpuCountRun &A) {
    const std::vector<int64_t> oi = layout(m, 0), ot = layout(m, 1);
    if (oi.back() > 0xFFFFFFF0ll || ot.back() > 0xFFFFFFF0ll) throw Error(EMGPU_ERR_UNSUPPORTED, "count table too large (the kernel indexes it with 32 bits)");
    uint32_t i_off[EMGPU_MAX_NI] = {0}, d_off[EMGPU_MAX_ND] = {0};
    memset(&A, 0, sizeof A);
    std::vector<std::pair<uint32_t, int>> small;   // (cells, position p | 64 + row k) of the counted tables
    for (int q = 0; q < P.ni; q++) {
        i_off[q] = (uint32_t)oi[P.i_var[q]];
        A.i_cells[q] = (uint32_t)(oi[(size_t)P.i_var[q] + 1] - oi[P.i_var[q]]);
        if (want_i) small.push_back({A.i_cells[q], q});
    }
    for (int k = 0; k < m.n_dyn() && k < EMGPU_MAX_ND; k++) {
        const int tv = m.temporal_map[(size_t)k][1] - 1;
        if (tv < 0 || tv >= m.n_transition || m.N_transition[(size_t)tv].empty()) throw Error(EMGPU_ERR_ARG, "dynamic variable without a transition table");
        d_off[k] = (uint32_t)ot[(size_t)tv];
        A.d_cells[k] = (uint32_t)(ot[(size_t)tv + 1] - ot[(size_t)tv]);
        if (want_t) small.push_back({A.d_cells[k], 64 + k});
    }
    const bool per_step = emgpu::fill_trace_graph(P, p, i_off, d_off, A.G);
    // the LDS partials: the smallest tables first, while they fit
    for (auto &x : A.i_lds) x = EMGPU_COUNT_NO_LDS;
    for (auto &x : A.d_lds) x = EMGPU_COUNT_NO_LDS;
    std::sort(small.begin(), small.end());
    for (const auto &s : small) {
        if (A.lds_used + s.first > lds_cells) break;
        (s.second >= 64 ? A.d_lds[s.second - 64] : A.i_lds[s.second]) = A.lds_used;
        A.lds_used += s.first;
    }
    // whose bins an observation reads (a parent is a non-zero stride: a stride is a product of bin counts)
    for (int q = 0; q < P.ni; q++) {
        A.i_mask[q] = 1u << q;
        for (int j = 0; j < q; j++) if (A.G.i_stride[q][j]) A.i_mask[q] |= 1u << j;
    }
    for (int k = 0; k < P.nd; k++) {
        A.d_nmask[k] = 1u << k;
        for (int q = 0; q < P.ni; q++) if (A.G.d_static[k][q]) A.d_smask[k] |= 1u << q;
        for (int kp = 0; kp < P.nd; kp++) {
            if (A.G.d_cur[k][kp]) A.d_cmask[k] |= 1u << kp;
            if (A.G.d_new[k][kp]) A.d_nmask[k] |= 1u << kp;
        }
    }
    return per_step;
}

// the two launchers behind one signature: the weighted kernel when the call has weights (`weights` at the first trajectory of A.G)
void launch_count(emgpu_ctx *ctx, const EmgpuCountRun &A, const uint32_t *weights, bool per_step) {
    if (!weights) return launch_recorded(ctx, emgpu::launch_count_dbn, A, per_step);
    EmgpuWCountRun W;
    W.C = A; W.weights = weights;
    launch_recorded(ctx, emgpu::launch_count_dbn_weighted, W, per_step);
}
const char *kernel_name(bool weighted, bool per_step) {
    if (weighted) return per_step ? "k_count_dbn[per-step,weighted]" : "k_count_dbn[frozen,weighted]";
    return per_step ? "k_count_dbn[per-step]" : "k_count_dbn[frozen]";
}

int count_device(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_score_params *p, const uint8_t *init_bin, const uint32_t *dyn_bin,
                 bool weighted, const uint32_t *weights, uint64_t *counts_initial, uint64_t *counts_transition) {
    if (const int rc = check_args(h, p, init_bin, dyn_bin, counts_initial, counts_transition, weighted, weights)) return rc;
    CTX_ENTER(ctx);
    Uploaded &u = get_uploaded(ctx, h);
    EmgpuCountRun A;
    const bool per_step = fill_count(h->m, u.cp.plan, p, counts_initial != nullptr, counts_transition != nullptr,
                                     weighted ? EMGPU_WCOUNT_LDS_CELLS : EMGPU_COUNT_LDS_CELLS, A);
    const size_t off = (size_t)p->col_offset;
    A.G.n = p->n; A.G.ld = p->ld ? p->ld : p->n;
    A.G.init_bin = init_bin ? init_bin + off : nullptr;
    A.G.dyn_bin = dyn_bin && p->sample_time > 1 ? dyn_bin + off : nullptr;
    A.G.bad = ctx->d_bad();
    A.counts_i = (unsigned long long *)counts_initial; A.counts_t = (unsigned long long *)counts_transition;
    ctx->last_launches = 0;
    launch_count(ctx, A, weights, per_step);
    return EMGPU_OK;
}

int count_host(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_score_params *p, const uint8_t *init_bin, const uint32_t *dyn_bin,
               bool weighted, const uint32_t *weights, uint64_t *counts_initial, uint64_t *counts_transition) {
    if (const int rc = check_args(h, p, init_bin, dyn_bin, counts_initial, counts_transition, weighted, weights)) return rc;
    CTX_ENTER(ctx);
    Uploaded &u = get_uploaded(ctx, h);
    EmgpuCountRun A;
    const bool per_step = fill_count(h->m, u.cp.plan, p, counts_initial != nullptr, counts_transition != nullptr,
                                     weighted ? EMGPU_WCOUNT_LDS_CELLS : EMGPU_COUNT_LDS_CELLS, A);
    ctx->last_launches = 0;
    ctx->last_kernel = kernel_name(weighted, per_step);
    if (p->n == 0) return EMGPU_OK;
    const int64_t ld = p->ld ? p->ld : p->n;
    const bool dyn = counts_transition && dyn_bin && p->sample_time > 1;
    const size_t ni = (size_t)A.G.ni, rows_d = dyn ? (size_t)((p->sample_time + 3) / 4) * (size_t)A.G.nd : 0;
    // the device tables of this call: the model's size, whatever n is
    const size_t cells_i = counts_initial ? (size_t)layout(h->m, 0).back() : 0, cells_t = counts_transition ? (size_t)layout(h->m, 1).back() : 0;
    CallBuffers B(ctx);
    uint64_t *d_counts = B.alloc<uint64_t>((cells_i + cells_t + 1) * sizeof(uint64_t));
    HIP_OK(hipMemsetAsync(d_counts, 0, (cells_i + cells_t + 1) * sizeof(uint64_t), ctx->stream));
    A.counts_i = counts_initial ? (unsigned long long *)d_counts : nullptr;
    A.counts_t = counts_transition ? (unsigned long long *)(d_counts + cells_i) : nullptr;
    enum { INIT, DYN, WEIGHT };   // the chunk's arrays: the bins as the kernel reads them, and a weighted call's 4 bytes per lane
    ChunkBlock blk(ctx, weighted ? "emgpu_count_dbn_weighted_host" : "emgpu_count_dbn_host", p->n, {{1, ni}, {4, rows_d}, {4, weighted ? 1u : 0u}});
    const size_t c = (size_t)blk.c();
    A.G.ld = blk.c();
    A.G.init_bin = (const uint8_t *)blk.at(INIT);
    A.G.dyn_bin = rows_d ? (const uint32_t *)blk.at(DYN) : nullptr;
    A.G.bad = ctx->d_bad();
    BadWordScope bad(ctx);
    blk.each([&](int64_t c0, int64_t cn) {
        const size_t src = (size_t)(p->col_offset + c0);
        HIP_OK(hipMemcpy2DAsync(blk.at(INIT), c, init_bin + src, (size_t)ld, (size_t)cn, ni, hipMemcpyHostToDevice, ctx->stream));
        if (rows_d) HIP_OK(hipMemcpy2DAsync(blk.at(DYN), 4 * c, dyn_bin + src, 4 * (size_t)ld, 4 * (size_t)cn, rows_d, hipMemcpyHostToDevice, ctx->stream));
        if (weighted) HIP_OK(hipMemcpyAsync(blk.at(WEIGHT), weights + c0, 4 * (size_t)cn, hipMemcpyHostToDevice, ctx->stream));   // not offset by col_offset
        A.G.n = cn;
        launch_count(ctx, A, weighted ? (const uint32_t *)blk.at(WEIGHT) : nullptr, per_step);
    });
    std::vector<uint64_t> got(cells_i + cells_t);
    B.down(got.data(), d_counts, got.size() * sizeof(uint64_t));
    const bool reported = bad.finish();
    for (size_t j = 0; j < cells_i; j++) counts_initial[j] += got[j];
    for (size_t j = 0; j < cells_t; j++) counts_transition[j] += got[cells_i + j];
    if (reported) return fail(EMGPU_ERR_ARG, kCountBadBin);
    return EMGPU_OK;
}

} // namespace

extern "C" {

int emgpu_count_layout(const emgpu_model *h, int32_t network, int64_t *offsets) {
    EMGPU_TRY
    if (!h || !offsets) return fail(EMGPU_ERR_ARG, "null argument");
    if (network != 0 && network != 1) return fail(EMGPU_ERR_ARG, "network must be 0 (initial) or 1 (transition)");
    const std::vector<int64_t> off = layout(h->m, network);
    memcpy(offsets, off.data(), off.size() * sizeof(int64_t));
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_count_dbn_device(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_score_params *p, const uint8_t *init_bin, const uint32_t *dyn_bin,
                           uint64_t *counts_initial, uint64_t *counts_transition) {
    EMGPU_TRY
    return count_device(ctx, h, p, init_bin, dyn_bin, false, nullptr, counts_initial, counts_transition);
    EMGPU_CATCH
}

int emgpu_count_dbn_host(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_score_params *p, const uint8_t *init_bin, const uint32_t *dyn_bin,
                         uint64_t *counts_initial, uint64_t *counts_transition) {
    EMGPU_TRY
    return count_host(ctx, h, p, init_bin, dyn_bin, false, nullptr, counts_initial, counts_transition);
    EMGPU_CATCH
}

int emgpu_count_dbn_weighted_device(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_score_params *p, const uint8_t *init_bin,
                                    const uint32_t *dyn_bin, const uint32_t *weights, uint64_t *counts_initial, uint64_t *counts_transition) {
    EMGPU_TRY
    return count_device(ctx, h, p, init_bin, dyn_bin, true, weights, counts_initial, counts_transition);
    EMGPU_CATCH
}

int emgpu_count_dbn_weighted_host(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_score_params *p, const uint8_t *init_bin,
                                  const uint32_t *dyn_bin, const uint32_t *weights, uint64_t *counts_initial, uint64_t *counts_transition) {
    EMGPU_TRY
    return count_host(ctx, h, p, init_bin, dyn_bin, true, weights, counts_initial, counts_transition);
    EMGPU_CATCH
}

} // extern "C"
