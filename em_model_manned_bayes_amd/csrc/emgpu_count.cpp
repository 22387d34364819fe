// emgpu_count.cpp -- emgpu_count_layout / emgpu_count_dbn_device / emgpu_count_dbn_host: the sufficient statistics of a trace (k_count_dbn,
// emgpu_kernels_count.hip; the definition is in emgpu_count.h and DESIGN.md), and emgpu_count_dbn_weighted_device / _host: the same with a
// u32 weight per trajectory (the kernel's weighted instances).  The host entry points upload and count chunk by chunk
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

// a call's arrays as the caller passed them; weights: null in an unweighted call, else one per trajectory (the weighted instances)
struct CountCall {
    const emgpu_score_params *p;
    const uint8_t *init_bin;
    const uint32_t *dyn_bin, *weights;
    uint64_t *counts_initial, *counts_transition;
};

// the caller's device arrays, counted where they are: one launch
int count_device(emgpu_ctx *ctx, const emgpu_model *, const CountCall &c, EmgpuCountRun &A, bool per_step) {
    const emgpu_score_params *p = c.p;
    const size_t off = (size_t)p->col_offset;
    A.G.n = p->n; A.G.ld = p->ld ? p->ld : p->n;
    A.G.init_bin = c.init_bin ? c.init_bin + off : nullptr;
    A.G.dyn_bin = c.dyn_bin && p->sample_time > 1 ? c.dyn_bin + off : nullptr;
    A.G.bad = ctx->d_bad();
    A.counts_i = (unsigned long long *)c.counts_initial; A.counts_t = (unsigned long long *)c.counts_transition;
    launch_recorded(ctx, emgpu::launch_count_dbn, A, c.weights, per_step);
    return EMGPU_OK;
}

// the caller's host arrays: uploaded and counted chunk by chunk, one launch per chunk
int count_host(emgpu_ctx *ctx, const emgpu_model *h, const CountCall &c, EmgpuCountRun &A, bool per_step) {
    const emgpu_score_params *p = c.p;
    const bool weighted = c.weights != nullptr;
    // an empty call reports its kernel too: with no table to count into yet (fill_count) the launcher names the instance and launches nothing
    const char *name = "";
    (void)emgpu::launch_count_dbn(A, c.weights, per_step, ctx->stream, &name);
    ctx->last_kernel = name;
    if (p->n == 0) return EMGPU_OK;
    const int64_t ld = p->ld ? p->ld : p->n;
    const bool dyn = c.counts_transition && c.dyn_bin && p->sample_time > 1;
    const size_t ni = (size_t)A.G.ni, rows_d = dyn ? (size_t)((p->sample_time + 3) / 4) * (size_t)A.G.nd : 0;
    // the device tables of this call: the model's size, whatever n is
    const size_t cells_i = c.counts_initial ? (size_t)layout(h->m, 0).back() : 0, cells_t = c.counts_transition ? (size_t)layout(h->m, 1).back() : 0;
    CallBuffers B(ctx);
    uint64_t *d_counts = B.alloc<uint64_t>((cells_i + cells_t + 1) * sizeof(uint64_t));
    HIP_OK(hipMemsetAsync(d_counts, 0, (cells_i + cells_t + 1) * sizeof(uint64_t), ctx->stream));
    A.counts_i = c.counts_initial ? (unsigned long long *)d_counts : nullptr;
    A.counts_t = c.counts_transition ? (unsigned long long *)(d_counts + cells_i) : nullptr;
    enum { INIT, DYN, WEIGHT };   // the chunk's arrays: the bins as the kernel reads them, and a weighted call's 4 bytes per lane
    ChunkBlock blk(ctx, weighted ? "emgpu_count_dbn_weighted_host" : "emgpu_count_dbn_host", p->n, {{1, ni}, {4, rows_d}, {4, weighted ? 1u : 0u}});
    const size_t cl = (size_t)blk.c();
    A.G.ld = blk.c();
    A.G.init_bin = (const uint8_t *)blk.at(INIT);
    A.G.dyn_bin = rows_d ? (const uint32_t *)blk.at(DYN) : nullptr;
    A.G.bad = ctx->d_bad();
    BadWordScope bad(ctx);
    blk.each([&](int64_t c0, int64_t cn) {
        const size_t src = (size_t)(p->col_offset + c0);
        HIP_OK(hipMemcpy2DAsync(blk.at(INIT), cl, c.init_bin + src, (size_t)ld, (size_t)cn, ni, hipMemcpyHostToDevice, ctx->stream));
        if (rows_d) HIP_OK(hipMemcpy2DAsync(blk.at(DYN), 4 * cl, c.dyn_bin + src, 4 * (size_t)ld, 4 * (size_t)cn, rows_d, hipMemcpyHostToDevice, ctx->stream));
        if (weighted) HIP_OK(hipMemcpyAsync(blk.at(WEIGHT), c.weights + c0, 4 * (size_t)cn, hipMemcpyHostToDevice, ctx->stream));   // not offset by col_offset
        A.G.n = cn;
        launch_recorded(ctx, emgpu::launch_count_dbn, A, weighted ? (const uint32_t *)blk.at(WEIGHT) : nullptr, per_step);
    });
    std::vector<uint64_t> got(cells_i + cells_t);
    B.down(got.data(), d_counts, got.size() * sizeof(uint64_t));
    const bool reported = bad.finish();
    for (size_t j = 0; j < cells_i; j++) c.counts_initial[j] += got[j];
    for (size_t j = 0; j < cells_t; j++) c.counts_transition[j] += got[cells_i + j];
    if (reported) return fail(EMGPU_ERR_ARG, kCountBadBin);
    return EMGPU_OK;
}

// What every entry point opens with, then its path: the argument check, the context, the uploaded model, the argument block under the form's
// cell cap (u64 partials hold half the cells) and a launch count of zero.  `weighted`: the entry point takes weights, which must be there.
int count(decltype(count_device) *path, emgpu_ctx *ctx, const emgpu_model *h, bool weighted, const CountCall &c) {
    if (const int rc = check_args(h, c.p, c.init_bin, c.dyn_bin, c.counts_initial, c.counts_transition, weighted, c.weights)) return rc;
    CTX_ENTER(ctx);
    EmgpuCountRun A;
    const bool per_step = fill_count(h->m, get_uploaded(ctx, h).cp.plan, c.p, c.counts_initial != nullptr, c.counts_transition != nullptr,
                                     weighted ? EMGPU_WCOUNT_LDS_CELLS : EMGPU_COUNT_LDS_CELLS, A);
    ctx->last_launches = 0;
    return path(ctx, h, c, A, per_step);
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
    return count(count_device, ctx, h, false, {p, init_bin, dyn_bin, nullptr, counts_initial, counts_transition});
    EMGPU_CATCH
}

int emgpu_count_dbn_host(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_score_params *p, const uint8_t *init_bin, const uint32_t *dyn_bin,
                         uint64_t *counts_initial, uint64_t *counts_transition) {
    EMGPU_TRY
    return count(count_host, ctx, h, false, {p, init_bin, dyn_bin, nullptr, counts_initial, counts_transition});
    EMGPU_CATCH
}

int emgpu_count_dbn_weighted_device(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_score_params *p, const uint8_t *init_bin,
                                    const uint32_t *dyn_bin, const uint32_t *weights, uint64_t *counts_initial, uint64_t *counts_transition) {
    EMGPU_TRY
    return count(count_device, ctx, h, true, {p, init_bin, dyn_bin, weights, counts_initial, counts_transition});
    EMGPU_CATCH
}

int emgpu_count_dbn_weighted_host(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_score_params *p, const uint8_t *init_bin,
                                  const uint32_t *dyn_bin, const uint32_t *weights, uint64_t *counts_initial, uint64_t *counts_transition) {
    EMGPU_TRY
    return count(count_host, ctx, h, true, {p, init_bin, dyn_bin, weights, counts_initial, counts_transition});
    EMGPU_CATCH
}

} // extern "C"
