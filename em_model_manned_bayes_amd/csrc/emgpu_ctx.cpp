// emgpu_ctx.cpp -- the context: its life cycle, the cache of uploaded models and the device buffers it keeps between calls.
// No CPU fallback anywhere: without a HIP device emgpu_ctx_create fails with EMGPU_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "emgpu_internal.hpp"

extern "C" {

int emgpu_ctx_create(int32_t device, emgpu_ctx **out) {
    EMGPU_TRY
    if (!out) return fail(EMGPU_ERR_ARG, "null argument");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(EMGPU_ERR_NO_DEVICE, "no HIP device visible: libemgpu has no CPU path");
    if (device < 0 || device >= count) return fail(EMGPU_ERR_ARG, "device index out of range");
    std::unique_ptr<emgpu_ctx> c(new emgpu_ctx());
    c->device = device;
    HIP_OK(hipSetDevice(device));
    HIP_OK(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    HIP_OK(hipMalloc((void **)&c->d_status, 2 * sizeof(uint32_t)));   // word 1: k_score_dbn's "a bin outside 1..r" (a plain store, no atomic)
    HIP_OK(hipMemset(c->d_status, 0, 2 * sizeof(uint32_t)));
    HIP_OK(hipMalloc((void **)&c->d_queue, sizeof(uint32_t)));
    HIP_OK(hipHostMalloc((void **)&c->h_status, 2 * sizeof(uint32_t), hipHostMallocDefault));
    c->h_status[0] = *c->h_bad() = 0;
    *out = c.release();
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_ctx_set_stream(emgpu_ctx *ctx, void *hip_stream) {
    if (!ctx) return fail(EMGPU_ERR_ARG, "null ctx");
    CTX_LOCK(ctx);
    ctx->stream = (hipStream_t)hip_stream; // NULL = the HIP default (null) stream
    return EMGPU_OK;
}

int emgpu_ctx_sync(emgpu_ctx *ctx) {
    EMGPU_TRY
    CTX_ENTER(ctx);
    HIP_OK(hipMemcpyAsync(ctx->h_status, ctx->d_status, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIP_OK(hipMemsetAsync(ctx->d_status, 0, sizeof(uint32_t), ctx->stream));   // (word 1 stays until it is the one reported)
    HIP_OK(hipStreamSynchronize(ctx->stream));
    const uint32_t st = ctx->h_status[0];
    if (st & 1u) return fail(EMGPU_ERR_REJECT_CAP, "rejection loop reached max_attempts for at least one trajectory");
    if (st & 4u) return fail(EMGPU_ERR_PRESET, "Attempt to preset a dependent variable (a row of the start grid presets a node without its parents, or a bin outside 1..r)");
    if (st & 2u) return fail(EMGPU_ERR_EVENT_CAP, "an event list did not fit event_cap rows");
    if (*ctx->h_bad()) {   // one error per call: a bad-bin report behind a sampler's error above is kept for the next sync
        HIP_OK(hipMemsetAsync(ctx->d_bad(), 0, sizeof(uint32_t), ctx->stream));
        HIP_OK(hipStreamSynchronize(ctx->stream));
        return fail(EMGPU_ERR_ARG, emgpu_detail::kScoreBadBin);
    }
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_ctx_trim(emgpu_ctx *ctx) {
    EMGPU_TRY
    CTX_ENTER(ctx);
    HIP_OK(hipStreamSynchronize(ctx->stream));
    for (auto &sc : ctx->scratch) { if (sc.p) HIP_OK(hipFree(sc.p)); sc.p = nullptr; sc.cap = 0; }
    ctx_release_host_side(ctx, false);
    return EMGPU_OK;
    EMGPU_CATCH
}

void emgpu_ctx_free(emgpu_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    for (auto &kv : ctx->cache) kv.second.free_tables();
    for (auto &sc : ctx->scratch) (void)hipFree(sc.p);
    ctx_release_host_side(ctx, true);
    (void)hipFree(ctx->d_status);
    (void)hipFree(ctx->d_queue);
    (void)hipFree(ctx->d_presets);
    (void)hipFree(ctx->d_layers);
    (void)hipFree(ctx->d_thr_base);
    (void)hipHostFree(ctx->h_status);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    for (int q = 0; q < emgpu_ctx::kSide; q++) {
        if (ctx->side[q]) (void)hipStreamDestroy(ctx->side[q]);
        if (ctx->ev_join[q]) (void)hipEventDestroy(ctx->ev_join[q]);
    }
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    delete ctx;
}

const char *emgpu_last_kernel_name(const emgpu_ctx *ctx) { return ctx ? ctx->last_kernel.c_str() : ""; }
int32_t emgpu_last_launch_count(const emgpu_ctx *ctx) { return ctx ? ctx->last_launches : 0; }

} // extern "C"

// ------------------------------------------------------------------------------------------------
// `pinned`: uids of the other models of the current call -- their tables may already sit in a launch's
// argument list (terminal propagation, mixed batches) and must survive the eviction.
// Entries outlive emgpu_model_free (a model does not know the contexts that uploaded it): they are
// reclaimed by this LRU sweep or by emgpu_ctx_free; at most 48 + the models of one call stay resident.
Uploaded &get_uploaded(emgpu_ctx *ctx, const emgpu_model *h, const std::set<uint64_t> *pinned) {
    if (ctx->cache.size() > 48 && ctx->cache.find(h->m.uid) == ctx->cache.end()) {
        // models come and go (their tables stay uploaded): drop the least recently used half
        HIP_OK(hipStreamSynchronize(ctx->stream));
        std::vector<std::pair<uint64_t, uint64_t>> byuse;
        for (auto &kv : ctx->cache)
            if (!pinned || !pinned->count(kv.first)) byuse.push_back({kv.second.last_use, kv.first});
        std::sort(byuse.begin(), byuse.end());
        for (size_t q = 0; q < byuse.size() / 2; q++) {
            ctx->cache[byuse[q].second].free_tables();
            ctx->cache.erase(byuse[q].second);
        }
    }
    Uploaded &u = ctx->cache[h->m.uid];
    u.last_use = ++ctx->use_clock;
    if (u.version == h->m.version && u.d_thr) return u;
    // (re)compile: tables depend on N, alpha, start, boundaries, rates
    CompiledPlan cp = *emgpu::plan_of(h->m);   // (the model keeps its plan: a second ctx, or a model read from the binary cache, does not search the thresholds again)
    HIP_OK(hipStreamSynchronize(ctx->stream)); // nothing in flight may still read the old tables
    u.free_tables();
    // 64 words of slack: k_terminal_propagate reads a row's thresholds in fixed groups (8, or every 6th up to index 41) and masks
    // the ones past the row's end instead of clamping every index
    const size_t nthr = cp.thr.size() + 64;
    HIP_OK(hipMalloc((void **)&u.d_thr, nthr * sizeof(uint32_t)));
    HIP_OK(hipMemset(u.d_thr + cp.thr.size(), 0xFF, 64 * sizeof(uint32_t)));
    HIP_OK(hipMalloc((void **)&u.d_bnd, cp.bnd.size() * sizeof(double)));
    if (!cp.thr.empty()) HIP_OK(hipMemcpy(u.d_thr, cp.thr.data(), cp.thr.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(u.d_bnd, cp.bnd.data(), cp.bnd.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_OK(hipMalloc((void **)&u.d_cthr, (cp.cthr.size() ? cp.cthr.size() : 1) * sizeof(uint32_t)));
    if (!cp.cthr.empty()) HIP_OK(hipMemcpy(u.d_cthr, cp.cthr.data(), cp.cthr.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    u.cp = std::move(cp);
    u.cp.plan.thr = u.d_thr;
    u.cp.plan.bnd = u.d_bnd;
    u.cp.plan.cthr = u.d_cthr;
    HIP_OK(hipMalloc((void **)&u.d_pthr, (u.cp.pthr.size() ? u.cp.pthr.size() : 4) * sizeof(uint32_t)));
    if (!u.cp.pthr.empty()) HIP_OK(hipMemcpy(u.d_pthr, u.cp.pthr.data(), u.cp.pthr.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    u.cp.plan.pthr = u.d_pthr;
    {   // the finished plan (device pointers in place) next to its tables, for k_uncor_fast_mixed
        std::vector<char> pf(emgpu::plan_f_bytes());
        emgpu::plan_f_fill(u.cp.plan, pf.data());
        HIP_OK(hipMalloc(&u.d_planf, pf.size()));
        HIP_OK(hipMemcpy(u.d_planf, pf.data(), pf.size(), hipMemcpyHostToDevice));
    }
    u.version = h->m.version;
    return u;
}

// the log-probability table behind per-sample log-weights, uploaded on first use (with the model version it was built for: get_uploaded
// frees every table when the model changes)
void ensure_logp(emgpu_ctx *ctx, Uploaded &u, const Model &m) {
    if (u.d_logp) return;
    const std::vector<double> lp = emgpu::initial_log_prob(m, u.lp_off);
    HIP_OK(hipMalloc((void **)&u.d_logp, (lp.size() + 1) * sizeof(double)));
    HIP_OK(hipMemcpyAsync(u.d_logp, lp.data(), lp.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_OK(hipStreamSynchronize(ctx->stream));
}

// the one place a buffer of the ctx is replaced by a larger one (the contract: emgpu_internal.hpp)
void ctx_grow(emgpu_ctx *ctx, void **p, size_t *cap, size_t need, size_t size) {
    if (*p && *cap >= need) return;
    HIP_OK(hipStreamSynchronize(ctx->stream));
    if (*p) HIP_OK(hipFree(*p));
    *p = nullptr; *cap = 0;
    HIP_OK(hipMalloc(p, size));
    *cap = size;
}

// slot-th scratch buffer of the ctx, at least `bytes` long (contents undefined; valid until the next request for the same slot)
void *ctx_scratch(emgpu_ctx *ctx, size_t slot, size_t bytes) {
    if (ctx->scratch.size() <= slot) ctx->scratch.resize(slot + 1);
    emgpu_ctx::Scratch &sc = ctx->scratch[slot];
    ctx_grow(ctx, &sc.p, &sc.cap, bytes, bytes + bytes / 8 + 256);   // some headroom: batch sizes that wobble do not reallocate
    return sc.p;
}
