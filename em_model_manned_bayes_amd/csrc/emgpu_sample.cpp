// emgpu_sample.cpp -- the DBN and BN sampling entry points on device pointers: a call's run and its output binding, the start-grid block,
// the launch through the dispatcher, the mixed-batch launcher and the multi-device fan-out.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "emgpu_internal.hpp"

void fill_run(emgpu_ctx *ctx, const Uploaded &u, const Model &m, const emgpu_sample_params *p, EmgpuRun &A) {
    memset(&A, 0, sizeof A);
    if (p->n < 0 || p->sample_time < 1 || p->sample_time > 65535) throw Error(EMGPU_ERR_ARG, "n < 0 or sample_time outside 1..65535");
    if (p->max_attempts < 1) throw Error(EMGPU_ERR_ARG, "max_attempts must be >= 1");
    A.seed = p->seed; A.first_index = p->first_index; A.n = p->n; A.T = p->sample_time;
    A.per_step = p->transition_mode == EMGPU_TRANSITION_PER_STEP;
    A.flags = p->flags; A.max_attempts = p->max_attempts;
    auto pos = [&](int idx1) -> int {
        if (idx1 == 0) return -1;
        if (idx1 < 1 || idx1 > m.n_initial) throw Error(EMGPU_ERR_ARG, "variable index out of range");
        return u.cp.pos_of_var[idx1 - 1];
    };
    A.pos_L = pos(p->idx_L); A.pos_v = pos(p->idx_v); A.pos_dh = pos(p->idx_dh);
    A.n_layers = 0; A.layers = nullptr;
    if (p->layers && p->n_layers > 0) {
        if (p->idx_L == 0) throw Error(EMGPU_ERR_ARG, "layers given without idx_L");
        if (!m.boundaries[p->idx_L - 1].empty() && !(p->flags & EMGPU_FLAG_NO_DEDISC))
            throw Error(EMGPU_ERR_ARG, "layers need L to stay a bin index (isOverwriteZeroBoundaries)");
        if (p->n_layers < m.r_initial[p->idx_L - 1]) throw Error(EMGPU_ERR_ARG, "layers has fewer rows than L has bins");
        const size_t bytes = (size_t)p->n_layers * 2 * sizeof(double);
        ctx_grow(ctx, (void **)&ctx->d_layers, &ctx->d_layers_cap, bytes, bytes);
        HIP_OK(hipMemcpyAsync(ctx->d_layers, p->layers, bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_OK(hipStreamSynchronize(ctx->stream)); // p->layers is caller memory
        A.layers = ctx->d_layers; A.n_layers = p->n_layers;
    }
    A.event_cap = p->event_cap;
    A.status = ctx->d_status;
    A.ld = p->n;
    A.indices = p->indices;
}

// Point the run at the caller's buffers: column col_offset of arrays whose trajectory dimension is ld.
static void bind_outputs(EmgpuRun &A, const Model &m, const emgpu_sample_params *p, const emgpu_sample_out *out, int64_t extra_offset = 0) {
    if ((out->ev_count != nullptr) != (out->events != nullptr)) throw Error(EMGPU_ERR_ARG, "ev_count and events go together");
    if (out->events && p->event_cap < 1) throw Error(EMGPU_ERR_ARG, "event_cap must be >= 1");
    const int64_t ld = out->ld ? out->ld : A.n, off = out->col_offset + extra_offset;
    if (ld < 0 || off < 0 || off + A.n > ld) throw Error(EMGPU_ERR_ARG, "col_offset + n exceeds ld");
    A.ld = ld;
    A.col0 = off;
    const size_t o = (size_t)off;
    A.init_bin = out->init_bin ? out->init_bin + o : nullptr;
    A.init_val = out->init_val ? out->init_val + o : nullptr;
    A.dyn_bin = out->dyn_bin ? out->dyn_bin + o : nullptr;
    A.dyn_val = out->dyn_val ? out->dyn_val + 4 * o : nullptr;
    A.ev_count = out->ev_count ? out->ev_count + o : nullptr;
    A.events = out->events ? reinterpret_cast<uint64_t *>(out->events) + o * (size_t)p->event_cap : nullptr;
    A.attempts = out->attempts ? out->attempts + o : nullptr;
    (void)m;
}

const EmgpuPresets *upload_presets(emgpu_ctx *ctx, Uploaded &u, const Model &m, const int32_t *start, double *log_weight, const int64_t *row) {
    EmgpuPresets Q;
    memset(&Q, 0, sizeof Q);
    Q.start = start; Q.log_weight = log_weight; Q.row = row;
    if (Q.log_weight) { ensure_logp(ctx, u, m); Q.logp = u.d_logp; memcpy(Q.lp_off, u.lp_off, sizeof Q.lp_off); }
    if (!ctx->d_presets) HIP_OK(hipMalloc((void **)&ctx->d_presets, sizeof(EmgpuPresets)));
    HIP_OK(hipStreamSynchronize(ctx->stream));   // (an earlier launch may still read the block)
    HIP_OK(hipMemcpyAsync(ctx->d_presets, &Q, sizeof Q, hipMemcpyHostToDevice, ctx->stream));
    HIP_OK(hipStreamSynchronize(ctx->stream));   // Q is a local
    return ctx->d_presets;
}

void launch_dbn(emgpu_ctx *ctx, const Uploaded &u, const EmgpuRun &A, hipStream_t stream, const EmgpuPresets *presets) {
    if (!stream) stream = ctx->stream;
    const EmgpuPlan &P = u.cp.plan;
    const emgpu::DbnChoice c = emgpu::choose_dbn(P, A, presets != nullptr);
    ctx->last_kernel = c.name;
    ctx->last_launches++;
    switch (c.family) {
    case emgpu::DbnFamily::Fast: launch_ok(emgpu::launch_uncor_fast(P, A, c, presets, stream)); break;
    case emgpu::DbnFamily::Step2: launch_ok(emgpu::launch_dbn_step2(P, A, c, presets, stream)); break;
    case emgpu::DbnFamily::Step: launch_ok(emgpu::launch_dbn_step(P, A, c, stream)); break;
    case emgpu::DbnFamily::Generic: launch_ok(emgpu::launch_dbn_generic(P, A, c, presets, stream)); break;
    }
}

// Run fn(d) for d = 0..n-1 on one host thread per device and fold the results: the first
// failing device's status and message become the caller's.
template <typename F>
static int on_devices(int n, F fn) {
    std::vector<int> rc((size_t)n, EMGPU_OK);
    std::vector<std::string> msg((size_t)n);
    auto body = [&](int d) {
        rc[d] = fn(d);
        if (rc[d] != EMGPU_OK) msg[d] = g_err; // g_err is thread-local
    };
    std::vector<std::thread> th;
    for (int d = 1; d < n; d++) th.emplace_back(body, d);
    body(0);
    for (auto &t : th) t.join();
    for (int d = 0; d < n; d++)
        if (rc[d] != EMGPU_OK) return fail(rc[d], "device " + std::to_string(d) + ": " + msg[d]);
    return EMGPU_OK;
}

void fill_bn(emgpu_ctx *ctx, const Uploaded &u, const Model &m, const emgpu_bn_params *p, EmgpuBnRun &A) {
    memset(&A, 0, sizeof A);
    if (p->n < 0 || p->max_attempts < 1) throw Error(EMGPU_ERR_ARG, "n < 0 or max_attempts < 1");
    A.seed = p->seed; A.first_index = p->first_index; A.n = p->n; A.ld = p->n; A.flags = p->flags; A.max_attempts = p->max_attempts;
    A.has_bounds = p->bounds_sample != nullptr;
    if (p->bounds_sample)
        for (int v = 0; v < m.n_initial; v++) {
            A.bounds[u.cp.pos_of_var[v]][0] = p->bounds_sample[2 * v];
            A.bounds[u.cp.pos_of_var[v]][1] = p->bounds_sample[2 * v + 1];
        }
    A.pos_own_speed = A.pos_int_speed = -1;
    if (p->idx_own_speed > 0 || p->idx_int_speed > 0) {
        if (p->idx_own_speed < 1 || p->idx_own_speed > m.n_initial || p->idx_int_speed < 1 || p->idx_int_speed > m.n_initial)
            throw Error(EMGPU_ERR_ARG, "speed variable index out of range");
        A.pos_own_speed = u.cp.pos_of_var[p->idx_own_speed - 1];
        A.pos_int_speed = u.cp.pos_of_var[p->idx_int_speed - 1];
    }
    A.min1 = p->min_vel1; A.max1 = p->max_vel1; A.min2 = p->min_vel2; A.max2 = p->max_vel2;
    A.status = ctx->d_status;
    A.start = p->start; A.log_weight = p->log_weight;
}

// shard d of n_ctx of a multi-device call: its parameters (the index range, and its own entries of the lists the call covers) and where it
// begins among the call's columns
static emgpu_sample_params shard_params(const emgpu_sample_params *p, const emgpu_model *h, int d, int n_ctx, int64_t *lo) {
    int64_t hi;
    emgpu_shard_range(p->n, d, n_ctx, lo, &hi);
    emgpu_sample_params q = *p;
    q.first_index = p->first_index + (uint64_t)*lo; q.n = hi - *lo;
    if (p->indices) q.indices = p->indices + *lo;   // shard d draws entries [lo, hi) of the list
    if (p->start) q.start = p->start + (size_t)*lo * (size_t)h->m.n_initial;   // ... and its own rows of the start grid
    return q;
}

extern "C" {

int emgpu_sample_dbn_device(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_sample_params *p, const emgpu_sample_out *out) {
    EMGPU_TRY
    if (!ctx || !h || !p || !out) return fail(EMGPU_ERR_ARG, "null argument");
    CTX_DEVICE(ctx);
    Uploaded &u = get_uploaded(ctx, h);
    EmgpuRun A;
    fill_run(ctx, u, h->m, p, A);
    bind_outputs(A, h->m, p, out);
    const EmgpuPresets *presets = nullptr;
    // a start grid / per-sample log-weights: a small block of device memory the kernel reads them through
    if (p->start || out->log_weight) presets = upload_presets(ctx, u, h->m, p->start, out->log_weight, nullptr);
    ctx->last_launches = 0;
    launch_dbn(ctx, u, A, nullptr, presets);
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_sample_dbn_blocks_device(emgpu_ctx *ctx, const emgpu_model *const *models, int32_t n_models,
                                   const emgpu_sample_params *p, const emgpu_block *blocks, int32_t n_blocks,
                                   const emgpu_sample_out *out) {
    EMGPU_TRY
    if (!ctx || !models || n_models < 1 || !p || (!blocks && n_blocks > 0) || n_blocks < 0 || !out) return fail(EMGPU_ERR_ARG, "null argument");
    if (p->start || out->log_weight) return fail(EMGPU_ERR_UNSUPPORTED, "a start grid / log-weights in a mixed-model batch: sample the models one by one");
    CTX_DEVICE(ctx);
    std::set<uint64_t> pinned;
    for (int i = 0; i < n_models; i++) {
        if (!models[i]) return fail(EMGPU_ERR_ARG, "null model");
        if (models[i]->m.n_initial != models[0]->m.n_initial || models[i]->m.n_dyn() != models[0]->m.n_dyn())
            return fail(EMGPU_ERR_ARG, "the models of a mixed batch must agree in n_initial and n_dyn (one trace shape)");
        pinned.insert(models[i]->m.uid);
    }
    emgpu_sample_out o = *out;
    if (!o.ld) o.ld = p->n;
    // Everything that can fail -- argument checks, table uploads (get_uploaded may synchronise the ctx stream), the runs and
    // their output bindings -- happens before the first launch: an error leaves nothing in flight.
    struct Live { const Uploaded *u; EmgpuRun A; int64_t col; int shape; };
    std::vector<Live> live;
    for (int b = 0; b < n_blocks; b++) {
        const emgpu_block &B = blocks[b];
        if (B.model < 0 || B.model >= n_models) return fail(EMGPU_ERR_ARG, "block names a model outside the list");
        if (B.n < 0 || B.first_index < p->first_index || B.first_index - p->first_index + (uint64_t)B.n > (uint64_t)p->n)
            return fail(EMGPU_ERR_ARG, "block outside [first_index, first_index + n)");
        if (B.n == 0) continue;
        const emgpu_model *h = models[B.model];
        const Uploaded &u = get_uploaded(ctx, h, &pinned);   // std::map: the reference stays valid, and nothing pinned is evicted
        const int64_t col = (int64_t)(B.first_index - p->first_index);
        emgpu_sample_params q = *p;
        q.first_index = B.first_index; q.n = B.n;
        if (p->indices) q.indices = p->indices + col;   // an index list covers the call's columns: block b draws its own entries
        Live L;
        L.u = &u; L.col = col;
        fill_run(ctx, u, h->m, &q, L.A);
        bind_outputs(L.A, h->m, &q, &o, col);
        // (event lists: k_uncor_fast_ev, one launch per block -- the shared launch writes the dense trace only)
        // (... and stores both dense outputs unconditionally)
        const emgpu::DbnChoice c = emgpu::choose_dbn(u.cp.plan, L.A, false);
        L.shape = (c.family == emgpu::DbnFamily::Fast && c.form == emgpu::FastForm::Dense) ? c.shape : -1;
        live.push_back(L);
    }
    ctx->last_launches = 0;
    if (live.empty()) return EMGPU_OK;
    // Blocks whose models run on the same k_uncor_fast instance share ONE launch (model id per workgroup); every other block
    // is its own launch.  With several launches they go round-robin over the ctx stream and three side streams, forked from
    // and joined back into the ctx stream with events (a caller sees one in-order operation).
    static const bool no_mixed_env = getenv("EMGPU_DEBUG_NO_MIXED_LAUNCH") != nullptr;
    const bool no_mixed = no_mixed_env || p->indices != nullptr;   // (an index list: one launch per block, k_uncor_fast_idx)
    struct Launch { int shape; std::vector<int> members; };
    std::vector<Launch> launches;
    // the run of a shared launch is common to its blocks but for the index range and the columns: the rejection test's variables
    // must sit at the same topological positions in every member
    auto same_positions = [](const EmgpuRun &a, const EmgpuRun &b) { return a.pos_L == b.pos_L && a.pos_v == b.pos_v && a.pos_dh == b.pos_dh; };
    for (int i = 0; i < (int)live.size(); i++) {
        Launch *into = nullptr;
        if (live[i].shape >= 0 && !no_mixed)
            for (auto &g : launches)
                if (g.shape == live[i].shape && (int)g.members.size() < EMGPU_MAX_MIXED && same_positions(live[g.members[0]].A, live[i].A)) { into = &g; break; }
        if (into) into->members.push_back(i);
        else launches.push_back(Launch{live[i].shape, {i}});
    }
    static const bool no_side = getenv("EMGPU_DEBUG_NO_SIDE_STREAMS") != nullptr;
    const bool fork = launches.size() >= 2 && !no_side;
    int used = 0; // side streams in use
    struct Join {   // runs on every way out: side streams that were forked are joined back even when a launch fails
        emgpu_ctx *ctx; int *used;
        ~Join() {
            for (int q = 0; q < *used; q++) {
                (void)hipEventRecord(ctx->ev_join[q], ctx->side[q]);
                (void)hipStreamWaitEvent(ctx->stream, ctx->ev_join[q], 0);
            }
        }
    } join{ctx, &used};
    if (fork) {
        if (!ctx->ev_fork) {
            HIP_OK(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
            for (int q = 0; q < emgpu_ctx::kSide; q++) {
                HIP_OK(hipStreamCreateWithFlags(&ctx->side[q], hipStreamNonBlocking));
                HIP_OK(hipEventCreateWithFlags(&ctx->ev_join[q], hipEventDisableTiming));
            }
        }
        HIP_OK(hipEventRecord(ctx->ev_fork, ctx->stream));
    }
    for (int g = 0; g < (int)launches.size(); g++) {
        hipStream_t st = ctx->stream;
        if (fork) {
            const int lane = g % (emgpu_ctx::kSide + 1);
            if (lane > 0) {
                st = ctx->side[lane - 1];
                if (lane > used) { HIP_OK(hipStreamWaitEvent(st, ctx->ev_fork, 0)); used = lane; }
            }
        }
        const Launch &G = launches[g];
        if (G.members.size() == 1) { launch_dbn(ctx, *live[G.members[0]].u, live[G.members[0]].A, st); continue; }
        // one launch for the group: the call's run with the outputs at column 0, the blocks as (plan, index range, column)
        const void *planf[EMGPU_MAX_MIXED];
        uint64_t first[EMGPU_MAX_MIXED];
        int64_t nn[EMGPU_MAX_MIXED], col[EMGPU_MAX_MIXED];
        for (size_t q = 0; q < G.members.size(); q++) {
            const Live &L = live[G.members[q]];
            planf[q] = L.u->d_planf; first[q] = L.A.first_index; nn[q] = L.A.n; col[q] = L.col;
        }
        const Live &L0 = live[G.members[0]];
        EmgpuRun A = L0.A;
        emgpu_sample_params q0 = *p;
        q0.n = L0.A.n;   // bind_outputs checks col + n against ld: column 0 with the first member's n always fits
        bind_outputs(A, models[0]->m, &q0, &o, 0);
        A.ld = L0.A.ld;
        hipError_t e = emgpu::launch_uncor_fast_mixed(A, (int)G.members.size(), planf, first, nn, col, G.shape, st);
        ctx->last_kernel = emgpu::uncor_fast_mixed_name(G.shape);
        ctx->last_launches++;
        launch_ok(e);
    }
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_sample_dbn_multi_device(emgpu_ctx *const *ctxs, int32_t n_ctx, const emgpu_model *h,
                                  const emgpu_sample_params *p, const emgpu_sample_out *outs) {
    EMGPU_TRY
    if (!ctxs || n_ctx < 1 || !h || !p || !outs) return fail(EMGPU_ERR_ARG, "null argument");
    for (int d = 0; d < n_ctx; d++) if (!ctxs[d]) return fail(EMGPU_ERR_ARG, "null ctx");
    return on_devices(n_ctx, [&](int d) {
        int64_t lo;
        // (device pointers valid on every device: managed / peer memory is the caller's business; outs[d].log_weight is the shard's own)
        const emgpu_sample_params q = shard_params(p, h, d, n_ctx, &lo);
        return emgpu_sample_dbn_device(ctxs[d], h, &q, &outs[d]);
    });
    EMGPU_CATCH
}

int emgpu_sample_dbn_multi_host(emgpu_ctx *const *ctxs, int32_t n_ctx, const emgpu_model *h,
                                const emgpu_sample_params *p, const emgpu_sample_out *out) {
    EMGPU_TRY
    if (!ctxs || n_ctx < 1 || !h || !p || !out) return fail(EMGPU_ERR_ARG, "null argument");
    for (int d = 0; d < n_ctx; d++) if (!ctxs[d]) return fail(EMGPU_ERR_ARG, "null ctx");
    if (p->n < 0) return fail(EMGPU_ERR_ARG, "n < 0");
    return on_devices(n_ctx, [&](int d) {
        int64_t lo;
        const emgpu_sample_params q = shard_params(p, h, d, n_ctx, &lo);   // (host lists: the shard uploads its own entries)
        emgpu_sample_out o = *out;
        o.ld = out->ld ? out->ld : p->n;
        o.col_offset = out->col_offset + lo;
        if (out->log_weight) o.log_weight = out->log_weight + lo;
        return emgpu_sample_dbn_host(ctxs[d], h, &q, &o);
    });
    EMGPU_CATCH
}

// (emgpu_sample_dbn_host: emgpu_host.cpp; the trace pool and the pinned pool: emgpu_memory.cpp)

int emgpu_sample_bn_device(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_bn_params *p, uint8_t *out_bin, float *out_val, int32_t *attempts) {
    EMGPU_TRY
    if (!ctx || !h || !p) return fail(EMGPU_ERR_ARG, "null argument");
    CTX_DEVICE(ctx);
    Uploaded &u = get_uploaded(ctx, h);
    EmgpuBnRun A;
    fill_bn(ctx, u, h->m, p, A);
    A.out_bin = out_bin; A.out_val = out_val; A.attempts = attempts;
    if (A.log_weight) { ensure_logp(ctx, u, h->m); A.logp = u.d_logp; memcpy(A.lp_off, u.lp_off, sizeof A.lp_off); }
    launch_named(ctx, [&](const char **name) { return emgpu::launch_bn(u.cp.plan, A, ctx->stream, name); });
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_sample_bn_host(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_bn_params *p, uint8_t *out_bin, float *out_val, int32_t *attempts) {
    EMGPU_TRY
    if (!ctx || !h || !p) return fail(EMGPU_ERR_ARG, "null argument");
    CTX_DEVICE(ctx);
    const size_t n = (size_t)(p->n > 0 ? p->n : 0), ni = h->m.n_initial;
    CallBuffers b(ctx);
    uint8_t *db = out_bin ? b.alloc<uint8_t>(ni * n + 1) : nullptr;
    float *dv = out_val ? b.alloc<float>(ni * n * 4 + 4) : nullptr;
    int32_t *da = attempts ? b.alloc<int32_t>(n * 4 + 4) : nullptr;
    emgpu_bn_params pd = *p;
    if (p->start && n) pd.start = b.copy_of(p->start, n * ni * 4);
    if (p->log_weight) pd.log_weight = b.alloc<double>(n * 8 + 8);
    int rc = emgpu_sample_bn_device(ctx, h, &pd, db, dv, da);
    if (rc == EMGPU_OK) {
        b.down(p->log_weight, pd.log_weight, n * 8);
        b.down(out_bin, db, ni * n);
        b.down(out_val, dv, ni * n * 4);
        b.down(attempts, da, n * 4);
        rc = emgpu_ctx_sync(ctx);
    }
    return rc;
    EMGPU_CATCH
}

} // extern "C"
