// emgpu_terminal.cpp -- the terminal model: the trajectory models' tables, the encounter chain (geometry draw, createEncounter,
// PropagateTrajectory, local_smooth) and the entry points that run it once or in rejection rounds.
#include <hip/hip_runtime.h>

#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "emgpu_internal.hpp"
#include "emgpu_rounds.hpp"

// Upload / validate the trajectory models of a terminal call and publish their table pointers in ctx->d_thr_base.
// Returns the first model's uploaded plan (the shapes every model shares).
static uint32_t rel_piv(const EmgpuPlan &P, int k) { return P.d_pivoff[k] ? P.d_pivoff[k] - P.d_off[0] : 0u; } // pivot rows relative to the first dynamic table
static uint32_t rel_c8(const EmgpuPlan &P, int k) { return P.d_c8off[k] ? P.d_c8off[k] - P.d_off[0] : 0u; }     // compact rows likewise
static const Uploaded *terminal_tables(emgpu_ctx *ctx, const emgpu_model *const *models, int32_t n_models, const std::set<uint64_t> *also_pinned = nullptr) {
    std::vector<const uint32_t *> bases;
    const Uploaded *first = nullptr;
    std::set<uint64_t> pinned; // the table pointers collected below must survive the cache's LRU sweep
    if (also_pinned) pinned = *also_pinned;
    for (int i = 0; i < n_models; i++) {
        if (!models[i]) throw Error(EMGPU_ERR_ARG, "null model");
        pinned.insert(models[i]->m.uid);
    }
    for (int i = 0; i < n_models; i++) {
        Uploaded &u = get_uploaded(ctx, models[i], &pinned);
        const EmgpuPlan &P = u.cp.plan;
        if (P.ni != 6 || P.nd != 3 || P.depend) throw Error(EMGPU_ERR_UNSUPPORTED, "trajectory model must have 6 initial and 3 independent dynamic variables");
        for (int q = 0; q < 6; q++)
            if (P.i_var[q] != q) throw Error(EMGPU_ERR_UNSUPPORTED, "trajectory model initial network must be in index order");
        {   // createEncounter.m:93-265 propagates heading, altitude and speed (variables 4, 5, 6): the kernel handles them by name
            bool seen[3] = {false, false, false};
            for (int k = 0; k < 3; k++)
                if (P.d_ivar[k] >= 3 && P.d_ivar[k] <= 5) seen[P.d_ivar[k] - 3] = true;
            if (!(seen[0] && seen[1] && seen[2])) throw Error(EMGPU_ERR_UNSUPPORTED, "trajectory model: the dynamic variables must be heading, altitude and speed (variables 4, 5, 6)");
        }
        if (P.d_ivar[0] > 5 || P.i_nb[1] < 3 || P.i_nb[2] < 3 || P.i_nb[3] < 3 || P.i_nb[4] < 3 || P.i_nb[5] < 3)
            throw Error(EMGPU_ERR_UNSUPPORTED, "distance, bearing, heading, altitude and speed need boundaries");
        if (P.i_nb[1] > 66 || P.i_nb[2] > 66 || P.i_nb[3] > 66 || P.i_nb[4] > 66 || P.i_nb[5] > 66)
            throw Error(EMGPU_ERR_UNSUPPORTED, "more than 64 cut points in a trajectory-model variable");
        if (!first) first = &u;
        else {
            const EmgpuPlan &Q = first->cp.plan;
            // the initial networks may differ (2 or 3 intents): only the dynamic tables' relative layout must agree
            bool same = (P.d_off[1] - P.d_off[0]) == (Q.d_off[1] - Q.d_off[0]) && (P.d_off[2] - P.d_off[0]) == (Q.d_off[2] - Q.d_off[0]) &&
                        memcmp(P.d_r, Q.d_r, sizeof P.d_r) == 0 && rel_piv(P, 0) == rel_piv(Q, 0) && rel_piv(P, 1) == rel_piv(Q, 1) && rel_piv(P, 2) == rel_piv(Q, 2) &&
                        rel_c8(P, 0) == rel_c8(Q, 0) && rel_c8(P, 1) == rel_c8(Q, 1) && rel_c8(P, 2) == rel_c8(Q, 2) &&
                        memcmp(P.d_stride_static, Q.d_stride_static, sizeof P.d_stride_static) == 0 &&
                        memcmp(P.d_stride_cur, Q.d_stride_cur, sizeof P.d_stride_cur) == 0 && u.cp.bnd == first->cp.bnd && memcmp(P.i_boff, Q.i_boff, sizeof P.i_boff) == 0 &&
                        memcmp(P.d_ivar, Q.d_ivar, sizeof P.d_ivar) == 0 && memcmp(P.d_tvar, Q.d_tvar, sizeof P.d_tvar) == 0;
            if (!same) throw Error(EMGPU_ERR_UNSUPPORTED, "trajectory models differ in shape or boundaries");
        }
        bases.push_back(u.d_thr + P.d_off[0]); // tables of the dynamic variables, relative to the first one
    }
    first = &get_uploaded(ctx, models[0], &pinned); // std::map keeps references valid and nothing pinned was erased
    ctx_grow(ctx, (void **)&ctx->d_thr_base, &ctx->d_thr_base_cap, bases.size() * sizeof(void *), bases.size() * sizeof(void *));
    HIP_OK(hipMemcpyAsync(ctx->d_thr_base, bases.data(), bases.size() * sizeof(void *), hipMemcpyHostToDevice, ctx->stream));
    HIP_OK(hipStreamSynchronize(ctx->stream));
    return first;
}

// One terminal encounter chain for `count` encounters: geometry draw (sample.m:29-77) -> createEncounter.m:21-49 -> PropagateTrajectory x 4
// (:52-72) -> local_smooth (:88-89) under EMGPU_FLAG_LOCAL_SMOOTH.  geom == null: geo and model_of are the caller's, and only the
// propagate + smooth tail runs (emgpu_propagate_terminal_device).
struct TerminalChain {
    const Model *gm; const Uploaded *geom;   // the geometry model and its upload
    const Uploaded *first;                   // the trajectory tables terminal_tables published in ctx->d_thr_base
    uint64_t seed, first_index;
    int64_t count;
    const uint64_t *indices;                 // the encounters' global indices (a later rejection round), or null: first_index + lane
    int quiet;                               // a re-draw cap voids the track without raising the ctx status
    int32_t max_attempts; const double *bounds_sample; const int32_t *idx; const double (*dyn_limits)[5];
    double tmax_s; int32_t max_resample, cap; uint32_t flags;
    uint8_t *geom_bin; float *geom_val; int32_t *attempts;   // the accepted geometry sample [n_i][count]
    const double *geo_in; const int32_t *model_of_in;        // geom == null: the tail's inputs
    double *geo; int32_t *model_of; float *traj; int32_t *rows;
};
// the geometry model and the ten trajectory models of a chain, uploaded, and the trajectory tables published
static void upload_terminal(emgpu_ctx *ctx, const emgpu_model *gm, const emgpu_model *const *traj_models, int32_t n_traj_models, TerminalChain &c) {
    std::set<uint64_t> pinned{gm->m.uid};   // the trajectory tables' pointers are published before the geometry model's upload
    for (int i = 0; i < n_traj_models; i++) if (traj_models[i]) pinned.insert(traj_models[i]->m.uid);
    c.first = terminal_tables(ctx, traj_models, n_traj_models, &pinned);
    c.gm = &gm->m; c.geom = &get_uploaded(ctx, gm, &pinned);
}
// what a chain takes from either parameter struct of a sampled call (their fields share their names); seed, count and cap are the caller's
template <typename Params> static void chain_params(TerminalChain &c, const Params *p) {
    c.first_index = p->first_index;
    c.max_attempts = p->max_attempts; c.bounds_sample = p->bounds_sample; c.idx = p->idx; c.dyn_limits = p->dyn_limits;
    c.tmax_s = p->tmax_s; c.max_resample = p->max_resample; c.flags = p->flags;
}
// what both sampled entry points refuse in the same words, behind the checks each has alone
static int terminal_models_ok(const emgpu_model *gm, int32_t n_traj_models, const int32_t idx[12]) {
    if (n_traj_models != 10) return fail(EMGPU_ERR_ARG, "the terminal model has 10 trajectory models (CorTerminalModel.m:84-100)");
    for (int k = 0; k < 12; k++) if (idx[k] < 1 || idx[k] > gm->m.n_initial) return fail(EMGPU_ERR_ARG, "geometry variable index out of range");
    return EMGPU_OK;
}
// the limits and thresholds of the filters (track.m:14-17, getDynamicLimits.m), from either parameter struct that carries them
template <typename Params> static void filter_thresholds(EmgpuTFilterRun &F, const Params *p) {
    memcpy(F.dl, p->dyn_limits, sizeof F.dl);
    for (int a = 0; a < 2; a++) { F.max_cum_turn[a] = p->max_cum_turn_deg[a]; F.pitch[a] = p->pitch_deg[a]; }
    F.min_enc_time_s = p->min_enc_time_s; F.thres_dist_ft = p->thres_dist_ft; F.thres_alt_low_ft = p->thres_alt_low_ft; F.thres_vertrate_ft_s = p->thres_vertrate_ft_s;
}
struct TerminalNames { const char *bn = "", *propagate = "", *smooth = ""; };   // what ran (smooth: " + k_terminal_smooth" or nothing)
static TerminalNames terminal_chain(emgpu_ctx *ctx, const TerminalChain &c) {
    // k_terminal_smooth keeps a track's block in one workgroup's registers: refused before anything is launched
    if ((c.flags & EMGPU_FLAG_LOCAL_SMOOTH) && EMGPU_TERMINAL_BLOCK_ROWS(c.cap) > 256) throw Error(EMGPU_ERR_UNSUPPORTED, "EMGPU_FLAG_LOCAL_SMOOTH: cap above 128");
    TerminalNames ran;
    if (c.geom) {
        emgpu_bn_params bp;
        memset(&bp, 0, sizeof bp);
        bp.seed = c.seed; bp.first_index = c.first_index; bp.n = c.count;
        bp.max_attempts = c.max_attempts; bp.bounds_sample = c.bounds_sample;
        bp.idx_own_speed = c.idx[3]; bp.idx_int_speed = c.idx[9];
        bp.min_vel1 = c.dyn_limits[0][0]; bp.max_vel1 = c.dyn_limits[0][1]; bp.min_vel2 = c.dyn_limits[1][0]; bp.max_vel2 = c.dyn_limits[1][1];
        EmgpuBnRun B;
        fill_bn(ctx, *c.geom, *c.gm, &bp, B);
        B.out_bin = c.geom_bin; B.out_val = c.geom_val; B.attempts = c.attempts; B.indices = c.indices;
        launch_ok(emgpu::launch_bn(c.geom->cp.plan, B, ctx->stream, &ran.bn));
        EmgpuTGeoRun G;
        memset(&G, 0, sizeof G);
        G.n = c.count; G.val = c.geom_val; G.geo = c.geo; G.model_of = c.model_of;
        for (int k = 0; k < 12; k++) G.idx[k] = c.idx[k] - 1;
        launch_ok(emgpu::launch_terminal_geo(G, ctx->stream));
    }
    EmgpuTermRun A;
    memset(&A, 0, sizeof A);
    A.seed = c.seed; A.first_index = c.first_index; A.n = c.count; A.thr_base = ctx->d_thr_base;
    A.geo = c.geom ? c.geo : c.geo_in; A.model_of = c.geom ? c.model_of : c.model_of_in;
    A.tmax_s = c.tmax_s; A.max_resample = c.max_resample; A.cap = c.cap; A.indices = c.indices; A.quiet = c.quiet;
    memcpy(A.dl, c.dyn_limits, sizeof A.dl);
    A.traj = c.traj; A.rows = c.rows; A.status = ctx->d_status; A.queue = ctx->d_queue;
    launch_ok(emgpu::launch_terminal_propagate(c.first->cp.plan, A, ctx->stream, &ran.propagate));
    if (c.flags & EMGPU_FLAG_LOCAL_SMOOTH) {
        launch_ok(emgpu::launch_terminal_smooth(c.traj, c.rows, 2 * c.count, c.cap, ctx->stream));
        ran.smooth = " + k_terminal_smooth";
    }
    return ran;
}

extern "C" {

int emgpu_propagate_terminal_device(emgpu_ctx *ctx, const emgpu_model *const *models, int32_t n_models,
                                    const emgpu_term_params *p, const double *geo, const int32_t *model_of,
                                    float *traj, int32_t *rows) {
    EMGPU_TRY
    if (!ctx || !models || n_models < 1 || !p || !geo || !model_of || !traj || !rows) return fail(EMGPU_ERR_ARG, "null argument");
    if (p->n < 0 || p->cap < 2 || p->max_resample < 1) return fail(EMGPU_ERR_ARG, "bad n / cap / max_resample");
    if (p->n >= ((int64_t)1 << 29)) return fail(EMGPU_ERR_ARG, "more than 2^29 encounters in one call");
    CTX_DEVICE(ctx);
    TerminalChain c{};
    c.first = terminal_tables(ctx, models, n_models);
    c.seed = p->seed; c.first_index = p->first_index; c.count = p->n;
    c.dyn_limits = p->dyn_limits; c.tmax_s = p->tmax_s; c.max_resample = p->max_resample; c.cap = p->cap; c.flags = p->flags;
    c.geo_in = geo; c.model_of_in = model_of; c.traj = traj; c.rows = rows;
    const TerminalNames ran = terminal_chain(ctx, c);
    ctx->last_kernel = std::string(ran.propagate) + ran.smooth;
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_propagate_terminal_host(emgpu_ctx *ctx, const emgpu_model *const *models, int32_t n_models,
                                  const emgpu_term_params *p, const double *geo, const int32_t *model_of,
                                  float *out, int32_t *rows) {
    EMGPU_TRY
    if (!ctx || !p || !geo || !model_of || !out || !rows) return fail(EMGPU_ERR_ARG, "null argument");
    if (p->cap < 2) return fail(EMGPU_ERR_ARG, "bad cap");
    const size_t out_bytes = (size_t)(p->n > 0 ? p->n : 0) * 2 * (size_t)EMGPU_TERMINAL_BLOCK_ROWS(p->cap) * 5 * sizeof(float);
    CTX_DEVICE(ctx);
    const size_t n = (size_t)(p->n > 0 ? p->n : 0), nl = 4 * n;
    CallBuffers b(ctx);
    double *dg = b.alloc<double>(n * 12 * sizeof(double) + 8);
    int32_t *dm = b.alloc<int32_t>(nl * 4 + 4), *dr = b.alloc<int32_t>(nl * 4 + 4);
    float *dout = b.alloc<float>(out_bytes + 4);
    b.up(dg, geo, n * 12 * sizeof(double));
    b.up(dm, model_of, nl * 4);
    if (n) HIP_OK(hipMemsetAsync(dout, 0, out_bytes, ctx->stream));
    int rc = emgpu_propagate_terminal_device(ctx, models, n_models, p, dg, dm, dout, dr);
    if (rc == EMGPU_OK) {
        b.down(out, dout, out_bytes);
        b.down(rows, dr, nl * 4);
        rc = emgpu_ctx_sync(ctx);
    }
    return rc;
    EMGPU_CATCH
}

int emgpu_sample_terminal_device(emgpu_ctx *ctx, const emgpu_model *gm, const emgpu_model *const *traj_models, int32_t n_traj_models,
                                 const emgpu_tsample_params *p, uint8_t *geom_bin, float *geom_val, double *geo, int32_t *model_of,
                                 float *traj, int32_t *rows, int32_t *attempts) {
    EMGPU_TRY
    if (!ctx || !gm || !traj_models || !p || !geom_val || !geo || !model_of || !traj || !rows) return fail(EMGPU_ERR_ARG, "null argument");
    if (p->n < 0 || p->cap < 2 || p->max_resample < 1 || p->max_attempts < 1) return fail(EMGPU_ERR_ARG, "bad n / cap / max_resample / max_attempts");
    if (p->n >= ((int64_t)1 << 29)) return fail(EMGPU_ERR_ARG, "more than 2^29 encounters in one call");
    if (int rc = terminal_models_ok(gm, n_traj_models, p->idx)) return rc;
    CTX_DEVICE(ctx);
    if (p->n == 0) return EMGPU_OK;
    TerminalChain c{};
    upload_terminal(ctx, gm, traj_models, n_traj_models, c);
    chain_params(c, p);
    c.seed = p->seed; c.count = p->n; c.cap = p->cap;
    c.geom_bin = geom_bin; c.geom_val = geom_val; c.attempts = attempts; c.geo = geo; c.model_of = model_of; c.traj = traj; c.rows = rows;
    const TerminalNames ran = terminal_chain(ctx, c);
    ctx->last_kernel = std::string(ran.bn) + " + k_terminal_geo" + ran.smooth + " + " + ran.propagate;   // (the dominant kernel stays last in the list)
    ctx->last_launches = *ran.smooth ? 4 : 3;
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_track_terminal_host(emgpu_ctx *ctx, const emgpu_model *gm, const emgpu_model *const *traj_models, int32_t n_traj_models,
                              const emgpu_ttrack_params *p, double *sample, double *traj, int32_t cap2, int32_t *len,
                              double *meta, int32_t *attempts) {
    EMGPU_TRY
    if (!ctx || !gm || !traj_models || !p) return fail(EMGPU_ERR_ARG, "null argument");
    if (p->n < 0 || p->max_resample < 1 || p->max_track_attempts < 1 || p->max_attempts < 1 || !(p->tmax_s >= 1) || (traj && cap2 < 2))
        return fail(EMGPU_ERR_ARG, "bad n / caps / tmax_s");
    // CheckCumTurn (CorTerminalModel.m:135-185) keeps the merged track's heading differences per lane: 2 (tmax_s + 3) - 2 <= 248
    if (p->tmax_s > 122) return fail(EMGPU_ERR_UNSUPPORTED, "tmax_s > 122 (the reference default is 120)");
    if (int rc = terminal_models_ok(gm, n_traj_models, p->idx)) return rc;
    CTX_DEVICE(ctx);
    const size_t n = (size_t)p->n, ni = (size_t)gm->m.n_initial;
    if (n == 0) return EMGPU_OK;
    const int cap = (int)p->tmax_s + 3;
    RoundScratch mem(ctx);
    float *d_val = mem.alloc<float>(ni * n * 4);
    double *d_geo = mem.alloc<double>(n * 12 * 8);
    int32_t *d_mo = mem.alloc<int32_t>(4 * n * 4), *d_rows = mem.alloc<int32_t>(4 * n * 4);
    float *d_out = mem.alloc<float>((size_t)2 * n * (size_t)EMGPU_TERMINAL_BLOCK_ROWS(cap) * 5 * 4);
    RejectionRounds rounds(ctx, mem, n, p->first_index, p->max_track_attempts);
    double *d_sample = sample ? mem.alloc<double>(n * ni * 8) : nullptr;
    double *d_traj = traj ? mem.alloc<double>(n * 2 * (size_t)cap2 * 6 * 8) : nullptr;
    int32_t *d_len = len ? mem.alloc<int32_t>(n * 2 * 4) : nullptr;
    double *d_meta = meta ? mem.alloc<double>(n * 4 * 8) : nullptr;
    int32_t *d_att = mem.alloc<int32_t>(n * 4);
    TerminalChain c{};
    upload_terminal(ctx, gm, traj_models, n_traj_models, c);
    chain_params(c, p);   // (flags: smoothed, the filters read the smoothed speed and altitude)
    c.quiet = 1; c.cap = cap;
    c.geom_val = d_val; c.geo = d_geo; c.model_of = d_mo; c.traj = d_out; c.rows = d_rows;
    // the filters (track.m:62-145)
    EmgpuTFilterRun F;
    memset(&F, 0, sizeof F);
    F.tracks = d_out; F.rows = d_rows; F.cap = cap; F.geo = d_geo; F.val = d_val; F.n_i = (int32_t)ni;
    filter_thresholds(F, p);
    F.accepted = rounds.accepted();
    F.sample = d_sample; F.traj = d_traj; F.cap2 = cap2; F.len = d_len; F.meta = d_meta; F.attempts = d_att;
    for (; rounds.more(); rounds.next()) {
        c.seed = p->seed + (uint64_t)rounds.round(); c.count = (int64_t)rounds.count(); c.indices = rounds.indices();
        const TerminalNames ran = terminal_chain(ctx, c);
        F.n = c.count; F.slot = rounds.slots(); F.attempt_no = rounds.attempt_no(); F.last_round = rounds.last_round();
        const char *name = "";
        launch_ok(emgpu::launch_terminal_filter(F, ctx->stream, &name));
        ctx->last_kernel = std::string(ran.bn) + " + " + ran.propagate + ran.smooth + " + " + name;
    }
    return copy_back_accepted(ctx, rounds.status("terminal track", "encounters"), [&] {
        auto back = [&](void *dst, const void *src, size_t bytes) { if (dst && bytes) HIP_OK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream)); };
        back(sample, d_sample, n * ni * 8); back(traj, d_traj, n * 2 * (size_t)cap2 * 6 * 8); back(len, d_len, n * 2 * 4);
        back(meta, d_meta, n * 4 * 8); back(attempts, d_att, n * 4);
    });
    EMGPU_CATCH
}

// The two kernels behind the propagation on tracks of the caller's: no context and no model, like the paired-tracks entry points (they
// need no table, no scratch and no status word), so they run on the stream given and on the calling thread's current device.
int emgpu_filter_terminal_device(void *hip_stream, const emgpu_tfilter_params *p, const double *geo, const float *tracks, const int32_t *rows,
                                 uint8_t *accepted, double *meta, int32_t *len, double *traj) {
    EMGPU_TRY
    if (!p) return fail(EMGPU_ERR_ARG, "null argument: p");
    if (!geo) return fail(EMGPU_ERR_ARG, "null argument: geo");
    if (!tracks) return fail(EMGPU_ERR_ARG, "null argument: tracks");
    if (!rows) return fail(EMGPU_ERR_ARG, "null argument: rows");
    if (!accepted) return fail(EMGPU_ERR_ARG, "null argument: accepted");
    if (p->n < 0 || p->n >= ((int64_t)1 << 29)) return fail(EMGPU_ERR_ARG, "n outside 0..2^29-1");
    // CheckCumTurn keeps a joined track's heading differences per lane: rf + rb - 2 <= 2 cap - 2 <= 248 (emgpu_track_terminal_host: tmax_s <= 122)
    if (p->cap < 2 || p->cap > 125) return fail(EMGPU_ERR_UNSUPPORTED, "cap outside 2..125");
    if (traj && p->cap2 < 1) return fail(EMGPU_ERR_ARG, "traj with cap2 < 1");
    if (((uintptr_t)geo | (uintptr_t)meta | (uintptr_t)traj) & 7u) return fail(EMGPU_ERR_ARG, "geo, meta and traj must be 8-byte aligned");
    if (((uintptr_t)tracks | (uintptr_t)rows | (uintptr_t)len) & 3u) return fail(EMGPU_ERR_ARG, "tracks, rows and len must be 4-byte aligned");
    if (p->n == 0) return EMGPU_OK;
    EmgpuTFilterRun F;
    memset(&F, 0, sizeof F);
    F.n = p->n; F.tracks = tracks; F.rows = rows; F.cap = p->cap; F.geo = geo;
    filter_thresholds(F, p);
    F.accepted = accepted; F.traj = traj; F.cap2 = p->cap2; F.len = len; F.meta = meta;
    const char *name = "";
    launch_ok(emgpu::launch_terminal_filter(F, (hipStream_t)hip_stream, &name));
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_smooth_terminal_device(void *hip_stream, int64_t n2, int32_t cap, float *tracks, const int32_t *rows) {
    EMGPU_TRY
    if (!tracks) return fail(EMGPU_ERR_ARG, "null argument: tracks");
    if (!rows) return fail(EMGPU_ERR_ARG, "null argument: rows");
    if (n2 < 0 || n2 >= ((int64_t)1 << 30)) return fail(EMGPU_ERR_ARG, "n2 outside 0..2^30-1");
    if (cap < 2) return fail(EMGPU_ERR_ARG, "cap < 2");
    // k_terminal_smooth keeps a track's block in one workgroup's LDS tile of 256 rows
    if (EMGPU_TERMINAL_BLOCK_ROWS(cap) > 256) return fail(EMGPU_ERR_UNSUPPORTED, "cap above 128");
    if (((uintptr_t)tracks | (uintptr_t)rows) & 3u) return fail(EMGPU_ERR_ARG, "tracks and rows must be 4-byte aligned");
    if (n2 == 0) return EMGPU_OK;
    launch_ok(emgpu::launch_terminal_smooth(tracks, rows, n2, cap, (hipStream_t)hip_stream));
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_debug_terminal_counters(emgpu_ctx *ctx, uint64_t *out, int32_t n) {
    EMGPU_TRY
    if (!ctx || !out || n < 1) return fail(EMGPU_ERR_ARG, "null argument");
    CTX_DEVICE(ctx);
    HIP_OK(hipStreamSynchronize(ctx->stream));
    const int rc = emgpu::terminal_debug_counters((unsigned long long *)out, n);
    if (rc < 0) return fail(EMGPU_ERR_HIP, "reading the counters failed");
    return rc;
    EMGPU_CATCH
}

} // extern "C"
