// emgpu_track.cpp -- tracks from samples: sample2track on device and host arrays, and the uncorrelated model's track driver (its dynamic
// limits, its rejection rounds, the entry points around them and the test hook of its point-mass step).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "emgpu_internal.hpp"
#include "emgpu_rounds.hpp"

extern "C" {

static int track_params_ok(const emgpu_track_params *p) {
    if (p->n < 0 || p->T < 1) return fail(EMGPU_ERR_ARG, "bad n / T");
    return EMGPU_OK;
}

int emgpu_sample2track_device(emgpu_ctx *ctx, const emgpu_track_params *p, const float *alt0, const float *speed0,
                              const float *dyn_val, double *xyz, uint8_t *flags, double *speed_minmax) {
    EMGPU_TRY
    if (!ctx || !p || !alt0 || !speed0 || !dyn_val) return fail(EMGPU_ERR_ARG, "null argument");
    if (int rc = track_params_ok(p)) return rc;
    if (p->nd < 1 || p->slot_vertrate < 0 || p->slot_vertrate >= p->nd || p->slot_acc < 0 || p->slot_acc >= p->nd ||
        p->slot_turnrate < 0 || p->slot_turnrate >= p->nd)
        return fail(EMGPU_ERR_ARG, "bad dense-trace rows");
    CTX_DEVICE(ctx);
    EmgpuTrackRun A{};
    A.n = p->n; A.T = p->T;
    set_track_units(A, p);
    A.alt0_f = alt0; A.speed0_f = speed0; A.dyn_val = dyn_val;
    A.nd = p->nd; A.s_vr = p->slot_vertrate; A.s_acc = p->slot_acc; A.s_tr = p->slot_turnrate;
    A.xyz = xyz; A.flags = flags; A.vmm = speed_minmax;
    launch_named(ctx, [&](const char **name) { return emgpu::launch_sample2track(A, true, ctx->stream, name); });
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_sample2track_host(emgpu_ctx *ctx, const emgpu_track_params *p, const double *alt0, const double *speed0,
                            const double *updates, double *xyz, uint8_t *flags, double *speed_minmax) {
    EMGPU_TRY
    if (!ctx || !p || !alt0 || !speed0 || !updates) return fail(EMGPU_ERR_ARG, "null argument");
    if (int rc = track_params_ok(p)) return rc;
    CTX_DEVICE(ctx);
    const size_t n = (size_t)p->n, T = (size_t)p->T;
    if (n == 0) return EMGPU_OK;
    // [n][T][3] -> [T][3][n] so that a wave reads 64 consecutive doubles
    std::vector<double> planar(T * 3 * n), hx, hv;   // (before the buffers: their copy-backs land here until the buffers' destructor syncs)
    for (size_t i = 0; i < n; i++)
        for (size_t t = 0; t < T; t++)
            for (size_t c = 0; c < 3; c++) planar[(t * 3 + c) * n + i] = updates[(i * T + t) * 3 + c];
    CallBuffers b(ctx);
    double *d_in = b.alloc<double>((planar.size() + 2 * n) * sizeof(double));
    double *d_xyz = b.alloc<double>((T + 1) * 3 * n * sizeof(double)), *d_vmm = b.alloc<double>(2 * n * sizeof(double));
    uint8_t *d_fl = b.alloc<uint8_t>(n);
    b.up(d_in, planar.data(), planar.size() * sizeof(double));
    b.up(d_in + planar.size(), alt0, n * sizeof(double));
    b.up(d_in + planar.size() + n, speed0, n * sizeof(double));
    EmgpuTrackRun A{};
    A.n = p->n; A.T = p->T;
    set_track_units(A, p);
    A.upd = d_in; A.alt0_d = d_in + planar.size(); A.speed0_d = d_in + planar.size() + n;
    A.xyz = d_xyz; A.flags = d_fl; A.vmm = d_vmm;
    launch_named(ctx, [&](const char **name) { return emgpu::launch_sample2track(A, false, ctx->stream, name); });
    if (xyz) { hx.resize((T + 1) * 3 * n); b.down(hx.data(), d_xyz, hx.size() * sizeof(double)); }
    b.down(flags, d_fl, n);
    if (speed_minmax) { hv.resize(2 * n); b.down(hv.data(), d_vmm, hv.size() * sizeof(double)); }
    const int rc = emgpu_ctx_sync(ctx);
    if (rc == EMGPU_OK && xyz)
        for (size_t i = 0; i < n; i++)
            for (size_t t = 0; t <= T; t++)
                for (size_t c = 0; c < 3; c++) xyz[(i * (T + 1) + t) * 3 + c] = hx[(t * 3 + c) * n + i];
    if (rc == EMGPU_OK && speed_minmax)
        for (size_t i = 0; i < n; i++) { speed_minmax[2 * i] = hv[i]; speed_minmax[2 * i + 1] = hv[n + i]; }
    return rc;
    EMGPU_CATCH
}

static emgpu::UncorTrackVars track_vars(const emgpu_utrack_params *p) {
    emgpu::UncorTrackVars tv;
    tv.idxG = p->idx_G; tv.idxA = p->idx_A; tv.idxL = p->idx_L; tv.idxV = p->idx_v; tv.idxDV = p->idx_dv; tv.idxDH = p->idx_dh; tv.idxDPsi = p->idx_dpsi;
    tv.is_rotorcraft = p->is_rotorcraft != 0;
    return tv;
}

int emgpu_uncor_dynamic_limits(const emgpu_model *h, const emgpu_utrack_params *vars, const double *initial,
                               double up_min, double up_max, double v_min, double v_max, double out[3]) {
    EMGPU_TRY
    if (!h || !vars || !initial || !out) return fail(EMGPU_ERR_ARG, "null argument");
    const emgpu::UncorLimits L = emgpu::build_uncor_limits(h->m, track_vars(vars));
    const double *e = L.table.data();
    if (L.ordered) {
        auto disc = [](double x, const double *cut, int n) { return (int)emgpu_discretize_bayes(x, cut, n); };
        const int dG = (int)initial[vars->idx_G - 1], dA = (int)initial[vars->idx_A - 1];
        int l0, l1, b0, b1;
        if (L.discL) l0 = l1 = (int)initial[vars->idx_L - 1];
        else { l0 = disc(up_min, L.cutL, L.ncL); l1 = disc(up_max, L.cutL, L.ncL); }
        b0 = disc(v_min * 0.592484, L.cutV, L.ncV); b1 = disc(v_max * 0.592484, L.cutV, L.ncV);
        if (dG < 1 || dG > L.rG || dA < 1 || dA > L.rA || l0 < 1 || l1 > L.rL || l0 > l1 || b0 > b1) return fail(EMGPU_ERR_ARG, "initial values outside the model's bins");
        e += ((((((size_t)(dG - 1) * L.rA + (size_t)(dA - 1)) * L.rL + (size_t)(l0 - 1)) * L.rL + (size_t)(l1 - 1)) * L.rV + (size_t)(b0 - 1)) * L.rV + (size_t)(b1 - 1)) * 3;
    }
    out[0] = e[0]; out[1] = e[1]; out[2] = e[2];
    return EMGPU_OK;
    EMGPU_CATCH
}

// The rounds of UncorEncounterModel.m:419-471 (see the header).  d_*: device outputs (any may be null).
// d_start: the call's start grid [p->n][n_initial] on the device, or null.
static int track_uncor_rounds(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_utrack_params *p, const int32_t *d_start, double *d_tracks, double *d_limits,
                              int32_t *d_attempts) {
    const Model &m = h->m;
    if (p->n < 0 || p->sample_time < 1 || p->sample_time > 65535) throw Error(EMGPU_ERR_ARG, "n < 0 or sample_time outside 1..65535");
    if (p->max_track_attempts < 1 || p->max_attempts < 1 || p->record_stride < 1 || (10 * p->sample_time) % p->record_stride)
        throw Error(EMGPU_ERR_ARG, "max_track_attempts / max_attempts must be >= 1 and record_stride must divide 10 * sample_time");
    const emgpu::UncorTrackVars tv = track_vars(p);
    const std::array<uint64_t, 3> lkey = {m.uid, m.version,
                                          (uint64_t)(uint8_t)tv.idxG | ((uint64_t)(uint8_t)tv.idxA << 8) | ((uint64_t)(uint8_t)tv.idxL << 16) | ((uint64_t)(uint8_t)tv.idxV << 24) |
                                              ((uint64_t)(uint8_t)tv.idxDV << 32) | ((uint64_t)(uint8_t)tv.idxDH << 40) | ((uint64_t)(uint8_t)tv.idxDPsi << 48) | ((uint64_t)tv.is_rotorcraft << 56)};
    if (ctx->limits_cache.size() > 32 && !ctx->limits_cache.count(lkey)) ctx->limits_cache.clear();
    auto lit = ctx->limits_cache.find(lkey);
    if (lit == ctx->limits_cache.end()) lit = ctx->limits_cache.emplace(lkey, emgpu::build_uncor_limits(m, tv)).first;
    const emgpu::UncorLimits &L = lit->second;
    if (m.n_dyn() < 3) throw Error(EMGPU_ERR_ARG, "dynvar:empty: the model needs dynamic variables for acceleration, vertical rate and turn rate");
    auto row_of = [&](int idx) {   // row of the temporal map == row of the dense trace
        for (size_t k = 0; k < m.temporal_map.size(); k++) if (m.temporal_map[k][0] == idx) return (int)k;
        throw Error(EMGPU_ERR_ARG, "dynvar:empty: \\dot v, \\dot h and \\dot \\psi must be dynamic variables");
    };
    const int sDV = row_of(p->idx_dv), sDH = row_of(p->idx_dh), sDPsi = row_of(p->idx_dpsi);
    const size_t n = (size_t)p->n, ni = (size_t)m.n_initial, nd = (size_t)m.n_dyn(), T = (size_t)p->sample_time, G4 = (T + 3) / 4;
    if (n == 0) return EMGPU_OK;
    RoundScratch mem(ctx);
    float *d_iv = mem.alloc<float>(ni * n * 4), *d_dv = mem.alloc<float>(G4 * nd * n * 16);
    double *d_lim = mem.alloc<double>(L.table.size() * 8);
    RejectionRounds rounds(ctx, mem, n, p->first_index, p->max_track_attempts);
    HIP_OK(hipMemcpyAsync(d_lim, L.table.data(), L.table.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_OK(hipStreamSynchronize(ctx->stream)); // L.table is a local
    Uploaded &u = get_uploaded(ctx, h);
    EmgpuUTrackRun R;
    memset(&R, 0, sizeof R);
    R.T = (int32_t)T; R.stride = p->record_stride; R.nd = (int32_t)nd; R.sDV = sDV; R.sDH = sDH; R.sDPsi = sDPsi;
    {   // UncorEncounterModel.m:397-414
        const std::vector<double> &bL = m.boundaries[p->idx_L - 1], &bV = m.boundaries[p->idx_v - 1], &bDH = m.boundaries[p->idx_dh - 1];
        R.min_alt = bL.empty() ? 0.0 : *std::min_element(bL.begin(), bL.end());
        R.max_alt = bL.empty() ? INFINITY : *std::max_element(bL.begin(), bL.end());
        R.dyn[0] = 1.7; R.dyn[1] = *std::max_element(bV.begin(), bV.end()) * 1.68780972222222;
        R.dyn[2] = *std::min_element(bDH.begin(), bDH.end()) / 60.0; R.dyn[3] = *std::max_element(bDH.begin(), bDH.end()) / 60.0;
        R.dyn[4] = 3.0 * (3.14159265358979323846 / 180.0); R.dyn[5] = 1000000.0;
    }
    R.ordered = L.ordered; R.rG = L.rG; R.rA = L.rA; R.rL = L.rL; R.rV = L.rV; R.ncL = L.ncL; R.ncV = L.ncV; R.discL = L.discL; R.discV = L.discV;
    memcpy(R.cutL, L.cutL, sizeof R.cutL); memcpy(R.cutV, L.cutV, sizeof R.cutV);
    R.lim = d_lim; R.tracks = d_tracks; R.S = (int64_t)(10 * T / (size_t)p->record_stride + 1); R.limits = d_limits;
    R.accepted = rounds.accepted(); R.attempts = d_attempts;
    for (; rounds.more(); rounds.next()) {
        const size_t count = rounds.count();
        emgpu_sample_params sp;
        memset(&sp, 0, sizeof sp);
        sp.seed = p->seed + (uint64_t)rounds.round();                     // :428  seed = seed + 1
        sp.first_index = p->first_index; sp.n = (int64_t)count; sp.sample_time = p->sample_time;
        sp.flags = p->flags & EMGPU_FLAG_QUANTIZE500; sp.max_attempts = p->max_attempts;
        sp.idx_L = p->idx_L; sp.idx_v = p->idx_v; sp.idx_dh = p->idx_dh;
        sp.indices = rounds.indices();
        EmgpuRun A;
        fill_run(ctx, u, m, &sp, A);
        A.init_val = d_iv; A.dyn_val = d_dv; A.ld = (int64_t)count;
        // a start grid: round 0 reads row i for lane i, a later round the rows of the trajectories it redraws (its slot list)
        const EmgpuPresets *presets = d_start ? upload_presets(ctx, u, m, d_start, nullptr, rounds.slots()) : nullptr;
        launch_dbn(ctx, u, A, nullptr, presets);                          // :424  self.sample(1, sample_time, 'seed', seed)
        const std::string sampler = ctx->last_kernel;
        R.n = (int64_t)count; R.ld = (int64_t)count;
        auto row = [&](int idx) -> const float * { return idx > 0 ? d_iv + (size_t)(idx - 1) * count : nullptr; };
        R.iG = row(p->idx_G); R.iA = row(p->idx_A); R.iL = row(p->idx_L); R.iV = row(p->idx_v);
        R.iDV = row(p->idx_dv); R.iDH = row(p->idx_dh); R.iDPsi = row(p->idx_dpsi);
        R.dyn_val = d_dv; R.slot = rounds.slots();
        R.attempt_no = rounds.attempt_no(); R.last_round = rounds.last_round();
        const char *name = "";
        launch_ok(emgpu::launch_uncor_track(R, ctx->stream, &name));
        ctx->last_kernel = sampler + " + " + name;
    }
    return rounds.status("track", "trajectories");
}

int emgpu_track_uncor_grid_device(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_utrack_params *p, const int32_t *start, double *tracks, double *limits,
                                  int32_t *attempts) {
    EMGPU_TRY
    if (!ctx || !h || !p) return fail(EMGPU_ERR_ARG, "null argument");
    CTX_DEVICE(ctx);
    return track_uncor_rounds(ctx, h, p, start, tracks, limits, attempts);
    EMGPU_CATCH
}
int emgpu_track_uncor_device(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_utrack_params *p, double *tracks, double *limits, int32_t *attempts) {
    return emgpu_track_uncor_grid_device(ctx, h, p, nullptr, tracks, limits, attempts);
}

int emgpu_track_uncor_host(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_utrack_params *p, double *tracks, double *limits, int32_t *attempts) {
    return emgpu_track_uncor_grid_host(ctx, h, p, nullptr, tracks, limits, attempts);
}
int emgpu_track_uncor_grid_host(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_utrack_params *p, const int32_t *start, double *tracks, double *limits,
                                int32_t *attempts) {
    EMGPU_TRY
    if (!ctx || !h || !p) return fail(EMGPU_ERR_ARG, "null argument");
    CTX_DEVICE(ctx);
    const size_t n = (size_t)(p->n > 0 ? p->n : 0);
    if (p->record_stride < 1 || p->sample_time < 1) return fail(EMGPU_ERR_ARG, "bad record_stride / sample_time");
    const size_t S = (size_t)(10 * p->sample_time / p->record_stride + 1);
    CallBuffers b(ctx);
    double *dt = tracks ? b.alloc<double>(n * S * 8 * sizeof(double) + 8) : nullptr;
    double *dl = limits ? b.alloc<double>(n * 3 * sizeof(double) + 8) : nullptr;
    int32_t *da = b.alloc<int32_t>(n * 4 + 4);
    const int32_t *ds = start && n ? b.copy_of(start, n * (size_t)h->m.n_initial * sizeof(int32_t)) : nullptr;
    return copy_back_accepted(ctx, track_uncor_rounds(ctx, h, p, ds, dt, dl, da), [&] {
        b.down(tracks, dt, n * S * 8 * sizeof(double));
        b.down(limits, dl, n * 3 * sizeof(double));
        b.down(attempts, da, n * 4);
    });
    EMGPU_CATCH
}

// Test hook: k_uncor_track on caller-given initial values and control rows (no sampling, no limits): what the point-mass step does with
// inputs a sampled batch seldom holds (a pitch command clamped to +-90 degrees that changes sign).
int emgpu_debug_uncor_dynamics_host(emgpu_ctx *ctx, int64_t n, int32_t T, int32_t record_stride, int32_t literal, const double dyn[6],
                                    const float *init, const float *controls, double *tracks) {
    EMGPU_TRY
    if (!ctx || !dyn || !init || !controls || !tracks || n < 1 || T < 1 || record_stride < 1 || (10 * T) % record_stride) return fail(EMGPU_ERR_ARG, "bad argument");
    CTX_DEVICE(ctx);
    const size_t G4 = (size_t)(T + 3) / 4, S = (size_t)(10 * T / record_stride + 1);
    std::vector<float> h_init(5 * (size_t)n), h_dyn(G4 * 3 * (size_t)n * 4, 0.f);
    for (int64_t i = 0; i < n; i++) {
        for (int k = 0; k < 5; k++) h_init[(size_t)k * n + i] = init[i * 5 + k];      // rows: L v \dot v \dot h \dot psi
        for (int c = 0; c < T; c++)
            for (int k = 0; k < 3; k++) h_dyn[((((size_t)c / 4) * 3 + k) * n + i) * 4 + c % 4] = controls[((size_t)i * T + c) * 3 + k];   // rows: \dot h, \dot psi, \dot v
    }
    CallBuffers b(ctx);
    float *d_init = b.alloc<float>(h_init.size() * 4), *d_dyn = b.alloc<float>(h_dyn.size() * 4);
    double *d_tr = b.alloc<double>((size_t)n * S * 8 * 8), *d_lim = b.alloc<double>(3 * 8);
    uint8_t *d_acc = b.alloc<uint8_t>((size_t)n);
    const double lim[3] = {-1e300, 1e300, 1e300};
    b.up(d_init, h_init.data(), h_init.size() * 4);
    b.up(d_dyn, h_dyn.data(), h_dyn.size() * 4);
    b.up(d_lim, lim, sizeof lim);
    EmgpuUTrackRun R;
    memset(&R, 0, sizeof R);
    R.n = n; R.ld = n; R.T = T; R.stride = record_stride;
    R.iL = d_init; R.iV = d_init + n; R.iDV = d_init + 2 * n; R.iDH = d_init + 3 * n; R.iDPsi = d_init + 4 * n;
    R.dyn_val = d_dyn; R.nd = 3; R.sDH = 0; R.sDPsi = 1; R.sDV = 2;
    memcpy(R.dyn, dyn, sizeof R.dyn);
    R.min_alt = -1e300; R.max_alt = 1e300; R.ordered = 0; R.lim = d_lim;
    R.tracks = d_tr; R.S = (int64_t)S; R.accepted = d_acc;
    launch_named(ctx, [&](const char **name) { return emgpu::launch_uncor_track(R, ctx->stream, name, literal); });
    b.down(tracks, d_tr, (size_t)n * S * 8 * 8);
    HIP_OK(hipStreamSynchronize(ctx->stream));
    return EMGPU_OK;
    EMGPU_CATCH
}

} // extern "C"
