// emgpu_host.cpp -- the chunked sampling path of the C ABI: emgpu_sample_dbn_host, emgpu_sample_uncor_host (UncorEncounterModel.sample's
// samples and controls built on the device) and emgpu_sample_text_host (em_sample's two text files formatted on the device,
// em_sample.m:85-99).  One driver, run_chunks, pipelines all three -- chunk k's launches | chunk k-1's copy over PCIe | chunk k-2's copy
// into the caller's arrays.  The chunk buffers, the staging buffers and the pinned pool are emgpu_memory.cpp's (emgpu_hostmem.hpp).
// Reference semantics: the loop over samples of UncorEncounterModel.m:244-300 and the host arrays it returns (:283-300).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <system_error>
#include <thread>

#include "emgpu_hostmem.hpp"

using namespace emgpu_detail;

namespace {
int host_threads() {
    static const int n = [] {
        const char *e = getenv("EMGPU_HOST_THREADS");
        int v = e ? atoi(e) : 0;
        if (v < 1) v = (int)std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
        return std::min(v, 64);
    }();
    return n;
}
template <typename F>
void run_parallel(int T, F fn) {   // fn(t) for t = 0..T-1, fn(0) on the calling thread; fn does not throw (memcpy loops)
    std::vector<std::thread> th;
    int started = 1;
    try {
        for (int t = 1; t < T; t++) { th.emplace_back(fn, t); started = t + 1; }
    } catch (const std::system_error &) {}   // the host will not give another thread: the parts not started run here (a joinable thread must not be destroyed)
    fn(0);
    for (int t = started; t < T; t++) fn(t);
    for (auto &x : th) x.join();
}

// ------------------------------------------------------------------------------------------------ the host path's chunked pipeline
struct ChunkPlan { size_t n, C, Cp, nchunks; };   // n trajectories in chunks of C (the last one may be short), C padded to Cp on the device
// `bpt` device bytes per trajectory; chunks of equal size, and with event lists (event_cap > 0: rows per list) or text rows (bytes per
// trajectory at most) a chunk's packed rows / bytes counted in 32 bits
ChunkPlan chunk_plan(size_t n, size_t bpt, bool direct, size_t event_cap) {
    const size_t target = host_chunk_target((size_t)(direct ? 1024 : 256) << 20);   // pinned outputs: larger pieces (the copy engine writes row by row into the caller's pitch)
    size_t C = std::max<size_t>(1024, target / std::max<size_t>(bpt, 1) / 1024 * 1024);
    if (event_cap) C = std::min(C, std::max<size_t>(1024, ((size_t)0xFFFF0000u / event_cap) / 1024 * 1024));
    if (C >= n) C = n;
    else {   // chunks of equal size: the last one is not a sliver (and a staged copy moves whole chunk buffers)
        const size_t k = (n + C - 1) / C;
        C = std::min(C, round_up((n + k - 1) / k, 1024));
    }
    return {n, C, round_up(C, 256), (n + C - 1) / C};
}

// Launch k / drain k-1 over the chunks: launch(k0, c, b) on the ctx stream and copy(k0, c, b) on the copy stream behind it for trajectories
// [k0, k0 + c) in chunk buffer b, then scatter(...) of the chunk before it on the host.  wait_rows: the host waits for the launches before
// copy() (which reads the row counts they left in h_total[2b], h_total[2b + 1]).  Stores the call's host_stats; emgpu_ctx_sync's status.
template <typename Launch, typename Copy, typename Scatter>
int run_chunks(emgpu_ctx *ctx, const ChunkPlan &P, bool direct, bool wait_rows, Clock::time_point t_call, emgpu_host_stats_t &st, Launch launch,
               Copy copy, Scatter scatter) {
    st.chunks = (int32_t)P.nchunks; st.chunk_n = (int32_t)P.C; st.threads = host_threads(); st.direct = direct ? 1 : 0;
    Events ev(8);   // per buffer b: 4b + {kernel start, kernel end, copy start, copy end}
    int rc = EMGPU_OK;
    try {
        for (size_t k = 0; k <= P.nchunks; k++) {
            if (k < P.nchunks) {
                const int b = (int)(k & 1);
                const size_t k0 = k * P.C, c = std::min(P.C, P.n - k0);
                HIP_OK(hipEventRecord(ev[4 * b], ctx->stream));
                launch(k0, c, b);
                HIP_OK(hipEventRecord(ev[4 * b + 1], ctx->stream));
                if (wait_rows) HIP_OK(hipEventSynchronize(ev[4 * b + 1]));   // (the launch stream holds nothing but this chunk)
                HIP_OK(hipStreamWaitEvent(ctx->copy_stream, ev[4 * b + 1], 0));
                HIP_OK(hipEventRecord(ev[4 * b + 2], ctx->copy_stream));
                copy(k0, c, b);
                HIP_OK(hipEventRecord(ev[4 * b + 3], ctx->copy_stream));
            }
            if (k > 0) {
                const int b = (int)((k - 1) & 1);
                const size_t k0 = (k - 1) * P.C, c = std::min(P.C, P.n - k0);
                HIP_OK(hipEventSynchronize(ev[4 * b + 3]));
                float ms = 0.f;
                HIP_OK(hipEventElapsedTime(&ms, ev[4 * b], ev[4 * b + 1])); st.kernel_ms += ms;
                HIP_OK(hipEventElapsedTime(&ms, ev[4 * b + 2], ev[4 * b + 3])); st.d2h_ms += ms;
                const auto t0 = Clock::now();
                scatter(k0, c, b);
                st.scatter_ms += ms_since(t0);
            }
        }
        rc = emgpu_ctx_sync(ctx);   // deferred per-trajectory errors of every chunk (rejection cap, event cap, presets)
    } catch (...) {
        (void)hipStreamSynchronize(ctx->stream);
        if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
        throw;
    }
    st.total_ms = ms_since(t_call);
    ctx->host_stats = st;
    return rc;
}

struct Job { char *dst; const char *src; size_t bytes; };
// the jobs on TT threads (job j on thread j % TT), then more(t) on each thread t
template <typename More>
void run_jobs(const std::vector<Job> &jobs, int TT, More more) {
    run_parallel(TT, [&](int t) {
        for (size_t j = (size_t)t; j < jobs.size(); j += (size_t)TT) memcpy(jobs[j].dst, jobs[j].src, jobs[j].bytes);
        more(t);
    });
}

int sample_nothing(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_sample_params *p) {   // n == 0: the arguments are still checked like any call's
    emgpu_sample_out d{};
    const int rc = emgpu_sample_dbn_device(ctx, h, p, &d);
    ctx->host_stats = emgpu_host_stats_t{};
    return rc == EMGPU_OK ? emgpu_ctx_sync(ctx) : rc;
}
} // namespace

extern "C" {

// ================================================================================================ the host path
// The start grid of a host-pointer call is caller (host) memory: uploaded once into the ctx's scratch, every chunk reads its own rows.
static const int32_t *upload_start_grid(emgpu_ctx *ctx, const int32_t *start, size_t n, size_t ni) {
    int32_t *ds = (int32_t *)ctx_scratch(ctx, 0, n * ni * sizeof(int32_t));
    HIP_OK(hipMemcpyAsync(ds, start, n * ni * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    return ds;
}

int emgpu_sample_dbn_host(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_sample_params *p, const emgpu_sample_out *out) {
    EMGPU_TRY
    if (!ctx || !h || !p || !out) return fail(EMGPU_ERR_ARG, "null argument");
    CTX_DEVICE(ctx);
    const auto t_call = Clock::now();
    const Model &m = h->m;
    const size_t n = (size_t)(p->n > 0 ? p->n : 0), ni = (size_t)m.n_initial, nd = (size_t)m.n_dyn();
    const size_t G4 = ((size_t)(p->sample_time > 0 ? p->sample_time : 0) + 3) / 4;
    // the host arrays may be dimensioned for a larger batch (ld) of which this call fills columns [off, off + n)
    const size_t ld = out->ld ? (size_t)out->ld : n, off = (size_t)out->col_offset;
    if (out->ld < 0 || out->col_offset < 0 || off + n > ld) return fail(EMGPU_ERR_ARG, "col_offset + n exceeds ld");
    if ((out->ev_count != nullptr) != (out->events != nullptr)) return fail(EMGPU_ERR_ARG, "ev_count and events go together");
    if (out->events && p->event_cap < 1) return fail(EMGPU_ERR_ARG, "event_cap must be >= 1");
    const size_t cap = out->events ? (size_t)p->event_cap : 0;
    if (n == 0) return sample_nothing(ctx, h, p);

    // ---- one chunk on the device: [small arrays | large arrays | event lists | packed rows | pack scratch]; what is staged is a prefix
    struct Arr { void *dst; size_t rows, elem, dev_off; bool offset_by_col; };
    std::vector<Arr> small, large;
    const bool direct = (out->init_bin || out->init_val || out->dyn_bin || out->dyn_val) &&
                        (!out->init_bin || is_pinned(out->init_bin)) && (!out->init_val || is_pinned(out->init_val)) &&
                        (!out->dyn_bin || is_pinned(out->dyn_bin)) && (!out->dyn_val || is_pinned(out->dyn_val));
    size_t bpt = 0;   // device bytes per trajectory
    bpt += (out->ev_count ? 4 : 0) + (out->attempts ? 4 : 0) + (out->log_weight ? 8 : 0);
    bpt += (out->init_bin ? ni : 0) + (out->init_val ? 4 * ni : 0);
    bpt += (out->dyn_bin ? 4 * G4 * nd : 0) + (out->dyn_val ? 16 * G4 * nd : 0);
    bpt += 16 * cap;   // the lists and their packed copy
    const ChunkPlan P = chunk_plan(n, bpt, direct, cap);
    const size_t C = P.C, Cp = P.Cp;
    size_t o = 0;
    auto put = [&](size_t bytes) { const size_t at = o; o = round_up(o + bytes, 256); return at; };
    if (out->ev_count) small.push_back({out->ev_count, 1, 4, put(Cp * 4), true});
    if (out->attempts) small.push_back({out->attempts, 1, 4, put(Cp * 4), true});
    if (out->log_weight) small.push_back({out->log_weight, 1, 8, put(Cp * 8), false});
    const size_t small_bytes = o;
    if (out->init_bin) large.push_back({out->init_bin, ni, 1, put(ni * Cp), true});
    if (out->init_val) large.push_back({out->init_val, ni, 4, put(ni * Cp * 4), true});
    if (out->dyn_bin) large.push_back({out->dyn_bin, G4 * nd, 4, put(G4 * nd * Cp * 4), true});
    if (out->dyn_val) large.push_back({out->dyn_val, G4 * nd, 16, put(G4 * nd * Cp * 16), true});
    const size_t stage_prefix = direct ? small_bytes : o;
    const size_t o_ev = cap ? put(Cp * cap * 8) : 0, o_packed = cap ? put(Cp * cap * 8) : 0;
    const size_t o_scratch = cap ? put(emgpu::pack_scratch_words((int64_t)Cp) * 4) : 0;
    const size_t dev_bytes = std::max<size_t>(o, 256);
    const size_t stage_bytes = std::max<size_t>(stage_prefix + (cap ? C * cap * 8 : 0), 256);
    if (!provision(ctx, P.nchunks, dev_bytes, stage_bytes)) return fail(EMGPU_ERR_HIP, "emgpu_sample_dbn_host: out of device memory");

    emgpu_sample_params pd = *p;
    if (p->start) {     // the start grid and the index list are caller (host) memory here: uploaded once, every chunk reads its rows
        pd.start = upload_start_grid(ctx, p->start, n, ni);
    }
    if (p->indices) {
        uint64_t *di = (uint64_t *)ctx_scratch(ctx, 1, n * sizeof(uint64_t));
        HIP_OK(hipMemcpyAsync(di, p->indices, n * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
        pd.indices = di;
    }
    if (p->start || p->indices) HIP_OK(hipStreamSynchronize(ctx->stream));

    emgpu_host_stats_t st{};
    size_t packed_rows[2] = {0, 0};
    auto launch = [&](size_t k0, size_t c, int b) {
        char *dev = (char *)ctx->chunk_buf[b].p;
        emgpu_sample_params q = pd;
        q.n = (int64_t)c;
        q.first_index = p->first_index + (uint64_t)k0;
        if (pd.indices) q.indices = pd.indices + k0;
        if (pd.start) q.start = pd.start + k0 * ni;
        emgpu_sample_out d{};
        d.ld = (int64_t)Cp;
        for (const Arr &a : small) {
            if (a.dst == out->ev_count) d.ev_count = (uint32_t *)(dev + a.dev_off);
            else if (a.dst == out->attempts) d.attempts = (int32_t *)(dev + a.dev_off);
            else d.log_weight = (double *)(dev + a.dev_off);
        }
        for (const Arr &a : large) {
            if (a.dst == out->init_bin) d.init_bin = (uint8_t *)(dev + a.dev_off);
            else if (a.dst == out->init_val) d.init_val = (float *)(dev + a.dev_off);
            else if (a.dst == out->dyn_bin) d.dyn_bin = (uint32_t *)(dev + a.dev_off);
            else d.dyn_val = (float *)(dev + a.dev_off);
        }
        if (cap) d.events = (emgpu_event *)(dev + o_ev);
        const int r = emgpu_sample_dbn_device(ctx, h, &q, &d);
        if (r != EMGPU_OK) throw Error(r, g_err);
        if (cap) {
            hipError_t e = emgpu::launch_pack_events((int64_t)c, (uint32_t)cap, d.ev_count, (const uint64_t *)(dev + o_ev), (uint32_t *)(dev + o_scratch),
                                                     (uint64_t *)(dev + o_packed), ctx->stream);
            if (e != hipSuccess) throw Error(EMGPU_ERR_HIP, std::string("pack launch: ") + hipGetErrorString(e));
            HIP_OK(hipMemcpyAsync(&ctx->h_total[2 * b], dev + o_scratch, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        }
    };
    auto copy = [&](size_t k0, size_t c, int b) {
        const char *dev = (const char *)ctx->chunk_buf[b].p;
        char *stg = (char *)ctx->h_stage[b];
        if (stage_prefix) HIP_OK(hipMemcpyAsync(stg, dev, stage_prefix, hipMemcpyDeviceToHost, ctx->copy_stream));
        st.bytes_d2h += (int64_t)stage_prefix;
        if (cap) packed_rows[b] = (size_t)ctx->h_total[2 * b];   // how many rows cross PCIe is known only now
        if (cap && packed_rows[b]) {
            HIP_OK(hipMemcpyAsync(stg + stage_prefix, dev + o_packed, packed_rows[b] * 8, hipMemcpyDeviceToHost, ctx->copy_stream));
            st.bytes_d2h += (int64_t)packed_rows[b] * 8;
            st.event_rows += (int64_t)packed_rows[b];
        }
        if (direct)   // pinned outputs: one pitched copy per array (56.5 GB/s of the 57 GB/s a plain pinned copy reaches -- tools/host_path_probe.py)
            for (const Arr &a : large) {
                char *dst = (char *)a.dst + (off + k0) * a.elem;
                if (ld == c && Cp == c) HIP_OK(hipMemcpyAsync(dst, dev + a.dev_off, a.rows * c * a.elem, hipMemcpyDeviceToHost, ctx->copy_stream));
                else HIP_OK(hipMemcpy2DAsync(dst, ld * a.elem, dev + a.dev_off, Cp * a.elem, c * a.elem, a.rows, hipMemcpyDeviceToHost, ctx->copy_stream));
                st.bytes_d2h += (int64_t)(a.rows * c * a.elem);
            }
    };
    auto scatter = [&](size_t k0, size_t c, int b) {
        const char *stg = (const char *)ctx->h_stage[b];
        std::vector<Job> jobs;
        for (const Arr &a : small) jobs.push_back({(char *)a.dst + ((a.offset_by_col ? off : 0) + k0) * a.elem, stg + a.dev_off, c * a.elem});
        if (!direct)
            for (const Arr &a : large)
                for (size_t r = 0; r < a.rows; r++) jobs.push_back({(char *)a.dst + (r * ld + off + k0) * a.elem, stg + a.dev_off + r * Cp * a.elem, c * a.elem});
        std::vector<uint32_t> offs;
        if (cap) {   // the lists' first packed rows: a prefix sum over the chunk's counts (what the device did, redone on 4 c bytes)
            const uint32_t *cnt = (const uint32_t *)(stg + small[0].dev_off);
            offs.resize(c + 1);
            uint32_t run = 0;
            for (size_t i = 0; i < c; i++) { offs[i] = run; run += std::min<uint32_t>(cnt[i], (uint32_t)cap); }
            offs[c] = run;
            if ((size_t)run != packed_rows[b]) throw Error(EMGPU_ERR_HIP, "emgpu_sample_dbn_host: packed event rows disagree with the counts");
        }
        size_t moved = cap ? packed_rows[b] * 8 : 0;
        for (const Job &j : jobs) moved += j.bytes;
        const int TT = (int)std::min<size_t>((size_t)host_threads(), std::max<size_t>(1, moved >> 20));   // a thread per MiB, at most host_threads()
        run_jobs(jobs, TT, [&](int t) {
            if (!cap) return;
            const uint64_t *packed = (const uint64_t *)(stg + stage_prefix);
            emgpu_event *hev = out->events + (off + k0) * cap;
            const size_t i0 = c * (size_t)t / (size_t)TT, i1 = c * ((size_t)t + 1) / (size_t)TT;
            for (size_t i = i0; i < i1; i++) memcpy(hev + i * cap, packed + offs[i], (size_t)(offs[i + 1] - offs[i]) * 8);
        });
    };
    // the row count is waited for only when there are lists: a dense-only chunk's copies queue behind its launches without the host
    return run_chunks(ctx, P, direct, /*wait_rows=*/cap > 0, t_call, st, launch, copy, scatter);
    EMGPU_CATCH
}

// ================================================================================================ UncorEncounterModel.sample's outputs
int emgpu_sample_uncor_host(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_sample_params *p, const emgpu_uncor_out *out) {
    EMGPU_TRY
    if (!ctx || !h || !p || !out) return fail(EMGPU_ERR_ARG, "null argument");
    if (!out->inits || !out->ev_count || !out->events || !out->ctrl_count || !out->controls || !out->totals)
        return fail(EMGPU_ERR_ARG, "inits, ev_count, events, ctrl_count, controls and totals are required");
    if (p->event_cap < 1) return fail(EMGPU_ERR_ARG, "event_cap must be >= 1");
    if (out->events_cap < 0 || out->controls_cap < 0) return fail(EMGPU_ERR_ARG, "events_cap and controls_cap must be >= 0");
    if (p->indices) return fail(EMGPU_ERR_ARG, "emgpu_sample_uncor_host: index lists are not supported");
    if (p->n < 0 || p->sample_time < 1 || p->sample_time > 65535) return fail(EMGPU_ERR_ARG, "n < 0 or sample_time outside 1..65535");
    const Model &m = h->m;
    for (int k = 0; k < 3; k++)
        if (out->ctrl_var[k] < 1 || out->ctrl_var[k] > m.n_initial) return fail(EMGPU_ERR_ARG, "ctrl_var: a variable id outside 1..n_initial");
    CTX_DEVICE(ctx);
    const auto t_call = Clock::now();
    const size_t n = (size_t)p->n, ni = (size_t)m.n_initial, T = (size_t)p->sample_time, cap = (size_t)p->event_cap;
    out->totals[0] = out->totals[1] = 0;
    if (n == 0) return sample_nothing(ctx, h, p);

    // ---- the caller's arrays: per trajectory (a chunk is one contiguous piece of each) and packed rows; each is written by the copy engine when
    // it is pinned, else through the staging buffer and the host threads
    struct Arr { char *dst; size_t elem; size_t dev_off = 0, stg_off = 0; bool staged = false; };
    Arr a_cnt{(char *)out->ev_count, 4}, a_att{(char *)out->attempts, 4}, a_ccnt{(char *)out->ctrl_count, 4}, a_init{(char *)out->inits, 8 * ni},
        a_smp{(char *)out->samples, 8 * ni * T}, a_ev{(char *)out->events, 8}, a_ctl{(char *)out->controls, 32};
    std::vector<Arr *> per_traj = {&a_cnt, &a_ccnt, &a_init};
    if (out->attempts) per_traj.push_back(&a_att);
    if (out->samples) per_traj.push_back(&a_smp);
    bool direct = true;
    for (Arr *a : per_traj) { a->staged = !is_pinned(a->dst); direct = direct && !a->staged; }
    for (Arr *a : {&a_ev, &a_ctl}) { a->staged = !is_pinned(a->dst); direct = direct && !a->staged; }

    const size_t bpt = 16 + 4 * ni + 8 * ni + (out->samples ? 8 * ni * T : 0) + 16 * cap + 32 * cap;   // device bytes per trajectory
    const ChunkPlan P = chunk_plan(n, bpt, direct, cap);
    const size_t C = P.C, Cp = P.Cp;
    size_t o = 0;
    auto put = [&](size_t bytes) { const size_t at = o; o = round_up(o + bytes, 256); return at; };
    a_cnt.dev_off = put(Cp * 4); a_att.dev_off = put(Cp * 4); a_ccnt.dev_off = put(Cp * 4);
    const size_t o_coff = put(Cp * 4), o_iv = put(ni * Cp * 4);
    a_init.dev_off = put(Cp * a_init.elem);
    if (out->samples) a_smp.dev_off = put(Cp * a_smp.elem);
    const size_t o_ev = put(Cp * cap * 8);
    a_ev.dev_off = put(Cp * cap * 8);
    a_ctl.dev_off = put(Cp * cap * 32);
    const size_t o_scr = put(emgpu::pack_scratch_words((int64_t)Cp) * 4), o_fscr = put(emgpu::pack_scratch_words((int64_t)Cp) * 4);
    const size_t dev_bytes = std::max<size_t>(o, 256);
    size_t so = 0;
    for (Arr *a : per_traj) if (a->staged) { a->stg_off = so; so = round_up(so + C * a->elem, 256); }
    for (Arr *a : {&a_ev, &a_ctl}) if (a->staged) { a->stg_off = so; so = round_up(so + C * cap * a->elem, 256); }
    const size_t stage_bytes = std::max<size_t>(so, 256);
    if (!provision(ctx, P.nchunks, dev_bytes, stage_bytes)) return fail(EMGPU_ERR_HIP, "emgpu_sample_uncor_host: out of device memory");
    const int32_t *d_start = nullptr;
    if (p->start) { d_start = upload_start_grid(ctx, p->start, n, ni); HIP_OK(hipStreamSynchronize(ctx->stream)); }

    emgpu_host_stats_t st{};
    size_t rows[2][2] = {{0, 0}, {0, 0}}, base[2][2] = {{0, 0}, {0, 0}};   // per buffer: event / control rows of its chunk and their first row in the call
    bool fits[2][2] = {{false, false}, {false, false}};
    size_t total_ev = 0, total_ctl = 0;
    auto launch = [&](size_t k0, size_t c, int b) {
        char *dev = (char *)ctx->chunk_buf[b].p;
        emgpu_sample_params q = *p;
        q.n = (int64_t)c;
        q.first_index = p->first_index + (uint64_t)k0;
        if (d_start) q.start = d_start + k0 * ni;
        emgpu_sample_out d{};
        d.ld = (int64_t)Cp;
        d.init_val = (float *)(dev + o_iv);
        d.ev_count = (uint32_t *)(dev + a_cnt.dev_off);
        d.events = (emgpu_event *)(dev + o_ev);
        if (out->attempts) d.attempts = (int32_t *)(dev + a_att.dev_off);
        const int r = emgpu_sample_dbn_device(ctx, h, &q, &d);
        if (r != EMGPU_OK) throw Error(r, g_err);
        launch_ok(emgpu::launch_pack_events((int64_t)c, (uint32_t)cap, d.ev_count, (const uint64_t *)(dev + o_ev), (uint32_t *)(dev + o_scr),
                                            (uint64_t *)(dev + a_ev.dev_off), ctx->stream));
        emgpu::EmgpuFormatRun F{};
        F.n = (int64_t)c; F.cap = (uint32_t)cap; F.T = (int32_t)T; F.ni = (int32_t)ni; F.ld = (int64_t)Cp;
        F.ev_count = d.ev_count; F.ev = (const uint64_t *)(dev + o_ev); F.init_val = d.init_val;
        F.id_dh = out->ctrl_var[0]; F.id_dpsi = out->ctrl_var[1]; F.id_dv = out->ctrl_var[2];
        F.ctrl_count = (uint32_t *)(dev + a_ccnt.dev_off); F.ctrl_off = (uint32_t *)(dev + o_coff); F.scratch = (uint32_t *)(dev + o_fscr);
        F.inits = (double *)(dev + a_init.dev_off); F.samples = out->samples ? (double *)(dev + a_smp.dev_off) : nullptr;
        F.controls = (double *)(dev + a_ctl.dev_off);
        launch_ok(emgpu::launch_format_uncor(F, ctx->stream));
        HIP_OK(hipMemcpyAsync(&ctx->h_total[2 * b], dev + o_scr, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_OK(hipMemcpyAsync(&ctx->h_total[2 * b + 1], dev + o_fscr, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    };
    auto copy = [&](size_t k0, size_t c, int b) {
        rows[b][0] = (size_t)ctx->h_total[2 * b]; rows[b][1] = (size_t)ctx->h_total[2 * b + 1];
        base[b][0] = total_ev; base[b][1] = total_ctl;
        total_ev += rows[b][0]; total_ctl += rows[b][1];
        fits[b][0] = total_ev <= (size_t)out->events_cap; fits[b][1] = total_ctl <= (size_t)out->controls_cap;
        const char *dev = (const char *)ctx->chunk_buf[b].p;
        char *stg = (char *)ctx->h_stage[b];
        auto down = [&](const Arr &a, size_t first, size_t count) {
            if (!count) return;
            char *dst = a.staged ? stg + a.stg_off : a.dst + first * a.elem;
            HIP_OK(hipMemcpyAsync(dst, dev + a.dev_off, count * a.elem, hipMemcpyDeviceToHost, ctx->copy_stream));
            st.bytes_d2h += (int64_t)(count * a.elem);
        };
        for (const Arr *a : per_traj) down(*a, k0, c);
        if (fits[b][0]) down(a_ev, base[b][0], rows[b][0]);   // (a call whose rows outgrow the caller's arrays still counts them: the totals)
        if (fits[b][1]) down(a_ctl, base[b][1], rows[b][1]);
        st.event_rows += (int64_t)rows[b][0];
    };
    auto scatter = [&](size_t k0, size_t c, int b) {
        const char *stg = (const char *)ctx->h_stage[b];
        std::vector<Job> jobs;
        auto add = [&](const Arr &a, size_t first, size_t count) {   // in pieces of about 1 MiB, so that the threads share a large array
            if (!a.staged || !count) return;
            const size_t bytes = count * a.elem, piece = (size_t)1 << 20;
            for (size_t q = 0; q < bytes; q += piece) jobs.push_back({a.dst + first * a.elem + q, stg + a.stg_off + q, std::min(piece, bytes - q)});
        };
        for (const Arr *a : per_traj) add(*a, k0, c);
        if (fits[b][0]) add(a_ev, base[b][0], rows[b][0]);
        if (fits[b][1]) add(a_ctl, base[b][1], rows[b][1]);
        run_jobs(jobs, (int)std::min<size_t>((size_t)host_threads(), std::max<size_t>(1, jobs.size())), [](int) {});   // a thread per job, at most host_threads()
    };
    const int rc = run_chunks(ctx, P, direct, /*wait_rows=*/true, t_call, st, launch, copy, scatter);
    if (rc == EMGPU_ERR_EVENT_CAP) {   // a list outgrew event_cap: what the lists need in full; their control rows are at most as many
        uint64_t need = 0;
        for (size_t i = 0; i < n; i++) need += out->ev_count[i];
        out->totals[0] = out->totals[1] = (int64_t)need;
        return rc;
    }
    out->totals[0] = (int64_t)total_ev;
    out->totals[1] = (int64_t)total_ctl;
    if (rc == EMGPU_OK && (total_ev > (size_t)out->events_cap || total_ctl > (size_t)out->controls_cap))
        return fail(EMGPU_ERR_EVENT_CAP, "emgpu_sample_uncor_host: the call has " + std::to_string(total_ev) + " event rows and " + std::to_string(total_ctl) +
                                             " control rows, events_cap / controls_cap are " + std::to_string(out->events_cap) + " / " + std::to_string(out->controls_cap));
    return rc;
    EMGPU_CATCH
}

// ================================================================================================ em_sample's text files
int emgpu_text_bound(const emgpu_model *h, int64_t n, int32_t sample_time, int64_t bytes[2]) {
    if (!h || !bytes) return fail(EMGPU_ERR_ARG, "null argument");
    if (n < 0 || sample_time < 1) return fail(EMGPU_ERR_ARG, "n < 0 or sample_time < 1");
    bytes[0] = n * (int64_t)emgpu::text_row_bound_initial(h->m.n_initial);
    bytes[1] = n * (int64_t)sample_time * (int64_t)emgpu::text_row_bound_transition(h->m.n_dyn());
    return EMGPU_OK;
}

int emgpu_sample_text_host(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_sample_params *p, const emgpu_text_out *out) {
    EMGPU_TRY
    if (!ctx || !h || !p || !out) return fail(EMGPU_ERR_ARG, "null argument");
    if (!out->initial || !out->transition || !out->totals) return fail(EMGPU_ERR_ARG, "initial, transition and totals are required");
    if (out->initial_cap < 0 || out->transition_cap < 0) return fail(EMGPU_ERR_ARG, "initial_cap and transition_cap must be >= 0");
    if (p->indices) return fail(EMGPU_ERR_ARG, "emgpu_sample_text_host: index lists are not supported");
    if (p->n < 0 || p->sample_time < 1) return fail(EMGPU_ERR_ARG, "n < 0 or sample_time < 1");
    if (out->id_first < 0 || out->id_first > ((int64_t)1 << 53) - p->n) return fail(EMGPU_ERR_ARG, "id_first < 0 or id_first + n > 2^53");
    CTX_DEVICE(ctx);
    const auto t_call = Clock::now();
    const Model &m = h->m;
    const size_t n = (size_t)p->n, ni = (size_t)m.n_initial, nd = (size_t)m.n_dyn(), T = (size_t)p->sample_time, G4 = (T + 3) / 4;
    const size_t rb_i = emgpu::text_row_bound_initial((int)ni), wt = T * emgpu::text_row_bound_transition((int)nd);   // worst case per trajectory
    out->totals[0] = out->totals[1] = 0;
    if (n == 0) return sample_nothing(ctx, h, p);

    // ---- the caller's buffers: the two texts (a chunk's bytes go behind the chunks' before it) and, when wanted, the dense arrays; each is
    // written by the copy engine when it is pinned, else through the staging buffer and the host threads
    struct Arr { char *dst; size_t rows, elem; size_t dev_off = 0, stg_off = 0; bool staged = false; };
    Arr a_iv{(char *)out->init_val, ni, 4}, a_dv{(char *)out->dyn_val, G4 * nd, 16};
    struct Txt { char *dst; size_t cap, per; size_t dev_off = 0, stg_off = 0; bool staged = false; };
    Txt tx[2] = {{out->initial, (size_t)out->initial_cap, rb_i}, {out->transition, (size_t)out->transition_cap, wt}};
    std::vector<Arr *> arrs;
    if (out->init_val && ni) arrs.push_back(&a_iv);
    if (out->dyn_val && nd) arrs.push_back(&a_dv);
    bool direct = true;
    for (Arr *a : arrs) { a->staged = !is_pinned(a->dst); direct = direct && !a->staged; }
    for (Txt &t : tx) { t.staged = !is_pinned(t.dst); direct = direct && !t.staged; }

    const size_t bpt = 5 * ni + 20 * G4 * nd + 12 + rb_i + wt;   // device bytes per trajectory
    // the scans count a chunk's bytes in 32 bits: the chunk is sized by a trajectory's worst case
    const ChunkPlan P = chunk_plan(n, bpt, direct, std::max(rb_i, wt));
    const size_t C = P.C, Cp = P.Cp;
    if (C * std::max(rb_i, wt) > (size_t)0xFFFFFFFFu) return fail(EMGPU_ERR_ARG, "emgpu_sample_text_host: sample_time too large: a chunk's text would not fit 32 bits");
    size_t o = 0;
    auto put = [&](size_t bytes) { const size_t at = o; o = round_up(o + std::max<size_t>(bytes, 1), 256); return at; };
    a_iv.dev_off = put(ni * Cp * 4);
    a_dv.dev_off = put(G4 * nd * Cp * 16);
    // (the sampler is asked for what emgpu_sample_dbn_host's callers ask it for, bins and attempts too: the same kernel instance serves both)
    const size_t o_ib = put(ni * Cp), o_db = put(G4 * nd * Cp * 4), o_at = put(Cp * 4);
    const size_t o_ci = put(Cp * 4), o_ct = put(Cp * 4);
    const size_t o_si = put(emgpu::pack_scratch_words((int64_t)Cp) * 4), o_st = put(emgpu::pack_scratch_words((int64_t)Cp) * 4);
    for (Txt &t : tx) t.dev_off = put(C * t.per);
    const size_t dev_bytes = std::max<size_t>(o, 256);
    size_t so = 0;
    for (Arr *a : arrs) if (a->staged) { a->stg_off = so; so = round_up(so + a->rows * Cp * a->elem, 256); }
    for (Txt &t : tx) if (t.staged) { t.stg_off = so; so = round_up(so + C * t.per, 256); }
    const size_t stage_bytes = std::max<size_t>(so, 256);
    if (!provision(ctx, P.nchunks, dev_bytes, stage_bytes)) return fail(EMGPU_ERR_HIP, "emgpu_sample_text_host: out of device memory");
    const int32_t *d_start = nullptr;
    if (p->start) { d_start = upload_start_grid(ctx, p->start, n, ni); HIP_OK(hipStreamSynchronize(ctx->stream)); }

    emgpu_host_stats_t st{};
    size_t bytes[2][2] = {{0, 0}, {0, 0}}, base[2][2] = {{0, 0}, {0, 0}}, total[2] = {0, 0};   // per buffer: the chunk's bytes and their place in the call's
    bool fits[2][2] = {{false, false}, {false, false}};
    auto launch = [&](size_t k0, size_t c, int b) {
        char *dev = (char *)ctx->chunk_buf[b].p;
        emgpu_sample_params q = *p;
        q.n = (int64_t)c;
        q.first_index = p->first_index + (uint64_t)k0;
        if (d_start) q.start = d_start + k0 * ni;
        emgpu_sample_out d{};
        d.ld = (int64_t)Cp;
        d.init_val = (float *)(dev + a_iv.dev_off);
        d.init_bin = (uint8_t *)(dev + o_ib);
        d.attempts = (int32_t *)(dev + o_at);
        if (nd) { d.dyn_val = (float *)(dev + a_dv.dev_off); d.dyn_bin = (uint32_t *)(dev + o_db); }
        const int r = emgpu_sample_dbn_device(ctx, h, &q, &d);
        if (r != EMGPU_OK) throw Error(r, g_err);
        emgpu::EmgpuTextRun R{};
        R.n = (int64_t)c; R.T = (int32_t)T; R.ni = (int32_t)ni; R.nd = (int32_t)nd; R.ld = (int64_t)Cp;
        R.init_val = d.init_val; R.dyn_val = (const float *)(dev + a_dv.dev_off); R.id_first = out->id_first + (int64_t)k0;
        R.cnt_i = (uint32_t *)(dev + o_ci); R.cnt_t = (uint32_t *)(dev + o_ct); R.scr_i = (uint32_t *)(dev + o_si); R.scr_t = (uint32_t *)(dev + o_st);
        R.text_i = dev + tx[0].dev_off; R.text_t = dev + tx[1].dev_off;
        launch_ok(emgpu::launch_text_rows(R, ctx->stream));
        HIP_OK(hipMemcpyAsync(&ctx->h_total[2 * b], dev + o_si, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_OK(hipMemcpyAsync(&ctx->h_total[2 * b + 1], dev + o_st, sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    };
    auto copy = [&](size_t k0, size_t c, int b) {
        const char *dev = (const char *)ctx->chunk_buf[b].p;
        char *stg = (char *)ctx->h_stage[b];
        for (int x = 0; x < 2; x++) {   // how many bytes cross PCIe is known only now
            bytes[b][x] = (size_t)ctx->h_total[2 * b + x];
            if (bytes[b][x] > c * tx[x].per) throw Error(EMGPU_ERR_HIP, "emgpu_sample_text_host: a chunk's text outgrew its bound");
            base[b][x] = total[x];
            total[x] += bytes[b][x];
            fits[b][x] = total[x] <= tx[x].cap;
            if (!fits[b][x] || !bytes[b][x]) continue;   // (a call whose text outgrows the caller's buffer still counts it: the totals)
            HIP_OK(hipMemcpyAsync(tx[x].staged ? stg + tx[x].stg_off : tx[x].dst + base[b][x], dev + tx[x].dev_off, bytes[b][x], hipMemcpyDeviceToHost, ctx->copy_stream));
            st.bytes_d2h += (int64_t)bytes[b][x];
        }
        for (const Arr *a : arrs) {
            if (a->staged) HIP_OK(hipMemcpyAsync(stg + a->stg_off, dev + a->dev_off, a->rows * Cp * a->elem, hipMemcpyDeviceToHost, ctx->copy_stream));
            else HIP_OK(hipMemcpy2DAsync(a->dst + k0 * a->elem, n * a->elem, dev + a->dev_off, Cp * a->elem, c * a->elem, a->rows, hipMemcpyDeviceToHost, ctx->copy_stream));
            st.bytes_d2h += (int64_t)(a->rows * (a->staged ? Cp : c) * a->elem);
        }
    };
    auto scatter = [&](size_t k0, size_t c, int b) {
        const char *stg = (const char *)ctx->h_stage[b];
        std::vector<Job> jobs;
        for (int x = 0; x < 2; x++) {
            if (!tx[x].staged || !fits[b][x]) continue;
            const size_t piece = (size_t)1 << 20;   // in pieces of about 1 MiB, so that the threads share a large text
            for (size_t q = 0; q < bytes[b][x]; q += piece) jobs.push_back({tx[x].dst + base[b][x] + q, stg + tx[x].stg_off + q, std::min(piece, bytes[b][x] - q)});
        }
        for (const Arr *a : arrs)
            if (a->staged)
                for (size_t r = 0; r < a->rows; r++) jobs.push_back({a->dst + (r * n + k0) * a->elem, stg + a->stg_off + r * Cp * a->elem, c * a->elem});
        run_jobs(jobs, (int)std::min<size_t>((size_t)host_threads(), std::max<size_t>(1, jobs.size())), [](int) {});
    };
    const int rc = run_chunks(ctx, P, direct, /*wait_rows=*/true, t_call, st, launch, copy, scatter);
    out->totals[0] = (int64_t)total[0];
    out->totals[1] = (int64_t)total[1];
    if (rc == EMGPU_OK && (total[0] > tx[0].cap || total[1] > tx[1].cap))
        return fail(EMGPU_ERR_EVENT_CAP, "emgpu_sample_text_host: the texts have " + std::to_string(total[0]) + " and " + std::to_string(total[1]) +
                                             " bytes, initial_cap / transition_cap are " + std::to_string(out->initial_cap) + " / " + std::to_string(out->transition_cap));
    return rc;
    EMGPU_CATCH
}

int emgpu_host_stats(const emgpu_ctx *ctx, emgpu_host_stats_t *out) {
    if (!ctx || !out) return fail(EMGPU_ERR_ARG, "null argument");
    *out = ctx->host_stats;
    return EMGPU_OK;
}

} // extern "C"
