// emgpu_host.cpp -- the parts of the C ABI that own memory on behalf of the caller (round 6):
//   * the trace pool: emgpu_trace_alloc / _out / _report / _free -- device memory for the sampler's outputs whose PLACEMENT has been
//     measured with the caller's own launch (profiles/r05_placement_probe.txt: the same launch writes one 36 GB allocation in 6.0 ms
//     and another in 7.1 ms);
//   * the pinned pool: emgpu_host_alloc / _free;
//   * emgpu_sample_dbn_host, emgpu_sample_uncor_host (UncorEncounterModel.sample's samples and controls built on the device) and
//     emgpu_sample_text_host (em_sample's two text files formatted on the device, em_sample.m:85-99): one driver, run_chunks, pipelines all three -- chunk k's launches | chunk k-1's copy over PCIe | chunk k-2's copy into the caller's arrays.
// Reference semantics: the loop over samples of UncorEncounterModel.m:244-300 and the host arrays it returns (:283-300).
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <system_error>
#include <thread>

#include "emgpu_internal.hpp"

struct emgpu_trace {
    emgpu_ctx::TraceBlock blk;
    emgpu_sample_out out{};
    emgpu_trace_report_t rep{};
};

namespace {
using Clock = std::chrono::steady_clock;
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }
size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ------------------------------------------------------------------------------------------------ device blocks
// How a block of the trace pool is obtained (round 6, tools/placement_probe5.py, profiles/r06_placement_probe.txt).  The same launch writes a
// 36 GB trace in 5.9, 6.6 or 7.0 ms depending on the allocation.  Blocks that hipMalloc hands out are mostly of the 6.6 ms kind, now and then
// of the others; ONE ADDRESS RANGE BACKED BY SEPARATELY CREATED 1 GiB PHYSICAL CHUNKS (hipMemAddressReserve + hipMemCreate + hipMemMap) is of the
// 5.9 ms kind four to six times out of six, of the 7.0 ms kind the rest (chunks of 256 MiB - 2 GiB alike, 4 GiB chunks like hipMalloc; where the
// range starts -- on a 1 GiB boundary or 2 MiB off one -- makes no difference: measured both ways).  Why is not known; the allocator does not need
// to know: blocks of 1 GiB and more are built that way (falling back to hipMalloc where the virtual-memory calls fail), smaller ones come from
// hipMalloc, and emgpu_trace_alloc MEASURES its candidates -- candidate 0 a plain hipMalloc block, so that the report shows what a caller's own
// allocation would have got.
// EMGPU_TRACE_ALLOC (read once; experiments) = "plain": hipMalloc only; "contiguous": hipExtMallocWithFlags(hipDeviceMallocContiguous);
// "vmm:<chunk MiB>": another chunk size.
struct VmmBlock { size_t bytes = 0, chunk = 0; std::vector<hipMemGenericAllocationHandle_t> handles; };
std::mutex g_vmm_mu;
std::map<void *, VmmBlock> g_vmm;
struct AllocMode { int mode; size_t chunk; };
const AllocMode &alloc_mode_once() {
    static const AllocMode am = [] {   // (a function-local static: initialised once, also when several host threads come here together)
        AllocMode a{3, (size_t)1 << 30};   // automatic: a range over 1 GiB chunks for blocks of 1 GiB and more, hipMalloc below (and as the fallback)
        const char *e = getenv("EMGPU_TRACE_ALLOC");
        if (e && !strncmp(e, "plain", 5)) a.mode = 0;
        if (e && !strncmp(e, "contiguous", 10)) a.mode = 1;
        if (e && !strncmp(e, "vmm", 3)) {
            a.mode = 2;
            if (e[3] == ':' && atol(e + 4) > 0) a.chunk = (size_t)atol(e + 4) << 20;
        }
        return a;
    }();
    return am;
}
int alloc_mode(size_t *chunk) {
    const AllocMode &a = alloc_mode_once();
    if (chunk) *chunk = a.chunk;
    return a.mode;
}
bool vmm_block(size_t bytes, void **p) {
    size_t chunk = 0;
    (void)alloc_mode(&chunk);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    hipMemAllocationProp prop;
    memset(&prop, 0, sizeof prop);
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = dev;
    size_t gran = 0;
    if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended) != hipSuccess || !gran) { (void)hipGetLastError(); return false; }
    chunk = round_up(chunk, gran);
    const size_t total = round_up(bytes, chunk);
    void *va = nullptr;   // (hipMemAddressReserve returns 2 MiB-aligned ranges whatever alignment it is asked for: tools/ubench/vmm_repro.hip)
    if (hipMemAddressReserve(&va, total, 0, nullptr, 0) != hipSuccess) { (void)hipGetLastError(); return false; }
    VmmBlock B;
    B.bytes = total; B.chunk = chunk;
    bool ok = true;
    for (size_t o = 0; o < total && ok; o += chunk) {
        hipMemGenericAllocationHandle_t hnd;
        if (hipMemCreate(&hnd, chunk, &prop, 0) != hipSuccess) { ok = false; break; }
        B.handles.push_back(hnd);
        if (hipMemMap((char *)va + o, chunk, 0, hnd, 0) != hipSuccess) { ok = false; break; }
    }
    if (ok) {
        hipMemAccessDesc acc;
        memset(&acc, 0, sizeof acc);
        acc.location = prop.location;
        acc.flags = hipMemAccessFlagsProtReadWrite;
        ok = hipMemSetAccess(va, total, &acc, 1) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        for (size_t i = 0; i < B.handles.size(); i++) { (void)hipMemUnmap((char *)va + i * chunk, chunk); (void)hipMemRelease(B.handles[i]); }
        (void)hipMemAddressFree(va, total);
        (void)hipGetLastError();
        return false;
    }
    std::lock_guard<std::mutex> lk(g_vmm_mu);
    g_vmm[va] = std::move(B);
    *p = va;
    return true;
}
bool device_block(size_t bytes, void **p, bool plain = false) {   // an allocation that reports failure instead of throwing (a candidate too many is not an error)
    *p = nullptr;
    const int mode = plain ? 0 : alloc_mode(nullptr);
    if (mode == 2) return vmm_block(bytes, p);
    if (mode == 3 && bytes >= ((size_t)1 << 30) && vmm_block(bytes, p)) return true;
    const hipError_t e = mode == 1 ? hipExtMallocWithFlags(p, bytes, hipDeviceMallocContiguous) : hipMalloc(p, bytes);
    if (e == hipSuccess) return true;
    (void)hipGetLastError();
    *p = nullptr;
    return false;
}
void device_release(void *p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_vmm_mu);
        auto it = g_vmm.find(p);
        if (it != g_vmm.end()) {
            VmmBlock &B = it->second;
            for (size_t i = 0; i < B.handles.size(); i++) { (void)hipMemUnmap((char *)p + i * B.chunk, B.chunk); (void)hipMemRelease(B.handles[i]); }
            // The physical chunks go back; the ADDRESS RANGE does not (unless EMGPU_VMM_FREE_VA is set).  A HIP runtime (the 7.0 build PyTorch wheels
            // bundle) crashes in hipMemMap -- VirtualGPU::submitVirtualMap -- when a new range overlaps one whose block had been the source of
            // hipMemcpyAsync calls before it was released (tools/copy_placement_probe.py; the 7.2 system runtime does not).  A reservation costs
            // address space only (47 bits of it: a thousand 36 GB traces are 36 TiB), so ranges are simply never handed back for re-use.
            static const bool free_va = getenv("EMGPU_VMM_FREE_VA") != nullptr;
            if (free_va) (void)hipMemAddressFree(p, B.bytes);
            g_vmm.erase(it);
            return;
        }
    }
    (void)hipFree(p);
}
void pool_release(emgpu_ctx *ctx) {
    for (auto &b : ctx->trace_pool) device_release(b.p);
    ctx->trace_pool.clear();
}
// a free block of the pool that fits (and is not more than a quarter too large), or a fresh allocation; {nullptr} when neither exists
emgpu_ctx::TraceBlock pool_take(emgpu_ctx *ctx, size_t bytes, bool *from_pool, bool plain = false) {
    int best = -1;
    for (int i = 0; i < (int)ctx->trace_pool.size(); i++) {
        const auto &b = ctx->trace_pool[(size_t)i];
        if (b.bytes >= bytes && b.bytes <= bytes + bytes / 4 + (1u << 20) && (best < 0 || b.bytes < ctx->trace_pool[(size_t)best].bytes)) best = i;
    }
    if (from_pool) *from_pool = best >= 0;
    if (best >= 0) {
        emgpu_ctx::TraceBlock b = ctx->trace_pool[(size_t)best];
        ctx->trace_pool.erase(ctx->trace_pool.begin() + best);
        return b;
    }
    emgpu_ctx::TraceBlock b;
    if (!device_block(bytes, &b.p, plain)) {   // out of memory: give the pool's idle blocks back and try once more
        HIP_OK(hipStreamSynchronize(ctx->stream));
        pool_release(ctx);
        if (!device_block(bytes, &b.p, plain)) return b;
    }
    b.bytes = bytes;
    return b;
}

// ------------------------------------------------------------------------------------------------ trace layout
struct TraceLayout {
    size_t o_ib = 0, o_iv = 0, o_db = 0, o_dv = 0, o_ec = 0, o_ev = 0, o_at = 0, bytes = 0;
    int64_t ld = 0;
};
TraceLayout trace_layout(const Model &m, const emgpu_sample_params *p, uint32_t want) {
    constexpr size_t kA = 2u << 20;   // every array of a trace starts on a 2 MiB boundary
    TraceLayout L;
    L.ld = (int64_t)round_up((size_t)std::max<int64_t>(p->n, 1), 1024);
    const size_t ld = (size_t)L.ld, ni = (size_t)m.n_initial, nd = (size_t)m.n_dyn(), G4 = ((size_t)p->sample_time + 3) / 4;
    size_t o = 0;
    auto put = [&](size_t bytes) { const size_t at = o; o = round_up(o + std::max<size_t>(bytes, 1), kA); return at; };
    if (want & EMGPU_TRACE_DENSE) { L.o_dv = put(G4 * nd * ld * 16); L.o_db = put(G4 * nd * ld * 4); }
    if (want & EMGPU_TRACE_INIT) { L.o_iv = put(ni * ld * 4); L.o_ib = put(ni * ld); }
    if (want & EMGPU_TRACE_EVENTS) { L.o_ev = put(ld * (size_t)p->event_cap * 8); L.o_ec = put(ld * 4); }
    if (want & EMGPU_TRACE_ATTEMPTS) L.o_at = put(ld * 4);
    L.bytes = std::max<size_t>(o, kA);
    return L;
}
void trace_bind(const TraceLayout &L, uint32_t want, void *base, emgpu_sample_out *o) {
    char *b = (char *)base;
    memset(o, 0, sizeof *o);
    if (want & EMGPU_TRACE_DENSE) { o->dyn_val = (float *)(b + L.o_dv); o->dyn_bin = (uint32_t *)(b + L.o_db); }
    if (want & EMGPU_TRACE_INIT) { o->init_val = (float *)(b + L.o_iv); o->init_bin = (uint8_t *)(b + L.o_ib); }
    if (want & EMGPU_TRACE_EVENTS) { o->events = (emgpu_event *)(b + L.o_ev); o->ev_count = (uint32_t *)(b + L.o_ec); }
    if (want & EMGPU_TRACE_ATTEMPTS) o->attempts = (int32_t *)(b + L.o_at);
    o->ld = L.ld;
    o->col_offset = 0;
}

struct Events {   // a few HIP events, destroyed on every path out
    std::vector<hipEvent_t> e;
    explicit Events(int n) : e((size_t)n, nullptr) { for (auto &x : e) HIP_OK(hipEventCreate(&x)); }
    ~Events() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
    hipEvent_t operator[](int i) const { return e[(size_t)i]; }
};

// `timed` launches of the caller's call into `o` after `warm` untimed ones: ms per launch (HIP events on the ctx stream)
float time_launches(emgpu_ctx *ctx, const emgpu_model *m, const emgpu_sample_params *p, const emgpu_sample_out *o, int warm, int timed, const Events &ev) {
    auto launch = [&]() {
        const int rc = emgpu_sample_dbn_device(ctx, m, p, o);
        if (rc != EMGPU_OK) throw Error(rc, g_err);
    };
    for (int i = 0; i < warm; i++) launch();
    HIP_OK(hipEventRecord(ev[0], ctx->stream));
    for (int i = 0; i < timed; i++) launch();
    HIP_OK(hipEventRecord(ev[1], ctx->stream));
    HIP_OK(hipEventSynchronize(ev[1]));
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, ev[0], ev[1]));
    return ms / (float)timed;
}

bool is_pinned(const void *p) {
    if (!p) return false;
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof a);
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

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
    size_t target = (size_t)(direct ? 1024 : 256) << 20;   // pinned outputs: larger pieces (the copy engine writes row by row into the caller's pitch)
    if (const char *e = getenv("EMGPU_HOST_CHUNK_MB")) { const long v = atol(e); if (v > 0) target = (size_t)v << 20; }
    size_t C = std::max<size_t>(1024, target / std::max<size_t>(bpt, 1) / 1024 * 1024);
    if (event_cap) C = std::min(C, std::max<size_t>(1024, ((size_t)0xFFFF0000u / event_cap) / 1024 * 1024));
    if (C >= n) C = n;
    else {   // chunks of equal size: the last one is not a sliver (and a staged copy moves whole chunk buffers)
        const size_t k = (n + C - 1) / C;
        C = std::min(C, round_up((n + k - 1) / k, 1024));
    }
    return {n, C, round_up(C, 256), (n + C - 1) / C};
}

// chunk buffers (blocks of the trace pool's allocator, unprobed) and pinned staging buffers of these sizes, one of each for a single chunk, two
// otherwise; the copy stream and h_total.  false: out of device memory
bool provision(emgpu_ctx *ctx, size_t nchunks, size_t dev_bytes, size_t stage_bytes) {
    const size_t nbuf = nchunks == 1 ? 1 : 2;
    for (size_t q = 0; q < nbuf; q++) {
        emgpu_ctx::TraceBlock &b = ctx->chunk_buf[q];
        if (b.bytes >= dev_bytes) continue;
        HIP_OK(hipStreamSynchronize(ctx->stream));
        if (b.p) { device_release(b.p); b = emgpu_ctx::TraceBlock(); }
        // (plain hipMalloc blocks: these buffers are the SOURCE of copies, which is all their placement could matter for -- measured: it does not)
        b = pool_take(ctx, dev_bytes + dev_bytes / 8, nullptr, /*plain=*/true);   // (some headroom: batch sizes that wobble do not reallocate)
        if (!b.p) return false;
    }
    if (ctx->h_stage_cap < stage_bytes) {
        const size_t want_cap = stage_bytes + stage_bytes / 8;
        for (auto &s : ctx->h_stage) { if (s) HIP_OK(hipHostFree(s)); s = nullptr; }
        ctx->h_stage_cap = 0;
        for (size_t b = 0; b < nbuf; b++) HIP_OK(hipHostMalloc(&ctx->h_stage[b], want_cap, hipHostMallocDefault));
        ctx->h_stage_cap = want_cap;
    }
    if (nbuf == 2 && !ctx->h_stage[1]) HIP_OK(hipHostMalloc(&ctx->h_stage[1], ctx->h_stage_cap, hipHostMallocDefault));
    if (!ctx->copy_stream) HIP_OK(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    if (!ctx->h_total) HIP_OK(hipHostMalloc((void **)&ctx->h_total, 4 * sizeof(uint64_t), hipHostMallocDefault));
    return true;
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

void ctx_release_host_side(emgpu_ctx *ctx, bool everything) {
    pool_release(ctx);
    if (everything) { for (void *p : ctx->device_blocks) device_release(p); ctx->device_blocks.clear(); }
    for (auto &b : ctx->chunk_buf) { device_release(b.p); b = emgpu_ctx::TraceBlock(); }
    for (auto &s : ctx->h_stage) { if (s) (void)hipHostFree(s); s = nullptr; }
    ctx->h_stage_cap = 0;
    for (auto it = ctx->host_pool.begin(); it != ctx->host_pool.end();) {
        if (!it->in_use || everything) { (void)hipHostFree(it->p); it = ctx->host_pool.erase(it); }
        else ++it;
    }
    if (everything) {
        if (ctx->h_total) (void)hipHostFree(ctx->h_total);
        ctx->h_total = nullptr;
        if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
        ctx->copy_stream = nullptr;
    }
}

// ------------------------------------------------------------------------------------------------ the file pipeline's text tables, parsed on the device
namespace {
size_t env_size(const char *name, size_t dflt) {
    const char *e = getenv(name);
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (size_t)v : dflt;
}

struct DeviceTable {   // the parsed table: a block of the traces' allocator, released on every path out
    double *d = nullptr;
    int64_t rows = 0, cap_rows = 0;
    uint64_t hard = 0;
    int32_t chunks = 0;
    double h2d_ms = 0, kernel_ms = 0, host_ms = 0;
    DeviceTable() = default;
    DeviceTable(const DeviceTable &) = delete;
    DeviceTable &operator=(const DeviceTable &) = delete;
    ~DeviceTable() { if (d) { (void)hipDeviceSynchronize(); device_release(d); } }
};

int64_t line_of(const char *text, size_t off) {   // 1-based line of byte off
    int64_t line = 1;
    for (const char *q = text, *e = text + off; q < e && (q = (const char *)memchr(q, '\n', (size_t)(e - q))) != nullptr; q++) line++;
    return line;
}

// text [nbytes] -> T.d [T.rows][ncol] on the device.  The text goes up in chunks cut behind a newline (EMGPU_HOST_CHUNK_MB, or
// EMGPU_DEBUG_PARSE_CHUNK_BYTES for tests that want the cuts at every position of a row), chunk k + 1's copy on the copy stream behind chunk k's
// parse; pageable text through the pinned staging buffers.  Offsets within a chunk are 32-bit, offsets into the text and rows 64-bit.
// Hard tokens (emgpu_kernels_parse.hip) are finished here with strtod; a chunk with more of them than the list holds (EMGPU_DEBUG_PARSE_HARD_CAP
// entries, default 65 536) is parsed again with a list of the counted size.  Throws Error(EMGPU_ERR_PARSE) naming the first malformed line.
void parse_to_device(emgpu_ctx *ctx, const char *what, const char *text, size_t nbytes, int ncol, DeviceTable &T) {
    T.cap_rows = (int64_t)(nbytes / (2 * (size_t)ncol)) + 1;   // a row of ncol numbers is at least 2 ncol - 1 bytes and what ends its line
    const size_t table_bytes = std::max<size_t>((size_t)T.cap_rows * (size_t)ncol * 8, 256);
    void *tp = nullptr;
    if (!device_block(table_bytes, &tp)) {
        HIP_OK(hipStreamSynchronize(ctx->stream));
        pool_release(ctx);
        if (!device_block(table_bytes, &tp))
            throw Error(EMGPU_ERR_HIP, std::string(what) + ": the parsed table (" + std::to_string(table_bytes) + " bytes) does not fit the device's memory");
    }
    T.d = (double *)tp;
    if (!nbytes) return;
    // ---- the cuts
    size_t target = (size_t)256 << 20;
    if (const char *e = getenv("EMGPU_HOST_CHUNK_MB")) { const long v = atol(e); if (v > 0) target = (size_t)v << 20; }
    target = std::min<size_t>(env_size("EMGPU_DEBUG_PARSE_CHUNK_BYTES", target), (size_t)0xC0000000u);
    std::vector<size_t> cut{0};
    size_t maxc = 0;
    while (cut.back() < nbytes) {
        const size_t a = cut.back();
        size_t b = nbytes;
        if (nbytes - a > target) {
            const void *q = memrchr(text + a, '\n', target);
            if (!q) q = memchr(text + a + target, '\n', nbytes - a - target);   // a line longer than a chunk: the chunk ends with it
            b = q ? (size_t)((const char *)q - text) + 1 : nbytes;
        }
        if (b - a > (size_t)0xFFFFFF00u) throw Error(EMGPU_ERR_ARG, std::string(what) + ": a line of more than 4 GB: a chunk's offsets would not fit 32 bits");
        maxc = std::max(maxc, b - a);
        cut.push_back(b);
    }
    const size_t nchunks = cut.size() - 1;
    T.chunks = (int32_t)nchunks;
    const size_t tiles_max = (maxc + emgpu::kParseTile - 1) / emgpu::kParseTile;
    const size_t hard_cap = env_size("EMGPU_DEBUG_PARSE_HARD_CAP", 65536);
    size_t o = 0;
    auto put = [&](size_t bytes) { const size_t at = o; o = round_up(o + std::max<size_t>(bytes, 1), 256); return at; };
    const size_t o_text = put(maxc + 8), o_cnt = put(tiles_max * 4), o_scr = put(emgpu::pack_scratch_words((int64_t)tiles_max) * 4);
    const size_t o_hard = put(hard_cap * sizeof(emgpu::EmgpuHardToken)), o_val = put(hard_cap * 8), o_misc = put(16);   // misc: err (u64), hard count (u32)
    const bool pinned = is_pinned(text);
    if (!provision(ctx, nchunks, o, pinned ? 256 : maxc)) throw Error(EMGPU_ERR_HIP, std::string(what) + ": out of device memory");
    Events ev(8);   // per buffer b: 4b + {copy start, copy end, parse start, parse end}
    auto upload = [&](size_t k) {
        const int b = (int)(k & 1);
        const char *src = text + cut[k];
        const size_t len = cut[k + 1] - cut[k];
        if (!pinned) { const auto t0 = Clock::now(); memcpy(ctx->h_stage[b], src, len); src = (const char *)ctx->h_stage[b]; T.host_ms += ms_since(t0); }
        HIP_OK(hipEventRecord(ev[4 * b], ctx->copy_stream));
        HIP_OK(hipMemcpyAsync((char *)ctx->chunk_buf[b].p + o_text, src, len, hipMemcpyHostToDevice, ctx->copy_stream));
        HIP_OK(hipEventRecord(ev[4 * b + 1], ctx->copy_stream));
    };
    struct Extra { void *p = nullptr; ~Extra() { if (p) (void)hipFree(p); } };
    try {
        HIP_OK(hipStreamSynchronize(ctx->stream));   // (the chunk buffers may still be read by an earlier call's copies)
        HIP_OK(hipStreamSynchronize(ctx->copy_stream));
        upload(0);
        for (size_t k = 0; k < nchunks; k++) {
            const int b = (int)(k & 1);
            char *dev = (char *)ctx->chunk_buf[b].p;
            const size_t len = cut[k + 1] - cut[k];
            emgpu::EmgpuParseRun P{};
            P.text = (const uint8_t *)(dev + o_text); P.nbytes = (uint32_t)len; P.ncol = ncol;
            P.cnt = (uint32_t *)(dev + o_cnt); P.scratch = (uint32_t *)(dev + o_scr);
            P.table = T.d; P.row_base = T.rows; P.table_rows = T.cap_rows;
            P.hard = (emgpu::EmgpuHardToken *)(dev + o_hard); P.hard_cap = (uint32_t)hard_cap;
            P.err = (unsigned long long *)(dev + o_misc); P.hard_count = (uint32_t *)(dev + o_misc + 8);
            HIP_OK(hipStreamWaitEvent(ctx->stream, ev[4 * b + 1], 0));
            HIP_OK(hipEventRecord(ev[4 * b + 2], ctx->stream));
            HIP_OK(hipMemsetAsync(dev + o_misc, 0xFF, 8, ctx->stream));
            HIP_OK(hipMemsetAsync(dev + o_misc + 8, 0, 8, ctx->stream));
            launch_ok(emgpu::launch_parse_count(P, ctx->stream));
            HIP_OK(hipMemcpyAsync(&ctx->h_total[2 * b], P.scratch, 8, hipMemcpyDeviceToHost, ctx->stream));
            if (k + 1 < nchunks) upload(k + 1);   // (its buffer's last reader, chunk k - 1's parse, has been waited for)
            HIP_OK(hipStreamSynchronize(ctx->stream));
            const uint64_t rows = ctx->h_total[2 * b];
            P.rows = (uint32_t)rows;
            launch_ok(emgpu::launch_parse_rows(P, ctx->stream));
            HIP_OK(hipMemcpyAsync(&ctx->h_total[2 * b], dev + o_misc, 16, hipMemcpyDeviceToHost, ctx->stream));
            HIP_OK(hipEventRecord(ev[4 * b + 3], ctx->stream));
            HIP_OK(hipStreamSynchronize(ctx->stream));
            const uint64_t err = ctx->h_total[2 * b];
            if (err != ~0ull)
                throw Error(EMGPU_ERR_PARSE, std::string(what) + ": line " + std::to_string(line_of(text, cut[k] + (size_t)err)) + " is not a row of " +
                                                 std::to_string(ncol) + " numbers");
            if (T.rows + (int64_t)rows > T.cap_rows) throw Error(EMGPU_ERR_PARSE, std::string(what) + ": more rows than the text has room for");
            const uint32_t nh = (uint32_t)ctx->h_total[2 * b + 1];
            Extra extra;
            const emgpu::EmgpuHardToken *d_list = P.hard;
            double *d_val = (double *)(dev + o_val);
            if (nh > hard_cap) {   // the list was too small: once more with one of the counted size (the values written meanwhile are the same)
                HIP_OK(hipMalloc(&extra.p, (size_t)nh * 24));
                P.hard = (emgpu::EmgpuHardToken *)extra.p; P.hard_cap = nh;
                d_list = P.hard; d_val = (double *)((char *)extra.p + (size_t)nh * 16);
                HIP_OK(hipMemsetAsync(dev + o_misc + 8, 0, 8, ctx->stream));
                launch_ok(emgpu::launch_parse_rows(P, ctx->stream));
                HIP_OK(hipStreamSynchronize(ctx->stream));
            }
            if (nh) {
                const auto t0 = Clock::now();
                std::vector<emgpu::EmgpuHardToken> list(nh);
                std::vector<double> val(nh);
                HIP_OK(hipMemcpy(list.data(), d_list, (size_t)nh * 16, hipMemcpyDeviceToHost));
                std::string tok;
                for (uint32_t i = 0; i < nh; i++) {
                    const char *q = text + cut[k] + list[i].off, *e = text + cut[k + 1], *r = q;
                    while (r < e && *r != ' ' && *r != '\t' && *r != '\n' && *r != '\r') r++;
                    tok.assign(q, r);
                    val[i] = strtod(tok.c_str(), nullptr);
                }
                HIP_OK(hipMemcpyAsync(d_val, val.data(), (size_t)nh * 8, hipMemcpyHostToDevice, ctx->stream));
                launch_ok(emgpu::launch_parse_patch(T.d, d_list, d_val, nh, ctx->stream));
                HIP_OK(hipStreamSynchronize(ctx->stream));
                T.host_ms += ms_since(t0);
            }
            float ms = 0.f;
            HIP_OK(hipEventElapsedTime(&ms, ev[4 * b], ev[4 * b + 1])); T.h2d_ms += ms;
            HIP_OK(hipEventElapsedTime(&ms, ev[4 * b + 2], ev[4 * b + 3])); T.kernel_ms += ms;
            T.rows += (int64_t)rows;
            T.hard += nh;
        }
    } catch (...) {
        (void)hipStreamSynchronize(ctx->stream);
        if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
        throw;
    }
}
} // namespace

extern "C" {

// ================================================================================================ the trace pool
int emgpu_trace_alloc(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_sample_params *p, uint32_t want, int32_t candidates, emgpu_trace **out) {
    EMGPU_TRY
    if (!ctx || !h || !p || !out) return fail(EMGPU_ERR_ARG, "null argument");
    if (p->n < 0 || p->sample_time < 1) return fail(EMGPU_ERR_ARG, "n < 0 or sample_time < 1");
    if (!(want & (EMGPU_TRACE_INIT | EMGPU_TRACE_DENSE | EMGPU_TRACE_EVENTS | EMGPU_TRACE_ATTEMPTS)) || (want & ~15u)) return fail(EMGPU_ERR_ARG, "want: a combination of EMGPU_TRACE_*");
    if ((want & EMGPU_TRACE_EVENTS) && p->event_cap < 1) return fail(EMGPU_ERR_ARG, "EMGPU_TRACE_EVENTS needs event_cap >= 1");
    if (candidates < 0 || candidates > 8) return fail(EMGPU_ERR_ARG, "candidates outside 0..8");
    CTX_LOCK(ctx);
    HIP_OK(hipSetDevice(ctx->device));
    const TraceLayout L = trace_layout(h->m, p, want);
    std::unique_ptr<emgpu_trace> t(new emgpu_trace());
    t->rep.bytes = (int64_t)L.bytes;
    t->rep.ld = L.ld;
    const bool automatic = candidates == 0;
    int target = automatic ? (L.bytes < ((size_t)1 << 30) ? 1 : 6) : candidates;   // (no early stop: a candidate costs a quarter of a second, and two
    if (p->n == 0) target = 1;                                                      //  medium ones that agree say nothing about a fast one further on)

    bool from_pool = false;
    std::vector<emgpu_ctx::TraceBlock> cands;
    // candidate 0 of a probe is what hipMalloc hands a caller (the report's first_allocation_ms); the others are the library's own kind
    cands.push_back(pool_take(ctx, L.bytes, &from_pool, /*plain=*/target > 1));
    if (!cands[0].p) return fail(EMGPU_ERR_HIP, "emgpu_trace_alloc: out of device memory (" + std::to_string(L.bytes) + " bytes)");
    auto give_up = [&]() { for (auto &c : cands) device_release(c.p); cands.clear(); };
    try {
        if (from_pool && (cands[0].probed || target == 1)) {   // placed by an earlier call (or the caller does not want a probe): take it as it is
            t->rep.candidates = 1;
            t->rep.reused = 1;
            t->rep.kept_ms = cands[0].ms;
        } else if (target == 1) {
            t->rep.candidates = 1;
        } else {
            auto room_for_one_more = [&]() {
                size_t fr = 0, tot = 0;
                if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); return false; }
                return fr >= L.bytes + ((size_t)4 << 30);
            };
            auto one_more = [&]() {
                if (!room_for_one_more()) return false;
                emgpu_ctx::TraceBlock b;
                if (!device_block(L.bytes, &b.p)) return false;   // (another process took the memory meanwhile)
                b.bytes = L.bytes;
                cands.push_back(b);
                return true;
            };
            while ((int)cands.size() < target && one_more()) {}
            if (cands.size() == 1) {
                t->rep.candidates = 1;   // no memory for a second candidate
            } else {
                Events ev(2);
                std::vector<emgpu_sample_out> outs(cands.size());
                for (size_t i = 0; i < cands.size(); i++) trace_bind(L, want, cands[i].p, &outs[i]);
                // the allocations above left the device idle and its clocks fell: load it first
                const auto t0 = Clock::now();
                while (ms_since(t0) < 500.0) (void)time_launches(ctx, h, p, &outs.back(), 0, 4, ev);
                std::vector<float> ms(cands.size(), 1e30f);
                for (int round = 0; round < 2; round++)   // a b c a b c: what is left of a ramp does not favour the last one
                    for (size_t i = 0; i < cands.size(); i++) ms[i] = std::min(ms[i], time_launches(ctx, h, p, &outs[i], 2, 5, ev));
                const size_t kept = (size_t)(std::min_element(ms.begin(), ms.end()) - ms.begin());
                t->rep.candidates = (int32_t)cands.size();
                t->rep.kept = (int32_t)kept;
                for (size_t i = 0; i < cands.size() && i < 8; i++) t->rep.ms[i] = ms[i];
                t->rep.first_allocation_ms = ms[0];
                t->rep.kept_ms = ms[kept];
                // the probe's launches may have left deferred per-trajectory bits (a rejection cap ...): the caller's own call will raise them again
                const int rc = emgpu_ctx_sync(ctx);
                if (rc == EMGPU_ERR_HIP) throw Error(rc, g_err);
                for (size_t i = 0; i < cands.size(); i++)
                    if (i != kept) device_release(cands[i].p);
                emgpu_ctx::TraceBlock k = cands[kept];
                k.probed = true;
                k.ms = ms[kept];
                cands.assign(1, k);
            }
        }
    } catch (...) {
        (void)hipStreamSynchronize(ctx->stream);
        give_up();
        throw;
    }
    t->blk = cands[0];
    trace_bind(L, want, t->blk.p, &t->out);
    *out = t.release();
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_trace_out(const emgpu_trace *t, emgpu_sample_out *out) {
    if (!t || !out) return fail(EMGPU_ERR_ARG, "null argument");
    *out = t->out;
    return EMGPU_OK;
}

int emgpu_trace_report(const emgpu_trace *t, emgpu_trace_report_t *out) {
    if (!t || !out) return fail(EMGPU_ERR_ARG, "null argument");
    *out = t->rep;
    return EMGPU_OK;
}

int emgpu_trace_free(emgpu_ctx *ctx, emgpu_trace *t) {
    EMGPU_TRY
    if (!t) return EMGPU_OK;
    if (!ctx) return fail(EMGPU_ERR_ARG, "null ctx");
    CTX_LOCK(ctx);
    HIP_OK(hipSetDevice(ctx->device));
    HIP_OK(hipStreamSynchronize(ctx->stream));   // nothing in flight may still write the block when somebody else takes it
    ctx->trace_pool.push_back(t->blk);
    delete t;
    return EMGPU_OK;
    EMGPU_CATCH
}

// Plain device memory from the same allocator as the traces (no probe): for outputs that are not a DBN trace -- the joined tracks of
// emgpu_sample_terminal_device, a consumer's own buffers.
int emgpu_device_alloc(emgpu_ctx *ctx, uint64_t bytes, void **out) {
    EMGPU_TRY
    if (!ctx || !out) return fail(EMGPU_ERR_ARG, "null argument");
    CTX_LOCK(ctx);
    HIP_OK(hipSetDevice(ctx->device));
    void *p = nullptr;
    const size_t need = std::max<size_t>((size_t)bytes, 256);
    if (!device_block(need, &p)) {
        HIP_OK(hipStreamSynchronize(ctx->stream));
        pool_release(ctx);
        if (!device_block(need, &p)) return fail(EMGPU_ERR_HIP, "emgpu_device_alloc: out of device memory (" + std::to_string(need) + " bytes)");
    }
    ctx->device_blocks.insert(p);
    *out = p;
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_device_free(emgpu_ctx *ctx, void *p) {
    EMGPU_TRY
    if (!p) return EMGPU_OK;
    if (!ctx) return fail(EMGPU_ERR_ARG, "null ctx");
    CTX_LOCK(ctx);
    if (!ctx->device_blocks.erase(p)) return fail(EMGPU_ERR_ARG, "emgpu_device_free: not a block of this ctx");
    HIP_OK(hipSetDevice(ctx->device));
    HIP_OK(hipStreamSynchronize(ctx->stream));
    device_release(p);
    return EMGPU_OK;
    EMGPU_CATCH
}

// ================================================================================================ the pinned pool
int emgpu_host_alloc(emgpu_ctx *ctx, uint64_t bytes, void **out) {
    EMGPU_TRY
    if (!ctx || !out) return fail(EMGPU_ERR_ARG, "null argument");
    CTX_LOCK(ctx);
    HIP_OK(hipSetDevice(ctx->device));
    const size_t need = std::max<size_t>((size_t)bytes, 64);   // (portable: emgpu_sample_dbn_multi_host hands one caller array to the contexts of several devices)
    emgpu_ctx::HostBlock *best = nullptr;
    for (auto &b : ctx->host_pool)
        if (!b.in_use && b.bytes >= need && b.bytes <= need + need / 2 + (1u << 20) && (!best || b.bytes < best->bytes)) best = &b;
    if (best) {
        best->in_use = true;
        *out = best->p;
        return EMGPU_OK;
    }
    void *p = nullptr;
    if (hipHostMalloc(&p, need, hipHostMallocPortable) != hipSuccess) {
        (void)hipGetLastError();
        for (auto it = ctx->host_pool.begin(); it != ctx->host_pool.end();)   // the pool's idle blocks first, then once more
            if (!it->in_use) { (void)hipHostFree(it->p); it = ctx->host_pool.erase(it); } else ++it;
        HIP_OK(hipHostMalloc(&p, need, hipHostMallocPortable));
    }
    ctx->host_pool.push_back({p, need, true});
    *out = p;
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_host_free(emgpu_ctx *ctx, void *p) {
    if (!p) return EMGPU_OK;
    if (!ctx) return fail(EMGPU_ERR_ARG, "null ctx");
    CTX_LOCK(ctx);
    for (auto &b : ctx->host_pool)
        if (b.p == p) {
            if (!b.in_use) return fail(EMGPU_ERR_ARG, "emgpu_host_free: block freed twice");
            b.in_use = false;
            // the pool keeps at most 16 GiB of idle pinned memory (callers that wander through many sizes would pin the host's RAM away)
            size_t idle = 0;
            for (const auto &q : ctx->host_pool) idle += q.in_use ? 0 : q.bytes;
            if (idle > ((size_t)16 << 30)) {
                (void)hipSetDevice(ctx->device);
                for (auto it = ctx->host_pool.begin(); it != ctx->host_pool.end();)
                    if (!it->in_use && it->p != p) { (void)hipHostFree(it->p); it = ctx->host_pool.erase(it); } else ++it;
            }
            return EMGPU_OK;
        }
    return fail(EMGPU_ERR_ARG, "emgpu_host_free: not a block of this ctx");
}

int emgpu_host_stats(const emgpu_ctx *ctx, emgpu_host_stats_t *out) {
    if (!ctx || !out) return fail(EMGPU_ERR_ARG, "null argument");
    *out = ctx->host_stats;
    return EMGPU_OK;
}

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
    CTX_LOCK(ctx);
    HIP_OK(hipSetDevice(ctx->device));
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
    CTX_LOCK(ctx);
    HIP_OK(hipSetDevice(ctx->device));
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
    CTX_LOCK(ctx);
    HIP_OK(hipSetDevice(ctx->device));
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

int emgpu_format_g_host(emgpu_ctx *ctx, const float *x, int64_t n, char *out, int64_t cap, uint64_t *offsets) {
    EMGPU_TRY
    if (!ctx || !offsets || (n > 0 && !x) || (cap > 0 && !out)) return fail(EMGPU_ERR_ARG, "null argument");
    if (n < 0 || cap < 0) return fail(EMGPU_ERR_ARG, "n < 0 or cap < 0");
    CTX_LOCK(ctx);
    HIP_OK(hipSetDevice(ctx->device));
    offsets[0] = 0;
    if (n == 0) return EMGPU_OK;
    const size_t C = (size_t)std::min<int64_t>(n, (int64_t)1 << 22);   // values per pass: their text is counted in 32 bits (12 C bytes)
    uint64_t total = 0, paths[2] = {0, 0};
    {
        CallBuffers B(ctx);
        float *d_x = B.alloc<float>(C * 4);
        uint32_t *d_cnt = B.alloc<uint32_t>(C * 4), *d_scr = B.alloc<uint32_t>(emgpu::pack_scratch_words((int64_t)C) * 4);
        char *d_text = B.alloc<char>(C * 12);
        uint64_t *d_off = B.alloc<uint64_t>(C * 8);
        unsigned long long *d_paths = B.alloc<unsigned long long>(16);
        HIP_OK(hipMemsetAsync(d_paths, 0, 16, ctx->stream));
        for (size_t k0 = 0; k0 < (size_t)n; k0 += C) {
            const size_t c = std::min(C, (size_t)n - k0);
            B.up(d_x, x + k0, c * 4);
            launch_ok(emgpu::launch_format_g(d_x, (int64_t)c, d_cnt, d_scr, d_text, total, d_off, d_paths, ctx->stream));
            uint64_t bytes = 0;
            B.down(&bytes, d_scr, sizeof bytes);
            B.down(offsets + k0, d_off, c * 8);
            HIP_OK(hipStreamSynchronize(ctx->stream));
            if (bytes > c * 12) throw Error(EMGPU_ERR_HIP, "emgpu_format_g_host: a pass's text outgrew its bound");
            if (total + bytes <= (uint64_t)cap) { B.down(out + total, d_text, (size_t)bytes); HIP_OK(hipStreamSynchronize(ctx->stream)); }
            total += bytes;
        }
        B.down(paths, d_paths, sizeof paths);
        HIP_OK(hipStreamSynchronize(ctx->stream));
    }
    ctx->format_paths[0] += paths[0];
    ctx->format_paths[1] += paths[1];
    offsets[n] = total;
    if (total > (uint64_t)cap) return fail(EMGPU_ERR_EVENT_CAP, "emgpu_format_g_host: the text has " + std::to_string(total) + " bytes, cap is " + std::to_string(cap));
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_debug_format_paths(emgpu_ctx *ctx, uint64_t out[2]) {
    if (!ctx || !out) return fail(EMGPU_ERR_ARG, "null argument");
    CTX_LOCK(ctx);
    out[0] = ctx->format_paths[0]; out[1] = ctx->format_paths[1];
    ctx->format_paths[0] = ctx->format_paths[1] = 0;
    return EMGPU_OK;
}

// ================================================================================================ sample2track's files
int64_t emgpu_csv_bound(int64_t n, int64_t rows) { return n < 0 || rows < 0 ? -1 : 22 * n + 74 * rows; }

int emgpu_parse_table_host(emgpu_ctx *ctx, const char *text, int64_t nbytes, int32_t ncol, double *out, int64_t rows_cap, int64_t *rows, uint64_t *hard_tokens) {
    EMGPU_TRY
    if (!ctx || !rows || (nbytes > 0 && !text) || (rows_cap > 0 && !out)) return fail(EMGPU_ERR_ARG, "null argument");
    if (nbytes < 0 || rows_cap < 0 || ncol < 1 || ncol > 4096) return fail(EMGPU_ERR_ARG, "nbytes < 0, rows_cap < 0 or ncol outside 1..4096");
    CTX_LOCK(ctx);
    HIP_OK(hipSetDevice(ctx->device));
    *rows = 0;
    if (hard_tokens) *hard_tokens = 0;
    DeviceTable T;
    parse_to_device(ctx, "emgpu_parse_table_host", text, (size_t)nbytes, ncol, T);
    *rows = T.rows;
    if (hard_tokens) *hard_tokens = T.hard;
    if (T.rows > rows_cap) return fail(EMGPU_ERR_EVENT_CAP, "emgpu_parse_table_host: the text has " + std::to_string(T.rows) + " rows, rows_cap is " + std::to_string(rows_cap));
    if (T.rows) HIP_OK(hipMemcpy(out, T.d, (size_t)T.rows * (size_t)ncol * 8, hipMemcpyDeviceToHost));
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_format_f0_host(emgpu_ctx *ctx, const double *x, int64_t n, char *out, int64_t cap, uint64_t *offsets) {
    EMGPU_TRY
    if (!ctx || !offsets || (n > 0 && !x) || (cap > 0 && !out)) return fail(EMGPU_ERR_ARG, "null argument");
    if (n < 0 || cap < 0) return fail(EMGPU_ERR_ARG, "n < 0 or cap < 0");
    CTX_LOCK(ctx);
    HIP_OK(hipSetDevice(ctx->device));
    offsets[0] = 0;
    if (n == 0) return EMGPU_OK;
    const size_t C = (size_t)std::min<int64_t>(n, (int64_t)1 << 22);   // values per pass: their text is counted in 32 bits (20 C bytes)
    uint64_t total = 0;
    {
        CallBuffers B(ctx);
        double *d_x = B.alloc<double>(C * 8);
        uint32_t *d_cnt = B.alloc<uint32_t>(C * 4), *d_scr = B.alloc<uint32_t>(emgpu::pack_scratch_words((int64_t)C) * 4);
        char *d_text = B.alloc<char>(C * 20);
        uint64_t *d_off = B.alloc<uint64_t>(C * 8);
        for (size_t k0 = 0; k0 < (size_t)n; k0 += C) {
            const size_t c = std::min(C, (size_t)n - k0);
            B.up(d_x, x + k0, c * 8);
            launch_ok(emgpu::launch_format_f0(d_x, (int64_t)c, d_cnt, d_scr, d_text, total, d_off, ctx->stream));
            uint64_t bytes = 0;
            B.down(&bytes, d_scr, sizeof bytes);
            B.down(offsets + k0, d_off, c * 8);
            HIP_OK(hipStreamSynchronize(ctx->stream));
            if (bytes > c * 20) throw Error(EMGPU_ERR_HIP, "emgpu_format_f0_host: a pass's text outgrew its bound");
            if (total + bytes <= (uint64_t)cap) { B.down(out + total, d_text, (size_t)bytes); HIP_OK(hipStreamSynchronize(ctx->stream)); }
            total += bytes;
        }
    }
    offsets[n] = total;
    if (total > (uint64_t)cap) return fail(EMGPU_ERR_EVENT_CAP, "emgpu_format_f0_host: the text has " + std::to_string(total) + " bytes, cap is " + std::to_string(cap));
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_tracks_text_host(emgpu_ctx *ctx, const emgpu_track_params *p, const emgpu_tracks_text_in *in, const emgpu_tracks_text_out *out) {
    EMGPU_TRY
    if (!ctx || !p || !in || !out) return fail(EMGPU_ERR_ARG, "null argument");
    if (!out->totals || !out->flags) return fail(EMGPU_ERR_ARG, "flags and totals are required");
    if (p->n < 0 || in->nbytes < 0 || (in->nbytes > 0 && !in->text)) return fail(EMGPU_ERR_ARG, "n < 0, or no text");
    if (p->n > 0 && (!in->id || !in->alt0 || !in->speed0)) return fail(EMGPU_ERR_ARG, "id, alt0 and speed0 are required");
    if (p->n > 0x7FFFFFFF) return fail(EMGPU_ERR_ARG, "more than 2^31 - 1 tracks in one call");
    if (in->ncol < 2 || in->ncol > 4096) return fail(EMGPU_ERR_ARG, "ncol outside 2..4096");
    for (int32_t c : {in->col_vertrate, in->col_acc, in->col_turnrate})
        if (c < 0 || c >= in->ncol) return fail(EMGPU_ERR_ARG, "an update column outside 0..ncol-1");
    if (out->csv_cap < 0 || out->xyz_cap < 0 || (out->csv && !out->offsets)) return fail(EMGPU_ERR_ARG, "csv_cap / xyz_cap < 0, or csv without offsets");
    CTX_LOCK(ctx);
    HIP_OK(hipSetDevice(ctx->device));
    const auto t_call = Clock::now();
    const size_t n = (size_t)p->n;
    const int ncol = in->ncol;
    for (int k = 0; k < 5; k++) out->totals[k] = 0;
    emgpu_host_stats_t st{};
    double phase[6] = {0, 0, 0, 0, 0, 0};   // upload, parse kernels, grouping + track kernels, CSV kernels, download, host work
    DeviceTable T;
    parse_to_device(ctx, "emgpu_tracks_text_host", in->text, (size_t)in->nbytes, ncol, T);
    const int64_t R = T.rows;
    out->totals[1] = R;
    out->totals[2] = (int64_t)T.hard;
    phase[0] = T.h2d_ms; phase[1] = T.kernel_ms; phase[5] = T.host_ms;
    st.chunks = T.chunks; st.threads = 1; st.direct = (is_pinned(in->text) && (!out->csv || is_pinned(out->csv))) ? 1 : 0;
    int rc = EMGPU_OK;
    uint64_t csv_total = 0, xyz_rows = 0;
    {
        CallBuffers B(ctx);
        Events ev(6);
        const size_t n1 = std::max<size_t>(n, 1);
        double *d_in = B.alloc<double>(3 * n1 * 8), *d_vmm = B.alloc<double>(2 * n1 * 8);
        int64_t *d_first = B.alloc<int64_t>(n1 * 8);
        int32_t *d_len = B.alloc<int32_t>(n1 * 4);
        uint8_t *d_flags = B.alloc<uint8_t>(n1);
        uint64_t *d_xoff = B.alloc<uint64_t>((n1 + 1) * 8);
        B.up(d_in, in->id, n * 8); B.up(d_in + n, in->alt0, n * 8); B.up(d_in + 2 * n, in->speed0, n * 8);
        // ---- the runs of equal ids, and every wanted id's run
        HIP_OK(hipEventRecord(ev[0], ctx->stream));
        emgpu::EmgpuRunTable G{};
        G.table = T.d; G.ncol = ncol; G.R = R;
        G.cnt = B.alloc<uint32_t>(std::max<size_t>((size_t)R, 1) * 4);
        G.scratch = B.alloc<uint32_t>(emgpu::pack_scratch_words(R) * 4);
        launch_ok(emgpu::launch_run_mark(G, ctx->stream));
        uint64_t runs = 0;
        B.down(&runs, G.scratch, 8);
        HIP_OK(hipStreamSynchronize(ctx->stream));
        if (runs >= 0x7FFFFFFFull) return fail(EMGPU_ERR_ARG, "emgpu_tracks_text_host: more than 2^31 - 1 runs of ids");
        size_t H = 16;
        while (H < 2 * runs) H <<= 1;
        G.run_id = B.alloc<double>(std::max<size_t>(runs, 1) * 8); G.run_first = B.alloc<int64_t>(std::max<size_t>(runs, 1) * 8);
        G.keys = B.alloc<unsigned long long>(H * 8); G.vals = B.alloc<uint32_t>(H * 4); G.mask = (uint32_t)(H - 1);
        G.dup = B.alloc<uint32_t>(4);
        HIP_OK(hipMemsetAsync(G.keys, 0xFF, H * 8, ctx->stream));
        HIP_OK(hipMemsetAsync(G.dup, 0, 4, ctx->stream));
        launch_ok(emgpu::launch_run_fill(G, ctx->stream));
        launch_ok(emgpu::launch_run_match(G, (uint32_t)runs, (int64_t)n, d_in, d_first, d_len, ctx->stream));
        uint32_t dup = 0;
        std::vector<int32_t> len(n);
        B.down(&dup, G.dup, 4);
        B.down(len.data(), d_len, n * 4);
        HIP_OK(hipStreamSynchronize(ctx->stream));
        const int64_t *d_rowidx = nullptr;
        if (dup) {   // an id owns more than one run: the reference's selection (every row with that id, in file order) through a stable sort on the host
            const auto t0 = Clock::now();
            out->totals[4] = 1;
            std::vector<double> ids((size_t)R);
            HIP_OK(hipMemcpy2D(ids.data(), 8, T.d, (size_t)ncol * 8, 8, (size_t)R, hipMemcpyDeviceToHost));
            std::vector<int64_t> order;
            order.reserve((size_t)R);
            for (int64_t r = 0; r < R; r++) if (ids[(size_t)r] == ids[(size_t)r]) order.push_back(r);
            std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return ids[(size_t)a] < ids[(size_t)b]; });
            std::vector<int64_t> first(n), rowidx;
            for (size_t i = 0; i < n; i++) {
                const double id = in->id[i];
                first[i] = (int64_t)rowidx.size();
                if (id == id) {
                    auto lo = std::lower_bound(order.begin(), order.end(), id, [&](int64_t a, double v) { return ids[(size_t)a] < v; });
                    for (; lo != order.end() && ids[(size_t)*lo] == id; ++lo) rowidx.push_back(*lo);
                }
                const int64_t l = (int64_t)rowidx.size() - first[i];
                if (l > 0x7FFFFFFF) return fail(EMGPU_ERR_ARG, "emgpu_tracks_text_host: a track of more than 2^31 - 1 rows");
                len[i] = (int32_t)l;
            }
            int64_t *d_ri = B.alloc<int64_t>(std::max<size_t>(rowidx.size(), 1) * 8);
            B.up(d_ri, rowidx.data(), rowidx.size() * 8);
            B.up(d_first, first.data(), n * 8);
            B.up(d_len, len.data(), n * 4);
            HIP_OK(hipStreamSynchronize(ctx->stream));   // (the vectors go out of scope)
            d_rowidx = d_ri;
            phase[5] += ms_since(t0);
        }
        std::vector<uint64_t> xoff(n + 1, 0);
        for (size_t i = 0; i < n; i++) {
            if (len[i] > 50000000) return fail(EMGPU_ERR_ARG, "emgpu_tracks_text_host: a track of more than 50 000 000 rows: its file would not fit 32 bits");
            xoff[i + 1] = xoff[i] + (uint64_t)len[i] + 1;
        }
        xyz_rows = xoff[n];
        if (out->lengths) memcpy(out->lengths, len.data(), n * 4);
        // ---- the tracks
        const bool want_csv = out->offsets != nullptr, want_xyz = want_csv || out->xyz;
        double *d_xyz = nullptr;
        if (want_xyz) {
            void *q = nullptr;
            if (hipMalloc(&q, std::max<size_t>((size_t)xyz_rows * 24, 256)) != hipSuccess) {
                (void)hipGetLastError();
                return fail(EMGPU_ERR_HIP, "emgpu_tracks_text_host: the positions (" + std::to_string(xyz_rows * 24) + " bytes) do not fit the device's memory");
            }
            d_xyz = (double *)q;
        }
        struct Free { void *p; ~Free() { if (p) { (void)hipDeviceSynchronize(); (void)hipFree(p); } } } free_xyz{d_xyz};
        B.up(d_xoff, xoff.data(), (n + 1) * 8);
        emgpu::EmgpuTrackTableRun A{};
        A.n = (int64_t)n;
        set_track_units(A, p);
        A.alt0 = d_in + n; A.speed0 = d_in + 2 * n;
        A.table = T.d; A.ncol = ncol; A.c_vr = in->col_vertrate; A.c_acc = in->col_acc; A.c_tr = in->col_turnrate;
        A.first = d_first; A.len = d_len; A.rowidx = d_rowidx; A.xoff = d_xoff; A.xyz = d_xyz; A.flags = d_flags; A.vmm = d_vmm;
        const char *name = "";
        const hipError_t e = emgpu::launch_sample2track_table(A, ctx->stream, &name);
        ctx->last_kernel = name;
        launch_ok(e);
        HIP_OK(hipEventRecord(ev[1], ctx->stream));
        B.down(out->flags, d_flags, n);
        B.down(out->speed_minmax, d_vmm, 2 * n * 8);
        // ---- the files
        std::vector<uint64_t> off(n + 1, 0);
        struct Free free_csv{nullptr};
        if (want_csv) {
            emgpu::EmgpuCsvRun C{};
            C.n = (int64_t)n; C.flags = d_flags; C.len = d_len; C.xoff = d_xoff; C.xyz = d_xyz;
            C.cnt = B.alloc<uint32_t>(n1 * 4); C.hostfmt = B.alloc<uint8_t>(n1);
            HIP_OK(hipEventRecord(ev[2], ctx->stream));
            launch_ok(emgpu::launch_csv_len(C, ctx->stream));
            HIP_OK(hipEventRecord(ev[3], ctx->stream));
            std::vector<uint32_t> cnt(n);
            std::vector<uint8_t> hostfmt(n);
            B.down(cnt.data(), C.cnt, n * 4);
            B.down(hostfmt.data(), C.hostfmt, n);
            HIP_OK(hipStreamSynchronize(ctx->stream));
            for (size_t i = 0; i < n; i++) { off[i + 1] = off[i] + cnt[i]; out->totals[3] += hostfmt[i]; }
            csv_total = off[n];
            memcpy(out->offsets, off.data(), (n + 1) * 8);
            float ms = 0.f;
            HIP_OK(hipEventElapsedTime(&ms, ev[2], ev[3])); phase[3] += ms;
            if (out->csv && csv_total && csv_total <= (uint64_t)out->csv_cap) {
                void *q = nullptr;
                if (hipMalloc(&q, (size_t)csv_total + 8) != hipSuccess) {
                    (void)hipGetLastError();
                    return fail(EMGPU_ERR_HIP, "emgpu_tracks_text_host: the CSV text (" + std::to_string(csv_total) + " bytes) does not fit the device's memory");
                }
                free_csv.p = q;
                uint64_t *d_off = B.alloc<uint64_t>(n1 * 8);
                B.up(d_off, off.data(), n * 8);
                C.off = d_off; C.csv = (char *)q;
                HIP_OK(hipEventRecord(ev[2], ctx->stream));
                launch_ok(emgpu::launch_csv_emit(C, ctx->stream));
                HIP_OK(hipEventRecord(ev[3], ctx->stream));
                HIP_OK(hipEventRecord(ev[4], ctx->stream));
                B.down(out->csv, q, (size_t)csv_total);
                HIP_OK(hipEventRecord(ev[5], ctx->stream));
                HIP_OK(hipStreamSynchronize(ctx->stream));
                HIP_OK(hipEventElapsedTime(&ms, ev[2], ev[3])); phase[3] += ms;
                HIP_OK(hipEventElapsedTime(&ms, ev[4], ev[5])); phase[4] += ms;
                st.bytes_d2h += (int64_t)csv_total;
            }
        }
        out->totals[0] = (int64_t)csv_total;
        if (out->xyz && xyz_rows <= (uint64_t)out->xyz_cap) { B.down(out->xyz, d_xyz, (size_t)xyz_rows * 24); st.bytes_d2h += (int64_t)xyz_rows * 24; }
        rc = emgpu_ctx_sync(ctx);
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, ev[0], ev[1])); phase[2] = ms;
    }
    st.kernel_ms = phase[1] + phase[2] + phase[3]; st.d2h_ms = phase[4]; st.scatter_ms = phase[5];
    st.total_ms = ms_since(t_call);
    ctx->host_stats = st;
    if (out->phase_ms) memcpy(out->phase_ms, phase, sizeof phase);
    if (rc == EMGPU_OK && out->csv && csv_total > (uint64_t)out->csv_cap)
        return fail(EMGPU_ERR_EVENT_CAP, "emgpu_tracks_text_host: the CSV text has " + std::to_string(csv_total) + " bytes, csv_cap is " + std::to_string(out->csv_cap));
    if (rc == EMGPU_OK && out->xyz && xyz_rows > (uint64_t)out->xyz_cap)
        return fail(EMGPU_ERR_EVENT_CAP, "emgpu_tracks_text_host: the tracks have " + std::to_string(xyz_rows) + " position rows, xyz_cap is " + std::to_string(out->xyz_cap));
    return rc;
    EMGPU_CATCH
}

} // extern "C"
