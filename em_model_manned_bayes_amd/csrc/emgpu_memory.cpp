// emgpu_memory.cpp -- the memory the C ABI owns on behalf of the caller:
//   * device blocks: the VMM / hipMalloc block allocator behind every large device buffer of the host-pointer entry points;
//   * the trace pool: emgpu_trace_alloc / _out / _report / _free -- device memory for the sampler's outputs whose PLACEMENT has been
//     measured with the caller's own launch (profiles/r05_placement_probe.txt: the same launch writes one 36 GB allocation in 6.0 ms
//     and another in 7.1 ms);
//   * emgpu_device_alloc / _free (plain blocks of the same allocator) and the pinned pool, emgpu_host_alloc / _free;
//   * the chunk pipeline's buffers (provision) and their release with the ctx (ctx_release_host_side).
// emgpu_hostmem.hpp declares what emgpu_host.cpp and emgpu_files.cpp use of this.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>

#include "emgpu_hostmem.hpp"

using namespace emgpu_detail;

struct emgpu_trace {
    emgpu_ctx::TraceBlock blk;
    emgpu_sample_out out{};
    emgpu_trace_report_t rep{};
};

namespace {
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
bool vmm_block(size_t bytes, void **p) {
    size_t chunk = alloc_mode_once().chunk;
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
} // namespace

namespace emgpu_detail {
bool device_block(size_t bytes, void **p, bool plain) {
    *p = nullptr;
    const int mode = plain ? 0 : alloc_mode_once().mode;
    if (mode == 2) return vmm_block(bytes, p);
    if (mode == 3 && bytes >= ((size_t)1 << 30) && vmm_block(bytes, p)) return true;
    const hipError_t e = mode == 1 ? hipExtMallocWithFlags(p, bytes, hipDeviceMallocContiguous) : hipMalloc(p, bytes);
    if (e == hipSuccess) return true;
    (void)hipGetLastError();
    *p = nullptr;
    return false;
}
void *device_block_or_trim(emgpu_ctx *ctx, size_t bytes, bool plain) {
    void *p = nullptr;
    if (device_block(bytes, &p, plain)) return p;
    HIP_OK(hipStreamSynchronize(ctx->stream));   // out of memory: give the pool's idle blocks back and try once more
    pool_release(ctx);
    (void)device_block(bytes, &p, plain);
    return p;
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
emgpu_ctx::TraceBlock pool_take(emgpu_ctx *ctx, size_t bytes, bool *from_pool, bool plain) {
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
    b.p = device_block_or_trim(ctx, bytes, plain);
    if (b.p) b.bytes = bytes;
    return b;
}
bool is_pinned(const void *p) {
    if (!p) return false;
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof a);
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeHost;
}

// ------------------------------------------------------------------------------------------------ the chunk pipeline's buffers
size_t host_chunk_target(size_t dflt) {
    if (const char *e = getenv("EMGPU_HOST_CHUNK_MB")) { const long v = atol(e); if (v > 0) return (size_t)v << 20; }
    return dflt;
}
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
} // namespace emgpu_detail

namespace {
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

extern "C" {

// ================================================================================================ the trace pool
int emgpu_trace_alloc(emgpu_ctx *ctx, const emgpu_model *h, const emgpu_sample_params *p, uint32_t want, int32_t candidates, emgpu_trace **out) {
    EMGPU_TRY
    if (!ctx || !h || !p || !out) return fail(EMGPU_ERR_ARG, "null argument");
    if (p->n < 0 || p->sample_time < 1) return fail(EMGPU_ERR_ARG, "n < 0 or sample_time < 1");
    if (!(want & (EMGPU_TRACE_INIT | EMGPU_TRACE_DENSE | EMGPU_TRACE_EVENTS | EMGPU_TRACE_ATTEMPTS)) || (want & ~15u)) return fail(EMGPU_ERR_ARG, "want: a combination of EMGPU_TRACE_*");
    if ((want & EMGPU_TRACE_EVENTS) && p->event_cap < 1) return fail(EMGPU_ERR_ARG, "EMGPU_TRACE_EVENTS needs event_cap >= 1");
    if (candidates < 0 || candidates > 8) return fail(EMGPU_ERR_ARG, "candidates outside 0..8");
    CTX_DEVICE(ctx);
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
    CTX_ENTER(ctx);
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
    CTX_DEVICE(ctx);
    const size_t need = std::max<size_t>((size_t)bytes, 256);
    void *p = device_block_or_trim(ctx, need);
    if (!p) return fail(EMGPU_ERR_HIP, "emgpu_device_alloc: out of device memory (" + std::to_string(need) + " bytes)");
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

// plain copies between a caller's host array and device memory, on the ctx stream, complete when the call returns
static int device_copy(emgpu_ctx *ctx, void *dst, const void *src, uint64_t bytes, hipMemcpyKind kind) {
    EMGPU_TRY
    if (!ctx) return fail(EMGPU_ERR_ARG, "null ctx");
    if (bytes == 0) return EMGPU_OK;
    if (!dst || !src) return fail(EMGPU_ERR_ARG, "null argument");
    CTX_DEVICE(ctx);
    HIP_OK(hipMemcpyAsync(dst, src, (size_t)bytes, kind, ctx->stream));
    HIP_OK(hipStreamSynchronize(ctx->stream));
    return EMGPU_OK;
    EMGPU_CATCH
}
int emgpu_device_upload(emgpu_ctx *ctx, void *dst_device, const void *src_host, uint64_t bytes) {
    return device_copy(ctx, dst_device, src_host, bytes, hipMemcpyHostToDevice);
}
int emgpu_device_download(emgpu_ctx *ctx, void *dst_host, const void *src_device, uint64_t bytes) {
    return device_copy(ctx, dst_host, src_device, bytes, hipMemcpyDeviceToHost);
}

// ================================================================================================ the pinned pool
int emgpu_host_alloc(emgpu_ctx *ctx, uint64_t bytes, void **out) {
    EMGPU_TRY
    if (!ctx || !out) return fail(EMGPU_ERR_ARG, "null argument");
    CTX_DEVICE(ctx);
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

} // extern "C"
