// emgpu_internal.hpp -- what the translation units behind include/emgpu.h share: the handle structs, the error plumbing and the
// ctx's device scratch.  Not installed; nothing outside csrc/ includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "../../include/emgpu.h"
#include "emgpu_launch.h"
#include "emgpu_model.hpp"

using emgpu::CompiledPlan;
using emgpu::Error;
using emgpu::Model;

struct emgpu_model {
    Model m;
};

namespace emgpu_detail {
std::string &last_error();                       // the calling thread's message (emgpu_last_error)
int fail(int code, const std::string &msg);      // records msg, returns code
} // namespace emgpu_detail
using emgpu_detail::fail;
#define g_err (emgpu_detail::last_error())

#define EMGPU_TRY try {
#define EMGPU_CATCH                                                      \
    }                                                                    \
    catch (const Error &e) { return fail(e.code, e.what()); }            \
    catch (const std::bad_alloc &) { return fail(EMGPU_ERR_ARG, "out of host memory"); } \
    catch (const std::exception &e) { return fail(EMGPU_ERR_ARG, e.what()); }

#define HIP_OK(expr)                                                                                  \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) throw Error(EMGPU_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

struct Uploaded {
    uint64_t version = 0;
    uint64_t last_use = 0;
    CompiledPlan cp;
    uint32_t *d_thr = nullptr;
    uint32_t *d_cthr = nullptr;
    uint32_t *d_pthr = nullptr;
    double *d_bnd = nullptr;
    void *d_planf = nullptr; // the plan itself (+ k_uncor_fast's resample thresholds) for launches that serve several models
    double *d_logp = nullptr; // log P of the initial network (emgpu::initial_log_prob), uploaded when a call first asks for log-weights
    uint32_t lp_off[EMGPU_MAX_NI] = {0};
    // log P of the transition network (emgpu::transition_log_prob) for emgpu_score_dbn_*, uploaded when a call first scores (the initial
    // network's is d_logp); like d_logp it belongs to `version`: get_uploaded frees every table when anything of the model has changed
    double *d_logpt = nullptr;
    uint32_t lpt_off[EMGPU_MAX_ND] = {0};   // by temporal-map row
    void free_tables() {
        (void)hipFree(d_thr); (void)hipFree(d_cthr); (void)hipFree(d_pthr); (void)hipFree(d_bnd); (void)hipFree(d_planf); (void)hipFree(d_logp);
        (void)hipFree(d_logpt);
        d_thr = d_cthr = d_pthr = nullptr; d_bnd = nullptr; d_planf = nullptr; d_logp = nullptr; d_logpt = nullptr;
    }
};

struct emgpu_ctx {
    std::recursive_mutex mu; // serialises calls on this ctx (the *_host entry points re-enter through *_device)
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    uint32_t *d_status = nullptr;   // two words: the sampler's status bits, the bad-bin word of k_score_dbn, k_count_dbn and k_discretize_dbn (emgpu_ctx_sync reads and clears both)
    uint32_t *d_queue = nullptr;  // k_terminal_propagate: the launch's track queue (one word, zeroed by the launcher)
    EmgpuPresets *d_presets = nullptr;   // the start grid / log-weight block of the last DBN call that had one
    uint32_t *h_status = nullptr; // pinned, two words
    static constexpr int kBadWord = 1;   // the bad-bin word's place in both (a plain store by the kernels, no atomic)
    uint32_t *d_bad() const { return d_status + kBadWord; }
    uint32_t *h_bad() const { return h_status + kBadWord; }
    std::map<uint64_t, Uploaded> cache; // by Model::uid
    uint64_t use_clock = 0;
    std::string last_kernel;
    int32_t last_launches = 0;
    double *d_layers = nullptr;
    size_t d_layers_cap = 0;
    const uint32_t **d_thr_base = nullptr; // terminal propagation: per-model table pointers
    size_t d_thr_base_cap = 0;             // bytes, like d_layers_cap
    // Side streams for the blocks of a mixed batch (created on first use): independent launches that share the ctx stream's
    // ordering at both ends, so that one block's tail runs under the next block's head instead of in front of it.
    static constexpr int kSide = 3;
    // Device scratch of the round drivers (UncorEncounterModel.track / CorTerminalModel.track), kept between calls and grown on demand:
    // a fresh hipMalloc + hipFree of several gigabytes per call cost tens of milliseconds, at random (measured: 29 vs 127 ms per call)
    struct Scratch { void *p = nullptr; size_t cap = 0; };
    std::vector<Scratch> scratch;
    // getDynamicLimits.m as a table, per (model uid, model version, the track variables): building it walks N_initial{v} and
    // N_initial{\dot h} over every (G, A, L range, v range) -- 4 ms on the host for uncor_1200code_v2p1, per call before it was kept
    std::map<std::array<uint64_t, 3>, emgpu::UncorLimits> limits_cache;
    hipStream_t side[kSide] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[kSide] = {nullptr, nullptr, nullptr};
    // ---- the trace pool (emgpu_trace_alloc / emgpu_trace_free, emgpu_memory.cpp): device blocks whose PLACEMENT has been measured.  A block
    // given back stays here and the next request it fits takes it without a new probe; emgpu_ctx_trim / emgpu_ctx_free release them.
    struct TraceBlock { void *p = nullptr; size_t bytes = 0; float ms = 0.f; bool probed = false; };
    std::vector<TraceBlock> trace_pool;
    std::set<void *> device_blocks;   // emgpu_device_alloc: blocks a caller holds (released with the ctx at the latest)
    // ---- the pipeline of the host-pointer entry points: a copy stream beside the launch stream, two chunk buffers on the device (blocks of
    // the trace pool), two pinned staging buffers, and pinned blocks handed to callers (emgpu_host_alloc)
    hipStream_t copy_stream = nullptr;
    TraceBlock chunk_buf[2];
    void *h_stage[2] = {nullptr, nullptr};
    size_t h_stage_cap = 0;
    uint64_t *h_total = nullptr;   // pinned, 2 words per chunk buffer: rows of its packed event lists, rows of its control rows
    struct HostBlock { void *p = nullptr; size_t bytes = 0; bool in_use = false; };
    std::vector<HostBlock> host_pool;
    emgpu_host_stats_t host_stats{};   // phases of the last emgpu_sample_dbn_host / emgpu_sample_uncor_host / emgpu_sample_text_host call
    uint64_t format_paths[2] = {0, 0}; // emgpu_format_g_host: values formatted on the 64-bit / the multiword path (emgpu_debug_format_paths)
};

// ---- how an entry point takes its ctx.  CTX_DEVICE: lock the ctx and make its device current -- behind an argument check that has
// already refused a null ctx in the entry point's own words ("null argument" with its other pointers, mostly).  CTX_ENTER: the same for an
// entry point whose check leaves the ctx to the macro, which says "null ctx": everything that can be said without a device has been said
// before ctx is looked at.  CTX_LOCK alone is for the entry points that touch no device (emgpu_ctx_set_stream, emgpu_debug_format_paths,
// emgpu_host_free) or have something to say between the lock and the device (emgpu_device_free).
#define CTX_LOCK(ctx) std::lock_guard<std::recursive_mutex> _ctx_lock((ctx)->mu)
#define CTX_DEVICE(ctx) CTX_LOCK(ctx); HIP_OK(hipSetDevice((ctx)->device))
#define CTX_ENTER(ctx) if (!(ctx)) return fail(EMGPU_ERR_ARG, "null ctx"); CTX_DEVICE(ctx)

// ---- a launcher's status.  launch_ok checks it (EMGPU_CATCH turns the throw into fail(EMGPU_ERR_HIP, "kernel launch: ...")).
inline void launch_ok(hipError_t e) {
    if (e != hipSuccess) throw Error(EMGPU_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
}
// launch(&name) launches and says which kernel it chose: the name goes into ctx->last_kernel BEFORE the status is checked, so that after a
// failed launch emgpu_last_kernel_name says which kernel failed; last_launches is not touched (these entry points never counted).  The trace
// units' emgpu_detail::launch_recorded (emgpu_tracechunk.hpp) is the other order on purpose: it counts, and names and counts only a launch
// that succeeded: emgpu_last_launch_count is the number of launches that were made, and there the name goes with the count.
template <typename Launch> void launch_named(emgpu_ctx *ctx, Launch launch) {
    const char *name = "";
    const hipError_t e = launch(&name);
    ctx->last_kernel = name;
    launch_ok(e);
}

// emgpu_ctx.cpp
// The model's tables on this ctx's device, uploaded (again) when the model's version is not the uploaded one.  `pinned`: uids that must survive
// the eviction of old entries (the other models of the current call).
Uploaded &get_uploaded(emgpu_ctx *ctx, const emgpu_model *h, const std::set<uint64_t> *pinned = nullptr);
void ensure_logp(emgpu_ctx *ctx, Uploaded &u, const Model &m);   // u.d_logp / u.lp_off, uploaded on first use
namespace emgpu_detail {
constexpr const char *kScoreBadBin = "a bin outside 1..r in the trace (score: the log-likelihood of those trajectories is NaN; count: the observations that read it were skipped), or a bad value in a trace of values (discretize: its bin is 0)";
}
// A device buffer the ctx owns, *p with room for *cap bytes, must hold `need` bytes.  Large enough (and there): nothing happens, and the
// contents stay.  Otherwise the ctx stream is synchronized (nothing in flight may still read the old block), the block freed, *p and *cap
// set to null / 0 -- a hipMalloc that throws leaves an empty buffer behind, never a pointer to freed memory for the next call to use and
// emgpu_ctx_free to free again -- and `size` bytes (>= need: the caller's head-room, if it wants any) allocated and recorded.
void ctx_grow(emgpu_ctx *ctx, void **p, size_t *cap, size_t need, size_t size);
// slot-th scratch buffer of the ctx, at least `bytes` long.  Two users share the slots: the host-path sampling entry points of emgpu_host.cpp
// take slot 0 (the start grid) and slot 1 (the index list) by number, and the round drivers of emgpu_terminal.cpp and emgpu_track.cpp (RoundScratch, emgpu_rounds.hpp) take 0 ... k in
// request order.  They never meet in one call: a host-path entry point samples through the *_device entry points and never enters a round
// driver, a round driver draws through launch_dbn / launch_bn and never enters the host path, and CTX_LOCK lets one call at a time use a ctx.
void *ctx_scratch(emgpu_ctx *ctx, size_t slot, size_t bytes);
// emgpu_sample.cpp: what the round drivers draw through
void fill_run(emgpu_ctx *ctx, const Uploaded &u, const Model &m, const emgpu_sample_params *p, EmgpuRun &A);   // the run of a DBN call, outputs unbound
// The block of device memory a launch reads its start grid / log-weight pointers through (one per ctx, rewritten per launch).
const EmgpuPresets *upload_presets(emgpu_ctx *ctx, Uploaded &u, const Model &m, const int32_t *start, double *log_weight, const int64_t *row);
void launch_dbn(emgpu_ctx *ctx, const Uploaded &u, const EmgpuRun &A, hipStream_t stream = nullptr, const EmgpuPresets *presets = nullptr);
void fill_bn(emgpu_ctx *ctx, const Uploaded &u, const Model &m, const emgpu_bn_params *p, EmgpuBnRun &A);      // the run of a BN call, outputs unbound
// emgpu_memory.cpp
void ctx_release_host_side(emgpu_ctx *ctx, bool everything);    // trim (false: pools and staging) / free (true: streams and events too)

// sample2track.m:113-139: the unit ratios and the speed limits of a track call, into the kernel argument struct of either track kernel
// (EmgpuTrackRun, EmgpuTrackTableRun)
template <typename Run> void set_track_units(Run &A, const emgpu_track_params *p) {
    A.ur_speed = p->ur_speed; A.ur_vertrate = p->ur_vertrate; A.ur_heading = p->ur_heading;
    A.min_speed = p->min_speed; A.max_speed = p->max_speed;
}

// The device buffers of one host-pointer call: fresh per call, freed when the call returns or throws, after the ctx stream has drained.
// up / down copy on the ctx stream and do nothing for zero bytes or a null host pointer.
class CallBuffers {
  public:
    explicit CallBuffers(emgpu_ctx *ctx) : ctx_(ctx) {}
    CallBuffers(const CallBuffers &) = delete;
    CallBuffers &operator=(const CallBuffers &) = delete;
    ~CallBuffers() {
        (void)hipStreamSynchronize(ctx_->stream);
        for (void *p : ptrs_) (void)hipFree(p);
    }
    template <typename T> T *alloc(size_t bytes) {
        ptrs_.push_back(nullptr);   // (the slot first: nothing can throw between the hipMalloc and the record)
        HIP_OK(hipMalloc(&ptrs_.back(), bytes));
        return static_cast<T *>(ptrs_.back());
    }
    // alloc for a block whose failure the caller reports in words of its own: null, with HIP's error cleared and the slot dropped
    template <typename T> T *try_alloc(size_t bytes) {
        ptrs_.push_back(nullptr);
        if (hipMalloc(&ptrs_.back(), bytes) == hipSuccess) return static_cast<T *>(ptrs_.back());
        (void)hipGetLastError();
        ptrs_.pop_back();
        return nullptr;
    }
    void up(void *dst, const void *src, size_t bytes) {
        if (bytes && src) HIP_OK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx_->stream));
    }
    // a device copy of a caller's array, complete when this returns (the array is the caller's memory: it may be gone behind the call)
    template <typename T> T *copy_of(const T *src, size_t bytes) {
        T *d = alloc<T>(bytes);
        up(d, src, bytes);
        HIP_OK(hipStreamSynchronize(ctx_->stream));
        return d;
    }
    void down(void *dst, const void *src, size_t bytes) {
        if (bytes && dst) HIP_OK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx_->stream));
    }

  private:
    emgpu_ctx *ctx_;
    std::vector<void *> ptrs_;
};
