// emgpu_tracechunk.hpp -- what the trace units share: emgpu_score.cpp, emgpu_count.cpp, emgpu_discretize.cpp and emgpu_trackval.cpp, each
// with a _device and a _host entry point.  A _host call holds one device block of about EMGPU_HOST_CHUNK_MB, never memory proportional to
// n, and walks the trace in chunks of c lanes (trajectories, tracks), serially and single-buffered: upload, launch, download, synchronize.
// (The sampling side's double-buffered pipeline is run_chunks in emgpu_host.cpp.)  DESIGN.md §24.
#pragma once
#include <algorithm>
#include <initializer_list>

#include "emgpu_hostmem.hpp"

namespace emgpu_detail {
// launcher(args..., the ctx stream, &name): its status checked, its kernel recorded and counted -- after success only, unlike launch_named
// (emgpu_internal.hpp), which names the kernel before it checks and never counts: see there
template <typename Launcher, typename... Args> void launch_recorded(emgpu_ctx *ctx, Launcher launcher, const Args &...args) {
    const char *name = "";
    launch_ok(launcher(args..., ctx->stream, &name));
    ctx->last_kernel = name; ctx->last_launches++;
}

// ---- a chunk's layout, a function of integers alone (tools/asan/chunk_layout_check.cpp runs it without a device)
struct ChunkArray { size_t width, rows; };   // a device array of a chunk: `rows` rows of c lanes, `width` bytes per lane
struct ChunkLayout {
    int64_t c = 0;            // lanes per chunk, a multiple of 256 (the device arrays' lane dimension)
    size_t off[4] = {0};      // where each array begins, a multiple of 256 bytes
    size_t bytes = 0;         // the block
};
// c lanes of all the arrays are about `target` bytes (never more lanes than n rounded up, never fewer than 256)
inline ChunkLayout chunk_layout(int64_t n, size_t target, std::initializer_list<ChunkArray> arrays) {
    ChunkLayout L;
    size_t per_lane = 0, k = 0;
    for (const ChunkArray &a : arrays) per_lane += a.width * a.rows;
    L.c = (int64_t)std::min<size_t>(round_up((size_t)n, 256), std::max<size_t>(target / per_lane / 256 * 256, 256));
    for (const ChunkArray &a : arrays) { L.off[k++] = L.bytes; L.bytes += round_up(a.width * a.rows * (size_t)L.c, 256); }
    L.bytes += 256;
    return L;
}

// ---- a chunk's device block and the walk over a call's n lanes.  When the scope ends, however it ends, the stream is synchronized and the
// block released.
class ChunkBlock {
  public:
    ChunkBlock(emgpu_ctx *ctx, const char *entry_point, int64_t n, std::initializer_list<ChunkArray> arrays)
        : ctx_(ctx), n_(n), L_(chunk_layout(n, host_chunk_target((size_t)256 << 20), arrays)) {
        dev_ = (char *)device_block_or_trim(ctx, L_.bytes, true);
        if (!dev_) throw Error(EMGPU_ERR_HIP, std::string(entry_point) + ": out of device memory for one chunk");
    }
    ChunkBlock(const ChunkBlock &) = delete;
    ChunkBlock &operator=(const ChunkBlock &) = delete;
    ~ChunkBlock() { (void)hipStreamSynchronize(ctx_->stream); device_release(dev_); }
    int64_t c() const { return L_.c; }
    char *at(int k) const { return dev_ + L_.off[k]; }   // array k
    // body(c0, cn) for every chunk [c0, c0 + cn) of the call: it uploads, sets the kernel's n, launches and downloads
    template <typename Body> void each(Body body) {
        for (int64_t c0 = 0; c0 < n_; c0 += L_.c) {
            body(c0, std::min<int64_t>(L_.c, n_ - c0));
            HIP_OK(hipStreamSynchronize(ctx_->stream));   // the next chunk overwrites the buffer; the caller's arrays are pageable
        }
    }

  private:
    emgpu_ctx *ctx_;
    int64_t n_;
    ChunkLayout L_;
    char *dev_ = nullptr;
};

// ---- the bad-value word (emgpu_ctx::d_bad) across a _host call.  k_score_dbn, k_count_dbn and k_discretize_dbn store a non-zero word there
// when they meet a bad bin or value; emgpu_ctx_sync reports and clears it.  A _host call reports its own findings itself, when it returns.
// But the word may already hold the report of an earlier _device call that nobody has synchronized on yet: that one is not this call's,
// and this call must neither report it nor lose it.  So the constructor takes it out before the first chunk (copy, clear, synchronize,
// remember), and finish() reads what this call's chunks left, puts the earlier report back for the emgpu_ctx_sync it belongs to and says
// whether this call has one of its own.  What the call downloads behind its last chunk it issues before finish(), whose synchronization
// completes it; what it adds to the caller's arrays it adds before it returns the error.
class BadWordScope {
  public:
    explicit BadWordScope(emgpu_ctx *ctx) : ctx_(ctx), pending_(exchange(false)) {}
    bool finish() { return exchange(pending_); }

  private:
    // whether the word is set behind everything issued so far; it is left set or clear as `set` says (any non-zero word is a report)
    bool exchange(bool set) {
        HIP_OK(hipMemcpyAsync(ctx_->h_bad(), ctx_->d_bad(), sizeof(uint32_t), hipMemcpyDeviceToHost, ctx_->stream));
        HIP_OK(hipMemsetAsync(ctx_->d_bad(), set ? 1 : 0, sizeof(uint32_t), ctx_->stream));
        HIP_OK(hipStreamSynchronize(ctx_->stream));
        return *ctx_->h_bad() != 0;
    }
    emgpu_ctx *ctx_;
    bool pending_;
};
} // namespace emgpu_detail
