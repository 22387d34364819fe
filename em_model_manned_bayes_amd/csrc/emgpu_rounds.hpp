// emgpu_rounds.hpp -- what the two round drivers share (CorTerminalModel.track in emgpu_terminal.cpp, UncorEncounterModel.track in
// emgpu_track.cpp): the scratch of a call, the rejection-round loop and the copy-back of what the rounds accepted.
#pragma once
#include <string>

#include "emgpu_internal.hpp"

// The device scratch of one round-driver call: the ctx's scratch blocks 0, 1, ... in request order (kept by the ctx between calls).  The
// stream is synchronized when the scope ends, however it ends: the rounds' launches read this scratch and the caller's buffers.
class RoundScratch {
  public:
    explicit RoundScratch(emgpu_ctx *ctx) : ctx_(ctx) {}
    RoundScratch(const RoundScratch &) = delete;
    RoundScratch &operator=(const RoundScratch &) = delete;
    ~RoundScratch() { (void)hipStreamSynchronize(ctx_->stream); }
    template <typename T> T *alloc(size_t bytes) { return static_cast<T *>(ctx_scratch(ctx_, slot_++, bytes ? bytes : 1)); }

  private:
    emgpu_ctx *ctx_;
    size_t slot_ = 0;
};

// What a round driver's host wrapper does with the rounds' status: under EMGPU_OK or EMGPU_ERR_REJECT_CAP (the accepted lanes are valid, the
// others carry attempts -1) copy() brings the outputs back, and the rounds' message survives whatever the copies do to the thread's.
template <typename Copy> int copy_back_accepted(emgpu_ctx *ctx, int rc, Copy copy) {
    if (rc != EMGPU_OK && rc != EMGPU_ERR_REJECT_CAP) return rc;
    const std::string msg = g_err;
    copy();
    HIP_OK(hipStreamSynchronize(ctx->stream));
    if (rc != EMGPU_OK) g_err = msg;
    return rc;
}

// The rejection rounds of a track call over n lanes: round j redraws what round j - 1 rejected, with attempt number j + 1, until nothing is
// left or max_rounds have run.  Owns the accepted flags, the two (global index, output slot) list pairs -- round j reads pair j & 1 (round 0
// none: lane i is global index first_index + i and slot i) and next() writes the other -- and the compaction's scratch.
class RejectionRounds {
  public:
    RejectionRounds(emgpu_ctx *ctx, RoundScratch &mem, size_t n, uint64_t first_index, int max_rounds)
        : ctx_(ctx), first_index_(first_index), max_(max_rounds), count_(n) {
        accepted_ = mem.alloc<uint8_t>(n);
        for (auto &q : gidx_) q = mem.alloc<uint64_t>(n * 8);
        for (auto &q : slot_) q = mem.alloc<int64_t>(n * 8);
        d_count_ = mem.alloc<uint32_t>(4 * emgpu::compact_scratch_words((int64_t)n));
    }
    bool more() const { return j_ < max_ && count_ > 0; }
    int round() const { return j_; }
    size_t count() const { return count_; }   // lanes of this round
    const uint64_t *indices() const { return j_ ? gidx_[j_ & 1] : nullptr; }
    const int64_t *slots() const { return j_ ? slot_[j_ & 1] : nullptr; }
    uint8_t *accepted() const { return accepted_; }
    int attempt_no() const { return j_ + 1; }
    int last_round() const { return j_ + 1 == max_; }
    // the end of a round: the lanes it rejected, in lane order, become the next round's lists
    void next() {
        const int cur = j_ & 1;
        HIP_OK(hipMemsetAsync(d_count_, 0, 4, ctx_->stream));
        launch_ok(emgpu::launch_compact_rejected((int64_t)count_, first_index_, accepted_, indices(), slots(), gidx_[cur ^ 1], slot_[cur ^ 1], d_count_, ctx_->stream));
        uint32_t hc = 0;
        HIP_OK(hipMemcpyAsync(&hc, d_count_, 4, hipMemcpyDeviceToHost, ctx_->stream));
        HIP_OK(hipStreamSynchronize(ctx_->stream));
        count_ = hc;
        j_++;
    }
    // after the last round: the draws' own deferred status (their rejection cap), then the lanes the rounds left rejected
    int status(const char *who, const char *what) const {
        const int rc = emgpu_ctx_sync(ctx_);
        if (rc != EMGPU_OK || count_ == 0) return rc;
        return fail(EMGPU_ERR_REJECT_CAP, std::string(who) + ": " + std::to_string(count_) + " " + what + " were still rejected after max_track_attempts");
    }

  private:
    emgpu_ctx *ctx_;
    uint64_t first_index_;
    int max_, j_ = 0;
    size_t count_;
    uint8_t *accepted_;
    uint64_t *gidx_[2];
    int64_t *slot_[2];
    uint32_t *d_count_;
};
