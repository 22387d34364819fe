// emgpu_hostmem.hpp -- what the host-pointer units share: emgpu_memory.cpp (which defines all of it), emgpu_host.cpp (the chunked
// sampling path), emgpu_files.cpp (the text tables and files) and emgpu_tracechunk.hpp (the chunk block and loop of the four chunked
// trace paths: emgpu_score.cpp, emgpu_count.cpp, emgpu_discretize.cpp and emgpu_trackval.cpp include that).  Nothing else includes it.
#pragma once
#include <chrono>

#include "emgpu_internal.hpp"

namespace emgpu_detail {
using Clock = std::chrono::steady_clock;
inline double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }
inline size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
// ---- device blocks of the traces' allocator (the placement comment in emgpu_memory.cpp)
bool device_block(size_t bytes, void **p, bool plain = false);   // an allocation that reports failure instead of throwing (a candidate too many is not an error)
// device_block, and once more after the pool's idle blocks have gone back where the device is out of memory; null: the message is the caller's
void *device_block_or_trim(emgpu_ctx *ctx, size_t bytes, bool plain = false);
void device_release(void *p);
void pool_release(emgpu_ctx *ctx);
// a free block of the pool that fits (and is not more than a quarter too large), or a fresh allocation; {nullptr} when neither exists
emgpu_ctx::TraceBlock pool_take(emgpu_ctx *ctx, size_t bytes, bool *from_pool, bool plain = false);
// chunk buffers (blocks of the trace pool's allocator, unprobed) and pinned staging buffers of these sizes, one of each for a single chunk, two
// otherwise; the copy stream and h_total.  false: out of device memory
bool provision(emgpu_ctx *ctx, size_t nchunks, size_t dev_bytes, size_t stage_bytes);
size_t host_chunk_target(size_t dflt);   // a chunk's device bytes: EMGPU_HOST_CHUNK_MB (MiB) where it is set, else dflt
bool is_pinned(const void *p);
struct Events {   // a few HIP events, destroyed on every path out
    std::vector<hipEvent_t> e;
    explicit Events(int n) : e((size_t)n, nullptr) { for (auto &x : e) HIP_OK(hipEventCreate(&x)); }
    ~Events() { for (auto x : e) if (x) (void)hipEventDestroy(x); }
    hipEvent_t operator[](int i) const { return e[(size_t)i]; }
};
} // namespace emgpu_detail
