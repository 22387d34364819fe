// emgpu_text_pack.h -- what the device text writers share (emgpu_kernels_text.hip: em_sample's rows; emgpu_kernels_csv.hip: sample2track's CSV
// rows): the counting and the LDS sink of a formatter, "%d", and the wave's pack-and-store of 64 rows of variable length.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace emgpu {
namespace {

__device__ const uint64_t kP10[20] = {1ull, 10ull, 100ull, 1000ull, 10000ull, 100000ull, 1000000ull, 10000000ull, 100000000ull, 1000000000ull,
                                      10000000000ull, 100000000000ull, 1000000000000ull, 10000000000000ull, 100000000000000ull,
                                      1000000000000000ull, 10000000000000000ull, 100000000000000000ull, 1000000000000000000ull,
                                      10000000000000000000ull};

struct LenSink {   // counts
    uint32_t n = 0;
    __device__ __forceinline__ void put(uint32_t) { n++; }
};
struct MemSink {   // writes (LDS)
    char *p;
    uint32_t n = 0;
    __device__ __forceinline__ void put(uint32_t c) { p[n++] = (char)c; }
};

// "%d" of a non-negative integer
template <class S>
__device__ inline void put_d(uint64_t v, S &out) {
    int nd = 1;
    for (uint64_t t = v; t >= 10; t /= 10) nd++;
    for (int i = nd - 1; i >= 0; i--) out.put('0' + (uint32_t)(v / kP10[i] % 10));
}

// 64 rows, lane l's in slots + l * RS (len bytes; 0: no row), to dst: packed in LDS behind dst's misalignment, then stored.  One wave per
// workgroup (the barriers are the wave's own).  Returns the bytes written.
__device__ inline uint32_t wave_emit(const char *slots, uint32_t RS, uint32_t len, char *packed, char *dst, uint32_t lane) {
    uint32_t inc = len;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(inc, d, 64); if (lane >= (uint32_t)d) inc += v; }
    const uint32_t W = __shfl(inc, 63, 64), off = inc - len;
    const uint32_t pad = (uint32_t)((uintptr_t)dst & 3u);
    const char *src = slots + lane * RS;
    for (uint32_t j = 0; j < len; j++) packed[pad + off + j] = src[j];
    __syncthreads();
    char *g0 = dst - pad;
    const uint32_t total = pad + W, q0 = pad ? 1u : 0u, ndw = total >> 2;   // dwords q0 .. ndw-1 are whole
    for (uint32_t q = q0 + lane; q < ndw; q += 64) reinterpret_cast<uint32_t *>(g0)[q] = reinterpret_cast<const uint32_t *>(packed)[q];
    if (lane < 4) {            // the bytes before the first whole dword
        const uint32_t b = lane;
        if (b >= pad && b < total && b < 4u * q0) g0[b] = packed[b];
    } else if (lane < 8) {     // and behind the last
        const uint32_t b = 4u * max(ndw, q0) + (lane - 4u);
        if (b < total) g0[b] = packed[b];
    }
    __syncthreads();
    return W;
}

// the first byte of list i when scratch holds launch_scan_counts of cnt: the workgroup's prefix + the counts in front of it among its 256
__device__ inline uint32_t offset_of(const uint32_t *cnt, const uint32_t *scratch, int64_t i, uint32_t lane) {
    const int64_t j0 = i & ~(int64_t)255;
    uint32_t s = 0;
    for (int64_t j = j0 + lane; j < i; j += 64) s += cnt[j];
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    return scratch[2 + (i >> 8)] + s;
}

} // namespace
} // namespace emgpu
