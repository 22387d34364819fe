// emgpu_kernels_csv.hip -- sample2track's CSV files formatted on the device (sample2track.m:274-279), for emgpu_tracks_text_host and
// emgpu_format_f0_host: per accepted track "time_s,x_ft,y_ft,z_ft\n", then "%i,%0.0f,%0.0f,%0.0f\n" for every second.
//
// "%0.0f".  For |v| < 2^63 the text is the decimal digits of rint(|v|) -- round to nearest, ties to even: one v_rndne_f64, and what C prints,
// which rounds the exact binary value -- behind a '-' whenever v's SIGN BIT is set: -0.3, -0.5 and -0.0 print "-0".  A track with a coordinate
// that is not finite or is 2^63 and more in magnitude is not formatted here: it is marked (hostfmt) and left to the host.
//
// The writer follows emgpu_kernels_text.hip: k_csv_len counts every track's bytes (the formatter with a counting sink); the offsets are a
// prefix sum over the tracks, made on the host, which wants them as the files' boundaries anyway and in 64 bits (a million tracks are 5 GB);
// k_csv_emit: one wave per track, lanes across 64 lines at a time (line 0 is the header), each into its own slot of LDS, then wave_emit
// (emgpu_text_pack.h) packs the wave's lines and stores whole dwords.
#include <hip/hip_runtime.h>

#include "emgpu_launch.h"
#include "emgpu_text_pack.h"

namespace emgpu {
namespace {

__device__ __forceinline__ bool f0_ok(double v) { return fabs(v) < 9223372036854775808.0; }   // (false for NaN)
template <class S>
__device__ inline void put_f0(double v, S &out) {   // f0_ok(v)
    if (__double_as_longlong(v) < 0) out.put('-');
    put_d((uint64_t)rint(fabs(v)), out);
}
template <class S>
__device__ inline void put_csv_row(uint32_t t, const double *r, S &out) {
    put_d(t, out);
    out.put(',');
    put_f0(r[0], out);
    out.put(',');
    put_f0(r[1], out);
    out.put(',');
    put_f0(r[2], out);
    out.put('\n');
}
template <class S>
__device__ inline void put_csv_header(S &out) {
    const char *h = "time_s,x_ft,y_ft,z_ft\n";
    for (int k = 0; k < 22; k++) out.put((uint32_t)h[k]);
}

constexpr uint32_t kCsvSlot = 76;   // a line is at most 10 + 3 * 20 + 4 = 74 bytes

__global__ void __launch_bounds__(256) k_csv_len(EmgpuCsvRun C) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= C.n) return;
    uint32_t bytes = 0;
    uint8_t host = 0;
    if (C.flags[i] == 0) {
        const double *r = C.xyz + 3 * C.xoff[i];
        const int rows = C.len[i] + 1;
        bool ok = true;
        for (int k = 0; k < 3 * rows; k++) ok = ok && f0_ok(r[k]);
        if (ok) {
            LenSink l;
            put_csv_header(l);
            for (int t = 0; t < rows; t++) put_csv_row((uint32_t)t, r + 3 * t, l);
            bytes = l.n;
        } else host = 1;
    }
    C.cnt[i] = bytes;
    C.hostfmt[i] = host;
}

extern __shared__ uint32_t s_csv[];   // [64 slots of kCsvSlot bytes | the packed lines: 64 kCsvSlot + 4 bytes]

__global__ void __launch_bounds__(64) k_csv_emit(EmgpuCsvRun C) {
    const int64_t i = blockIdx.x;
    if (C.cnt[i] == 0) return;
    const uint32_t lane = threadIdx.x;
    char *slots = reinterpret_cast<char *>(s_csv), *packed = slots + 64u * kCsvSlot;
    char *dst = C.csv + C.off[i];
    const double *r = C.xyz + 3 * C.xoff[i];
    const int lines = C.len[i] + 2;   // the header and seconds 0 .. len
    for (int j0 = 0; j0 < lines; j0 += 64) {
        const int j = j0 + (int)lane;
        MemSink out{slots + lane * kCsvSlot};
        if (j == 0) put_csv_header(out);
        else if (j < lines) put_csv_row((uint32_t)(j - 1), r + 3 * (size_t)(j - 1), out);
        dst += wave_emit(slots, kCsvSlot, out.n, packed, dst, lane);
    }
}

// emgpu_format_f0_host: one value per entry
__global__ void __launch_bounds__(256) k_f0_len(const double *x, int64_t n, uint32_t *cnt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    LenSink l;
    if (f0_ok(x[i])) put_f0(x[i], l);
    cnt[i] = l.n;
}
__global__ void __launch_bounds__(64) k_f0_emit(const double *x, int64_t n, const uint32_t *cnt, const uint32_t *scratch, char *text, uint64_t base,
                                               uint64_t *offsets) {
    const uint32_t lane = threadIdx.x, RS = 20;
    const int64_t i0 = (int64_t)blockIdx.x * 64, i = i0 + lane;
    char *slots = reinterpret_cast<char *>(s_csv), *packed = slots + 64u * RS;
    MemSink out{slots + lane * RS};
    if (i < n && f0_ok(x[i])) put_f0(x[i], out);
    const uint32_t o = offset_of(cnt, scratch, i0, lane);
    uint32_t inc = out.n;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(inc, d, 64); if (lane >= (uint32_t)d) inc += v; }
    if (i < n) offsets[i] = base + o + (inc - out.n);
    (void)wave_emit(slots, RS, out.n, packed, text + o, lane);
}

size_t lds_bytes(uint32_t RS) { return (size_t)128 * RS + 8; }
} // namespace

hipError_t launch_csv_len(const EmgpuCsvRun &C, hipStream_t s) {
    if (C.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_csv_len, dim3((unsigned)((C.n + 255) / 256)), dim3(256), 0, s, C);
    return hipGetLastError();
}

hipError_t launch_csv_emit(const EmgpuCsvRun &C, hipStream_t s) {
    if (C.n <= 0) return hipSuccess;
    if (C.n > 0x7FFFFFFF) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_csv_emit, dim3((unsigned)C.n), dim3(64), lds_bytes(kCsvSlot), s, C);
    return hipGetLastError();
}

hipError_t launch_format_f0(const double *x, int64_t n, uint32_t *cnt, uint32_t *scratch, char *text, uint64_t base, uint64_t *offsets, hipStream_t s) {
    if (n <= 0) return hipMemsetAsync(scratch, 0, 2 * sizeof(uint32_t), s);
    hipLaunchKernelGGL(k_f0_len, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n, cnt);
    const hipError_t e = launch_scan_counts(n, 0xFFFFFFFFu, cnt, scratch, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_f0_emit, dim3((unsigned)((n + 63) / 64)), dim3(64), lds_bytes(20), s, x, n, cnt, scratch, text, base, offsets);
    return hipGetLastError();
}

} // namespace emgpu
