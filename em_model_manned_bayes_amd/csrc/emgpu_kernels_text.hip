// emgpu_kernels_text.hip -- em_sample's text rows formatted on the device (em_sample.m:85-99), for emgpu_sample_text_host and
// emgpu_format_g_host: an exact C "%g" (precision 6) of every f32 widened to double and of the non-negative integers an id or a
// second can be, and the writers of the two files' rows.
//
// The formatter.  A positive value is m * 2^e with m an integer (f32: 24 bits, e = -149..104; an id: the integer itself, e = 0).  With X its
// decimal exponent, q7 = floor(v * 10^(6 - X)) (seven digits) and `sticky` = "the rest is not zero" decide the six printed digits exactly:
// the seventh digit and the sticky bit round half to even on the binary value itself, as glibc does.  X comes from the bit length
// (floor((L - 1) log10 2) is X or X - 1; a q7 of eight digits says which).  Two paths compute (q7, sticky):
//   fast   everything fits 64 bits: integers below 2^64, and fractions from 10^-6 up (m * 10^(6-X) < 2^24 * 10^12 < 2^64);
//   slow   six 32-bit limbs: f32 values of 2^64 and more are divided by 10^(X-6), nine digits at a time; fractions below 10^-6 are
//          multiplied by 10^(6-X) (at most 2^27 * 2^149 = 2^176) and shifted.
// Every value of the shipped models (10^-4 .. 10^6) takes the fast path; tests reach the slow one through emgpu_format_g_host.
//
// The writers.  Rows have variable length: k_text_len counts every trajectory's bytes (the formatter with a counting sink), launch_scan_counts
// turns them into offsets, then one wave formats 64 rows (k_text_transition: one trajectory, lanes across seconds; k_text_initial and
// k_g_emit: lanes across trajectories / values), each lane into its own slot of LDS; a wave scan of the lengths packs the rows in LDS
// behind the destination's own misalignment, and the wave stores whole dwords, lane after lane -- only the up to three bytes before the first
// and after the last whole dword go out as bytes (the neighbouring rows' bytes in those dwords belong to other waves).
// Formatting twice costs ALU only; the alternative, rows at a fixed stride in device memory and a compaction pass, triples the traffic.
#include <hip/hip_runtime.h>

#include "emgpu_launch.h"
#include "emgpu_text_pack.h"   // the sinks, "%d" and the wave's pack-and-store, shared with the CSV writer

namespace emgpu {
namespace {

// ---- six little-endian 32-bit limbs
__device__ inline void mul_small(uint32_t (&a)[6], uint32_t f) {
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) { c += (uint64_t)a[i] * f; a[i] = (uint32_t)c; c >>= 32; }
}
__device__ inline uint32_t divmod_small(uint32_t (&a)[6], uint32_t d) {   // a /= d; the remainder
    uint64_t r = 0;
#pragma unroll
    for (int i = 5; i >= 0; i--) { const uint64_t cur = (r << 32) | a[i]; a[i] = (uint32_t)(cur / d); r = cur % d; }
    return (uint32_t)r;
}

// v = m * 2^e > 0 (m != 0; e >= 0: bit length of v at most 160; e < 0: m < 2^24 and e >= -149).  The six digits D (10^5 <= D < 10^6) and the
// decimal exponent X of "%.5e"; returns true when the slow path computed them.
__device__ inline bool decimal6(uint64_t m, int e, uint32_t &D, int &X) {
    const int L = 64 - __clzll((long long)m) + e;   // 2^(L-1) <= v < 2^L
    X = ((L - 1) * 78913) >> 18;                     // floor((L-1) log10 2): the decimal exponent or one less
    const bool fast = e >= 0 ? L <= 64 : (m < (1ull << 24) && X >= -6);
    uint64_t q;
    bool sticky = false;
    const int s = 6 - X;
    if (fast) {
        if (s >= 0) {
            const uint64_t num = m * kP10[s];
            if (e >= 0) q = num << e;
            else { q = num >> -e; sticky = (num & ((1ull << -e) - 1)) != 0; }
        } else {
            uint64_t V = m;
            if (e >= 0) V = m << e;
            else { sticky = (m & ((1ull << -e) - 1)) != 0; V = m >> -e; }
            const uint64_t p = kP10[-s];
            q = V / p;
            sticky = sticky || V % p != 0;
        }
    } else if (e >= 0) {   // an integer of more than 64 bits: / 10^(X-6)
        uint32_t a[6] = {0, 0, 0, 0, 0, 0};
        const int li = e >> 5, bit = e & 31;
        const uint64_t lo = m << bit, hi = bit ? m >> (64 - bit) : 0ull;   // m << e over three limbs from limb li
#pragma unroll
        for (int i = 0; i < 6; i++) {
            if (i == li) a[i] = (uint32_t)lo;
            if (i == li + 1) a[i] = (uint32_t)(lo >> 32);
            if (i == li + 2) a[i] = (uint32_t)hi;
        }
        int rest = -s;
        for (; rest >= 9; rest -= 9) sticky = divmod_small(a, 1000000000u) != 0 || sticky;
        if (rest) sticky = divmod_small(a, (uint32_t)kP10[rest]) != 0 || sticky;
        q = ((uint64_t)a[1] << 32) | a[0];
    } else {               // a fraction below 10^-6: * 10^(6-X), then >> -e
        uint32_t a[6] = {(uint32_t)m, 0, 0, 0, 0, 0};
        int rest = s;
        for (; rest >= 9; rest -= 9) mul_small(a, 1000000000u);
        if (rest) mul_small(a, (uint32_t)kP10[rest]);
        const int k = -e, li = k >> 5, bit = k & 31;
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            if (i == li) lo = a[i];
            if (i == li + 1) hi = a[i];
            if (i < li) sticky = sticky || a[i] != 0;
        }
        sticky = sticky || (lo & ((1u << bit) - 1u)) != 0;
        q = bit ? (lo >> bit) | (hi << (32 - bit)) : lo;   // (q < 10^8: the limbs above hold nothing)
    }
    if (q >= 10000000ull) { sticky = sticky || q % 10 != 0; q /= 10; X++; }   // the estimate of X was one short
    const uint32_t q7 = (uint32_t)q, d7 = q7 % 10u;
    D = q7 / 10u;
    if (d7 > 5u || (d7 == 5u && (sticky || (D & 1u)))) D++;   // half to even on the exact value
    if (D == 1000000u) { D = 100000u; X++; }
    return !fast;
}

// "%g" of m * 2^e (m != 0) after the sign
template <class S>
__device__ inline bool put_g(uint64_t m, int e, S &out) {
    uint32_t D;
    int X;
    const bool slow = decimal6(m, e, D, X);
    uint32_t dg[6], r = D;
#pragma unroll
    for (int i = 5; i >= 0; i--) { dg[i] = r % 10u; r /= 10u; }
    int nz = 6;   // significant digits without the trailing zeros
#pragma unroll
    for (int i = 5; i >= 1; i--) if (nz == i + 1 && dg[i] == 0) nz = i;
    if (X < -4 || X >= 6) {
        out.put('0' + dg[0]);
        if (nz > 1) out.put('.');
#pragma unroll
        for (int i = 1; i < 6; i++) if (i < nz) out.put('0' + dg[i]);
        out.put('e');
        out.put(X < 0 ? '-' : '+');
        const uint32_t ax = (uint32_t)(X < 0 ? -X : X);   // (two digits: |X| <= 47 for every value this is called with)
        out.put('0' + ax / 10u);
        out.put('0' + ax % 10u);
    } else if (X >= 0) {
#pragma unroll
        for (int i = 0; i < 6; i++) {
            if (i < nz || i <= X) out.put('0' + dg[i]);
            if (i == X && nz > X + 1) out.put('.');
        }
    } else {
        out.put('0');
        out.put('.');
        for (int z = 0; z < -X - 1; z++) out.put('0');
#pragma unroll
        for (int i = 0; i < 6; i++) if (i < nz) out.put('0' + dg[i]);
    }
    return slow;
}

// "%g" of an f32 widened to double, non-finite values as the host writer spells them; true: the slow path
template <class S>
__device__ inline bool put_f32(float x, S &out) {
    const uint32_t b = __float_as_uint(x), E = (b >> 23) & 255u, F = b & 0x7FFFFFu;
    if (E == 255u) {
        if (F) { out.put('N'); out.put('a'); out.put('N'); return false; }
        if (b >> 31) out.put('-');
        out.put('I'); out.put('n'); out.put('f');
        return false;
    }
    if (b >> 31) out.put('-');
    if (!E && !F) { out.put('0'); return false; }
    return E ? put_g((uint64_t)(F | 0x800000u), (int)E - 150, out) : put_g((uint64_t)F, -149, out);
}
// "%g" of a non-negative integer below 2^53
template <class S>
__device__ inline void put_u(uint64_t v, S &out) {
    if (!v) { out.put('0'); return; }
    (void)put_g(v, 0, out);
}
template <class S>
__device__ inline void put_initial_row(const EmgpuTextRun &R, int64_t i, S &out) {
    put_d((uint64_t)(R.id_first + i), out);
    out.put(' ');
    for (int v = 0; v < R.ni; v++) {
        (void)put_f32(R.init_val[(size_t)v * R.ld + i], out);
        if (v + 1 < R.ni) out.put(' ');
    }
    out.put('\n');
}

// the bytes of every trajectory's rows: cnt_i[i] (its initial row), cnt_t[i] (its T transition rows)
__global__ void __launch_bounds__(256) k_text_len(EmgpuTextRun R) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= R.n) return;
    LenSink li;
    put_initial_row(R, i, li);
    R.cnt_i[i] = li.n;
    LenSink id;
    put_u((uint64_t)(R.id_first + i), id);
    LenSink lt;
    for (int t = 0; t < R.T; t++) put_u((uint64_t)t, lt);
    lt.n += (uint32_t)R.T * (id.n + 2u + (R.nd ? 0u : 1u));   // "<id> <t> " in front of every row (and the newline of a row without values)
    const float4 *dv = (const float4 *)R.dyn_val;
    for (int g = 0; g < (R.T + 3) / 4; g++)
        for (int k = 0; k < R.nd; k++) {
            const float4 x = dv[((size_t)g * R.nd + k) * R.ld + i];
            const int rem = R.T - 4 * g;
            (void)put_f32(x.x, lt);
            if (rem > 1) (void)put_f32(x.y, lt);
            if (rem > 2) (void)put_f32(x.z, lt);
            if (rem > 3) (void)put_f32(x.w, lt);
            lt.n += (uint32_t)min(rem, 4);   // the space or newline behind each
        }
    R.cnt_t[i] = lt.n;
}

extern __shared__ uint32_t s_text[];   // [64 slots of RS bytes | the packed rows: 64 RS + 4 bytes]

// one wave per trajectory, lanes across 64 seconds at a time.  Workgroup b serves trajectory (b % 8) * ceil(n / 8) + b / 8: the waves of one
// XCD (workgroups go round the eight of them) read neighbouring trajectories, whose values share cache lines.
__global__ void __launch_bounds__(64) k_text_transition(EmgpuTextRun R, uint32_t RS) {
    const int64_t per = (R.n + 7) / 8, i = (int64_t)(blockIdx.x & 7u) * per + (blockIdx.x >> 3);
    if ((int64_t)(blockIdx.x >> 3) >= per || i >= R.n) return;
    const uint32_t lane = threadIdx.x;
    char *slots = reinterpret_cast<char *>(s_text), *packed = slots + 64u * RS;
    char *dst = R.text_t + offset_of(R.cnt_t, R.scr_t, i, lane);
    const uint64_t id = (uint64_t)(R.id_first + i);
    for (int t0 = 0; t0 < R.T; t0 += 64) {
        const int t = t0 + (int)lane;
        MemSink out{slots + lane * RS};
        if (t < R.T) {
            put_u(id, out);
            out.put(' ');
            put_u((uint64_t)t, out);
            out.put(' ');
            for (int k = 0; k < R.nd; k++) {
                (void)put_f32(R.dyn_val[(((size_t)(t >> 2) * R.nd + k) * R.ld + i) * 4 + (t & 3)], out);
                if (k + 1 < R.nd) out.put(' ');
            }
            out.put('\n');
        }
        dst += wave_emit(slots, RS, out.n, packed, dst, lane);
    }
}

// one wave per 64 trajectories
__global__ void __launch_bounds__(64) k_text_initial(EmgpuTextRun R, uint32_t RS) {
    const uint32_t lane = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * 64, i = i0 + lane;
    char *slots = reinterpret_cast<char *>(s_text), *packed = slots + 64u * RS;
    MemSink out{slots + lane * RS};
    if (i < R.n) put_initial_row(R, i, out);
    (void)wave_emit(slots, RS, out.n, packed, R.text_i + offset_of(R.cnt_i, R.scr_i, i0, lane), lane);
}

// emgpu_format_g_host: one value per entry.  paths[0] / paths[1]: the finite non-zero values that took the fast / the slow path
__global__ void __launch_bounds__(256) k_g_len(const float *x, int64_t n, uint32_t *cnt, unsigned long long *paths) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    LenSink l;
    bool slow = false, counted = false;
    if (i < n) {
        const uint32_t b = __float_as_uint(x[i]);
        counted = (b & 0x7FFFFFFFu) != 0 && ((b >> 23) & 255u) != 255u;
        slow = put_f32(x[i], l);
        cnt[i] = l.n;
    }
    const unsigned long long ms = __ballot(counted && slow), mf = __ballot(counted && !slow);
    if ((threadIdx.x & 63) == 0) {
        if (mf) atomicAdd(&paths[0], (unsigned long long)__popcll(mf));
        if (ms) atomicAdd(&paths[1], (unsigned long long)__popcll(ms));
    }
}
__global__ void __launch_bounds__(64) k_g_emit(const float *x, int64_t n, const uint32_t *cnt, const uint32_t *scratch, char *text, uint64_t base,
                                              uint64_t *offsets) {
    const uint32_t lane = threadIdx.x, RS = 12;
    const int64_t i0 = (int64_t)blockIdx.x * 64, i = i0 + lane;
    char *slots = reinterpret_cast<char *>(s_text), *packed = slots + 64u * RS;
    MemSink out{slots + lane * RS};
    if (i < n) (void)put_f32(x[i], out);
    const uint32_t o = offset_of(cnt, scratch, i0, lane);
    uint32_t inc = out.n;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(inc, d, 64); if (lane >= (uint32_t)d) inc += v; }
    if (i < n) offsets[i] = base + o + (inc - out.n);
    (void)wave_emit(slots, RS, out.n, packed, text + o, lane);
}

size_t lds_bytes(uint32_t RS) { return (size_t)128 * RS + 8; }
} // namespace

uint32_t text_row_bound_initial(int ni) { return 21u + 13u * (uint32_t)ni; }
uint32_t text_row_bound_transition(int nd) { return 13u * (2u + (uint32_t)nd); }

hipError_t launch_text_rows(const EmgpuTextRun &R, hipStream_t s) {
    if (R.n <= 0) return hipSuccess;
    const uint32_t rs_i = (text_row_bound_initial(R.ni) + 3u) & ~3u, rs_t = (text_row_bound_transition(R.nd) + 3u) & ~3u;
    if (lds_bytes(rs_i) > 65536 || lds_bytes(rs_t) > 65536) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_text_len, dim3((unsigned)((R.n + 255) / 256)), dim3(256), 0, s, R);
    hipError_t e = launch_scan_counts(R.n, 0xFFFFFFFFu, R.cnt_i, R.scr_i, s);
    if (e != hipSuccess) return e;
    e = launch_scan_counts(R.n, 0xFFFFFFFFu, R.cnt_t, R.scr_t, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_text_initial, dim3((unsigned)((R.n + 63) / 64)), dim3(64), lds_bytes(rs_i), s, R, rs_i);
    hipLaunchKernelGGL(k_text_transition, dim3((unsigned)(8 * ((R.n + 7) / 8))), dim3(64), lds_bytes(rs_t), s, R, rs_t);
    return hipGetLastError();
}

hipError_t launch_format_g(const float *x, int64_t n, uint32_t *cnt, uint32_t *scratch, char *text, uint64_t base, uint64_t *offsets,
                           unsigned long long *paths, hipStream_t s) {
    if (n <= 0) return hipMemsetAsync(scratch, 0, 2 * sizeof(uint32_t), s);
    hipLaunchKernelGGL(k_g_len, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, n, cnt, paths);
    const hipError_t e = launch_scan_counts(n, 0xFFFFFFFFu, cnt, scratch, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_g_emit, dim3((unsigned)((n + 63) / 64)), dim3(64), lds_bytes(12), s, x, n, cnt, scratch, text, base, offsets);
    return hipGetLastError();
}

} // namespace emgpu
