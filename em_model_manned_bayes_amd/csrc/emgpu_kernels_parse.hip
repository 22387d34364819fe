// emgpu_kernels_parse.hip -- the numeric text tables of the file pipeline (initial.txt, transition.txt) parsed on the device, for
// emgpu_parse_table_host and emgpu_tracks_text_host (readtable(..., 'Delimiter', ' ', 'HeaderLines', 1), sample2track.m:69-72), and the grouping of
// the transition rows by id (sample2track.m:192-193) without a sort.
//
// Rows.  A row is a line that holds more than separators.  k_parse_count counts, per tile of 64 bytes, the rows that BEGIN there (a byte behind
// a newline, or byte 0 of the chunk, whose line is not blank); launch_scan_counts -- the scan the event packer and the text writer use -- turns the
// counts into each tile's first row; k_parse_rows finds its tile's rows again and parses them.
// k_parse_rows: one lane per TILE, not per row: the lane that found a row start parses that row at once (a row of em_sample is 10 .. 60 bytes, so a
// tile holds one to six of them and the lanes of a wave stay within a factor of their neighbours' work).  Bytes are read as aligned dwords from
// global memory (every dword once per lane that walks it, out of L2 / the vector cache, whose lines the wave's 64 consecutive tiles cover exactly);
// staging lines into LDS would add a pass for bytes that are each looked at once, and sub-dword LDS reads are no cheaper than the shifts here.
//
// Values.  Exact: the digits of the mantissa go into a 64-bit integer w, the decimal exponent into d; when w < 2^53 and |d| <= 22 the value is
// w * 10^d or w / 10^-d, one IEEE operation on two exactly representable doubles (Clinger's fast path; the library is built with
// -ffp-contract=off and without fast-math: the divide is IEEE's).  Every other token is HARD: its table position and byte offset go into a list
// and the host finishes it with strtod.  nan / inf / infinity are written here.  Grammar: include/emgpu.h, emgpu_parse_table_host.
#include <hip/hip_runtime.h>

#include "emgpu_launch.h"

namespace emgpu {
namespace {

__device__ const double kP10d[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

// the chunk's bytes through aligned dwords
struct Bytes {
    const uint32_t *w;
    uint32_t n;          // bytes of the chunk
    uint32_t cur = 0, at = 0xFFFFFFFFu;
    __device__ __forceinline__ uint32_t get(uint32_t p) {   // byte p, or '\n' behind the end (a last line without its newline ends like any other)
        if (p >= n) return '\n';
        if ((p >> 2) != at) { at = p >> 2; cur = w[at]; }
        return (cur >> (8u * (p & 3u))) & 255u;
    }
};
__device__ __forceinline__ bool is_sep(uint32_t c) { return c == ' ' || c == '\t'; }
__device__ __forceinline__ bool is_digit(uint32_t c) { return c - '0' < 10u; }
// the end of the line at p: '\n' (or the end of the chunk), or a '\r' directly in front of one
__device__ __forceinline__ bool at_eol(Bytes &B, uint32_t p) {
    const uint32_t c = B.get(p);
    return c == '\n' || (c == '\r' && B.get(p + 1) == '\n');
}
// the line that begins at p holds more than separators
__device__ __forceinline__ bool is_row(Bytes &B, uint32_t p) {
    if (p >= B.n) return false;
    while (is_sep(B.get(p))) p++;
    return !at_eol(B, p);
}

// rows that begin in tile `tile`; F(p) is called for each
template <class F>
__device__ __forceinline__ uint32_t tile_rows(Bytes &B, uint32_t tile, F f) {
    const uint32_t p0 = tile * kParseTile, p1 = min(p0 + kParseTile, B.n);
    uint32_t c = 0;
    bool start = p0 == 0 || B.get(p0 - 1) == '\n';
    for (uint32_t p = p0; p < p1; p++) {
        const uint32_t ch = B.get(p);
        if (start && (is_sep(ch) || ch == '\r' ? is_row(B, p) : ch != '\n')) { f(p, c); c++; }
        start = ch == '\n';
    }
    return c;
}

__global__ void __launch_bounds__(256) k_parse_count(EmgpuParseRun P, uint32_t tiles) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= tiles) return;
    Bytes B{reinterpret_cast<const uint32_t *>(P.text), P.nbytes};
    P.cnt[i] = tile_rows(B, i, [](uint32_t, uint32_t) {});
}

// one token at p (not a separator, not the end of the line): the value, or hard; p moves behind it.  false: not a number of the grammar
__device__ inline bool parse_token(Bytes &B, uint32_t &p, double &val, bool &hard) {
    uint32_t c = B.get(p);
    bool neg = false;
    if (c == '+' || c == '-') { neg = c == '-'; c = B.get(++p); }
    hard = false;
    if (is_digit(c) || c == '.') {
        uint64_t w = 0;
        int d = 0;
        bool any = false, longer = false;
        for (; is_digit(c); c = B.get(++p)) {
            any = true;
            if (w < 1000000000000000000ull) w = w * 10u + (c - '0');
            else { longer = true; d++; }
        }
        if (c == '.') {
            for (c = B.get(++p); is_digit(c); c = B.get(++p)) {
                any = true;
                if (w < 1000000000000000000ull) { w = w * 10u + (c - '0'); d--; }
                else longer = true;
            }
        }
        if (!any) return false;
        if ((c | 0x20u) == 'e') {
            c = B.get(++p);
            bool eneg = false;
            if (c == '+' || c == '-') { eneg = c == '-'; c = B.get(++p); }
            if (!is_digit(c)) return false;
            int e = 0;
            for (; is_digit(c); c = B.get(++p)) e = min(e * 10 + (int)(c - '0'), 100000);
            d += eneg ? -e : e;
        }
        if (longer || w >= (1ull << 53) || d > 22 || d < -22) { hard = true; val = 0.0; return true; }
        const double x = (double)(long long)w;
        val = d >= 0 ? x * kP10d[d] : x / kP10d[-d];
        if (neg) val = -val;
        return true;
    }
    // nan | inf | infinity, any letter case
    const char *word = nullptr;
    int len = 0;
    if ((c | 0x20u) == 'n') { word = "nan"; len = 3; }
    else if ((c | 0x20u) == 'i') { word = "infinity"; len = 8; }
    else return false;
    int k = 0;
    while (k < len && (B.get(p) | 0x20u) == (uint32_t)word[k]) { p++; k++; }
    if (!(k == len || (len == 8 && k == 3))) return false;
    val = __longlong_as_double((long long)((neg ? 0x8000000000000000ull : 0ull) | (len == 3 ? 0x7FF8000000000000ull : 0x7FF0000000000000ull)));
    return true;
}

// the row at p into table row `row`; false: malformed
__device__ inline bool parse_row(const EmgpuParseRun &P, Bytes &B, uint32_t p, int64_t row) {
    for (int c = 0; c < P.ncol; c++) {
        while (is_sep(B.get(p))) p++;
        if (at_eol(B, p)) return false;   // too few
        const uint32_t tok = p;
        double v;
        bool hard;
        if (!parse_token(B, p, v, hard)) return false;
        if (!is_sep(B.get(p)) && !at_eol(B, p)) return false;   // something clings to the number
        const uint64_t pos = (uint64_t)row * (uint64_t)P.ncol + (uint64_t)c;
        if (row >= P.table_rows) continue;   // (only a file with malformed rows has more rows than its bytes allow: they are still looked at)
        P.table[pos] = v;
        if (hard) {
            const uint32_t k = atomicAdd(P.hard_count, 1u);
            if (k < P.hard_cap) P.hard[k] = EmgpuHardToken{pos, tok, 0u};
        }
    }
    while (is_sep(B.get(p))) p++;
    return at_eol(B, p);   // else: too many
}

__global__ void __launch_bounds__(256) k_parse_rows(EmgpuParseRun P, uint32_t tiles) {
    __shared__ uint32_t s_w[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t c = i < tiles ? P.cnt[i] : 0u;
    uint32_t inc = c;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(inc, d, 64); if (lane >= (uint32_t)d) inc += v; }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    uint32_t base = P.scratch[2 + blockIdx.x] + inc - c;
    for (uint32_t q = 0; q < wv; q++) base += s_w[q];
    if (!c) return;
    Bytes B{reinterpret_cast<const uint32_t *>(P.text), P.nbytes};
    (void)tile_rows(B, i, [&](uint32_t p, uint32_t k) {
        const uint32_t r = base + k;
        if (r >= P.rows) return;   // (cannot happen: the counts are this function's own)
        Bytes R{B.w, B.n};
        if (!parse_row(P, R, p, P.row_base + (int64_t)r)) atomicMin(P.err, (unsigned long long)p);
    });
}

__global__ void __launch_bounds__(256) k_parse_patch(double *table, const EmgpuHardToken *hard, const double *val, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) table[hard[i].pos] = val[i];
}

// ---- runs of equal ids
__device__ __forceinline__ double id_of(const EmgpuRunTable &G, int64_t r) { return G.table[(size_t)r * (size_t)G.ncol]; }
__device__ __forceinline__ unsigned long long key_of(double id) {   // ids are compared as doubles: -0 is 0
    return id == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(id);
}
__device__ __forceinline__ uint32_t slot_of(unsigned long long k, uint32_t mask) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33;
    return (uint32_t)k & mask;
}

__global__ void __launch_bounds__(256) k_run_mark(EmgpuRunTable G) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r < G.R) G.cnt[r] = (r == 0 || id_of(G, r) != id_of(G, r - 1)) ? 1u : 0u;
}

__global__ void __launch_bounds__(256) k_run_fill(EmgpuRunTable G) {
    __shared__ uint32_t s_w[4];
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t c = r < G.R ? G.cnt[r] : 0u;
    uint32_t inc = c;
    for (int d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(inc, d, 64); if (lane >= (uint32_t)d) inc += v; }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    uint32_t j = G.scratch[2 + blockIdx.x] + inc - c;
    for (uint32_t q = 0; q < wv; q++) j += s_w[q];
    if (!c) return;
    const double id = id_of(G, r);
    G.run_id[j] = id;
    G.run_first[j] = r;
    if (id != id) return;   // a NaN equals no id: its rows belong to no track
    const unsigned long long key = key_of(id);
    for (uint32_t s = slot_of(key, G.mask);; s = (s + 1u) & G.mask) {
        const unsigned long long old = atomicCAS(&G.keys[s], ~0ull, key);
        if (old == ~0ull) { G.vals[s] = j; break; }
        if (old == key) { *G.dup = 1u; break; }   // a second run of this id: the rows are interleaved
    }
}

__global__ void __launch_bounds__(256) k_run_match(EmgpuRunTable G, uint32_t runs, int64_t n, const double *ids, int64_t *first, int32_t *len) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double id = ids[i];
    int64_t f = 0, l = 0;
    if (id == id) {
        const unsigned long long key = key_of(id);
        for (uint32_t s = slot_of(key, G.mask);; s = (s + 1u) & G.mask) {
            const unsigned long long k = G.keys[s];
            if (k == ~0ull) break;
            if (k == key) {
                const uint32_t j = G.vals[s];
                f = G.run_first[j];
                l = (j + 1u < runs ? G.run_first[j + 1u] : G.R) - f;
                break;
            }
        }
    }
    first[i] = f;
    len[i] = (int32_t)l;
}

} // namespace

hipError_t launch_parse_count(const EmgpuParseRun &P, hipStream_t s) {
    const uint32_t tiles = (uint32_t)(((uint64_t)P.nbytes + kParseTile - 1) / kParseTile);
    if (tiles) hipLaunchKernelGGL(k_parse_count, dim3((tiles + 255u) / 256u), dim3(256), 0, s, P, tiles);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : launch_scan_counts((int64_t)tiles, 0xFFFFFFFFu, P.cnt, P.scratch, s);
}

hipError_t launch_parse_rows(const EmgpuParseRun &P, hipStream_t s) {
    const uint32_t tiles = (uint32_t)(((uint64_t)P.nbytes + kParseTile - 1) / kParseTile);
    if (!tiles || !P.rows) return hipSuccess;
    hipLaunchKernelGGL(k_parse_rows, dim3((tiles + 255u) / 256u), dim3(256), 0, s, P, tiles);
    return hipGetLastError();
}

hipError_t launch_parse_patch(double *table, const EmgpuHardToken *hard, const double *val, uint32_t n, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_parse_patch, dim3((n + 255u) / 256u), dim3(256), 0, s, table, hard, val, n);
    return hipGetLastError();
}

hipError_t launch_run_mark(const EmgpuRunTable &G, hipStream_t s) {
    if (G.R > 0) hipLaunchKernelGGL(k_run_mark, dim3((unsigned)((G.R + 255) / 256)), dim3(256), 0, s, G);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : launch_scan_counts(G.R, 0xFFFFFFFFu, G.cnt, G.scratch, s);
}

hipError_t launch_run_fill(const EmgpuRunTable &G, hipStream_t s) {
    if (G.R <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_run_fill, dim3((unsigned)((G.R + 255) / 256)), dim3(256), 0, s, G);
    return hipGetLastError();
}

hipError_t launch_run_match(const EmgpuRunTable &G, uint32_t runs, int64_t n, const double *ids, int64_t *first, int32_t *len, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_run_match, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, G, runs, n, ids, first, len);
    return hipGetLastError();
}

} // namespace emgpu
