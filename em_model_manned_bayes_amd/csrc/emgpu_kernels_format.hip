// emgpu_kernels_format.hip -- what UncorEncounterModel.sample hands back (UncorEncounterModel.m:283-300), built on the device from one chunk's
// event lists for emgpu_sample_uncor_host:
//   k_count_controls   rows with dt > 0 per list (one wave per list, lanes across rows);
//   k_ctrl_offsets     their exclusive prefix over the chunk (the workgroup bases come from launch_scan_counts);
//   k_events2samples   events2samples.m:9-26 -- samples[i] as f64 [n_initial][T]: column t of variable v holds the value of the latest row that
//                      names v and ends at at <= t with at < T (at = cumsum(dt) within the list), else init_val[v][i];
//   k_events2controls  events2controls.m:11-31 and the unit conversions of UncorEncounterModel.m:291-297 -- one row [t0, dh / 60,
//                      dpsi * (pi / 180), dv * 1.68780972222222] per row with dt > 0, where t0 is the list time before the row and the three
//                      values are the samples of those variables at column t0; also inits[i] = init_val[.][i] as f64.
// One wave per list in the two writers.  k_events2samples walks the list once per variable with the lanes across 64 columns at a time (the list
// is time-ordered, so a block of columns consumes the rows that end inside it, and its last column carries into the next block): every column
// is written once, 8-byte stores coalesced along T.  k_events2controls takes 64 rows at a time, lanes across rows: the time of each row is a
// wave prefix sum of dt, the value of a variable before row r is the row of the latest lane below r that names it (a ballot), and the control
// rows are packed by a second ballot.  Bound: HBM writes of 8 n_initial T bytes per list (13.4 KB for v2p1 at T = 240), then PCIe.
// Built with -ffp-contract=off: the conversions round like the f64 numpy code (a true IEEE divide by 60, x * (M_PI / 180.0) as np.deg2rad).
#include <hip/hip_runtime.h>

#include <cmath>

#include "emgpu_launch.h"

namespace emgpu {

namespace {
struct Row { uint32_t dt, var; float val; };
__device__ inline Row row_of(uint64_t w) {   // emgpu_event: dt u16 | var u8 | bin u8 | value f32
    Row r;
    r.dt = (uint32_t)(w & 0xFFFFu);
    r.var = (uint32_t)((w >> 16) & 0xFFu);
    r.val = __uint_as_float((uint32_t)(w >> 32));
    return r;
}
__device__ inline int64_t wave_list(int64_t n) {   // this wave's list, or -1 (wave-uniform)
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    return i < n ? i : -1;
}
} // namespace

__global__ void __launch_bounds__(256) k_count_controls(EmgpuFormatRun F) {
    const int64_t i = wave_list(F.n);
    if (i < 0) return;
    const uint32_t lane = threadIdx.x & 63u, c = min(F.ev_count[i], F.cap);
    const uint64_t *L = F.ev + (size_t)i * F.cap;
    uint32_t k = 0;
    for (uint32_t b = 0; b < c; b += 64) {
        const uint32_t r = b + lane;
        k += (uint32_t)__popcll(__ballot(r < c && (L[r] & 0xFFFFu) != 0u));
    }
    if (lane == 0) F.ctrl_count[i] = k;
}

__global__ void __launch_bounds__(256) k_ctrl_offsets(EmgpuFormatRun F) {
    __shared__ uint32_t s_w[4];
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t c = i < F.n ? F.ctrl_count[i] : 0u;
    uint32_t inc = c;   // inclusive scan over the wave's 64 lists
    for (int d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(inc, d, 64); if (lane >= (uint32_t)d) inc += v; }
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    uint32_t base = F.scratch[2 + blockIdx.x];
    for (uint32_t q = 0; q < w; q++) base += s_w[q];
    if (i < F.n) F.ctrl_off[i] = base + inc - c;
}

__global__ void __launch_bounds__(256) k_events2samples(EmgpuFormatRun F) {
    const int64_t i = wave_list(F.n);
    if (i < 0) return;
    const int32_t lane = (int32_t)(threadIdx.x & 63u), T = F.T;
    const uint32_t c = min(F.ev_count[i], F.cap);
    const uint64_t *L = F.ev + (size_t)i * F.cap;
    double *S = F.samples + (size_t)i * (size_t)F.ni * (size_t)T;
    for (int32_t v = 0; v < F.ni; v++) {
        double carry = (double)F.init_val[(size_t)v * (size_t)F.ld + (size_t)i];
        uint32_t r = 0, at = 0;
        for (int32_t t0 = 0; t0 < T; t0 += 64) {
            const int32_t t = t0 + lane;
            const uint32_t last = (uint32_t)t0 + 63u;
            double cur = carry;
            for (; r < c; r++) {   // the rows that end inside this block of columns, in order
                const Row e = row_of(L[r]);
                const uint32_t a = at + e.dt;
                if (a > last) break;
                if (e.var == (uint32_t)(v + 1) && a < (uint32_t)T && a <= (uint32_t)t) cur = (double)e.val;
                at = a;
            }
            if (t < T) S[(size_t)v * (size_t)T + (size_t)t] = cur;
            carry = __shfl(cur, 63, 64);
        }
    }
}

__global__ void __launch_bounds__(256) k_events2controls(EmgpuFormatRun F) {
    const int64_t i = wave_list(F.n);
    if (i < 0) return;
    const uint32_t lane = threadIdx.x & 63u, c = min(F.ev_count[i], F.cap);
    const uint64_t below = (1ull << lane) - 1ull;
    const uint64_t *L = F.ev + (size_t)i * F.cap;
    if ((int32_t)lane < F.ni) F.inits[(size_t)i * (size_t)F.ni + lane] = (double)F.init_val[(size_t)lane * (size_t)F.ld + (size_t)i];
    const int32_t id[3] = {F.id_dh, F.id_dpsi, F.id_dv};
    double x[3];   // the value of each control variable before the current block of rows (wave-uniform)
    for (int k = 0; k < 3; k++) x[k] = (double)F.init_val[(size_t)(id[k] - 1) * (size_t)F.ld + (size_t)i];
    uint32_t at0 = 0, out = F.ctrl_off[i];
    for (uint32_t b = 0; b < c; b += 64) {
        const uint32_t r = b + lane;
        const bool valid = r < c;
        const Row e = valid ? row_of(L[r]) : Row{0u, 0u, 0.f};
        uint32_t inc = e.dt;   // inclusive scan of dt over the block
        for (int d = 1; d < 64; d <<= 1) { const uint32_t v = __shfl_up(inc, d, 64); if (lane >= (uint32_t)d) inc += v; }
        const uint32_t at = at0 + inc, t0 = at - e.dt;
        double xv[3];
        for (int k = 0; k < 3; k++) {
            // rows below this one that set variable k (they all end at or before t0); the latest wins
            const uint64_t m = __ballot(valid && e.var == (uint32_t)id[k] && at < (uint32_t)F.T);
            const uint64_t mb = m & below;
            const int src = mb ? 63 - __clzll((long long)mb) : 0;
            const float sv = __shfl(e.val, src, 64);
            xv[k] = mb ? (double)sv : x[k];
            if (m) x[k] = (double)__shfl(e.val, 63 - __clzll((long long)m), 64);
        }
        const bool crow = valid && e.dt > 0u;
        const uint64_t cm = __ballot(crow);
        if (crow) {
            double *o = F.controls + 4 * (size_t)(out + (uint32_t)__popcll(cm & below));
            o[0] = (double)t0;
            o[1] = xv[0] / 60.0;                  // dh: fpm -> fps          :295
            o[2] = xv[1] * (M_PI / 180.0);        // dpsi: deg/s -> rad/s    :296 (np.deg2rad)
            o[3] = xv[2] * 1.68780972222222;      // dv: kt/s -> ft/s^2      :297
        }
        out += (uint32_t)__popcll(cm);
        at0 += __shfl(inc, 63, 64);
    }
}

hipError_t launch_format_uncor(const EmgpuFormatRun &F, hipStream_t s) {
    if (F.n <= 0) return hipMemsetAsync(F.scratch, 0, 2 * sizeof(uint32_t), s);
    const unsigned nw = (unsigned)((F.n + 3) / 4), nb = (unsigned)((F.n + 255) / 256);
    hipLaunchKernelGGL(k_count_controls, dim3(nw), dim3(256), 0, s, F);
    hipError_t e = launch_scan_counts(F.n, 0xFFFFFFFFu, F.ctrl_count, F.scratch, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_ctrl_offsets, dim3(nb), dim3(256), 0, s, F);
    hipLaunchKernelGGL(k_events2controls, dim3(nw), dim3(256), 0, s, F);
    if (F.samples) hipLaunchKernelGGL(k_events2samples, dim3(nw), dim3(256), 0, s, F);
    return hipGetLastError();
}

} // namespace emgpu
