// emgpu_kernels_fast.hip -- launchers of the dense forms of the fast kernel (emgpu_kernels_fast.h): k_uncor_fast (the benchmark),
// k_uncor_fast_idx, k_uncor_fast_mixed; a call that wants an event list goes on to emgpu_kernels_fast_ev.hip.
#include "emgpu_kernels_fast.h"

namespace emgpu {

// the forms of the other translation units
hipError_t launch_uncor_fast_events(const EmgpuPlan &P, const EmgpuRun &A, const FastArgs &F, const DbnChoice &c, hipStream_t s);   // emgpu_kernels_fast_ev.hip
hipError_t launch_uncor_fast_start(const EmgpuPlan &P, const EmgpuRun &A, const FastArgs &F, const DbnChoice &c, const EmgpuPresets *Q, hipStream_t s);   // emgpu_kernels_fast_ps.hip

size_t plan_f_bytes() { return sizeof(PlanF); }
void plan_f_fill(const EmgpuPlan &P, void *host_buf) {
    PlanF *pf = static_cast<PlanF *>(host_buf);
    pf->P = P; pf->F = fast_args_of(P);
}

// A: the call's run with the outputs bound at column 0; block b = n[b] trajectories from global index first[b] on, written from
// column col[b] on, with the device-resident plan d_planf[b] (plan_f_fill); all of instance `shape`.
hipError_t launch_uncor_fast_mixed(const EmgpuRun &A, int nb, const void *const *d_planf, const uint64_t *first, const int64_t *n, const int64_t *col,
                                   int shape, hipStream_t s) {
    if (nb < 1 || nb > EMGPU_MAX_MIXED) return hipErrorInvalidValue;
    MixedHead H{};
    H.A = A;
    H.nb = nb;
    uint64_t wg = 0;
    for (int b = 0; b < nb; b++) {
        H.blk[b] = MixedBlock{static_cast<const PlanF *>(d_planf[b]), first[b], n[b], col[b]};
        H.wg_begin[b] = (uint32_t)wg;
        wg += fast_blocks(n[b], A.col0 + col[b]);   // lined up with the trace's columns (k_uncor_fast_mixed)
    }
    for (int b = nb; b <= EMGPU_MAX_MIXED; b++) H.wg_begin[b] = (uint32_t)wg;
    for (int b = nb; b < EMGPU_MAX_MIXED; b++) H.blk[b] = H.blk[nb - 1];
    if (wg == 0) return hipSuccess;
    if (wg > 0x7FFFFFFFull) return hipErrorInvalidValue;
    return EMGPU_FAST_LAUNCH(k_uncor_fast_mixed, shape, (unsigned)wg, 0, s, H);
}

hipError_t launch_uncor_fast(const EmgpuPlan &P, const EmgpuRun &A, const DbnChoice &c, const EmgpuPresets *Q, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    const FastArgs F = fast_args_of(P);
    if (c.start) return launch_uncor_fast_start(P, A, F, c, Q, s);
    if (c.form == FastForm::Idx) return EMGPU_FAST_LAUNCH(k_uncor_fast_idx, c.shape, fast_blocks(A.n, A.col0), 0, s, P, A, F);
    if (c.form != FastForm::Dense) return launch_uncor_fast_events(P, A, F, c, s);
    // EMGPU_DEBUG_EXTRA_LDS: bytes of unused dynamic LDS per workgroup, to study occupancy sensitivity
    static const int extra_lds = getenv("EMGPU_DEBUG_EXTRA_LDS") ? atoi(getenv("EMGPU_DEBUG_EXTRA_LDS")) : 0;
    return EMGPU_FAST_LAUNCH(k_uncor_fast, c.shape, fast_blocks(A.n, A.col0), (size_t)extra_lds, s, P, A, F);
}

#ifdef EMGPU_DEBUG_COUNTERS
extern "C" int emgpu_debug_counters(unsigned long long *out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dbg), sizeof(g_dbg)) != hipSuccess) return -1;
    if (reset) { unsigned long long z[8] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_dbg), z, sizeof z); }
    return 0;
}
#endif

} // namespace emgpu
