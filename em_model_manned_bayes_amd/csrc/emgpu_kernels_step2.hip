// emgpu_kernels_step2.hip -- launchers of the general, the frozen and the 4-variable parent-mask instances of k_dbn_step2
// (emgpu_kernels_step2.h); which of them a call runs on: choose_dbn (emgpu_dispatch.h)
#include "emgpu_kernels_step2.h"

namespace emgpu {

// the general instances of a shape: every parent, with or without "reg" and a common width (the event lists: the per-variable-width
// instances only -- half the instances for the rarer output)
template <int NI, int ND>
static hipError_t launch_t(const EmgpuPlan &P, const EmgpuRun &A, const Step2Args &F, const DbnChoice &c, hipStream_t s) {
    const dim3 g((unsigned)((A.n + 255) / 256)), b(256);
    constexpr uint32_t C = ND == 4 ? kCurAll4 : kCurAll3, N = ND == 4 ? kNewAll4 : kNewAll3;
    if (c.ev == 2 && c.reg) hipLaunchKernelGGL((k_dbn_step2<NI, ND, 0, true, C, N, false, 2>), g, b, step2_extra_lds(), s, P, A, F);
    else if (c.ev == 2) hipLaunchKernelGGL((k_dbn_step2<NI, ND, 0, false, C, N, false, 2>), g, b, step2_extra_lds(), s, P, A, F);
    else if (c.ev == 1 && c.reg) hipLaunchKernelGGL((k_dbn_step2<NI, ND, 0, true, C, N, false, 1>), g, b, step2_extra_lds(), s, P, A, F);
    else if (c.ev == 1) hipLaunchKernelGGL((k_dbn_step2<NI, ND, 0, false, C, N, false, 1>), g, b, step2_extra_lds(), s, P, A, F);
    else if (c.wmode == 4) hipLaunchKernelGGL((k_dbn_step2<NI, ND, 4, true, C, N>), g, b, step2_extra_lds(), s, P, A, F);
    else if (c.wmode == 8) hipLaunchKernelGGL((k_dbn_step2<NI, ND, 8, true, C, N>), g, b, step2_extra_lds(), s, P, A, F);
    else if (c.reg) hipLaunchKernelGGL((k_dbn_step2<NI, ND, 0, true, C, N>), g, b, step2_extra_lds(), s, P, A, F);
    else hipLaunchKernelGGL((k_dbn_step2<NI, ND, 0, false, C, N>), g, b, step2_extra_lds(), s, P, A, F);
    return hipGetLastError();
}

// the instances built for the parent masks of the 4-variable families (EMGPU_S2_CASES_ND4)
static hipError_t launch_masked4(const EmgpuPlan &P, const EmgpuRun &A, const Step2Args &F, const DbnChoice &c, hipStream_t s) {
    const dim3 g((unsigned)((A.n + 255) / 256)), b(256);
    int q = 0;
#define EMGPU_S2_CASE(NI_, ND_, W_, C_, N_, TAG_) \
    if (c.mask_case == q++) { EMGPU_S2_LAUNCH(NI_, ND_, W_, true, C_, N_, false); return hipGetLastError(); }
    EMGPU_S2_CASES_ND4
#undef EMGPU_S2_CASE
    return hipErrorNotSupported;
}

Step2Args step2_args_of(const EmgpuPlan &P) {
    Step2Args F{};
    for (int k = 0; k < P.nd; k++) {
        F.slot[k] = P.d_row[k];
        for (int a = 0; a < P.nact; a++)
            if (P.a_dyn[a] == k) F.Rk[k] = P.a_R[a];
        F.RR1[k] = ((F.Rk[k] >> 16) + 1u) * 0x00010001u;
    }
    return F;
}

// (Staging the tables in LDS was measured and dropped: random 16-byte gathers from LDS pay bank
// conflicts and the extra LDS costs a workgroup of occupancy -- cor_v1 36.9 ms staged, 28.9 ms through L1/L2.)
hipError_t launch_dbn_step2(const EmgpuPlan &P0, const EmgpuRun &A, const DbnChoice &c, const EmgpuPresets *Q, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    const EmgpuPlan P = step2_plan(P0, A);
    const Step2Args F = step2_args_of(P);
    if (c.start) return launch_dbn_step2_start(P, A, F, c, Q, s);
    if (c.mask_case >= kStep2CasesNd4) return launch_masked3(P, A, F, c, s);
    if (c.mask_case >= 0) return launch_masked4(P, A, F, c, s);
    if (c.frozen) {   // fast branch: four dynamic variables, or fewer than three
        const dim3 g((unsigned)((A.n + 255) / 256)), b(256);
        if (c.reg) EMGPU_S2_LAUNCH(16, 4, 4, true, 0x8421u, 0u, true);   // littoral_cor_v1: every variable's only dynamic parent is its own current bin
        else EMGPU_S2_LAUNCH(16, 4, 0, false, kCurAll4, 0u, true);
        return hipGetLastError();
    }
    if (c.shape == 0) return launch_t<7, 3>(P, A, F, c, s);
    if (c.shape == 1) return launch_t<9, 3>(P, A, F, c, s);
    return launch_t<16, 4>(P, A, F, c, s);
}

#ifdef EMGPU_DEBUG_COUNTERS
extern "C" int emgpu_debug_counters_step2(unsigned long long *out, int reset) {   // this translation unit's copy of g_dbg
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dbg), sizeof(g_dbg)) != hipSuccess) return -1;
    if (reset) { unsigned long long z[8] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_dbg), z, sizeof z); }
    return 0;
}
#endif

} // namespace emgpu
