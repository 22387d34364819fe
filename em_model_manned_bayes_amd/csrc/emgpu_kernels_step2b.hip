// emgpu_kernels_step2b.hip -- the instances of k_dbn_step2 (emgpu_kernels_step2.h) built for the parent masks and column widths of the
// shipped 3-variable model families; a translation unit of its own so that they compile beside the 4-variable ones.
#include "emgpu_kernels_step2.h"

namespace emgpu {

// (dense output only for the width-specific ones, WMODE 16 + mask of the 4-word variables: a width decided at run time is a
// wave-uniform branch per draw with both forms of the draw behind it)
hipError_t launch_masked3(const EmgpuPlan &P, const EmgpuRun &A, const Step2Args &F, const DbnChoice &c, hipStream_t s) {
    const dim3 g((unsigned)((A.n + 255) / 256)), b(256);
    int q = kStep2CasesNd4;
#define EMGPU_S2_CASE(NI_, ND_, W_, C_, N_, TAG_) \
    if (c.mask_case == q++) { EMGPU_S2_LAUNCH(NI_, ND_, W_, true, C_, N_, false); return hipGetLastError(); }
#define EMGPU_S2_CASE_W(NI_, ND_, WM_, C_, N_, TAG_)                                                                                      \
    if (c.mask_case == q++) {                                                                                                            \
        hipLaunchKernelGGL((k_dbn_step2<NI_, ND_, 16 + WM_, true, C_, N_, false, false>), g, b, step2_extra_lds(), s, P, A, F);          \
        return hipGetLastError();                                                                                                        \
    }
    EMGPU_S2_CASES_ND3
#undef EMGPU_S2_CASE_W
#undef EMGPU_S2_CASE
    return hipErrorNotSupported;
}

#ifdef EMGPU_DEBUG_COUNTERS
extern "C" int emgpu_debug_counters_step2b(unsigned long long *out, int reset) {   // this translation unit's copy of g_dbg
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dbg), sizeof(g_dbg)) != hipSuccess) return -1;
    if (reset) { unsigned long long z[8] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_dbg), z, sizeof z); }
    return 0;
}
#endif

} // namespace emgpu
