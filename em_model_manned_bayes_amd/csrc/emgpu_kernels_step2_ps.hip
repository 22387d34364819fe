// emgpu_kernels_step2_ps.hip -- the +start instances of k_dbn_step2 (emgpu_kernels_step2.h): a start GRID in one launch (one row of presets
// per trajectory, InitStartTerminal.m:57-90, RUN_uncor.m:35-47) and / or per-sample log-weights for the models k_uncor_fast does not take
// (cor_v1, littoral_cor_v1, the dependent-branch family, EMGPU_TRANSITION_PER_STEP), at the per-timestep kernel's pace instead of
// k_dbn_generic's.  A translation unit of their own: they compile beside the other instances, whose objects do not change.
// Only the GENERAL instance of each shape has a twin here (not "reg", widths left to run time, every parent: it takes every
// step2_eligible model of its shape), in two forms:
//   dense   EV = 0: one or both dense outputs (null-tested stores)
//   list    EV = 2: the event list alone, its rows built by the wave
// The list AND the dense trace with a start grid stay on k_dbn_generic, and so does an index list (not step2_eligible).
// The presets pointer is an argument of these kernels alone: EmgpuPlan, EmgpuRun and Step2Args are what every other instance gets, and the
// plan is still at offset 0 of the kernel-argument segment.
#include "emgpu_kernels_step2.h"

namespace emgpu {

// The 16-variable twins read the initial network -- the lane's presets included -- through the kernel-argument segment
// (init_network_ps_karg); the list twins then need fewer registers than the instances whose body they share (139 / 134 against 153, three
// waves per SIMD either way).  The DENSE 16-variable twins are the one exception to "the same waves per SIMD as the shared body": the
// four-wave form of that body (step2_sc_form, 128 registers) already spills 15 / 5 vector registers without presets, and a +start kernel may
// spill none, so these two are built for three waves in the LBK form (requests looked up in the owner's LDS row, rows of 44 words): 142 /
// 138 registers, no vector spill.
template <int NI, int ND, uint32_t CUR, uint32_t NEW, bool FRZ, int EV>
__global__ void __launch_bounds__(256, ND == 4 ? 3 : 4) k_dbn_step2_ps(const EmgpuPlan P, const EmgpuRun A, const Step2Args F, const EmgpuPresets *Q) {
    constexpr int WMODE = 0;
    constexpr bool REG = false, PS = true;
#include "emgpu_kernels_step2_body.h"
}

template <int NI, int ND, uint32_t CUR, uint32_t NEW, bool FRZ>
static hipError_t launch_ps_t(const EmgpuPlan &P, const EmgpuRun &A, const Step2Args &F, const DbnChoice &c, const EmgpuPresets *Q, hipStream_t s) {
    const dim3 g((unsigned)((A.n + 255) / 256)), b(256);
    if (c.ev == 0) hipLaunchKernelGGL((k_dbn_step2_ps<NI, ND, CUR, NEW, FRZ, 0>), g, b, step2_extra_lds(), s, P, A, F, Q);
    else hipLaunchKernelGGL((k_dbn_step2_ps<NI, ND, CUR, NEW, FRZ, 2>), g, b, step2_extra_lds(), s, P, A, F, Q);
    return hipGetLastError();
}

// P, F: the call's step2_plan and its arguments; c.ev: 0 or 2 (choose_dbn)
hipError_t launch_dbn_step2_start(const EmgpuPlan &P, const EmgpuRun &A, const Step2Args &F, const DbnChoice &c, const EmgpuPresets *Q, hipStream_t s) {
    if (Q == nullptr || c.ev == 1) return hipErrorNotSupported;
    if (c.shape == 0) return launch_ps_t<7, 3, kCurAll3, kNewAll3, false>(P, A, F, c, Q, s);
    if (c.shape == 1) return launch_ps_t<9, 3, kCurAll3, kNewAll3, false>(P, A, F, c, Q, s);
    if (!c.frozen) return launch_ps_t<16, 4, kCurAll4, kNewAll4, false>(P, A, F, c, Q, s);
    return launch_ps_t<16, 4, kCurAll4, 0u, true>(P, A, F, c, Q, s);
}

} // namespace emgpu
