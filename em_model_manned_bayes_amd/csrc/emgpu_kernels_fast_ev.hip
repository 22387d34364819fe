// emgpu_kernels_fast_ev.hip -- launchers of the event-list forms of the fast kernel (emgpu_kernels_fast.h, emgpu_events.h), a translation
// unit of their own so that they compile beside the dense forms:
//   k_uncor_fast_evu  the list alone (what UncorEncounterModel.sample / dbn_hierarchical_sample return): the rows of a block built 64 at
//                     a time by the wave ("ROWS BY THE WAVE"), any number of rated variables up to 16 - 3; _long: its form for lists of
//                     hundreds of rows per wave and block
//   k_uncor_fast_ev   the list AND the dense trace, at most five rated variables: result slots + a row loop per lane
//   k_uncor_fast_evw  the same for more rated variables (haa_v1: seven), on the widest instance
#include "emgpu_kernels_fast.h"

namespace emgpu {

// c.form: Evu / EvuLong / Evw / Ev (choose_dbn); Evw and EvuLong have the widest instance alone
hipError_t launch_uncor_fast_events(const EmgpuPlan &P, const EmgpuRun &A, const FastArgs &F, const DbnChoice &c, hipStream_t s) {
    const unsigned blocks = fast_blocks(A.n, A.col0);
    switch (c.form) {
    case FastForm::EvuLong: hipLaunchKernelGGL((k_uncor_fast_evu_long<9, 6, 6, 6>), dim3(blocks), dim3(256), 0, s, P, A, F); return hipGetLastError();
    case FastForm::Evu: return EMGPU_FAST_LAUNCH(k_uncor_fast_evu, c.shape, blocks, 0, s, P, A, F);
    case FastForm::Evw: hipLaunchKernelGGL((k_uncor_fast_evw<9, 6, 6, 6>), dim3(blocks), dim3(256), 0, s, P, A, F); return hipGetLastError();
    case FastForm::Ev: return EMGPU_FAST_LAUNCH(k_uncor_fast_ev, c.shape, blocks, 0, s, P, A, F);
    default: return hipErrorNotSupported;
    }
}

} // namespace emgpu
