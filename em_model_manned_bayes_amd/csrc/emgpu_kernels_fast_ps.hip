// emgpu_kernels_fast_ps.hip -- the +start instances of the fast kernel (emgpu_kernels_fast.h): a start GRID in one launch (one row of
// presets per trajectory, InitStartTerminal.m:57-90, RUN_uncor.m:35-47) and / or per-sample log-weights, at the fast kernel's pace
// instead of k_dbn_generic's.  A translation unit of their own: they compile beside the other forms, whose objects do not grow.
//   dense   the body of k_uncor_fast_idx: one or both dense outputs, a contiguous range or an index list (the rounds of
//           UncorEncounterModel.track)
//   list    the bodies of k_uncor_fast_evu / _evu_long: the event list alone (what UncorEncounterModel.sample returns)
// The list AND the dense trace with a start grid stay on k_dbn_generic (k_uncor_fast_ev has no registers to spare).
// The presets pointer is an argument of these kernels alone: EmgpuRun, FastArgs and EmgpuPlan are what every other instance gets.
// An instance reports the name of the instance whose body it shares with "+start" appended (choose_dbn).
#include "emgpu_kernels_fast.h"

namespace emgpu {

template <int NI, int M0, int M1, int M2>
__global__ void __launch_bounds__(256, EMGPU_FAST_WAVES) k_uncor_fast_idx_ps(const EmgpuPlan P, const EmgpuRun A, const FastArgs F, const EmgpuPresets *Q) {
    uncor_fast_body<NI, M0, M1, M2, false, false, true, 0, true>(P, A, F, (int64_t)blockIdx.x * 256 - (A.col0 & 255), Q);
}
template <int NI, int M0, int M1, int M2>
__global__ void __launch_bounds__(256, 4) k_uncor_fast_evu_ps(const EmgpuPlan P, const EmgpuRun A, const FastArgs F, const EmgpuPresets *Q) {
    uncor_fast_body<NI, M0, M1, M2, false, true, true, 2, true>(P, A, F, (int64_t)blockIdx.x * 256 - (A.col0 & 255), Q);
}
template <int NI, int M0, int M1, int M2>
__global__ void __launch_bounds__(256, 3) k_uncor_fast_evu_long_ps(const EmgpuPlan P, const EmgpuRun A, const FastArgs F, const EmgpuPresets *Q) {
    uncor_fast_body<NI, M0, M1, M2, false, true, true, 3, true>(P, A, F, (int64_t)blockIdx.x * 256 - (A.col0 & 255), Q);
}

// c.form: Idx (the dense outputs, whichever are asked for), Evu or EvuLong (choose_dbn)
hipError_t launch_uncor_fast_start(const EmgpuPlan &P, const EmgpuRun &A, const FastArgs &F, const DbnChoice &c, const EmgpuPresets *Q, hipStream_t s) {
    if (Q == nullptr) return hipErrorNotSupported;
    const unsigned blocks = fast_blocks(A.n, A.col0);
    if (c.form == FastForm::EvuLong) {
        hipLaunchKernelGGL((k_uncor_fast_evu_long_ps<9, 6, 6, 6>), dim3(blocks), dim3(256), 0, s, P, A, F, Q);
        return hipGetLastError();
    }
    return with_fast_shape(c.shape, [&](auto t) {
        using S = decltype(t);
        if (c.form == FastForm::Idx) hipLaunchKernelGGL((k_uncor_fast_idx_ps<S::NI, S::M0, S::M1, S::M2>), dim3(blocks), dim3(256), 0, s, P, A, F, Q);
        else hipLaunchKernelGGL((k_uncor_fast_evu_ps<S::NI, S::M0, S::M1, S::M2>), dim3(blocks), dim3(256), 0, s, P, A, F, Q);
        return hipGetLastError();
    });
}

} // namespace emgpu
