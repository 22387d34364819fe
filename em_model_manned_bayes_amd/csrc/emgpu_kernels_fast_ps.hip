// emgpu_kernels_fast_ps.hip -- the +start instances of the fast kernel (emgpu_kernels_fast.h): a start GRID in one launch (one row of
// presets per trajectory, InitStartTerminal.m:57-90, RUN_uncor.m:35-47) and / or per-sample log-weights, at the fast kernel's pace
// instead of k_dbn_generic's.  A translation unit of their own: they compile beside the other forms, whose objects do not grow.
//   dense   the body of k_uncor_fast_idx: one or both dense outputs, a contiguous range or an index list (the rounds of
//           UncorEncounterModel.track)
//   list    the bodies of k_uncor_fast_evu / _evu_long: the event list alone (what UncorEncounterModel.sample returns)
// The list AND the dense trace with a start grid stay on k_dbn_generic (k_uncor_fast_ev has no registers to spare).
// The presets pointer is an argument of these kernels alone: EmgpuRun, FastArgs and EmgpuPlan are what every other instance gets.
// An instance reports the name of the instance whose body it shares; the dispatcher appends "+start".
#include <stdio.h>

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

// The rules of launch_uncor_fast_events (emgpu_kernels_fast_ev.hip) for the list alone, restated: a call reaches the +start form of the
// instance it would reach without a grid.  EMGPU_DEBUG_EVENT_ROWS: as there ("lane" / "wide" send a list alone to the per-lane row loops,
// which have no +start form: such a call stays on k_dbn_generic; "long" forces the long queue).
static const char *rows_env() { static const char *e = getenv("EMGPU_DEBUG_EVENT_ROWS"); return e; }
static bool uncor_fast_list_alone(const EmgpuPlan &P, const EmgpuRun &A) {
    const char *e = rows_env();
    const bool force_long = e != nullptr && e[0] == 'l' && e[1] == 'o';
    const bool force_lane = e != nullptr && e[0] == 'l' && !force_long, force_wide = e != nullptr && e[0] == 'w' && e[1] == 'i';
    const bool plain = (A.flags & (EMGPU_FLAG_NO_RESAMPLE | EMGPU_FLAG_NO_DEDISC)) != 0;
    return A.dyn_bin == nullptr && A.dyn_val == nullptr && ((!force_lane && !force_wide) || plain) && ev_plan_wide_ok(P, A);
}
static bool uncor_fast_list_long(const EmgpuPlan &P, const EmgpuRun &A) {
    const char *e = rows_env();
    const bool force_long = e != nullptr && e[0] == 'l' && e[1] == 'o';
    double rate = 0.0;   // rows expected per wave and 8-second block from the resample rates alone
    if (!(A.flags & EMGPU_FLAG_NO_RESAMPLE))
        for (int a = 0; a < P.nact; a++) rate += (double)P.a_R[a] * (1.0 / 4294967296.0);
    return rate * 512.0 > 300.0 || (force_long && P.ni <= 9);
}

// 0: none (the call stays on k_dbn_generic), 1: dense, 2: list alone.  The (plan, run) pair is fast_uncor_eligible.
int uncor_fast_start_form(const EmgpuPlan &P, const EmgpuRun &A) {
    if (A.ev_count == nullptr) return 1;
    return uncor_fast_list_alone(P, A) ? 2 : 0;
}

template <int NI, int M0, int M1, int M2>
static hipError_t launch_ps_t(int form, const EmgpuPlan &P, const EmgpuRun &A, const FastArgs &F, const EmgpuPresets *Q, hipStream_t s) {
    const int64_t blocks = (A.n + (A.col0 & 255) + 255) / 256;
    if (form == 1) hipLaunchKernelGGL((k_uncor_fast_idx_ps<NI, M0, M1, M2>), dim3((unsigned)blocks), dim3(256), 0, s, P, A, F, Q);
    else hipLaunchKernelGGL((k_uncor_fast_evu_ps<NI, M0, M1, M2>), dim3((unsigned)blocks), dim3(256), 0, s, P, A, F, Q);
    return hipGetLastError();
}

// name: room for 64 characters; receives the name of the instance whose body runs (without the "+start")
hipError_t launch_uncor_fast_start(const EmgpuPlan &P, const EmgpuRun &A, const EmgpuPresets *Q, hipStream_t s, char *name) {
    name[0] = 0;
    if (A.n <= 0) return hipSuccess;
    const int form = uncor_fast_start_form(P, A), shape = fast_shape_of(P);
    if (form == 0 || shape < 0 || Q == nullptr) return hipErrorNotSupported;
    const FastArgs F = fast_args_of(P);
    if (form == 2 && uncor_fast_list_long(P, A)) {
        const int64_t blocks = (A.n + (A.col0 & 255) + 255) / 256;
        snprintf(name, 64, "%s<%d,%d,%d,%d>", "k_uncor_fast_evu_long", 9, 6, 6, 6);
        hipLaunchKernelGGL((k_uncor_fast_evu_long_ps<9, 6, 6, 6>), dim3((unsigned)blocks), dim3(256), 0, s, P, A, F, Q);
        return hipGetLastError();
    }
    const FastShape &f = kFastShapes[shape];
    snprintf(name, 64, "%s<%d,%d,%d,%d>", form == 1 ? "k_uncor_fast_idx" : "k_uncor_fast_evu", f.ni, f.m0, f.m1, f.m2);
    switch (shape) {
    case 0: return launch_ps_t<7, 2, 2, 2>(form, P, A, F, Q, s);
    case 1: return launch_ps_t<7, 2, 4, 2>(form, P, A, F, Q, s);
    case 2: return launch_ps_t<7, 2, 4, 4>(form, P, A, F, Q, s);
    case 3: return launch_ps_t<7, 4, 2, 4>(form, P, A, F, Q, s);
    case 4: return launch_ps_t<7, 4, 6, 4>(form, P, A, F, Q, s);
    case 5: return launch_ps_t<7, 4, 6, 6>(form, P, A, F, Q, s);
    case 6: return launch_ps_t<7, 6, 6, 6>(form, P, A, F, Q, s);
    case 7: return launch_ps_t<9, 6, 6, 6>(form, P, A, F, Q, s);
    default: return hipErrorNotSupported;
    }
}

} // namespace emgpu
