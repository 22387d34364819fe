// emgpu_dispatch.h -- which kernel instance a sampling call runs on.  choose_dbn decides once per call, on the host, from the plan and
// the run alone (it reads no device memory and calls no HIP function); the launchers of emgpu_launch.h take its choice and only launch.
// The shape tables, the name tables and the list of parent-mask cases the choice is made from live here and in emgpu_dispatch.cpp;
// no kernel text.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "emgpu_plan.h"

namespace emgpu {

// ---- the fast kernel's instances <NI,M0,M1,M2>, by the number of DISTINCT thresholds per column of the three dynamic variables
// (EmgpuPlan::d_meff): X(shape index, NI, M0, M1, M2).  A model runs on the first instance that covers it.
#define EMGPU_FAST_SHAPES(X) \
    X(0, 7, 2, 2, 2) X(1, 7, 2, 4, 2) X(2, 7, 2, 4, 4) X(3, 7, 4, 2, 4) X(4, 7, 4, 6, 4) X(5, 7, 4, 6, 6) X(6, 7, 6, 6, 6) X(7, 9, 6, 6, 6)
constexpr int kFastWidest = 7;   // <9,6,6,6>: the one instance of k_uncor_fast_evw and k_uncor_fast_evu_long
// workgroups of a fast-kernel launch: workgroup w covers columns [256 w, 256 w + 256) of the TRACE, so n trajectories written from column
// col on lead with col mod 256 idle lanes
inline unsigned fast_blocks(int64_t n, int64_t col) { return (unsigned)((n + (col & 255) + 255) / 256); }

// ---- the instances of k_dbn_step2 built for the parent masks (step_parent_masks) of the shipped model families, regular models only:
// EMGPU_S2_CASE(NI, ND, W, CUR, NEW, tag) takes a call with or without the event list (W: 4 / 8 = every column that wide, 0 = widths
// decided per variable at run time), EMGPU_S2_CASE_W(NI, ND, WM, CUR, NEW, tag) the dense outputs only (WM: mask of the 4-word variables,
// WMODE 16 + WM).  The first case that fits is taken.  choose_dbn and the launchers expand the same lists: DbnChoice::mask_case counts
// through EMGPU_S2_CASES_ND4 (emgpu_kernels_step2.hip), then through EMGPU_S2_CASES_ND3 (emgpu_kernels_step2b.hip).
#define EMGPU_S2_CASES_ND4 \
    EMGPU_S2_CASE(16, 4, 4, 0x8421u, 0x2100u, "[cor]")   /* cor_v1: two independent aircraft, turn rate after vertical rate */ \
    EMGPU_S2_CASE(16, 4, 8, 0x8421u, 0x2100u, "[cor]")
#define EMGPU_S2_CASES_ND3 \
    EMGPU_S2_CASE_W(7, 3, 4, 0x0421u, 0x0310u, "[chain,w884]")       /* glider_v1 */ \
    EMGPU_S2_CASE_W(7, 3, 0, 0x0421u, 0x0310u, "[chain,w888]")       /* paraglider_v1 */ \
    EMGPU_S2_CASE_W(7, 3, 7, 0x0421u, 0x0210u, "[2<-1,w444]")        /* littoral_uncor_v1 */ \
    EMGPU_S2_CASE_W(7, 3, 4, 0x0421u, 0x0210u, "[2<-1,w884]")        /* paramotor_v1 */ \
    EMGPU_S2_CASE_W(7, 3, 5, 0x0421u, 0x0210u, "[2<-1,w484]")        /* skydiving_v1 */ \
    EMGPU_S2_CASE_W(7, 3, 0, 0x0421u, 0x0110u, "[1<-0,2<-0,w888]")   /* fai1_v1 */ \
    EMGPU_S2_CASE_W(7, 3, 2, 0x0421u, 0x0110u, "[1<-0,2<-0,w848]")   /* fai5_v1 */ \
    EMGPU_S2_CASE_W(7, 3, 6, 0x0421u, 0x0300u, "[2<-0,1,w844]")      /* uncor_1200code_v1 */ \
    EMGPU_S2_CASE_W(7, 3, 5, 0x0577u, 0x0000u, "[per-step,w484]")    /* uncor_1200code_v2p1 under EMGPU_TRANSITION_PER_STEP */ \
    EMGPU_S2_CASE_W(7, 3, 0, 0x0577u, 0x0000u, "[per-step,w888]")    /* the v1.2 and allcode families under EMGPU_TRANSITION_PER_STEP */ \
    EMGPU_S2_CASE(7, 3, 0, 0x0421u, 0x0310u, "[chain]")              /* glider_v1, paraglider_v1 */ \
    EMGPU_S2_CASE(7, 3, 0, 0x0421u, 0x0210u, "[2<-1]")               /* littoral_uncor_v1, paramotor_v1, skydiving_v1 */ \
    EMGPU_S2_CASE(7, 3, 0, 0x0421u, 0x0110u, "[1<-0,2<-0]")          /* fai1_v1, fai5_v1 */ \
    EMGPU_S2_CASE(7, 3, 0, 0x0421u, 0x0300u, "[2<-0,1]")             /* uncor_1200code_v1 */ \
    EMGPU_S2_CASE(7, 3, 0, 0x0577u, 0x0000u, "[per-step]")           /* EMGPU_TRANSITION_PER_STEP on the conventional uncorrelated models */

// which dynamic variables are parents of which in the transition network, as the per-timestep kernel's instances see it:
// bit 4k+q of cur_mask: the time-t node of dynamic variable q is a parent of (t+1) node k; of new_mask: its (t+1) node is (q < k)
void step_parent_masks(const EmgpuPlan &P, uint32_t *cur_mask, uint32_t *new_mask);
// the plan k_dbn_step2 runs a call on: EMGPU_FLAG_NO_RESAMPLE leaves no variable a rate (no resample stream, no resample pass)
EmgpuPlan step2_plan(const EmgpuPlan &P, const EmgpuRun &A);

enum class DbnFamily : int32_t { Fast, Step2, Step, Generic };
enum class FastForm : int32_t {
    Dense,     // k_uncor_fast: both dense outputs of a contiguous range
    Idx,       // k_uncor_fast_idx: an index list, or only one of the dense outputs
    Ev,        // k_uncor_fast_ev: the list AND the dense trace, at most five rated variables
    Evw,       // k_uncor_fast_evw: the same for more rated variables, on the widest instance
    Evu,       // k_uncor_fast_evu: the list alone, its rows built by the wave
    EvuLong,   // k_uncor_fast_evu_long: its form for lists of hundreds of rows per wave and block, on the widest instance
};

struct DbnChoice {
    DbnFamily family;
    bool start;        // the +start twin of a Fast or Step2 instance runs (k_dbn_generic takes presets as it is)
    // Fast: shape = index into EMGPU_FAST_SHAPES.  Step2, Step: 0 <7,3>, 1 <9,3>, 2 <16,4>.  Generic: 0 <7,3,4>, 1 <7,3,7>, 2 <9,3,9>, 3 <16,4,4>, 4 <16,4,16>
    int32_t shape;
    FastForm form;     // Fast
    // Step2: the instance's template arguments beside the shape
    int32_t wmode;     // WMODE: 4 / 8, or 0 = decided per variable at run time (a mask case: as its list entry says)
    bool reg, frozen;  // REG, FRZ
    int32_t mask_case; // -1: the instance of every parent (or, frozen and reg, of each variable's own current bin); else the entry of the case lists
    int32_t ev;        // EV: 0 the dense trace, 1 the event list as well, 2 the list alone with its rows built by the wave
    // Step
    bool lds, compact; // the tables staged in LDS (lds_bytes of them) / read in their compact form
    size_t lds_bytes;
    char name[96];     // what ctx.last_kernel() reports
};

// presets: the call carries a start grid / per-sample log-weights
DbnChoice choose_dbn(const EmgpuPlan &P, const EmgpuRun &A, bool presets);
// the name of the mixed-batch launch of the blocks whose choice is (Fast, Dense, shape)
const char *uncor_fast_mixed_name(int shape);

} // namespace emgpu
