#pragma once
// emgpu_kernels_step2.h -- (the kernel; its instances are spread over emgpu_kernels_step2.hip, emgpu_kernels_step2b.hip and emgpu_kernels_step2_ps.hip so that they compile side by side)
// k_dbn_step2 -- the per-timestep DBN (dbn_sample.m:65-93: dependent-branch models such as
// cor_v1 and the glider family, and EMGPU_TRANSITION_PER_STEP) with dense output, built like
// k_uncor_fast: one lane = one trajectory, 8 seconds per loop iteration, packed 16-bit compares
// on the primary (high) halfwords, MSB-first flag streams, wave-cooperative dediscretize.
//
// What differs from the fast-branch kernel: a variable's CPT column changes every second with the
// dynamic state (asub2ind.m:13-14 as strides over the current and the freshly drawn bins), so the
// column is fetched per draw with ONE 16-byte gather through L1/L2 (a buffer resource, byte offsets): its packed-compare form
// (EmgpuPlan::d_poffpk: three T' pairs + the nibble map by fired count), whatever the column's width.
// The columns of one dependency level are gathered together, the next second's level-0 columns as soon as this second's
// level 0 is decided.  The secondary (low) halfword block of a variable is generated only at a second where
// some lane of the wave met a tie between a draw's high halfword and a threshold's (p = 2^-16 per
// compare); the draw is then redone with the full 32 bits, in place, because later seconds depend on it.
// Interior blocks run unguarded; the first block of a trajectory and a partial last one take a rolled loop on full draws.
// Bound: VALU issue (Philox + ~16 instructions per draw, 84 % of the cycles on cor_v1) and one exposed L1/L2 round trip per second.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "emgpu_coop.h"
#include "emgpu_device.h"
#include "emgpu_events.h"
#include "emgpu_launch.h"

namespace emgpu {


struct Step2Args {
    uint32_t Rk[EMGPU_MAX_ND];   // resample hit threshold of dynamic variable k (0 = rate 0), < 0xFFFF0000
    uint32_t slot[EMGPU_MAX_ND]; // output row of dynamic variable k
    uint32_t RR1[EMGPU_MAX_ND];  // (Rk >> 16) + 1 in both halfwords: the packed resample compare of a whole block
};

// Dependency level of (t+1) node k among the dynamic variables: 0 when none of its parents is another (t+1) node, else one more than
// the deepest such parent (NEW: bit 4k+q <=> the (t+1) node of q is a parent of k, q < k).  The columns of one level are fetched
// together: their round trips through L1/L2 overlap instead of following each other.
template <uint32_t NEW>
constexpr int s2_level(int k) {
    int l = 0;
    for (int q = 0; q < k; q++)
        if ((NEW >> (4 * k + q)) & 1u) { const int lq = s2_level<NEW>(q) + 1; l = lq > l ? lq : l; }
    return l;
}

template <uint32_t CUR, uint32_t NEW>
constexpr bool s2_pre(int k) {
    if (s2_level<NEW>(k) != 0) return false;
    for (int q = 0; q < 4; q++)
        if (((CUR >> (4 * k + q)) & 1u) && s2_level<NEW>(q) != 0) return false;
    return true;
}

constexpr uint32_t kSelBase2 = 0x0c0c0c00u; // v_perm_b32 selector: bytes 1-3 zero, byte 0 <- table[borrows]

// ---- the packed compare of an interior second (EmgpuPlan::d_poffpk) ------------------------------------------------------
// One draw against a column's T' pairs: x_h = the half ODD of w goes to BOTH halves of a packed subtract, each against its own
// threshold; d = min(sat(x_h - T'), 2) is 0 not fired, 1 the low halfword decides, 2 fired; the pairs are added up and the two
// halves folded: the result is 2 * (thresholds fired), odd exactly when the draw needs its low halfword.  Six (NW = 3) or four
// (NW = 2: columns of at most 3 thresholds; T'3 = 0xFFFF never fires) thresholds in 3 NW + 1 instructions, no carry, no VCC,
// no wait states (the carry chain: 3 per threshold plus a min per threshold for the tie).
template <bool ODD, int NW>
__device__ __forceinline__ uint32_t pk_fired2(uint32_t w, uint32_t t01, uint32_t t23, uint32_t t45) {
    uint32_t d0, d1, d2 = 0u, acc;
    if (ODD) {
        asm("v_pk_sub_u16 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1] clamp" : "=v"(d0) : "v"(w), "v"(t01));
        asm("v_pk_sub_u16 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1] clamp" : "=v"(d1) : "v"(w), "v"(t23));
        if (NW == 3) asm("v_pk_sub_u16 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1] clamp" : "=v"(d2) : "v"(w), "v"(t45));
    } else {
        asm("v_pk_sub_u16 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1] clamp" : "=v"(d0) : "v"(w), "v"(t01));
        asm("v_pk_sub_u16 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1] clamp" : "=v"(d1) : "v"(w), "v"(t23));
        if (NW == 3) asm("v_pk_sub_u16 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1] clamp" : "=v"(d2) : "v"(w), "v"(t45));
    }
    asm("v_pk_min_u16 %0, %0, 2 op_sel_hi:[1,0]" : "+v"(d0));
    asm("v_pk_min_u16 %0, %0, 2 op_sel_hi:[1,0]" : "+v"(d1));
    asm("v_pk_add_u16 %0, %1, %2" : "=v"(acc) : "v"(d0), "v"(d1));
    if (NW == 3) {
        asm("v_pk_min_u16 %0, %0, 2 op_sel_hi:[1,0]" : "+v"(d2));
        asm("v_pk_add_u16 %0, %0, %1" : "+v"(acc) : "v"(d2));
    }
    uint32_t s;
    asm("v_add_u32_sdwa %0, %1, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:WORD_1" : "=v"(s) : "v"(acc));
    return s;
}
// The same decision for a column of at most 3 thresholds in its PLAIN form {H0, H1, H2, map} (EmgpuPlan::d_poffpk): a_t = H_t - x_h with plain
// subtracts; fired <=> a_t < 0, tie <=> a_t == 0 (x_h = 0 against H = 0 included).  Returns the bin's bit offset in the map (7 * fired);
// tie receives min(a_t) as unsigned: 0 exactly on a tie.
template <bool ODD>
__device__ __forceinline__ uint32_t plain_fired7(uint32_t w, uint32_t h0, uint32_t h1, uint32_t h2, uint32_t &tie) {
    const uint32_t xh = ODD ? (w >> 16) : (w & 0xFFFFu);
    const uint32_t a0 = h0 - xh, a1 = h1 - xh, a2 = h2 - xh;
    uint32_t off;
    asm("v_add3_u32 %0, %1, %2, %3" : "=v"(off) : "v"(a0 >> 29), "v"(a1 >> 29), "v"(a2 >> 29));
    asm("v_min3_u32 %0, %1, %2, %3" : "=v"(tie) : "v"(a0), "v"(a1), "v"(a2));
    return off;
}
// s | (the half ODD of z): z carries a 1 in the halves whose x_h is 0 (a tie with any threshold whose high half is 0)
template <bool ODD>
__device__ __forceinline__ uint32_t or_half(uint32_t s, uint32_t z) {
    uint32_t r;
    if (ODD) asm("v_or_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1" : "=v"(r) : "v"(s), "v"(z));
    else asm("v_or_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_0" : "=v"(r) : "v"(s), "v"(z));
    return r;
}
// bin * stride + acc, everything in vector registers (no scalar operand: no wait states to respect)
__device__ __forceinline__ uint32_t mad24v(uint32_t bin, uint32_t stride, uint32_t acc) {
    uint32_t r;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(r) : "v"(bin), "v"(stride), "v"(acc));
    return r;
}

// The rare exact redo of one draw, out of line so that the 32 copies of the hot per-second body stay small:
// the secondary block is generated and the compare repeated on the full 32-bit draw (select_random.m:19-20).
__device__ __attribute__((noinline)) uint32_t exact_borrows(uint32_t c0, uint32_t c1, uint32_t attempt, uint32_t k0, uint32_t k1,
                                                            uint32_t hi_word, uint32_t tvar, uint32_t g8, uint32_t j,
                                                            uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3, uint32_t t4, uint32_t t5) {
    const Rng rng{c0, c1, attempt, k0, k1};
    const uint4 tl = rng.block(EMGPU_SEC_TRANS_LO, tvar, g8);
    const uint32_t q = j >> 1;
    const uint32_t wl = q == 0 ? tl.x : (q == 1 ? tl.y : (q == 2 ? tl.z : tl.w));
    const uint32_t hi = (j & 1u) ? (hi_word & 0xFFFF0000u) : (hi_word << 16), lo = (j & 1u) ? (wl >> 16) : (wl & 0xFFFFu);
    const uint32_t x = clamp32(hi | lo);
    return (x < t0 ? 1u : 0u) + (x < t1 ? 1u : 0u) + (x < t2 ? 1u : 0u) + (x < t3 ? 1u : 0u) + (x < t4 ? 1u : 0u) + (x < t5 ? 1u : 0u);
}
__device__ __attribute__((noinline)) uint32_t exact_hit(uint32_t c0, uint32_t c1, uint32_t attempt, uint32_t k0, uint32_t k1,
                                                        uint32_t hi_word, uint32_t ivar, uint32_t g8, uint32_t j, uint32_t R) {
    const Rng rng{c0, c1, attempt, k0, k1};
    const uint4 rl = rng.block(EMGPU_SEC_RES_LO, ivar, g8);
    const uint32_t q = j >> 1;
    const uint32_t wl = q == 0 ? rl.x : (q == 1 ? rl.y : (q == 2 ? rl.z : rl.w));
    const uint32_t hi = (j & 1u) ? (hi_word & 0xFFFF0000u) : (hi_word << 16), lo = (j & 1u) ? (wl >> 16) : (wl & 0xFFFFu);
    return clamp32(hi | lo) < R ? 1u : 0u;                                                  // resample_events.m:24
}

// WMODE: 4 / 8 = every variable's columns are 4 / 8 words wide, 0 = decided per variable at run time, 16 + m = variable k is 4 words wide
// iff bit k of m is set (s2_w4).  A width left to run time is a wave-uniform branch per draw with both forms of the draw behind it.
// REG ("regular"): exactly ND dynamic variables, all with a resample rate > 0.  The specialised
// instances drop the wave-uniform tests and the code behind them (cor_v1: 25.2 -> 20.8 ms).
// CUR / NEW: which dynamic variables are parents of which (t+1) node (bit 4k+q; step_parent_masks): an instance built for a
// model's masks multiplies only the strides that exist (cor_v1: 6 of 22) and fetches the columns of a dependency level together.
// FRZ: the FAST branch of dbn_sample.m:95-166 on this kernel -- the parent configuration of every transition is frozen at the
// initial state (the column of a variable never changes along a trajectory).  For the fast-branch models k_uncor_fast does not
// take (four dynamic variables: littoral_cor_v1); the per-second gathers then hit the same line every time.
// EV: the event list as well (emgpu_events.h): what UncorEncounterModel.sample / dbn_hierarchical_sample return for these models.
template <int WMODE>
__device__ __forceinline__ bool s2_w4(const EmgpuPlan &P, int k) {
    return WMODE == 4 || (WMODE >= 16 ? (((WMODE - 16) >> k) & 1) != 0 : (WMODE == 0 && P.d_pw[k] == 4));
}



// EMGPU_DEBUG_EXTRA_LDS: bytes of unused dynamic LDS per workgroup (tools/occupancy_probe.sh: what does a kernel lose with one wave less?)
inline size_t step2_extra_lds() {
    static const int extra = getenv("EMGPU_DEBUG_EXTRA_LDS") ? atoi(getenv("EMGPU_DEBUG_EXTRA_LDS")) : 0;
    return (size_t)extra;
}

// The dense 16-variable instances take a fourth wave: self-contained requests (coop_dedisc_sc: LDS rows of 36 words instead of 44, four
// workgroups per CU) and the initial network through the kernel-argument segment (155 -> <= 128 registers).  Same box, tools/ab_bench.sh:
// cor_v1 `[cor] w4` 11.42 -> 10.98 ms, cor_v2p1_like `[cor] w8` 14.72 -> 14.48, littoral_cor_v1 `[frozen] w4` 11.02 -> 10.65, balloon_v1 /
// weatherballoon_v1 on the run-time-width instance 7.29 -> 6.13 / 7.48 -> 6.49.  (With the owner's bin looked up in registers -- a select
// over the variables -- instead of in its own, not yet used, result slots, only the first and the last of these gained.)
constexpr bool step2_sc_form(int NI, int ND, int WMODE, bool FRZ, int EV) {
    return ND == 4 && NI == 16 && EV == 0;
}

// waves per SIMD an instance is built for
constexpr int step2_waves(int NI, int ND, int WMODE, bool FRZ, int EV) {
    return ((ND == 4 && !step2_sc_form(NI, ND, WMODE, FRZ, EV)) || EV == 1) ? 3 : 4;
}

// EV: 0 the dense trace; 1 the event list as well (result slots + a row loop per lane, emgpu_events.h); 2 the list ALONE, its rows built
// by the wave ("ROWS BY THE WAVE": no result slots, no fill)
// The body is text (emgpu_kernels_step2_body.h): the +start instances of emgpu_kernels_step2_ps.hip are the same body with PS = true and
// one more argument.
template <int NI, int ND, int WMODE, bool REG, uint32_t CUR, uint32_t NEW, bool FRZ = false, int EV = 0>
__global__ void __launch_bounds__(256, step2_waves(NI, ND, WMODE, FRZ, EV)) k_dbn_step2(const EmgpuPlan P, const EmgpuRun A, const Step2Args F) {
    constexpr bool PS = false;
    const EmgpuPresets *const Q = nullptr;
#include "emgpu_kernels_step2_body.h"
}

// every parent / the full chain of dependencies: the instance any model can run on
constexpr uint32_t kCurAll3 = 0x0777u, kNewAll3 = 0x0310u, kCurAll4 = 0xFFFFu, kNewAll4 = 0x7310u;

// one instance, with or without the event list (c: the call's DbnChoice)
#define EMGPU_S2_LAUNCH(NI_, ND_, W_, REG_, C_, N_, FRZ_)                                                                      \
    do {                                                                                                                       \
        if (c.ev == 2) hipLaunchKernelGGL((k_dbn_step2<NI_, ND_, W_, REG_, C_, N_, FRZ_, 2>), g, b, step2_extra_lds(), s, P, A, F); \
        else if (c.ev == 1) hipLaunchKernelGGL((k_dbn_step2<NI_, ND_, W_, REG_, C_, N_, FRZ_, 1>), g, b, step2_extra_lds(), s, P, A, F); \
        else hipLaunchKernelGGL((k_dbn_step2<NI_, ND_, W_, REG_, C_, N_, FRZ_, 0>), g, b, step2_extra_lds(), s, P, A, F);                        \
    } while (0)


// the per-variable arguments of a plan (the call's step2_plan)
Step2Args step2_args_of(const EmgpuPlan &P);

// entries of EMGPU_S2_CASES_ND4: DbnChoice::mask_case counts on through EMGPU_S2_CASES_ND3 from here
#define EMGPU_S2_CASE(NI_, ND_, W_, C_, N_, TAG_) +1
constexpr int kStep2CasesNd4 = 0 EMGPU_S2_CASES_ND4;
#undef EMGPU_S2_CASE

// the instances built for the 3-variable families (emgpu_kernels_step2b.hip) and the +start instances (emgpu_kernels_step2_ps.hip)
hipError_t launch_masked3(const EmgpuPlan &P, const EmgpuRun &A, const Step2Args &F, const DbnChoice &c, hipStream_t s);
hipError_t launch_dbn_step2_start(const EmgpuPlan &P, const EmgpuRun &A, const Step2Args &F, const DbnChoice &c, const EmgpuPresets *Q, hipStream_t s);

} // namespace emgpu
