// emgpu_device.h -- device-side primitives shared by every kernel: Philox4x32 (EMGPU_PHILOX_ROUNDS rounds), the uniform,
// the threshold draw and dediscretize.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/emgpu.h"
#include "emgpu_plan.h"

namespace emgpu {

// Philox4x32-R, R = EMGPU_PHILOX_ROUNDS (Salmon et al. SC'11; emgpu_plan.h).  The key is wave-uniform (the seed), so the key schedule
// lives in SGPRs / literals; each round is two v_mad_u64_u32 (32x32->64) and four XORs.
__device__ __forceinline__ uint4 philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < EMGPU_PHILOX_ROUNDS; r++) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        // three-input XOR in one v_bitop3_b32 (truth table 0x96), gfx950
        const uint32_t n0 = __builtin_amdgcn_bitop3_b32((uint32_t)(p1 >> 32), c1, k0 + (uint32_t)r * 0x9E3779B9u, 0x96);
        const uint32_t n2 = __builtin_amdgcn_bitop3_b32((uint32_t)(p0 >> 32), c3, k1 + (uint32_t)r * 0xBB67AE85u, 0x96);
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
    }
    return make_uint4(c0, c1, c2, c3);
}

// Per-trajectory RNG handle: counter words 0..2 are fixed per (trajectory, attempt).
struct Rng {
    uint32_t c0, c1, attempt, k0, k1;
    __device__ __forceinline__ uint4 block(uint32_t section, uint32_t a, uint32_t blk) const {
        return philox4x32(c0, c1, attempt, (section << 28) | (a << 20) | blk, k0, k1);
    }
};

// word w of a block; w is compile-time or wave-uniform at every call site
__device__ __forceinline__ uint32_t word_of(const uint4 &v, int w) { return w == 0 ? v.x : (w == 1 ? v.y : (w == 2 ? v.z : v.w)); }

// halfword j (0..7) of a block, already shifted into the HIGH half of a 32-bit word
__device__ __forceinline__ uint32_t half_hi(const uint4 &v, int j) {
    const uint32_t w = word_of(v, j >> 1);
    return (j & 1) ? (w & 0xFFFF0000u) : (w << 16);
}
// halfword j (0..7) of a block in the LOW half
__device__ __forceinline__ uint32_t half_lo(const uint4 &v, int j) {
    const uint32_t w = word_of(v, j >> 1);
    return (j & 1) ? (w >> 16) : (w & 0xFFFFu);
}
// split slot: the full 32-bit draw from its primary (hi) and secondary (lo) blocks
__device__ __forceinline__ uint32_t split_draw(const uint4 &hi, const uint4 &lo, int j) { return half_hi(hi, j) | half_lo(lo, j); }

// x' of uniform32
__device__ __forceinline__ uint32_t clamp32(uint32_t x) { return x < 0xFFFFFFFEu ? x : 0xFFFFFFFEu; }

// u = (x' + 0.5) * 2^-32, exact in f64
__device__ __forceinline__ double uniform32(uint32_t x) { return ((double)clamp32(x) + 0.5) * (1.0 / 4294967296.0); }

// select_random.m:17-20 on precompiled thresholds: 0-based bin = #{k < r-1 : x' >= X[k]}
__device__ __forceinline__ int draw_bin(const uint32_t *__restrict__ t, int r, uint32_t x) {
    const uint32_t xp = clamp32(x);
    int b = 0;
    for (int k = 0; k < r - 1; k++) b += (xp >= t[k]) ? 1 : 0;
    return b;
}

// dediscretize.m:33-39  a + (b-a)*rand, in f64 without FMA contraction (bit-exact with the oracle)
__device__ __forceinline__ double dedisc_f64(const double *__restrict__ bnd, int boff, int bin0, uint32_t x) {
#pragma clang fp contract(off)
    const double a = bnd[boff + bin0];
    const double b = bnd[boff + bin0 + 1];
    const double d = b - a;
    const double m = d * uniform32(x);
    return a + m;
}

// sin and cos of |x| <= pi/4 (a reduced angle): Taylor sums to x^19 / x^18 in Horner form on explicit fma -- truncation below
// 1e-19; measured against the exact values (tests/test_gpu_device_math.py): the sine within 2 ulp of the exact
// result (relative: s = x exactly from 2^-27 down), the cosine within 2 units of 2^-53 (absolute); measured worst 0.66 ulp and 1.23 units.  The library's sin() / cos() spend
// three times the instructions on a range reduction that such an argument never needs.  Used where outputs are compared at a tolerance
// (tracks), never on the sampling path.  Domain: |x| <= pi/4 and the ulp beyond it that a reduction's rounding leaves.  Outside it the
// truncated series loses accuracy and, from |x| ~ 1e154 on (x * x overflows), gives infinities: +-inf gives (NaN, -inf).  NaN gives NaN.
// sincos_small_core is the sum alone: its sine of -0.0 is +0.0 (x * z * ps is +0 there, and -0 + +0 = +0), which is right for the callers
// whose reduced argument is never -0.0 (sincosd_small, ut_sincos); sincos_small gives a zero sine its argument's sign: sin(+-0) = +-0.
// A constant held in a SCALAR register pair at its use.  The f64 coefficients of a loop body are loop invariants: left to the compiler they are
// materialised once, ahead of the loop, and then sit in vector registers for its whole length -- 60 of them in k_terminal_propagate, a third
// of its budget and a whole wave of occupancy.  As scalar operands (one per VALU instruction) they cost two s_mov each at the use.
__device__ __forceinline__ double sk64(double c) { asm volatile("" : "+s"(c)); return c; }
// SK: the coefficients as scalar operands (sk64)
template <bool SK = false>
__device__ __forceinline__ void sincos_small_core(double x, double &s, double &c) {
    auto K = [](double v) { return SK ? sk64(v) : v; };
    const double z = x * x;
    double ps = K(-1.0 / 121645100408832000.0);          // -1/19!
    ps = fma(ps, z, K(1.0 / 355687428096000.0));         //  1/17!
    ps = fma(ps, z, K(-1.0 / 1307674368000.0));          // -1/15!
    ps = fma(ps, z, K(1.0 / 6227020800.0));              //  1/13!
    ps = fma(ps, z, K(-1.0 / 39916800.0));               // -1/11!
    ps = fma(ps, z, K(1.0 / 362880.0));                  //  1/9!
    ps = fma(ps, z, K(-1.0 / 5040.0));                   // -1/7!
    ps = fma(ps, z, K(1.0 / 120.0));                     //  1/5!
    ps = fma(ps, z, K(-1.0 / 6.0));                      // -1/3!
    s = fma(x * z, ps, x);
    double pc = K(-1.0 / 6402373705728000.0);            // -1/18!
    pc = fma(pc, z, K(1.0 / 20922789888000.0));          //  1/16!
    pc = fma(pc, z, K(-1.0 / 87178291200.0));            // -1/14!
    pc = fma(pc, z, K(1.0 / 479001600.0));               //  1/12!
    pc = fma(pc, z, K(-1.0 / 3628800.0));                // -1/10!
    pc = fma(pc, z, K(1.0 / 40320.0));                   //  1/8!
    pc = fma(pc, z, K(-1.0 / 720.0));                    // -1/6!
    pc = fma(pc, z, K(1.0 / 24.0));                      //  1/4!
    c = (1.0 - 0.5 * z) + (z * z) * pc;
}
template <bool SK = false>
__device__ __forceinline__ void sincos_small(double x, double &s, double &c) {
    sincos_small_core<SK>(x, s, c);
    s = (s == 0.0) ? x : s;   // a zero sine is the sine of a zero (a nonzero x down to the smallest subnormal gives s = x): its sign
}
// cosd / sind with MATLAB's reduction in degrees: n = round(x/90), x - 90 n in [-45, 45], quadrant m = mod(n, 4); the quotient is
// round(deg * (1/90)), which differs from the oracle's round(deg / 90) only for doubles next to a tie k * 90 + 45, where the two remainders
// (+45 and -45 degrees of neighbouring quadrants) name the same angle.  Domain |deg| < 2^53 (deg - 90 n is exact there): exactly 0 and +-1 at
// every multiple of 90 with the signs MATLAB's reduction gives the zeros (sind(180) = -0, cosd(90) = -0; the reduced argument is never
// -0.0, sind(-0.0) = +0), elsewhere within 2 units of 2^-53 of the exact values (absolute; measured worst 1.61).  NaN and +-inf give NaN in both results.
// |deg| >= 2^53 is outside: n * 90 is no longer exact and, from 90 * 2^63 on, n is outside the integer conversion, so the results are
// not the sine and cosine of deg (measured: unrelated values in [-1, 1]); nothing traps.
__device__ __forceinline__ void sincosd_small(double deg, double &s, double &c) {
    const double n = round(deg * (1.0 / 90.0));
    const double x = (3.14159265358979323846 / 180.0) * (deg - n * 90.0);
    const int m = (int)((long long)n & 3ll);
    double sx, cx;
    sincos_small_core<false>(x, sx, cx);
    s = (m == 0) ? sx : ((m == 1) ? cx : ((m == 2) ? -sx : -cx));
    c = (m == 0) ? cx : ((m == 1) ? -sx : ((m == 2) ? -cx : sx));
}

// run-time (wave-uniform) index into a tiny register array without scratch.  Written with bit
// masks on purpose: a ?: chain over a[q] is folded by LLVM into a variable-index load, which
// forces the whole array into scratch/LDS.
__device__ __forceinline__ uint32_t pick_bits(uint32_t v, bool sel) { return v & (sel ? 0xFFFFFFFFu : 0u); }
template <int N>
__device__ __forceinline__ int pick(const int (&a)[N], int idx) {
    uint32_t r = 0u;
#pragma unroll
    for (int q = 0; q < N; q++) r |= pick_bits((uint32_t)a[q], idx == q);
    return (int)r;
}
template <int N>
__device__ __forceinline__ double pick(const double (&a)[N], int idx) {
    uint32_t lo = 0u, hi = 0u;
#pragma unroll
    for (int q = 0; q < N; q++) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(a[q]);
        lo |= pick_bits((uint32_t)b, idx == q);
        hi |= pick_bits((uint32_t)(b >> 32), idx == q);
    }
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
template <int N, typename T>
__device__ __forceinline__ void put(T (&a)[N], int idx, T v) {
#pragma unroll
    for (int q = 0; q < N; q++) a[q] = (idx == q) ? v : a[q];
}

// UncorEncounterModel.m:196, 500 * (floor(num / 500) + (mod(num, 500) > 250)), bit for bit for every num.  MATLAB's mod is the floored one:
// for num < 0 fmod's remainder r stands for r + 500, and r + 500 > 250 exactly when r > -250 (the sum is exact next to 250).  NaN and
// +-inf give themselves (fmod is NaN, the comparison false).
__device__ __forceinline__ double round500(double num) {
    const double r = fmod(num, 500.0);
    return 500.0 * (floor(num / 500.0) + ((r > 250.0 || (r < 0.0 && r > -250.0)) ? 1.0 : 0.0));
}

// The presets of one lane (bn_sample.m:44-50): sp[p] = the preset bin (1-based) of the node at position p or 0; a lane's own row of the
// start grid (entry of variable id, 0 = unset) wins over the model's start.  A preset node needs all its parents preset ('Attempt to
// preset a dependent variable', :47) and a bin inside 1..r: otherwise bit 2 of *status is raised (EMGPU_ERR_PRESET) and the preset is
// dropped.  Returns the lane's log-weight: the sum over its preset nodes of log P(preset | parents) read from `logp` (0 without a table).
template <int NI>
__device__ __forceinline__ double lane_presets(const EmgpuPlan &P, const int32_t *start_row, const double *logp, const uint32_t *lp_off, uint32_t *status, int (&sp)[NI]) {
    uint32_t mask = 0u;
    double lw = 0.0;
    uint32_t colbin[NI];
#pragma unroll
    for (int p = 0; p < NI; p++) {
        sp[p] = 0; colbin[p] = 0u;
        if (p >= P.ni) continue;
        int s = start_row ? start_row[P.i_var[p]] : 0;
        if (s == 0) s = (int)P.i_start[p];
        if (s == 0) continue;
        bool ok = s >= 1 && s <= (int)P.i_r[p];
        uint32_t col = 0u;
#pragma unroll
        for (int q = 0; q < p; q++) {
            if (P.i_stride[p][q] == 0u) continue;
            if (!((mask >> q) & 1u)) ok = false;
            col += P.i_stride[p][q] * colbin[q];
        }
        if (!ok) { atomicOr(status, 4u); continue; }
        sp[p] = s; colbin[p] = (uint32_t)(s - 1); mask |= 1u << p;
        if (logp) lw += logp[lp_off[p] + (size_t)col * (uint32_t)P.i_r[p] + (uint32_t)(s - 1)];
    }
    return lw;
}

// The presets a lane draws its initial network under, for the two init_network_ps forms: from its row of a start grid (Qp->start, row
// Qp->row[lane], or lane itself without a row list) with its log-weight stored where wanted (Qp->log_weight), or the model's own start
// (Qp null, or live = false: a lane outside the run reads no row and writes no weight).  PlanPtr: const EmgpuPlan *, or a KargPlan (below)
// whose entries stay loads from the kernel-argument segment.
template <int NI, typename PlanPtr>
__device__ __forceinline__ void lane_start(PlanPtr P, const EmgpuRun &A, const EmgpuPresets *Qp, int64_t lane, bool live, int (&sp)[NI]) {
    if (Qp && live) {
        const EmgpuPresets &Q = *Qp;
        const int64_t row = Q.row ? Q.row[lane] : lane;
        const double lw = lane_presets<NI>(*(const EmgpuPlan *)P, Q.start ? Q.start + (size_t)row * (size_t)P->ni : nullptr, Q.log_weight ? Q.logp : nullptr, Q.lp_off, A.status, sp);
        if (Q.log_weight) Q.log_weight[row] = lw;
    } else {
#pragma unroll
        for (int p = 0; p < NI; p++) sp[p] = p < P->ni ? (int)P->i_start[p] : 0;
    }
}

// What every DBN kernel stores of lane i after the draw: bit 1 of *status when no attempt was accepted, the attempts used, and the initial
// state by variable id.  A macro over the kernel's own P, A, NI, bin[] and val[], not a function: k_dbn_step and k_dbn_step2 take the plan
// and the run by value, and handing them on by reference changed the code of their instances (HISTORY.md section 32).
#define EMGPU_STORE_INIT(i, attempts_used)                                                                             \
    {                                                                                                                  \
        if (attempts_used < 0) atomicOr(A.status, 1u);                                                                 \
        if (A.attempts) A.attempts[i] = attempts_used;                                                                 \
        _Pragma("unroll") for (int p = 0; p < NI; p++) {                                                               \
            if (p < P.ni) {                                                                                            \
                if (A.init_bin) A.init_bin[(size_t)P.i_var[p] * A.ld + i] = (uint8_t)(bin[p] + 1);                     \
                if (A.init_val) A.init_val[(size_t)P.i_var[p] * A.ld + i] = (float)val[p];                             \
            }                                                                                                          \
        }                                                                                                              \
    }

// Initial network + dediscretize + rejection loop, shared by every DBN kernel: four forms of one body (emgpu_init_body.h), by how the plan
// is read and where a node's preset comes from.  bin[]: 0-based bins by topological position; val[]: dediscretised f64.  Each returns the
// number of attempts used (>= 1) or -1 when max_attempts was reached, and leaves rng.attempt at the accepted attempt.
#define EMGPU_INIT_P(f) P.f
#define EMGPU_INIT_FRESH_PLAN
// The plan by reference, the model's own presets.
template <int NI>
__device__ __forceinline__ int32_t init_network(const EmgpuPlan &P, const EmgpuRun &A, Rng &rng, int (&bin)[NI], double (&val)[NI]) {
    int32_t attempts_used = -1;
    const bool no_dedisc = (A.flags & EMGPU_FLAG_NO_DEDISC) != 0;
#define EMGPU_INIT_PRESET(p) const auto &preset = P.i_start[p];
#include "emgpu_init_body.h"
#undef EMGPU_INIT_PRESET
    return attempts_used;
}

// The same with the lane's presets possibly coming from a start grid and its log-weight wanted (lane_start): k_dbn_generic and the +start
// instances of the fast kernel.  live = false: a lane outside the run (the fast kernel keeps those alive as workers of their wave).
template <int NI>
__device__ __forceinline__ int32_t init_network_ps(const EmgpuPlan &P, const EmgpuRun &A, const EmgpuPresets *Qp, Rng &rng, int (&bin)[NI], double (&val)[NI], int64_t lane,
                                                   bool live = true) {
    int32_t attempts_used = -1;
    const bool no_dedisc = (A.flags & EMGPU_FLAG_NO_DEDISC) != 0;
    int sp[NI];
    lane_start<NI>(&P, A, Qp, lane, live, sp);
#define EMGPU_INIT_PRESET(p) const int preset = sp[p];
#include "emgpu_init_body.h"
#undef EMGPU_INIT_PRESET
    return attempts_used;
}
#undef EMGPU_INIT_P
#undef EMGPU_INIT_FRESH_PLAN

// init_network for the dense 16-variable instances of k_dbn_step2 (and the -DEMGPU_FAST_INIT_KARG measuring variant of k_uncor_fast),
// reading the plan through the kernel-argument segment with the pointer laundered once per attempt.  The initial network of 16 variables
// uses 120 parent strides + five small tables: as loop invariants of the attempt loop they are loaded ahead of it, outlive the scalar
// register file (657 v_writelane ahead of the loop, 708 v_readlane inside it) and keep 30 vector registers as spill space for the whole
// kernel: 155 registers, three waves per SIMD.  Loaded where they are used they are scalar loads and nothing else: <= 128 registers, which
// (with the 36-word LDS rows of coop_dedisc_sc) is a fourth wave.
typedef const __attribute__((address_space(4))) EmgpuPlan *KargPlan;
#define EMGPU_INIT_P(f) P->f
#define EMGPU_INIT_FRESH_PLAN KargPlan P = Pk; asm volatile("" : "+s"(P));   // (the plan's entries are loaded where this attempt uses them)
template <int NI>
__device__ __forceinline__ int32_t init_network_karg(KargPlan Pk, const EmgpuRun &A, Rng &rng, int (&bin)[NI], double (&val)[NI]) {
    int32_t attempts_used = -1;
    const bool no_dedisc = (A.flags & EMGPU_FLAG_NO_DEDISC) != 0;
#define EMGPU_INIT_PRESET(p) const auto &preset = P->i_start[p];
#include "emgpu_init_body.h"
#undef EMGPU_INIT_PRESET
    return attempts_used;
}

// init_network_ps the same way, for the +start twin of the dense 16-variable instances (emgpu_kernels_step2_ps.hip): the lane's presets
// are worked out once, through a pointer laundered of its own (lane_presets' 120 strides are not kept for the attempt loop), and live in
// vector registers across the attempts; everything else of the plan is loaded where an attempt uses it.
template <int NI>
__device__ __forceinline__ int32_t init_network_ps_karg(KargPlan Pk, const EmgpuRun &A, const EmgpuPresets *Qp, Rng &rng, int (&bin)[NI], double (&val)[NI], int64_t lane,
                                                        bool live) {
    int32_t attempts_used = -1;
    const bool no_dedisc = (A.flags & EMGPU_FLAG_NO_DEDISC) != 0;
    int sp[NI];
    {
        EMGPU_INIT_FRESH_PLAN
        lane_start<NI>(P, A, Qp, lane, live, sp);
    }
#define EMGPU_INIT_PRESET(p) const int &preset = sp[p];
#include "emgpu_init_body.h"
#undef EMGPU_INIT_PRESET
    return attempts_used;
}
#undef EMGPU_INIT_P
#undef EMGPU_INIT_FRESH_PLAN

} // namespace emgpu
