// emgpu_device_math.h -- the hand-written trigonometry of the track kernels that is not in emgpu_device.h: k_terminal_propagate's
// t_k / t_sincosd, k_terminal_geo's f_sincosd and k_uncor_track's ut_sincos / ut_rcp / ut_atan / ut_asin_small.  They live here, and not
// in the one kernel file that uses each, so that emgpu_kernels_mathprobe.hip (emgpu_debug_device_math) evaluates the very functions the
// product kernels call.  Every figure below is measured on an MI355X against long-double values of the exact argument
// (tests/test_gpu_device_math.py): "units" are absolute errors in units of 2^-53, "ulp" is relative to the exact result.
#pragma once
#include <hip/hip_runtime.h>

#include "emgpu_device.h"

namespace emgpu {

// A constant held in a SCALAR register pair at its use: the f64 constants of the step loop are loop invariants, and left to the compiler
// they are materialised once and then occupy ~60 vector registers through the whole loop of a kernel that is short of them.
__device__ __forceinline__ double t_k(double c) { asm volatile("" : "+s"(c)); return c; }
// cosd / sind: MATLAB's reduction in degrees (n = round(x/90), x - 90 n in [-45, 45], quadrant mod(n, 4)) + the Horner sums of
// sincos_small (emgpu_device.h: same coefficients, same order of operations => the same bits), coefficients as scalar operands.
// Domain, accuracy and what happens outside: sincosd_small's (emgpu_device.h); equal to it bit for bit on every argument tested.
__device__ __forceinline__ void t_sincosd(double deg, double &s, double &c) {
    const double n = round(deg * t_k(1.0 / 90.0));
    const double x = t_k(3.14159265358979323846 / 180.0) * (deg - n * 90.0);
    const int m = (int)((long long)n & 3ll);
    const double z = x * x;
    double ps = t_k(-1.0 / 121645100408832000.0);
    ps = fma(ps, z, t_k(1.0 / 355687428096000.0));
    ps = fma(ps, z, t_k(-1.0 / 1307674368000.0));
    ps = fma(ps, z, t_k(1.0 / 6227020800.0));
    ps = fma(ps, z, t_k(-1.0 / 39916800.0));
    ps = fma(ps, z, t_k(1.0 / 362880.0));
    ps = fma(ps, z, t_k(-1.0 / 5040.0));
    ps = fma(ps, z, t_k(1.0 / 120.0));
    ps = fma(ps, z, t_k(-1.0 / 6.0));
    const double sx = fma(x * z, ps, x);
    double pc = t_k(-1.0 / 6402373705728000.0);
    pc = fma(pc, z, t_k(1.0 / 20922789888000.0));
    pc = fma(pc, z, t_k(-1.0 / 87178291200.0));
    pc = fma(pc, z, t_k(1.0 / 479001600.0));
    pc = fma(pc, z, t_k(-1.0 / 3628800.0));
    pc = fma(pc, z, t_k(1.0 / 40320.0));
    pc = fma(pc, z, t_k(-1.0 / 720.0));
    pc = fma(pc, z, t_k(1.0 / 24.0));
    const double cx = (1.0 - 0.5 * z) + (z * z) * pc;
    s = (m == 0) ? sx : ((m == 1) ? cx : ((m == 2) ? -sx : -cx));
    c = (m == 0) ? cx : ((m == 1) ? -sx : ((m == 2) ? -cx : sx));
}

// MATLAB's reduction in degrees (see t_sincosd) around the library's sin / cos, with the oracle's quotient deg / 90 (sincosd_small and
// t_sincosd multiply by 1/90: the two quotients round to different sides of a tie for some doubles next to a k * 90 + 45, and then reduce
// the same angle to +45 and to -45 degrees of neighbouring quadrants -- both are the same exact value).  Domain |deg| < 2^53: exact 0 and +-1 at every
// multiple of 90, elsewhere within 2 units of 2^-53 (absolute; measured worst 1.20).  NaN and +-inf give NaN in both results; |deg| >= 2^53 as sincosd_small.
__device__ __forceinline__ void f_sincosd(double deg, double &s, double &c) {
    const double n = round(deg / 90.0);
    const double x = (3.14159265358979323846 / 180.0) * (deg - n * 90.0);
    const int m = (int)((long long)n & 3ll);
    const double sx = sin(x), cx = cos(x);
    s = (m == 0) ? sx : ((m == 1) ? cx : ((m == 2) ? -sx : -cx));
    c = (m == 0) ? cx : ((m == 1) ? -sx : ((m == 2) ? -cx : sx));
}

// sin and cos of an angle of moderate size (|x| < 1e5; pitch, bank, heading in radians): k = rint(x * 2/pi), the remainder
// x - k * pi/2 taken in two pieces of pi/2 (the first has 33 significant bits: k * hi is exact), Horner sums on the remainder
// (sincos_small, emgpu_device.h), the quadrant from k.  About 45 instructions for both
// where the library's sin() + cos() take 180; results within 2 units of the exact values (measured worst 1.53) -- ABSOLUTE, in units of 2^-53:
// near a multiple of pi/2 the small component keeps the reduction's absolute error, up to 4e9 ulps of itself (the
// tracks are compared at 1e-9).  sin(+-0) = +-0.  Domain: every x.  |x| >= 1e5 goes to the library's sin() and cos(); NaN and +-inf give NaN in both.
template <bool SK = false>   // SK: coefficients as scalar operands (sk64): for the variant that evaluates these once per recorded row only
__device__ __forceinline__ void ut_sincos(double x, double &s, double &c) {
    if (!(fabs(x) < 1.0e5)) { s = sin(x); c = cos(x); return; }
    const double k = rint(x * 0.63661977236758134308);                 // 2/pi
    double r = fma(-k, 1.57079632673412561417, x);                     // pi/2, first 33 bits
    r = fma(-k, 6.07710050650619224932e-11, r);                        // pi/2 - the above
    double sr, cr;
    sincos_small_core<SK>(r, sr, cr);   // (scalar-operand coefficients in the literal step -- three waves instead of two -- were measured: +4 %, it is issue-bound)
    const int q = (int)((long long)k & 3ll);
    s = (q == 0) ? sr : ((q == 1) ? cr : ((q == 2) ? -sr : -cr));
    c = (q == 0) ? cr : ((q == 1) ? -sr : ((q == 2) ? -cr : sr));
    s = (x == 0.0) ? x : s;   // sin(-0.0) = -0.0: the remainder of -0.0 is +0.0 (fma(+0, hi, -0))
}

// 1 / d to one ulp (measured: correctly rounded on every one of 135 164 arguments): v_rcp_f64 and two Newton steps (5 instructions; the IEEE-exact division the compiler emits for `/`
// takes ~35).  The dynamics divide six times per 0.1 s step as written; here they share ONE reciprocal, 1 / (v cos(phi)).
// Domain: finite normal d whose reciprocal is normal (2^-1022 <= |d| <= 2^1022).  Outside it (measured): +-0, +-inf and NaN
// give NaN (fma(-0, inf, 1)); a subnormal d gives NaN where 1 / d overflows and an inexact quotient otherwise; |d| > 2^1022 gave the
// correctly rounded subnormal on every argument tried.
__device__ __forceinline__ double ut_rcp(double d) {
    double x = __builtin_amdgcn_rcp(d);
    double e = fma(-d, x, 1.0);
    x = fma(x, e, x);
    e = fma(-d, x, 1.0);
    return fma(x, e, x);
}
// atan on fdlibm's breakpoints (s_atan.c: 7/16, 11/16, 19/16, 39/16) and kernel polynomial, the reduced argument's division through
// ut_rcp, selects instead of branches; within 2 ulp of the exact value (measured worst 1.06; tests/test_gpu_device_math.py).  Domain: finite x.
// Outside it and at its edge: NaN gives NaN; +-inf gives NaN, not +-pi/2 (ut_rcp(inf) = 0 and fma(-inf, 0, 1) is NaN -- no infinite
// argument reaches it from k_uncor_track); atan(-0.0) is +0.0 (the sign is restored by `x < 0`).
template <bool SK = false>
__device__ __forceinline__ double ut_atan(double x) {
    auto K = [](double v) { return SK ? sk64(v) : v; };
    const double ax = fabs(x);
    double num = ax, den = 1.0, c = 0.0;
    if (ax >= 0.4375) { num = fma(2.0, ax, -1.0); den = 2.0 + ax; c = 4.63647609000806093515e-01; }      // atan(0.5)
    if (ax >= 0.6875) { num = ax - 1.0; den = ax + 1.0; c = 7.85398163397448278999e-01; }                 // atan(1)
    if (ax >= 1.1875) { num = ax - 1.5; den = fma(1.5, ax, 1.0); c = 9.82793723247329054082e-01; }        // atan(1.5)
    if (ax >= 2.4375) { num = -1.0; den = ax; c = 1.57079632679489655800e+00; }                           // atan(inf)
    const double t = num * ut_rcp(den);
    const double z = t * t, w = z * z;
    double s1 = fma(w, K(1.62858201153657823623e-02), K(4.97687799461593236017e-02));
    s1 = fma(w, s1, K(6.66107313738753120669e-02));
    s1 = fma(w, s1, K(9.09088713343650656196e-02));
    s1 = fma(w, s1, K(1.42857142725034663711e-01));
    s1 = fma(w, s1, K(3.33333333333329318027e-01));
    s1 = z * s1;
    double s2 = fma(w, K(-3.65315727442169155270e-02), K(-5.83357013379057348645e-02));
    s2 = fma(w, s2, K(-7.69187620504482999495e-02));
    s2 = fma(w, s2, K(-1.11111104054623557880e-01));
    s2 = fma(w, s2, K(-1.99999999998764832476e-01));
    s2 = w * s2;
    const double r = c + (t - t * (s1 + s2));
    return x < 0 ? -r : r;
}
// asin for |x| < 0.5 (a climb angle below 30 degrees): fdlibm's rational kernel (e_asin.c), its division through ut_rcp; within
// 2 ulp of the exact value (measured worst 0.61), asin(+-0) = +-0.  Domain |x| < 0.5, which both call sites guard (`fabs(..) < 0.5 ? ut_asin_small :
// asin`); outside it the rational kernel simply loses accuracy (finite for finite x), NaN gives NaN.
template <bool SK = false>
__device__ __forceinline__ double ut_asin_small(double x) {
    auto K = [](double v) { return SK ? sk64(v) : v; };
    const double t = x * x;
    double p = fma(t, K(3.47933107596021167570e-05), K(7.91534994289814532176e-04));
    p = fma(t, p, K(-4.00555345006794114027e-02));
    p = fma(t, p, K(2.01212532134862925881e-01));
    p = fma(t, p, K(-3.25565818622400915405e-01));
    p = fma(t, p, K(1.66666666666666657415e-01));
    p = t * p;
    double q = fma(t, K(7.70381505559019352791e-02), K(-6.88283971605453293030e-01));
    q = fma(t, q, K(2.02094576023350569471e+00));
    q = fma(t, q, K(-2.40339491173441421878e+00));
    q = fma(t, q, K(1.0));
    return fma(x, p * ut_rcp(q), x);
}

} // namespace emgpu
