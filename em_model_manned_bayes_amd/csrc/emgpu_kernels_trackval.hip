// emgpu_kernels_trackval.hip -- k_track_values<PLANAR | ROWS, float | double>: device-resident 1 Hz tracks into the values of a trace
// (vertical rate, acceleration, turn rate per second; altitude, speed and the three rates of second 0 as the initial rows), one lane per
// track, sequential in time, 256-lane workgroups.  The definition is in emgpu_trackval.h; the kernel is the inverse of k_sample2track.
//
// A lane walks its track point by point and keeps the previous point, the previous displacement's speed, heading and climb in registers:
// point p closes displacement p - 1 and, from p = 2 on, second p - 2 of the values.  Four seconds of a variable are gathered in registers
// and leave as one 16-byte store (two for doubles), coalesced along the track index, into dyn_val [ceil(T/4)][nd][ld][4]; the elements of
// the last group behind T are written 0.  Only the rows named in the argument block are written.
//   PLANAR  xyz [P][3][n], what emgpu_sample2track_device writes: three coalesced 8-byte loads per lane and point.
//   ROWS    xyz [n][P][3], what a file holds: a lane's own row is 24 * P bytes away from its neighbour's, so the workgroup stages tiles of
//           (256 tracks x EMGPU_TV_TILE = 8 points) through LDS: consecutive lanes load consecutive doubles of a track's 192-byte segment
//           (2.7 segments per wave-load), and each lane then reads its own track's points with 8-byte LDS reads.  A track's tile row is
//           padded to 25 doubles (50 dwords): 32 lanes' ds_read_b64 then fall on 64 distinct banks.  256 * 25 * 8 = 51 200 bytes per
//           workgroup, so three workgroups (12 waves) share a CU's 160 KiB.
// Both layouts run the same arithmetic in the same order: their outputs are bit-equal.  Plain vector stores only; no atomics.
// Compiler's figures (hipcc -O3, gfx950) are in DESIGN.md section 23.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "emgpu_trackval.h"

namespace {
constexpr int kBlock = EMGPU_TV_BLOCK, kTile = EMGPU_TV_TILE, kStride = EMGPU_TV_STRIDE, kSeg = 3 * EMGPU_TV_TILE;
constexpr double kDegPerRad = 57.29577951308232;

__device__ __forceinline__ void store4(float *p, const double q[4]) {
    *reinterpret_cast<float4 *>(p) = make_float4((float)q[0], (float)q[1], (float)q[2], (float)q[3]);
}
__device__ __forceinline__ void store4(double *p, const double q[4]) {
    *reinterpret_cast<double2 *>(p) = make_double2(q[0], q[1]);
    *reinterpret_cast<double2 *>(p + 2) = make_double2(q[2], q[3]);
}

template <bool ROWS, typename V>
__global__ __launch_bounds__(kBlock) void k_track_values(const EmgpuTrackValuesRun A) {
#pragma clang fp contract(off)
    __shared__ double tile[ROWS ? kBlock * kStride : 1];
    const int64_t i0 = (int64_t)blockIdx.x * kBlock, i = i0 + threadIdx.x;
    const bool live = i < A.n;
    if (!ROWS && !live) return;       // (ROWS: every lane of the workgroup meets the barriers; a lane without a track stores nothing)
    const size_t n = (size_t)A.n, ld = (size_t)A.ld, P = (size_t)A.P;
    const int T = A.P - 2;
    V *const iv = live ? (V *)A.init_val : nullptr;
    V *const dv = live ? (V *)A.dyn_val : nullptr;
    const int tracks = (int)std::min<int64_t>(kBlock, A.n - i0);
    double px = 0.0, py = 0.0, pz = 0.0, ps = 0.0, ph = 0.0, pdz = 0.0;   // h[-1] = 0
    double q[3][4];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int s = 0; s < 4; s++) q[k][s] = 0.0;
    auto flush = [&](int g) {       // group g of four seconds, the three variables
#pragma unroll
        for (int k = 0; k < 3; k++) {
            store4(dv + 4 * (((size_t)g * (size_t)A.nd + (size_t)A.slot[k]) * ld + (size_t)i), q[k]);
#pragma unroll
            for (int s = 0; s < 4; s++) q[k][s] = 0.0;
        }
    };
    for (int p0 = 0; p0 < A.P; p0 += kTile) {     // p0 is a multiple of 8: second p - 2 of point p = p0 + j lies in element (j + 2) % 4 of its group
        if (ROWS) {
            __syncthreads();                      // the previous tile has been read
            const int seg = 3 * std::min(kTile, A.P - p0);
            for (int e = threadIdx.x; e < kBlock * kSeg; e += kBlock) {
                const int tr = e / kSeg, j = e % kSeg;
                if (tr < tracks && j < seg) tile[tr * kStride + j] = A.xyz[((size_t)(i0 + tr) * P + (size_t)p0) * 3 + (size_t)j];
            }
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < kTile; j++) {
            const int p = p0 + j;
            if (p < A.P) {                        // (uniform)
                double x, y, z;
                if (ROWS) {
                    const double *c = tile + threadIdx.x * kStride + 3 * j;
                    x = c[0]; y = c[1]; z = c[2];
                } else {
                    const size_t o = (size_t)p * 3 * n + (size_t)i;
                    x = A.xyz[o]; y = A.xyz[o + n]; z = A.xyz[o + 2 * n];
                }
                if (p == 0) {
                    if (iv && A.row[0] >= 0) iv[(size_t)A.row[0] * ld + (size_t)i] = (V)z;
                } else {
                    const double dx = x - px, dy = y - py, dz = z - pz;
                    const double s = __builtin_sqrt(dx * dx + dy * dy);
                    const double h = s == 0.0 ? ph : atan2(dy, dx) * kDegPerRad;
                    if (p == 1) {
                        if (iv && A.row[1] >= 0) iv[(size_t)A.row[1] * ld + (size_t)i] = (V)(s / A.ur_speed);
                    } else {
                        const int el = (j + 2) & 3;
                        const double d = h - ph;
                        const double w = d - 360.0 * __builtin_floor((d + 180.0) / 360.0);
                        q[0][el] = pdz / A.ur_vertrate;
                        q[1][el] = (s - ps) / A.ur_speed;
                        q[2][el] = w / A.ur_heading;
                        if (p == 2 && iv) {
#pragma unroll
                            for (int k = 0; k < 3; k++)
                                if (A.row[2 + k] >= 0) iv[(size_t)A.row[2 + k] * ld + (size_t)i] = (V)q[k][0];
                        }
                        if (el == 3 && dv) flush((p - 2) >> 2);
                    }
                    ps = s; ph = h; pdz = dz;
                }
                px = x; py = y; pz = z;
            }
        }
    }
    if ((T & 3) && dv) flush(T >> 2);             // the last group: its elements behind T are 0
}

template <bool ROWS, typename V>
void launch(const EmgpuTrackValuesRun &A, hipStream_t s) {
    hipLaunchKernelGGL((k_track_values<ROWS, V>), dim3((unsigned)((A.n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, A);
}
} // namespace

namespace emgpu {
hipError_t launch_track_values(const EmgpuTrackValuesRun &A, bool rows, bool f64, hipStream_t s, const char **name) {
    if (name) *name = rows ? (f64 ? "k_track_values[ROWS,f64]" : "k_track_values[ROWS,f32]") : (f64 ? "k_track_values[PLANAR,f64]" : "k_track_values[PLANAR,f32]");
    if (A.n <= 0 || (!A.init_val && !A.dyn_val)) return hipSuccess;
    if (rows) { if (f64) launch<true, double>(A, s); else launch<true, float>(A, s); }
    else { if (f64) launch<false, double>(A, s); else launch<false, float>(A, s); }
    return hipGetLastError();
}
} // namespace emgpu
