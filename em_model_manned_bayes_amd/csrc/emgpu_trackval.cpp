// emgpu_trackval.cpp -- emgpu_track_values_device / emgpu_track_values_host: 1 Hz tracks into the values of a trace (k_track_values,
// emgpu_kernels_trackval.hip; the definition is in emgpu_trackval.h and DESIGN.md).  The host entry point takes tracks as a file holds them
// ([n][points][3]): a chunk of tracks is one contiguous piece of the caller's array, so it is uploaded as it lies and the ROWS kernel reads
// it; nothing is transposed on the host.  It works chunk by chunk (emgpu_tracechunk.hpp).
#include <cmath>
#include <cstring>

#include "emgpu_plan.h"
#include "emgpu_tracechunk.hpp"
#include "emgpu_trackval.h"

using namespace emgpu_detail;

namespace {
// what can be said without a device: EMGPU_OK, or the error (recorded)
int check_args(const emgpu_track_values_params *p, const double *xyz, const void *init_val, const void *dyn_val) {
    if (!p || !xyz) return fail(EMGPU_ERR_ARG, "null argument");
    if (!init_val && !dyn_val) return fail(EMGPU_ERR_ARG, "null init_val and dyn_val: nothing to write");
    if (p->points < 3 || p->points - 2 > 65535) return fail(EMGPU_ERR_ARG, "points outside 3..65537 (1..65535 seconds of values)");
    if (p->n < 0) return fail(EMGPU_ERR_ARG, "n < 0");
    const int64_t ld = p->ld ? p->ld : p->n;
    if (ld < 0 || p->col_offset < 0 || p->col_offset + p->n > ld) return fail(EMGPU_ERR_ARG, "col_offset + n exceeds ld");
    if (p->value_type != EMGPU_VALUE_F32 && p->value_type != EMGPU_VALUE_F64) return fail(EMGPU_ERR_ARG, "unknown value_type");
    if (p->layout != EMGPU_TRACKS_PLANAR && p->layout != EMGPU_TRACKS_ROWS) return fail(EMGPU_ERR_ARG, "unknown layout");
    for (const double ur : {p->ur_speed, p->ur_vertrate, p->ur_heading})
        if (!std::isfinite(ur) || ur == 0.0) return fail(EMGPU_ERR_ARG, "a unit ratio is 0 or not finite");
    if (init_val) {
        if (p->n_initial < 1 || p->n_initial > EMGPU_MAX_NI) return fail(EMGPU_ERR_ARG, "n_initial outside 1..EMGPU_MAX_NI");
        const int32_t row[5] = {p->row_alt, p->row_speed, p->row_vertrate, p->row_acc, p->row_turnrate};
        for (int a = 0; a < 5; a++) {
            if (row[a] < -1 || row[a] >= p->n_initial) return fail(EMGPU_ERR_ARG, "an initial row outside -1..n_initial-1");
            for (int b = 0; b < a; b++)
                if (row[a] >= 0 && row[a] == row[b]) return fail(EMGPU_ERR_ARG, "two values name the same initial row");
        }
    }
    if (dyn_val) {
        if (p->nd < 3 || p->nd > EMGPU_MAX_ND) return fail(EMGPU_ERR_ARG, "nd outside 3..EMGPU_MAX_ND");
        const int32_t slot[3] = {p->slot_vertrate, p->slot_acc, p->slot_turnrate};
        for (int a = 0; a < 3; a++) {
            if (slot[a] < 0 || slot[a] >= p->nd) return fail(EMGPU_ERR_ARG, "a dynamic slot outside 0..nd-1");
            for (int b = 0; b < a; b++)
                if (slot[a] == slot[b]) return fail(EMGPU_ERR_ARG, "two values name the same dynamic slot");
        }
    }
    return EMGPU_OK;
}

} // namespace

extern "C" {

int emgpu_track_values_device(emgpu_ctx *ctx, const emgpu_track_values_params *p, const double *xyz, void *init_val, void *dyn_val) {
    EMGPU_TRY
    if (const int rc = check_args(p, xyz, init_val, dyn_val)) return rc;
    const bool f64 = p->value_type == EMGPU_VALUE_F64;
    const size_t es = f64 ? 8 : 4, off = (size_t)p->col_offset;
    if (((uintptr_t)xyz & 7u) || ((uintptr_t)init_val & (es - 1)) || ((uintptr_t)dyn_val & 15u))
        return fail(EMGPU_ERR_ARG, "xyz must be 8-byte aligned, init_val aligned to its element and dyn_val 16-byte aligned");
    CTX_ENTER(ctx);
    EmgpuTrackValuesRun A{};
    A.n = p->n; A.ld = p->ld ? p->ld : p->n; A.P = p->points; A.nd = p->nd;
    const int32_t row[5] = {p->row_alt, p->row_speed, p->row_vertrate, p->row_acc, p->row_turnrate};
    memcpy(A.row, row, sizeof row);
    A.slot[0] = p->slot_vertrate; A.slot[1] = p->slot_acc; A.slot[2] = p->slot_turnrate;
    A.ur_speed = p->ur_speed; A.ur_vertrate = p->ur_vertrate; A.ur_heading = p->ur_heading;
    A.xyz = xyz;
    A.init_val = init_val ? (char *)init_val + es * off : nullptr;
    A.dyn_val = dyn_val ? (char *)dyn_val + 4 * es * off : nullptr;
    ctx->last_launches = 0;
    launch_recorded(ctx, emgpu::launch_track_values, A, p->layout == EMGPU_TRACKS_ROWS, f64);
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_track_values_host(emgpu_ctx *ctx, const emgpu_track_values_params *p, const double *xyz, void *init_val, void *dyn_val) {
    EMGPU_TRY
    if (const int rc = check_args(p, xyz, init_val, dyn_val)) return rc;
    if (p->layout != EMGPU_TRACKS_ROWS) return fail(EMGPU_ERR_ARG, "emgpu_track_values_host takes tracks as rows (EMGPU_TRACKS_ROWS)");
    CTX_ENTER(ctx);
    const bool f64 = p->value_type == EMGPU_VALUE_F64;
    ctx->last_launches = 0;
    ctx->last_kernel = f64 ? "k_track_values[ROWS,f64]" : "k_track_values[ROWS,f32]";
    if (p->n == 0) return EMGPU_OK;
    const int64_t ld = p->ld ? p->ld : p->n;
    const size_t es = f64 ? 8 : 4, P = (size_t)p->points, G4 = (P - 2 + 3) / 4;
    // the chunk's device arrays are compact: initial rows 0..4 (altitude, speed, the three rates) and three rows per group of four seconds;
    // the copies back put each row where the caller named it
    const int32_t row[5] = {p->row_alt, p->row_speed, p->row_vertrate, p->row_acc, p->row_turnrate};
    const int32_t slot[3] = {p->slot_vertrate, p->slot_acc, p->slot_turnrate};
    const size_t ni = init_val ? 5 : 0, rows_d = dyn_val ? 3 * G4 : 0;
    enum { XYZ, INIT_VAL, DYN_VAL };   // the chunk's arrays: the tracks as they lie (one row of 24 P bytes per lane), the values as the kernel writes them
    ChunkBlock blk(ctx, "emgpu_track_values_host", p->n, {{24 * P, 1}, {es, ni}, {4 * es, rows_d}});
    const size_t c = (size_t)blk.c();
    EmgpuTrackValuesRun A{};
    A.ld = blk.c(); A.P = p->points; A.nd = 3;
    for (int a = 0; a < 5; a++) A.row[a] = row[a] >= 0 ? a : -1;
    for (int k = 0; k < 3; k++) A.slot[k] = k;
    A.ur_speed = p->ur_speed; A.ur_vertrate = p->ur_vertrate; A.ur_heading = p->ur_heading;
    A.xyz = (const double *)blk.at(XYZ);
    A.init_val = ni ? blk.at(INIT_VAL) : nullptr;
    A.dyn_val = rows_d ? blk.at(DYN_VAL) : nullptr;
    blk.each([&](int64_t c0, int64_t cn) {
        const size_t dst = (size_t)(p->col_offset + c0);
        HIP_OK(hipMemcpyAsync(blk.at(XYZ), xyz + 3 * P * (size_t)c0, 24 * P * (size_t)cn, hipMemcpyHostToDevice, ctx->stream));
        A.n = cn;
        launch_recorded(ctx, emgpu::launch_track_values, A, true, f64);
        for (int a = 0; ni && a < 5; a++)
            if (row[a] >= 0)
                HIP_OK(hipMemcpyAsync((char *)init_val + es * ((size_t)row[a] * (size_t)ld + dst), blk.at(INIT_VAL) + es * (size_t)a * c, es * (size_t)cn,
                                      hipMemcpyDeviceToHost, ctx->stream));
        for (int k = 0; rows_d && k < 3; k++)
            HIP_OK(hipMemcpy2DAsync((char *)dyn_val + 4 * es * ((size_t)slot[k] * (size_t)ld + dst), 4 * es * (size_t)p->nd * (size_t)ld,
                                    blk.at(DYN_VAL) + 4 * es * (size_t)k * c, 4 * es * 3 * c, 4 * es * (size_t)cn, G4, hipMemcpyDeviceToHost,
                                    ctx->stream));
    });
    return EMGPU_OK;
    EMGPU_CATCH
}

} // extern "C"
