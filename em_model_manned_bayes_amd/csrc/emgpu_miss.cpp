// emgpu_miss.cpp -- emgpu_miss_distance_device: miss distance, CPA time and NMAC flags of paired tracks (k_miss_distance,
// emgpu_kernels_miss.hip; the definition is in emgpu_miss.h and DESIGN.md).  The one entry point of the library that takes no context: it
// needs no model table, no scratch and no status word, so it runs on the stream it is given and on the calling thread's current device.
#include "emgpu_internal.hpp"
#include "emgpu_miss.h"

namespace {
// what can be said without a device: EMGPU_OK, or the error (recorded)
int check_args(const emgpu_miss_params *p, const double *xyz_a, const double *xyz_b, const int64_t *idx_a, const int64_t *idx_b,
               const void *hmd, const void *vmd, const void *t_cpa, const void *flags, const void *totals) {
    if (!p) return fail(EMGPU_ERR_ARG, "null argument: p");
    if (!xyz_a) return fail(EMGPU_ERR_ARG, "null argument: xyz_a");
    if (!xyz_b) return fail(EMGPU_ERR_ARG, "null argument: xyz_b");
    if (!hmd && !vmd && !t_cpa && !flags && !totals) return fail(EMGPU_ERR_ARG, "null hmd, vmd, t_cpa, flags and totals: nothing to write");
    if (p->points < 1 || p->points > 65537) return fail(EMGPU_ERR_ARG, "points outside 1..65537");
    if (p->n_pairs < 0 || p->n_pairs > ((int64_t)1 << 32)) return fail(EMGPU_ERR_ARG, "n_pairs outside 0..2^32");
    if (p->n_a < 1) return fail(EMGPU_ERR_ARG, "n_a < 1");
    if (p->n_b < 1) return fail(EMGPU_ERR_ARG, "n_b < 1");
    if (p->ld_a != 0 && p->ld_a < p->n_a) return fail(EMGPU_ERR_ARG, "ld_a < n_a");
    if (p->ld_b != 0 && p->ld_b < p->n_b) return fail(EMGPU_ERR_ARG, "ld_b < n_b");
    if (!idx_a && p->n_a > 1 && p->n_pairs > p->n_a) return fail(EMGPU_ERR_ARG, "n_pairs > n_a without idx_a");
    if (!idx_b && p->n_b > 1 && p->n_pairs > p->n_b) return fail(EMGPU_ERR_ARG, "n_pairs > n_b without idx_b");
    if (!(p->nmac_h_ft >= 0.0)) return fail(EMGPU_ERR_ARG, "nmac_h_ft is negative or NaN");
    if (!(p->nmac_v_ft >= 0.0)) return fail(EMGPU_ERR_ARG, "nmac_v_ft is negative or NaN");
    return EMGPU_OK;
}
} // namespace

extern "C" {

int emgpu_miss_distance_device(void *hip_stream, const emgpu_miss_params *p, const double *xyz_a, const double *xyz_b, const int64_t *idx_a,
                               const int64_t *idx_b, const double *pose_b, const uint32_t *weights, double *hmd, double *vmd,
                               int32_t *t_cpa, uint8_t *flags, uint64_t *totals) {
    EMGPU_TRY
    if (const int rc = check_args(p, xyz_a, xyz_b, idx_a, idx_b, hmd, vmd, t_cpa, flags, totals)) return rc;
    if (((uintptr_t)xyz_a | (uintptr_t)xyz_b | (uintptr_t)idx_a | (uintptr_t)idx_b | (uintptr_t)pose_b | (uintptr_t)hmd | (uintptr_t)vmd |
         (uintptr_t)totals) & 7u)
        return fail(EMGPU_ERR_ARG, "xyz_a, xyz_b, idx_a, idx_b, pose_b, hmd, vmd and totals must be 8-byte aligned");
    if (((uintptr_t)weights | (uintptr_t)t_cpa) & 3u) return fail(EMGPU_ERR_ARG, "weights and t_cpa must be 4-byte aligned");
    if (p->n_pairs == 0) return EMGPU_OK;
    EmgpuMissRun A{};
    A.n_pairs = p->n_pairs; A.n_a = p->n_a; A.n_b = p->n_b;
    A.ld_a = p->ld_a ? p->ld_a : p->n_a; A.ld_b = p->ld_b ? p->ld_b : p->n_b;
    A.P = p->points; A.nmac_h = p->nmac_h_ft; A.nmac_v = p->nmac_v_ft;
    A.xyz_a = xyz_a; A.xyz_b = xyz_b; A.idx_a = idx_a; A.idx_b = idx_b; A.pose = pose_b; A.weights = weights;
    A.hmd = hmd; A.vmd = vmd; A.t_cpa = t_cpa; A.flags = flags; A.totals = (unsigned long long *)totals;
    launch_ok(emgpu::launch_miss_distance(A, (hipStream_t)hip_stream, nullptr));
    return EMGPU_OK;
    EMGPU_CATCH
}

} // extern "C"
