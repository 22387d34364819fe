// emgpu_encounter.cpp -- emgpu_encounter_pose_device: the intruder's heading, its entry point on the encounter cylinder and the swept
// volume per second of paired tracks (k_encounter_pose, emgpu_kernels_encounter.hip; the definition is in emgpu_encounter.h and DESIGN.md).
// Like emgpu_miss_distance_device it takes no context: no model table, no scratch, no status word; it runs on the stream it is given and on
// the calling thread's current device.
#include <cmath>

#include "emgpu_internal.hpp"
#include "emgpu_encounter.h"

namespace {
// what can be said without a device: EMGPU_OK, or the error (recorded)
int check_args(const emgpu_encounter_params *p, const double *xyz_a, const double *xyz_b, const int64_t *idx_a, const int64_t *idx_b,
               const void *weights_in, const void *pose, const void *rate, const void *flags, const void *weights_out) {
    if (!p) return fail(EMGPU_ERR_ARG, "null argument: p");
    if (!xyz_a) return fail(EMGPU_ERR_ARG, "null argument: xyz_a");
    if (!xyz_b) return fail(EMGPU_ERR_ARG, "null argument: xyz_b");
    if (!pose && !rate && !flags && !weights_out) return fail(EMGPU_ERR_ARG, "null pose, rate, flags and weights_out: nothing to write");
    if (p->points < 2 || p->points > 65537) return fail(EMGPU_ERR_ARG, "points outside 2..65537");
    if (p->n_pairs < 0 || p->n_pairs > ((int64_t)1 << 32)) return fail(EMGPU_ERR_ARG, "n_pairs outside 0..2^32");
    if (p->n_a < 1) return fail(EMGPU_ERR_ARG, "n_a < 1");
    if (p->n_b < 1) return fail(EMGPU_ERR_ARG, "n_b < 1");
    if (p->ld_a != 0 && p->ld_a < p->n_a) return fail(EMGPU_ERR_ARG, "ld_a < n_a");
    if (p->ld_b != 0 && p->ld_b < p->n_b) return fail(EMGPU_ERR_ARG, "ld_b < n_b");
    if (!idx_a && p->n_a > 1 && p->n_pairs > p->n_a) return fail(EMGPU_ERR_ARG, "n_pairs > n_a without idx_a");
    if (!idx_b && p->n_b > 1 && p->n_pairs > p->n_b) return fail(EMGPU_ERR_ARG, "n_pairs > n_b without idx_b");
    if (!(std::isfinite(p->radius_ft) && p->radius_ft > 0.0)) return fail(EMGPU_ERR_ARG, "radius_ft is not a finite positive number");
    if (!(std::isfinite(p->half_height_ft) && p->half_height_ft > 0.0)) return fail(EMGPU_ERR_ARG, "half_height_ft is not a finite positive number");
    if (!(std::isfinite(p->rate_scale) && p->rate_scale > 0.0)) return fail(EMGPU_ERR_ARG, "rate_scale is not a finite positive number");
    if (p->max_attempts < 1 || p->max_attempts > 16) return fail(EMGPU_ERR_ARG, "max_attempts outside 1..16");
    if (weights_in && !weights_out) return fail(EMGPU_ERR_ARG, "weights_in without weights_out");
    return EMGPU_OK;
}
} // namespace

extern "C" {

int emgpu_encounter_pose_device(void *hip_stream, const emgpu_encounter_params *p, const double *xyz_a, const double *xyz_b, const int64_t *idx_a,
                                const int64_t *idx_b, const uint32_t *weights_in, double *pose, double *rate, uint8_t *flags,
                                uint32_t *weights_out) {
    EMGPU_TRY
    if (const int rc = check_args(p, xyz_a, xyz_b, idx_a, idx_b, weights_in, pose, rate, flags, weights_out)) return rc;
    if (((uintptr_t)xyz_a | (uintptr_t)xyz_b | (uintptr_t)idx_a | (uintptr_t)idx_b | (uintptr_t)pose | (uintptr_t)rate) & 7u)
        return fail(EMGPU_ERR_ARG, "xyz_a, xyz_b, idx_a, idx_b, pose and rate must be 8-byte aligned");
    if (((uintptr_t)weights_in | (uintptr_t)weights_out) & 3u) return fail(EMGPU_ERR_ARG, "weights_in and weights_out must be 4-byte aligned");
    if (p->n_pairs == 0) return EMGPU_OK;
    EmgpuEncounterRun A{};
    A.n_pairs = p->n_pairs; A.n_a = p->n_a; A.n_b = p->n_b;
    A.ld_a = p->ld_a ? p->ld_a : p->n_a; A.ld_b = p->ld_b ? p->ld_b : p->n_b;
    A.seed = p->seed; A.first_index = p->first_index; A.max_attempts = p->max_attempts;
    A.R = p->radius_ft; A.H = p->half_height_ft; A.rate_scale = p->rate_scale;
    A.ks = (4.0 * A.R) * A.H;                       // the side's projected area per unit of horizontal speed: 2 R x 2 H
    A.ke = (3.14159265358979323846 * A.R) * A.R;    // an end's area
    A.xyz_a = xyz_a; A.xyz_b = xyz_b; A.idx_a = idx_a; A.idx_b = idx_b; A.weights_in = weights_in;
    A.pose = pose; A.rate = rate; A.flags = flags; A.weights_out = weights_out;
    launch_ok(emgpu::launch_encounter_pose(A, (hipStream_t)hip_stream, nullptr));
    return EMGPU_OK;
    EMGPU_CATCH
}

} // extern "C"
