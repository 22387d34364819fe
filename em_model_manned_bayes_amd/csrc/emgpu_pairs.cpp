// emgpu_pairs.cpp -- the six entry points on paired 1 Hz tracks (the pairing: emgpu_pairs.h), side by side: emgpu_miss_distance_device
// (k_miss_distance, emgpu_miss.h), emgpu_miss_segments_device (k_miss_segments, emgpu_miss_seg.h), emgpu_encounter_pose_device
// (k_encounter_pose, emgpu_encounter.h), emgpu_cpa_pose_device (k_cpa_pose, emgpu_cpa.h), emgpu_well_clear_device (k_well_clear,
// emgpu_well_clear.h) and emgpu_avoid_device (k_avoid, emgpu_avoid.h).  They take no context: they need no model table, no scratch and
// no status word, so they run on the stream they are given and on the calling thread's current device.
#include <cmath>
#include <initializer_list>

#include "emgpu_internal.hpp"
#include "emgpu_avoid.h"
#include "emgpu_cpa.h"
#include "emgpu_encounter.h"
#include "emgpu_miss.h"
#include "emgpu_miss_seg.h"
#include "emgpu_well_clear.h"

namespace {
// What can be said about a pairing without a device, for either params struct: EMGPU_OK, or the error (recorded).  have_out: the caller
// passed an output; `nothing`: its message when it passed none.  min_points: 1 where one second is enough, 2 where a velocity is read.
template <class Params>
int check_pairing(const Params *p, const double *xyz_a, const double *xyz_b, const int64_t *idx_a, const int64_t *idx_b, bool have_out,
                  const char *nothing, int min_points) {
    if (!p) return fail(EMGPU_ERR_ARG, "null argument: p");
    if (!xyz_a) return fail(EMGPU_ERR_ARG, "null argument: xyz_a");
    if (!xyz_b) return fail(EMGPU_ERR_ARG, "null argument: xyz_b");
    if (!have_out) return fail(EMGPU_ERR_ARG, nothing);
    if (p->points < min_points || p->points > 65537) return fail(EMGPU_ERR_ARG, "points outside " + std::to_string(min_points) + "..65537");
    if (p->n_pairs < 0 || p->n_pairs > ((int64_t)1 << 32)) return fail(EMGPU_ERR_ARG, "n_pairs outside 0..2^32");
    if (p->n_a < 1) return fail(EMGPU_ERR_ARG, "n_a < 1");
    if (p->n_b < 1) return fail(EMGPU_ERR_ARG, "n_b < 1");
    if (p->ld_a != 0 && p->ld_a < p->n_a) return fail(EMGPU_ERR_ARG, "ld_a < n_a");
    if (p->ld_b != 0 && p->ld_b < p->n_b) return fail(EMGPU_ERR_ARG, "ld_b < n_b");
    if (!idx_a && p->n_a > 1 && p->n_pairs > p->n_a) return fail(EMGPU_ERR_ARG, "n_pairs > n_a without idx_a");
    if (!idx_b && p->n_b > 1 && p->n_pairs > p->n_b) return fail(EMGPU_ERR_ARG, "n_pairs > n_b without idx_b");
    return EMGPU_OK;
}

// the pairing's part of an argument block, the pitches' default (0 = n_x) filled in
template <class Params>
void fill_pairing(const Params *p, const double *xyz_a, const double *xyz_b, const int64_t *idx_a, const int64_t *idx_b, EmgpuPairDims &dim,
                  EmgpuPairCols &col) {
    dim = {p->n_pairs, p->n_a, p->n_b, p->ld_a ? p->ld_a : p->n_a, p->ld_b ? p->ld_b : p->n_b};
    col = {xyz_a, xyz_b, idx_a, idx_b};
}
// The refusals of a threshold or an address.  They throw: EMGPU_CATCH records the message and returns the code, as for a failed launch.
void not_negative(double v, const std::string &name) {
    if (!(v >= 0.0)) throw Error(EMGPU_ERR_ARG, name + " is negative or NaN");
}
void finite_positive(double v, const char *name) {
    if (!(std::isfinite(v) && v > 0.0)) throw Error(EMGPU_ERR_ARG, std::string(name) + " is not a finite positive number");
}
template <class Params>
void nmac_thresholds(const Params *p) {
    not_negative(p->nmac_h_ft, "nmac_h_ft");
    not_negative(p->nmac_v_ft, "nmac_v_ft");
}
// the four thresholds of the well-clear volume, named <prefix>tau_s ...
void volume_thresholds(const std::string &prefix, double tau_s, double dmod_ft, double hmd_ft, double h_ft) {
    not_negative(tau_s, prefix + "tau_s");
    not_negative(dmod_ft, prefix + "dmod_ft");
    not_negative(hmd_ft, prefix + "hmd_ft");
    not_negative(h_ft, prefix + "h_ft");
}
// every address of ptrs (null: none given) on a multiple of `bytes`, a power of two; `names` lists them for the message
void aligned(std::initializer_list<const void *> ptrs, unsigned bytes, const char *names) {
    uintptr_t bits = 0;
    for (const void *q : ptrs) bits |= (uintptr_t)q;
    if (bits & (bytes - 1u)) throw Error(EMGPU_ERR_ARG, std::string(names) + " must be " + std::to_string(bytes) + "-byte aligned");
}
} // namespace

extern "C" {

int emgpu_miss_distance_device(void *hip_stream, const emgpu_miss_params *p, const double *xyz_a, const double *xyz_b, const int64_t *idx_a,
                               const int64_t *idx_b, const double *pose_b, const uint32_t *weights, double *hmd, double *vmd,
                               int32_t *t_cpa, uint8_t *flags, uint64_t *totals) {
    EMGPU_TRY
    if (const int rc = check_pairing(p, xyz_a, xyz_b, idx_a, idx_b, hmd || vmd || t_cpa || flags || totals,
                                     "null hmd, vmd, t_cpa, flags and totals: nothing to write", 1))
        return rc;
    nmac_thresholds(p);
    aligned({xyz_a, xyz_b, idx_a, idx_b, pose_b, hmd, vmd, totals}, 8, "xyz_a, xyz_b, idx_a, idx_b, pose_b, hmd, vmd and totals");
    aligned({weights, t_cpa}, 4, "weights and t_cpa");
    if (p->n_pairs == 0) return EMGPU_OK;
    EmgpuMissRun A{};
    fill_pairing(p, xyz_a, xyz_b, idx_a, idx_b, A.dim, A.col);
    A.P = p->points; A.nmac_h = p->nmac_h_ft; A.nmac_v = p->nmac_v_ft; A.pose = pose_b; A.weights = weights;
    A.hmd = hmd; A.vmd = vmd; A.t_cpa = t_cpa; A.flags = flags; A.totals = (unsigned long long *)totals;
    launch_ok(emgpu::launch_miss_distance(A, (hipStream_t)hip_stream, nullptr));
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_miss_segments_device(void *hip_stream, const emgpu_miss_params *p, const double *xyz_a, const double *xyz_b, const int64_t *idx_a,
                               const int64_t *idx_b, const double *pose_b, const uint32_t *weights, double *hmd, double *vmd,
                               double *t_cpa_s, uint8_t *flags, uint64_t *totals) {
    EMGPU_TRY
    if (const int rc = check_pairing(p, xyz_a, xyz_b, idx_a, idx_b, hmd || vmd || t_cpa_s || flags || totals,
                                     "null hmd, vmd, t_cpa_s, flags and totals: nothing to write", 1))
        return rc;
    nmac_thresholds(p);
    aligned({xyz_a, xyz_b, idx_a, idx_b, pose_b, hmd, vmd, t_cpa_s, totals}, 8, "xyz_a, xyz_b, idx_a, idx_b, pose_b, hmd, vmd, t_cpa_s and totals");
    aligned({weights}, 4, "weights");
    if (p->n_pairs == 0) return EMGPU_OK;
    EmgpuMissSegRun A{};
    fill_pairing(p, xyz_a, xyz_b, idx_a, idx_b, A.dim, A.col);
    A.P = p->points; A.nmac_h = p->nmac_h_ft; A.nmac_v = p->nmac_v_ft; A.pose = pose_b; A.weights = weights;
    A.hmd = hmd; A.vmd = vmd; A.t_cpa_s = t_cpa_s; A.flags = flags; A.totals = (unsigned long long *)totals;
    launch_ok(emgpu::launch_miss_segments(A, (hipStream_t)hip_stream, nullptr));
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_encounter_pose_device(void *hip_stream, const emgpu_encounter_params *p, const double *xyz_a, const double *xyz_b, const int64_t *idx_a,
                                const int64_t *idx_b, const uint32_t *weights_in, double *pose, double *rate, uint8_t *flags,
                                uint32_t *weights_out) {
    EMGPU_TRY
    if (const int rc = check_pairing(p, xyz_a, xyz_b, idx_a, idx_b, pose || rate || flags || weights_out,
                                     "null pose, rate, flags and weights_out: nothing to write", 2))
        return rc;
    finite_positive(p->radius_ft, "radius_ft");
    finite_positive(p->half_height_ft, "half_height_ft");
    finite_positive(p->rate_scale, "rate_scale");
    if (p->max_attempts < 1 || p->max_attempts > 16) return fail(EMGPU_ERR_ARG, "max_attempts outside 1..16");
    if (weights_in && !weights_out) return fail(EMGPU_ERR_ARG, "weights_in without weights_out");
    aligned({xyz_a, xyz_b, idx_a, idx_b, pose, rate}, 8, "xyz_a, xyz_b, idx_a, idx_b, pose and rate");
    aligned({weights_in, weights_out}, 4, "weights_in and weights_out");
    if (p->n_pairs == 0) return EMGPU_OK;
    EmgpuEncounterRun A{};
    fill_pairing(p, xyz_a, xyz_b, idx_a, idx_b, A.dim, A.col);
    A.seed = p->seed; A.first_index = p->first_index; A.max_attempts = p->max_attempts;
    A.R = p->radius_ft; A.H = p->half_height_ft; A.rate_scale = p->rate_scale;
    A.ks = (4.0 * A.R) * A.H;                       // the side's projected area per unit of horizontal speed: 2 R x 2 H
    A.ke = (3.14159265358979323846 * A.R) * A.R;    // an end's area
    A.weights_in = weights_in; A.pose = pose; A.rate = rate; A.flags = flags; A.weights_out = weights_out;
    launch_ok(emgpu::launch_encounter_pose(A, (hipStream_t)hip_stream, nullptr));
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_cpa_pose_device(void *hip_stream, const emgpu_cpa_pose_params *p, const double *xyz_a, const double *xyz_b, const int64_t *idx_a,
                          const int64_t *idx_b, const uint32_t *weights_in, double *pose, double *rate, int32_t *t_cpa, uint8_t *flags,
                          uint32_t *weights_out) {
    EMGPU_TRY
    if (const int rc = check_pairing(p, xyz_a, xyz_b, idx_a, idx_b, pose || rate || t_cpa || flags || weights_out,
                                     "null pose, rate, t_cpa, flags and weights_out: nothing to write", 2))
        return rc;
    finite_positive(p->hmd_max_ft, "hmd_max_ft");
    finite_positive(p->vmd_max_ft, "vmd_max_ft");
    finite_positive(p->rate_scale, "rate_scale");
    if (p->max_attempts < 1 || p->max_attempts > 16) return fail(EMGPU_ERR_ARG, "max_attempts outside 1..16");
    if (p->t_lo < 0) return fail(EMGPU_ERR_ARG, "t_lo is negative");
    if (p->t_hi < p->t_lo) return fail(EMGPU_ERR_ARG, "t_hi < t_lo");
    if (p->t_hi > p->points - 2) return fail(EMGPU_ERR_ARG, "t_hi > points - 2: point t_hi + 1 is read");
    if (weights_in && !weights_out) return fail(EMGPU_ERR_ARG, "weights_in without weights_out");
    aligned({xyz_a, xyz_b, idx_a, idx_b, pose, rate}, 8, "xyz_a, xyz_b, idx_a, idx_b, pose and rate");
    aligned({weights_in, weights_out, t_cpa}, 4, "weights_in, weights_out and t_cpa");
    if (p->n_pairs == 0) return EMGPU_OK;
    EmgpuCpaRun A{};
    fill_pairing(p, xyz_a, xyz_b, idx_a, idx_b, A.dim, A.col);
    A.seed = p->seed; A.first_index = p->first_index; A.max_attempts = p->max_attempts;
    A.t_lo = p->t_lo; A.span = (uint32_t)(p->t_hi - p->t_lo + 1);
    A.Hm = p->hmd_max_ft; A.Vm = p->vmd_max_ft; A.rate_scale = p->rate_scale;
    A.kc = (4.0 * A.Hm) * A.Vm;                     // the miss plane's area per unit of horizontal relative speed: 2 Hm x 2 Vm
    A.weights_in = weights_in; A.pose = pose; A.rate = rate; A.t_cpa = t_cpa; A.flags = flags; A.weights_out = weights_out;
    launch_ok(emgpu::launch_cpa_pose(A, (hipStream_t)hip_stream, nullptr));
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_well_clear_device(void *hip_stream, const emgpu_well_clear_params *p, const double *xyz_a, const double *xyz_b, const int64_t *idx_a,
                            const int64_t *idx_b, const double *pose_b, const uint32_t *weights, const uint8_t *miss_flags, int32_t *t_first,
                            int32_t *n_lost, double *tau_min, uint8_t *flags, uint64_t *totals) {
    EMGPU_TRY
    if (const int rc = check_pairing(p, xyz_a, xyz_b, idx_a, idx_b, t_first || n_lost || tau_min || flags || totals,
                                     "null t_first, n_lost, tau_min, flags and totals: nothing to write", 1))
        return rc;
    volume_thresholds("", p->tau_s, p->dmod_ft, p->hmd_ft, p->h_ft);
    aligned({xyz_a, xyz_b, idx_a, idx_b, pose_b, tau_min, totals}, 8, "xyz_a, xyz_b, idx_a, idx_b, pose_b, tau_min and totals");
    aligned({weights, t_first, n_lost}, 4, "weights, t_first and n_lost");
    if (p->n_pairs == 0) return EMGPU_OK;
    EmgpuWellClearRun A{};
    fill_pairing(p, xyz_a, xyz_b, idx_a, idx_b, A.dim, A.col);
    A.P = p->points; A.tau_s = p->tau_s; A.D2 = p->dmod_ft * p->dmod_ft; A.H2 = p->hmd_ft * p->hmd_ft; A.h = p->h_ft;
    A.pose = pose_b; A.weights = weights; A.miss_flags = miss_flags;
    A.t_first = t_first; A.n_lost = n_lost; A.tau_min = tau_min; A.flags = flags; A.totals = (unsigned long long *)totals;
    launch_ok(emgpu::launch_well_clear(A, (hipStream_t)hip_stream, nullptr));
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_avoid_device(void *hip_stream, const emgpu_avoid_params *p, const double *xyz_a, const double *xyz_b, const int64_t *idx_a,
                       const int64_t *idx_b, const double *pose_b, const uint32_t *weights, double *hmd, double *vmd, double *vmd_mit,
                       int32_t *t_cpa, int32_t *t_alert, uint8_t *flags, uint64_t *totals) {
    EMGPU_TRY
    if (const int rc = check_pairing(p, xyz_a, xyz_b, idx_a, idx_b, hmd || vmd || vmd_mit || t_cpa || t_alert || flags || totals,
                                     "null hmd, vmd, vmd_mit, t_cpa, t_alert, flags and totals: nothing to write", 1))
        return rc;
    volume_thresholds("alert_", p->alert_tau_s, p->alert_dmod_ft, p->alert_hmd_ft, p->alert_h_ft);
    nmac_thresholds(p);
    if (p->delay_s < 0) return fail(EMGPU_ERR_ARG, "delay_s is negative");
    if (!(std::isfinite(p->rate_fps) && p->rate_fps >= 0.0)) return fail(EMGPU_ERR_ARG, "rate_fps is negative, NaN or infinite");
    if (!(p->accel_fps2 > 0.0)) return fail(EMGPU_ERR_ARG, "accel_fps2 is not positive or NaN");
    not_negative(p->dz_max_ft, "dz_max_ft");
    aligned({xyz_a, xyz_b, idx_a, idx_b, pose_b, hmd, vmd, vmd_mit, totals}, 8, "xyz_a, xyz_b, idx_a, idx_b, pose_b, hmd, vmd, vmd_mit and totals");
    aligned({weights, t_cpa, t_alert}, 4, "weights, t_cpa and t_alert");
    if (p->n_pairs == 0) return EMGPU_OK;
    EmgpuAvoidRun A{};
    fill_pairing(p, xyz_a, xyz_b, idx_a, idx_b, A.dim, A.col);
    A.P = p->points; A.delay = std::min(p->delay_s, 65537);   // (a longer delay moves no point either: P <= 65537)
    A.tau_s = p->alert_tau_s; A.D2 = p->alert_dmod_ft * p->alert_dmod_ft; A.H2 = p->alert_hmd_ft * p->alert_hmd_ft; A.h = p->alert_h_ft;
    A.nmac_h = p->nmac_h_ft; A.nmac_v = p->nmac_v_ft;
    A.rate = p->rate_fps; A.tr = p->rate_fps / p->accel_fps2; A.half_tr = 0.5 * A.tr; A.half_a = 0.5 * p->accel_fps2; A.dz_max = p->dz_max_ft;
    A.pose = pose_b; A.weights = weights;
    A.hmd = hmd; A.vmd = vmd; A.vmd_mit = vmd_mit; A.t_cpa = t_cpa; A.t_alert = t_alert; A.flags = flags;
    A.totals = (unsigned long long *)totals;
    launch_ok(emgpu::launch_avoid(A, (hipStream_t)hip_stream, nullptr));
    return EMGPU_OK;
    EMGPU_CATCH
}

} // extern "C"
