// emgpu_dispatch.cpp -- choose_dbn (emgpu_dispatch.h): every rule that sends a sampling call to a kernel instance, and every name an
// instance reports.  Host code only.
#include "emgpu_dispatch.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/emgpu.h"

namespace emgpu {
namespace {

// ---- debug variables (tests, A/B runs), each read once per process
// EMGPU_DEBUG_EVENT_ROWS: "lane" = a list alone also takes the per-lane row loops (k_uncor_fast_ev / _evw, k_dbn_step2 with EV = 1),
// "wide" = every fast-branch list takes k_uncor_fast_evw (its instance holds any fast-branch shape), "long" = every fast-branch list alone
// takes k_uncor_fast_evu_long; any value keeps k_dbn_step2 off the rows built by the wave
struct EventRows { bool set, lane, wide, force_long; };
const EventRows &event_rows() {
    static const EventRows r = [] {
        const char *e = getenv("EMGPU_DEBUG_EVENT_ROWS");
        EventRows v{};
        v.set = e != nullptr;
        v.force_long = v.set && e[0] == 'l' && e[1] == 'o';
        v.lane = v.set && e[0] == 'l' && !v.force_long;
        v.wide = v.set && e[0] == 'w' && e[1] == 'i';
        return v;
    }();
    return r;
}
bool env_set(const char *name) { return getenv(name) != nullptr; }

// ---- event lists: can a plan's list be written by the block kernels?
bool rates_below_edge(const EmgpuPlan &P) {   // every rate below the packed compare's limit (R_h + 1 must fit 16 bits)
    for (int a = 0; a < P.nact; a++)
        if (P.a_R[a] >= 0xFFFF0000u) return false;
    return true;
}
// result slots + a row loop per lane: at most 8 - nd variables with a rate
bool ev_plan_ok(const EmgpuPlan &P, const EmgpuRun &A) { return P.nact <= 8 - P.nd && P.nact <= 5 && A.event_cap >= 1 && rates_below_edge(P); }
// the wide list and the rows built by the wave: 16 - nd streams
bool ev_plan_wide_ok(const EmgpuPlan &P, const EmgpuRun &A) { return P.nact <= 16 - P.nd && A.event_cap >= 1 && rates_below_edge(P); }

bool wants_list(const EmgpuRun &A) { return A.ev_count != nullptr || A.events != nullptr; }
bool list_alone(const EmgpuRun &A) { return A.ev_count != nullptr && A.dyn_bin == nullptr && A.dyn_val == nullptr; }
// plain dbn_sample.m (no resample rows, the value of a row is its bin) returns a list and nothing else
bool plain(const EmgpuRun &A) { return (A.flags & (EMGPU_FLAG_NO_RESAMPLE | EMGPU_FLAG_NO_DEDISC)) != 0; }
// the rate of dynamic variable k is one the packed resample compare takes
bool dyn_rate_below(const EmgpuPlan &P, int k, uint32_t limit) {
    for (int a = 0; a < P.nact; a++)
        if (P.a_dyn[a] == k && P.a_R[a] >= limit) return false;
    return true;
}
int shape_73_93_164(const EmgpuPlan &P) { return (P.ni <= 7 && P.nd <= 3) ? 0 : ((P.ni <= 9 && P.nd <= 3) ? 1 : 2); }

// ---- the fast kernel
struct FastShape { int ni, m0, m1, m2; };
#define EMGPU_X(Q, NI, M0, M1, M2) {NI, M0, M1, M2},
const FastShape kFastShapes[] = {EMGPU_FAST_SHAPES(EMGPU_X)};
#undef EMGPU_X
const char *const kFastNames[4][8] = {   // by FastForm (Dense, Idx, Ev; Evu in row 3) and shape
    {"k_uncor_fast<7,2,2,2>", "k_uncor_fast<7,2,4,2>", "k_uncor_fast<7,2,4,4>", "k_uncor_fast<7,4,2,4>", "k_uncor_fast<7,4,6,4>",
     "k_uncor_fast<7,4,6,6>", "k_uncor_fast<7,6,6,6>", "k_uncor_fast<9,6,6,6>"},
    {"k_uncor_fast_idx<7,2,2,2>", "k_uncor_fast_idx<7,2,4,2>", "k_uncor_fast_idx<7,2,4,4>", "k_uncor_fast_idx<7,4,2,4>", "k_uncor_fast_idx<7,4,6,4>",
     "k_uncor_fast_idx<7,4,6,6>", "k_uncor_fast_idx<7,6,6,6>", "k_uncor_fast_idx<9,6,6,6>"},
    {"k_uncor_fast_ev<7,2,2,2>", "k_uncor_fast_ev<7,2,4,2>", "k_uncor_fast_ev<7,2,4,4>", "k_uncor_fast_ev<7,4,2,4>", "k_uncor_fast_ev<7,4,6,4>",
     "k_uncor_fast_ev<7,4,6,6>", "k_uncor_fast_ev<7,6,6,6>", "k_uncor_fast_ev<9,6,6,6>"},
    {"k_uncor_fast_evu<7,2,2,2>", "k_uncor_fast_evu<7,2,4,2>", "k_uncor_fast_evu<7,2,4,4>", "k_uncor_fast_evu<7,4,2,4>", "k_uncor_fast_evu<7,4,6,4>",
     "k_uncor_fast_evu<7,4,6,6>", "k_uncor_fast_evu<7,6,6,6>", "k_uncor_fast_evu<9,6,6,6>"}};
const char *const kFastEvwName = "k_uncor_fast_evw<9,6,6,6>", *const kFastEvuLongName = "k_uncor_fast_evu_long<9,6,6,6>";
const char *const kFastMixedNames[8] = {"k_uncor_fast_mixed<7,2,2,2>", "k_uncor_fast_mixed<7,2,4,2>", "k_uncor_fast_mixed<7,2,4,4>",
                                        "k_uncor_fast_mixed<7,4,2,4>", "k_uncor_fast_mixed<7,4,6,4>", "k_uncor_fast_mixed<7,4,6,6>",
                                        "k_uncor_fast_mixed<7,6,6,6>", "k_uncor_fast_mixed<9,6,6,6>"};

int fast_shape_of(const EmgpuPlan &P) {
    for (size_t q = 0; q < sizeof kFastShapes / sizeof kFastShapes[0]; q++) {
        const FastShape &f = kFastShapes[q];
        if (P.ni <= f.ni && P.d_meff[0] <= f.m0 && P.d_meff[1] <= f.m1 && P.d_meff[2] <= f.m2) return (int)q;
    }
    return -1;
}

// a list asked for alone goes to the rows built by the wave (plain dbn_sample.m: always, no other form serves it)
bool fast_rows_by_wave(const EmgpuPlan &P, const EmgpuRun &A) {
    const EventRows &env = event_rows();
    return list_alone(A) && ((!env.lane && !env.wide) || plain(A)) && ev_plan_wide_ok(P, A);
}

bool fast_eligible(const EmgpuPlan &P, const EmgpuRun &A) {
    if (P.nd != 3 || P.depend || A.per_step) return false;
    if (wants_list(A) && !ev_plan_ok(P, A) && !(ev_plan_wide_ok(P, A) && P.ni <= 9)) return false;
    if (plain(A) && !(list_alone(A) && ev_plan_wide_ok(P, A))) return false;   // k_uncor_fast_evu serves exactly that
    for (int k = 0; k < 3; k++)
        if (P.d_nb[k] == 0 || P.d_nb[k] > 16 || P.d_meff[k] == 0 || !dyn_rate_below(P, k, 0xFFFF0000u)) return false;   // rate ~ 1: generic path
    return fast_shape_of(P) >= 0;
}

// The form of a fast_eligible call.  With presets only Idx (whatever dense outputs are asked for), Evu and EvuLong have a +start twin
// (k_uncor_fast_ev has no registers to spare): null = the call stays on k_dbn_generic.  Returns the instance's name.
const char *choose_fast(const EmgpuPlan &P, const EmgpuRun &A, bool presets, DbnChoice &c) {
    const EventRows &env = event_rows();
    c.shape = fast_shape_of(P);
    if (A.ev_count == nullptr) {
        c.form = (presets || A.indices != nullptr || A.dyn_bin == nullptr || A.dyn_val == nullptr) ? FastForm::Idx : FastForm::Dense;
    } else if (fast_rows_by_wave(P, A)) {
        // rows expected per wave and 8-second block from the resample rates alone (transition rows come on top): several hundred of them
        // (haa_v1: 1.27 per second and lane -> 650) would take the short queue's 254 requests per round three or four rounds per block
        double rate = 0.0;
        if (!(A.flags & EMGPU_FLAG_NO_RESAMPLE))
            for (int a = 0; a < P.nact; a++) rate += (double)P.a_R[a] * (1.0 / 4294967296.0);
        c.form = (rate * 512.0 > 300.0 || (env.force_long && P.ni <= 9)) ? FastForm::EvuLong : FastForm::Evu;
    } else if (presets) {
        return nullptr;
    } else {   // more rated variables than eight streams hold: the wide list
        c.form = (!ev_plan_ok(P, A) || (env.wide && ev_plan_wide_ok(P, A))) ? FastForm::Evw : FastForm::Ev;
    }
    if (c.form == FastForm::Evw || c.form == FastForm::EvuLong) c.shape = kFastWidest;
    return c.form == FastForm::Evw ? kFastEvwName : c.form == FastForm::EvuLong ? kFastEvuLongName
                                                  : kFastNames[c.form == FastForm::Evu ? 3 : (int)c.form][c.shape];
}

// ---- k_dbn_step2
// the instances' names by shape (<7,3>, <9,3>, <16,4>) and form (w4 reg, w8 reg, reg, general), and the frozen instances'
const char *const kStep2Names[3][4] = {
    {"k_dbn_step2<7,3,w4,reg>", "k_dbn_step2<7,3,w8,reg>", "k_dbn_step2<7,3,reg>", "k_dbn_step2<7,3>"},
    {"k_dbn_step2<9,3,w4,reg>", "k_dbn_step2<9,3,w8,reg>", "k_dbn_step2<9,3,reg>", "k_dbn_step2<9,3>"},
    {"k_dbn_step2<16,4,w4,reg>", "k_dbn_step2<16,4,w8,reg>", "k_dbn_step2<16,4,reg>", "k_dbn_step2<16,4>"}};
const char *const kStep2FrozenName = "k_dbn_step2<16,4>[frozen]", *const kStep2FrozenW4Name = "k_dbn_step2<16,4,w4,reg>[frozen]";

// a list asked for alone: its rows are built by the wave (EMGPU_DEBUG_EVENT_ROWS: tests keep the per-lane row loop reachable)
bool step2_rows_by_wave(const EmgpuPlan &P, const EmgpuRun &A) {
    return A.dyn_bin == nullptr && A.dyn_val == nullptr && !event_rows().set && ev_plan_wide_ok(P, A);
}

// P: step2_plan of the call
bool step2_eligible(const EmgpuPlan &P, const EmgpuRun &A) {
    static const bool off = env_set("EMGPU_DEBUG_NO_STEP2");
    if (off || A.indices != nullptr) return false;   // an index list: k_uncor_fast_idx for the fast-branch models, else the generic kernel
    if (P.nd < 1 || P.nd > 4) return false;
    // (a fast-branch model -- frozen columns, FRZ -- that k_uncor_fast did not take: four dynamic variables, or one or two: balloon_v1)
    if (plain(A) && !list_alone(A)) return false;   // the event instances serve plain dbn_sample.m, the rows' values taken from their bins
    if (wants_list(A)) {
        // the event streams of a block belong to the INSTANCE that runs the model (ND = 4 for the frozen instances and the 16-variable
        // shape, else 3), not to the model: a model with fewer dynamic variables than its instance may carry more rates than the
        // instance has streams for.  Rows by the wave: 16 - ND streams; result slots + a row loop per lane: 8 - ND
        const bool inst4 = !(P.depend || A.per_step) || shape_73_93_164(P) == 2;
        if (step2_rows_by_wave(P, A) ? P.nact > (inst4 ? 12 : 13) : (!ev_plan_ok(P, A) || P.nact > (inst4 ? 4 : 5))) return false;
    }
    for (int k = 0; k < P.nd; k++) {
        if (P.d_nb[k] == 0 || P.d_nb[k] > 16 || P.d_pw[k] == 0 || !dyn_rate_below(P, k, 0xFFFF0000u)) return false;   // rate ~ 1: older kernels
        for (int q = 0; q < P.nd; q++)
            if ((uint64_t)P.d_stride_cur[k][q] * 16u >= (1u << 24) || (uint64_t)P.d_stride_new[k][q] * 16u >= (1u << 24))
                return false; // 24-bit multiplies of the strides in bytes
    }
    return true;
}

// the first entry of the case lists that takes the call, or -1
int step2_mask_case(const EmgpuPlan &P, const EmgpuRun &A, int wmode, uint32_t cur, uint32_t nw, int *case_w, const char **tag) {
    if (A.ev_count == nullptr && (A.dyn_bin == nullptr || A.dyn_val == nullptr)) return -1;   // these instances store both dense outputs unconditionally
    uint32_t wm = 0u;   // the 4-word variables
    for (int k = 0; k < P.nd; k++) wm |= (P.d_pw[k] == 4 ? 1u : 0u) << k;
    int q = 0;
#define EMGPU_S2_CASE(NI_, ND_, W_, C_, N_, TAG_)                                                                  \
    if (P.ni <= NI_ && P.nd == ND_ && (W_ == 0 || wmode == W_) && cur == C_ && nw == N_) { *case_w = W_; *tag = TAG_; return q; } \
    q++;
#define EMGPU_S2_CASE_W(NI_, ND_, WM_, C_, N_, TAG_)                                                               \
    if (A.ev_count == nullptr && P.ni <= NI_ && P.nd == ND_ && wm == WM_ && cur == C_ && nw == N_) { *case_w = 16 + WM_; *tag = TAG_; return q; } \
    q++;
    EMGPU_S2_CASES_ND4
    EMGPU_S2_CASES_ND3
#undef EMGPU_S2_CASE
#undef EMGPU_S2_CASE_W
    return -1;
}

// The instance of a step2_eligible call (P: its step2_plan).  With presets only the GENERAL instance of each shape -- not "reg", widths
// left to run time, every parent -- has a +start twin, for the dense outputs and for the list alone with its rows built by the wave:
// null = the call stays on k_dbn_generic.  Returns the instance's name, *tag its mask case's.
const char *choose_step2(const EmgpuPlan &P, const EmgpuRun &A, bool presets, DbnChoice &c, const char **tag) {
    c.ev = A.ev_count == nullptr ? 0 : (step2_rows_by_wave(P, A) ? 2 : 1);
    if (presets && c.ev == 1) return nullptr;
    c.frozen = !(P.depend || A.per_step);   // fast branch: four dynamic variables, or fewer than three
    c.shape = c.frozen ? 2 : shape_73_93_164(P);
    c.wmode = 0; c.reg = false; c.mask_case = -1;
    bool all_res = true;          // every dynamic variable has a rate
    int wmode = P.d_pw[0];        // the width all columns share, or 0
    for (int k = 0; k < P.nd; k++) {
        all_res = all_res && !dyn_rate_below(P, k, 1u);
        if (P.d_pw[k] != wmode) wmode = 0;
    }
    const bool reg = all_res && P.nd == (shape_73_93_164(P) == 2 ? 4 : 3);
    uint32_t cur, nw;
    step_parent_masks(P, &cur, &nw);   // (frozen: nw = 0 -- a (t+1) parent among the dynamic variables sets EmgpuPlan::depend)
    const char *base;
    static const bool no_masks = env_set("EMGPU_DEBUG_NO_STEP2_MASKS");
    if (presets) {
        base = c.frozen ? kStep2FrozenName : kStep2Names[c.shape][3];
    } else if (c.frozen) {
        // littoral_cor_v1: every variable's only dynamic parent is its own current bin
        const bool own = reg && wmode == 4 && cur == 0x8421u && (A.ev_count != nullptr || (A.dyn_bin != nullptr && A.dyn_val != nullptr));
        if (own) { c.wmode = 4; c.reg = true; }
        base = own ? kStep2FrozenW4Name : kStep2FrozenName;
    } else {
        const int w = c.shape == 2 ? wmode : 0;   // the 3-variable families run the per-variable width instance
        if (reg && !no_masks && (c.shape != 2 || wmode == 4 || wmode == 8)) c.mask_case = step2_mask_case(P, A, w, cur, nw, &c.wmode, tag);
        if (c.mask_case >= 0) {
            c.reg = true;
            base = kStep2Names[c.shape][w == 4 ? 0 : (w == 8 ? 1 : 2)];
        } else {
            c.reg = reg;
            c.wmode = (reg && c.ev == 0 && (wmode == 4 || wmode == 8)) ? wmode : 0;   // event lists: the per-variable-width instances only
            base = kStep2Names[c.shape][reg ? (wmode == 4 ? 0 : (wmode == 8 ? 1 : 2)) : 3];
        }
    }
    return base;
}

// ---- k_dbn_step: the per-timestep DBN with dense output, columns of any width up to 9 bins
const char *const kStepNames[3][2] = {{"k_dbn_step<7,3,8>", "k_dbn_step<7,3,8,lds>"}, {"k_dbn_step<9,3,8>", "k_dbn_step<9,3,8,lds>"},
                                      {"k_dbn_step<16,4,8>", "k_dbn_step<16,4,8,lds>"}};

bool step_eligible(const EmgpuPlan &P, const EmgpuRun &A) {
    if (A.indices != nullptr) return false; // an index list goes through the generic kernel
    if (P.nd < 1 || P.nd > 4 || !(P.depend || A.per_step) || wants_list(A) || plain(A)) return false;
    for (int k = 0; k < P.nd; k++)
        if (P.d_nb[k] == 0 || P.d_nb[k] > 16 || P.d_r[k] > 9 || !dyn_rate_below(P, k, 0xFFFFFFFFu)) return false;
    return true;
}

const char *choose_step(const EmgpuPlan &P, DbnChoice &c) {
    static const bool no_compact = env_set("EMGPU_DEBUG_STEP_NO_COMPACT"), no_lds = env_set("EMGPU_DEBUG_STEP_NO_LDS");
    c.compact = !no_compact;
    for (int k = 0; k < P.nd; k++) c.compact = c.compact && P.d_meff[k] != 0;
    const size_t bytes = (size_t)(c.compact ? P.cthr_total : P.thr_total - P.d_off[0]) * sizeof(uint32_t);
    c.lds = !no_lds && bytes <= 32768;   // stage the dynamic tables in LDS when two workgroups per CU still fit beside the cooperative area
    c.lds_bytes = c.lds ? bytes : 0;
    c.shape = shape_73_93_164(P);
    return kStepNames[c.shape][c.lds ? 1 : 0];
}

// ---- k_dbn_generic: takes every call
const char *const kGenericNames[5] = {"k_dbn_generic<7,3,4>", "k_dbn_generic<7,3,7>", "k_dbn_generic<9,3,9>", "k_dbn_generic<16,4,4>",
                                      "k_dbn_generic<16,4,16>"};

const char *choose_generic(const EmgpuPlan &P, DbnChoice &c) {
    c.shape = (P.ni <= 7 && P.nd <= 3 && P.nact <= 4) ? 0 : (P.ni <= 7 && P.nd <= 3 && P.nact <= 7) ? 1
            : (P.ni <= 9 && P.nd <= 3 && P.nact <= 9) ? 2 : (P.nact <= 4 ? 3 : 4);
    return kGenericNames[c.shape];
}

} // namespace

void step_parent_masks(const EmgpuPlan &P, uint32_t *cur_mask, uint32_t *new_mask) {
    uint32_t c = 0u, n = 0u;
    for (int k = 0; k < P.nd; k++)
        for (int q = 0; q < P.nd; q++) {
            if (P.d_stride_cur[k][q] != 0u) c |= 1u << (4 * k + q);
            if (P.d_stride_new[k][q] != 0u) n |= 1u << (4 * k + q);
        }
    *cur_mask = c; *new_mask = n;
}

EmgpuPlan step2_plan(const EmgpuPlan &P, const EmgpuRun &A) {
    EmgpuPlan Q = P;
    if (A.flags & EMGPU_FLAG_NO_RESAMPLE) Q.nact = 0;   // (the instances without "reg")
    return Q;
}

const char *uncor_fast_mixed_name(int shape) { return shape >= 0 && shape < 8 ? kFastMixedNames[shape] : "none"; }

// A start grid / per-sample log-weights: the +start instances of the fast kernel serve the dense outputs alone and the list alone of a
// fast-branch model, those of the per-timestep kernel the same two forms of every other model it takes; the list and the dense trace
// together, an index list off the fast kernel, and what neither kernel takes run on the general kernel.
DbnChoice choose_dbn(const EmgpuPlan &P, const EmgpuRun &A, bool presets) {
    DbnChoice c;
    memset(&c, 0, sizeof c);
    c.mask_case = -1;
    const EmgpuPlan P2 = step2_plan(P, A);
    const char *base, *tag = "";
    if (fast_eligible(P, A) && (base = choose_fast(P, A, presets, c)) != nullptr) c.family = DbnFamily::Fast;
    else if (step2_eligible(P2, A) && (base = choose_step2(P2, A, presets, c, &tag)) != nullptr) c.family = DbnFamily::Step2;
    else if (!presets && step_eligible(P, A)) { c.family = DbnFamily::Step; base = choose_step(P, c); }
    else { c.family = DbnFamily::Generic; base = choose_generic(P, c); }
    c.start = presets && c.family != DbnFamily::Generic;
    // the name: the instance's literal, its mask case's tag, the event list written as well, the +start twin -- appended here and nowhere else
    const char *list = c.family != DbnFamily::Step2 || c.ev == 0 ? "" : (c.ev == 2 ? "+rows-by-wave+events" : "+events");
    if (A.n <= 0) base = tag = list = "";   // an empty call launches nothing and names no kernel
    snprintf(c.name, sizeof c.name, "%s%s%s%s", base, tag, list, c.start ? "+start" : "");
    return c;
}

} // namespace emgpu
