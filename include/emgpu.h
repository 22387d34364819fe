/*
 * emgpu.h -- C ABI of libemgpu.so: the MI355X-native replacement of the sampling hot path of
 * Airspace-Encounter-Models/em-model-manned-bayes.
 *
 * The reference has no FFI boundary of its own (plain MATLAB functions and handle classes); this
 * header is the boundary a maintainer binds instead.  Every entry point cites the reference
 * interface it replaces (paths relative to the reference's code/matlab/).  The MATLAB-side mex
 * binding and the Python ctypes binding are shown in INTEGRATION.md.
 *
 * Conventions
 *   - C linkage, plain pointers and sizes, no C++/torch types.
 *   - Every function returns an int status (EMGPU_OK or a negative EMGPU_ERR_*); the text of the
 *     last error of the calling thread is returned by emgpu_last_error().
 *   - The caller owns every output buffer.  The library owns only emgpu_model / emgpu_ctx handles.
 *   - Variable ids, bins and the temporal map are 1-based at this boundary, like the reference.
 *   - Matrices that mirror MATLAB arrays are column-major (N{i} is r_i x q_i, em_read.m:191-198).
 *   - Re-entrant per ctx; a ctx is bound to one device and launches on one HIP stream.  Calls on
 *     the same ctx from several threads are serialised by a lock inside the ctx; models are only
 *     read by the sampling calls (setters must not race with sampling, as in any MATLAB handle class).
 */
#ifndef EMGPU_H
#define EMGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EMGPU_OK 0
#define EMGPU_ERR_ARG (-1)          /* bad argument / shape                                        */
#define EMGPU_ERR_IO (-2)           /* file could not be opened                                    */
#define EMGPU_ERR_PARSE (-3)        /* 'Unknown field' em_read.m:104, malformed sections           */
#define EMGPU_ERR_PRESET (-4)       /* 'Attempt to preset a dependent variable' bn_sample.m:47     */
#define EMGPU_ERR_HIP (-5)          /* HIP runtime error                                           */
#define EMGPU_ERR_REJECT_CAP (-6)   /* rejection loop hit max_attempts (reference loops forever)   */
#define EMGPU_ERR_EVENT_CAP (-7)    /* an event list did not fit event_cap rows                    */
#define EMGPU_ERR_NO_DEVICE (-8)    /* no HIP device: the product path has no CPU fallback         */
#define EMGPU_ERR_UNSUPPORTED (-9)  /* model shape beyond the compiled maxima                      */
#define EMGPU_ERR_PRIOR (-10)       /* 'prior:notdbe' / 'prior:unknown' bn_dirichlet_prior.m:28,37 */
#define EMGPU_ERR_SORT (-11)        /* 'Network could not be hierarchically sorted' bn_sort.m:23   */

typedef struct emgpu_model emgpu_model; /* parsed model + priors + start (EncounterModel.m:5-70)   */
typedef struct emgpu_ctx emgpu_ctx;     /* one device + one stream + uploaded tables               */

const char *emgpu_last_error(void);
const char *emgpu_version(void);   /* "emgpu <version> (gfx950) philox4x32-<rounds> src:<hash of the sources it was built from>" */
/* Rounds of the Philox4x32 generator this build draws with (7; builds before round 3 and -DEMGPU_PHILOX_ROUNDS=10 builds: 10).  The
 * round count is part of the sampler's identity: the same (seed, global index) gives other samples under another count, so data and
 * goldens of one count are not comparable with, or resumable by, a build of the other -- check it where that matters. */
int32_t emgpu_philox_rounds(void);
/* Revision of the RNG slot map (which Philox counter word every draw of the reference's algorithm takes).  Like the
 * round count it is part of the sampler's identity: a change gives other samples for the same (seed, global index).
 *   1  rounds 1-4 of this library
 *   2  round 5 on ("emgpu 0.4" is the first version string to say so): terminal propagation takes an attempt's FIRST dediscretize draw from word 3 of its TERM_TRANS block (createEncounter.m:203,
 *      208,216); every other section unchanged -- uncor / cor samples are identical under 1 and 2, terminal tracks are not. */
int32_t emgpu_slot_map_revision(void);

/* ------------------------------------------------------------------------------------------------
 * Model: replaces em_read.m:1-206 and the data half of @EncounterModel/EncounterModel.m
 * ---------------------------------------------------------------------------------------------- */

/* em_read(parameters_filename, 'idxZeroBoundaries', idx, 'isOverwriteZeroBoundaries', flag)
 * (em_read.m:1,41-42).  idx_zero_boundaries may be NULL (=> [1 2 3], em_read.m:42). */
int emgpu_model_load_txt(const char *path, const int32_t *idx_zero_boundaries, int32_t n_idx,
                         int32_t is_overwrite_zero_boundaries, emgpu_model **out);

/* Binary model cache: em_read parses 0.5-3 MB of text and the plan compiler then searches a quantile threshold for
 * every count -- emgpu_model_save_bin writes the parsed model (every field of em_read.m:47-107, the priors, `start`) AND its compiled plan
 * to one file; emgpu_model_load_bin reads it back (no parse, no search).  The file carries the hash of the library's sources
 * (emgpu_version()): a file written by other sources is refused with EMGPU_ERR_PARSE and the caller reads the .txt again.  A loaded model
 * is an ordinary model: setters invalidate its plan like anybody's. */
int emgpu_model_save_bin(const emgpu_model *m, const char *path);
int emgpu_model_load_bin(const char *path, emgpu_model **out);

/* Build a model from caller arrays (the MATLAB struct contract of dbn_sample.m:25-33), so that
 * MATLAB-side edits of N_initial / N_transition / boundaries propagate.
 *   G_*: n x n row-major uint8, [parent][child] (em_read.m:204, bn_sample.m:42).
 *   N_initial: concatenation over nodes 1..n_initial of r_i x q_i column-major counts.
 *   N_transition: concatenation over nodes n_initial+1..n_transition (em_read.m:92).
 *   temporal_map: n_dyn x 2 row-major (var at t, var at t+1), may be NULL when n_transition==0.
 *   boundaries: concatenated, bnd_len[i]==0 means '*' (em_read.m:97-99).  zero_bins (0 = none)
 *   may be NULL => derived like extract_zero_bins (em_read.m:143-156).
 *   labels_* : '\n'-separated, may be NULL. */
typedef struct {
    int32_t n_initial, n_transition, n_dyn, _pad;
    const uint8_t *G_initial, *G_transition;
    const int32_t *r_initial, *r_transition;
    const int32_t *temporal_map;
    const double *N_initial;
    int64_t n_N_initial;
    const double *N_transition;
    int64_t n_N_transition;
    const double *boundaries;
    const int32_t *bnd_len;
    const int32_t *zero_bins;
    const double *resample_rates;
    const char *labels_initial, *labels_transition;
} emgpu_model_desc;
int emgpu_model_from_arrays(const emgpu_model_desc *d, emgpu_model **out);
void emgpu_model_free(emgpu_model *m);

typedef struct {
    int32_t n_initial, n_transition, n_dyn;
    int32_t is_dynvar_depend;  /* any(G_transition(dyn,dyn),'all')  dbn_sample.m:55 */
    int64_t n_N_initial, n_N_transition;
    int32_t max_r, n_resample_active;
} emgpu_model_info_t;
int emgpu_model_info(const emgpu_model *m, emgpu_model_info_t *out);

/* Field access.  get_* copy into out (cap elements) and return the element count (>=0) or an
 * error (<0); passing out==NULL returns the count only. */
enum {
    EMGPU_F_R_INITIAL = 1, EMGPU_F_R_TRANSITION, EMGPU_F_ORDER_INITIAL, EMGPU_F_ORDER_TRANSITION,
    EMGPU_F_TEMPORAL_MAP,   /* n_dyn x 2 row-major                                         */
    EMGPU_F_ZERO_BINS, EMGPU_F_START, EMGPU_F_G_INITIAL, EMGPU_F_G_TRANSITION, /* n*n row-major */
    EMGPU_F_N_INITIAL = 32, EMGPU_F_N_TRANSITION, EMGPU_F_ALPHA_INITIAL, EMGPU_F_ALPHA_TRANSITION,
                            /* node = 1-based variable id; r x q column-major                */
    EMGPU_F_BOUNDARIES,     /* node = 1-based initial variable                               */
    EMGPU_F_RESAMPLE_RATES,
    EMGPU_F_LABELS_INITIAL = 64, EMGPU_F_LABELS_TRANSITION /* '\n'-separated, via get_text   */
};
int64_t emgpu_model_get_i32(const emgpu_model *m, int32_t field, int32_t *out, int64_t cap);
int64_t emgpu_model_get_f64(const emgpu_model *m, int32_t field, int32_t node, double *out, int64_t cap);
int64_t emgpu_model_get_text(const emgpu_model *m, int32_t field, char *out, int64_t cap);
int emgpu_model_set_f64(emgpu_model *m, int32_t field, int32_t node, const double *v, int64_t n);

/* EncounterModel.prior / set.prior (EncounterModel.m:45,194-203) -> bn_dirichlet_prior.m:18-37.
 * kind: 0 = numeric constant `value`; 1 = 'dbe' (1/(r*q)).  Rebuilds both alpha sets. */
int emgpu_model_set_prior(emgpu_model *m, int32_t kind, double value);
/* setTransitionPriors.m:12-33: alpha_transition{ii}(kk, n(kk-1)+1:n*kk) = prior for every dynamic
 * variable that has parents (used by createEncounter.m:129). */
int emgpu_model_set_transition_stay_prior(emgpu_model *m, double prior);
/* EncounterModel.start (EncounterModel.m:52,205-207): n_initial entries, 0 = unset ([] or NaN). */
int emgpu_model_set_start(emgpu_model *m, const int32_t *start, int32_t n);
/* Importance-sampling hook next to `start` and `layers` (UncorEncounterModel.m:204,259-272; InitStartTerminal.m:1-92):
 * log of the model probability of the preset values, sum over preset nodes of log P(x_i = start_i | parents) with
 * P = (N + alpha) column-normalised.  Preset nodes have only preset parents (bn_sample.m:45-47), so this is ONE number per
 * call -- the log-weight of every sample drawn with this `start` (0 when nothing is preset, -inf for an impossible preset).
 * A start GRID (one row of presets per sample) with per-sample weights: emgpu_sample_params.start / emgpu_sample_out.log_weight and
 * emgpu_bn_params.start / .log_weight. */
int emgpu_model_start_log_weight(const emgpu_model *m, double *out);
/* The same per row of a start grid, on the host (no ctx): out[i] = the log-weight of a sample drawn with row i of start [n][n_initial]
 * (by variable id; 0 = unset: the model's own `start` then applies) -- bit for bit what emgpu_sample_out.log_weight receives for that row
 * (the same table of log P, summed over the preset nodes in topological order).  EMGPU_ERR_PRESET, naming the first offending row, under the
 * sampler's two rules: a bin outside 1..r, or a preset node with a parent that is not preset.  What the entry points without a weight output
 * (emgpu_sample_uncor_host, emgpu_sample_text_host, emgpu_track_uncor_grid_*) leave to the caller. */
int emgpu_start_grid_log_weight(const emgpu_model *m, const int32_t *start, int64_t n, double *out);
/* log P(bin | column) of one node as the library computes it: P = N + alpha (alpha as set_prior / the stay prior left it), entry (b, j) =
 * log(w / tot) with tot the column's entries added in ascending bin order; an all-zero column is 0.0 for bin 1 and -inf for the others
 * (select_random.m:17-20).  network: 0 initial, 1 transition; node: 1-based variable id; r x q entries column-major, with the count and
 * capacity conventions of emgpu_model_get_f64 (0 entries for a transition node without a table).  These are the entries
 * emgpu_start_grid_log_weight and emgpu_score_dbn_* add up. */
int64_t emgpu_model_log_prob(const emgpu_model *m, int32_t network, int32_t node, double *out, int64_t cap);
/* EncounterModel.zero_bins (EncounterModel.m:40; derived once by em_read.m:110-114,143-156 and, like in
 * the reference, NOT re-derived when boundaries are replaced): n_initial entries, 0 = none. */
int emgpu_model_set_zero_bins(emgpu_model *m, const int32_t *zero_bins, int32_t n);

/* ------------------------------------------------------------------------------------------------
 * Context
 * ---------------------------------------------------------------------------------------------- */
/* A ctx owns: a stream, the uploaded tables of the models it has sampled (an LRU cache of ~48) and the device scratch of the
 * host-pointer and .track entry points (kept between calls and grown on demand -- a fresh hipMalloc / hipFree of gigabytes per call
 * costs up to 100 ms; emgpu_ctx_free releases everything). */
int emgpu_ctx_create(int32_t device, emgpu_ctx **out);
/* Launch on a caller stream (a hipStream_t passed as void*; NULL = the HIP default stream).
 * A new ctx launches on its own non-blocking stream until this is called. */
int emgpu_ctx_set_stream(emgpu_ctx *ctx, void *hip_stream);
/* Wait for the ctx stream and report deferred per-trajectory errors of *_device calls
 * (EMGPU_ERR_REJECT_CAP / EMGPU_ERR_EVENT_CAP). */
int emgpu_ctx_sync(emgpu_ctx *ctx);
/* Give the device scratch of the host-pointer and .track entry points back (it is kept between calls and only ever grows: one
 * 1 M x 240 s dense host call leaves 3-4 GB with the ctx); the uploaded model tables stay.  Synchronises the ctx stream. */
int emgpu_ctx_trim(emgpu_ctx *ctx);
void emgpu_ctx_free(emgpu_ctx *ctx);

/* ------------------------------------------------------------------------------------------------
 * Sampling: replaces UncorEncounterModel.sample (UncorEncounterModel.m:192-313) and what it calls:
 * dbn_hierarchical_sample.m:1, dbn_sample.m:1, bn_sample.m:1, select_random.m:1, asub2ind.m:1,
 * resample_events.m:1, dediscretize.m:1.
 * ---------------------------------------------------------------------------------------------- */
enum { EMGPU_TRANSITION_REFERENCE_AUTO = 0, EMGPU_TRANSITION_PER_STEP = 1 };
#define EMGPU_FLAG_QUANTIZE500 1u /* 'isQuantize500' UncorEncounterModel.m:202,266-268            */
#define EMGPU_FLAG_NO_RESAMPLE 2u /* skip resample_events (plain dbn_sample.m semantics)           */
#define EMGPU_FLAG_NO_DEDISC 4u   /* skip dediscretize: values are the bin indices                 */
#define EMGPU_FLAG_NO_TERMINATOR 8u /* event lists end without the [T-sum(dt) 0 0] row            */
#define EMGPU_FLAG_LOCAL_SMOOTH 16u /* terminal tracks: smooth speed (5 s) and altitude (15 s) like createEncounter.m:88-89.  local_smooth is
                                       em-core's (not vendored: UNPINNED); the stand-in is a centred moving average whose window shrinks
                                       symmetrically at a track's ends (row i = mean of rows i-k..i+k, k = min((w-1)/2, i, n-1-i)) */

typedef struct {
    uint64_t seed;        /* Philox key.  'seed' of .sample (UncorEncounterModel.m:201)            */
    uint64_t first_index; /* global index of trajectory 0 of this call (multi-GPU sharding)        */
    int64_t n;            /* n_samples                                                             */
    int32_t sample_time;  /* T, seconds (>=1)                                                      */
    int32_t transition_mode;
    uint32_t flags;
    int32_t max_attempts; /* rejection cap (reference: unbounded while, UncorEncounterModel.m:248) */
    int32_t idx_L, idx_v, idx_dh; /* 1-based ids of "L","v","\dot h" (UncorEncounterModel.m:225-229);
                                     idx_v==0 || idx_dh==0 disables the rejection test (:275)      */
    int32_t n_layers;     /* rows of `layers` (r_L) or 0                                           */
    const double *layers; /* n_layers x 2 row-major [lo hi] (UncorEncounterModel.m:204,259-260)    */
    int32_t event_cap;    /* rows per trajectory in `events`                                       */
    int32_t _pad;
    const uint64_t *indices; /* optional: n global indices replacing first_index + i (a device pointer for
                                *_device calls, a host pointer for *_host): arbitrary subsets of a batch, e.g.
                                the trajectories .track re-draws; NULL = the contiguous range               */
    const int32_t *start;    /* optional: a start GRID -- n rows of n_initial preset bins by variable id (row-major; 0 = unset: the
                                model's own `start` then applies), one row per trajectory: what a loop over EncounterModel.start values
                                (UncorEncounterModel.m:204, bn_sample.m:44-50) does in as many calls, in ONE.  A device pointer for
                                *_device calls, a host pointer for *_host.  A row that presets a node without presetting its parents,
                                or a bin outside 1..r, is reported as EMGPU_ERR_PRESET (by emgpu_ctx_sync for *_device calls).
                                A fast-branch model (what runs on k_uncor_fast without a grid) is served at that kernel's pace by its
                                +start instances when the call asks for the dense outputs alone (with or without `indices`) or for
                                the event list alone.  Every other model the per-timestep kernel takes (cor_v1, littoral_cor_v1, the
                                dependent-branch family, EMGPU_TRANSITION_PER_STEP) is served the same two forms, without `indices`,
                                by the +start instances of k_dbn_step2 (the general instance of the model's shape).  The list and the
                                dense trace together, `indices` outside the fast branch, and what neither kernel takes run on the
                                general kernel.  The same holds for calls that ask for log-weights.                                */
} emgpu_sample_params;

/* Event row (8 bytes): what one row [dt var value] of out_events{i} carries. */
typedef struct {
    uint16_t dt;  /* seconds since the previous row                                               */
    uint8_t var;  /* 1-based initial-network variable, 0 = terminator row                         */
    uint8_t bin;  /* discrete value                                                               */
    float value;  /* dediscretised value                                                          */
} emgpu_event;

/* Device-native outputs (time-blocked SoA; any pointer may be NULL to skip that output).
 * G4 = ceil(T/4).  Column c of trajectory i (c = 0 is the initial state, events2samples.m:15-26):
 *   dyn_bin[((c/4)*n_dyn + k)*n + i]        byte (c%4) of the uint32 = bin (1-based)
 *   dyn_val[(((c/4)*n_dyn + k)*n + i)*4 + c%4]
 * with k = row of the temporal map (ascending variable id).  Padding columns >= T are 0.
 *
 * Writing a shard into a larger shared trace: `ld` is the trajectory dimension of the buffers (0 = the
 * call's own n) and `col_offset` the column of trajectory 0 of this call, i.e. trajectory i lands in
 * column col_offset + i of arrays dimensioned [..][ld] (events: list col_offset + i of [ld][event_cap]).
 * That is how the ranks / devices / model blocks of one batch fill one trace without temporaries
 * (SURVEY.md 8e "sort/block by model id"; RUN_1_emsample.m:24-47 is the reference's only sharding). */
typedef struct {
    uint8_t *init_bin;   /* [n_initial][n]                                                        */
    float *init_val;     /* [n_initial][n]                                                        */
    uint32_t *dyn_bin;   /* [G4][n_dyn][n]                                                        */
    float *dyn_val;      /* [G4][n_dyn][n][4]                                                     */
    uint32_t *ev_count;  /* [n] rows written (may exceed event_cap => EMGPU_ERR_EVENT_CAP)        */
    emgpu_event *events; /* [n][event_cap]                                                        */
    int32_t *attempts;   /* [n] attempts used by the rejection loop; <0 => cap hit                */
    int64_t ld;          /* trajectory dimension of every buffer above; 0 => params.n             */
    int64_t col_offset;  /* column of trajectory 0 of this call; col_offset + n <= ld             */
    double *log_weight;  /* [n] (NOT offset by col_offset) per-trajectory importance weight of its presets: the sum over the trajectory's
                            preset nodes of log P(preset | parents), P = (N + alpha) column-normalised -- emgpu_model_start_log_weight
                            per row of the start grid; NULL: not wanted                            */
} emgpu_sample_out;

/* Asynchronous: enqueue on the ctx stream with DEVICE pointers in `out`; returns after launch.
 * Deferred errors are reported by emgpu_ctx_sync. */
int emgpu_sample_dbn_device(emgpu_ctx *ctx, const emgpu_model *m, const emgpu_sample_params *p,
                            const emgpu_sample_out *out);
/* Synchronous, for the MATLAB / Python class layer: HOST pointers in `out` (UncorEncounterModel.m:283-300 hands host arrays back).
 * A pipeline (round 6): the batch is cut into chunks; chunk k's kernel runs on the ctx stream while chunk k-1 crosses PCIe on a copy
 * stream into pinned memory and chunk k-2 is copied into the caller's arrays by a few host threads (pageable arrays), or the copy engine
 * writes straight into the caller's arrays (arrays from emgpu_host_alloc / hipHostMalloc / hipHostRegister).  Event lists are packed on
 * the device first (a prefix sum over ev_count): sum(ev_count) rows cross PCIe, not n x event_cap.  PCIe-inclusive: reported by bench.py
 * as `host_path`, never as the headline.  Of `events` only rows [0, min(ev_count[i], event_cap)) of list i are defined on return. */
int emgpu_sample_dbn_host(emgpu_ctx *ctx, const emgpu_model *m, const emgpu_sample_params *p,
                          const emgpu_sample_out *out);

/* UncorEncounterModel.sample's four outputs (UncorEncounterModel.m:283-300), built on the device: HOST pointers, synchronous.  The pipeline of
 * emgpu_sample_dbn_host, with three steps more on the launch stream after a chunk's event lists are packed -- events2samples.m:9-26 (samples),
 * events2controls.m:11-31 with the unit conversions of :291-297 (controls) and the inits as f64 -- so that what crosses PCIe is the caller's
 * arrays themselves.  Each array is written by the copy engine when it is pinned, else through the library's staging buffers.
 *   samples[i][v][t]  the value of the latest row of list i that names variable v and ends at at <= t with at < T (at = the sum of dt over the
 *                     list up to and including the row), else init_val of v -- column t of out_samples{i}
 *   controls          one row per event row with dt > 0: [t0, x_dh / 60, x_dpsi * (pi / 180), x_dv * 1.68780972222222], t0 the list time
 *                     before the row, x_* the samples of ctrl_var[0..2] at column t0 -- out_EME{i}.event
 * Both lists are packed over the call: list i's rows start at the sum of the counts before it.  The draws are those of emgpu_sample_dbn_host
 * with the same params (counter-based: chunking and capacities do not change them), and ctx's last kernel is the sampler's.
 * EMGPU_ERR_EVENT_CAP when a list outgrows event_cap (totals: the rows the lists need in full, for both totals) or the rows outgrow events_cap /
 * controls_cap (totals: exact); a retry with that room gives the same draws.  params.start (a HOST pointer: uploaded once, every chunk reads
 * its own rows; the weights: emgpu_start_grid_log_weight) is honoured; params.indices is not supported. */
typedef struct {
    double *inits;          /* [n][n_initial] row-major: out_inits                                                               */
    uint32_t *ev_count;     /* [n] rows of list i (> event_cap => EMGPU_ERR_EVENT_CAP)                                          */
    emgpu_event *events;    /* [events_cap] rows, list after list                                                                */
    int64_t events_cap;
    uint32_t *ctrl_count;   /* [n] control rows of trajectory i (its event rows with dt > 0)                                     */
    double *controls;       /* [controls_cap][4] rows [t, dh ft/s, dpsi rad/s, dv ft/s^2], trajectory after trajectory          */
    int64_t controls_cap;
    double *samples;        /* [n][n_initial][sample_time], or NULL: not wanted                                                  */
    int32_t *attempts;      /* [n], or NULL                                                                                      */
    int64_t *totals;        /* [2] out: event rows, control rows of the call                                                     */
    int32_t ctrl_var[3];    /* 1-based ids of "\dot h", "\dot \psi", "\dot v": the control columns in idxEME order (:291)         */
    int32_t _pad;
} emgpu_uncor_out;
int emgpu_sample_uncor_host(emgpu_ctx *ctx, const emgpu_model *m, const emgpu_sample_params *p, const emgpu_uncor_out *out);

/* em_sample's two text files (em_sample.m:57-104; RUN_1_emsample.m), formatted on the device: HOST pointers, synchronous.  The pipeline of
 * emgpu_sample_dbn_host with the dense trace as its device-side product; behind a chunk's sampler launch its rows are formatted (an exact C "%g":
 * six significant digits rounded half to even on the binary value of the f32 widened to double, NaN / Inf / -Inf spelled so) and packed, and
 * what crosses PCIe is the bytes of the files, without their header lines:
 *   initial     one row per trajectory i: "%d " of id_first + i, the n_initial values as "%g" joined by one space, "\n"     (em_sample.m:85-88)
 *   transition  one row per (i, t), t = 0 .. sample_time-1, trajectory after trajectory: "%g %g " of id_first + i and t, the n_dyn values of second t
 *               in temporal-map order as "%g" joined by one space, "\n" (:91-96; the id goes through "%g" here: 1000000 prints as 1e+06)
 * The draws are those of emgpu_sample_dbn_host with the same params (counter-based: chunking and capacities do not change them), the model's own
 * `start` applies, and ctx's last kernel is the sampler's.  totals[0], totals[1]: the bytes of the two texts.  EMGPU_ERR_EVENT_CAP when a text
 * outgrows its capacity (totals: exact, the buffer's content undefined); a retry with that room gives the same bytes.  Pinned buffers
 * (emgpu_host_alloc) are written by the copy engine, pageable ones through the library's staging buffers.  emgpu_text_bound gives capacities
 * that always suffice: bytes[0] = n (21 + 13 n_initial), bytes[1] = n sample_time 13 (2 + n_dyn) -- a "%g" is at most 12 characters, an id
 * through "%d" at most 20, and one character follows each.  params.start (a HOST pointer, n rows: a trajectory's own row wins over the model's
 * `start`) is honoured; params.indices is not supported; id_first >= 0 and
 * id_first + n <= 2^53 (beyond, an id is no longer a double).  emgpu_host_stats describes the call. */
typedef struct {
    char *initial;          /* [initial_cap] bytes                                                                               */
    int64_t initial_cap;
    char *transition;       /* [transition_cap] bytes                                                                            */
    int64_t transition_cap;
    int64_t *totals;        /* [2] out: bytes of the initial / the transition text                                               */
    int64_t id_first;       /* the id of trajectory 0 (em_sample.m:85 counts from 1)                                             */
    float *init_val;        /* [n_initial][n], or NULL: the values the rows print, as emgpu_sample_out lays them out              */
    float *dyn_val;         /* [G4][n_dyn][n][4], or NULL                                                                        */
} emgpu_text_out;
int emgpu_sample_text_host(emgpu_ctx *ctx, const emgpu_model *m, const emgpu_sample_params *p, const emgpu_text_out *out);
int emgpu_text_bound(const emgpu_model *m, int64_t n, int32_t sample_time, int64_t bytes[2]);
/* "%g" of n f32 values by the same device function, one after the other without separators: value i is out[offsets[i] .. offsets[i + 1])
 * (offsets: n + 1 entries).  EMGPU_ERR_EVENT_CAP when cap bytes do not hold them (offsets[n]: the bytes needed).  For tests of the formatter
 * on chosen values, and for callers that write text of their own. */
int emgpu_format_g_host(emgpu_ctx *ctx, const float *x, int64_t n, char *out, int64_t cap, uint64_t *offsets);
/* Test hook: how many finite non-zero values the emgpu_format_g_host calls on this ctx have formatted on the 64-bit path (out[0]) and on the
 * multiword path (out[1]: f32 values of 2^64 and more, and below 10^-6) since the counters were last read; reading clears them. */
int emgpu_debug_format_paths(emgpu_ctx *ctx, uint64_t out[2]);

/* ------------------------------------------------------------------------------------------------
 * Trace placement (round 6).  WHERE a 36 GB trace lies in device memory decides how fast the sampler writes it: the same launch takes
 * 5.9, 6.6 or 7.0 ms depending on the allocation, launch after launch (profiles/r05_placement_probe.txt, profiles/r06_placement_probe.txt).
 * A consumer of emgpu_sample_dbn_device therefore asks the LIBRARY for its trace instead of calling hipMalloc.  Two things happen there:
 *   (i)  blocks of 1 GiB and more are ONE address range backed by separately created 1 GiB physical chunks (the HIP virtual-memory calls):
 *        four to six of six such blocks are of the fast kind where hipMalloc's are mostly of the middle one (why is not known: measured);
 *   (ii) emgpu_trace_alloc allocates `candidates` blocks, times the caller's own call (m, p) on each -- 0.5 s of launches to load the device,
 *        then two rounds of 2 untimed + 5 timed launches per candidate, the better round counts -- keeps the fastest and frees the others.
 *        Candidate 0 is a plain hipMalloc block: report.first_allocation_ms is what the caller's own allocation would have got.
 * What the loop over samples of UncorEncounterModel.m:244 writes into is, here, one such trace.
 *   want        EMGPU_TRACE_* : which outputs the trace holds (events: [ld][p->event_cap] rows)
 *   candidates  0 = automatic: one block (nothing timed) below 1 GiB, where the launch is too short for placement to matter; else 6, or as
 *               many as the device's free memory holds.  1 = one block of kind (i), nothing timed.  n > 1: that many.
 * The trace's trajectory dimension ld is p->n rounded up to 1 024 columns (every row of every array starts on a 1 KiB boundary).
 * emgpu_trace_free gives the block back to the ctx's POOL: the next emgpu_trace_alloc it fits (and is not more than 25 % too large for) takes
 * it without a new probe (report.reused = 1).  emgpu_ctx_trim / emgpu_ctx_free release the pool (the memory goes back to the device; the
 * ADDRESS RANGE of a chunked block is never re-used -- a HIP runtime crashes when a new range overlaps a released one that had been the source
 * of copies; address space is the only cost).  A trace must be freed before its ctx.  The probe launches overwrite the trace with the samples
 * of (p->seed, p->first_index ...): the same samples the caller's own call will write.
 * ---------------------------------------------------------------------------------------------- */
#define EMGPU_TRACE_INIT 1u     /* init_bin + init_val                  */
#define EMGPU_TRACE_DENSE 2u    /* dyn_bin + dyn_val                    */
#define EMGPU_TRACE_EVENTS 4u   /* ev_count + events[ld][p->event_cap]  */
#define EMGPU_TRACE_ATTEMPTS 8u /* attempts                             */
typedef struct emgpu_trace emgpu_trace;
typedef struct {
    int64_t bytes;             /* size of one candidate = one device allocation                                         */
    int64_t ld;                /* trajectory dimension of every array of the trace                                      */
    int32_t candidates;        /* blocks allocated and timed (1: nothing was timed)                                     */
    int32_t kept;              /* index of the kept one, in allocation order                                            */
    int32_t reused;            /* 1: a block of the ctx's pool, placed by an earlier call; nothing was timed now        */
    int32_t _pad;
    float ms[8];               /* per candidate: ms per launch, the better of its two rounds                            */
    float first_allocation_ms; /* = ms[0]: what a caller who keeps the first allocation gets (0: nothing was timed)     */
    float kept_ms;
} emgpu_trace_report_t;
int emgpu_trace_alloc(emgpu_ctx *ctx, const emgpu_model *m, const emgpu_sample_params *p, uint32_t want, int32_t candidates,
                      emgpu_trace **out);
/* The trace as the `out` argument of emgpu_sample_dbn_device / _blocks_device: device pointers, ld set, col_offset 0. */
int emgpu_trace_out(const emgpu_trace *t, emgpu_sample_out *out);
int emgpu_trace_report(const emgpu_trace *t, emgpu_trace_report_t *out);
int emgpu_trace_free(emgpu_ctx *ctx, emgpu_trace *t);

/* Device memory from the allocator the traces come from (nothing is timed): for outputs that are not a DBN trace -- the joined tracks of
 * emgpu_sample_terminal_device (createEncounter.m:74-84), a consumer's own buffers.  Freed by emgpu_device_free, or with the ctx. */
int emgpu_device_alloc(emgpu_ctx *ctx, uint64_t bytes, void **out);
int emgpu_device_free(emgpu_ctx *ctx, void *p);
/* Plain copies between a caller's host array and device memory (a block of emgpu_device_alloc, a trace), on the ctx stream behind the launches
 * already issued; complete when the call returns.  They do not read the deferred status: emgpu_ctx_sync still reports it. */
int emgpu_device_upload(emgpu_ctx *ctx, void *dst_device, const void *src_host, uint64_t bytes);
int emgpu_device_download(emgpu_ctx *ctx, void *dst_host, const void *src_device, uint64_t bytes);

/* ------------------------------------------------------------------------------------------------
 * Scoring a trace: log P(trajectory | model) of every trajectory of a trace in the layout of emgpu_sample_out (init_bin [n_initial][ld],
 * dyn_bin [G4][n_dyn][ld]; ld 0 = n; the call reads columns col_offset .. col_offset + n).  The outputs log_lik [n] and initial [n]
 * (may be NULL) are NOT offset, like log_weight.
 *   log_lik[i] is a double acc that starts at +0.0 and receives, one IEEE addition at a time, entries of emgpu_model_log_prob:
 *   1. for the initial nodes in topological order (order_initial): the entry at the node's bin, in the column its parents' bins select
 *      (asub2ind.m:13-14, parents in ascending index).  initial[i] = acc after this step;
 *   2. for t = 1 .. sample_time-1, and within t for the rows k of the temporal map in ascending order (the k of dyn_bin): the entry of that
 *      variable's (t+1) node at its bin in column t, in the column its parents select.
 *   Parent bins: per step (dbn_sample.m:65-93; EMGPU_TRANSITION_PER_STEP, or REFERENCE_AUTO when is_dynvar_depend) a static parent's bin in
 *   init_bin, a time-t node's bin in column t-1, a (t+1) node's bin in column t; frozen (dbn_sample.m:97-135; REFERENCE_AUTO otherwise)
 *   every parent's bin at column 0 (static parents: init_bin), for all t.
 * -inf entries make the sum -inf; valid bins never give NaN.  A bin outside 1..r among the bins the call reads (init_bin; for sample_time > 1
 * columns 0 .. sample_time-1 of dyn_bin) makes THAT trajectory's log_lik NaN (initial: when the bin is one of init_bin); no read leaves the
 * tables, and the call reports EMGPU_ERR_ARG: _host by its return value (the outputs are written), _device at the next emgpu_ctx_sync.
 * The report of a _device call is a word of the ctx: it stays pending through later calls until an emgpu_ctx_sync returns it.  A sync that
 * has a sampler's deferred error to return (rejection cap, preset, event cap) returns that one and keeps the bad-bin report for the next
 * sync; a _host call reports its own trace only and leaves a pending _device report in place.
 * dyn_bin may be NULL when sample_time == 1 or the model has no transition network.
 * The number is the probability under the networks alone: the normalisation by the rejection loop of UncorEncounterModel.sample (altitude,
 * speed, `layers`) is NOT part of it.  For importance weights between two models of one shape, subtract two scores of the same trace.
 * _host works in chunks of EMGPU_HOST_CHUNK_MB device bytes (default 256) and needs no device memory proportional to n. */
typedef struct {
    int64_t n;
    int32_t sample_time, transition_mode;
    int64_t ld, col_offset;
} emgpu_score_params;
int emgpu_score_dbn_device(emgpu_ctx *ctx, const emgpu_model *m, const emgpu_score_params *p, const uint8_t *init_bin, const uint32_t *dyn_bin,
                           double *log_lik, double *initial);
int emgpu_score_dbn_host(emgpu_ctx *ctx, const emgpu_model *m, const emgpu_score_params *p, const uint8_t *init_bin, const uint32_t *dyn_bin,
                         double *log_lik, double *initial);

/* ------------------------------------------------------------------------------------------------
 * Counting a trace: the sufficient statistics of a trace in the layout above -- how often every cell of the model's count tables N_initial /
 * N_transition was observed.  The inverse of sampling: what EncounterModel.setParameters(N_initial, N_transition, ...) and preallocNInitial
 * (EncounterModel.m) take, which the reference only ever reads from a file.  Parameters: emgpu_score_params, with the rules of
 * emgpu_score_dbn_* (sample_time 1..65535; dyn_bin may be NULL only when nothing transitions, or when the transition network is not counted).
 * An OBSERVATION is one of
 *   (a) an initial node v of a trajectory: the cell (bin of v, column selected by its parents' bins) of N_initial{v} (asub2ind.m:13-14,
 *       parents in ascending index);
 *   (b) for t = 1 .. sample_time-1 and every row k of the temporal map, the (t+1) node of row k at column t: a cell of that node's
 *       N_transition, parent bins read exactly as emgpu_score_dbn_* reads them under the same transition_mode: per step
 *       (EMGPU_TRANSITION_PER_STEP, or REFERENCE_AUTO on a dependent-branch model), frozen at column 0 otherwise.
 *       PER_STEP gives the sufficient statistics of a DBN seen as data.  The frozen mode is the inverse of the reference's frozen-parent
 *       sampler (dbn_sample.m:97-135): a trace drawn that way counts back into the tables it was drawn from.
 * Each observation adds exactly 1 to its cell: nothing is clamped or saturated and no add is lost.  An observation whose own bin, or any
 * parent bin it reads, lies outside 1..r is SKIPPED: it adds nothing, no load or store leaves the buffers, and every other observation of
 * that trajectory still counts (skipping is per observation, not per trajectory: that is what one pass can do).  A call that skipped anything
 * reports EMGPU_ERR_ARG through the channel and by the rules of scoring: _host by its return value, with the counts written; _device at the
 * next emgpu_ctx_sync, through the same pending word.
 * The counts are uint64_t, one array per network: the nodes by variable id 1 .. n_initial (1 .. n_transition), each r x q column-major with
 * exactly the element order and count of emgpu_model_get_f64(EMGPU_F_N_INITIAL / EMGPU_F_N_TRANSITION, node), concatenated; a transition
 * node without a table has 0 elements.  emgpu_count_layout writes the nodes' element offsets and the total: offsets[n nodes + 1]; network 0 =
 * initial, 1 = transition; host only, no ctx.
 * Calls ACCUMULATE: the caller zeroes the arrays, and may count many traces (or ranks: add the per-rank tables) into one.  One call of
 * 10 M x 240 s can put 2.4e9 into one cell, hence 64 bits; the conversion to the model's f64 N is exact below 2^53.
 * Either counts pointer may be NULL: that network is not counted (and its observations report nothing).
 * _host works in chunks of EMGPU_HOST_CHUNK_MB device bytes into device tables of its own and adds them to the caller's host arrays once, at
 * the end; it needs no device memory proportional to n. */
int emgpu_count_layout(const emgpu_model *m, int32_t network, int64_t *offsets);
int emgpu_count_dbn_device(emgpu_ctx *ctx, const emgpu_model *m, const emgpu_score_params *p, const uint8_t *init_bin, const uint32_t *dyn_bin,
                           uint64_t *counts_initial, uint64_t *counts_transition);
int emgpu_count_dbn_host(emgpu_ctx *ctx, const emgpu_model *m, const emgpu_score_params *p, const uint8_t *init_bin, const uint32_t *dyn_bin,
                         uint64_t *counts_initial, uint64_t *counts_transition);

/* ------------------------------------------------------------------------------------------------
 * Counting a trace with integer weights (importance-weighted N).  Everything not restated here is the unweighted count's:
 * the observations, the parent bins per transition mode, the layout of emgpu_count_layout, accumulation, NULL counts pointers.
 *   weights   const uint32_t[n], one entry per trajectory of the window; NOT offset by col_offset (like log_lik).  _device: a device
 *             pointer, _host: a host pointer.  NULL is EMGPU_ERR_ARG: the unweighted call exists for that.
 *   adds      every observation of trajectory i adds weights[i] to its cell, an exact uint64 addition: the result does not depend on the
 *             order of the adds (no float atomics anywhere).
 *   weight 0  the trajectory adds nothing and reports nothing.  Its bins may hold anything, bins outside 1..r included: it never raises
 *             the bad-bin report.  A weight of 0 is the mask that leaves a trajectory of a device-resident trace out.
 *   weight >0 the unweighted rules: an observation that reads a bin outside 1..r is skipped, the others count, and the call reports
 *             EMGPU_ERR_ARG through the same word and protocol (_host by its return value, _device at the next emgpu_ctx_sync).
 *   bounds    no load or store leaves the buffers, whatever the bins and weights are.
 *   one call  n * max(1, sample_time - 1) > 2^32 is refused with EMGPU_ERR_ARG (split the call): below that bound no cell can wrap within a
 *             call, because 2^32 * (2^32 - 1) < 2^64.  Accumulating over several calls stays the caller's business.
 * All argument checks come before any device work.  Weights come from log-weights by a host-side quantization (native.quantize_weights). */
int emgpu_count_dbn_weighted_device(emgpu_ctx *ctx, const emgpu_model *m, const emgpu_score_params *p, const uint8_t *init_bin,
                                    const uint32_t *dyn_bin, const uint32_t *weights, uint64_t *counts_initial, uint64_t *counts_transition);
int emgpu_count_dbn_weighted_host(emgpu_ctx *ctx, const emgpu_model *m, const emgpu_score_params *p, const uint8_t *init_bin,
                                  const uint32_t *dyn_bin, const uint32_t *weights, uint64_t *counts_initial, uint64_t *counts_transition);

/* ------------------------------------------------------------------------------------------------
 * Discretizing a trace: VALUES in the layout of emgpu_sample_out (init_val [n_initial][ld], dyn_val [G4][n_dyn][ld][4]) into the BINS
 * emgpu_score_dbn_* and emgpu_count_dbn_* take (init_bin u8 [n_initial][ld]; dyn_bin u32 [G4][n_dyn][ld], byte c % 4 of word c / 4 = column
 * c), and the repeat / change counts behind a model's resample rates: the training side's discretize_bayes.m, hierarchical_cutpoints.m and
 * hierarchical_discretize.m in one pass.  ld (0 = n) and col_offset apply to the inputs and the outputs alike; columns outside the window,
 * and columns >= sample_time of a larger trace, are neither read nor written (the padding bytes of the last word are written 0).
 * For one value x, promoted exactly to double, of variable v with r bins and boundaries b[0..r] (EMGPU_F_BOUNDARIES):
 *   coarse bin   d = 1 + #{q in 1..r-1 : x >= b[q]} (discretize_bayes.m:14-22): below b[0] gives 1, at or above b[r] gives r, +-inf follow
 *                the compares, a value that equals a cut point belongs to the upper bin;
 *   wrap         where bit v (variable id - 1) of wrap_mask is set: d = 1 + mod(d - 1, r - 1) (hierarchical_discretize.m:29);
 *   categorical  a variable without boundaries ('*', em_read.m:97-99): x must be an integer in 1..r and d = x; never wrapped, no fine bin;
 *   bad value    NaN, or a categorical value that is no integer in 1..r: the bin written is 0 (which scoring and counting treat as outside
 *                1..r), no pair that holds the value is counted, no other value is affected, and the call reports EMGPU_ERR_ARG through the
 *                channel and by the rules of scoring: _host by its return value, with the outputs written; _device at the next
 *                emgpu_ctx_sync, through the same pending word;
 *   fine bin     n_fine in 2..255, for every variable with boundaries: a = b[d-1], h = (b[d] - a) / n_fine,
 *                f = 1 + #{k in 1..n_fine-1 : x >= a + k * h}: one double multiply and one double add per cut, not contracted, the
 *                expression of hierarchical_cutpoints.m:14; equal to hierarchical_discretize.m:37-41 because a + k * h does not decrease in k;
 *   pairs        (hierarchical_discretize.m:43-49) for row k of the temporal map, of variable v, and columns c = 1 .. sample_time-1: when
 *                both values are good, d[c] == d[c-1] and d[c] is not v's zero bin (EMGPU_F_ZERO_BINS), repeat[v] += 1 if
 *                f[c] == f[c-1], else change[v] += 1.  Categorical and static variables receive nothing.
 * repeat and change are uint64_t[n_initial] by variable id, which calls ACCUMULATE into (emgpu_count_dbn_*): EncounterModel.m:243 derives
 * resample_rates = all_change ./ (all_repeat + all_change) from them.  n_fine = 0: bins only, and both may be NULL.
 * Either half (init_val with init_bin, dyn_val with dyn_bin) may be NULL, as a pair.  value_type: EMGPU_VALUE_F32, the sampler's arrays, or
 * EMGPU_VALUE_F64, the same layout with 8-byte elements (tracks given as doubles are not rounded before the compare).  _device: dyn_val
 * 16-byte aligned.  _host works in chunks of EMGPU_HOST_CHUNK_MB device bytes and needs no device memory proportional to n. */
#define EMGPU_VALUE_F32 0
#define EMGPU_VALUE_F64 1
typedef struct {
    int64_t n;
    int32_t sample_time;
    int32_t n_fine;        /* 0, or 2..255 */
    int64_t ld, col_offset;
    int32_t value_type;    /* EMGPU_VALUE_* */
    uint32_t wrap_mask;    /* bit v - 1: variable v wraps */
} emgpu_discretize_params;
int emgpu_discretize_dbn_device(emgpu_ctx *ctx, const emgpu_model *m, const emgpu_discretize_params *p, const void *init_val,
                                const void *dyn_val, uint8_t *init_bin, uint32_t *dyn_bin, uint64_t *repeat, uint64_t *change);
int emgpu_discretize_dbn_host(emgpu_ctx *ctx, const emgpu_model *m, const emgpu_discretize_params *p, const void *init_val,
                              const void *dyn_val, uint8_t *init_bin, uint32_t *dyn_bin, uint64_t *repeat, uint64_t *change);

/* ------------------------------------------------------------------------------------------------
 * Values from tracks: 1 Hz TRACKS (what emgpu_sample2track_*, emgpu_tracks_text_host and a track file hold) into the VALUES of a trace, in
 * the layout emgpu_discretize_dbn_* reads.  The inverse of sample2track.m:183-237, line by line.
 * One track is `points` = P >= 3 positions (x, y, z) in feet, one second apart, as doubles; it yields T = P - 2 seconds of values (row T - 1
 * of the forward update never moved the track, so it cannot be recovered).  All arithmetic is double and not contracted:
 *   displacement  t = 0 .. P-2: dx = x[t+1] - x[t], dy = y[t+1] - y[t], dz = z[t+1] - z[t]             (sample2track.m:211-212, :201)
 *   speed         s[t] = sqrt(dx * dx + dy * dy): two multiplies, one add, an IEEE square root           (:211-212: |speed * (cosd, sind)|)
 *   heading       h[t] = atan2(dy, dx) * 57.29577951308232, one multiply; where s[t] == 0, h[t] = h[t-1], with h[-1] = 0: a standing
 *                 aircraft keeps its heading                                                             (:211-212: the angle; :189)
 *   values        t = 0 .. T-1, true divisions:
 *                 vertical rate  dz[t] / ur_vertrate                                                     (:201 with :131)
 *                 acceleration   (s[t+1] - s[t]) / ur_speed                                              (:204 with :132)
 *                 turn rate      w / ur_heading, d = h[t+1] - h[t], w = d - 360 * floor((d + 180) / 360): w lies in [-180, 180), a
 *                                reversal is -180                                                        (:207 with :133)
 *   initial rows  altitude z[0] (:186), speed s[0] / ur_speed (:188 with :126), the three rates their value at t = 0.
 * Non-finite coordinates are not special-cased and nothing is reported (emgpu_discretize_dbn_* gives a NaN bin 0 and reports it).  A bad
 * point k (0-based) touches, and nothing else: with a bad z, the vertical rates of seconds k-1 and k (and the altitude row for k = 0);
 * with a bad x or y, the accelerations and turn rates of seconds k-2, k-1 and k (and the speed row for k <= 1), and the turn rates of a
 * standing run (s == 0) that directly follows second k, which holds the heading of displacement k.  A NaN coordinate makes all of these
 * NaN.  An infinite z gives infinite vertical rates; an infinite x or y gives accelerations +-inf, NaN, -+inf, but FINITE turn rates that
 * differ from the clean track's: atan2 of an infinite displacement is a multiple of 90 degrees.  The initial rows follow their second 0.
 * Outputs: init_val V [n_initial][ld] and dyn_val V [ceil(T/4)][nd][ld][4] (element t % 4 of group t / 4 = second t), V = float (one
 * rounding of the double) or double by value_type.  Only the rows named are written: row_* in init_val (-1: not written), slot_* in
 * dyn_val; every other row (G, A, any other variable) stays untouched and is the caller's to fill.  The elements of the last group behind T
 * are written 0.  ld (0 = n) and col_offset as for emgpu_discretize_dbn_*.  Either half may be NULL (its rows or slots are then not looked
 * at), not both.  layout: EMGPU_TRACKS_PLANAR xyz [P][3][n], what emgpu_sample2track_device writes; EMGPU_TRACKS_ROWS xyz [n][P][3], what
 * emgpu_sample2track_host returns and a file holds.  Both give bit-equal values.
 * _device: one launch on the ctx's stream; dyn_val 16-byte aligned.  _host: ROWS only, host arrays; works in chunks of EMGPU_HOST_CHUNK_MB
 * device bytes (a chunk of tracks is uploaded as it lies: nothing is transposed on the host).
 * Out of scope: tracks of unequal length in one call (cut them into windows of equal length), smoothing, the terminal model's traj layout,
 * geodetic coordinates, and fitting a model. */
#define EMGPU_TRACKS_PLANAR 0
#define EMGPU_TRACKS_ROWS 1
typedef struct {
    int64_t n;
    int32_t points;        /* P: 3 .. 65537 */
    int32_t value_type;    /* EMGPU_VALUE_* */
    int64_t ld, col_offset;
    int32_t n_initial, nd; /* rows of init_val; rows per group of four seconds of dyn_val */
    int32_t row_alt, row_speed, row_vertrate, row_acc, row_turnrate;   /* 0-based rows of init_val; -1: not written */
    int32_t slot_vertrate, slot_acc, slot_turnrate;                    /* 0-based rows of a dyn_val group */
    int32_t layout;        /* EMGPU_TRACKS_* */
    int32_t reserved;
    double ur_speed, ur_vertrate, ur_heading;                          /* as in emgpu_track_params */
} emgpu_track_values_params;
int emgpu_track_values_device(emgpu_ctx *ctx, const emgpu_track_values_params *p, const double *xyz, void *init_val, void *dyn_val);
int emgpu_track_values_host(emgpu_ctx *ctx, const emgpu_track_values_params *p, const double *xyz, void *init_val, void *dyn_val);

/* ------------------------------------------------------------------------------------------------
 * Miss distance of paired tracks: horizontal miss distance (HMD), vertical miss distance (VMD) at that moment, the time of closest
 * approach (CPA) and whether the encounter is a near mid-air collision (NMAC): CorTerminalModel.m:117-133 (getGeneratedMissDistance) and
 * track.m:175 (nmac = abs(hmd_ft) < 500 & abs(vmd_ft) < 100), for any two sets of 1 Hz tracks.
 * Inputs     two sets of tracks in the PLANAR layout xyz f64 [P][3][ld] that emgpu_sample2track_device writes: set A has n_a columns with
 *            pitch ld_a, set B n_b columns with pitch ld_b (0 = n).  Both hold the same P = `points` >= 1 points, one second apart,
 *            starting at the same second, in feet.
 * Pairs      n_pairs of them.  idx_a / idx_b: optional const int64_t [n_pairs] device arrays.  With idx_x == NULL pair i uses column i of
 *            set X when n_x > 1 (which requires n_pairs <= n_x) and column 0 when n_x == 1: one ownship against every intruder.
 * Pose of B  pose_b: optional const double [5][n_pairs], {c, s, ox, oy, oz} per pair.  Per point x' = (c * x - s * y) + ox,
 *            y' = (s * x + c * y) + oy, z' = z + oz: each product and sum one IEEE double operation in the order written, nothing
 *            contracted.  The caller supplies cosine and sine, so no device sin / cos enters the result.  NULL: B's points are used as
 *            they lie, with no arithmetic (uncor tracks all start at the origin heading east: without a pose no pairing of them is useful).
 * Per second p = 0 .. P-1: dx = xa - xb', dy = ya - yb', d[p] = sqrt(dx * dx + dy * dy) (two multiplies, one add, an IEEE square root;
 *            :122-124, in feet), dz[p] = zb' - za (:125).
 * CPA        t_cpa = the first p at which d[p] is smallest, seconds whose d is NaN skipped (MATLAB's min, :127); hmd = d[t_cpa],
 *            vmd = dz[t_cpa] (:128).  The minimum is over the square roots, not the squares: two different squares can round to one root,
 *            and then the earlier second wins.  No second with a non-NaN d: hmd = vmd = NaN, t_cpa = -1, EMGPU_MISS_NO_CPA.
 * Flags      uint8 per pair.  EMGPU_MISS_NMAC_CPA: hmd < nmac_h_ft && fabs(vmd) < nmac_v_ft (track.m:175).  EMGPU_MISS_NMAC_ANY: some
 *            second has d[p] < nmac_h_ft && fabs(dz[p]) < nmac_v_ft.  NaN compares false.  EMGPU_MISS_NO_CPA.  EMGPU_MISS_BAD_INDEX: an
 *            index outside 0 .. n_x-1; no load is made for that pair, its outputs are NaN, NaN, -1 and it has no other flag.  No load or
 *            store leaves the buffers, whatever the indices and coordinates hold.
 * Outputs    hmd f64 [n_pairs], vmd f64 [n_pairs], t_cpa int32 [n_pairs], flags uint8 [n_pairs], each may be NULL; totals uint64 [8], which
 *            the call ADDS to (the caller zeroes it, as for the count tables): [0] pairs evaluated (indices in range), [1] NMAC at CPA,
 *            [2] NMAC at any second, [3] no CPA, [4] bad index, [5] sum of w over the evaluated pairs, [6] sum of w * NMAC_CPA,
 *            [7] sum of w * NMAC_ANY.  weights: optional const uint32_t [n_pairs] (NULL: 1), the integer weights of the weighted count.
 *            They enter the totals only: every pair is evaluated whatever its weight.  The totals are integers, so the result does not
 *            depend on the order of the adds; with n_pairs <= 2^32 no entry can wrap within a call.  totals[6] / totals[5] is the
 *            importance-weighted NMAC rate.
 * The call takes no context: hip_stream is a hipStream_t as emgpu_ctx_set_stream takes it (NULL: the HIP default stream), the device is
 * the calling thread's current one, every pointer but p is a device pointer, and the call is asynchronous on that stream.
 * EMGPU_ERR_ARG, with a message that names the argument, before any device work: NULL p, xyz_a or xyz_b; every output NULL; points < 1 or
 * > 65537; n_pairs < 0 or > 2^32; n_a or n_b < 1; ld_x < n_x; idx_x == NULL with n_x > 1 and n_pairs > n_x; a threshold that is negative
 * or NaN.  n_pairs == 0 succeeds and launches nothing.
 * Out of scope: tracks of different length or start time (a lag per pair), interpolation between the 1 Hz samples, the ROWS layout, a
 * _host entry point (the chunk driver belongs to the context; the Python binding uploads with torch), the terminal model's traj layout,
 * slant range, and a cross-entropy driver loop. */
#define EMGPU_MISS_NMAC_CPA 1u
#define EMGPU_MISS_NMAC_ANY 2u
#define EMGPU_MISS_NO_CPA 4u
#define EMGPU_MISS_BAD_INDEX 8u
typedef struct {
    int64_t n_pairs;
    int64_t n_a, n_b;
    int64_t ld_a, ld_b;    /* 0 = n_a / n_b */
    int32_t points;        /* P: 1 .. 65537 */
    int32_t reserved;
    double nmac_h_ft, nmac_v_ft;
} emgpu_miss_params;
int emgpu_miss_distance_device(void *hip_stream, const emgpu_miss_params *p, const double *xyz_a, const double *xyz_b, const int64_t *idx_a,
                               const int64_t *idx_b, const double *pose_b, const uint32_t *weights, double *hmd, double *vmd,
                               int32_t *t_cpa, uint8_t *flags, uint64_t *totals);

/* ------------------------------------------------------------------------------------------------
 * Miss distance between the seconds: CPA and NMAC on track segments.  emgpu_miss_distance_device looks at the two aircraft at whole seconds
 * only; two 250 kt aircraft close at up to 844 ft/s and cross the 1000 ft NMAC disc in 1.2 s, so a pair can pass through an NMAC between
 * two samples and the per-second HMD is biased high.  This call reads both tracks as PIECEWISE LINEAR between their 1 Hz points and
 * minimises in closed form per segment.  The params struct, the inputs, the pairing, the pose arithmetic and the bad-index rule are
 * emgpu_miss_distance_device's; so are "no context, asynchronous, device pointers".
 * Everything is f64; every product, sum, quotient and root is one IEEE operation in the order written; nothing is contracted; a NaN
 * compares false.  H = nmac_h_ft, V = nmac_v_ft.
 * Per point p = 0 .. P-1, as above: dx[p] = xa - xb', dy[p] = ya - yb', dz[p] = zb' - za, d[p] = sqrt(dx * dx + dy * dy).
 * Per segment p = 1 .. P-1, between points p-1 and p, with (x0, y0, z0) = (dx, dy, dz)[p-1] and z1 = dz[p]:
 *            ex = dx[p] - x0, ey = dy[p] - y0, ez = z1 - z0;  ee = ex * ex + ey * ey, re = x0 * ex + y0 * ey.
 *            The segment is VALID iff ee, re, z0 and ez are all finite; an invalid segment contributes nothing.
 *            ts = ee > 0 ? (-re) / ee : 0.0.
 *            Interior candidate, iff ts > 0 && ts < 1: px = x0 + ts * ex, py = y0 + ts * ey, ds = sqrt(px * px + py * py),
 *            zs = z0 + ts * ez, at time (double)(p-1) + ts.
 *            Between test: near = min(z0, z1) < V && max(z0, z1) > -V.  If ez != 0: t0 = (-V - z0) / ez, t1 = (V - z0) / ez,
 *            lo = max(min(t0, t1), 0), hi = min(max(t0, t1), 1), as compares and selects (mn = t0 < t1 ? t0 : t1, mx = t0 < t1 ? t1 : t0,
 *            lo = mn > 0 ? mn : 0, hi = mx < 1 ? mx : 1); otherwise lo = 0, hi = 1.  tc = ts; tc = tc > lo ? tc : lo;
 *            tc = tc < hi ? tc : hi.  qx = x0 + tc * ex, qy = y0 + tc * ey, dc = sqrt(qx * qx + qy * qy).
 *            between = near && lo < hi && dc < H.  dc is the horizontal distance minimised over the part of the segment that lies inside
 *            the vertical band: no discriminant, no cancellation.
 * CPA        The candidates in time order: point 0, interior of segment 1, point 1, interior of segment 2, ...  A candidate is taken iff
 *            cand == cand && (none yet || cand < best): the first of equal minima stays.  hmd and vmd are the winner's d and dz (ds and zs
 *            for an interior winner); t_cpa_s is (double)p for a point and (p-1) + ts for an interior.  No candidate: NaN, NaN, -1.0,
 *            EMGPU_MISS_NO_CPA.
 * Flags      uint8 per pair; bits 1, 2, 4 and 8 keep their names.  EMGPU_MISS_NMAC_CPA: from this call's hmd and vmd.  EMGPU_MISS_NMAC_ANY:
 *            some point has d < H && fabs(dz) < V, or some valid segment has `between`.  EMGPU_MISS_CPA_BETWEEN: the CPA is an interior
 *            candidate.  EMGPU_MISS_NMAC_BETWEEN: NMAC_ANY is set and no point has it.  A bad index: NaN, NaN, -1.0 and
 *            EMGPU_MISS_BAD_INDEX alone, no load.
 * Outputs    hmd, vmd, t_cpa_s f64 [n_pairs], flags uint8 [n_pairs], each may be NULL; totals uint64 [10], ADDED to: [0..7] with the
 *            meanings above (NMAC_CPA and NMAC_ANY being this call's), [8] pairs with NMAC_BETWEEN, [9] sum of w over those pairs.
 * EMGPU_ERR_ARG as for emgpu_miss_distance_device, with the same messages for what the two share; t_cpa_s must be 8-byte aligned, and the
 * nothing-to-write message names this call's outputs.  points >= 1; n_pairs == 0 succeeds and launches nothing.
 * Out of scope: curved interpolation, slant range, a lag per pair, the ROWS layout, a _host entry point, a mex command. */
#define EMGPU_MISS_CPA_BETWEEN 16u
#define EMGPU_MISS_NMAC_BETWEEN 32u
int emgpu_miss_segments_device(void *hip_stream, const emgpu_miss_params *p, const double *xyz_a, const double *xyz_b, const int64_t *idx_a,
                               const int64_t *idx_b, const double *pose_b, const uint32_t *weights, double *hmd, double *vmd,
                               double *t_cpa_s, uint8_t *flags, uint64_t *totals /* [10] */);

/* ------------------------------------------------------------------------------------------------
 * Placing the intruder on the encounter cylinder: per pair a random heading of the intruder, its entry point on the surface of a cylinder
 * of radius R and half height H around the ownship, at a point where it flies INTO the cylinder, and the volume the cylinder sweeps per
 * second relative to it (Kochenderfer et al., "Airspace Encounter Models for Estimating Collision Risk": airspace density x E[rate] is the
 * encounter rate, sum(w rate NMAC) / sum(w rate) is P(NMAC | encounter)).  The call writes the pose {c, s, ox, oy, oz} that
 * emgpu_miss_distance_device reads, the rate, and optionally integer weights with the rate folded in.
 * Inputs     the two PLANAR sets of emgpu_miss_distance_device (A = ownship, B = intruder), n_a, n_b, ld_a, ld_b, n_pairs, idx_a / idx_b
 *            with the same column selection, n_x = 1 broadcast and bad-index rule.  points >= 2; only points 0 and 1 are read.
 * Draws      Philox as everywhere: key = seed, counter = {g_lo, g_hi, 0, 13 << 28 | a << 20 | block} with
 *            g = first_index + i; section 13 is ENCOUNTER; u(x) = (min(x, 2^32 - 2) + 0.5) * 2^-32.
 *            A unit-disc point (a = 0: the heading; a = 1: an end-cap position): attempt j = 0 .. max_attempts-1 takes words 2 (j & 1) and
 *            2 (j & 1) + 1 of block j >> 1, p = 2 u - 1, q = 2 u' - 1; the first attempt with 0 < p * p + q * q <= 1 is taken; none:
 *            (p, q) = (1, 0) and EMGPU_ENC_FALLBACK.  a = 2, block 0: word 0 = u1 (surface), word 1 = u2 (lateral offset), word 2 = u3
 *            (height).
 * Per pair   all in f64, every product, sum, quotient and root one IEEE operation in the order written, nothing contracted, no device
 *            sin / cos / atan2:
 *            1. (ax, ay, az) = A[1] - A[0], (bx, by, bz) = B[1] - B[0]: the displacements of the first second.
 *            2. r = sqrt(p * p + q * q), c = p / r, s = q / r (a = 0); vx = c * bx - s * by, vy = s * bx + c * by.
 *            3. rx = vx - ax, ry = vy - ay, wr = bz - az, g = sqrt(rx * rx + ry * ry).
 *            4. Qs = ks * g, Qe = ke * fabs(wr), with ks = (4 * R) * H and ke = (pi * R) * R computed once on the host; Q = Qs + Qe.
 *               !(Q > 0) or Q infinite: EMGPU_ENC_NO_ENTRY, ox = oy = oz = NaN, rate 0, weight 0; c and s are written as drawn, no a = 1
 *               or a = 2 draw enters, and the pair has no EMGPU_ENC_END.
 *            5. Side entry iff u1 * Q < Qs: ex = rx / g, ey = ry / g, m = 2 * u2 - 1, l = R * m, h = R * sqrt(1 - m * m),
 *               relx = (-h) * ex - l * ey, rely = l * ex - h * ey, dz = H * (2 * u3 - 1): uniform in the lateral offset, on the half
 *               that faces the relative velocity.  Otherwise EMGPU_ENC_END: (p', q') the a = 1 disc point, relx = R * p', rely = R * q',
 *               dz = +H when wr < 0, else -H (an intruder that descends relative to the ownship enters through the top).  The a = 1
 *               draw and its EMGPU_ENC_FALLBACK belong to end entries only.
 *            6. ox = (A0x + relx) - (c * B0x - s * B0y), oy = (A0y + rely) - (s * B0x + c * B0y), oz = (A0z + dz) - B0z.
 *            7. rate = Q.
 *            8. weights_out = f <= 2^32 - 1 ? f : 2^32 - 1 with f = floor(w * (Q / rate_scale) + 0.5), w = weights_in[i] (NULL: 1);
 *               EMGPU_ENC_SATURATED when the clamp acted (a NaN f, 0 * inf, clamps too).  Without weights_out no weight is formed and
 *               the flag is never set.
 * Outputs    pose f64 [5][n_pairs], rate f64 [n_pairs], flags uint8 [n_pairs], weights_out uint32 [n_pairs]; each may be NULL, not all.
 *            A bad index: pose NaN, rate 0, weight 0, EMGPU_ENC_BAD_INDEX alone, no load.  No load or store leaves the buffers.
 * The call takes no context and no model, like emgpu_miss_distance_device: hip_stream, the current device, device pointers, asynchronous.
 * EMGPU_ERR_ARG, with a message that names the argument, before any device work: NULL p, xyz_a or xyz_b; every output NULL; points < 2 or
 * > 65537; the n_pairs / n_x / ld_x / idx_x rules of emgpu_miss_distance_device; radius_ft, half_height_ft or rate_scale not finite or
 * <= 0; max_attempts outside 1 .. 16; weights_in without weights_out.  n_pairs == 0 succeeds and launches nothing.
 * Out of scope: a caller-supplied heading, the ROWS layout, a _host entry point, float weights, the terminal model's traj layout.  A
 * placement such that the CPA falls at a chosen second is emgpu_cpa_pose_device, below. */
#define EMGPU_ENC_END 1u
#define EMGPU_ENC_FALLBACK 2u
#define EMGPU_ENC_NO_ENTRY 4u
#define EMGPU_ENC_SATURATED 8u
#define EMGPU_ENC_BAD_INDEX 16u
typedef struct {
    int64_t n_pairs;
    int64_t n_a, n_b;
    int64_t ld_a, ld_b;    /* 0 = n_a / n_b */
    int32_t points;        /* P: 2 .. 65537 */
    int32_t max_attempts;  /* 1 .. 16 */
    uint64_t seed, first_index;
    double radius_ft, half_height_ft;
    double rate_scale;     /* > 0; enters weights_out only */
} emgpu_encounter_params;
int emgpu_encounter_pose_device(void *hip_stream, const emgpu_encounter_params *p, const double *xyz_a, const double *xyz_b, const int64_t *idx_a,
                                const int64_t *idx_b, const uint32_t *weights_in, double *pose, double *rate, uint8_t *flags,
                                uint32_t *weights_out);

/* ------------------------------------------------------------------------------------------------
 * Placing the intruder at a drawn closest approach: per pair a random heading of the intruder, a second tc at which the two aircraft pass,
 * a signed lateral miss within +-Hm and a vertical offset within +-Vm at that second, and the pose {c, s, ox, oy, oz} such that, both
 * flying on as they do during second tc, the pass happens exactly so.  The flux of intruders through that "miss plane", 2 Hm wide and
 * 2 Vm high, perpendicular to the relative horizontal velocity, is uniform in both offsets, so the pair carries a rate as a cylinder
 * entry does: (2 Hm) (2 Vm) g with g the relative horizontal speed.  Where emgpu_encounter_pose_device spends most pairs on entries that
 * miss by far, every pair placed here passes within Hm and Vm: the placement for rare events.  Totals and weights downstream keep their
 * meaning (sum(w rate NMAC) / n estimates E[rate NMAC]) as long as Hm and Vm cover the NMAC thresholds.
 * Inputs     the two PLANAR sets of emgpu_miss_distance_device (A = ownship, B = intruder), n_a, n_b, ld_a, ld_b, n_pairs, idx_a / idx_b
 *            with the same column selection, n_x = 1 broadcast and bad-index rule.  points >= 2; only points tc and tc + 1 are read.
 * Draws      section 13 as above, two streams of their own, so that no existing draw moves: a = 3 is the heading's unit-disc point, taken
 *            exactly as a = 0 above (none found: (p, q) = (1, 0) and EMGPU_CPA_FALLBACK); a = 4, block 0: word 0 = u1 (lateral), word 1 =
 *            u2 (vertical), word 2 = x (the second).
 * Per pair   all in f64, every product, sum, quotient and root one IEEE operation in the order written, nothing contracted, no device
 *            sin / cos / atan2:
 *            0. span = t_hi - t_lo + 1, tc = t_lo + ((uint64)x * span >> 32): integer arithmetic, always below t_lo + span; with
 *               t_lo == t_hi it is that second.
 *            1. (ax, ay, az) = A[tc+1] - A[tc], (bx, by, bz) = B[tc+1] - B[tc] (az and bz enter nothing below).
 *            2. r = sqrt(p * p + q * q), c = p / r, s = q / r (a = 3); vx = c * bx - s * by, vy = s * bx + c * by.
 *            3. rx = vx - ax, ry = vy - ay, g = sqrt(rx * rx + ry * ry).
 *            4. Q = kc * g, with kc = (4 * Hm) * Vm computed once on the host.  !(Q > 0) or Q infinite: EMGPU_CPA_NO_PASS (no horizontal
 *               relative motion, or a NaN horizontal coordinate), ox = oy = oz = NaN, rate 0, weight 0; c, s and tc are written as drawn.
 *            5. ex = rx / g, ey = ry / g; l = Hm * (2 * u1 - 1), relx = (-l) * ey, rely = l * ex: perpendicular to the relative velocity;
 *               dz = Vm * (2 * u2 - 1).
 *            6. ox = (Atc_x + relx) - (c * Btc_x - s * Btc_y), oy = (Atc_y + rely) - (s * Btc_x + c * Btc_y), oz = (Atc_z + dz) - Btc_z:
 *               emgpu_miss_distance_device's convention, applied at point tc.
 *            7. rate = Q, t_cpa = tc.
 *            8. weights_out = f <= 2^32 - 1 ? f : 2^32 - 1 with f = floor(w * (Q / rate_scale) + 0.5), w = weights_in[i] (NULL: 1);
 *               EMGPU_CPA_SATURATED when the clamp acted (a NaN f, 0 * inf, clamps too).  Without weights_out no weight is formed and
 *               the flag is never set.
 * Outputs    pose f64 [5][n_pairs], rate f64 [n_pairs], t_cpa int32 [n_pairs], flags uint8 [n_pairs], weights_out uint32 [n_pairs]; each
 *            may be NULL, not all.  A bad index: pose NaN, rate 0, weight 0, t_cpa -1, EMGPU_CPA_BAD_INDEX alone, no load and no draw.
 *            No load or store leaves the buffers.  The flags have the values of the EMGPU_ENC_* bits they correspond to.
 * The call takes no context and no model: hip_stream, the current device, device pointers, asynchronous.
 * EMGPU_ERR_ARG, with a message that names the argument, before any device work: everything emgpu_encounter_pose_device refuses (points
 * outside 2 .. 65537); hmd_max_ft, vmd_max_ft or rate_scale not finite or <= 0; t_lo < 0, t_hi < t_lo or t_hi > points - 2; weights_in
 * without weights_out.  n_pairs == 0 succeeds and launches nothing.
 * Out of scope: a caller-supplied heading or offsets, a CPA inside a second, the ROWS layout, a _host entry point, float weights, a mex
 * command, the terminal model's traj layout. */
#define EMGPU_CPA_FALLBACK 2u
#define EMGPU_CPA_NO_PASS 4u
#define EMGPU_CPA_SATURATED 8u
#define EMGPU_CPA_BAD_INDEX 16u
typedef struct {
    int64_t n_pairs;
    int64_t n_a, n_b;
    int64_t ld_a, ld_b;    /* 0 = n_a / n_b */
    int32_t points;        /* P: 2 .. 65537 */
    int32_t max_attempts;  /* 1 .. 16 */
    uint64_t seed, first_index;
    int32_t t_lo, t_hi;    /* the seconds the pass is drawn from: 0 <= t_lo <= t_hi <= points - 2 */
    double hmd_max_ft, vmd_max_ft;
    double rate_scale;     /* > 0; enters weights_out only */
} emgpu_cpa_pose_params;
int emgpu_cpa_pose_device(void *hip_stream, const emgpu_cpa_pose_params *p, const double *xyz_a, const double *xyz_b, const int64_t *idx_a,
                          const int64_t *idx_b, const uint32_t *weights_in, double *pose, double *rate, int32_t *t_cpa, uint8_t *flags,
                          uint32_t *weights_out);

/* ------------------------------------------------------------------------------------------------
 * Loss of DAA well clear of paired tracks: the second event beside the NMAC that detect-and-avoid evaluations report.  A pair has lost
 * well clear at a second when the two aircraft are within h_ft vertically AND horizontally either inside DMOD or closing such that the
 * modified tau is at most tau_s with a predicted horizontal miss of at most hmd_ft.  The predicate is evaluated at every whole second on
 * the relative state emgpu_miss_distance_device forms; P(LoWC | encounter) and P(NMAC | LoWC) follow from the weighted totals.
 * Inputs     emgpu_miss_distance_device's: the two PLANAR sets, n_a, n_b, ld_a, ld_b, n_pairs, idx_a / idx_b with the same column
 *            selection, n_x = 1 broadcast and bad-index rule; the optional pose_b [5][n_pairs], applied per point exactly as stated there;
 *            the optional weights uint32 [n_pairs].  One more optional input, miss_flags const uint8 [n_pairs]: the flags output of
 *            emgpu_miss_distance_device or emgpu_miss_segments_device for the same pairs; only its EMGPU_MISS_NMAC_ANY bit is read.
 * Thresholds tau_s (35 s), dmod_ft (4000 ft), hmd_ft (4000 ft), h_ft (450 ft) are the usual ones; the struct has no defaults.
 *            D2 = dmod_ft * dmod_ft, H2 = hmd_ft * hmd_ft, computed once on the host.
 * Everything is f64; every product, sum and quotient is one IEEE double operation in the order written; nothing is contracted; a NaN
 * compares false.  No square root enters.
 * Relative state at point p = 0 .. P-1, as above: dx = xa - xb', dy = ya - yb', dz = zb' - za.  The relative velocity at point p is the
 *            forward difference of the segment that starts there, the last point taking the last segment's: with q = min(p, P-2),
 *            ux = dx[q+1] - dx[q], uy = dy[q+1] - dy[q]; for P = 1, ux = uy = 0.
 * Per point  with (x, y, z) = (dx, dy, dz)[p]:
 *            rr = x * x + y * y, rv = x * ux + y * uy, vv = ux * ux + uy * uy
 *            valid   = rr, rv, vv and z all finite
 *            inside  = rr <= D2;  closing = rv < 0
 *            tau     = inside ? 0 : (closing ? (D2 - rr) / rv : +inf)
 *            tc      = vv > 0 ? (-rv) / vv : 0;  tc = tc > 0 ? tc : 0
 *            px = x + tc * ux, py = y + tc * uy, hp2 = px * px + py * py
 *            by_tau  = !inside && closing && tau <= tau_s && hp2 <= H2
 *            lost[p] = valid && fabs(z) <= h_ft && (inside || by_tau)
 *            The comparisons are <=, as the well-clear standard states them: this DIFFERS from the NMAC test of the miss-distance calls,
 *            which uses <.
 * Outputs    per pair, each may be NULL: t_first int32 [n_pairs], the first p with lost[p], -1 if none; n_lost int32 [n_pairs], the number
 *            of such p; tau_min f64 [n_pairs], the smallest tau over the valid points (+inf if none of them is inside or closing, NaN if
 *            no point is valid); flags uint8 [n_pairs]: EMGPU_WC_LOST (some lost[p]), EMGPU_WC_AT_START (lost[0]), EMGPU_WC_NO_DATA (no
 *            valid point), EMGPU_WC_BAD_INDEX (as for the miss-distance calls: nothing loaded; -1, 0, NaN written; no other flag),
 *            EMGPU_WC_INSIDE_DMOD (some lost point had `inside`), EMGPU_WC_BY_TAU (some lost point had `by_tau`).
 *            totals uint64 [10], ADDED to, w = weights[i] (NULL: 1): [0] pairs evaluated, [1] LOST, [2] AT_START, [3] NO_DATA,
 *            [4] BAD_INDEX, [5] sum of w over the evaluated pairs, [6] sum of w * LOST, [7] sum of w * AT_START, [8] pairs with LOST whose
 *            miss_flags has EMGPU_MISS_NMAC_ANY (0 without miss_flags), [9] sum of w over those.  [9] / [6] is the weighted
 *            P(NMAC | LoWC); ([6] - [7]) / ([5] - [7]) is P(LoWC) over the pairs that did not start inside the volume.  At least one of
 *            the per-pair outputs and totals must be given.  No load or store leaves the buffers.
 * The call takes no context and no model: hip_stream, the current device, device pointers, asynchronous.
 * EMGPU_ERR_ARG, with a message that names the argument, before any device work: everything emgpu_miss_distance_device refuses about the
 * pairing (points outside 1 .. 65537), with the same messages; tau_s, dmod_ft, hmd_ft or h_ft negative or NaN; every output NULL; a
 * pointer that is not aligned to its element (8 bytes for doubles, indices and totals; 4 for weights, t_first and n_lost).  n_pairs == 0
 * succeeds and launches nothing.
 * Out of scope: the predicate between the seconds, vertical tau and the terminal / TCAS-RA variants of the volume, the severity metric
 * (SLoWC), an alerting or avoidance logic, the ROWS layout, a _host entry point, a mex command, a lag per pair. */
#define EMGPU_WC_LOST 1u
#define EMGPU_WC_AT_START 2u
#define EMGPU_WC_NO_DATA 4u
#define EMGPU_WC_BAD_INDEX 8u
#define EMGPU_WC_INSIDE_DMOD 16u
#define EMGPU_WC_BY_TAU 32u
typedef struct {
    int64_t n_pairs;
    int64_t n_a, n_b;
    int64_t ld_a, ld_b;    /* 0 = n_a / n_b */
    int32_t points;        /* P: 1 .. 65537 */
    int32_t reserved;
    double tau_s, dmod_ft, hmd_ft, h_ft;
} emgpu_well_clear_params;
int emgpu_well_clear_device(void *hip_stream, const emgpu_well_clear_params *p, const double *xyz_a, const double *xyz_b, const int64_t *idx_a,
                            const int64_t *idx_b, const double *pose_b, const uint32_t *weights, const uint8_t *miss_flags, int32_t *t_first,
                            int32_t *n_lost, double *tau_min, uint8_t *flags, uint64_t *totals /* [10] */);

/* ------------------------------------------------------------------------------------------------
 * Ownship vertical avoidance on paired tracks: alert, manoeuvre, risk ratio.  The calls above are UNMITIGATED: both aircraft fly their
 * tracks blindly.  Here the ownship (set A) answers the first alert with one vertical manoeuvre, and the call reports the NMAC with and
 * without it: sum(w NMAC_MIT) / sum(w NMAC_UNMIT) is the risk ratio.  The alert is the per-point predicate of emgpu_well_clear_device with
 * thresholds of its own; the manoeuvre is a closed form of the seconds since the alert, so no mitigated track is written anywhere.
 * Inputs     emgpu_well_clear_device's, without miss_flags: the two PLANAR sets (A = ownship, B = intruder), n_a, n_b, ld_a, ld_b, n_pairs,
 *            idx_a / idx_b with the same column selection, n_x = 1 broadcast and bad-index rule; the optional pose_b [5][n_pairs]; the
 *            optional weights uint32 [n_pairs].
 * Parameters the struct has no defaults.  The Python binding's (alert_tau_s 60 s, alert_dmod_ft 4000 ft, alert_hmd_ft 4000 ft, alert_h_ft
 *            700 ft; nmac_h_ft 500 ft, nmac_v_ft 100 ft; delay_s 5 s, rate_fps 25 ft/s = 1500 ft/min, accel_fps2 8 ft/s^2, about 0.25 g,
 *            dz_max_ft +inf) are an ILLUSTRATION, not the alerting thresholds of any standard.  The host forms once D2 = alert_dmod_ft *
 *            alert_dmod_ft, H2 = alert_hmd_ft * alert_hmd_ft, tr = rate_fps / accel_fps2, half_tr = 0.5 * tr, half_a = 0.5 * accel_fps2;
 *            accel_fps2 = +inf is allowed and gives tr = 0: the full rate from the first second.
 * Everything is f64; every product, sum, quotient and root is one IEEE double operation in the order written; nothing is contracted; a NaN
 * compares false.
 * State      dx, dy, dz[p], d[p] = sqrt(dx * dx + dy * dy) as for emgpu_miss_distance_device (dz = zb' - za); the relative velocity
 *            (ux, uy) at point p as for emgpu_well_clear_device (q = min(p, P-2); P = 1: 0), and wz = dz[q+1] - dz[q] (P = 1: 0).
 * Alert      alert[p] = lost[p] of emgpu_well_clear_device with tau_s = alert_tau_s, D2, H2 and h_ft = alert_h_ft, on the UNMITIGATED state.
 *            t_alert = the first p with alert[p], -1 if none.  Only the first alert acts: no reversal, no strengthening.
 * Sense      fixed at t_alert from the intruder's predicted vertical offset at the horizontal closest approach: with (x, y, z) the state
 *            there and tc the clamped tc of the predicate, zp = z + tc * wz; descend = zp > 0 || (!(zp < 0) && z > 0); otherwise the
 *            ownship climbs.  A zero or NaN zp falls back to the sign of z, and z = 0 climbs.
 * Manoeuvre  t0 = t_alert + delay_s.  For a point p with k = p - t0 >= 1, kd = (double)k:
 *            g = kd < tr ? half_a * (kd * kd) : rate_fps * (kd - half_tr);  g = g < dz_max_ft ? g : dz_max_ft
 *            dz'[p] = climb ? dz[p] - g : dz[p] + g
 *            For k <= 0, or without an alert, dz'[p] = dz[p] exactly (no arithmetic).  The horizontal state is untouched.  The alert of
 *            point p is known when point p + 1 arrives, so k >= 1 is causal even with delay_s = 0.
 * Outputs    per pair, each may be NULL: hmd, vmd f64 and t_cpa int32 [n_pairs], bit for bit what emgpu_miss_distance_device writes
 *            (no second holding a number: NaN, NaN, -1); vmd_mit f64 [n_pairs] = dz'[t_cpa] (NaN without a CPA); t_alert int32 [n_pairs];
 *            flags uint8 [n_pairs]: EMGPU_AVOID_ALERTED; EMGPU_AVOID_CLIMB (only with ALERTED); EMGPU_AVOID_NMAC_UNMIT (some p with
 *            d[p] < nmac_h_ft && fabs(dz[p]) < nmac_v_ft: emgpu_miss_distance_device's NMAC_ANY); EMGPU_AVOID_NMAC_MIT (the same test with
 *            dz'[p]); EMGPU_AVOID_LATE (ALERTED and t0 >= P - 1: no point was moved); EMGPU_AVOID_NO_CPA (no second holds a number);
 *            EMGPU_AVOID_BAD_INDEX (nothing loaded; NaN, NaN, -1, NaN, -1 written; no other flag).
 *            totals uint64 [12], ADDED to, w = weights[i] (NULL: 1), "induced" = NMAC_MIT && !NMAC_UNMIT: [0] pairs evaluated,
 *            [1] ALERTED, [2] NMAC_UNMIT, [3] NMAC_MIT, [4] induced, [5] NO_CPA, [6] BAD_INDEX, [7] sum of w over the evaluated pairs,
 *            [8] sum of w * ALERTED, [9] sum of w * NMAC_UNMIT, [10] sum of w * NMAC_MIT, [11] sum of w * induced.  [10] / [9] is the
 *            weighted risk ratio.  No load or store leaves the buffers.
 * The call takes no context and no model: hip_stream, the current device, device pointers, asynchronous.
 * EMGPU_ERR_ARG, with a message that names the argument, before any device work: everything emgpu_miss_distance_device refuses about the
 * pairing (points outside 1 .. 65537), with the same messages; one of the six thresholds negative or NaN; delay_s < 0; rate_fps negative,
 * NaN or infinite; accel_fps2 <= 0 or NaN; dz_max_ft negative or NaN; every output NULL; a pointer that is not aligned to its element
 * (8 bytes for doubles, indices and totals; 4 for weights, t_cpa and t_alert).  n_pairs == 0 succeeds and launches nothing.
 * Out of scope: horizontal manoeuvres, a sense reversal or a second alert, an intruder that reacts, the mitigated loss of well clear (its
 * ratio needs a second predicate per second and is a call of its own), evaluation between the seconds, the ROWS layout, a _host entry
 * point, a mex command, a limit on the altitude or on the ownship's total vertical rate. */
#define EMGPU_AVOID_ALERTED 1u
#define EMGPU_AVOID_CLIMB 2u
#define EMGPU_AVOID_NMAC_UNMIT 4u
#define EMGPU_AVOID_NMAC_MIT 8u
#define EMGPU_AVOID_LATE 16u
#define EMGPU_AVOID_NO_CPA 32u
#define EMGPU_AVOID_BAD_INDEX 64u
typedef struct {
    int64_t n_pairs;
    int64_t n_a, n_b;
    int64_t ld_a, ld_b;    /* 0 = n_a / n_b */
    int32_t points;        /* P: 1 .. 65537 */
    int32_t delay_s;       /* >= 0: whole seconds between the alert and the start of the manoeuvre */
    double alert_tau_s, alert_dmod_ft, alert_hmd_ft, alert_h_ft;
    double nmac_h_ft, nmac_v_ft;
    double rate_fps, accel_fps2, dz_max_ft;
} emgpu_avoid_params;
int emgpu_avoid_device(void *hip_stream, const emgpu_avoid_params *p, const double *xyz_a, const double *xyz_b, const int64_t *idx_a,
                       const int64_t *idx_b, const double *pose_b, const uint32_t *weights, double *hmd, double *vmd, double *vmd_mit,
                       int32_t *t_cpa, int32_t *t_alert, uint8_t *flags, uint64_t *totals /* [12] */);

/* Pinned host memory for the outputs of the *_host entry points (hipHostMalloc, kept in a per-ctx pool: pinning gigabytes costs about as
 * much as copying them).  emgpu_sample_dbn_host recognises pinned output arrays and lets the copy engine write straight into them;
 * pageable arrays go through the library's own pinned staging buffers and a few host threads (below). */
int emgpu_host_alloc(emgpu_ctx *ctx, uint64_t bytes, void **out);
int emgpu_host_free(emgpu_ctx *ctx, void *p);   /* back to the pool; emgpu_ctx_trim releases the pool's free blocks */

/* Phases of the last emgpu_sample_dbn_host, emgpu_sample_uncor_host, emgpu_sample_text_host or emgpu_tracks_text_host call on this ctx (each call is a pipeline: chunk k's kernel runs
 * while chunk k-1 crosses PCIe and chunk k-2 is copied from staging into the caller's arrays, so the phases overlap and do not add up to
 * total_ms). */
typedef struct {
    double total_ms;        /* wall time of the call                                                                    */
    double kernel_ms;       /* sum of the chunks' launch durations (HIP events on the launch stream)                    */
    double d2h_ms;          /* sum of the chunks' copy durations (HIP events on the copy stream)                        */
    double scatter_ms;      /* host wall time spent copying staging -> caller arrays (0 for pinned outputs)             */
    int64_t bytes_d2h;      /* bytes that crossed PCIe                                                                  */
    int64_t event_rows;     /* rows of the event lists copied (the lists are packed on the device first)               */
    int32_t chunks, chunk_n;
    int32_t threads;        /* host threads of the scatter                                                              */
    int32_t direct;         /* 1: every large output was pinned memory (no staging)                                    */
} emgpu_host_stats_t;
int emgpu_host_stats(const emgpu_ctx *ctx, emgpu_host_stats_t *out);

/* ------------------------------------------------------------------------------------------------
 * One batch, several models / several devices.  The reference shards only by running em_sample in
 * a parfor over model files (RUN_1_emsample.m:13,24-47) and loops over samples serially
 * (UncorEncounterModel.m:244); trajectories are independent and every RNG slot is keyed by the GLOBAL
 * sample index, so any split gives the same trajectories.
 * ---------------------------------------------------------------------------------------------- */

/* The contiguous block [*lo, *hi) of `rank` when n_total indices are split over `world` parts (the
 * first n_total % world parts get one extra): the split every sharded entry point below uses. */
int emgpu_shard_range(int64_t n_total, int32_t rank, int32_t world, int64_t *lo, int64_t *hi);
int emgpu_device_count(int32_t *count);

/* Mixed-model batch (BASELINE.json configs[3]): block b samples trajectories
 * [first_index, first_index + n) (global indices) from models[model] into columns
 * out->col_offset + (first_index - p->first_index) + [0, n) of ONE shared trace whose trajectory
 * dimension is out->ld (0 => p->n).  p->n / p->first_index describe the range the trace covers;
 * every block must lie inside it.  All models must agree in n_initial and n_dyn (the trace shape).
 * One launch per block on the ctx stream; device pointers; asynchronous. */
typedef struct {
    int32_t model, _pad;
    uint64_t first_index;
    int64_t n;
} emgpu_block;
int emgpu_sample_dbn_blocks_device(emgpu_ctx *ctx, const emgpu_model *const *models, int32_t n_models,
                                   const emgpu_sample_params *p, const emgpu_block *blocks, int32_t n_blocks,
                                   const emgpu_sample_out *out);
/* The blocks of the equal-contiguous-block assignment "model m owns emgpu_shard_range(n_total, m,
 * n_models)" that intersect [lo, hi) (one rank's share): writes at most n_models entries, returns the count. */
int32_t emgpu_mixed_blocks(int64_t n_total, int32_t n_models, int64_t lo, int64_t hi, emgpu_block *blocks);

/* One call, several devices (one host thread + one HIP stream per device inside a
 * call): [p->first_index, p->first_index + p->n) is split with emgpu_shard_range over the n_ctx
 * contexts (each bound to its own device -- or to the same one, which only adds streams).
 *   _multi_host:   HOST pointers in `out` dimensioned for all p->n trajectories; synchronous; deferred
 *                  errors (rejection / event cap) are returned.  What a single-threaded MATLAB / Python
 *                  caller uses to drive 8 GPUs.
 *   _multi_device: outs[d] holds DEVICE pointers on ctx d's device for ITS shard only (ld / col_offset
 *                  as above, relative to the shard); asynchronous: emgpu_ctx_sync each ctx afterwards. */
int emgpu_sample_dbn_multi_host(emgpu_ctx *const *ctxs, int32_t n_ctx, const emgpu_model *m,
                                const emgpu_sample_params *p, const emgpu_sample_out *out);
int emgpu_sample_dbn_multi_device(emgpu_ctx *const *ctxs, int32_t n_ctx, const emgpu_model *m,
                                  const emgpu_sample_params *p, const emgpu_sample_out *outs);

/* bn_sample(G,r,N,alpha,num_samples,start,order) (bn_sample.m:1) on the initial network with an
 * optional dediscretize + rejection stage = the geometry draw of @CorTerminalModel/sample.m:29-77.
 * out_bin [n_initial][n] uint8, out_val [n_initial][n] float (device or host per the suffix). */
typedef struct {
    uint64_t seed, first_index;
    int64_t n;
    uint32_t flags;          /* EMGPU_FLAG_NO_DEDISC => plain bn_sample                           */
    int32_t max_attempts;
    const double *bounds_sample; /* n_initial x 2 row-major or NULL (sample.m:45-53)              */
    int32_t idx_own_speed, idx_int_speed; /* 1-based; 0 = no speed test (sample.m:64-70)          */
    double min_vel1, max_vel1, min_vel2, max_vel2;
    const int32_t *start;    /* optional start grid [n][n_initial] and per-sample log-weights [n]: as in emgpu_sample_params /
                                emgpu_sample_out -- InitStartTerminal.m:57-90 builds such a grid and RUN_terminal.m:33-50 loops over its 18
                                rows with one .sample call each; here the grid is ONE launch (device pointers for _device, host for _host) */
    double *log_weight;
} emgpu_bn_params;
int emgpu_sample_bn_device(emgpu_ctx *ctx, const emgpu_model *m, const emgpu_bn_params *p,
                           uint8_t *out_bin, float *out_val, int32_t *attempts);
int emgpu_sample_bn_host(emgpu_ctx *ctx, const emgpu_model *m, const emgpu_bn_params *p,
                         uint8_t *out_bin, float *out_val, int32_t *attempts);

/* ------------------------------------------------------------------------------------------------
 * Terminal trajectory propagation: replaces PropagateTrajectory (@CorTerminalModel/createEncounter.m:
 * 93-265) for both aircraft and both directions of n encounters (createEncounter.m:52-72); em-core's
 * local_smooth (:88-89) only as the stand-in of EMGPU_FLAG_LOCAL_SMOOTH.  models[]: trajectory models with the 6 initial variables
 * {intent, distance, bearing, heading, altitude, speed} and 3 dynamic ones, all of the same shapes and
 * boundaries; the caller has applied setTransitionPriors(...,1) (createEncounter.m:129) through
 * emgpu_model_set_transition_stay_prior.
 *   geo      [n][12] f64: x0_nm y0_nm z0_ft v0_ft_s heading0_deg intent for aircraft 1, then 2
 *            (createEncounter.m:41-49)
 *   model_of [4n] i32: index into models[] for track 4e + role, role = 2*(aircraft-1) + (backward)
 *   traj     [2n][W][5] f32: TRACK-MAJOR -- the joined, time-ordered track of aircraft 2e + (aircraft-1), i.e. what
 *            createEncounter.m:74-84 builds ([fwd, bck(1, 2:end)] sorted by t_s): row C+t holds second t (t < 0: the backward
 *            track), fields x_nm y_nm z_ft heading_deg v_ft_s (createEncounter.m:162-167); t_s is the row number minus C and is
 *            not stored.  C = EMGPU_TERMINAL_T0_ROW(cap) (cap rounded up to a multiple of 8: eight rows are 160 bytes, so the pieces
 *            a wave writes start on 32-byte boundaries), W = EMGPU_TERMINAL_BLOCK_ROWS(cap) = 2 C.
 *            Only rows C-(rows_bck-1) .. C+(rows_fwd-1) are written; the rest of the block is left untouched.
 *            (Rounds 1-3 wrote six row-synchronous planes [6][cap][4n]; a lane now starts its next track the moment its own ends, so
 *            the lanes of a wave are at unrelated rows and the output is by track.)
 *   rows     [4n] i32: seconds of track 4e + role, its t = 0 row included (<= tmax_s + 2); negative => cap / resample cap exceeded
 * ---------------------------------------------------------------------------------------------- */
#define EMGPU_TERMINAL_T0_ROW(cap) (((cap) + 7) & ~7)
#define EMGPU_TERMINAL_BLOCK_ROWS(cap) (2 * EMGPU_TERMINAL_T0_ROW(cap))
typedef struct {
    uint64_t seed, first_index;
    int64_t n;                   /* < 2^29 encounters per call                                      */
    double tmax_s;               /* 120 in @CorTerminalModel/track.m:33                            */
    int32_t max_resample, cap;   /* inner re-draw cap (reference: unbounded); rows per direction   */
    double dyn_limits[2][5];     /* per aircraft: minVel_ft_s maxVel_ft_s maxTurnRate_deg_s
                                    maxAltitude_ft maxVertRate_ft_s (getDynamicLimits.m:15-62)     */
    uint32_t flags, _pad;        /* EMGPU_FLAG_LOCAL_SMOOTH: the joined tracks' v_ft_s and z_ft are smoothed in place (:88-89)  */
} emgpu_term_params;
int emgpu_propagate_terminal_device(emgpu_ctx *ctx, const emgpu_model *const *models, int32_t n_models,
                                    const emgpu_term_params *p, const double *geo, const int32_t *model_of,
                                    float *traj, int32_t *rows);
int emgpu_propagate_terminal_host(emgpu_ctx *ctx, const emgpu_model *const *models, int32_t n_models,
                                  const emgpu_term_params *p, const double *geo, const int32_t *model_of,
                                  float *traj, int32_t *rows);

/* CorTerminalModel.sample + createEncounter for n encounters in one call, everything device-resident (RUN_terminal.m:39-44 without the
 * filters of track.m): the geometry draw of @CorTerminalModel/sample.m:29-77 (bn_sample + dediscretize + box / speed rejection), the
 * inputs of createEncounter.m:21-49 (x0 y0 from distance and bearing, the trajectory model of each of the four tracks) and
 * PropagateTrajectory x 4 (createEncounter.m:52-72), three launches on the ctx stream, asynchronous (emgpu_ctx_sync reports a geometry
 * rejection cap or a re-draw cap).  geom_model: the 15-variable geometry network; traj_models[10] in CorTerminalModel.m:84-100 order with
 * the stay prior set.  DEVICE pointers:
 *   geom_bin [n_i][n] u8 (may be NULL), geom_val [n_i][n] f32: the accepted geometry sample;  attempts [n] i32 (may be NULL)
 *   geo [n][12] f64, model_of [4n] i32: the inputs of createEncounter (outputs here);  traj, rows: as emgpu_propagate_terminal_device
 * EMGPU_FLAG_LOCAL_SMOOTH with EMGPU_TERMINAL_BLOCK_ROWS(cap) > 256 is refused with EMGPU_ERR_UNSUPPORTED before anything is launched, like
 * emgpu_propagate_terminal_device refuses it (it used to run three launches and fail in the smoother's launcher with EMGPU_ERR_HIP). */
typedef struct {
    uint64_t seed, first_index;
    int64_t n;
    double tmax_s;
    int32_t max_resample, cap;
    double dyn_limits[2][5];
    int32_t max_attempts;            /* cap of the geometry rejection loop (sample.m:32; unbounded in the reference) */
    uint32_t flags;                  /* EMGPU_FLAG_LOCAL_SMOOTH                                              */
    const double *bounds_sample;     /* HOST pointer: n_initial x 2 row-major or NULL (sample.m:45-53)       */
    int32_t idx[12];                 /* 1-based geometry variable ids: own {distance bearing alt speed heading intent}, then int */
} emgpu_tsample_params;
int emgpu_sample_terminal_device(emgpu_ctx *ctx, const emgpu_model *geom_model, const emgpu_model *const *traj_models, int32_t n_traj_models,
                                 const emgpu_tsample_params *p, uint8_t *geom_bin, float *geom_val, double *geo, int32_t *model_of,
                                 float *traj, int32_t *rows, int32_t *attempts);

/* sample2track.m:183-237 -- the 1 Hz dead-reckoning track `sample2track` builds from the em_sample
 * files, and its rejection tests, for n trajectories in one launch:
 *   z += vertrate*ur_vertrate; speed += acc*ur_speed; heading += turnrate*ur_heading;
 *   x += speed*cosd(heading); y += speed*sind(heading)            (:201-212, previous speed/heading)
 * flags[i] bit 0: some z < 0 (CFIT, :234-237); bit 1: some speed <= min or >= max (:240); the
 * reference keeps a track iff flags[i] == 0 (:243).  speed, min_speed, max_speed are in model
 * units (knots) and are converted with ur_speed like :126-139.
 * _device: consumes the sampler's device output in place -- alt0/speed0 = rows of init_val,
 *   dyn_val = the time-blocked dense trace with nd rows per block, slot_* = the rows holding
 *   \dot h, \dot v, \dot\psi; xyz f64 [T+1][3][n], speed_minmax f64 [2][n] (either may be NULL).
 * _host: values as parsed from initial.txt / transition.txt: updates [n][T][3] = vertical rate,
 *   acceleration, turn rate; xyz [n][T+1][3], speed_minmax [n][2] (either may be NULL). */
typedef struct {
    int64_t n;
    int32_t T;                 /* transition rows per id */
    int32_t nd;                /* _device: rows per dense block */
    int32_t slot_vertrate, slot_acc, slot_turnrate;
    int32_t reserved;
    double ur_speed, ur_vertrate, ur_heading;
    double min_speed, max_speed;
} emgpu_track_params;
int emgpu_sample2track_device(emgpu_ctx *ctx, const emgpu_track_params *p, const float *alt0, const float *speed0,
                              const float *dyn_val, double *xyz, uint8_t *flags, double *speed_minmax);
int emgpu_sample2track_host(emgpu_ctx *ctx, const emgpu_track_params *p, const double *alt0, const double *speed0,
                            const double *updates, double *xyz, uint8_t *flags, double *speed_minmax);

/* ------------------------------------------------------------------------------------------------
 * sample2track's files read and written on the device (sample2track.m:69-72 readtable, :192-193 the rows of an id, :183-243 the track,
 * :274-279 the CSV file): what legacy.sample2track(text="device") is made of.
 *
 * emgpu_parse_table_host -- a numeric text table (the bytes of initial.txt / transition.txt behind their header line) -> out [rows][ncol] f64,
 * row-major, rows in file order (:69-72).  Lines end in "\n" (a "\r" in front of it is dropped; the last line may lack it); lines that hold
 * only spaces and tabs are skipped; numbers are separated by runs of spaces or tabs, and separators may trail.  A number is
 *     [+-]? (digits [. digits?] | . digits) ([eE] [+-]? digits)?     or     [+-]? (nan | inf | infinity), in any letter case.
 * Narrower than numpy.loadtxt on purpose: no '#' comments, no hex, no '_'.  Anything else, or a line that does not hold ncol numbers, is
 * EMGPU_ERR_PARSE, and emgpu_last_error names the 1-based line (of `text`) of the first such line.  EXACT: every value is the correctly rounded
 * double of its decimal text (strtod), the sign of -0 included.  On the device: with w the mantissa's digits as an integer and d the decimal
 * exponent (the exponent field minus the digits behind the point), w < 2^53 and |d| <= 22 give w * 10^d or w / 10^-d in one IEEE operation;
 * every other number is a HARD token, finished by the host with strtod (*hard_tokens: how many; none in a file em_sample wrote from the shipped
 * models: "%g" prints six digits, and their values lie between 10^-4 and 10^6).  The text goes up in chunks cut at a newline
 * (EMGPU_HOST_CHUNK_MB), one chunk's copy behind the parse of the one before; pinned text (emgpu_host_alloc) without staging.
 * EMGPU_ERR_EVENT_CAP when rows_cap rows do not hold the table (*rows: exact).
 *
 * emgpu_format_f0_host -- "%0.0f" of n doubles by the device function the CSV rows use, one after the other: value i is
 * out[offsets[i] .. offsets[i + 1]) (offsets: n + 1 entries; capacity protocol of emgpu_format_g_host).  For |v| < 2^63: the digits of v rounded
 * to the nearest integer, ties to even, behind a '-' when v's sign bit is set ("-0" for -0.3).  Other values have length 0: the device does
 * not format them.
 *
 * emgpu_tracks_text_host -- the transition text is parsed as above and stays on the device; runs of equal ids in its column 0 are found
 * without a sort and each of the p->n wanted ids is matched to its run (an id without rows: a track of length 0; the same id twice: the same
 * rows twice; ids are compared as doubles); k_sample2track_table integrates every track from its rows where they lie (same operations as
 * emgpu_sample2track_host: bit-equal results), and for every track with flags 0 the bytes of its file are formatted on the device:
 * "time_s,x_ft,y_ft,z_ft\n", then "%i,%0.0f,%0.0f,%0.0f\n" for t = 0 .. lengths[i] (:277-278).  When an id owns more than one run (interleaved
 * rows) the rows of an id are selected on the host by a stable sort of the id column, as the reference's logical index does, and
 * totals[4] = 1; the results are the same.  p: the unit ratios and the speed limits (p->T is not used: every track has its own length).
 *   totals[0] bytes of the CSV text   [1] rows of the transition table   [2] hard tokens   [3] accepted tracks left to the caller's formatter
 *   (a coordinate that is not finite, or 2^63 and more in magnitude: offsets[i + 1] == offsets[i] although flags[i] == 0; ask for xyz)
 *   [4] 1: the ids were not contiguous
 * csv == NULL with offsets: the files are measured, not written; offsets == NULL: no CSV work at all.  EMGPU_ERR_EVENT_CAP when csv_cap bytes
 * do not hold the text, or xyz_cap rows the positions (every other output is complete, totals exact; a retry with that room gives the same
 * bytes).  emgpu_csv_bound(n, rows) = 22 n + 74 rows always suffices for n files with `rows` position rows in all (a line: 10 characters of
 * "%i", three times a sign and 19 digits, three commas, the newline); real files are near 20 bytes per row.  Host memory: the transition text
 * and the CSV text; files larger than memory are out of scope.  emgpu_host_stats describes the call.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    const char *text;          /* the transition table's rows (behind the header line)                                              */
    int64_t nbytes;
    int32_t ncol;              /* numbers per row; column 0 is the id                                                               */
    int32_t col_vertrate, col_acc, col_turnrate;   /* 0-based columns of the three updates (:131-133)                              */
    const double *id;          /* [n] per wanted track: its id, initial altitude (ft) and speed (model units), from the initial table */
    const double *alt0;
    const double *speed0;
} emgpu_tracks_text_in;
typedef struct {
    uint8_t *flags;            /* [n] bit 0 CFIT, bit 1 speed (as emgpu_sample2track_host)                                         */
    double *speed_minmax;      /* [n][2], or NULL                                                                                   */
    int32_t *lengths;          /* [n] transition rows of track i, or NULL                                                           */
    char *csv;                 /* [csv_cap] the files' bytes, track after track, or NULL                                            */
    int64_t csv_cap;
    uint64_t *offsets;         /* [n + 1] file i is csv[offsets[i] .. offsets[i + 1]); NULL: no CSV work                            */
    int64_t *totals;           /* [5] see above                                                                                     */
    double *xyz;               /* [xyz_cap][3] positions, track after track, lengths[i] + 1 rows each, or NULL                       */
    int64_t xyz_cap;
    double *phase_ms;          /* [6] upload, parse kernels, grouping + track kernels, CSV kernels, download, host work; or NULL    */
} emgpu_tracks_text_out;
int emgpu_parse_table_host(emgpu_ctx *ctx, const char *text, int64_t nbytes, int32_t ncol, double *out, int64_t rows_cap, int64_t *rows,
                           uint64_t *hard_tokens);
int emgpu_format_f0_host(emgpu_ctx *ctx, const double *x, int64_t n, char *out, int64_t cap, uint64_t *offsets);
int64_t emgpu_csv_bound(int64_t n, int64_t rows);
int emgpu_tracks_text_host(emgpu_ctx *ctx, const emgpu_track_params *p, const emgpu_tracks_text_in *in, const emgpu_tracks_text_out *out);

/* ------------------------------------------------------------------------------------------------
 * UncorEncounterModel.track (@UncorEncounterModel/UncorEncounterModel.m:318-471) with coordSys 'NEU': per trajectory
 * sample -> dynamics -> the rejection tests of :462-470 against @UncorEncounterModel/getDynamicLimits.m:1-130, retried
 * with the next seed (:424-428: attempt j of EVERY trajectory uses the Philox key seed + j; the trajectory is told apart by
 * its global index).  Rounds: round j samples the trajectories still rejected (round 0: the whole contiguous range on the
 * fast kernels, later rounds an index list), integrates and tests them on the device; only a counter crosses PCIe per round.
 * DYNAMICS: the reference calls em-core's run_dynamics_fast / computeVerticalRate, which it does not vendor.  The point-mass
 * model used instead (dt 0.1 s, first-order pitch / bank response limited by dyn(5:6); "dynamics unpinned") is stated in
 * HISTORY.md section 10 and at the top of csrc/emgpu_kernels_utrack.hip.  The 'geodetic' branch (:480-540: DEM, obstacles, placeTrack) is out of scope.
 *   tracks   [n][S][8] f64: time_s north_ft east_ft up_ft speed_ft_s phi_rad theta_rad psi_rad, S = 10*T/record_stride + 1
 *   limits   [n][3] f64: minVel_ft_s maxVel_ft_s maxVertRate_ft_s of the accepted attempt (getDynamicLimits.m:129-133)
 *   attempts [n] i32: attempts used (>= 1); -1 => max_track_attempts reached (the call then returns EMGPU_ERR_REJECT_CAP)
 * Any output may be NULL.  _host: host pointers; _device: device pointers.  Both synchronise the ctx stream.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    uint64_t seed, first_index;  /* 'initialSeed' (:327)                                               */
    int64_t n;
    int32_t sample_time;         /* seconds                                                            */
    uint32_t flags;              /* EMGPU_FLAG_QUANTIZE500                                             */
    int32_t max_track_attempts;  /* cap of the outer while (:421; unbounded in the reference)          */
    int32_t max_attempts;        /* cap of .sample's own loop (:248)                                   */
    int32_t idx_G, idx_A, idx_L, idx_v, idx_dv, idx_dh, idx_dpsi; /* 1-based variable ids (:385-391), 0 = absent */
    int32_t is_rotorcraft;       /* self.isRotorcraft (:181-185)                                       */
    int32_t record_stride;       /* keep every record_stride-th 0.1 s step: 1 = the reference's timetable, 10 = 1 Hz */
    int32_t _pad;
} emgpu_utrack_params;
int emgpu_track_uncor_host(emgpu_ctx *ctx, const emgpu_model *m, const emgpu_utrack_params *p,
                           double *tracks, double *limits, int32_t *attempts);
int emgpu_track_uncor_device(emgpu_ctx *ctx, const emgpu_model *m, const emgpu_utrack_params *p,
                             double *tracks, double *limits, int32_t *attempts);
/* The same with a start GRID: start [p->n][n_initial] as emgpu_sample_params.start (a HOST pointer for _host, a DEVICE pointer for _device;
 * NULL: exactly the functions above).  Every attempt of trajectory i is drawn under row i: round 0 reads row i for lane i, a later round
 * reads the rows of the trajectories it redraws.  Keys and indices are unchanged: attempt j of trajectory i has key seed + j and global index
 * first_index + i.  A fast-branch model's sampler runs on the +start instance of k_uncor_fast_idx in every round; any other model's round 0
 * on the +start instance of k_dbn_step2 and its later rounds (index lists) on the general kernel.  EMGPU_ERR_PRESET as for
 * emgpu_sample_dbn_*; the weights: emgpu_start_grid_log_weight. */
int emgpu_track_uncor_grid_host(emgpu_ctx *ctx, const emgpu_model *m, const emgpu_utrack_params *p, const int32_t *start,
                                double *tracks, double *limits, int32_t *attempts);
int emgpu_track_uncor_grid_device(emgpu_ctx *ctx, const emgpu_model *m, const emgpu_utrack_params *p, const int32_t *start,
                                  double *tracks, double *limits, int32_t *attempts);
/* getDynamicLimits.m:1-130 for one trajectory on the host (what the table of the track kernel holds): initial = the
 * n_initial sampled values (bins for categorical variables), the extrema over the 10 Hz result in ft and ft/s. */
int emgpu_uncor_dynamic_limits(const emgpu_model *m, const emgpu_utrack_params *vars, const double *initial,
                               double up_min_ft, double up_max_ft, double speed_min_ft_s, double speed_max_ft_s, double out[3]);

/* ------------------------------------------------------------------------------------------------
 * CorTerminalModel.track (@CorTerminalModel/track.m:45-150): per encounter, loop { geometry sample (sample.m) ->
 * createEncounter -> the filters of :62-145 (CPA within +-10 s, overlap >= minEncTime_s, runway proximity, vertical intent,
 * CheckDynamicLimits with CheckCumTurn: CorTerminalModel.m:117-316) } until one passes.  Rounds on the device like
 * emgpu_track_uncor_*: attempt j of every encounter uses the Philox key seed + j (the reference continues one MT19937 stream,
 * track.m:36-58) and the encounter's global index; a track that hits the re-draw cap voids its attempt.
 * em-core's computeVerticalRate / computeHeadingRate (not vendored) are forward differences of the 1 s samples; `isClimb`
 * (track.m:122,134, undefined in the reference) is read as is_climb; local_smooth (createEncounter.m:88-89) is the flagged stand-in of
 * EMGPU_FLAG_LOCAL_SMOOTH (off: the filters read the unsmoothed tracks).
 *   geom_model   the 15-variable geometry network; traj_models[10] in CorTerminalModel.m:84-100 order with the stay prior set
 *   sample   [n][n_initial(geom)] f64   the accepted geometry sample (out_results(ii).sample, track.m:158)
 *   traj     [n][2][cap2][6] f64        ownship / intruder, time-ordered: t_s x_nm y_nm z_ft heading_deg v_ft_s (createEncounter.m:74-84)
 *   len      [n][2] i32 rows of each;  meta [n][4] f64: tcpa_s hmd_ft vmd_ft enc_time_s (:79, :90);  attempts [n] i32 (-1: cap)
 * Host pointers; any output may be NULL.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    uint64_t seed, first_index;      /* 'initialSeed' (track.m:11)                                         */
    int64_t n;
    double tmax_s;                   /* 120 (track.m:33)                                                   */
    int32_t max_resample;            /* re-draw cap inside PropagateTrajectory                             */
    int32_t max_track_attempts;      /* cap of the while of track.m:55 (unbounded in the reference)        */
    int32_t max_attempts;            /* cap of the geometry rejection loop (sample.m:32)                   */
    uint32_t flags;                  /* EMGPU_FLAG_LOCAL_SMOOTH: the filters read the smoothed tracks, like the reference's (:88-89) */
    double dyn_limits[2][5];         /* per aircraft: minVel maxVel maxTurnRate_deg_s maxAltitude maxVertRate (getDynamicLimits.m:15-62) */
    double max_cum_turn_deg[2], pitch_deg[2];
    double min_enc_time_s, thres_dist_ft, thres_alt_low_ft, thres_vertrate_ft_s;  /* track.m:14-17 */
    const double *bounds_sample;     /* n_initial x 2 row-major or NULL (sample.m:45-53)                   */
    int32_t idx[12];                 /* 1-based geometry variable ids: own {distance bearing alt speed heading intent}, then int */
} emgpu_ttrack_params;
int emgpu_track_terminal_host(emgpu_ctx *ctx, const emgpu_model *geom_model, const emgpu_model *const *traj_models, int32_t n_traj_models,
                              const emgpu_ttrack_params *p, double *sample, double *traj, int32_t cap2, int32_t *len,
                              double *meta, int32_t *attempts);

/* The two kernels emgpu_track_terminal_host runs behind the propagation, each on tracks of the caller's: what a test hands a track of its
 * choosing to.  The calls take no context and no model, like emgpu_miss_distance_device: hip_stream, the current device, DEVICE pointers,
 * asynchronous.  EMGPU_ERR_ARG / EMGPU_ERR_UNSUPPORTED before any device work; n == 0 (n2 == 0): EMGPU_OK without a launch.
 *
 * emgpu_filter_terminal_device -- k_terminal_filter once: the filters of track.m:79-145 on n encounters, one decision each.
 *   geo      [n][12] f64 as emgpu_propagate_terminal_device's; only the two intents (entries 5 and 11) are read
 *   tracks   [2n][EMGPU_TERMINAL_BLOCK_ROWS(cap)][5] f32, rows [4n] i32: as emgpu_propagate_terminal_device writes them.  Every rows entry
 *            must be <= cap (the kernel reads rows C-(rows_bck-1) .. C+(rows_fwd-1) of a block); an entry < 1 voids the attempt
 *   accepted [n] u8: 1 = every filter passed, else 0
 *   meta [n][4] f64, len [n][2] i32, traj [n][2][cap2][6] f64 as emgpu_track_terminal_host's (any may be NULL): written for ACCEPTED
 *            encounters only, a rejected encounter's entries are left as they were; traj holds the first min(len, cap2) rows of a track
 * cap outside 2..125 is EMGPU_ERR_UNSUPPORTED (CheckCumTurn keeps at most 248 heading differences per lane: emgpu_track_terminal_host's
 * tmax_s <= 122).
 *
 * emgpu_smooth_terminal_device -- k_terminal_smooth: v_ft_s and z_ft of n2 joined tracks ([n2][EMGPU_TERMINAL_BLOCK_ROWS(cap)][5], rows
 * [2 n2]: forward, backward per track) smoothed in place (EMGPU_FLAG_LOCAL_SMOOTH's stand-in); a track with a rows entry < 1 is left alone.
 * EMGPU_TERMINAL_BLOCK_ROWS(cap) > 256 is EMGPU_ERR_UNSUPPORTED. */
typedef struct {
    int64_t n;                       /* < 2^29 encounters                                                  */
    int32_t cap, cap2;               /* rows per direction of `tracks` (2..125); rows per track of `traj`  */
    double dyn_limits[2][5];         /* as emgpu_ttrack_params, and so are the rest                        */
    double max_cum_turn_deg[2], pitch_deg[2];
    double min_enc_time_s, thres_dist_ft, thres_alt_low_ft, thres_vertrate_ft_s;
} emgpu_tfilter_params;
int emgpu_filter_terminal_device(void *hip_stream, const emgpu_tfilter_params *p, const double *geo, const float *tracks, const int32_t *rows,
                                 uint8_t *accepted, double *meta, int32_t *len, double *traj);
int emgpu_smooth_terminal_device(void *hip_stream, int64_t n2, int32_t cap, float *tracks, const int32_t *rows);

/* Introspection for benchmarks/tests: name of the kernel variant the last *_device call used and
 * the algorithmic output bytes per trajectory of that call (5*n_i + 5*T*n_d for dense output). */
const char *emgpu_last_kernel_name(const emgpu_ctx *ctx);
/* Kernel launches the last emgpu_sample_dbn_*_device call on this ctx issued (a mixed batch whose models share a kernel
 * instance is ONE launch with the model id per workgroup; RUN_1_emsample.m:13,24-47 is the reference's per-file loop). */
int32_t emgpu_last_launch_count(const emgpu_ctx *ctx);

/* Test hooks into the plan compiler (host only): the u32 quantile thresholds of one CPT column
 * (r weights -> r-1 thresholds; bin = 1 + #{k : min(x, 2^32-2) >= out[k]} reproduces
 * select_random.m:17-20 for u = (min(x, 2^32-2) + 0.5) * 2^-32) and the resample hit threshold
 * (hit <=> min(x, 2^32-2) < R reproduces `u < rate`, resample_events.m:24). */
int emgpu_debug_column_thresholds(const double *weights, int32_t r, uint32_t *out);
uint32_t emgpu_debug_bernoulli_threshold(double rate);
/* Column `col` (0-based, asub2ind order) of the k-th dynamic variable's transition table as the
 * kernels read it: the r-1 quantile thresholds (thr, room for 15) and the compacted form -- *meff
 * distinct thresholds (cthr, room for 7) plus the nibble map, bin = (map >> 4n) & 15 with
 * n = #{t < meff : min(x, 2^32-2) >= cthr[t]}.  *meff = 0: this variable is not compacted.
 * k counts the temporal_map rows in plan order; *tvar receives the 1-based transition variable. */
int emgpu_debug_dynamic_column(const emgpu_model *m, int32_t k, int64_t col, int32_t *tvar, int32_t *r, int64_t *q,
                               uint32_t *thr, int32_t *meff, uint32_t *cthr, uint32_t *map);
/* The same column in the padded form the per-timestep kernel loads: *width = 4 words {t0, t1, t2, map} or
 * 8 words {t0..t5, map_lo, map_hi} (0: the variable has no padded table); unused thresholds repeat the last real one (2^32-1 if none);
 * the map is a byte table: entry b = 1-based bin when b of the 3 (6) thresholds did NOT fire. */
int emgpu_debug_padded_column(const emgpu_model *m, int32_t k, int64_t col, int32_t *width, uint32_t *words);
/* The same column in the packed-compare form of the per-timestep kernel (4 words): {T'0 | T'1 << 16, T'2 | T'3 << 16, T'4 | T'5 << 16,
 * nibble map}.  With x_h the draw's high halfword and d_t = min(sat16(x_h - T'_t), 2): the sum over t is 2 * (thresholds fired),
 * odd exactly when the draw's low halfword decides some compare; nibble (sum / 2) of the map is the 1-based bin
 * (select_random.m:17-20 on the high halfword alone; x_h = 0 is always referred to the full 32-bit compare).
 * A variable whose padded width is 4 (at most 3 thresholds) holds the PLAIN form instead: {H0, H1, H2, map}, H_t = the threshold's high
 * half (0x10000: no such threshold); with a_t = H_t - x_h: a_t < 0 <=> threshold t fired, a_t == 0 <=> the low halfword decides; the
 * 1-based bin is (map >> 7 * fired) & 15. */
int emgpu_debug_pk_column(const emgpu_model *m, int32_t k, int64_t col, uint32_t *words);

/* Test hook: the point-mass dynamics kernel of emgpu_track_uncor_* (k_uncor_track) on caller-given inputs, without sampling or limits.
 *   init [n][5] f32: L (ft), v (kt), \dot v (kt/s), \dot h (ft/min), \dot psi (deg/s) -- the sampled values of UncorEncounterModel.m:434-446
 *   controls [n][T][3] f32: \dot h (ft/min), \dot psi (deg/s), \dot v (kt/s) active during each second (events2controls.m:16-27)
 *   dyn[6]: v_low v_high dh_min dh_max q_max r_max (:414);  literal != 0: the literal step even where the reduced one applies
 *   tracks [n][10 T / record_stride + 1][8] f64 as emgpu_track_uncor_host.  Host pointers. */
int emgpu_debug_uncor_dynamics_host(emgpu_ctx *ctx, int64_t n, int32_t T, int32_t record_stride, int32_t literal, const double dyn[6],
                                    const float *init, const float *controls, double *tracks);

/* Test hook: one of the track kernels' hand-written device math functions (emgpu_device.h, emgpu_device_math.h) evaluated on x[0..n), one
 * lane per element: out0[i] (and out1[i]) = fn(x[i]).  The sin/cos pairs (fn <= EMGPU_MATH_UT_SINCOS_SK) write the sine to out0 and the
 * cosine to out1; out1 may be NULL and is ignored by the one-result functions.  Device pointers, no context: it runs on the stream given
 * and the calling thread's current device, asynchronously.  EMGPU_ERR_ARG before any device work: an unknown fn, n < 0 or n > 2^32, NULL x
 * or out0, a pointer that is not 8-byte aligned.  n == 0: EMGPU_OK without a launch.  What each function computes, its domain and what it
 * does outside: its header comment; the measured errors: DESIGN.md section 39. */
#define EMGPU_MATH_SINCOS_SMALL 0        /* sincos_small<false>  (radians, |x| <= pi/4)                     */
#define EMGPU_MATH_SINCOS_SMALL_SK 1     /* sincos_small<true>   (coefficients as scalar operands)          */
#define EMGPU_MATH_SINCOSD_SMALL 2       /* sincosd_small        (degrees; k_sample2track*)                 */
#define EMGPU_MATH_T_SINCOSD 3           /* t_sincosd            (degrees; k_terminal_propagate's loop)     */
#define EMGPU_MATH_F_SINCOSD 4           /* f_sincosd            (degrees; k_terminal_geo)                  */
#define EMGPU_MATH_UT_SINCOS 5           /* ut_sincos<false>     (radians; k_uncor_track)                   */
#define EMGPU_MATH_UT_SINCOS_SK 6        /* ut_sincos<true>                                                 */
#define EMGPU_MATH_UT_ATAN 7             /* ut_atan<false>                                                  */
#define EMGPU_MATH_UT_ATAN_SK 8          /* ut_atan<true>                                                   */
#define EMGPU_MATH_UT_ASIN_SMALL 9       /* ut_asin_small<false> (|x| < 0.5)                                */
#define EMGPU_MATH_UT_ASIN_SMALL_SK 10   /* ut_asin_small<true>                                             */
#define EMGPU_MATH_UT_RCP 11             /* ut_rcp               (1 / x)                                    */
#define EMGPU_MATH_ROUND500 12           /* round500             (UncorEncounterModel.m:196)                */
int emgpu_debug_device_math(void *hip_stream, int32_t fn, int64_t n, const double *x, double *out0, double *out1);

/* Measuring builds of k_terminal_propagate (-DEMGPU_TERM_COUNTERS; tools/term_counters.py): the lanes that took each path of the loop
 * since the last call (24 counters, cleared by the call).  Returns 1, or 0 in a normal build (out untouched). */
int emgpu_debug_terminal_counters(emgpu_ctx *ctx, uint64_t *out, int32_t n);

/* Which dynamic variables are parents of which (t+1) node, in plan order k = 0..n_dyn-1: bit 4k+q of cur_mask = the time-t
 * node of dynamic variable q is a parent of k's (t+1) node; of new_mask = its (t+1) node is (dbn_sample.m:65-93: the
 * dependent branch; q < k by the topological order).  The per-timestep kernel picks its instance by these masks. */
int emgpu_debug_parent_masks(const emgpu_model *m, uint32_t *cur_mask, uint32_t *new_mask);

/* Which kernel instance emgpu_sample_dbn_device / _host would run this call on: the name emgpu_last_kernel_name reports after it (the
 * instance, then "+rows-by-wave+events" / "+events" for an event list and "+start" for a start grid or log-weights), written to
 * name[0..cap).  Host only, no ctx: only WHICH pointers of p and out are null is read (p->start or out->log_weight: presets), never
 * what they point to.  EMGPU_ERR_ARG when the name does not fit cap. */
int emgpu_debug_kernel_choice(const emgpu_model *m, const emgpu_sample_params *p, const emgpu_sample_out *out, char *name, int32_t cap);

/* Host helpers that mirror small reference functions (used by the class layer and tests). */
int32_t emgpu_discretize_bayes(double x, const double *thresholds, int32_t n); /* discretize_bayes.m:14-22 */
int64_t emgpu_asub2ind(const int32_t *siz, const int32_t *x, int32_t n);       /* asub2ind.m:13-14        */

#ifdef __cplusplus
}
#endif
#endif /* EMGPU_H */
