// emgpu_launch.h -- host-callable launchers implemented in the .hip translation units.
#pragma once
#include <hip/hip_runtime.h>

#include "emgpu_dispatch.h"
#include "emgpu_plan.h"

namespace emgpu {
// The sampler's kernels: c = choose_dbn(P, A, presets != nullptr) names the instance, the launcher launches it.
hipError_t launch_dbn_generic(const EmgpuPlan &P, const EmgpuRun &A, const DbnChoice &c, const EmgpuPresets *presets, hipStream_t s);
hipError_t launch_uncor_fast(const EmgpuPlan &P, const EmgpuRun &A, const DbnChoice &c, const EmgpuPresets *presets, hipStream_t s);
hipError_t launch_dbn_step2(const EmgpuPlan &P, const EmgpuRun &A, const DbnChoice &c, const EmgpuPresets *presets, hipStream_t s);
hipError_t launch_dbn_step(const EmgpuPlan &P, const EmgpuRun &A, const DbnChoice &c, hipStream_t s);
hipError_t launch_bn(const EmgpuPlan &P, const EmgpuBnRun &A, hipStream_t s, const char **name);
// Mixed-model batch in one launch: nb <= EMGPU_MAX_MIXED blocks whose choice is the dense fast kernel at the same shape
// (uncor_fast_mixed_name).  A model's plan lives in device memory (plan_f_bytes() bytes filled by plan_f_fill on the host, then uploaded).
size_t plan_f_bytes();
void plan_f_fill(const EmgpuPlan &P, void *host_buf);
hipError_t launch_uncor_fast_mixed(const EmgpuRun &A, int nb, const void *const *d_planf, const uint64_t *first, const int64_t *n, const int64_t *col,
                                   int shape, hipStream_t s);
hipError_t launch_terminal_propagate(const EmgpuPlan &P, const EmgpuTermRun &A, hipStream_t s, const char **name);
int terminal_debug_counters(unsigned long long *out, int n);   // -DEMGPU_TERM_COUNTERS builds: the loop's path counters (0: not such a build)
// createEncounter.m:88-89 through the stand-in of EMGPU_FLAG_LOCAL_SMOOTH: v_ft_s (5 s) and z_ft (15 s) of n2 joined tracks, in place
hipError_t launch_terminal_smooth(float *traj, const int32_t *rows, int64_t n2, int32_t cap, hipStream_t s);
hipError_t launch_terminal_geo(const EmgpuTGeoRun &A, hipStream_t s);
hipError_t launch_terminal_filter(const EmgpuTFilterRun &A, hipStream_t s, const char **name);
hipError_t launch_uncor_track(const EmgpuUTrackRun &A, hipStream_t s, const char **name, int force_literal = 0);
// rejected lanes of a round -> the next round's index lists, in lane order; count: compact_scratch_words(n) words of device
// scratch, count[0] receives the number of rejected lanes
size_t compact_scratch_words(int64_t n);
hipError_t launch_compact_rejected(int64_t n, uint64_t first_index, const uint8_t *accepted, const uint64_t *gidx_in, const int64_t *slot_in,
                                   uint64_t *gidx_out, int64_t *slot_out, uint32_t *count, hipStream_t s);
// event lists [n][cap] -> one packed run of rows (emgpu_kernels_pack.hip): scratch = pack_scratch_words(n) words, of which the first two
// receive the total row count (u64) and word 2 + b the first packed row of workgroup b's 256 lists; packed: room for n x cap rows
size_t pack_scratch_words(int64_t n);
hipError_t launch_pack_events(int64_t n, uint32_t cap, const uint32_t *cnt, const uint64_t *ev, uint32_t *scratch, uint64_t *packed, hipStream_t s);
// the first two steps of launch_pack_events alone: scratch receives the total of min(cnt[i], cap) (u64 in words 0-1) and, in word 2 + b, the
// exclusive prefix of workgroup b's 256 counts
hipError_t launch_scan_counts(int64_t n, uint32_t cap, const uint32_t *cnt, uint32_t *scratch, hipStream_t s);
// UncorEncounterModel.sample's outputs from a chunk's event lists [n][cap] (emgpu_kernels_format.hip), for emgpu_sample_uncor_host
struct EmgpuFormatRun {
    int64_t n;               // lists of the chunk
    uint32_t cap;            // rows per list in `ev`
    int32_t T, ni;           // sample_time, n_initial
    int64_t ld;              // trajectory dimension of init_val ([ni][ld])
    const uint32_t *ev_count;
    const uint64_t *ev;      // emgpu_event rows, list i at ev + i * cap
    const float *init_val;
    int32_t id_dh, id_dpsi, id_dv;   // 1-based variable ids of the control columns (UncorEncounterModel.m:291)
    uint32_t *ctrl_count;    // [n] out: rows with dt > 0
    uint32_t *ctrl_off;      // [n] out: first control row of list i within the chunk
    uint32_t *scratch;       // pack_scratch_words(n) words: words 0-1 receive the chunk's total control rows (u64)
    double *inits;           // [n][ni] out
    double *samples;         // [n][ni][T] out, or null
    double *controls;        // [rows][4] out, room for sum(min(ev_count, cap)) rows
};
hipError_t launch_format_uncor(const EmgpuFormatRun &F, hipStream_t s);
// em_sample's text rows from a chunk's dense trace (emgpu_kernels_text.hip), for emgpu_sample_text_host: em_sample.m:85-99
struct EmgpuTextRun {
    int64_t n;               // trajectories of the chunk
    int32_t T, ni, nd;       // sample_time, n_initial, n_dyn
    int64_t ld;              // trajectory dimension of init_val ([ni][ld]) and dyn_val ([G4][nd][ld][4])
    const float *init_val, *dyn_val;
    int64_t id_first;        // the id printed for trajectory 0 of the chunk (>= 0)
    uint32_t *cnt_i, *cnt_t; // [n] out: bytes of trajectory i's initial row / of its T transition rows
    uint32_t *scr_i, *scr_t; // pack_scratch_words(n) words each: words 0-1 receive the chunk's bytes (u64)
    char *text_i, *text_t;   // out: the rows, trajectory after trajectory; room for n * text_row_bound_initial(ni) / n * T * text_row_bound_transition(nd)
};
uint32_t text_row_bound_initial(int ni);      // 21 + 13 ni: "%d " of an id below 2^63, then ni values of at most 12 characters and what follows each
uint32_t text_row_bound_transition(int nd);   // 13 (2 + nd): id, second and nd values, each "%g" at most 12 characters, and what follows each
hipError_t launch_text_rows(const EmgpuTextRun &R, hipStream_t s);
// "%g" of n f32 values, one after the other: cnt [n], scratch pack_scratch_words(n) words (words 0-1: the bytes, u64), text: room for 12 n bytes,
// offsets [n]: base + the first byte of value i; paths[0] / paths[1] += the finite non-zero values formatted on the 64-bit / the multiword path
hipError_t launch_format_g(const float *x, int64_t n, uint32_t *cnt, uint32_t *scratch, char *text, uint64_t base, uint64_t *offsets,
                           unsigned long long *paths, hipStream_t s);
hipError_t launch_sample2track(const EmgpuTrackRun &A, bool dense, hipStream_t s, const char **name);

// ---- sample2track's files on the device (emgpu_tracks_text_host, emgpu_parse_table_host)
// One chunk of a numeric text table (emgpu_kernels_parse.hip): bytes [0, nbytes) begin at a line start and end behind a newline or at the end of
// the file.  `text` is 4-byte aligned and readable up to nbytes rounded up to a multiple of 4.
struct EmgpuHardToken { uint64_t pos; uint32_t off, _pad; };   // table element (row * ncol + column) and the token's first byte within the chunk
constexpr uint32_t kParseTile = 64;                            // bytes of text per lane of the counting passes
struct EmgpuParseRun {
    const uint8_t *text;
    uint32_t nbytes;
    int32_t ncol;
    uint32_t *cnt;             // [tiles] out: rows (lines holding more than separators) that begin in each tile of kParseTile bytes
    uint32_t *scratch;         // pack_scratch_words(tiles) words: words 0-1 receive the chunk's rows (u64)
    uint32_t rows;             // (launch_parse_rows) the chunk's rows
    double *table;             // [..][ncol] row-major; the chunk's first row is row_base
    int64_t row_base, table_rows;   // rows the table has room for: rows beyond are checked, not stored
    EmgpuHardToken *hard;      // [hard_cap] out: tokens outside the exact fast path, for the host's strtod
    uint32_t hard_cap;
    uint32_t *hard_count;      // out (+=): hard tokens met, also those the list had no room for
    unsigned long long *err;   // out (min=): the first byte of the first malformed row (chunk offset); ~0 before
};
hipError_t launch_parse_count(const EmgpuParseRun &P, hipStream_t s);   // cnt, scratch
hipError_t launch_parse_rows(const EmgpuParseRun &P, hipStream_t s);    // table, hard, err
hipError_t launch_parse_patch(double *table, const EmgpuHardToken *hard, const double *val, uint32_t n, hipStream_t s);   // table[hard[i].pos] = val[i]
// Runs of equal ids in column 0 of table [R][ncol] (sample2track.m:192-193 without a sort): mark + scan + fill give run_id / run_first
// (scratch words 0-1: the number of runs); the runs go into an open-addressing table (keys: 2^k entries preset to ~0, *dup = 1 when an id owns
// two runs); each of n wanted ids is matched to its run (first row and length; length 0 when there is none).
struct EmgpuRunTable {
    const double *table; int32_t ncol; int64_t R;
    uint32_t *cnt, *scratch;                 // [R], pack_scratch_words(R)
    double *run_id; int64_t *run_first;      // [runs]
    unsigned long long *keys; uint32_t *vals; uint32_t mask; uint32_t *dup;
};
hipError_t launch_run_mark(const EmgpuRunTable &G, hipStream_t s);
hipError_t launch_run_fill(const EmgpuRunTable &G, hipStream_t s);
hipError_t launch_run_match(const EmgpuRunTable &G, uint32_t runs, int64_t n, const double *ids, int64_t *first, int32_t *len, hipStream_t s);
// k_sample2track_table: lane i integrates len[i] rows of the parsed table, rows first[i] .. (or rowidx[first[i] ..] when ids are interleaved)
struct EmgpuTrackTableRun {
    int64_t n;
    double ur_speed, ur_vertrate, ur_heading, min_speed, max_speed;
    const double *alt0, *speed0;            // [n]
    const double *table; int32_t ncol, c_vr, c_acc, c_tr;
    const int64_t *first; const int32_t *len; const int64_t *rowidx;
    const uint64_t *xoff;                   // [n + 1]: first position row of track i (len[i] + 1 rows each)
    double *xyz;                            // [xoff[n]][3] out
    uint8_t *flags; double *vmm;            // [n], [n][2] out
};
hipError_t launch_sample2track_table(const EmgpuTrackTableRun &A, hipStream_t s, const char **name);
// sample2track.m:277-278 (emgpu_kernels_csv.hip): "time_s,x_ft,y_ft,z_ft\n" and "%i,%0.0f,%0.0f,%0.0f\n" per second for every track with flags 0
struct EmgpuCsvRun {
    int64_t n;
    const uint8_t *flags; const int32_t *len; const uint64_t *xoff; const double *xyz;
    uint32_t *cnt;               // [n] out (launch_csv_len): bytes of track i's file; 0: rejected, or left to the host formatter
    uint8_t *hostfmt;            // [n] out: 1 = accepted, but a coordinate is not finite or 2^63 and more in magnitude
    const uint64_t *off;         // [n] (launch_csv_emit): first byte of track i's file in csv
    char *csv;
};
hipError_t launch_csv_len(const EmgpuCsvRun &C, hipStream_t s);
hipError_t launch_csv_emit(const EmgpuCsvRun &C, hipStream_t s);
// "%0.0f" of n doubles, one after the other (emgpu_format_f0_host): as launch_format_g; a value the device does not format has length 0
hipError_t launch_format_f0(const double *x, int64_t n, uint32_t *cnt, uint32_t *scratch, char *text, uint64_t base, uint64_t *offsets, hipStream_t s);
} // namespace emgpu
