// emgpu_files.cpp -- the file pipeline of the C ABI, text in and text out on the device:
//   * text tables in: parse_to_device behind emgpu_parse_table_host and emgpu_tracks_text_host (the files sample2track.m reads);
//   * values out: emgpu_format_g_host ("%g" of f32, em_sample's files) and emgpu_format_f0_host ("%0.0f" of f64), one pass loop;
//   * sample2track's track files: emgpu_tracks_text_host -- rows grouped by id, the track kernel, the CSV text -- and emgpu_csv_bound.
// Device blocks, the chunk buffers and the staging buffers are emgpu_memory.cpp's (emgpu_hostmem.hpp).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "emgpu_hostmem.hpp"

using namespace emgpu_detail;

// ------------------------------------------------------------------------------------------------ the file pipeline's text tables, parsed on the device
namespace {
size_t env_size(const char *name, size_t dflt) {
    const char *e = getenv(name);
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (size_t)v : dflt;
}

struct DeviceTable {   // the parsed table: a block of the traces' allocator, released on every path out
    double *d = nullptr;
    int64_t rows = 0, cap_rows = 0;
    uint64_t hard = 0;
    int32_t chunks = 0;
    double h2d_ms = 0, kernel_ms = 0, host_ms = 0;
    DeviceTable() = default;
    DeviceTable(const DeviceTable &) = delete;
    DeviceTable &operator=(const DeviceTable &) = delete;
    ~DeviceTable() { if (d) { (void)hipDeviceSynchronize(); device_release(d); } }
};

int64_t line_of(const char *text, size_t off) {   // 1-based line of byte off
    int64_t line = 1;
    for (const char *q = text, *e = text + off; q < e && (q = (const char *)memchr(q, '\n', (size_t)(e - q))) != nullptr; q++) line++;
    return line;
}

// where text [nbytes] is cut into chunks of about `target` bytes, each ending behind a newline: chunk k is [cut[k], cut[k + 1])
std::vector<size_t> chunk_cuts(const char *text, size_t nbytes, size_t target, const char *who) {
    std::vector<size_t> cut{0};
    while (cut.back() < nbytes) {
        const size_t a = cut.back();
        size_t b = nbytes;
        if (nbytes - a > target) {
            const void *q = memrchr(text + a, '\n', target);
            if (!q) q = memchr(text + a + target, '\n', nbytes - a - target);   // a line longer than a chunk: the chunk ends with it
            b = q ? (size_t)((const char *)q - text) + 1 : nbytes;
        }
        if (b - a > (size_t)0xFFFFFF00u) throw Error(EMGPU_ERR_ARG, std::string(who) + ": a line of more than 4 GB: a chunk's offsets would not fit 32 bits");
        cut.push_back(b);
    }
    return cut;
}

// text [nbytes] -> T.d [T.rows][ncol] on the device.  The text goes up in chunks cut behind a newline (EMGPU_HOST_CHUNK_MB, or
// EMGPU_DEBUG_PARSE_CHUNK_BYTES for tests that want the cuts at every position of a row), chunk k + 1's copy on the copy stream behind chunk k's
// parse; pageable text through the pinned staging buffers.  Offsets within a chunk are 32-bit, offsets into the text and rows 64-bit.
// Hard tokens (emgpu_kernels_parse.hip) are finished here with strtod; a chunk with more of them than the list holds (EMGPU_DEBUG_PARSE_HARD_CAP
// entries, default 65 536) is parsed again with a list of the counted size.  Throws Error(EMGPU_ERR_PARSE) naming the first malformed line.
void parse_to_device(emgpu_ctx *ctx, const char *what, const char *text, size_t nbytes, int ncol, DeviceTable &T) {
    T.cap_rows = (int64_t)(nbytes / (2 * (size_t)ncol)) + 1;   // a row of ncol numbers is at least 2 ncol - 1 bytes and what ends its line
    const size_t table_bytes = std::max<size_t>((size_t)T.cap_rows * (size_t)ncol * 8, 256);
    T.d = (double *)device_block_or_trim(ctx, table_bytes);
    if (!T.d) throw Error(EMGPU_ERR_HIP, std::string(what) + ": the parsed table (" + std::to_string(table_bytes) + " bytes) does not fit the device's memory");
    if (!nbytes) return;
    const size_t target = std::min<size_t>(env_size("EMGPU_DEBUG_PARSE_CHUNK_BYTES", host_chunk_target((size_t)256 << 20)), (size_t)0xC0000000u);
    const std::vector<size_t> cut = chunk_cuts(text, nbytes, target, what);
    const size_t nchunks = cut.size() - 1;
    size_t maxc = 0;
    for (size_t k = 0; k < nchunks; k++) maxc = std::max(maxc, cut[k + 1] - cut[k]);
    T.chunks = (int32_t)nchunks;
    const size_t tiles_max = (maxc + emgpu::kParseTile - 1) / emgpu::kParseTile;
    const size_t hard_cap = env_size("EMGPU_DEBUG_PARSE_HARD_CAP", 65536);
    size_t o = 0;
    auto put = [&](size_t bytes) { const size_t at = o; o = round_up(o + std::max<size_t>(bytes, 1), 256); return at; };
    const size_t o_text = put(maxc + 8), o_cnt = put(tiles_max * 4), o_scr = put(emgpu::pack_scratch_words((int64_t)tiles_max) * 4);
    const size_t o_hard = put(hard_cap * sizeof(emgpu::EmgpuHardToken)), o_val = put(hard_cap * 8), o_misc = put(16);   // misc: err (u64), hard count (u32)
    const bool pinned = is_pinned(text);
    if (!provision(ctx, nchunks, o, pinned ? 256 : maxc)) throw Error(EMGPU_ERR_HIP, std::string(what) + ": out of device memory");
    Events ev(8);   // per buffer b: 4b + {copy start, copy end, parse start, parse end}
    auto upload = [&](size_t k) {
        const int b = (int)(k & 1);
        const char *src = text + cut[k];
        const size_t len = cut[k + 1] - cut[k];
        if (!pinned) { const auto t0 = Clock::now(); memcpy(ctx->h_stage[b], src, len); src = (const char *)ctx->h_stage[b]; T.host_ms += ms_since(t0); }
        HIP_OK(hipEventRecord(ev[4 * b], ctx->copy_stream));
        HIP_OK(hipMemcpyAsync((char *)ctx->chunk_buf[b].p + o_text, src, len, hipMemcpyHostToDevice, ctx->copy_stream));
        HIP_OK(hipEventRecord(ev[4 * b + 1], ctx->copy_stream));
    };
    struct Extra { void *p = nullptr; ~Extra() { if (p) (void)hipFree(p); } };
    try {
        HIP_OK(hipStreamSynchronize(ctx->stream));   // (the chunk buffers may still be read by an earlier call's copies)
        HIP_OK(hipStreamSynchronize(ctx->copy_stream));
        upload(0);
        for (size_t k = 0; k < nchunks; k++) {
            const int b = (int)(k & 1);
            char *dev = (char *)ctx->chunk_buf[b].p;
            const size_t len = cut[k + 1] - cut[k];
            emgpu::EmgpuParseRun P{};
            P.text = (const uint8_t *)(dev + o_text); P.nbytes = (uint32_t)len; P.ncol = ncol;
            P.cnt = (uint32_t *)(dev + o_cnt); P.scratch = (uint32_t *)(dev + o_scr);
            P.table = T.d; P.row_base = T.rows; P.table_rows = T.cap_rows;
            P.hard = (emgpu::EmgpuHardToken *)(dev + o_hard); P.hard_cap = (uint32_t)hard_cap;
            P.err = (unsigned long long *)(dev + o_misc); P.hard_count = (uint32_t *)(dev + o_misc + 8);
            HIP_OK(hipStreamWaitEvent(ctx->stream, ev[4 * b + 1], 0));
            HIP_OK(hipEventRecord(ev[4 * b + 2], ctx->stream));
            HIP_OK(hipMemsetAsync(dev + o_misc, 0xFF, 8, ctx->stream));
            HIP_OK(hipMemsetAsync(dev + o_misc + 8, 0, 8, ctx->stream));
            launch_ok(emgpu::launch_parse_count(P, ctx->stream));
            HIP_OK(hipMemcpyAsync(&ctx->h_total[2 * b], P.scratch, 8, hipMemcpyDeviceToHost, ctx->stream));
            if (k + 1 < nchunks) upload(k + 1);   // (its buffer's last reader, chunk k - 1's parse, has been waited for)
            HIP_OK(hipStreamSynchronize(ctx->stream));
            const uint64_t rows = ctx->h_total[2 * b];
            P.rows = (uint32_t)rows;
            launch_ok(emgpu::launch_parse_rows(P, ctx->stream));
            HIP_OK(hipMemcpyAsync(&ctx->h_total[2 * b], dev + o_misc, 16, hipMemcpyDeviceToHost, ctx->stream));
            HIP_OK(hipEventRecord(ev[4 * b + 3], ctx->stream));
            HIP_OK(hipStreamSynchronize(ctx->stream));
            const uint64_t err = ctx->h_total[2 * b];
            if (err != ~0ull)
                throw Error(EMGPU_ERR_PARSE, std::string(what) + ": line " + std::to_string(line_of(text, cut[k] + (size_t)err)) + " is not a row of " +
                                                 std::to_string(ncol) + " numbers");
            if (T.rows + (int64_t)rows > T.cap_rows) throw Error(EMGPU_ERR_PARSE, std::string(what) + ": more rows than the text has room for");
            const uint32_t nh = (uint32_t)ctx->h_total[2 * b + 1];
            Extra extra;
            const emgpu::EmgpuHardToken *d_list = P.hard;
            double *d_val = (double *)(dev + o_val);
            if (nh > hard_cap) {   // the list was too small: once more with one of the counted size (the values written meanwhile are the same)
                HIP_OK(hipMalloc(&extra.p, (size_t)nh * 24));
                P.hard = (emgpu::EmgpuHardToken *)extra.p; P.hard_cap = nh;
                d_list = P.hard; d_val = (double *)((char *)extra.p + (size_t)nh * 16);
                HIP_OK(hipMemsetAsync(dev + o_misc + 8, 0, 8, ctx->stream));
                launch_ok(emgpu::launch_parse_rows(P, ctx->stream));
                HIP_OK(hipStreamSynchronize(ctx->stream));
            }
            if (nh) {
                const auto t0 = Clock::now();
                std::vector<emgpu::EmgpuHardToken> list(nh);
                std::vector<double> val(nh);
                HIP_OK(hipMemcpy(list.data(), d_list, (size_t)nh * 16, hipMemcpyDeviceToHost));
                std::string tok;
                for (uint32_t i = 0; i < nh; i++) {
                    const char *q = text + cut[k] + list[i].off, *e = text + cut[k + 1], *r = q;
                    while (r < e && *r != ' ' && *r != '\t' && *r != '\n' && *r != '\r') r++;
                    tok.assign(q, r);
                    val[i] = strtod(tok.c_str(), nullptr);
                }
                HIP_OK(hipMemcpyAsync(d_val, val.data(), (size_t)nh * 8, hipMemcpyHostToDevice, ctx->stream));
                launch_ok(emgpu::launch_parse_patch(T.d, d_list, d_val, nh, ctx->stream));
                HIP_OK(hipStreamSynchronize(ctx->stream));
                T.host_ms += ms_since(t0);
            }
            float ms = 0.f;
            HIP_OK(hipEventElapsedTime(&ms, ev[4 * b], ev[4 * b + 1])); T.h2d_ms += ms;
            HIP_OK(hipEventElapsedTime(&ms, ev[4 * b + 2], ev[4 * b + 3])); T.kernel_ms += ms;
            T.rows += (int64_t)rows;
            T.hard += nh;
        }
    } catch (...) {
        (void)hipStreamSynchronize(ctx->stream);
        if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
        throw;
    }
}

// ------------------------------------------------------------------------------------------------ values as text, pass by pass
constexpr size_t kFormatPass = (size_t)1 << 22;   // values per pass: a pass's text (bytes_per_value bytes a value at most) is counted in 32 bits

// The pass loop of emgpu_format_g_host / emgpu_format_f0_host (`who`): x [n] through launch(d_x, c, d_cnt, d_scr, d_text, total, d_off) into
// out [cap] and offsets [n + 1].  A pass that would end beyond cap stays on the device (and every later one: the total only grows); the
// offsets and the total go on, the status is EMGPU_ERR_EVENT_CAP and offsets[n] what the call needs.
template <typename T, typename Launch>
int format_values(emgpu_ctx *ctx, const char *who, const T *x, int64_t n, char *out, int64_t cap, uint64_t *offsets, size_t bytes_per_value, Launch launch) {
    const size_t C = std::min((size_t)n, kFormatPass);
    uint64_t total = 0;
    CallBuffers B(ctx);
    T *d_x = B.alloc<T>(C * sizeof(T));
    uint32_t *d_cnt = B.alloc<uint32_t>(C * 4), *d_scr = B.alloc<uint32_t>(emgpu::pack_scratch_words((int64_t)C) * 4);
    char *d_text = B.alloc<char>(C * bytes_per_value);
    uint64_t *d_off = B.alloc<uint64_t>(C * 8);
    for (size_t k0 = 0; k0 < (size_t)n; k0 += C) {
        const size_t c = std::min(C, (size_t)n - k0);
        B.up(d_x, x + k0, c * sizeof(T));
        launch_ok(launch(d_x, (int64_t)c, d_cnt, d_scr, d_text, total, d_off));
        uint64_t bytes = 0;
        B.down(&bytes, d_scr, sizeof bytes);
        B.down(offsets + k0, d_off, c * 8);
        HIP_OK(hipStreamSynchronize(ctx->stream));
        if (bytes > c * bytes_per_value) throw Error(EMGPU_ERR_HIP, std::string(who) + ": a pass's text outgrew its bound");
        if (total + bytes <= (uint64_t)cap) { B.down(out + total, d_text, (size_t)bytes); HIP_OK(hipStreamSynchronize(ctx->stream)); }
        total += bytes;
    }
    offsets[n] = total;
    if (total <= (uint64_t)cap) return EMGPU_OK;
    return fail(EMGPU_ERR_EVENT_CAP, std::string(who) + ": the text has " + std::to_string(total) + " bytes, cap is " + std::to_string(cap));
}

// ------------------------------------------------------------------------------------------------ sample2track's files
// One emgpu_tracks_text_host call: what its three phases -- group_rows, run_tracks, emit_csv, in this order -- take from the entry point
// and hand on to each other.  The device pointers are buffers of the call's CallBuffers.
struct TracksCall {
    emgpu_ctx *ctx; const emgpu_track_params *p; const emgpu_tracks_text_in *in; const emgpu_tracks_text_out *out; const DeviceTable *T;
    size_t n, n1;                                // tracks wanted; max(n, 1)
    double *d_in, *d_vmm;                        // [3][n]: the wanted ids, alt0, speed0; [2][n]: speed_minmax
    uint8_t *d_flags; uint64_t *d_xoff;          // [n]; [n + 1]: track i's first position row
    // group_rows: track i is rows first[i] ... first[i] + len[i] - 1 of the table, or of rowidx where an id's rows are not one run
    int64_t *d_first; int32_t *d_len; const int64_t *d_rowidx; std::vector<int32_t> len;
    std::vector<uint64_t> xoff; double *d_xyz; uint64_t xyz_rows;   // run_tracks (xoff feeds an asynchronous upload: it lives as long as the call)
    uint64_t csv_total;                          // emit_csv
    emgpu_host_stats_t st; double phase[6];      // phase: upload, parse kernels, grouping + track kernels, CSV kernels, download, host work
};

// the runs of equal ids, and every wanted id's run; an id that owns several runs sends the call through the host grouping (totals[4] = 1)
void group_rows(TracksCall &S, CallBuffers &B, const Events &ev) {
    emgpu_ctx *ctx = S.ctx;
    const size_t n = S.n;
    const int64_t R = S.T->rows;
    const int ncol = S.in->ncol;
    HIP_OK(hipEventRecord(ev[0], ctx->stream));
    emgpu::EmgpuRunTable G{};
    G.table = S.T->d; G.ncol = ncol; G.R = R;
    G.cnt = B.alloc<uint32_t>(std::max<size_t>((size_t)R, 1) * 4);
    G.scratch = B.alloc<uint32_t>(emgpu::pack_scratch_words(R) * 4);
    launch_ok(emgpu::launch_run_mark(G, ctx->stream));
    uint64_t runs = 0;
    B.down(&runs, G.scratch, 8);
    HIP_OK(hipStreamSynchronize(ctx->stream));
    if (runs >= 0x7FFFFFFFull) throw Error(EMGPU_ERR_ARG, "emgpu_tracks_text_host: more than 2^31 - 1 runs of ids");
    size_t H = 16;
    while (H < 2 * runs) H <<= 1;
    G.run_id = B.alloc<double>(std::max<size_t>(runs, 1) * 8); G.run_first = B.alloc<int64_t>(std::max<size_t>(runs, 1) * 8);
    G.keys = B.alloc<unsigned long long>(H * 8); G.vals = B.alloc<uint32_t>(H * 4); G.mask = (uint32_t)(H - 1);
    G.dup = B.alloc<uint32_t>(4);
    HIP_OK(hipMemsetAsync(G.keys, 0xFF, H * 8, ctx->stream));
    HIP_OK(hipMemsetAsync(G.dup, 0, 4, ctx->stream));
    launch_ok(emgpu::launch_run_fill(G, ctx->stream));
    launch_ok(emgpu::launch_run_match(G, (uint32_t)runs, (int64_t)n, S.d_in, S.d_first, S.d_len, ctx->stream));
    uint32_t dup = 0;
    std::vector<int32_t> &len = S.len;
    len.resize(n);
    B.down(&dup, G.dup, 4);
    B.down(len.data(), S.d_len, n * 4);
    HIP_OK(hipStreamSynchronize(ctx->stream));
    if (!dup) return;
    // an id owns more than one run: the reference's selection (every row with that id, in file order) through a stable sort on the host
    const auto t0 = Clock::now();
    S.out->totals[4] = 1;
    std::vector<double> ids((size_t)R);
    HIP_OK(hipMemcpy2D(ids.data(), 8, S.T->d, (size_t)ncol * 8, 8, (size_t)R, hipMemcpyDeviceToHost));
    std::vector<int64_t> order;
    order.reserve((size_t)R);
    for (int64_t r = 0; r < R; r++) if (ids[(size_t)r] == ids[(size_t)r]) order.push_back(r);
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return ids[(size_t)a] < ids[(size_t)b]; });
    std::vector<int64_t> first(n), rowidx;
    for (size_t i = 0; i < n; i++) {
        const double id = S.in->id[i];
        first[i] = (int64_t)rowidx.size();
        if (id == id) {
            auto lo = std::lower_bound(order.begin(), order.end(), id, [&](int64_t a, double v) { return ids[(size_t)a] < v; });
            for (; lo != order.end() && ids[(size_t)*lo] == id; ++lo) rowidx.push_back(*lo);
        }
        const int64_t l = (int64_t)rowidx.size() - first[i];
        if (l > 0x7FFFFFFF) throw Error(EMGPU_ERR_ARG, "emgpu_tracks_text_host: a track of more than 2^31 - 1 rows");
        len[i] = (int32_t)l;
    }
    int64_t *d_ri = B.alloc<int64_t>(std::max<size_t>(rowidx.size(), 1) * 8);
    B.up(d_ri, rowidx.data(), rowidx.size() * 8);
    B.up(S.d_first, first.data(), n * 8);
    B.up(S.d_len, len.data(), n * 4);
    HIP_OK(hipStreamSynchronize(ctx->stream));   // (the vectors go out of scope)
    S.d_rowidx = d_ri;
    S.phase[5] += ms_since(t0);
}

// the position rows' offsets, the positions' block and the track kernel; flags and speed_minmax start on their way back
void run_tracks(TracksCall &S, CallBuffers &B, const Events &ev) {
    emgpu_ctx *ctx = S.ctx;
    const size_t n = S.n;
    S.xoff.assign(n + 1, 0);
    for (size_t i = 0; i < n; i++) {
        if (S.len[i] > 50000000) throw Error(EMGPU_ERR_ARG, "emgpu_tracks_text_host: a track of more than 50 000 000 rows: its file would not fit 32 bits");
        S.xoff[i + 1] = S.xoff[i] + (uint64_t)S.len[i] + 1;
    }
    S.xyz_rows = S.xoff[n];
    if (S.out->lengths) memcpy(S.out->lengths, S.len.data(), n * 4);
    if (S.out->offsets || S.out->xyz) {
        // (B frees the block with the call's other buffers, after it has synchronised ctx->stream: everything that touches it runs on that stream)
        S.d_xyz = B.try_alloc<double>(std::max<size_t>((size_t)S.xyz_rows * 24, 256));
        if (!S.d_xyz) throw Error(EMGPU_ERR_HIP, "emgpu_tracks_text_host: the positions (" + std::to_string(S.xyz_rows * 24) + " bytes) do not fit the device's memory");
    }
    B.up(S.d_xoff, S.xoff.data(), (n + 1) * 8);
    emgpu::EmgpuTrackTableRun A{};
    A.n = (int64_t)n;
    set_track_units(A, S.p);
    A.alt0 = S.d_in + n; A.speed0 = S.d_in + 2 * n;
    A.table = S.T->d; A.ncol = S.in->ncol; A.c_vr = S.in->col_vertrate; A.c_acc = S.in->col_acc; A.c_tr = S.in->col_turnrate;
    A.first = S.d_first; A.len = S.d_len; A.rowidx = S.d_rowidx; A.xoff = S.d_xoff; A.xyz = S.d_xyz; A.flags = S.d_flags; A.vmm = S.d_vmm;
    launch_named(ctx, [&](const char **name) { return emgpu::launch_sample2track_table(A, ctx->stream, name); });
    HIP_OK(hipEventRecord(ev[1], ctx->stream));
    B.down(S.out->flags, S.d_flags, n);
    B.down(S.out->speed_minmax, S.d_vmm, 2 * n * 8);
}

// every track's file length, the files' offsets and -- where the caller gave a buffer that holds them -- the files themselves
void emit_csv(TracksCall &S, CallBuffers &B, const Events &ev) {
    emgpu_ctx *ctx = S.ctx;
    const emgpu_tracks_text_out *out = S.out;
    const size_t n = S.n;
    std::vector<uint64_t> off(n + 1, 0);
    emgpu::EmgpuCsvRun C{};
    C.n = (int64_t)n; C.flags = S.d_flags; C.len = S.d_len; C.xoff = S.d_xoff; C.xyz = S.d_xyz;
    C.cnt = B.alloc<uint32_t>(S.n1 * 4); C.hostfmt = B.alloc<uint8_t>(S.n1);
    HIP_OK(hipEventRecord(ev[2], ctx->stream));
    launch_ok(emgpu::launch_csv_len(C, ctx->stream));
    HIP_OK(hipEventRecord(ev[3], ctx->stream));
    std::vector<uint32_t> cnt(n);
    std::vector<uint8_t> hostfmt(n);
    B.down(cnt.data(), C.cnt, n * 4);
    B.down(hostfmt.data(), C.hostfmt, n);
    HIP_OK(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < n; i++) { off[i + 1] = off[i] + cnt[i]; out->totals[3] += hostfmt[i]; }
    S.csv_total = off[n];
    memcpy(out->offsets, off.data(), (n + 1) * 8);
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, ev[2], ev[3])); S.phase[3] += ms;
    if (!out->csv || !S.csv_total || S.csv_total > (uint64_t)out->csv_cap) return;
    char *d_csv = B.try_alloc<char>((size_t)S.csv_total + 8);   // (freed by B like the positions' block)
    if (!d_csv) throw Error(EMGPU_ERR_HIP, "emgpu_tracks_text_host: the CSV text (" + std::to_string(S.csv_total) + " bytes) does not fit the device's memory");
    uint64_t *d_off = B.alloc<uint64_t>(S.n1 * 8);
    B.up(d_off, off.data(), n * 8);
    C.off = d_off; C.csv = d_csv;
    HIP_OK(hipEventRecord(ev[2], ctx->stream));
    launch_ok(emgpu::launch_csv_emit(C, ctx->stream));
    HIP_OK(hipEventRecord(ev[3], ctx->stream));
    HIP_OK(hipEventRecord(ev[4], ctx->stream));
    B.down(out->csv, d_csv, (size_t)S.csv_total);
    HIP_OK(hipEventRecord(ev[5], ctx->stream));
    HIP_OK(hipStreamSynchronize(ctx->stream));
    HIP_OK(hipEventElapsedTime(&ms, ev[2], ev[3])); S.phase[3] += ms;
    HIP_OK(hipEventElapsedTime(&ms, ev[4], ev[5])); S.phase[4] += ms;
    S.st.bytes_d2h += (int64_t)S.csv_total;
}
} // namespace

extern "C" {

int emgpu_format_g_host(emgpu_ctx *ctx, const float *x, int64_t n, char *out, int64_t cap, uint64_t *offsets) {
    EMGPU_TRY
    if (!ctx || !offsets || (n > 0 && !x) || (cap > 0 && !out)) return fail(EMGPU_ERR_ARG, "null argument");
    if (n < 0 || cap < 0) return fail(EMGPU_ERR_ARG, "n < 0 or cap < 0");
    CTX_DEVICE(ctx);
    offsets[0] = 0;
    if (n == 0) return EMGPU_OK;
    uint64_t paths[2] = {0, 0};
    CallBuffers B(ctx);
    unsigned long long *d_paths = B.alloc<unsigned long long>(16);
    HIP_OK(hipMemsetAsync(d_paths, 0, 16, ctx->stream));
    const int rc = format_values(ctx, "emgpu_format_g_host", x, n, out, cap, offsets, 12,
                                 [&](auto... pass) { return emgpu::launch_format_g(pass..., d_paths, ctx->stream); });
    B.down(paths, d_paths, sizeof paths);
    HIP_OK(hipStreamSynchronize(ctx->stream));
    ctx->format_paths[0] += paths[0];
    ctx->format_paths[1] += paths[1];
    return rc;
    EMGPU_CATCH
}

int emgpu_debug_format_paths(emgpu_ctx *ctx, uint64_t out[2]) {
    if (!ctx || !out) return fail(EMGPU_ERR_ARG, "null argument");
    CTX_LOCK(ctx);
    out[0] = ctx->format_paths[0]; out[1] = ctx->format_paths[1];
    ctx->format_paths[0] = ctx->format_paths[1] = 0;
    return EMGPU_OK;
}

int emgpu_format_f0_host(emgpu_ctx *ctx, const double *x, int64_t n, char *out, int64_t cap, uint64_t *offsets) {
    EMGPU_TRY
    if (!ctx || !offsets || (n > 0 && !x) || (cap > 0 && !out)) return fail(EMGPU_ERR_ARG, "null argument");
    if (n < 0 || cap < 0) return fail(EMGPU_ERR_ARG, "n < 0 or cap < 0");
    CTX_DEVICE(ctx);
    offsets[0] = 0;
    if (n == 0) return EMGPU_OK;
    return format_values(ctx, "emgpu_format_f0_host", x, n, out, cap, offsets, 20, [&](auto... pass) { return emgpu::launch_format_f0(pass..., ctx->stream); });
    EMGPU_CATCH
}

// ================================================================================================ sample2track's files
int64_t emgpu_csv_bound(int64_t n, int64_t rows) { return n < 0 || rows < 0 ? -1 : 22 * n + 74 * rows; }

int emgpu_parse_table_host(emgpu_ctx *ctx, const char *text, int64_t nbytes, int32_t ncol, double *out, int64_t rows_cap, int64_t *rows, uint64_t *hard_tokens) {
    EMGPU_TRY
    if (!ctx || !rows || (nbytes > 0 && !text) || (rows_cap > 0 && !out)) return fail(EMGPU_ERR_ARG, "null argument");
    if (nbytes < 0 || rows_cap < 0 || ncol < 1 || ncol > 4096) return fail(EMGPU_ERR_ARG, "nbytes < 0, rows_cap < 0 or ncol outside 1..4096");
    CTX_DEVICE(ctx);
    *rows = 0;
    if (hard_tokens) *hard_tokens = 0;
    DeviceTable T;
    parse_to_device(ctx, "emgpu_parse_table_host", text, (size_t)nbytes, ncol, T);
    *rows = T.rows;
    if (hard_tokens) *hard_tokens = T.hard;
    if (T.rows > rows_cap) return fail(EMGPU_ERR_EVENT_CAP, "emgpu_parse_table_host: the text has " + std::to_string(T.rows) + " rows, rows_cap is " + std::to_string(rows_cap));
    if (T.rows) HIP_OK(hipMemcpy(out, T.d, (size_t)T.rows * (size_t)ncol * 8, hipMemcpyDeviceToHost));
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_tracks_text_host(emgpu_ctx *ctx, const emgpu_track_params *p, const emgpu_tracks_text_in *in, const emgpu_tracks_text_out *out) {
    EMGPU_TRY
    if (!ctx || !p || !in || !out) return fail(EMGPU_ERR_ARG, "null argument");
    if (!out->totals || !out->flags) return fail(EMGPU_ERR_ARG, "flags and totals are required");
    if (p->n < 0 || in->nbytes < 0 || (in->nbytes > 0 && !in->text)) return fail(EMGPU_ERR_ARG, "n < 0, or no text");
    if (p->n > 0 && (!in->id || !in->alt0 || !in->speed0)) return fail(EMGPU_ERR_ARG, "id, alt0 and speed0 are required");
    if (p->n > 0x7FFFFFFF) return fail(EMGPU_ERR_ARG, "more than 2^31 - 1 tracks in one call");
    if (in->ncol < 2 || in->ncol > 4096) return fail(EMGPU_ERR_ARG, "ncol outside 2..4096");
    for (int32_t c : {in->col_vertrate, in->col_acc, in->col_turnrate})
        if (c < 0 || c >= in->ncol) return fail(EMGPU_ERR_ARG, "an update column outside 0..ncol-1");
    if (out->csv_cap < 0 || out->xyz_cap < 0 || (out->csv && !out->offsets)) return fail(EMGPU_ERR_ARG, "csv_cap / xyz_cap < 0, or csv without offsets");
    CTX_DEVICE(ctx);
    const auto t_call = Clock::now();
    const size_t n = (size_t)p->n;
    for (int k = 0; k < 5; k++) out->totals[k] = 0;
    DeviceTable T;
    parse_to_device(ctx, "emgpu_tracks_text_host", in->text, (size_t)in->nbytes, in->ncol, T);
    out->totals[1] = T.rows;
    out->totals[2] = (int64_t)T.hard;
    TracksCall S{ctx, p, in, out, &T, n, std::max<size_t>(n, 1)};
    S.phase[0] = T.h2d_ms; S.phase[1] = T.kernel_ms; S.phase[5] = T.host_ms;
    S.st.chunks = T.chunks; S.st.threads = 1; S.st.direct = (is_pinned(in->text) && (!out->csv || is_pinned(out->csv))) ? 1 : 0;
    int rc = EMGPU_OK;
    {
        CallBuffers B(ctx);
        Events ev(6);   // 0, 1: grouping + track kernels; 2, 3: a CSV kernel; 4, 5: the CSV's download
        S.d_in = B.alloc<double>(3 * S.n1 * 8); S.d_vmm = B.alloc<double>(2 * S.n1 * 8);
        S.d_first = B.alloc<int64_t>(S.n1 * 8); S.d_len = B.alloc<int32_t>(S.n1 * 4);
        S.d_flags = B.alloc<uint8_t>(S.n1); S.d_xoff = B.alloc<uint64_t>((S.n1 + 1) * 8);
        B.up(S.d_in, in->id, n * 8); B.up(S.d_in + n, in->alt0, n * 8); B.up(S.d_in + 2 * n, in->speed0, n * 8);
        group_rows(S, B, ev);
        run_tracks(S, B, ev);
        if (out->offsets) emit_csv(S, B, ev);
        out->totals[0] = (int64_t)S.csv_total;
        if (out->xyz && S.xyz_rows <= (uint64_t)out->xyz_cap) { B.down(out->xyz, S.d_xyz, (size_t)S.xyz_rows * 24); S.st.bytes_d2h += (int64_t)S.xyz_rows * 24; }
        rc = emgpu_ctx_sync(ctx);
        float ms = 0.f;
        HIP_OK(hipEventElapsedTime(&ms, ev[0], ev[1])); S.phase[2] = ms;
    }
    S.st.kernel_ms = S.phase[1] + S.phase[2] + S.phase[3]; S.st.d2h_ms = S.phase[4]; S.st.scatter_ms = S.phase[5];
    S.st.total_ms = ms_since(t_call);
    ctx->host_stats = S.st;
    if (out->phase_ms) memcpy(out->phase_ms, S.phase, sizeof S.phase);
    if (rc == EMGPU_OK && out->csv && S.csv_total > (uint64_t)out->csv_cap)
        return fail(EMGPU_ERR_EVENT_CAP, "emgpu_tracks_text_host: the CSV text has " + std::to_string(S.csv_total) + " bytes, csv_cap is " + std::to_string(out->csv_cap));
    if (rc == EMGPU_OK && out->xyz && S.xyz_rows > (uint64_t)out->xyz_cap)
        return fail(EMGPU_ERR_EVENT_CAP, "emgpu_tracks_text_host: the tracks have " + std::to_string(S.xyz_rows) + " position rows, xyz_cap is " + std::to_string(out->xyz_cap));
    return rc;
    EMGPU_CATCH
}

} // extern "C"
