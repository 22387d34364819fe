// emgpu_capi.cpp -- the part of the C ABI declared in include/emgpu.h that never sees a context: the error plumbing, the version (this
// unit carries the source hash), the model accessors and the plain functions.  The context: emgpu_ctx.cpp; sampling: emgpu_sample.cpp;
// the terminal model: emgpu_terminal.cpp; tracks: emgpu_track.cpp; the device-free debug getters: emgpu_debug.cpp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/emgpu.h"
#include "emgpu_launch.h"
#include "emgpu_model.hpp"

#include "emgpu_internal.hpp"

namespace emgpu_detail {
std::string &last_error() {
    thread_local std::string e;
    return e;
}
int fail(int code, const std::string &msg) {
    last_error() = msg;
    return code;
}
} // namespace emgpu_detail

template <typename T, typename V>
static int64_t copy_out(const V &v, T *out, int64_t cap) {
    if (out) {
        if ((int64_t)v.size() > cap) return fail(EMGPU_ERR_ARG, "output buffer too small");
        for (size_t i = 0; i < v.size(); i++) out[i] = (T)v[i];
    }
    return (int64_t)v.size();
}

extern "C" {

const char *emgpu_last_error(void) { return g_err.c_str(); }
#ifndef EMGPU_SRC_HASH
#define EMGPU_SRC_HASH "unhashed"
#endif
#define EMGPU_STR2(x) #x
#define EMGPU_STR(x) EMGPU_STR2(x)
const char *emgpu_version(void) { return "emgpu 0.4 (gfx950) philox4x32-" EMGPU_STR(EMGPU_PHILOX_ROUNDS) " src:" EMGPU_SRC_HASH; }
int32_t emgpu_philox_rounds(void) { return EMGPU_PHILOX_ROUNDS; }
int32_t emgpu_slot_map_revision(void) { return 2; }

int emgpu_model_load_txt(const char *path, const int32_t *idx_zero_boundaries, int32_t n_idx,
                         int32_t is_overwrite_zero_boundaries, emgpu_model **out) {
    EMGPU_TRY
    if (!path || !out) return fail(EMGPU_ERR_ARG, "null argument");
    std::unique_ptr<Model> m(emgpu::load_txt(path, idx_zero_boundaries, n_idx, is_overwrite_zero_boundaries != 0));
    *out = new emgpu_model{std::move(*m)};
    return EMGPU_OK;
    EMGPU_CATCH
}

/* em_read.m:47-107 once, then the binary cache */
int emgpu_model_save_bin(const emgpu_model *m, const char *path) {
    EMGPU_TRY
    if (!m || !path) return fail(EMGPU_ERR_ARG, "null argument");
    emgpu::save_bin(m->m, path, EMGPU_SRC_HASH);
    return EMGPU_OK;
    EMGPU_CATCH
}
int emgpu_model_load_bin(const char *path, emgpu_model **out) {
    EMGPU_TRY
    if (!path || !out) return fail(EMGPU_ERR_ARG, "null argument");
    std::unique_ptr<Model> m(emgpu::load_bin(path, EMGPU_SRC_HASH));
    emgpu_model *h = new emgpu_model{std::move(*m)};
    *out = h;
    return EMGPU_OK;
    EMGPU_CATCH
}

static std::vector<std::string> split_nl(const char *s) {
    std::vector<std::string> out;
    if (!s) return out;
    std::string cur;
    for (const char *p = s; *p; p++) {
        if (*p == '\n') { out.push_back(cur); cur.clear(); }
        else cur.push_back(*p);
    }
    out.push_back(cur);
    return out;
}

int emgpu_model_from_arrays(const emgpu_model_desc *d, emgpu_model **out) {
    EMGPU_TRY
    if (!d || !out || d->n_initial <= 0 || !d->G_initial || !d->r_initial || !d->N_initial) return fail(EMGPU_ERR_ARG, "null/empty argument");
    if (d->n_initial > EMGPU_MAX_NI) return fail(EMGPU_ERR_UNSUPPORTED, "more initial variables than EMGPU_MAX_NI");
    for (int i = 0; i < d->n_initial; i++)
        if (d->r_initial[i] < 1 || d->r_initial[i] > EMGPU_MAX_R) return fail(EMGPU_ERR_ARG, "r_initial entry outside 1..EMGPU_MAX_R");
    if (d->n_transition > 0) {
        if (d->n_transition < d->n_initial || !d->r_transition) return fail(EMGPU_ERR_ARG, "transition arrays missing");
        for (int i = 0; i < d->n_transition; i++)
            if (d->r_transition[i] < 1 || d->r_transition[i] > EMGPU_MAX_R) return fail(EMGPU_ERR_ARG, "r_transition entry outside 1..EMGPU_MAX_R");
        if (d->n_dyn < 0 || d->n_dyn > d->n_transition - d->n_initial || (d->n_dyn > 0 && !d->temporal_map))
            return fail(EMGPU_ERR_ARG, "n_dyn must be within 0..n_transition-n_initial (with a temporal_map)");
        for (int k = 0; k < d->n_dyn; k++)
            if (d->temporal_map[2 * k] < 1 || d->temporal_map[2 * k] > d->n_initial || d->temporal_map[2 * k + 1] <= d->n_initial ||
                d->temporal_map[2 * k + 1] > d->n_transition)
                return fail(EMGPU_ERR_ARG, "temporal_map row outside (1..n_initial, n_initial+1..n_transition)");
    }
    if (d->boundaries && d->bnd_len)
        for (int i = 0; i < d->n_initial; i++)
            if (d->bnd_len[i] != 0 && d->bnd_len[i] != d->r_initial[i] + 1)
                return fail(EMGPU_ERR_ARG, "bnd_len[i] must be 0 ('*') or r_initial[i] + 1");
    if (d->zero_bins)
        for (int i = 0; i < d->n_initial; i++)
            if (d->zero_bins[i] < 0 || d->zero_bins[i] > d->r_initial[i]) return fail(EMGPU_ERR_ARG, "zero_bins entry outside 0..r");
    std::unique_ptr<emgpu_model> h(new emgpu_model());
    Model &m = h->m;
    const int ni = d->n_initial, nt = d->n_transition;
    m.n_initial = ni;
    m.n_transition = nt;
    m.G_initial.assign(d->G_initial, d->G_initial + (size_t)ni * ni);
    m.r_initial.assign(d->r_initial, d->r_initial + ni);
    m.labels_initial = split_nl(d->labels_initial);
    m.labels_transition = split_nl(d->labels_transition);
    auto q_of = [](const std::vector<uint8_t> &G, int n, const std::vector<int> &r, int c) {
        int64_t q = 1;
        for (int p = 0; p < n; p++) if (G[(size_t)p * n + c]) q *= r[p];
        return q;
    };
    m.N_initial.resize(ni);
    int64_t idx = 0;
    for (int i = 0; i < ni; i++) {
        int64_t cnt = q_of(m.G_initial, ni, m.r_initial, i) * m.r_initial[i];
        if (idx + cnt > d->n_N_initial) return fail(EMGPU_ERR_ARG, "N_initial too short");
        m.N_initial[i].assign(d->N_initial + idx, d->N_initial + idx + cnt);
        idx += cnt;
    }
    if (idx != d->n_N_initial) return fail(EMGPU_ERR_ARG, "N_initial length mismatch");
    if (nt > 0) {
        if (!d->G_transition || !d->r_transition || !d->N_transition || nt < ni) return fail(EMGPU_ERR_ARG, "transition arrays missing");
        m.G_transition.assign(d->G_transition, d->G_transition + (size_t)nt * nt);
        m.r_transition.assign(d->r_transition, d->r_transition + nt);
        m.N_transition.resize(nt);
        idx = 0;
        for (int i = ni; i < nt; i++) {
            int64_t cnt = q_of(m.G_transition, nt, m.r_transition, i) * m.r_transition[i];
            if (idx + cnt > d->n_N_transition) return fail(EMGPU_ERR_ARG, "N_transition too short");
            m.N_transition[i].assign(d->N_transition + idx, d->N_transition + idx + cnt);
            idx += cnt;
        }
        if (idx != d->n_N_transition) return fail(EMGPU_ERR_ARG, "N_transition length mismatch");
        if (d->temporal_map)
            for (int k = 0; k < d->n_dyn; k++) m.temporal_map.push_back({d->temporal_map[2 * k], d->temporal_map[2 * k + 1]});
    }
    m.boundaries.assign(ni, {});
    if (d->boundaries && d->bnd_len) {
        int64_t o = 0;
        for (int i = 0; i < ni; i++) {
            m.boundaries[i].assign(d->boundaries + o, d->boundaries + o + d->bnd_len[i]);
            o += d->bnd_len[i];
        }
    }
    if (d->zero_bins) m.zero_bins.assign(d->zero_bins, d->zero_bins + ni);
    if (d->resample_rates) m.resample_rates.assign(d->resample_rates, d->resample_rates + ni);
    m.finalize();
    *out = h.release();
    return EMGPU_OK;
    EMGPU_CATCH
}

void emgpu_model_free(emgpu_model *m) { delete m; }

int emgpu_model_info(const emgpu_model *h, emgpu_model_info_t *out) {
    if (!h || !out) return fail(EMGPU_ERR_ARG, "null argument");
    const Model &m = h->m;
    memset(out, 0, sizeof *out);
    out->n_initial = m.n_initial;
    out->n_transition = m.n_transition;
    out->n_dyn = m.n_dyn();
    out->is_dynvar_depend = (m.n_transition > 0 && m.n_dyn() > 0) ? (int)m.is_dynvar_depend() : 0;
    for (auto &v : m.N_initial) out->n_N_initial += (int64_t)v.size();
    for (auto &v : m.N_transition) out->n_N_transition += (int64_t)v.size();
    for (int r : m.r_initial) out->max_r = r > out->max_r ? r : out->max_r;
    for (int r : m.r_transition) out->max_r = r > out->max_r ? r : out->max_r;
    for (double r : m.resample_rates) out->n_resample_active += r > 0.0;
    return EMGPU_OK;
}

int64_t emgpu_model_get_i32(const emgpu_model *h, int32_t field, int32_t *out, int64_t cap) {
    if (!h) return fail(EMGPU_ERR_ARG, "null model");
    const Model &m = h->m;
    switch (field) {
    case EMGPU_F_R_INITIAL: return copy_out(m.r_initial, out, cap);
    case EMGPU_F_R_TRANSITION: return copy_out(m.r_transition, out, cap);
    case EMGPU_F_ORDER_INITIAL: return copy_out(m.order_initial, out, cap);
    case EMGPU_F_ORDER_TRANSITION: return copy_out(m.order_transition, out, cap);
    case EMGPU_F_ZERO_BINS: return copy_out(m.zero_bins, out, cap);
    case EMGPU_F_START: return copy_out(m.start, out, cap);
    case EMGPU_F_G_INITIAL: return copy_out(m.G_initial, out, cap);
    case EMGPU_F_G_TRANSITION: return copy_out(m.G_transition, out, cap);
    case EMGPU_F_TEMPORAL_MAP: {
        std::vector<int> f;
        for (auto &t : m.temporal_map) { f.push_back(t[0]); f.push_back(t[1]); }
        return copy_out(f, out, cap);
    }
    default: return fail(EMGPU_ERR_ARG, "unknown i32 field");
    }
}

int64_t emgpu_model_get_f64(const emgpu_model *h, int32_t field, int32_t node, double *out, int64_t cap) {
    if (!h) return fail(EMGPU_ERR_ARG, "null model");
    const Model &m = h->m;
    auto in_range = [&](size_t n) { return node >= 1 && (size_t)node <= n; };
    switch (field) {
    case EMGPU_F_N_INITIAL: if (!in_range(m.N_initial.size())) break; return copy_out(m.N_initial[node - 1], out, cap);
    case EMGPU_F_ALPHA_INITIAL: if (!in_range(m.A_initial.size())) break; return copy_out(m.A_initial[node - 1], out, cap);
    case EMGPU_F_N_TRANSITION: if (!in_range(m.N_transition.size())) break; return copy_out(m.N_transition[node - 1], out, cap);
    case EMGPU_F_ALPHA_TRANSITION: if (!in_range(m.A_transition.size())) break; return copy_out(m.A_transition[node - 1], out, cap);
    case EMGPU_F_BOUNDARIES: if (!in_range(m.boundaries.size())) break; return copy_out(m.boundaries[node - 1], out, cap);
    case EMGPU_F_RESAMPLE_RATES: return copy_out(m.resample_rates, out, cap);
    default: return fail(EMGPU_ERR_ARG, "unknown f64 field");
    }
    return fail(EMGPU_ERR_ARG, "node out of range");
}

int64_t emgpu_model_log_prob(const emgpu_model *h, int32_t network, int32_t node, double *out, int64_t cap) {
    EMGPU_TRY
    if (!h) return fail(EMGPU_ERR_ARG, "null model");
    return copy_out(emgpu::node_log_prob(h->m, network, node), out, cap);
    EMGPU_CATCH
}

int64_t emgpu_model_get_text(const emgpu_model *h, int32_t field, char *out, int64_t cap) {
    if (!h) return fail(EMGPU_ERR_ARG, "null model");
    const std::vector<std::string> *v = field == EMGPU_F_LABELS_INITIAL ? &h->m.labels_initial
                                      : field == EMGPU_F_LABELS_TRANSITION ? &h->m.labels_transition : nullptr;
    if (!v) return fail(EMGPU_ERR_ARG, "unknown text field");
    std::string s;
    for (size_t i = 0; i < v->size(); i++) { if (i) s.push_back('\n'); s += (*v)[i]; }
    if (out) {
        if ((int64_t)s.size() + 1 > cap) return fail(EMGPU_ERR_ARG, "output buffer too small");
        memcpy(out, s.c_str(), s.size() + 1);
    }
    return (int64_t)s.size() + 1;
}

int emgpu_model_set_f64(emgpu_model *h, int32_t field, int32_t node, const double *v, int64_t n) {
    EMGPU_TRY
    if (!h || (!v && n != 0) || n < 0) return fail(EMGPU_ERR_ARG, "null argument or negative length");
    Model &m = h->m;
    auto assign_same = [&](std::vector<std::vector<double>> &dst) {
        if (node < 1 || (size_t)node > dst.size()) throw Error(EMGPU_ERR_ARG, "node out of range");
        if ((int64_t)dst[node - 1].size() != n) throw Error(EMGPU_ERR_ARG, "size mismatch: tables keep their r x q shape");
        dst[node - 1].assign(v, v + n);
    };
    switch (field) {
    case EMGPU_F_N_INITIAL: assign_same(m.N_initial); break;
    case EMGPU_F_N_TRANSITION: assign_same(m.N_transition); break;
    case EMGPU_F_ALPHA_INITIAL: assign_same(m.A_initial); break;
    case EMGPU_F_ALPHA_TRANSITION: assign_same(m.A_transition); break;
    case EMGPU_F_BOUNDARIES:
        if (node < 1 || node > m.n_initial) throw Error(EMGPU_ERR_ARG, "node out of range");
        // numel(boundaries) == r + 1 in every shipped file (dediscretize.m:33-38 reads params(d+1)); 0 = categorical ('*')
        if (n != 0 && n != (int64_t)m.r_initial[node - 1] + 1) throw Error(EMGPU_ERR_ARG, "boundaries need 0 or r+1 entries");
        // (zero_bins is its own property in the reference, derived once by em_read.m:110-114 and not by
        // set.boundaries: use emgpu_model_set_zero_bins to change it)
        m.boundaries[node - 1].assign(v, v + n);
        break;
    case EMGPU_F_RESAMPLE_RATES:
        if (n != m.n_initial) throw Error(EMGPU_ERR_ARG, "resample_rates needs n_initial entries");
        m.resample_rates.assign(v, v + n);
        break;
    default: throw Error(EMGPU_ERR_ARG, "field is not settable");
    }
    m.version++;
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_model_set_prior(emgpu_model *h, int32_t kind, double value) {
    EMGPU_TRY
    if (!h) return fail(EMGPU_ERR_ARG, "null model");
    if (kind != 0 && kind != 1) return fail(EMGPU_ERR_PRIOR, "Unknown prior, if char expecting prior = 'dbe'");
    h->m.set_prior(kind, value);
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_model_set_transition_stay_prior(emgpu_model *h, double prior) {
    EMGPU_TRY
    if (!h) return fail(EMGPU_ERR_ARG, "null model");
    h->m.set_transition_stay_prior(prior);
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_model_set_start(emgpu_model *h, const int32_t *start, int32_t n) {
    if (!h || !start || n != h->m.n_initial) return fail(EMGPU_ERR_ARG, "start needs n_initial entries");
    for (int i = 0; i < n; i++)
        if (start[i] < 0 || start[i] > h->m.r_initial[i]) return fail(EMGPU_ERR_ARG, "start bin out of range");
    h->m.start.assign(start, start + n);
    h->m.version++;
    return EMGPU_OK;
}

int emgpu_model_start_log_weight(const emgpu_model *h, double *out) {
    EMGPU_TRY
    if (!h || !out) return fail(EMGPU_ERR_ARG, "null argument");
    *out = h->m.start_log_weight();
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_start_grid_log_weight(const emgpu_model *h, const int32_t *start, int64_t n, double *out) {
    EMGPU_TRY
    if (!h || n < 0 || (n > 0 && (!start || !out))) return fail(EMGPU_ERR_ARG, "null argument or n < 0");
    emgpu::start_grid_log_weight(h->m, start, n, out);
    return EMGPU_OK;
    EMGPU_CATCH
}

int emgpu_model_set_zero_bins(emgpu_model *h, const int32_t *zero_bins, int32_t n) {
    if (!h || !zero_bins || n != h->m.n_initial) return fail(EMGPU_ERR_ARG, "zero_bins needs n_initial entries");
    for (int i = 0; i < n; i++)
        if (zero_bins[i] < 0 || zero_bins[i] > h->m.r_initial[i]) return fail(EMGPU_ERR_ARG, "zero bin out of range");
    h->m.zero_bins.assign(zero_bins, zero_bins + n);
    h->m.version++;
    return EMGPU_OK;
}

int emgpu_shard_range(int64_t n_total, int32_t rank, int32_t world, int64_t *lo, int64_t *hi) {
    if (n_total < 0 || world < 1 || rank < 0 || rank >= world || !lo || !hi) return fail(EMGPU_ERR_ARG, "bad shard arguments");
    const int64_t base = n_total / world, rem = n_total % world;
    *lo = rank * base + (rank < rem ? rank : rem);
    *hi = *lo + base + (rank < rem ? 1 : 0);
    return EMGPU_OK;
}

int emgpu_device_count(int32_t *count) {
    if (!count) return fail(EMGPU_ERR_ARG, "null argument");
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    *count = c;
    return EMGPU_OK;
}

int32_t emgpu_mixed_blocks(int64_t n_total, int32_t n_models, int64_t lo, int64_t hi, emgpu_block *blocks) {
    if (n_total < 0 || n_models < 1 || !blocks || lo < 0 || hi > n_total) return fail(EMGPU_ERR_ARG, "bad block arguments");
    int32_t k = 0;
    for (int32_t m = 0; m < n_models; m++) {
        int64_t a, b;
        emgpu_shard_range(n_total, m, n_models, &a, &b);
        const int64_t a2 = a > lo ? a : lo, b2 = b < hi ? b : hi;
        if (b2 > a2) blocks[k++] = emgpu_block{m, 0, (uint64_t)a2, b2 - a2};
    }
    return k;
}

int32_t emgpu_discretize_bayes(double x, const double *thresholds, int32_t n) {
    // discretize_bayes.m:17-21
    if (n <= 0 || !thresholds) return 1;
    if (x >= thresholds[n - 1]) return n + 1;
    for (int i = 0; i < n; i++)
        if (x < thresholds[i]) return i + 1;
    return n + 1;
}

int64_t emgpu_asub2ind(const int32_t *siz, const int32_t *x, int32_t n) {
    // asub2ind.m:13-14
    int64_t k = 1, ndx = 1;
    for (int i = 0; i < n; i++) { ndx += k * (int64_t)(x[i] - 1); k *= siz[i]; }
    return ndx;
}

} // extern "C"
