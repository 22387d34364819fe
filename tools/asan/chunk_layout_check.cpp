// AddressSanitizer / UBSan harness (CPU build, nothing of HIP is called): chunk_layout of emgpu_tracechunk.hpp for the four chunked trace
// entry points, beside the formulas each of them carried itself before the layout had one owner, evaluated literally.  c and every offset
// must be equal; the block may be larger by the 256-byte tail alone.  Prints one line per case; exit status 1 on the first difference.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I /opt/rocm/include \
//       -I em_model_manned_bayes_amd/csrc tools/asan/chunk_layout_check.cpp -o chunk_layout_check && ./chunk_layout_check
#include <cstdio>
#include <vector>

#include "emgpu_tracechunk.hpp"

using emgpu_detail::ChunkLayout;
using emgpu_detail::chunk_layout;
using emgpu_detail::round_up;

namespace {
struct Old { int64_t c; std::vector<size_t> off; size_t total; };
int64_t old_c(int64_t n, size_t target, size_t per_lane) {
    return (int64_t)std::min<size_t>(round_up((size_t)n, 256), std::max<size_t>(target / per_lane / 256 * 256, 256));
}
Old old_score(int64_t n, size_t target, size_t ni, size_t rows_d) {
    const size_t per_lane = ni + 4 * rows_d + 16;
    const int64_t c = old_c(n, target, per_lane);
    const size_t o_dyn = round_up(ni * (size_t)c, 256), o_ll = o_dyn + round_up(4 * rows_d * (size_t)c, 256), o_in = o_ll + 8 * (size_t)c;
    return {c, {0, o_dyn, o_ll, o_in}, o_in + 8 * (size_t)c};
}
Old old_count(int64_t n, size_t target, size_t ni, size_t rows_d) {
    const size_t per_lane = ni + 4 * rows_d;
    const int64_t c = old_c(n, target, per_lane);
    const size_t o_dyn = round_up(ni * (size_t)c, 256);
    return {c, {0, o_dyn}, o_dyn + round_up(4 * rows_d * (size_t)c, 256) + 256};
}
Old old_discretize(int64_t n, size_t target, size_t ni, size_t rows_d, size_t es) {
    const size_t per_lane = ni * (es + 1) + rows_d * (4 * es + 4);
    const int64_t c = old_c(n, target, per_lane);
    const size_t o_dv = round_up(ni * es * (size_t)c, 256), o_ib = o_dv + round_up(4 * es * rows_d * (size_t)c, 256);
    const size_t o_db = o_ib + round_up(ni * (size_t)c, 256), total = o_db + round_up(4 * rows_d * (size_t)c, 256) + 256;
    return {c, {0, o_dv, o_ib, o_db}, total};
}
Old old_trackval(int64_t n, size_t target, size_t P, size_t ni, size_t rows_d, size_t es) {
    const size_t per_lane = 24 * P + ni * es + rows_d * 4 * es;
    const int64_t c = old_c(n, target, per_lane);
    const size_t o_iv = round_up(24 * P * (size_t)c, 256), o_dv = o_iv + round_up(ni * es * (size_t)c, 256);
    return {c, {0, o_iv, o_dv}, o_dv + round_up(4 * es * rows_d * (size_t)c, 256) + 256};
}

int bad = 0;
void compare(const char *what, int64_t n, size_t target, const Old &o, const ChunkLayout &L) {
    bool same = o.c == L.c && (L.bytes == o.total || L.bytes == o.total + 256);
    printf("%-34s n %7lld target %10zu | c %7lld %7lld | off", what, (long long)n, target, (long long)o.c, (long long)L.c);
    for (size_t k = 0; k < o.off.size(); k++) {
        printf(" %zu/%zu", o.off[k], L.off[k]);
        same = same && o.off[k] == L.off[k];
    }
    printf(" | bytes %zu %zu %s\n", o.total, L.bytes, same ? "ok" : "DIFFERENT");
    bad += !same;
}
} // namespace

int main() {
    const size_t MiB = (size_t)1 << 20, ni = 7, nd = 3;   // uncor_1200code_v2p1
    const size_t targets[] = {1 * MiB, 256 * MiB};         // the tests' EMGPU_HOST_CHUNK_MB = 1, and the default
    // n: 1, 255, 256, 257, and those of tests/test_gpu_trace_chunks.py (2 c + 89 at each shape's c under 1 MiB)
    const int64_t ns[] = {1, 255, 256, 257, 601, 1113, 2137, 9817, 10329, 91225, 299609, 1000000};
    for (size_t target : targets)
        for (int64_t n : ns) {
            for (size_t T : {1, 5, 61, 240}) {
                const size_t G4 = (T + 3) / 4;
                for (size_t rows_d : {(size_t)0, T > 1 ? G4 * nd : 0}) {
                    compare("score", n, target, old_score(n, target, ni, rows_d), chunk_layout(n, target, {{1, ni}, {4, rows_d}, {8, 1}, {8, 1}}));
                    compare("count", n, target, old_count(n, target, ni, rows_d), chunk_layout(n, target, {{1, ni}, {4, rows_d}}));
                }
                for (size_t es : {4, 8})
                    for (int half = 1; half < 4; half++) {   // the initial half alone, the dynamic half alone, both
                        const size_t a = half & 1 ? ni : 0, d = half & 2 ? G4 * nd : 0;
                        compare(es == 4 ? "discretize f32" : "discretize f64", n, target, old_discretize(n, target, a, d, es),
                                chunk_layout(n, target, {{es, a}, {4 * es, d}, {1, a}, {4, d}}));
                    }
            }
            for (size_t P : {3, 62, 242})
                for (size_t es : {4, 8})
                    for (int half = 1; half < 4; half++) {
                        const size_t a = half & 1 ? 5 : 0, d = half & 2 ? 3 * ((P - 2 + 3) / 4) : 0;
                        compare(es == 4 ? "track values f32" : "track values f64", n, target, old_trackval(n, target, P, a, d, es),
                                chunk_layout(n, target, {{24 * P, 1}, {es, a}, {4 * es, d}}));
                    }
        }
    printf(bad ? "%d cases DIFFERENT\n" : "all equal (%d)\n", bad);
    return bad ? 1 : 0;
}
