// emgpu_pairs.h -- the pairing of two sets of 1 Hz tracks, once: what k_miss_distance (emgpu_miss.h) and k_encounter_pose (emgpu_encounter.h)
// mean by "pair i".  Both argument blocks open with EmgpuPairDims and carry EmgpuPairCols; emgpu_pairs.cpp checks and fills them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

// The pairing (include/emgpu.h).  Set X (A or B) is xyz f64 PLANAR [P][3][ld_x] in feet, n_x columns of pitch ld_x.  Pair i of n_pairs
// takes column ia of set A and column ib of set B: idx_x[i] where idx_x is given; without idx_x, i when n_x > 1, else 0 (one ownship
// against every intruder).  A pair whose ia is outside 0 .. n_a-1 or whose ib is outside 0 .. n_b-1 is a bad pair: it loads nothing and
// its outputs say so (the BAD_INDEX flag of either kernel).
struct EmgpuPairDims {
    int64_t n_pairs, n_a, n_b, ld_a, ld_b;
};
struct EmgpuPairCols {
    const double *xyz_a, *xyz_b;
    const int64_t *idx_a, *idx_b;   // [n_pairs] or null
};

// the column of set X (n columns) that pair i takes
__device__ __forceinline__ int64_t pair_column(const int64_t *idx, int64_t n, int64_t i) { return idx ? idx[i] : (n > 1 ? i : 0); }

// The grid of both kernels, one lane per pair: min(tiles, 2048) workgroups of `block` lanes (k_miss_distance pays its atomics once per
// workgroup) that walk the tiles of `block` pairs, tile j of workgroup w being w + j * gridDim.x.
inline dim3 pair_grid(int64_t n_pairs, int block) { return dim3((unsigned)std::min<int64_t>((n_pairs + block - 1) / block, 2048)); }
