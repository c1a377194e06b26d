// ntt_plan.hpp -- host planning of the Fr transforms (msm_fr_ntt; kernels in
// fr_ntt.hip).  Plain C++, no HIP: abi.cpp's msm_ntt_plan() and the CPU tests
// use it without a device.
//
// A transform of n = 2^log_n elements is a sequence of Stockham passes.  Pass
// i has radix R_i = 2^k_i; with s = R_1 .. R_(i-1) and m = n / (s R_i) it maps
//   y[q + s (R_i p + k)] = w_(n/s)^(p k) sum_j x[q + s p + (n / R_i) j] w_(R_i)^(j k)
// (q < s, p < m), so every pass reads and writes natural order and no pass
// exists only to permute.  A workgroup holds a TILE of 2^t elements in LDS:
// R_i rows of C adjacent columns (q + s p consecutive), which makes every
// global run C x 32 bytes long.  One pass covers n <= 2^t (C = 1, the run is
// the transform).  Longer transforms take C = 4 (128-byte runs) and radices of
// at most 2^(t - 2), balanced over the fewest passes.
#pragma once
#include <stddef.h>

#include <vector>

#include "env_size.hpp"

namespace msm {

constexpr int NTT_MAX_LOG = 26;
constexpr int NTT_TILE_DEFAULT = 10, NTT_TILE_MIN = 2, NTT_TILE_MAX = 11;
constexpr size_t NTT_CHUNK_DEFAULT = (size_t)1 << 20;  // elements (32 MiB) per chunk

// log2 of the tile: MSM_NTT_TILE=<log2> in 2..11 overrides the default, read at each call
inline int ntt_tile() {
  const size_t e = env_size("MSM_NTT_TILE");
  return e >= (size_t)NTT_TILE_MIN && e <= (size_t)NTT_TILE_MAX ? (int)e : NTT_TILE_DEFAULT;
}
// elements per chunk: MSM_NTT_CHUNK=<elements> overrides the default, read at each call
inline size_t ntt_chunk() {
  const size_t e = env_size("MSM_NTT_CHUNK");
  return e ? e : NTT_CHUNK_DEFAULT;
}
// log2 of the columns of a tile in a transform of several passes (tiles below
// 2^4 exist for the tests: they keep two columns, 64-byte runs)
inline int ntt_cols_log(int tile) { return tile >= 4 ? 2 : 1; }

// log2 of the radix of every pass, in order (empty for log_n = 0: a copy)
inline std::vector<int> ntt_plan(int log_n, int tile) {
  std::vector<int> r;
  if (log_n <= 0) return r;
  if (log_n <= tile) {
    r.push_back(log_n);
    return r;
  }
  const int cap = tile - ntt_cols_log(tile);
  const int np = (log_n + cap - 1) / cap;
  for (int i = 0; i < np; ++i) r.push_back(log_n / np + (i < log_n % np ? 1 : 0));
  return r;
}

}  // namespace msm
