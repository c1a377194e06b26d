// ches_setup.hpp -- the group-independent host setup of the CHES "nh + q/5"
// bucket-set method (ches.hip): parameters of ref ches_config_files, bucket set
// B (ref auxiliaryfunc.h:257-288), digit hash (ref main_p1.cpp:140-152) and its
// compact device form.  Plain C++, no HIP: the engines, the C ABI and the CPU
// test of the reduction plan (tests/test_reduce_plan_host.py) share it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

namespace msm {

// parameters of ref ches_config_files/config_file_n_exp_*.h
struct ChesParams {
  int n_exp, beta, q_exp, h, a_h, d_max, b_size, q_exp_bgmw, h_bgmw;
};

// bits 0..23 of a packed digit-hash entry: the bucket's index in B (CH_IDX_MASK, ches_kernels.hpp)
constexpr uint32_t kChesHashIdxMask = 0x00ffffffu;

// ------------------------------------------------------------- parameters --
// values of ref ches_config_files/config_file_n_exp_{8..21}.h and the _beta
// variants (n_exp, beta, q exponent, h, a_h, d_max, |B|, BGMW95 q exponent, h)
inline const ChesParams kChesTable[] = {
    {8, 0, 12, 22, 7, 6, 857, 10, 26},         {9, 0, 13, 20, 231, 6, 1725, 11, 24},
    {10, 0, 13, 20, 231, 6, 1725, 12, 22},     {11, 0, 14, 19, 7, 6, 3417, 13, 20},
    {12, 0, 14, 19, 7, 6, 3417, 13, 20},       {13, 0, 16, 16, 29677, 6, 18343, 15, 17},
    {14, 0, 16, 16, 29677, 6, 18343, 15, 17},  {15, 0, 16, 16, 29677, 6, 18343, 16, 16},
    {16, 0, 19, 14, 231, 6, 109244, 17, 15},   {16, 1, 18, 15, 7, 6, 54618, 17, 15},
    {17, 0, 20, 13, 29677, 6, 220931, 17, 15}, {17, 1, 19, 14, 231, 6, 109244, 17, 15},
    {18, 0, 20, 13, 29677, 6, 220931, 19, 14}, {19, 0, 20, 13, 29677, 6, 220931, 20, 13},
    {20, 0, 22, 12, 7419, 6, 874437, 20, 13},  {20, 1, 20, 13, 29677, 6, 220931, 20, 13},
    {21, 0, 22, 12, 7419, 6, 874437, 22, 12},
};

inline bool ches_params_for(int n_exp, int beta, ChesParams *out) {
  for (const ChesParams &p : kChesTable)
    if (p.n_exp == n_exp && p.beta == beta) {
      *out = p;
      return true;
    }
  return false;
}

// omega2(v) + omega3(v) even  (ref auxiliaryfunc.h:217-255)
inline bool even23(int v) {
  int e = 0;
  while (v % 2 == 0) v /= 2, ++e;
  while (v % 3 == 0) v /= 3, ++e;
  return (e & 1) == 0;
}

// bucket set B of ref auxiliaryfunc.h:257-288 (ascending): {0,1} u {i <= q/2 :
// even23(i)}, then the two pruning passes (membership tested as the passes run,
// as std::set::erase does there), then every even23 value <= a_h + 1 re-inserted.
inline std::vector<int> ches_bucket_set(int q, int a_h) {
  size_t lim = std::max<size_t>((size_t)q / 2 + 1, (size_t)a_h + 2);
  std::vector<uint8_t> in(lim, 0);
  in[0] = in[1] = 1;
  for (int i = 2; i <= q / 2; ++i) in[i] = even23(i);
  for (int i = q / 4; i < q / 2; ++i) {
    int t = q - 2 * i;
    if (in[i] && t >= 0 && (size_t)t < lim && in[t]) in[t] = 0;
  }
  for (int i = q / 6; i < q / 4; ++i) {
    int t = q - 3 * i;
    if (in[i] && t >= 0 && (size_t)t < lim && in[t]) in[t] = 0;
  }
  for (int i = 1; i <= a_h + 1; ++i)
    if (even23(i)) in[i] = 1;
  std::vector<int> B;
  for (size_t v = 0; v < lim; ++v)
    if (in[v]) B.push_back((int)v);
  return B;
}

// packed digit hash (ches_kernels.hpp layout), q + 1 entries.  ref
// main_p1.cpp:140-152: every (m, b) writes H[q - m b] = (m, b, alpha=1), then
// H[m b] = (m, b, 0); later writes win.
inline std::vector<uint32_t> ches_digit_hash(const std::vector<int> &B, int q) {
  std::vector<uint32_t> H((size_t)q + 1, 0);
  for (int alpha = 1; alpha >= 0; --alpha)
    for (int m = 1; m <= 3; ++m)
      for (size_t i = 0; i < B.size(); ++i) {
        long mb = (long)m * B[i];
        if (mb > q) continue;
        size_t d = alpha ? (size_t)(q - mb) : (size_t)mb;
        H[d] = (uint32_t)i | ((uint32_t)(m - 1) << 24) | ((uint32_t)alpha << 31);
      }
  return H;
}

// The same map in the compact device form (ches_kernels.hpp "digit code"):
// a 4-bit code per digit value, 8 per word, (q >> 3) + 2 words, and the rank
// table {membership bits, prefix count} per 32 values of [0, max B].  Throws if
// some H[d] is not (m, (alpha ? q - d : d) / m, alpha).
inline void ches_digit_code(const std::vector<int> &B, int q, std::vector<uint32_t> &code,
                            std::vector<uint32_t> &rank) {
  const std::vector<uint32_t> H = ches_digit_hash(B, q);
  code.assign(((size_t)q >> 3) + 2, 0);
  for (size_t d = 0; d <= (size_t)q; ++d) {
    const uint32_t m = ((H[d] >> 24) & 3u) + 1, alpha = H[d] >> 31;
    const int b = B[H[d] & kChesHashIdxMask];
    uint32_t c = (m - 1) | (alpha << 2);
    if (b == 0) {
      c |= 8u;  // bucket value 0: entry skipped
    } else {
      const long v = alpha ? (long)q - (long)d : (long)d;
      if (v % m != 0 || v / m != b) throw std::runtime_error("CHES digit map is not arithmetic at d=" + std::to_string(d));
    }
    code[d >> 3] |= c << (4 * (d & 7));
  }
  const size_t words = ((size_t)B.back() >> 5) + 1;
  rank.assign(2 * words, 0);
  for (int v : B) rank[2 * ((size_t)v >> 5)] |= 1u << (v & 31);
  uint32_t run = 0;
  for (size_t w = 0; w < words; ++w) {
    rank[2 * w + 1] = run;
    run += (uint32_t)__builtin_popcount(rank[2 * w]);
  }
}

}  // namespace msm
