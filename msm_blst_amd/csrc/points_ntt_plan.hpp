// points_ntt_plan.hpp -- the schedule of the NTT over group elements
// (points_ntt.hip; msm_points_ntt).  Plain C++, no HIP include: the kernels, the
// engine's host loop and the host model of the C ABI (points_ntt_model.hpp, Fr
// elements in place of points) all call the functions below, and nothing else
// knows the schedule.
//
// A transform of n = 2^log_n elements is a radix-2 decimation in frequency, in
// place on a working array x, as a list of PASSES:
//   pass p < log_n       the butterfly level of span h = n >> (p + 1): butterfly t
//                        < n / 2 pairs a and b = a + h, a = (t / h) 2h + t mod h,
//                        x[a] <- x[a] + x[b], x[b] <- [omega_n^e](x[a] - x[b]) with
//                        e = (a mod h) (n / 2h).  At h = 1 every e is 0: the level
//                        multiplies nothing.
//   pass log_n (inverse) every element times n^-1: item t < n is x[t], its
//                        "exponent" is n / 2, the slot after the n / 2 twiddles
//                        where the twiddle table keeps n^-1.
// The DIF leaves X[k] at x[bitrev(k)].  The inverse transform is the forward one
// read at (n - j) mod n, so one table of omega_n^e, e < n / 2, serves both.
//
// The four flag combinations only differ in two maps:
//   pn_in_map(i)   the source position whose element starts at x[i]
//   pn_out_map(q)  the index of x that holds the result written at position q
//
// Sizes: a call is cut into chunks of whole transforms; the items of a pass over
// all transforms of a chunk form one index space g = transform * items + t, cut
// into slices that run one after another.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "env_size.hpp"

// (the MSM_FN style of fp.hpp, for the host AND the kernels of one translation unit)
#ifdef __HIP__
#define PN_FN __host__ __device__ inline
#else
#define PN_FN inline
#endif

namespace msm {

constexpr int PN_MAX_LOG = 24;
constexpr int PN_INVERSE = 1, PN_BITREV = 8;  // MSM_NTT_INVERSE, MSM_POLY_BITREV
constexpr size_t PN_CHUNK_DEFAULT = (size_t)1 << 20;  // points
constexpr size_t PN_SLICE_DEFAULT = (size_t)1 << 18;  // items (butterflies) of a launch

PN_FN size_t pn_bitrev(size_t v, int log_n) {
  size_t r = 0;
  for (int i = 0; i < log_n; ++i) r |= ((v >> i) & 1) << (log_n - 1 - i);
  return r;
}

// ---- passes ----
PN_FN int pn_passes(int log_n, int flags) { return log_n + ((flags & PN_INVERSE) && log_n ? 1 : 0); }
PN_FN bool pn_is_scale(int log_n, int pass) { return pass == log_n; }
// items of one transform in a pass, as a shift
PN_FN int pn_items_log(int log_n, int pass) { return pn_is_scale(log_n, pass) ? log_n : log_n - 1; }
// does the pass multiply (a table, its rows and a ladder)?  The last level does not.
PN_FN bool pn_laddered(int log_n, int pass) { return pn_is_scale(log_n, pass) || pass < log_n - 1; }

// item t of a pass: b, the element that is multiplied (and for a level a = b - h,
// its partner), and the index e of its scalar in the twiddle table
struct PnItem {
  size_t a, b, e;
};
PN_FN PnItem pn_item(int log_n, int pass, size_t t) {
  PnItem it;
  if (pn_is_scale(log_n, pass)) {
    it.a = it.b = t;
    it.e = ((size_t)1 << log_n) >> 1;
    return it;
  }
  const int hl = log_n - 1 - pass;  // log2 of the span
  const size_t h = (size_t)1 << hl, r = t & (h - 1);
  it.a = ((t >> hl) << (hl + 1)) + r;
  it.b = it.a + h;
  it.e = r << pass;  // (a mod h) (n / 2h)
  return it;
}
// entries of the twiddle table: omega_n^e for e < n / 2, then n^-1
PN_FN size_t pn_twiddles(int log_n) { return (((size_t)1 << log_n) >> 1) + 1; }

// ---- maps ----
PN_FN size_t pn_in_map(int log_n, int flags, size_t i) {
  // the forward transform under BITREV reads its element i at position bitrev(i)
  return ((flags & PN_BITREV) && !(flags & PN_INVERSE)) ? pn_bitrev(i, log_n) : i;
}
PN_FN size_t pn_out_map(int log_n, int flags, size_t q) {
  const size_t n = (size_t)1 << log_n;
  if (!(flags & PN_INVERSE)) return pn_bitrev(q, log_n);  // X[q] sits at x[bitrev(q)]
  // result j of the inverse is X[(n - j) mod n]; under BITREV it is written at bitrev(j)
  const size_t j = (flags & PN_BITREV) ? pn_bitrev(q, log_n) : q;
  return pn_bitrev((n - j) & (n - 1), log_n);
}

// ---- sizes (both overrides are read at each call) ----
inline size_t pn_chunk() {
  const size_t e = env_size("MSM_POINTS_NTT_CHUNK");
  return e ? e : PN_CHUNK_DEFAULT;
}
inline size_t pn_slice() {
  const size_t e = env_size("MSM_POINTS_NTT_SLICE");
  return e ? e : PN_SLICE_DEFAULT;
}
// whole transforms per chunk: a transform longer than the chunk is a chunk of its own
inline size_t pn_chunk_transforms(int log_n, size_t batch, size_t chunk) {
  const size_t t = chunk >> log_n;
  return t < 1 ? 1 : (t > batch ? batch : t);
}
// items of the largest slice of any laddered pass over `transforms` transforms (the size of the table buffers)
inline size_t pn_slice_items(int log_n, int flags, size_t transforms, size_t slice) {
  size_t m = 0;
  for (int p = 0; p < pn_passes(log_n, flags); ++p) {
    if (!pn_laddered(log_n, p)) continue;
    const size_t items = transforms << pn_items_log(log_n, p);
    const size_t s = items < slice ? items : slice;
    if (s > m) m = s;
  }
  return m;
}

}  // namespace msm
