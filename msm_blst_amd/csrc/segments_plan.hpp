// segments_plan.hpp -- host planning of the segmented sums and MSMs
// (msm_points_msm_segments; kernels in point_segments.hip).  Plain C++, no HIP:
// abi.cpp's msm_segments_plan() and the CPU tests use it without a device.
//
// The points of segment j are offsets[j] <= i < offsets[j + 1].  They are cut
// into PIECES: at most L consecutive points of ONE segment.  One lane (G2: one
// lane pair) of the hot kernel sums one piece; the doublings of its Straus
// ladder are shared by the points of the piece.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "env_size.hpp"

namespace msm {

constexpr size_t SEG_PIECE_MAX = 64;
// lanes that are resident at once at the register budget of the hot kernel:
// 256 CUs x 4 SIMDs x 2 waves x 64 lanes; a G2 piece takes a lane pair
constexpr size_t SEG_LANES = (size_t)256 * 4 * 2 * 64;
// device bytes a chunk allocates per point: the 8 table rows (112 G each), the 7
// xyzz multiples (224 G; the partials reuse them), a segment result (224 G), and
// the level buffers of the inversion trees (7 x 56 G x 8/7 x 1/8, rounded up)
constexpr size_t SEG_POINT_BYTES = 8 * 112 + 7 * 224 + 224 + 72;
constexpr size_t SEG_CHUNK_BUDGET = (size_t)3 << 30;  // bytes of the above per chunk

// points (and segments written) per chunk: MSM_POINTS_SEGMENTS_CHUNK=<points>
// overrides the default, read at each call
inline size_t seg_chunk(int group) {
  const size_t e = env_size("MSM_POINTS_SEGMENTS_CHUNK");
  return e ? e : SEG_CHUNK_BUDGET / (SEG_POINT_BYTES * (size_t)group);
}

// The piece length for m points in flight.  A piece of L points pays the 4
// doublings of a window once instead of L times, but the chip wants pieces to
// fill its lanes: L is the longest that still leaves a piece for every resident
// lane (pair), clamped to [1, SEG_PIECE_MAX].  Measured at 2^20 points (DESIGN
// 18): one piece per lane beats two (the rule this started from) by about 15 %
// on G1 and 11 % on G2, and half a piece per lane loses to both.
// MSM_POINTS_SEGMENTS_PIECE=<points> overrides it, read at each call.
inline size_t seg_piece_len(size_t m, int group) {
  const size_t e = env_size("MSM_POINTS_SEGMENTS_PIECE");
  if (e) return std::min(e, SEG_PIECE_MAX);
  const size_t lanes = SEG_LANES / (size_t)group;
  return std::min(std::max(m / lanes, (size_t)1), SEG_PIECE_MAX);
}

// The pieces of the points lo <= i < hi (o[0] <= lo <= hi <= o[k]), in order;
// j: a segment at or before the one that holds lo.  emit(start, count, segment)
// is called per piece; returns their number.  Empty segments have none.
template <class Emit>
inline size_t seg_cut(const size_t *o, size_t k, size_t L, size_t lo, size_t hi, size_t j, Emit emit) {
  size_t np = 0;
  for (; j < k && o[j] < hi; ++j) {
    const size_t a = std::max(o[j], lo), b = std::min(o[j + 1], hi);
    for (size_t s = a; s < b; s += L, ++np) emit(s, std::min(L, b - s), j);
  }
  return np;
}

// offsets must be non-decreasing (o[0] >= 0 holds for size_t)
inline bool seg_offsets_ok(const size_t *o, size_t k) {
  for (size_t j = 0; j < k; ++j)
    if (o[j + 1] < o[j]) return false;
  return true;
}

}  // namespace msm
