// segments_plan.hpp -- host planning of the segmented sums and MSMs
// (msm_points_msm_segments; kernels in point_segments.hip) and of the bulk
// pairings (pairing.hip), which cut their calls the same way.  Plain C++, no
// HIP: abi.cpp's msm_segments_plan() and the CPU tests use it without a device.
//
// The points of segment j are offsets[j] <= i < offsets[j + 1].  They are cut
// into PIECES: at most L consecutive points of ONE segment.  One lane (G2: one
// lane pair) of the hot kernel sums one piece; the doublings of its Straus
// ladder are shared by the points of the piece.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

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

// ---- the chunks of a call (point_segments.hip, pairing.hip) ----
// A call is cut into chunks of at most C points that write at most C segments.
// A chunk boundary may fall inside a segment: what the chunk summed of the open
// segment is carried into the next chunk as one more partial, in front of that
// chunk's pieces.  The partials of one segment lie side by side (a run).

// what a lane (pair) of the kernels knows about its partial
struct SegMeta {
  uint32_t start, count;  // the piece: first point (relative to the chunk) and points; the carried partial has none
  uint32_t rel, len;      // position in the run of partials of its segment, and the length of that run
};

// the sizes of a call of `total` points in k segments at `chunk` points per chunk
struct SegSizes {
  size_t C;     // bounds the points AND the segments written per chunk (a chunk of empty segments has no points)
  size_t CP;    // points of a chunk
  size_t pmax;  // partials of a chunk: a piece per point where every segment is short, and the carry
  size_t META;  // bytes of a plan: pmax entries, then a source per segment written
};
inline SegSizes seg_sizes(size_t total, size_t k, size_t chunk) {
  SegSizes z;
  z.C = std::min(std::max(total, k), std::min(chunk, (size_t)1 << 30));
  z.CP = std::min(z.C, std::max(total, (size_t)1));
  z.pmax = z.CP + 1;
  z.META = z.pmax * sizeof(SegMeta) + z.C * sizeof(uint32_t);
  return z;
}

// begin(), then next() per chunk until it returns false.  The vectors are
// reused from chunk to chunk and from call to call.
class SegPlanner {
 public:
  // ---- the chunk that the last next() planned ----
  size_t i = 0, e = 0;               // its points [i, e)
  size_t j = 0, je = 0;              // segments [j, je) end in it and are written
  uint32_t pc = 0;                   // 1: meta[0] is the partial carried in (points o[j] .. i - 1 of segment j)
  std::vector<SegMeta> meta;         // its partials: the carried one, then a piece each
  std::vector<uint32_t> src;         // per segment written: the partial that starts its run, or ~0 (empty)
  size_t maxrun = 0;                 // the longest run
  size_t open_src = ~(size_t)0;      // the partial that starts the run of the segment left open, or ~0
  size_t cnt() const { return e - i; }
  size_t nseg() const { return je - j; }
  size_t np() const { return meta.size(); }
  size_t npieces() const { return meta.size() - pc; }
  bool carry() const { return open_src != ~(size_t)0; }  // a partial leaves the chunk

  // o: k + 1 offsets; L: the piece length; who: the engine, for the error text
  void begin(const size_t *o, size_t k, const SegSizes &z, size_t L, const char *who) {
    o_ = o, k_ = k, z_ = z, L_ = L, who_ = who;
    i = e = o[0], j = je = 0, open_src = ~(size_t)0;
  }
  bool next() {
    i = e, j = je;  // first point not yet summed, first segment not yet written
    if (j >= k_) return false;
    pc = carry() ? 1 : 0;
    e = std::min(i + z_.C, o_[k_]);
    while (je < k_ && o_[je + 1] <= e && je - j < z_.C) ++je;
    if (je < k_ && o_[je + 1] <= e) e = o_[je];  // C segments already: stop where the last of them ends
    meta.clear();
    src.assign(je - j, ~0u);
    if (pc) meta.push_back(SegMeta{0, 0, 0, 0});
    run0_ = 0, runseg_ = j, maxrun = 0, open_src = ~(size_t)0;
    seg_cut(o_, k_, L_, i, e, j, [&](size_t s, size_t c, size_t seg) {
      if (seg != runseg_) {
        close_run(meta.size());
        runseg_ = seg;
      }
      meta.push_back(SegMeta{(uint32_t)(s - i), (uint32_t)c, 0, 0});
    });
    close_run(meta.size());
    if (np() > z_.pmax || nseg() > z_.C || cnt() > z_.CP)
      throw std::runtime_error(std::string(who_) + ": plan larger than its buffers");
    return true;
  }

 private:
  const size_t *o_ = nullptr;
  size_t k_ = 0, L_ = 1, run0_ = 0, runseg_ = 0;
  SegSizes z_{};
  const char *who_ = "";
  void close_run(size_t end) {  // partials [run0_, end) belong to segment runseg_
    for (size_t p = run0_; p < end; ++p) meta[p].rel = (uint32_t)(p - run0_), meta[p].len = (uint32_t)(end - run0_);
    if (end > run0_) {
      maxrun = std::max(maxrun, end - run0_);
      if (runseg_ < je) src[runseg_ - j] = (uint32_t)run0_;
      else open_src = run0_;
    }
    run0_ = end;
  }
};

}  // namespace msm
