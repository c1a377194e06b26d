// reduce_plan.hpp -- the weighted bucket reduction (WeightedReducer, engine.hpp)
// as a plan in plain vectors and numbers: the index tables of every level of
// segment sums, and the steps of one reduction with their buffers and strides.
// Plain C++, no HIP: the reducer uploads the tables and turns every step into
// one launch, the CPU test walks the same steps over integers with every buffer
// at exactly the planned size (tests/test_reduce_plan_host.py).  DESIGN 30.
//
// sum_i w_i S_i = sum_u u L_u + 2^s sum_v v H_v  with u = w_i mod 2^s,
// v = w_i >> s, L_u = sum_{i: low(w_i) = u} S_i, H_v = sum_{i: high(w_i) = v} S_i.
// L and H are segment sums over one list of bucket indices (level 0: chunks of
// <= C within a segment; then pairwise levels until one partial per segment;
// then a dense scatter into 2 blocks of 2^s slots per window).  The reduction
// ends in the dense stage (ScanReducer: T = sum_b b A_b per block, and one 2^s
// Horner step on the host) or, for one-window plans, in bit sums: B_j = sum of
// the partials whose value has bit j (j < s: low half, then the high half), the
// same chunk / pairwise / scatter levels over the final partials, ~log2(2^s s /
// 8) + 2 levels instead of the dense stage's 2 s, and T = sum_j 2^j B_j on the
// host.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <stdexcept>
#include <vector>

namespace msm {

// one level of segment sums: output t = sum of inputs [starts[t], starts[t + 1])
struct ReduceLevel {
  std::vector<uint32_t> starts;  // nout + 1, non-decreasing
  size_t nout = 0;
};

enum ReduceBuf { kRedBuckets, kRedPart0, kRedPart1, kRedDense };
enum ReduceEnding { kEndDense, kEndBits };
constexpr size_t kNoItems = ~(size_t)0;

// dst[m dstride + t] = sum_{k in [starts[t], starts[t + 1])} src[m sstride + (items ? items[k] : k)]
struct ReduceStep {
  ReduceBuf src;
  size_t sstride;  // elements per MSM
  size_t items;    // offset into ReducePlan::items, or kNoItems: the inputs are contiguous
  int level;       // ReducePlan::level(level)
  ReduceBuf dst;
  size_t dstride;
};

struct ReducePlan {
  int sbits = 1, nwin = 1, c0 = 8;  // s, windows, the level-0 chunk chosen
  size_t nbuckets = 0;
  // [level-0 items | final permutation | bit items | bit permutation]
  std::vector<uint32_t> items;
  size_t l0_off = 0, perm_off = 0, bit_off = 0, bperm_off = 0;
  // segment phase: level 0, the pairwise levels, the dense scatter (always >= 2);
  // bit phase (one-window plans, else empty): its levels, the scatter to 2 s slots
  std::vector<ReduceLevel> seg, bit;
  // elements per MSM of the two partial buffers: the steps alternate between
  // them, level 0 into part 0; the odd levels are at most half of level 0
  size_t maxp = 1, maxp1 = 1;

  size_t dense_slots() const { return (size_t)2 * nwin << sbits; }
  size_t bit_slots() const { return (size_t)2 * nwin * sbits; }
  bool has_bit_tail() const { return !bit.empty(); }
  size_t levels() const { return seg.size() + bit.size(); }
  const ReduceLevel &level(int t) const { return (size_t)t < seg.size() ? seg[t] : bit[t - seg.size()]; }

  // Levels of segment sums over items whose segments are `cur` (equal ones
  // adjacent): chunks of at most C within a segment, then pairwise until
  // nothing merges.  Appended to `out`; `cur` becomes the segment of each final
  // partial.
  static void chunk_levels(std::vector<uint32_t> &cur, int C, std::vector<ReduceLevel> &out) {
    const size_t first = out.size();
    do {
      ReduceLevel lv;
      std::vector<uint32_t> nseg;
      size_t k = 0;
      while (k < cur.size()) {
        lv.starts.push_back((uint32_t)k);
        nseg.push_back(cur[k]);
        size_t e = k + 1;
        while (e < cur.size() && e - k < (size_t)C && cur[e] == cur[k]) ++e;
        k = e;
      }
      lv.starts.push_back((uint32_t)cur.size());
      if (out.size() > first && nseg.size() == cur.size()) break;  // nothing merged: one partial per segment
      lv.nout = nseg.size();
      out.push_back(lv);
      cur.swap(nseg);
      C = 2;
    } while (!cur.empty());
  }

  // The scatter level: slot -> its single partial (or empty) among the final
  // partials of segments `cur`, through a permutation appended to the items.
  size_t scatter_level(const std::vector<uint32_t> &cur, size_t nslots, std::vector<ReduceLevel> &out) {
    const size_t off = items.size();
    std::vector<int> at(nslots, -1);
    for (size_t k = 0; k < cur.size(); ++k) at[cur[k]] = (int)k;
    ReduceLevel lv;
    for (size_t sl = 0; sl < nslots; ++sl) {
      lv.starts.push_back((uint32_t)(items.size() - off));
      if (at[sl] >= 0) items.push_back((uint32_t)at[sl]);
    }
    lv.starts.push_back((uint32_t)(items.size() - off));
    lv.nout = nslots;
    out.push_back(lv);
    return off;
  }

  // win[i] in [0, nwin): the window of bucket i (empty = all in window 0).
  // c0: level-0 chunk length, 0: by plan size.  A chunk of C items is C - 1
  // dependent adds in one lane.  Large plans keep 8 (few lanes per item, fewest
  // levels); small ones (a few hundred thousand items: plain Pippenger at 2^16,
  // CHES shards of 2^17..2^19) would leave the chip < 1 wave per SIMD deep with
  // 7-add chains (the 2^16 level 0 ran 103 us for 311 K adds,
  // profiles/archive_r01_r04.txt (r04_fixed_cost.txt)), so they take 4 or 2 and
  // one or two more (tail) levels.  The adds are the same in total (items -
  // segments).  lane_factor: lanes per item (G2 segment sums run on lane pairs).
  static ReducePlan build(const std::vector<uint32_t> &w, const std::vector<uint32_t> &win, int nwin, int c0,
                          int lane_factor) {
    if (nwin < 1 || (!win.empty() && win.size() != w.size())) throw std::runtime_error("WeightedReducer: bad windows");
    ReducePlan p;
    p.nbuckets = w.size();
    p.nwin = nwin;
    uint32_t maxw = 0;
    for (uint32_t x : w) maxw = std::max(maxw, x);
    int bits = 0;
    while (bits < 32 && ((uint64_t)1 << bits) <= maxw) ++bits;
    p.sbits = std::max(1, (bits + 1) / 2);
    const uint32_t S = 1u << p.sbits;
    // dense slot layout: window ww -> [L block (2 ww) S | H block (2 ww + 1) S]
    std::vector<std::vector<uint32_t>> byv((size_t)nwin * S), byu((size_t)nwin * S);
    for (size_t i = 0; i < w.size(); ++i) {
      const size_t ww = win.empty() ? 0 : win[i];
      if (ww >= (size_t)nwin) throw std::runtime_error("WeightedReducer: window out of range");
      uint32_t v = w[i] >> p.sbits, u = w[i] & (S - 1);
      if (v) byv[ww * S + v].push_back((uint32_t)i);
      if (u) byu[ww * S + u].push_back((uint32_t)i);
    }
    std::vector<uint32_t> cur;  // the segment (dense slot) of each item, then of each partial
    for (int ww = 0; ww < nwin; ++ww) {
      for (uint32_t v = 1; v < S; ++v)
        for (uint32_t i : byv[(size_t)ww * S + v]) p.items.push_back(i), cur.push_back((2 * ww + 1) * S + v - 1);
      for (uint32_t u = 1; u < S; ++u)
        for (uint32_t i : byu[(size_t)ww * S + u]) p.items.push_back(i), cur.push_back(2 * ww * S + u - 1);
    }
    const size_t lane_items = p.items.size() * (size_t)lane_factor;
    p.c0 = c0 ? c0 : lane_items >= ((size_t)3 << 19) ? 8 : lane_items >= ((size_t)600 << 10) ? 4 : 2;
    chunk_levels(cur, p.c0, p.seg);
    p.perm_off = p.scatter_level(cur, p.dense_slots(), p.seg);
    p.bit_off = p.bperm_off = p.items.size();
    if (nwin == 1) {
      // bit segment (block, j): the final partials p of block = cur[p] / S whose
      // value cur[p] % S + 1 has bit j.  Pairwise from the first level: the tail
      // is latency-bound (a chunk of 8 is 7 serial adds in one lane)
      std::vector<uint32_t> bseg;
      for (uint32_t bs = 0; bs < p.bit_slots(); ++bs) {
        const uint32_t blk = bs / (uint32_t)p.sbits, j = bs % (uint32_t)p.sbits;
        for (size_t q = 0; q < cur.size(); ++q)
          if (cur[q] / S == blk && (((cur[q] % S) + 1) >> j & 1u)) p.items.push_back((uint32_t)q), bseg.push_back(bs);
      }
      if (!bseg.empty()) chunk_levels(bseg, 2, p.bit);
      p.bperm_off = p.scatter_level(bseg, p.bit_slots(), p.bit);
    }
    for (size_t l = 0; l + 1 < p.seg.size(); ++l) {
      p.maxp = std::max(p.maxp, p.seg[l].nout);
      if (l & 1) p.maxp1 = std::max(p.maxp1, p.seg[l].nout);
    }
    // the bit levels go on alternating from wherever the segment levels ended:
    // every one fits either buffer
    for (size_t l = 0; l + 1 < p.bit.size(); ++l) p.maxp = std::max(p.maxp, p.bit[l].nout), p.maxp1 = std::max(p.maxp1, p.bit[l].nout);
    return p;
  }

  // The steps of one reduction, level 0 first.  The only place that knows the
  // ping-pong and the strides: every step but the last writes the partial
  // buffer the step before it did not (level 0: part 0, maxp per MSM; part 1:
  // maxp1), the last scatters into the dense buffer (dense_slots() per MSM, or
  // bit_slots() when the reduction ends in bit sums: the segment phase then
  // stops before its scatter and the bit phase follows).
  std::vector<ReduceStep> steps(ReduceEnding end) const {
    if (end == kEndBits && !has_bit_tail()) throw std::runtime_error("WeightedReducer: no bit tail in this plan");
    std::vector<ReduceStep> out;
    ReduceStep st{kRedBuckets, nbuckets, kNoItems, 0, kRedBuckets, nbuckets};
    int nb = 0;
    auto push = [&](int level, size_t item_off, bool last, size_t slots) {
      st = ReduceStep{st.dst, st.dstride, item_off, level, last ? kRedDense : nb ? kRedPart1 : kRedPart0,
                      last ? slots : nb ? maxp1 : maxp};
      out.push_back(st);
      nb ^= 1;
    };
    const size_t L = seg.size(), LB = bit.size();
    for (size_t l = 0; l < (end == kEndBits ? L - 1 : L); ++l)
      push((int)l, l == 0 ? l0_off : l + 1 == L ? perm_off : kNoItems, l + 1 == L, dense_slots());
    for (size_t l = 0; end == kEndBits && l < LB; ++l)
      push((int)(L + l), l + 1 == LB ? bperm_off : l == 0 ? bit_off : kNoItems, l + 1 == LB, bit_slots());
    return out;
  }

  // elements of buffer b (a partial buffer or the dense buffer) for nmsm MSMs, either ending
  size_t elems(ReduceBuf b, size_t nmsm) const {
    return nmsm * (b == kRedPart0 ? maxp : b == kRedPart1 ? maxp1 : b == kRedDense ? dense_slots() : nbuckets);
  }
};

}  // namespace msm
