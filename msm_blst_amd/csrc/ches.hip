// ches.hip -- host orchestration of the CHES "nh + q/5" bucket-set MSM
// (LuoGuiwen/MSM_blst, method `pippenger_variant_q_over_5_CHES`,
// ref main_p1.cpp:192-246) on one MI355X.
//
// Setup (once per context): parameters of ref ches_config_files, bucket set B
// (ref auxiliaryfunc.h:257-288), digit hash (ref main_p1.cpp:140-152) and the
// precomputed table T[3(i h + j) + m - 1] = m q^j P_i (ref main_p1.cpp:155-172),
// the latter built on the GPU and kept resident in HBM in the engine's
// internal limb layout.
//
// Per MSM (all on device, one stream):
//   digits   k_ches_digits: MB radix-q digits + per-bucket counts/ranks
//   sort     exclusive scan of counts, k_ches_scatter, bucket schedule by size
//   accum    k_accumulate: one lane per bucket, xyzz += +-T[slot]
//   reduce   WeightedReducer: sum_i B[i] S_i (replaces the d-trick loop of
//            ref multi_scalar.c:301-321 with a GPU-parallel regrouping)
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "ches_kernels.hpp"
#include "coop.hpp"
#include "engine.hpp"
#include "hoststage.hpp"
#include "pair_kernels.hpp"

#ifndef MSM_GROUP
#error "define MSM_GROUP (1 or 2)"
#endif

namespace msm {

#if MSM_GROUP == 1  // group-independent host setup: compiled once
// ------------------------------------------------------------- parameters --
// values of ref ches_config_files/config_file_n_exp_{8..21}.h and the _beta
// variants (n_exp, beta, q exponent, h, a_h, d_max, |B|, BGMW95 q exponent, h)
static const ChesParams kChesTable[] = {
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

bool ches_params_for(int n_exp, int beta, ChesParams *out) {
  for (const ChesParams &p : kChesTable)
    if (p.n_exp == n_exp && p.beta == beta) {
      *out = p;
      return true;
    }
  return false;
}

// omega2(v) + omega3(v) even  (ref auxiliaryfunc.h:217-255)
static bool even23(int v) {
  int e = 0;
  while (v % 2 == 0) v /= 2, ++e;
  while (v % 3 == 0) v /= 3, ++e;
  return (e & 1) == 0;
}

// ref auxiliaryfunc.h:257-288: {0,1} u {i <= q/2 : even23(i)}, then the two
// pruning passes (membership tested as the passes run, as std::set::erase
// does there), then every even23 value <= a_h + 1 re-inserted.
std::vector<int> ches_bucket_set(int q, int a_h) {
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

// ref main_p1.cpp:140-152: every (m, b) writes H[q - m b] = (m, b, alpha=1),
// then H[m b] = (m, b, 0); later writes win.  Packed per ches_kernels.hpp.
std::vector<uint32_t> ches_digit_hash(const std::vector<int> &B, int q) {
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

void ches_digit_code(const std::vector<int> &B, int q, std::vector<uint32_t> &code, std::vector<uint32_t> &rank) {
  const std::vector<uint32_t> H = ches_digit_hash(B, q);
  code.assign(((size_t)q >> 3) + 2, 0);
  for (size_t d = 0; d <= (size_t)q; ++d) {
    const uint32_t m = ((H[d] >> 24) & 3u) + 1, alpha = H[d] >> 31;
    const int b = B[H[d] & CH_IDX_MASK];
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
#endif  // MSM_GROUP == 1

// a tail level of segment sums: few outputs are latency-bound, so one add
// spreads over 4 waves (coop.hpp: G1 one lane per wave, G2 a lane pair per wave);
// nmsm > 1: the MSMs of a batch group, src / dst advanced by their strides
template <int G>
static void launch_segsum_tail(hipStream_t s, const Xyzz<typename FieldOf<G>::F> *src, const uint32_t *ix,
                               const uint32_t *st, Xyzz<typename FieldOf<G>::F> *dst, size_t nout, bool coop,
                               int nmsm = 1, size_t sstride = 0, size_t dstride = 0) {
  if (coop && nout * (size_t)nmsm <= 16384) {
    if constexpr (G == 1)
      hipLaunchKernelGGL(k_segsum_c<G>, dim3(nblk(nout, 64), (unsigned)nmsm), dim3(256), 0, s, src, ix, st, dst, nout,
                         sstride, dstride);
    else
      hipLaunchKernelGGL(k_segsum_c2p, dim3(nblk(nout, 32), (unsigned)nmsm), dim3(256), 0, s, src, ix, st, dst, nout,
                         sstride, dstride);
  } else {
    launch_segsum<G>(s, src, ix, st, dst, nout, nmsm, sstride, dstride);
  }
}

// -------------------------------------------------------------- scan reduce --
// coop levels of the dense stage: only those with at most this many adds.  A
// 4-wave add is the shortest latency for a narrow level, but its waves are 4x
// the one-lane form's: a suffix step over a batch group's 20 x 2 x 1024 slots
// ran 24 us per level coop (0.8 rounds of wave slots, 2.5 waves per SIMD
// sharing issue) -- the batch's last, exposed tail (profiles/r06_small_trace.txt).
// MSM_DENSE_COOP_MAX=<adds> overrides (0: every level one lane per add).
static size_t dense_coop_max() {
  static const size_t v = [] {
    const char *e = getenv("MSM_DENSE_COOP_MAX");
    return e ? (size_t)std::max(0, atoi(e)) : (size_t)16384;
  }();
  return v;
}

template <int G>
void ScanReducer<G>::launch(hipStream_t s, const void *Abuf, int W, int S, bool coop_req) {
  typedef typename FieldOf<G>::F F;
  if (S < 1 || (S & (S - 1))) throw std::runtime_error("ScanReducer: S must be a power of two");
  const size_t NT = (size_t)W * S;
  bool coop = coop_req && NT <= dense_coop_max();  // the suffix steps: NT adds each
  buf[0].ensure(NT * sizeof(Xyzz<F>));
  buf[1].ensure(NT * sizeof(Xyzz<F>));
  fin.ensure((size_t)W * 144 * G);
  const Xyzz<F> *src = reinterpret_cast<const Xyzz<F> *>(Abuf);
  int cur = 0;
  for (int d = 1; d < S; d <<= 1) {  // suffix sums T_k = sum_{b >= k} A_b
    Xyzz<F> *dst = buf[cur].as<Xyzz<F>>();
    if constexpr (G == 2) {  // lane pairs (fp2l.hpp); coop: one add over 4 waves (coop.hpp)
      if (coop)
        hipLaunchKernelGGL(k_suffix_step_c2p, dim3(nblk(NT, 32)), dim3(256), 0, s, src, dst, S, d, W);
      else
        hipLaunchKernelGGL(k_suffix_step2p, dim3(nblk(2 * NT, 64)), dim3(64), 0, s, src, dst, S, d, W);
    } else {
      if (coop) hipLaunchKernelGGL(k_suffix_step_c<G>, dim3(nblk(NT, 64)), dim3(256), 0, s, src, dst, S, d, W);
      else hipLaunchKernelGGL(k_suffix_step<G>, dim3(nblk(NT, 64)), dim3(64), 0, s, src, dst, S, d, W);
    }
    MSM_HIP_CHECK(hipGetLastError());
    src = dst;
    cur ^= 1;
  }
  for (size_t len = NT; len > (size_t)W; len >>= 1) {  // sum_k T_k = sum_b b A_b
    Xyzz<F> *dst = buf[cur].as<Xyzz<F>>();
    coop = coop_req && len / 2 <= dense_coop_max();  // this pair step: len / 2 adds
    if constexpr (G == 2) {
      if (coop)
        hipLaunchKernelGGL(k_pair_step_c2p, dim3(nblk(len / 2, 32)), dim3(256), 0, s, src, dst, len / 2);
      else
        hipLaunchKernelGGL(k_pair_step2p, dim3(nblk(len, 64)), dim3(64), 0, s, src, dst, len / 2);
    } else {
      if (coop) hipLaunchKernelGGL(k_pair_step_c<G>, dim3(nblk(len / 2, 64)), dim3(256), 0, s, src, dst, len / 2);
      else hipLaunchKernelGGL(k_pair_step<G>, dim3(nblk(len / 2, 64)), dim3(64), 0, s, src, dst, len / 2);
    }
    MSM_HIP_CHECK(hipGetLastError());
    src = dst;
    cur ^= 1;
  }
  hipLaunchKernelGGL(k_finalize<G>, dim3(nblk(W, 64)), dim3(64), 0, s, src, fin.as<uint64_t>(), W);
  MSM_HIP_CHECK(hipGetLastError());
}
template <int G>
void ScanReducer<G>::read(hipStream_t s, int W, std::vector<hfp::Jac<HF>> &out) {
  out.resize(W);
  MSM_HIP_CHECK(hipMemcpyAsync(out.data(), fin.p, (size_t)W * sizeof(hfp::Jac<HF>), hipMemcpyDeviceToHost, s));
  MSM_HIP_CHECK(hipStreamSynchronize(s));
}
template struct ScanReducer<MSM_GROUP>;

// ---------------------------------------------------------- reduction plan --
// sum_i w_i S_i = sum_u u L_u + 2^s sum_v v H_v  with u = w_i mod 2^s,
// v = w_i >> s, L_u = sum_{i: low(w_i) = u} S_i, H_v = sum_{i: high(w_i) = v} S_i.
// L and H are segment sums over one list of bucket indices (level 0: chunks of
// <= 8 within a segment; then pairwise levels until one partial per segment;
// then a dense scatter into 2 windows of 2^s slots), followed by the dense
// 2-window ScanReducer and a 2^s Horner step on the host.
template <int G>
void WeightedReducer<G>::plan(const std::vector<uint32_t> &w, const std::vector<uint32_t> &win, int nwin, int c0) {
  typedef typename FieldOf<G>::F F;
  if (nwin < 1 || (!win.empty() && win.size() != w.size())) throw std::runtime_error("WeightedReducer: bad windows");
  bsize_ = w.size();
  nwin_ = nwin;
  starts_.clear();
  nout_.clear();
  uint32_t maxw = 0;
  for (uint32_t x : w) maxw = std::max(maxw, x);
  int bits = 0;
  while (bits < 32 && ((uint64_t)1 << bits) <= maxw) ++bits;
  sbits_ = std::max(1, (bits + 1) / 2);
  const uint32_t S = 1u << sbits_;
  // dense slot layout: window ww -> [L block (2 ww) S | H block (2 ww + 1) S]
  std::vector<std::vector<uint32_t>> byv((size_t)nwin * S), byu((size_t)nwin * S);
  for (size_t i = 0; i < w.size(); ++i) {
    const size_t ww = win.empty() ? 0 : win[i];
    if (ww >= (size_t)nwin) throw std::runtime_error("WeightedReducer: window out of range");
    uint32_t v = w[i] >> sbits_, u = w[i] & (S - 1);
    if (v) byv[ww * S + v].push_back((uint32_t)i);
    if (u) byu[ww * S + u].push_back((uint32_t)i);
  }
  std::vector<uint32_t> idx, seg;
  for (int ww = 0; ww < nwin; ++ww) {
    for (uint32_t v = 1; v < S; ++v)
      for (uint32_t i : byv[(size_t)ww * S + v]) idx.push_back(i), seg.push_back((2 * ww + 1) * S + v - 1);
    for (uint32_t u = 1; u < S; ++u)
      for (uint32_t i : byu[(size_t)ww * S + u]) idx.push_back(i), seg.push_back(2 * ww * S + u - 1);
  }
  // level 0 + pairwise levels
  std::vector<uint32_t> cur_seg = seg;
  // Level-0 chunk length: a chunk of C items is C - 1 dependent adds in one
  // lane.  Large plans keep 8 (few lanes per item, fewest levels); small ones
  // (a few hundred thousand items: plain Pippenger at 2^16, CHES shards of
  // 2^17..2^19) would leave the chip < 1 wave per SIMD deep with 7-add chains
  // (the 2^16 level 0 ran 103 us for 311 K adds, profiles/archive_r01_r04.txt (r04_fixed_cost.txt)),
  // so they take 4 or 2 and one or two more (tail) levels.  The adds are the
  // same in total (items - segments); MSM_L0_CHUNK=<2..64> overrides.
  static const int C0env = [] {
    const char *e = getenv("MSM_L0_CHUNK");  // A/B knob: level-0 chunk length
    return e ? std::max(2, std::min(64, atoi(e))) : 0;
  }();
  const size_t lane_items = idx.size() * (G == 2 ? 2 : 1);  // G2 segment sums run on lane pairs
  int C = C0env ? C0env : c0 ? c0 : lane_items >= ((size_t)3 << 19) ? 8 : lane_items >= ((size_t)600 << 10) ? 4 : 2;
  c0_ = C;
  while (true) {
    std::vector<uint32_t> st, nseg;
    size_t k = 0;
    while (k < cur_seg.size()) {
      st.push_back((uint32_t)k);
      nseg.push_back(cur_seg[k]);
      size_t e = k + 1;
      while (e < cur_seg.size() && e - k < (size_t)C && cur_seg[e] == cur_seg[k]) ++e;
      k = e;
    }
    st.push_back((uint32_t)cur_seg.size());
    bool first = starts_.empty();
    if (!first && nseg.size() == cur_seg.size()) break;  // nothing merged: one partial per segment
    starts_.emplace_back();
    starts_.back().ensure(st.size() * 4);
    MSM_HIP_CHECK(hipMemcpy(starts_.back().p, st.data(), st.size() * 4, hipMemcpyHostToDevice));
    nout_.push_back(nseg.size());
    cur_seg.swap(nseg);
    C = 2;
    if (cur_seg.empty()) break;
  }
  // bit phase (sync tail of one-window plans): segment (block, j) over the
  // final partials p of block = cur_seg[p] / S whose value cur_seg[p] % S + 1
  // has bit j; chunks of 8, pairwise levels, then a scatter to 2 s slots
  std::vector<uint32_t> bidx;
  bits_ = nwin == 1;
  bstarts_.clear();
  bnout_.clear();
  if (bits_) {
    const uint32_t NB2 = 2u * (uint32_t)nwin * (uint32_t)sbits_;
    std::vector<uint32_t> bseg;
    for (uint32_t bs = 0; bs < NB2; ++bs) {
      const uint32_t blk = bs / (uint32_t)sbits_, j = bs % (uint32_t)sbits_;
      for (size_t q = 0; q < cur_seg.size(); ++q)
        if (cur_seg[q] / S == blk && (((cur_seg[q] % S) + 1) >> j & 1u)) bidx.push_back((uint32_t)q), bseg.push_back(bs);
    }
    int Cb = 2;  // pairwise from the first level: the tail is latency-bound (a chunk of 8 is 7 serial adds in one lane)
    while (!bseg.empty()) {
      std::vector<uint32_t> st, nseg;
      size_t k = 0;
      while (k < bseg.size()) {
        st.push_back((uint32_t)k);
        nseg.push_back(bseg[k]);
        size_t e = k + 1;
        while (e < bseg.size() && e - k < (size_t)Cb && bseg[e] == bseg[k]) ++e;
        k = e;
      }
      st.push_back((uint32_t)bseg.size());
      if (!bnout_.empty() && nseg.size() == bseg.size()) break;
      bstarts_.emplace_back();
      bstarts_.back().ensure(st.size() * 4);
      MSM_HIP_CHECK(hipMemcpy(bstarts_.back().p, st.data(), st.size() * 4, hipMemcpyHostToDevice));
      bnout_.push_back(nseg.size());
      bseg.swap(nseg);
      Cb = 2;
    }
    std::vector<uint32_t> bdst(NB2 + 1, 0), bperm;
    std::vector<int> bat(NB2, -1);
    for (size_t k = 0; k < bseg.size(); ++k) bat[bseg[k]] = (int)k;
    for (uint32_t sl = 0; sl < NB2; ++sl) {
      bdst[sl] = (uint32_t)bperm.size();
      if (bat[sl] >= 0) bperm.push_back((uint32_t)bat[sl]);
    }
    bdst[NB2] = (uint32_t)bperm.size();
    bstarts_.emplace_back();
    bstarts_.back().ensure(bdst.size() * 4);
    MSM_HIP_CHECK(hipMemcpy(bstarts_.back().p, bdst.data(), bdst.size() * 4, hipMemcpyHostToDevice));
    bnout_.push_back(NB2);
    bidx.insert(bidx.end(), bperm.begin(), bperm.end());
    bperm_off_ = bidx.size() - bperm.size();
    bfin_.ensure((size_t)NB2 * 144 * G);
  }
  // dense scatter: slot -> its single partial (or empty), via a permutation
  const size_t NS = (size_t)2 * nwin * S;
  std::vector<uint32_t> dst(NS + 1, 0), perm;
  std::vector<int> at(NS, -1);
  for (size_t k = 0; k < cur_seg.size(); ++k) at[cur_seg[k]] = (int)k;
  for (size_t sl = 0; sl < NS; ++sl) {
    dst[sl] = (uint32_t)perm.size();
    if (at[sl] >= 0) perm.push_back((uint32_t)at[sl]);
  }
  dst[NS] = (uint32_t)perm.size();
  starts_.emplace_back();
  starts_.back().ensure(dst.size() * 4);
  MSM_HIP_CHECK(hipMemcpy(starts_.back().p, dst.data(), dst.size() * 4, hipMemcpyHostToDevice));
  nout_.push_back(NS);
  std::vector<uint32_t> all = idx;  // [level-0 item list | final permutation | bit phase items | bit permutation]
  all.insert(all.end(), perm.begin(), perm.end());
  final_perm_off_ = idx.size();
  bidx_off_ = all.size();
  bperm_off_ += bidx_off_;
  all.insert(all.end(), bidx.begin(), bidx.end());
  idx_.ensure(std::max<size_t>(all.size(), 1) * 4);
  if (!all.empty()) MSM_HIP_CHECK(hipMemcpy(idx_.p, all.data(), all.size() * 4, hipMemcpyHostToDevice));
  maxp_ = 1;
  for (size_t l = 0; l + 1 < nout_.size(); ++l) maxp_ = std::max(maxp_, nout_[l]);
  for (size_t l = 0; l + 1 < bnout_.size(); ++l) maxp_ = std::max(maxp_, bnout_[l]);  // bit phase levels
  maxp1_ = 1;  // batch group tails: level l writes part_[l & 1]; the odd levels are at most half of level 0
  for (size_t l = 1; l + 1 < nout_.size(); l += 2) maxp1_ = std::max(maxp1_, nout_[l]);
  // (the group bit tail, launch_tail_group_bits, alternates its levels over both
  // part_ buffers: every bit level fits either)
  for (size_t l = 0; l + 1 < bnout_.size(); ++l) maxp1_ = std::max(maxp1_, bnout_[l]);
  for (int st = 0; st < NSETS; ++st) {  // a new plan: sets are (re)sized on their next use
    part_[st][0].release();
    part_[st][1].release();
    dense_buf_[st].release();
  }
  ensure_set(0);
}

template <int G>
void WeightedReducer<G>::ensure_set(int set) {
  typedef typename FieldOf<G>::F F;
  if (set < 0 || set >= NSETS) throw std::runtime_error("WeightedReducer: bad buffer set");
  part_[set][0].ensure(maxp_ * sizeof(Xyzz<F>));
  part_[set][1].ensure(maxp_ * sizeof(Xyzz<F>));
  dense_buf_[set].ensure((size_t)2 * nwin_ * ((size_t)1 << sbits_) * sizeof(Xyzz<F>));
}

template <int G>
void WeightedReducer<G>::launch_head(hipStream_t s, const void *Sbuf, int set) {
  typedef typename FieldOf<G>::F F;
  ensure_set(set);
  const size_t L = nout_.size();
  const Xyzz<F> *src = reinterpret_cast<const Xyzz<F> *>(Sbuf);
  Xyzz<F> *dst = L == 1 ? dense_buf_[set].as<Xyzz<F>>() : part_[set][0].as<Xyzz<F>>();
  const uint32_t *ix = L == 1 ? idx_.as<uint32_t>() + final_perm_off_ : idx_.as<uint32_t>();
  launch_segsum<G>(s, src, ix, starts_[0].as<uint32_t>(), dst, nout_[0]);
  MSM_HIP_CHECK(hipGetLastError());
}

template <int G>
void WeightedReducer<G>::launch_tail(hipStream_t s, int set, bool coop) {
  typedef typename FieldOf<G>::F F;
  const size_t L = nout_.size();
  const Xyzz<F> *src = part_[set][0].as<Xyzz<F>>();
  if (bits_ && L >= 2) {
    // phase-1 levels 1 .. L-2 (level L-1 is the dense scatter, not used here),
    // then the bit phase: its level 0 reads the final partials through the
    // bit item list, later levels are contiguous, the last scatters to 2 s slots
    int cur = 0;
    auto segsum = [&](const Xyzz<F> *a, const uint32_t *ix, const uint32_t *st, Xyzz<F> *d, size_t nout) {
      if (!nout) return;
      launch_segsum_tail<G>(s, a, ix, st, d, nout, coop);
      MSM_HIP_CHECK(hipGetLastError());
    };
    for (size_t l = 1; l + 1 < L; ++l) {
      Xyzz<F> *dst = part_[set][l & 1].as<Xyzz<F>>();
      segsum(src, nullptr, starts_[l].as<uint32_t>(), dst, nout_[l]);
      src = dst;
      cur = (int)(l & 1);
    }
    const size_t LB = bnout_.size();
    for (size_t l = 0; l < LB; ++l) {
      const bool last = l + 1 == LB;
      Xyzz<F> *dst = last ? dense_buf_[set].as<Xyzz<F>>() : part_[set][cur ^ 1].as<Xyzz<F>>();
      const uint32_t *ix = l == 0 ? idx_.as<uint32_t>() + bidx_off_ : last ? idx_.as<uint32_t>() + bperm_off_ : nullptr;
      segsum(src, ix, bstarts_[l].as<uint32_t>(), dst, bnout_[l]);
      src = dst;
      cur ^= 1;
    }
    hipLaunchKernelGGL(k_finalize<G>, dim3(nblk(bit_slots(), 64)), dim3(64), 0, s, src, bfin_.as<uint64_t>(),
                       (int)bit_slots());
    MSM_HIP_CHECK(hipGetLastError());
    return;
  }
  for (size_t l = 1; l < L; ++l) {
    const bool last = l + 1 == L;
    Xyzz<F> *dst = last ? dense_buf_[set].as<Xyzz<F>>() : part_[set][l & 1].as<Xyzz<F>>();
    const uint32_t *ix = last ? idx_.as<uint32_t>() + final_perm_off_ : nullptr;
    if (nout_[l]) launch_segsum_tail<G>(s, src, ix, starts_[l].as<uint32_t>(), dst, nout_[l], coop);
    MSM_HIP_CHECK(hipGetLastError());
    src = dst;
  }
  dense_[set].launch(s, dense_buf_[set].p, 2 * nwin_, 1 << sbits_, coop);
}

template <int G>
void WeightedReducer<G>::ensure_group(int set, int nmsm) {
  typedef typename FieldOf<G>::F F;
  if (set < 0 || set >= NSETS || nmsm < 1) throw std::runtime_error("WeightedReducer: bad group");
  part_[set][0].ensure((size_t)nmsm * maxp_ * sizeof(Xyzz<F>));
  part_[set][1].ensure((size_t)nmsm * maxp1_ * sizeof(Xyzz<F>));
  if (bits_) bgfin_[set].ensure((size_t)nmsm * bit_bytes());
  dense_buf_[set].ensure((size_t)nmsm * dense_slots() * sizeof(Xyzz<F>));
  const size_t NT = (size_t)nmsm * dense_slots();  // ScanReducer::launch's buffers for W = 2 nwin nmsm
  dense_[set].buf[0].ensure(NT * sizeof(Xyzz<F>));
  dense_[set].buf[1].ensure(NT * sizeof(Xyzz<F>));
  dense_[set].fin.ensure((size_t)nmsm * out_bytes());
}

template <int G>
typename WeightedReducer<G>::HeadArgs WeightedReducer<G>::head_args(int set, int slot) {
  typedef typename FieldOf<G>::F F;
  const bool only = nout_.size() == 1;  // level 0 is also the last level
  Xyzz<F> *dst = only ? dense_buf_[set].as<Xyzz<F>>() + (size_t)slot * dense_slots()
                      : part_[set][0].as<Xyzz<F>>() + (size_t)slot * maxp_;
  const uint32_t *ix = only ? idx_.as<uint32_t>() + final_perm_off_ : idx_.as<uint32_t>();
  return HeadArgs{ix, starts_[0].as<uint32_t>(), dst, nout_[0]};
}

template <int G>
void WeightedReducer<G>::launch_head_slot(hipStream_t s, const void *Sbuf, int set, int slot) {
  typedef typename FieldOf<G>::F F;
  const HeadArgs a = head_args(set, slot);
  launch_segsum<G>(s, reinterpret_cast<const Xyzz<F> *>(Sbuf), a.idx, a.starts, static_cast<Xyzz<F> *>(a.dst),
                   a.nout);
  MSM_HIP_CHECK(hipGetLastError());
}

template <int G>
void WeightedReducer<G>::launch_head_slots(hipStream_t s, const void *Sbuf, size_t sstride, int set, int slot0,
                                           int nmsm) {
  typedef typename FieldOf<G>::F F;
  const bool only = nout_.size() == 1;  // level 0 is also the last level
  const HeadArgs a = head_args(set, slot0);
  launch_segsum<G>(s, reinterpret_cast<const Xyzz<F> *>(Sbuf), a.idx, a.starts, static_cast<Xyzz<F> *>(a.dst), a.nout,
                   nmsm, sstride, only ? dense_slots() : maxp_);
  MSM_HIP_CHECK(hipGetLastError());
}

template <int G>
void WeightedReducer<G>::launch_tail_group(hipStream_t s, int set, int nmsm, bool coop) {
  typedef typename FieldOf<G>::F F;
  const size_t L = nout_.size();
  const Xyzz<F> *src = part_[set][0].as<Xyzz<F>>();
  for (size_t l = 1; l < L; ++l) {
    const bool last = l + 1 == L;
    Xyzz<F> *dst = last ? dense_buf_[set].as<Xyzz<F>>() : part_[set][l & 1].as<Xyzz<F>>();
    const uint32_t *ix = last ? idx_.as<uint32_t>() + final_perm_off_ : nullptr;
    const size_t sstride = (l & 1) ? maxp_ : maxp1_;  // level l - 1 wrote part_[(l - 1) & 1]
    // coop (the batch's last group: nothing left to overlap): the narrow levels
    // over 4 waves per add
    launch_segsum_tail<G>(s, src, ix, starts_[l].as<uint32_t>(), dst, nout_[l], coop, nmsm, sstride,
                          last ? dense_slots() : (l & 1) ? maxp1_ : maxp_);
    MSM_HIP_CHECK(hipGetLastError());
    src = dst;
  }
  dense_[set].launch(s, dense_buf_[set].p, 2 * nwin_ * nmsm, 1 << sbits_, coop);
}

// The group tail ending in bit sums (one-window plans): the segment levels,
// then per MSM the 2 s bit sums B_j (the bit phase of launch_tail, every level
// one launch for the group), finalized to nmsm x 2 s Jacobians; the host
// combines T = sum_j 2^j B_j (combine_bits).  ~10 levels instead of the 2 s of
// the dense stage: for the batch's LAST group, whose tail runs after the last
// accumulation with the chip otherwise idle (Ches::run_jobs).
template <int G>
void WeightedReducer<G>::launch_tail_group_bits(hipStream_t s, int set, int nmsm, bool coop) {
  typedef typename FieldOf<G>::F F;
  const size_t L = nout_.size(), LB = bnout_.size();
  if (!has_bit_tail()) throw std::runtime_error("WeightedReducer: no bit tail in this plan");
  const Xyzz<F> *src = part_[set][0].as<Xyzz<F>>();
  size_t sstride = maxp_;
  int cur = 0;
  for (size_t l = 1; l + 1 < L; ++l) {  // segment levels 1 .. L-2 (L-1 is the dense scatter)
    Xyzz<F> *dst = part_[set][l & 1].as<Xyzz<F>>();
    const size_t dstride = (l & 1) ? maxp1_ : maxp_;
    if (nout_[l]) launch_segsum_tail<G>(s, src, nullptr, starts_[l].as<uint32_t>(), dst, nout_[l], coop, nmsm, sstride,
                                        dstride);
    MSM_HIP_CHECK(hipGetLastError());
    src = dst;
    sstride = dstride;
    cur = (int)(l & 1);
  }
  for (size_t l = 0; l < LB; ++l) {
    const bool last = l + 1 == LB;
    const int nb = cur ^ 1;
    Xyzz<F> *dst = last ? dense_buf_[set].as<Xyzz<F>>() : part_[set][nb].as<Xyzz<F>>();
    const size_t dstride = last ? bit_slots() : nb ? maxp1_ : maxp_;
    const uint32_t *ix = l == 0 ? idx_.as<uint32_t>() + bidx_off_ : last ? idx_.as<uint32_t>() + bperm_off_ : nullptr;
    if (bnout_[l])
      launch_segsum_tail<G>(s, src, ix, bstarts_[l].as<uint32_t>(), dst, bnout_[l], coop, nmsm, sstride, dstride);
    MSM_HIP_CHECK(hipGetLastError());
    src = dst;
    sstride = dstride;
    cur = nb;
  }
  const int W = (int)((size_t)nmsm * bit_slots());
  hipLaunchKernelGGL(k_finalize<G>, dim3(nblk((size_t)W, 64)), dim3(64), 0, s, src, bgfin_[set].as<uint64_t>(), W);
  MSM_HIP_CHECK(hipGetLastError());
}

template <int G>
void WeightedReducer<G>::copy_out_group_bits(hipStream_t s, int set, int nmsm, void *host) {
  MSM_HIP_CHECK(hipMemcpyAsync(host, bgfin_[set].p, (size_t)nmsm * bit_bytes(), hipMemcpyDefault, s));
}

// window 0's sum_b b S_b from its 2 s bit sums (bit j of the weight: low half
// block j < s, high half s + j): Horner from the top bit, as read_windows
template <int G>
hfp::Jac<typename HostField<G>::F> WeightedReducer<G>::combine_bits(const void *host) const {
  const hfp::Jac<HF> *B = reinterpret_cast<const hfp::Jac<HF> *>(host);
  const hfp::Jac<HF> *lo = B, *hi = B + sbits_;
  hfp::Jac<HF> acc = hi[sbits_ - 1];
  for (int j = 2 * sbits_ - 2; j >= 0; --j) {
    acc = hfp::dbl(acc);
    acc = hfp::addj(acc, j >= sbits_ ? hi[j - sbits_] : lo[j]);
  }
  return acc;
}

template <int G>
void WeightedReducer<G>::copy_out_group(hipStream_t s, int set, int nmsm, void *host) {
  // host (read-back) or device (an exchange buffer, ChesMulti's RCCL gather)
  MSM_HIP_CHECK(hipMemcpyAsync(host, dense_[set].fin.p, (size_t)nmsm * out_bytes(), hipMemcpyDefault, s));
}

template <int G>
void WeightedReducer<G>::copy_out(hipStream_t s, int set, void *host) {
  MSM_HIP_CHECK(hipMemcpyAsync(host, dense_[set].fin.p, out_bytes(), hipMemcpyDeviceToHost, s));
}

template <int G>
std::vector<hfp::Jac<typename HostField<G>::F>> WeightedReducer<G>::combine(const void *host) const {
  const hfp::Jac<HF> *T = reinterpret_cast<const hfp::Jac<HF> *>(host);
  std::vector<hfp::Jac<HF>> out(nwin_);
  for (int ww = 0; ww < nwin_; ++ww) out[ww] = horner(std::vector<hfp::Jac<HF>>{T[2 * ww], T[2 * ww + 1]}, sbits_);
  return out;
}

template <int G>
std::vector<hfp::Jac<typename HostField<G>::F>> WeightedReducer<G>::read_windows(hipStream_t s) {
  if (bits_ && nout_.size() >= 2) {  // launch_tail's bit sums: T = sum_j 2^j B_j, Horner from the top bit
    std::vector<hfp::Jac<HF>> B(bit_slots());
    MSM_HIP_CHECK(hipMemcpyAsync(B.data(), bfin_.p, bit_slots() * sizeof(hfp::Jac<HF>), hipMemcpyDeviceToHost, s));
    MSM_HIP_CHECK(hipStreamSynchronize(s));
    std::vector<hfp::Jac<HF>> out(nwin_);
    for (int ww = 0; ww < nwin_; ++ww) {
      // bit j of the window's weight: low half block 2 ww (j < s), high half block 2 ww + 1
      const hfp::Jac<HF> *lo = &B[(size_t)2 * ww * sbits_], *hi = lo + sbits_;
      hfp::Jac<HF> acc = hi[sbits_ - 1];
      for (int j = 2 * sbits_ - 2; j >= 0; --j) {
        acc = hfp::dbl(acc);
        acc = hfp::addj(acc, j >= sbits_ ? hi[j - sbits_] : lo[j]);
      }
      out[ww] = acc;
    }
    return out;
  }
  std::vector<uint8_t> host(out_bytes());
  copy_out(s, 0, host.data());
  MSM_HIP_CHECK(hipStreamSynchronize(s));
  return combine(host.data());
}

template <int G>
hfp::Jac<typename HostField<G>::F> WeightedReducer<G>::combine_windows(const void *host, int c) const {
  const hfp::Jac<HF> *T = reinterpret_cast<const hfp::Jac<HF> *>(host);
  // terms (exponent, point): L_w at c w, H_w at c w + s; Horner from the top
  std::vector<std::pair<long, int>> terms;
  for (int ww = 0; ww < nwin_; ++ww) {
    terms.emplace_back((long)c * ww, 2 * ww);
    terms.emplace_back((long)c * ww + sbits_, 2 * ww + 1);
  }
  std::sort(terms.begin(), terms.end());
  hfp::Jac<HF> acc = T[terms.back().second];
  long e = terms.back().first;
  for (int k = (int)terms.size() - 2; k >= 0; --k) {
    for (; e > terms[k].first; --e) acc = hfp::dbl(acc);
    acc = hfp::addj(acc, T[terms[k].second]);
  }
  for (; e > 0; --e) acc = hfp::dbl(acc);
  return acc;
}

template <int G>
hfp::Jac<typename HostField<G>::F> WeightedReducer<G>::read_total(hipStream_t s, int c) {
  if (bits_ && nout_.size() >= 2) {  // one-window plan ended in bit sums (launch_tail): its T_0 is the total
    const std::vector<hfp::Jac<HF>> T = read_windows(s);
    return horner(T, c);
  }
  std::vector<uint8_t> host(out_bytes());
  copy_out(s, 0, host.data());
  MSM_HIP_CHECK(hipStreamSynchronize(s));
  return combine_windows(host.data(), c);
}

template class WeightedReducer<MSM_GROUP>;

// ------------------------------------------------------------------ Ches --
template <int G>
Ches<G>::Ches(int device, const ChesParams &p) : dev_(device), p_(p) {
  DeviceGuard g(dev_);
  if (p.q_exp < 2 || p.q_exp > 24 || p.h < 1 || p.h > 32 || (long)p.q_exp * p.h < 255)
    throw std::runtime_error("bad CHES parameters");
  const int q = 1 << p.q_exp;
  B_ = ches_bucket_set(q, p.a_h);
  if (p.b_size > 0 && (int)B_.size() != p.b_size)
    throw std::runtime_error("bucket set size " + std::to_string(B_.size()) + " != configured " +
                             std::to_string(p.b_size));
  std::vector<uint32_t> code, rank;
  ches_digit_code(B_, q, code, rank);
  code_.ensure(code.size() * 4);
  rank_.ensure(rank.size() * 4);
  MSM_HIP_CHECK(hipMemcpy(code_.p, code.data(), code.size() * 4, hipMemcpyHostToDevice));
  MSM_HIP_CHECK(hipMemcpy(rank_.p, rank.data(), rank.size() * 4, hipMemcpyHostToDevice));
  for (size_t k = 1; k < B_.size() && B_[k] <= p.a_h + 1; ++k) small_ = (int)k;
  plan_buckets(0);
  ev_.resize(8);
  for (auto &e : ev_) MSM_HIP_CHECK(hipEventCreate(&e));
}
template <int G>
Ches<G>::~Ches() {
  for (auto &e : ev_) (void)hipEventDestroy(e);
  for (auto &e : acc_ev_) (void)hipEventDestroy(e);
  for (auto &e : bev_) (void)hipEventDestroy(e);
  for (int t = 0; t < kBSets; ++t) {
    if (ev_tail_[t]) (void)hipEventDestroy(ev_tail_[t]);
    if (tails_[t]) (void)hipStreamDestroy(tails_[t]);
  }
  if (host_out_) (void)hipHostFree(host_out_);
  if (host_bits_) (void)hipHostFree(host_bits_);
  if (fstream_) (void)hipStreamDestroy(fstream_);
  if (cstream_) (void)hipStreamDestroy(cstream_);
}

// bucket space = B plus (copies_ - 1) copies of the small buckets 1..small_;
// copies_ is chosen so a copy receives ~kTopCopyLen top-digit entries
// (n / (small_ copies)).  Every copy is one more bucket, two general adds in
// level 0 of the reduction; a longer copy is a longer accumulation lane.
// MSM_TOP_COPY_LEN: A/B knob (12 / 24 / 32 measured: 12 is the fastest at 2^20
// and at the 2^17 shard).
constexpr int kTopCopyLen = 12;
template <int G>
void Ches<G>::plan_buckets(size_t n) {
  static const size_t len = [] {
    const char *e = getenv("MSM_TOP_COPY_LEN");
    return (size_t)(e ? std::max(1, std::min(4096, atoi(e))) : kTopCopyLen);
  }();
  int want = 1;
  if (small_ > 0 && n > 0) {
    size_t c = (n + (size_t)small_ * len - 1) / ((size_t)small_ * len);
    want = (int)std::min<size_t>(std::max<size_t>(c, 1), 256);
  }
  if (want == copies_ && red_.size()) return;
  copies_ = want;
  std::vector<uint32_t> w(B_.begin(), B_.end());
  for (int c = 1; c < copies_; ++c)
    for (int k = 1; k <= small_; ++k) w.push_back((uint32_t)B_[k]);
  if (w.size() >= (1u << 24)) throw std::runtime_error("CHES bucket space exceeds 24-bit indices");
  red_.plan(w);
  const int bc_env = BatchKnobs::env().batch_l0_chunk;  // the batch reducer's level-0 chunk (0: red_'s)
  if (bc_env && red_.level0_chunk() != bc_env) {
    bred_.plan(w, bc_env);
    batch_red_ = &bred_;
  } else {
    batch_red_ = &red_;
  }
}

// Accumulation lanes of a batch (run_batch): 3 (G1) or 2 (G2) when one
// accumulation's lanes (one per bucket for G1, two for G2) fill fewer than ~3 rounds of the chip's
// wave slots (1024 SIMDs x the kernel's waves per SIMD x 64 lanes: 3 for
// k_accumulate<1>, 2 for k_accumulate2p), else 1.  MSM_BATCH_LANES=1|2|3
// overrides.
template <int G>
int Ches<G>::batch_lanes() const {
  if (const int env = BatchKnobs::env().batch_lanes) return env;
  // G1 small MSMs take three lanes since round 4's single reduction group per
  // batch (2^17 / 2^18 / 2^19 batches 0.52 / 0.86 / 1.40 -> 0.49 / 0.80 / 1.35
  // ms per MSM, profiles/archive_r01_r04.txt (r04_small_lanes_ab.txt)); G2 keeps two (not measured)
  const size_t lanes = bucket_count() * (G == 2 ? 2 : 1);
  return lanes < (size_t)3 * (G == 2 ? 2 : 3) * 1024 * 64 ? (G == 1 ? 3 : 2) : 1;
}

template <int G>
void Ches<G>::build_table(const void *pts, size_t n, bool on_device, hipStream_t s) {
  typedef typename FieldOf<G>::F F;
  DeviceGuard g(dev_);
  const size_t K = 3 * (size_t)p_.h;
  if (n == 0) {
    n_ = 0;
    return;
  }
  if (K * n >= (1ull << 31)) throw std::runtime_error("CHES table too large for 31-bit slots");
  const size_t raw = n * 96 * G;
  const void *src = pts;
  DevBuf stage, base;
  if (!on_device) {
    stage.ensure(raw);
    MSM_HIP_CHECK(hipMemcpyAsync(stage.p, pts, raw, hipMemcpyHostToDevice, s));
    src = stage.p;
  }
  base.ensure(n * sizeof(Aff<F>));
  hipLaunchKernelGGL(k_convert_points<G>, dim3(nblk(n, 256)), dim3(256), 0, s, (const uint64_t *)src,
                     base.as<Aff<F>>(), n);
  MSM_HIP_CHECK(hipGetLastError());
  table_.ensure(K * n * sizeof(AffP<F>));
  const size_t chunk = std::min<size_t>(n, (size_t)1 << 16);
  DevBuf scratch, pref;
  scratch.ensure(K * chunk * sizeof(Xyzz<F>));
  pref.ensure(K * chunk * sizeof(F));
  for (size_t i0 = 0; i0 < n; i0 += chunk) {
    size_t cnt = std::min(chunk, n - i0);
    if constexpr (G == 2)  // lane pairs: no spills (pair_kernels.hpp)
      hipLaunchKernelGGL((k_ches_table2p<3>), dim3(nblk(2 * cnt, 128)), dim3(128), 0, s, base.as<Aff<F>>(), i0, cnt,
                         p_.q_exp, p_.h, scratch.as<Xyzz<F>>(), pref.as<F>(), table_.as<AffP<F>>());
    else
      hipLaunchKernelGGL((k_ches_table<G, 3>), dim3(nblk(cnt, 64)), dim3(64), 0, s, base.as<Aff<F>>(), i0, cnt,
                         p_.q_exp, p_.h, scratch.as<Xyzz<F>>(), pref.as<F>(), table_.as<AffP<F>>());
    MSM_HIP_CHECK(hipGetLastError());
  }
  MSM_HIP_CHECK(hipStreamSynchronize(s));
  n_ = n;
  plan_buckets(n);
}

template <int G>
void Ches<G>::reserve_table(size_t n) {
  typedef typename FieldOf<G>::F F;
  DeviceGuard g(dev_);
  const size_t cnt = 3 * (size_t)p_.h * n;
  if (cnt >= (1ull << 31)) throw std::runtime_error("table too large for 31-bit slots");
  table_.ensure(std::max<size_t>(cnt, 1) * sizeof(AffP<F>));
  n_ = n;
  plan_buckets(n);
}

template <int G>
void Ches<G>::put_table(const void *tab, size_t first, size_t count, bool on_device, hipStream_t s) {
  typedef typename FieldOf<G>::F F;
  DeviceGuard g(dev_);
  if (first + count > table_rows()) throw std::runtime_error("table rows out of range");
  if (!count) return;
  const void *src = tab;
  DevBuf stage;
  if (!on_device) {
    stage.ensure(count * 96 * G);
    MSM_HIP_CHECK(hipMemcpyAsync(stage.p, tab, count * 96 * G, hipMemcpyHostToDevice, s));
    src = stage.p;
  }
  hipLaunchKernelGGL((k_convert_points<G, AffP<F>>), dim3(nblk(count, 256)), dim3(256), 0, s, (const uint64_t *)src,
                     table_.as<AffP<F>>() + first, count);
  MSM_HIP_CHECK(hipGetLastError());
  MSM_HIP_CHECK(hipStreamSynchronize(s));
}

template <int G>
void Ches<G>::set_table(const void *tab, size_t n, bool on_device, hipStream_t s) {
  reserve_table(n);
  put_table(tab, 0, table_rows(), on_device, s);
}

template <int G>
void Ches<G>::get_table(void *out, size_t first, size_t count, hipStream_t s) {
  typedef typename FieldOf<G>::F F;
  DeviceGuard g(dev_);
  if (first + count > 3 * (size_t)p_.h * n_) throw std::runtime_error("table range out of bounds");
  if (!count) return;
  DevBuf o;
  o.ensure(count * 96 * G);
  hipLaunchKernelGGL((k_export_affine<G, AffP<F>>), dim3(nblk(count, 256)), dim3(256), 0, s,
                     table_.as<AffP<F>>() + first, o.as<uint64_t>(), count);
  MSM_HIP_CHECK(hipGetLastError());
  MSM_HIP_CHECK(hipMemcpyAsync(out, o.p, count * 96 * G, hipMemcpyDeviceToHost, s));
  MSM_HIP_CHECK(hipStreamSynchronize(s));
}

template <int G>
void Ches<G>::digits_sort(hipStream_t s, const uint8_t *d_scalars, size_t stride, size_t set_stride, int nsets,
                          int set, int fine_bt) {
  const size_t n = n_, h = (size_t)p_.h, ne = n * h, NB = bucket_count();
  ChesFrontSet &f = fs_[set];
  f.sort.fine_bt = fine_bt;
  f.sorted.ensure(ne * nsets * 4 + 64);  // + the accumulation's 16-B payload window past a run's end
  f.counts.ensure(NB * nsets * 4);
  f.offsets.ensure(NB * nsets * 4);
  f.order.ensure(NB * nsets * 4);
  // Fused front (the h of every reference configuration): the digits are
  // computed twice -- counted per coarse bin, then binned -- instead of being
  // written as keys / vals and read back twice by the sort (5 launches after
  // the scan's 2 instead of 8; MSM_FRONT_FUSED=0 selects the unfused front)
  static const bool fused_env = [] {
    const char *e = getenv("MSM_FRONT_FUSED");
    return !e || atoi(e) != 0;
  }();
  if (fused_env && (p_.h == 12 || p_.h == 13 || p_.h == 14 || p_.h == 16 || p_.h == 19 || p_.h == 20)) {
    const int ntiles = (int)nblk(n, 256);
    const BucketSort::Geom g = f.sort.prepare(s, ne, (uint32_t)NB, nsets, ntiles);
#define MSM_CHES_FRONT(HT)                                                                                             \
  do {                                                                                                                 \
    hipLaunchKernelGGL(k_ches_front_hist<HT>, dim3(ntiles, nsets), dim3(256), 0, s, d_scalars, stride, n, p_.q_exp,   \
                       code_.as<uint32_t>(), rank_.as<uint2>(), (uint32_t)B_.size(), (uint32_t)small_,                 \
                       (uint32_t)copies_, set_stride, g.fb_bits, g.ncb, g.ntiles, f.sort.ghist.as<uint32_t>(),         \
                       f.sort.classes.as<uint32_t>());                                                                  \
    MSM_HIP_CHECK(hipGetLastError());                                                                                  \
    if (profile_) MSM_HIP_CHECK(hipEventRecord(ev_[1], s));                                                            \
    f.sort.scan(s, g);                                                                                                 \
    hipLaunchKernelGGL(k_ches_front_coarse<HT>, dim3(ntiles, nsets), dim3(256), (size_t)(2 * g.ncb + 512 * HT) * 4, s, \
                       d_scalars, stride, n, p_.q_exp, code_.as<uint32_t>(), rank_.as<uint2>(), (uint32_t)B_.size(),  \
                       (uint32_t)small_, (uint32_t)copies_, set_stride, g.fb_bits, g.ncb, g.ntiles,                   \
                       f.sort.gbase.as<uint32_t>(), f.sort.okeys.as<uint32_t>(), f.sort.ovals.as<uint32_t>());         \
    MSM_HIP_CHECK(hipGetLastError());                                                                                  \
  } while (0)
    switch (p_.h) {
      case 12: MSM_CHES_FRONT(12); break;
      case 13: MSM_CHES_FRONT(13); break;
      case 14: MSM_CHES_FRONT(14); break;
      case 16: MSM_CHES_FRONT(16); break;
      case 19: MSM_CHES_FRONT(19); break;
      default: MSM_CHES_FRONT(20); break;
    }
#undef MSM_CHES_FRONT
    f.sort.finish(s, g, ne, (uint32_t)NB, f.sorted.as<uint32_t>(), f.counts.as<uint32_t>(), f.offsets.as<uint32_t>(),
                  f.order.as<uint32_t>(), nsets);
    return;
  }
  f.keys.ensure(ne * nsets * 4);
  f.vals.ensure(ne * nsets * 4);
#define MSM_CHES_DIGITS(HT)                                                                                   \
  hipLaunchKernelGGL(k_ches_digits<HT>, dim3(nblk(n, 256), nsets), dim3(256), 0, s, d_scalars, stride, n, p_.q_exp, \
                     p_.h, code_.as<uint32_t>(), rank_.as<uint2>(), f.keys.as<uint32_t>(), f.vals.as<uint32_t>(),     \
                     (uint32_t)B_.size(), (uint32_t)small_, (uint32_t)copies_, set_stride)
  switch (p_.h) {  // the h of the reference configurations (ches_config_files)
    case 12: MSM_CHES_DIGITS(12); break;
    case 13: MSM_CHES_DIGITS(13); break;
    case 14: MSM_CHES_DIGITS(14); break;
    case 16: MSM_CHES_DIGITS(16); break;
    case 19: MSM_CHES_DIGITS(19); break;
    case 20: MSM_CHES_DIGITS(20); break;
    default: MSM_CHES_DIGITS(0); break;
  }
#undef MSM_CHES_DIGITS
  MSM_HIP_CHECK(hipGetLastError());
  if (profile_) MSM_HIP_CHECK(hipEventRecord(ev_[1], s));
  f.sort.run(s, f.keys.as<uint32_t>(), f.vals.as<uint32_t>(), ne, (uint32_t)NB, f.sorted.as<uint32_t>(),
             f.counts.as<uint32_t>(), f.offsets.as<uint32_t>(), f.order.as<uint32_t>(), nsets);
}

template <int G>
void Ches<G>::accumulate(hipStream_t s, int set, int r, int bset, const void *table) {
  typedef typename FieldOf<G>::F F;
  const size_t NB = bucket_count();
  ChesFrontSet &f = fs_[set];
  buckets_[bset].ensure(NB * sizeof(Xyzz<F>));
  launch_accumulate<G>(s, f.sort.sched(f.order.as<uint32_t>(), f.sorted.as<uint32_t>(), r, NB),
                       table ? static_cast<const AffP<F> *>(table) : table_.as<AffP<F>>(),
                       buckets_[bset].as<Xyzz<F>>(), NB);
  MSM_HIP_CHECK(hipGetLastError());
}

template <int G>
void Ches<G>::accumulate_sets(hipStream_t s, int set, int R, int gb, const void *table) {
  typedef typename FieldOf<G>::F F;
  const size_t NB = bucket_count();
  ChesFrontSet &f = fs_[set];
  launch_accumulate_sets<G>(s, f.sort.sched(f.order.as<uint32_t>(), f.sorted.as<uint32_t>(), 0, NB), f.sort.stride(NB),
                            table ? static_cast<const AffP<F> *>(table) : table_.as<AffP<F>>(),
                            gbuckets_[gb].as<Xyzz<F>>(), NB, R);
  MSM_HIP_CHECK(hipGetLastError());
}

template <int G>
float Ches<G>::time_accumulation(hipStream_t s, const uint8_t *d_scalars, size_t set_stride, int nsets, int reps) {
  DeviceGuard g(dev_);
  if (n_ == 0 || nsets < 1 || reps < 1) throw std::runtime_error("time_accumulation: no table / bad arguments");
  digits_sort(s, d_scalars, 32, set_stride, nsets, 0);
  gbuckets_[0].ensure((size_t)nsets * bucket_count() * sizeof(Xyzz<typename FieldOf<G>::F>));
  accumulate_sets(s, 0, nsets, 0, nullptr);  // warm
  hipEvent_t a, b;
  MSM_HIP_CHECK(hipEventCreate(&a));
  MSM_HIP_CHECK(hipEventCreate(&b));
  MSM_HIP_CHECK(hipEventRecord(a, s));
  for (int r = 0; r < reps; ++r) accumulate_sets(s, 0, nsets, 0, nullptr);
  MSM_HIP_CHECK(hipEventRecord(b, s));
  MSM_HIP_CHECK(hipEventSynchronize(b));
  float ms = 0;
  MSM_HIP_CHECK(hipEventElapsedTime(&ms, a, b));
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  return ms / (float)reps;
}

template <int G>
void Ches<G>::run(hipStream_t s, const uint8_t *d_scalars, size_t stride, hfp::Jac<HF> *out) {
  DeviceGuard g(dev_);
  if (stride < 32) throw std::runtime_error("CHES scalars must be 32-byte strings");
  if (n_ == 0) {
    std::memset(out, 0, sizeof(*out));
    return;
  }
  if (profile_) MSM_HIP_CHECK(hipEventRecord(ev_[0], s));
  digits_sort(s, d_scalars, stride, 0, 1, 0);
  if (profile_) MSM_HIP_CHECK(hipEventRecord(ev_[2], s));
  accumulate(s, 0, 0, 0);
  if (profile_) MSM_HIP_CHECK(hipEventRecord(ev_[3], s));
  red_.launch(s, buckets_[0].p);
  if (profile_) MSM_HIP_CHECK(hipEventRecord(ev_[4], s));
  *out = red_.read(s);
  if (profile_) {
    MSM_HIP_CHECK(hipEventRecord(ev_[5], s));
    MSM_HIP_CHECK(hipEventSynchronize(ev_[5]));
    float ms;
    MSM_HIP_CHECK(hipEventElapsedTime(&ms, ev_[0], ev_[1]));
    times_.digits = ms;
    MSM_HIP_CHECK(hipEventElapsedTime(&ms, ev_[1], ev_[2]));
    times_.sort = ms;
    MSM_HIP_CHECK(hipEventElapsedTime(&ms, ev_[2], ev_[3]));
    times_.accumulate = ms;
    MSM_HIP_CHECK(hipEventElapsedTime(&ms, ev_[3], ev_[4]));
    times_.reduce = ms;
    MSM_HIP_CHECK(hipEventElapsedTime(&ms, ev_[4], ev_[5]));
    times_.finalize = ms;
    MSM_HIP_CHECK(hipEventElapsedTime(&ms, ev_[0], ev_[5]));
    times_.total = ms;
    times_.accumulate_launches = 1;
  }
}

// The batch (run_jobs): plan, sink and issue loops in batch_plan.hpp, DESIGN 29.

// every operation of the issue loops as the one HIP call or launch it stands for
template <int G>
struct Ches<G>::BatchSink {
  Ches &e;
  const BatchPlan &p;
  WeightedReducer<G> &red;
  hipStream_t st[kBatchStreams];
  const uint8_t *scalars;
  size_t stride, set_stride;
  const void *const *tables;
  // where the groups' window sums land: the pinned read-back slots, or the
  // caller's device exchange buffer (dev_out: ChesMulti gathers it over RCCL
  // and combines on the host; the host combine is then skipped)
  uint8_t *out_base;
  bool prof;
  std::vector<size_t> prof_k;  // profiling: acc_ev_ pairs recorded (per MSM, or per accumulation group)

  hipEvent_t ev(size_t i) const { return i < p.events ? e.bev_[i] : e.ev_tail_[i - p.events]; }
  const uint8_t *job_scalars(size_t k) const {
    return scalars + (k / p.nseg) * set_stride + (k % p.nseg) * e.n_ * stride;
  }
  const void *job_table(size_t k) const { return tables[k % p.nseg]; }
  uint8_t *slots(size_t g) const { return e.scal_.template as<uint8_t>() + (g % p.nsg) * p.fg_max * p.sslot; }

  void wait(int s, size_t i) { MSM_HIP_CHECK(hipStreamWaitEvent(st[s], ev(i), 0)); }
  void record(size_t i, int s) { MSM_HIP_CHECK(hipEventRecord(ev(i), st[s])); }
  void host_wait(size_t i) { MSM_HIP_CHECK(hipEventSynchronize(ev(i))); }
  void sync(int s) { MSM_HIP_CHECK(hipStreamSynchronize(st[s])); }
  void copy_set(size_t g, size_t k) {
    MSM_HIP_CHECK(hipMemcpyAsync(slots(g) + (k - p.fgb[g]) * p.sslot, job_scalars(k), p.sslot, hipMemcpyHostToDevice,
                                 st[kCopy]));
  }
  void front(size_t g) {
    e.digits_sort(st[kFront], p.host ? slots(g) : job_scalars(p.fgb[g]), stride, p.host ? p.sslot : p.jstride,
                  (int)(p.fgb[g + 1] - p.fgb[g]), (int)(g % p.nfr), p.fine_bt);
  }
  void accumulate(int s, size_t g, size_t k, int bset) {
    e.accumulate(st[s], (int)(g % p.nfr), (int)(k - p.fgb[g]), bset, job_table(k));
  }
  void accumulate_group(int s, size_t g, int gb) {
    e.accumulate_sets(st[s], (int)(g % p.nfr), (int)(p.fgb[g + 1] - p.fgb[g]), gb, job_table(p.fgb[g]));
  }
  void level0(int s, int bset, int rset, int slot) { red.launch_head_slot(st[s], e.buckets_[bset].p, rset, slot); }
  void level0_group(int s, int gb, size_t off, int rset, int slot0, int m) {
    const size_t NB = e.bucket_count();
    red.launch_head_slots(st[s], e.gbuckets_[gb].template as<uint8_t>() + off * NB * sizeof(Xyzz<typename FieldOf<G>::F>),
                          NB, rset, slot0, m);
  }
  // the dense stage into the read-back slots, or (the last group, bit_tail) the bit phase into host_bits_
  void tail(int s, int rset, size_t first, size_t m, bool last) {
    if (p.bit_tail && last) {
      red.launch_tail_group_bits(st[s], rset, (int)m, p.tail_coop);
      red.copy_out_group_bits(st[s], rset, (int)m, e.host_bits_);
    } else {
      red.launch_tail_group(st[s], rset, (int)m, p.tail_coop && last);
      red.copy_out_group(st[s], rset, (int)m, out_base + first * red.out_bytes());
    }
  }
  void combine(size_t, size_t) {}
  void prof_begin(int s, size_t k) {
    if (prof) MSM_HIP_CHECK(hipEventRecord(e.acc_ev_[2 * k], st[s]));
  }
  void prof_end(int s, size_t k) {
    if (!prof) return;
    MSM_HIP_CHECK(hipEventRecord(e.acc_ev_[2 * k + 1], st[s]));
    prof_k.push_back(k);
  }
};

// The batch's own streams, created at the first batch.  Fronts at the greatest
// priority: their short memory-bound kernels take the first CU slots an
// accumulation releases (the next accumulation waits for them); the reductions
// at normal priority, beside the accumulations (the same priority for both
// measured equal, tools/batch_sched.py).
template <int G>
void Ches<G>::batch_streams() {
  if (fstream_) return;
  int least = 0, greatest = 0;
  MSM_HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
  MSM_HIP_CHECK(hipStreamCreateWithPriority(&fstream_, hipStreamNonBlocking, greatest));
  for (int t = 0; t < kBSets; ++t) {
    MSM_HIP_CHECK(hipStreamCreateWithPriority(&tails_[t], hipStreamNonBlocking, 0));
    MSM_HIP_CHECK(hipEventCreateWithFlags(&ev_tail_[t], hipEventDisableTiming));
  }
  MSM_HIP_CHECK(hipStreamCreateWithFlags(&cstream_, hipStreamNonBlocking));
  // a stream's hardware queue is set up at its first launch: do that here,
  // not inside the first batch that happens to use the stream
  prime_.ensure(256);
  for (hipStream_t q : {fstream_, tails_[0], tails_[1], cstream_}) MSM_HIP_CHECK(hipMemsetAsync(prime_.p, 0, 256, q));
  for (hipStream_t q : {fstream_, tails_[0], tails_[1], cstream_}) MSM_HIP_CHECK(hipStreamSynchronize(q));
}

template <int G>
BatchPlan Ches<G>::batch_plan(size_t nsets, size_t nseg, size_t stride, size_t set_stride, bool scalars_on_host,
                              bool dev_out) const {
  BatchShape z;
  z.nsets = nsets, z.nseg = nseg, z.n = n_, z.stride = stride, z.set_stride = set_stride, z.h = p_.h;
  z.buckets = bucket_count(), z.lanes = batch_lanes(), z.group = G;
  z.host = scalars_on_host, z.dev_out = dev_out, z.bit_tail_ok = batch_red_->has_bit_tail();
  z.bucket_bytes = sizeof(Xyzz<typename FieldOf<G>::F>);
  z.out_bytes = batch_red_->out_bytes(), z.bit_bytes = batch_red_->bit_bytes();
  return BatchPlan::ches(z, BatchKnobs::env());
}

static void ensure_pinned(void *&buf, size_t &have, size_t need, size_t alloc) {
  if (have >= need) return;
  if (buf) (void)hipHostFree(buf);
  buf = nullptr;
  have = 0;
  MSM_HIP_CHECK(hipHostMalloc(&buf, alloc, hipHostMallocDefault));
  have = alloc;
}

// every buffer and event the issue loops touch exists before the first launch
template <int G>
void Ches<G>::batch_buffers(const BatchPlan &p, hipStream_t s, size_t stride) {
  ensure_pinned(host_out_, host_out_bytes_, p.out_need, p.out_alloc);
  ensure_pinned(host_bits_, host_bits_bytes_, p.bits_need, p.bits_alloc);
  for (int b = 0; b < p.bucket_sets; ++b) (p.sched == kAccGroups ? gbuckets_ : buckets_)[b].ensure(p.bucket_set_bytes);
  if ((int)fs_.size() < p.nfr) fs_.resize(p.nfr);
  for (int t = 0; t < p.nred; ++t) batch_red_->ensure_group(t, (int)p.group_max);
  // front sets sized for a whole front group (the sort's scan scratch too): run
  // one sort of fg_max sets per set before the loop if they are not yet sized
  // (fg_max dummy sets of all-zero scalars, outside the batch timing)
  bool unsized = false;
  for (int f = 0; f < p.nfr; ++f) unsized |= fs_[f].sorted.bytes < p.sorted_min;
  scal_.ensure(p.scal_bytes);
  if (unsized) scal_.ensure(p.scal_dummy_bytes);
  for (int f = 0; f < p.nfr; ++f)
    if (fs_[f].sorted.bytes < p.sorted_min) {
      MSM_HIP_CHECK(hipMemsetAsync(scal_.p, 0, p.fg_max * p.sslot, s));
      digits_sort(s, scal_.as<uint8_t>(), stride, p.sslot, (int)p.fg_max, f);
      MSM_HIP_CHECK(hipStreamSynchronize(s));
    }
  while (profile_ && acc_ev_.size() < std::max<size_t>(2 * p.count, 2 * 64)) {
    hipEvent_t e;
    MSM_HIP_CHECK(hipEventCreate(&e));
    acc_ev_.push_back(e);
  }
  while (bev_.size() < std::max(p.events, p.events_floor)) {
    hipEvent_t e;
    MSM_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    bev_.push_back(e);
  }
}

// the per-MSM host Horner (~20 us each) over the host worker threads (with one
// reduction group per batch every combine runs after the last tail), and the
// profiling read-out: accumulation time per MSM over the batch
template <int G>
void Ches<G>::batch_finish(const BatchPlan &p, const std::vector<size_t> &prof_k, hfp::Jac<HF> *outs, bool dev_out,
                           bool prof) {
  WeightedReducer<G> &red = *batch_red_;
  const size_t ob = red.out_bytes(), bb = red.bit_bytes();
  const size_t last_first = p.rg.first(p.rg.groups() - 1);  // the last group's MSMs: host_bits_ when bit_tail
  auto combine_k = [&](size_t k) {
    outs[k] = p.bit_tail && k >= last_first ? red.combine_bits((const uint8_t *)host_bits_ + (k - last_first) * bb)
                                            : red.combine((const uint8_t *)host_out_ + k * ob)[0];
  };
  if (dev_out) {
    // the window sums stay in dev_out for the caller's exchange
  } else if (p.count >= 4) {
    WorkerPool::get().parallel_for(p.count, combine_k);
  } else {
    for (size_t k = 0; k < p.count; ++k) combine_k(k);
  }
  if (!prof) return;
  float sum = 0;
  for (size_t k : prof_k) {
    float ms;
    MSM_HIP_CHECK(hipEventSynchronize(acc_ev_[2 * k + 1]));
    MSM_HIP_CHECK(hipEventElapsedTime(&ms, acc_ev_[2 * k], acc_ev_[2 * k + 1]));
    sum += ms;
  }
  times_ = PhaseTimes();
  times_.accumulate = sum / (float)p.count;
  times_.accumulate_launches = (int)prof_k.size();
}

template <int G>
void Ches<G>::run_jobs(hipStream_t s, const uint8_t *scalars, size_t stride, size_t set_stride, size_t nsets,
                       size_t nseg, const void *const *tables, hfp::Jac<HF> *outs, bool scalars_on_host,
                       void *dev_out) {
  DeviceGuard g(dev_);
  if (stride < 32) throw std::runtime_error("CHES scalars must be 32-byte strings");
  if (nseg < 1) throw std::runtime_error("run_jobs: no segments");
  if (nsets * nseg == 0) return;
  if (n_ == 0) {
    std::memset(outs, 0, sizeof(*outs) * nsets * nseg);
    return;
  }
  batch_streams();
  const BatchPlan p = batch_plan(nsets, nseg, stride, set_stride, scalars_on_host, dev_out != nullptr);
  batch_buffers(p, s, stride);
  const bool prof = profile_;
  profile_ = false;
  BatchSink sink{*this,  p,          *batch_red_, {s, tails_[0], tails_[1], fstream_, cstream_},
                 scalars, stride,    set_stride,  tables,
                 static_cast<uint8_t *>(dev_out ? dev_out : host_out_), prof, {}};
  BatchIssue<BatchSink>(p, sink).run();
  profile_ = prof;
  batch_finish(p, sink.prof_k, outs, dev_out != nullptr, prof);
}

template class Ches<MSM_GROUP>;

}  // namespace msm
