// ches.hip -- host orchestration of the CHES "nh + q/5" bucket-set MSM
// (LuoGuiwen/MSM_blst, method `pippenger_variant_q_over_5_CHES`,
// ref main_p1.cpp:192-246) on one MI355X.
//
// Setup (once per context): parameters of ref ches_config_files, bucket set B
// (ref auxiliaryfunc.h:257-288), digit hash (ref main_p1.cpp:140-152), all three
// group-independent host code in ches_setup.hpp, and the
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
#include "fp_ops_test.hpp"
#include "hoststage.hpp"
#include "pair_kernels.hpp"

#ifndef MSM_GROUP
#error "define MSM_GROUP (1 or 2)"
#endif

namespace msm {

static_assert(kChesHashIdxMask == CH_IDX_MASK, "ches_setup.hpp and ches_kernels.hpp disagree on the digit hash layout");

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

// One step of the dense stage.  coop: one add over 4 waves (coop.hpp), for
// steps of at most dense_coop_max() adds; else one add per lane (G2: per lane
// pair, fp2l.hpp).  A suffix step is W S adds, a pair step `half`.
template <int G>
static void launch_suffix_step(hipStream_t s, const Xyzz<typename FieldOf<G>::F> *src,
                               Xyzz<typename FieldOf<G>::F> *dst, int S, int d, int W, bool coop) {
  const size_t NT = (size_t)W * S;
  coop = coop && NT <= dense_coop_max();
  if constexpr (G == 2) {
    if (coop) hipLaunchKernelGGL(k_suffix_step_c2p, dim3(nblk(NT, 32)), dim3(256), 0, s, src, dst, S, d, W);
    else hipLaunchKernelGGL(k_suffix_step2p, dim3(nblk(2 * NT, 64)), dim3(64), 0, s, src, dst, S, d, W);
  } else {
    if (coop) hipLaunchKernelGGL(k_suffix_step_c<G>, dim3(nblk(NT, 64)), dim3(256), 0, s, src, dst, S, d, W);
    else hipLaunchKernelGGL(k_suffix_step<G>, dim3(nblk(NT, 64)), dim3(64), 0, s, src, dst, S, d, W);
  }
}
template <int G>
static void launch_pair_step(hipStream_t s, const Xyzz<typename FieldOf<G>::F> *src, Xyzz<typename FieldOf<G>::F> *dst,
                             size_t half, bool coop) {
  coop = coop && half <= dense_coop_max();
  if constexpr (G == 2) {
    if (coop) hipLaunchKernelGGL(k_pair_step_c2p, dim3(nblk(half, 32)), dim3(256), 0, s, src, dst, half);
    else hipLaunchKernelGGL(k_pair_step2p, dim3(nblk(2 * half, 64)), dim3(64), 0, s, src, dst, half);
  } else {
    if (coop) hipLaunchKernelGGL(k_pair_step_c<G>, dim3(nblk(half, 64)), dim3(256), 0, s, src, dst, half);
    else hipLaunchKernelGGL(k_pair_step<G>, dim3(nblk(half, 64)), dim3(64), 0, s, src, dst, half);
  }
}

template <int G>
void ScanReducer<G>::launch(hipStream_t s, const void *Abuf, int W, int S, bool coop) {
  typedef typename FieldOf<G>::F F;
  if (S < 1 || (S & (S - 1))) throw std::runtime_error("ScanReducer: S must be a power of two");
  const size_t NT = (size_t)W * S;
  buf[0].ensure(NT * sizeof(Xyzz<F>));
  buf[1].ensure(NT * sizeof(Xyzz<F>));
  fin.ensure((size_t)W * 144 * G);
  const Xyzz<F> *src = reinterpret_cast<const Xyzz<F> *>(Abuf);
  int cur = 0;
  auto step = [&](auto &&launch_step) {
    Xyzz<F> *dst = buf[cur].as<Xyzz<F>>();
    launch_step(dst);
    MSM_HIP_CHECK(hipGetLastError());
    src = dst;
    cur ^= 1;
  };
  for (int d = 1; d < S; d <<= 1)  // suffix sums T_k = sum_{b >= k} A_b
    step([&](Xyzz<F> *dst) { launch_suffix_step<G>(s, src, dst, S, d, W, coop); });
  for (size_t len = NT; len > (size_t)W; len >>= 1)  // sum_k T_k = sum_b b A_b
    step([&](Xyzz<F> *dst) { launch_pair_step<G>(s, src, dst, len / 2, coop); });
  hipLaunchKernelGGL(k_finalize<G>, dim3(nblk(W, 64)), dim3(64), 0, s, src, fin.as<uint64_t>(), W);
  MSM_HIP_CHECK(hipGetLastError());
}
template struct ScanReducer<MSM_GROUP>;

// -------------------------------------------------------- weighted reducer --
// the plan (reduce_plan.hpp) and its tables on the device
template <int G>
void WeightedReducer<G>::plan(const std::vector<uint32_t> &w, const std::vector<uint32_t> &win, int nwin, int c0) {
  static const int C0env = [] {
    const char *e = getenv("MSM_L0_CHUNK");  // A/B knob: level-0 chunk length
    return e ? std::max(2, std::min(64, atoi(e))) : 0;
  }();
  plan_ = ReducePlan::build(w, win, nwin, C0env ? C0env : c0, G == 2 ? 2 : 1);
  steps_[kEndDense] = plan_.steps(kEndDense);
  steps_[kEndBits] = has_bit_tail() ? plan_.steps(kEndBits) : std::vector<ReduceStep>();
  starts_.clear();
  starts_.resize(plan_.levels());
  auto upload = [](DevBuf &d, const std::vector<uint32_t> &v) {
    d.ensure(std::max<size_t>(v.size(), 1) * 4);
    if (!v.empty()) MSM_HIP_CHECK(hipMemcpy(d.p, v.data(), v.size() * 4, hipMemcpyHostToDevice));
  };
  // the segment phase's scatter after the bit phase
  const int L = (int)plan_.seg.size(), LT = (int)plan_.levels();
  for (int t = 0; t < LT; ++t)
    if (t != L - 1) upload(starts_[t], plan_.level(t).starts);
  upload(starts_[L - 1], plan_.level(L - 1).starts);
  upload(idx_, plan_.items);
  for (int st = 0; st < NSETS; ++st) {  // a new plan: sets are (re)sized on their next use
    part_[st][0].release();
    part_[st][1].release();
    dense_buf_[st].release();
  }
}

template <int G>
void WeightedReducer<G>::ensure(int set, int nmsm) {
  typedef typename FieldOf<G>::F F;
  if (set < 0 || set >= NSETS || nmsm < 1) throw std::runtime_error("WeightedReducer: bad group");
  part_[set][0].ensure(plan_.elems(kRedPart0, nmsm) * sizeof(Xyzz<F>));
  part_[set][1].ensure(plan_.elems(kRedPart1, nmsm) * sizeof(Xyzz<F>));
  if (has_bit_tail()) bgfin_[set].ensure((size_t)nmsm * bit_bytes());
  const size_t NT = plan_.elems(kRedDense, nmsm);  // also ScanReducer::launch's buffers for W = 2 nwin nmsm
  dense_buf_[set].ensure(NT * sizeof(Xyzz<F>));
  dense_[set].buf[0].ensure(NT * sizeof(Xyzz<F>));
  dense_[set].buf[1].ensure(NT * sizeof(Xyzz<F>));
  dense_[set].fin.ensure((size_t)nmsm * out_bytes());
}

template <int G>
void WeightedReducer<G>::head(hipStream_t s, const void *Sbuf, size_t sstride, int set, int slot0, int nmsm) {
  typedef typename FieldOf<G>::F F;
  const ReduceStep &st = steps_[kEndDense].front();  // level 0 is the same in either ending
  launch_segsum<G>(s, reinterpret_cast<const Xyzz<F> *>(Sbuf), idx_.as<uint32_t>() + st.items,
                   starts_[st.level].template as<uint32_t>(),
                   buf(set, st.dst).template as<Xyzz<F>>() + (size_t)slot0 * st.dstride, plan_.level(st.level).nout, nmsm,
                   sstride, st.dstride);
  MSM_HIP_CHECK(hipGetLastError());
}

template <int G>
void WeightedReducer<G>::tail(hipStream_t s, int set, int nmsm, ReduceEnding end, bool coop) {
  typedef typename FieldOf<G>::F F;
  const std::vector<ReduceStep> &steps = steps_[end];
  if (steps.empty()) throw std::runtime_error("WeightedReducer: no bit tail in this plan");
  for (size_t k = 1; k < steps.size(); ++k) {
    const ReduceStep &st = steps[k];
    const size_t nout = plan_.level(st.level).nout;
    if (!nout) continue;
    launch_segsum_tail<G>(s, buf(set, st.src).template as<Xyzz<F>>(),
                          st.items == kNoItems ? nullptr : idx_.as<uint32_t>() + st.items,
                          starts_[st.level].template as<uint32_t>(), buf(set, st.dst).template as<Xyzz<F>>(), nout, coop,
                          nmsm, st.sstride, st.dstride);
    MSM_HIP_CHECK(hipGetLastError());
  }
  if (end == kEndDense) {
    dense_[set].launch(s, dense_buf_[set].p, 2 * plan_.nwin * nmsm, 1 << plan_.sbits, coop);
  } else {  // nmsm x 2 s bit sums to Jacobians; the host combines T = sum_j 2^j B_j (combine_bits)
    const int W = (int)((size_t)nmsm * plan_.bit_slots());
    hipLaunchKernelGGL(k_finalize<G>, dim3(nblk((size_t)W, 64)), dim3(64), 0, s, dense_buf_[set].as<Xyzz<F>>(),
                       bgfin_[set].as<uint64_t>(), W);
    MSM_HIP_CHECK(hipGetLastError());
  }
}

template <int G>
void WeightedReducer<G>::copy_out(hipStream_t s, int set, int nmsm, ReduceEnding end, void *dst, hipMemcpyKind kind) {
  const bool bits = end == kEndBits;
  MSM_HIP_CHECK(hipMemcpyAsync(dst, bits ? bgfin_[set].p : dense_[set].fin.p,
                               (size_t)nmsm * (bits ? bit_bytes() : out_bytes()), kind, s));
}

template <int G>
std::vector<hfp::Jac<typename HostField<G>::F>> WeightedReducer<G>::combine(const void *host) const {
  const hfp::Jac<HF> *T = reinterpret_cast<const hfp::Jac<HF> *>(host);
  std::vector<hfp::Jac<HF>> out(plan_.nwin);
  for (int ww = 0; ww < plan_.nwin; ++ww)
    out[ww] = horner(std::vector<hfp::Jac<HF>>{T[2 * ww], T[2 * ww + 1]}, plan_.sbits);
  return out;
}

// window 0's sum_b b S_b from its 2 s bit sums (bit j of the weight: low half
// block j < s, high half s + j): Horner from the top bit
template <int G>
hfp::Jac<typename HostField<G>::F> WeightedReducer<G>::combine_bits(const void *host) const {
  const int sbits = plan_.sbits;
  const hfp::Jac<HF> *B = reinterpret_cast<const hfp::Jac<HF> *>(host);
  const hfp::Jac<HF> *lo = B, *hi = B + sbits;
  hfp::Jac<HF> acc = hi[sbits - 1];
  for (int j = 2 * sbits - 2; j >= 0; --j) {
    acc = hfp::dbl(acc);
    acc = hfp::addj(acc, j >= sbits ? hi[j - sbits] : lo[j]);
  }
  return acc;
}

template <int G>
hfp::Jac<typename HostField<G>::F> WeightedReducer<G>::combine_windows(const void *host, int c) const {
  const hfp::Jac<HF> *T = reinterpret_cast<const hfp::Jac<HF> *>(host);
  // terms (exponent, point): L_w at c w, H_w at c w + s; Horner from the top
  std::vector<std::pair<long, int>> terms;
  for (int ww = 0; ww < plan_.nwin; ++ww) {
    terms.emplace_back((long)c * ww, 2 * ww);
    terms.emplace_back((long)c * ww + plan_.sbits, 2 * ww + 1);
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

// the synchronous reads of set 0 (after launch)
template <int G>
std::vector<hfp::Jac<typename HostField<G>::F>> WeightedReducer<G>::read_windows(hipStream_t s) {
  const ReduceEnding end = sync_ending();
  std::vector<uint8_t> host(end == kEndBits ? bit_bytes() : out_bytes());
  copy_out(s, 0, 1, end, host.data(), hipMemcpyDeviceToHost);
  MSM_HIP_CHECK(hipStreamSynchronize(s));
  if (end == kEndBits) return {combine_bits(host.data())};  // a one-window plan
  return combine(host.data());
}

template <int G>
hfp::Jac<typename HostField<G>::F> WeightedReducer<G>::read_total(hipStream_t s, int c) {
  if (sync_ending() == kEndBits) return read_windows(s)[0];  // one window: its T_0 is the total
  std::vector<uint8_t> host(out_bytes());
  copy_out(s, 0, 1, kEndDense, host.data(), hipMemcpyDeviceToHost);
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
  void level0(int s, int bset, int rset, int slot) {
    red.head(st[s], e.buckets_[bset].p, e.bucket_count(), rset, slot, 1);
  }
  void level0_group(int s, int gb, size_t off, int rset, int slot0, int m) {
    const size_t NB = e.bucket_count();
    red.head(st[s], e.gbuckets_[gb].template as<uint8_t>() + off * NB * sizeof(Xyzz<typename FieldOf<G>::F>), NB, rset,
             slot0, m);
  }
  // the dense stage into the read-back slots, or (the last group, bit_tail) the bit phase into host_bits_
  void tail(int s, int rset, size_t first, size_t m, bool last) {
    const ReduceEnding end = p.bit_tail && last ? kEndBits : kEndDense;
    red.tail(st[s], rset, (int)m, end, p.tail_coop && last);
    red.copy_out(st[s], rset, (int)m, end, end == kEndBits ? e.host_bits_ : out_base + first * red.out_bytes());
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
  for (int t = 0; t < p.nred; ++t) batch_red_->ensure(t, (int)p.group_max);
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

// msm_test_fp_ops, op 28 (fp_ops_test.hpp): the cooperative add through the
// dense stage's own pair step, launched as launch_pair_step launches it, on
// device 0, synchronously.  The whole out buffer makes the round trip, so the
// caller sees whether a slot past n was written.
template <int G>
void test_coop_pair_add(const uint32_t *in, uint32_t *out, size_t n, size_t cap) {
  typedef typename FieldOf<G>::F F;
  if (!n) return;
  DeviceGuard g(0);
  DevBuf din, dout;
  din.ensure(2 * n * sizeof(Xyzz<F>));
  dout.ensure(cap * sizeof(Xyzz<F>));
  MSM_HIP_CHECK(hipMemcpy(din.p, in, 2 * n * sizeof(Xyzz<F>), hipMemcpyHostToDevice));
  MSM_HIP_CHECK(hipMemcpy(dout.p, out, cap * sizeof(Xyzz<F>), hipMemcpyHostToDevice));
  // (not through launch_pair_step: MSM_DENSE_COOP_MAX must not choose another kernel here)
  if constexpr (G == 2)
    hipLaunchKernelGGL(k_pair_step_c2p, dim3(nblk(n, 32)), dim3(256), 0, 0, din.as<Xyzz<F>>(), dout.as<Xyzz<F>>(), n);
  else
    hipLaunchKernelGGL(k_pair_step_c<G>, dim3(nblk(n, 64)), dim3(256), 0, 0, din.as<Xyzz<F>>(), dout.as<Xyzz<F>>(), n);
  MSM_HIP_CHECK(hipGetLastError());
  MSM_HIP_CHECK(hipDeviceSynchronize());
  MSM_HIP_CHECK(hipMemcpy(out, dout.p, cap * sizeof(Xyzz<F>), hipMemcpyDeviceToHost));
}
template void test_coop_pair_add<MSM_GROUP>(const uint32_t *, uint32_t *, size_t, size_t);

}  // namespace msm
