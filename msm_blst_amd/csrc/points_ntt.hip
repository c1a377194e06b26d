// points_ntt.hip -- batched NTTs over group elements on one MI355X:
// dst[k] = sum_j [omega_n^(j k)] src[j] over n = 2^log_n affine points of G1 or
// G2, and its inverse (no reference counterpart: the loop a setup or an FK20
// prover writes over blst_p{1,2}_mult and blst_p{1,2}_add_or_double; DESIGN.md
// section 31).  The schedule -- passes, pairs, twiddle exponents, maps, slices --
// is points_ntt_plan.hpp; this file is its kernels and the loop that issues them.
//
// Data at rest between passes is Xyzz<F> in internal limbs, nothing is normalised
// per element.  Per chunk:
//   k_pn_load    blst affine source -> xyzz in x, through the input map
//   per pass, per slice of its items:
//     k_pn_bfly    (a level) S = A + B -> x[a], D = A - B -> x[b], the general
//                  xyzz_add: the doubling branch for A == B, infinity for A == -B
//     k_pn_table   (a pass that multiplies) the multiples 1D .. 8D of x[b] as xyzz:
//                  one xyzz_dbl, six general adds, restarting from D after a
//                  multiple that is infinity; row m of item u at xz[(m - 1) cnt + u]
//     (ta_tree)    the 8 cnt multiples -> canonical affine rows (TA_XYZZ_ROWS), so
//                  the ladder keeps the mixed addition
//     k_pn_ladder  the window loop of k_pm_ladder (pm_common.hpp) over 255 bits of
//                  the item's scalar tw + e 32 -> x[b]
//   k_pn_store   x through the output map -> a flat xyzz array
//   (ta_tree)    -> blst affine output (TA_XYZZ_BLST): the only normalisation of data
// k_pn_bfly and k_pn_table are two kernels where the issue's sketch has one: S, D
// and a chain of general adds in one body keep three xyzz points and the add's
// temporaries live; apart they each fit without spills in both groups, at the
// price of one more store and load of D per butterfly (224 G bytes against
// about 2900 field products).  The kernel boundary between writing the table and
// reading it is the tree's.
//
// G1 runs one lane per item, G2 one lane PAIR per item (Fp2L, fp2l.hpp); the
// zero tests combine the pair, so whole pairs take every branch.
//
// Products per butterfly of a laddered level as built (G1; an fp_mul2 priced
// 1.5, so the regrouped general add is 12.5; tools/points_ntt_timing.py): S and
// D 2 x 12.5, the table 8.5 + 6 x 12.5 = 83.5, its rows 8 x 8.6 = 69, the ladder
// 2712: 2890.  The last level costs 25, the n^-1 pass of the inverse one table,
// rows and ladder per ELEMENT: 2865.
#include "points_ntt.hpp"

#include <cstring>
#include <vector>

#include "pair_kernels.hpp"
#include "pm_common.hpp"
#include "points_ntt_model.hpp"
#include "to_affine.hpp"

#ifndef MSM_GROUP
#error "define MSM_GROUP (1 or 2)"
#endif

namespace msm {

// lane (pair) i < cnt (cnt a multiple of n): x[i] = the source point of its transform at pn_in_map
template <int G>
static __global__ void __launch_bounds__(128)
    k_pn_load(const uint64_t *__restrict__ pts, size_t cnt, int log_n, int flags,
              Xyzz<typename FieldOf<G>::F> *__restrict__ x) {
  typedef typename PmLane<G>::LF LF;
  const size_t tt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int comp = G == 2 ? (int)(tt & 1) : 0;
  const size_t i = G == 2 ? tt >> 1 : tt;
  if (i >= cnt) return;  // whole pairs only
  const size_t mask = ((size_t)1 << log_n) - 1;
  const uint64_t *src = pts + ((i & ~mask) + pn_in_map(log_n, flags, i & mask)) * 12 * G;
  Aff<LF> p;
  fp_from_blst(pm_c(p.x), src + 6 * comp);
  fp_from_blst(pm_c(p.y), src + 6 * G + 6 * comp);
  const bool zx = f_is_zero_exact(p.x), zy = f_is_zero_exact(p.y);
  Xyzz<LF> q;
  if (zx & zy) xyzz_set_inf(q);  // uniform over a pair
  else xyzz_from_aff(q, p, false);
  pm_st_xyzz(&x[i], q, comp);
}

// lane (pair) u < cnt: butterfly g0 + u of level `pass`
template <int G>
static __global__ void __launch_bounds__(128)
    k_pn_bfly(Xyzz<typename FieldOf<G>::F> *__restrict__ x, size_t g0, size_t cnt, int log_n, int pass) {
  typedef typename PmLane<G>::LF LF;
  const size_t tt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int comp = G == 2 ? (int)(tt & 1) : 0;
  const size_t u = G == 2 ? tt >> 1 : tt;
  if (u >= cnt) return;  // whole pairs only
  const int il = pn_items_log(log_n, pass);
  const size_t g = g0 + u, base = (g >> il) << log_n;
  const PnItem it = pn_item(log_n, pass, g & (((size_t)1 << il) - 1));
  Xyzz<LF> a, b;
  pm_ld_xyzz(a, &x[base + it.a], comp);
  pm_ld_xyzz(b, &x[base + it.b], comp);
  {
    Xyzz<LF> s = a;
    xyzz_add(s, b);
    pm_st_xyzz(&x[base + it.a], s, comp);
  }
  if (!xyzz_is_inf(b)) {  // -B, reduced as xyzz_from_aff reduces a negated Y
    LF y = b.y;
    f_neg4(b.y, y);
    f_nred(b.y);
  }
  xyzz_add(a, b);
  pm_st_xyzz(&x[base + it.b], a, comp);
}

// lane (pair) u < cnt: xz[(m - 1) cnt + u] = [m] D for m = 1 .. 8, D = the element item g0 + u multiplies
template <int G>
static __global__ void __launch_bounds__(128)
    k_pn_table(const Xyzz<typename FieldOf<G>::F> *__restrict__ x, size_t g0, size_t cnt, int log_n, int pass,
               Xyzz<typename FieldOf<G>::F> *__restrict__ xz) {
  typedef typename PmLane<G>::LF LF;
  const size_t tt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int comp = G == 2 ? (int)(tt & 1) : 0;
  const size_t u = G == 2 ? tt >> 1 : tt;
  if (u >= cnt) return;  // whole pairs only
  const int il = pn_items_log(log_n, pass);
  const size_t g = g0 + u, base = (g >> il) << log_n;
  const PnItem it = pn_item(log_n, pass, g & (((size_t)1 << il) - 1));
  Xyzz<LF> d, q;
  pm_ld_xyzz(d, &x[base + it.b], comp);
  pm_st_xyzz(&xz[u], d, comp);
  xyzz_dbl(q, d);
  pm_st_xyzz(&xz[cnt + u], q, comp);
#pragma unroll 1
  for (int m = 3; m <= PM_ROWS; ++m) {
    xyzz_add(q, d);  // (an infinite q restarts from D; q == D doubles)
    pm_st_xyzz(&xz[(size_t)(m - 1) * cnt + u], q, comp);
  }
}

// lane (pair) u < cnt: x[b] = [tw[e]] D from the rows of item g0 + u
template <int G>
static __global__ void __launch_bounds__(128, 2)
    k_pn_ladder(const Aff<typename FieldOf<G>::F> *__restrict__ rows, const uint8_t *__restrict__ tw,
                Xyzz<typename FieldOf<G>::F> *__restrict__ x, size_t g0, size_t cnt, int log_n, int pass) {
  typedef typename PmLane<G>::LF LF;
  const size_t tt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int comp = G == 2 ? (int)(tt & 1) : 0;
  const size_t u = G == 2 ? tt >> 1 : tt;
  if (u >= cnt) return;  // whole pairs only
  const int il = pn_items_log(log_n, pass);
  const size_t g = g0 + u, base = (g >> il) << log_n;
  const PnItem it = pn_item(log_n, pass, g & (((size_t)1 << il) - 1));
  Xyzz<LF> acc;
  pm_ladder_loop<G>(acc, rows + u, cnt, tw + it.e * 32, 255, comp);
  pm_st_xyzz(&x[base + it.b], acc, comp);
}

// lane (pair) i < cnt: y[i] = x at pn_out_map of its transform
template <int G>
static __global__ void __launch_bounds__(128)
    k_pn_store(const Xyzz<typename FieldOf<G>::F> *__restrict__ x, size_t cnt, int log_n, int flags,
               Xyzz<typename FieldOf<G>::F> *__restrict__ y) {
  typedef typename PmLane<G>::LF LF;
  const size_t tt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int comp = G == 2 ? (int)(tt & 1) : 0;
  const size_t i = G == 2 ? tt >> 1 : tt;
  if (i >= cnt) return;  // whole pairs only
  const size_t mask = ((size_t)1 << log_n) - 1;
  Xyzz<LF> q;
  pm_ld_xyzz(q, &x[(i & ~mask) + pn_out_map(log_n, flags, i & mask)], comp);
  pm_st_xyzz(&y[i], q, comp);
}

template <int G>
const uint8_t *PointsNtt<G>::twiddles(hipStream_t, int log_n) {
  DevBuf &b = tw_[log_n];
  if (!b.p) {
    const std::vector<hfr::Fr> t = pn_twiddle_table(log_n);
    std::vector<uint8_t> bytes(t.size() * 32);
    for (size_t i = 0; i < t.size(); ++i) hfr::to_scalar(&bytes[i * 32], t[i]);  // the plain integers pm_digit reads
    b.ensure(bytes.size());
    MSM_HIP_CHECK(hipMemcpy(b.p, bytes.data(), bytes.size(), hipMemcpyHostToDevice));
  }
  return b.as<uint8_t>();
}

template <int G>
void PointsNtt<G>::chunk(hipStream_t s, const void *d_src, void *d_dst, int log_n, size_t tc, int flags,
                         const uint8_t *tw, size_t slice) {
  typedef typename FieldOf<G>::F SF;
  static_assert(sizeof(Aff<SF>) == ROW && sizeof(Xyzz<SF>) == XYZZ && sizeof(SF) == ELEM, "stored sizes");
  const size_t cnt = tc << log_n;
  if (cnt * XYZZ > x_.bytes || cnt * XYZZ > xz_.bytes) throw std::runtime_error("points_ntt: working buffer too small");
  const unsigned B = 128;
  Xyzz<SF> *x = x_.as<Xyzz<SF>>(), *xz = xz_.as<Xyzz<SF>>();
  hipLaunchKernelGGL(k_pn_load<G>, dim3(nblk(cnt * G, B)), dim3(B), 0, s, static_cast<const uint64_t *>(d_src), cnt,
                     log_n, flags, x);
  MSM_HIP_CHECK(hipGetLastError());
  for (int p = 0; p < pn_passes(log_n, flags); ++p) {
    const size_t items = tc << pn_items_log(log_n, p);
    const bool level = !pn_is_scale(log_n, p), mult = pn_laddered(log_n, p);
    for (size_t g0 = 0; g0 < items; g0 += slice) {
      const size_t sc = std::min(slice, items - g0);
      const unsigned nb = nblk(sc * G, B);
      if (level) {
        hipLaunchKernelGGL(k_pn_bfly<G>, dim3(nb), dim3(B), 0, s, x, g0, sc, log_n, p);
        MSM_HIP_CHECK(hipGetLastError());
      }
      if (!mult) continue;
      if ((size_t)PM_ROWS * sc * XYZZ > xz_.bytes || (size_t)PM_ROWS * sc * ROW > rows_.bytes)
        throw std::runtime_error("points_ntt: table buffer too small");
      hipLaunchKernelGGL(k_pn_table<G>, dim3(nb), dim3(B), 0, s, (const Xyzz<SF> *)x, g0, sc, log_n, p, xz);
      MSM_HIP_CHECK(hipGetLastError());
      ta_tree<G>(s, lv_.p, lv_.bytes, TA_XYZZ_ROWS, xz, rows_.p, (size_t)PM_ROWS * sc);
      hipLaunchKernelGGL(k_pn_ladder<G>, dim3(nb), dim3(B), 0, s, (const Aff<SF> *)rows_.as<Aff<SF>>(), tw, x, g0, sc,
                         log_n, p);
      MSM_HIP_CHECK(hipGetLastError());
    }
  }
  hipLaunchKernelGGL(k_pn_store<G>, dim3(nblk(cnt * G, B)), dim3(B), 0, s, (const Xyzz<SF> *)x, cnt, log_n, flags, xz);
  MSM_HIP_CHECK(hipGetLastError());
  ta_tree<G>(s, lv_.p, lv_.bytes, TA_XYZZ_BLST, xz, d_dst, cnt);
}

template <int G>
void PointsNtt<G>::run(hipStream_t cs, const void *src, void *dst, int log_n, size_t batch, int flags, bool src_dev,
                       bool dst_dev) {
  if (!batch) return;
  if (log_n < 0 || log_n > PN_MAX_LOG) throw std::runtime_error("points_ntt: bad log_n");
  DeviceGuard g(dev_);
  const size_t slice = pn_slice();
  const size_t T = pn_chunk_transforms(log_n, batch, pn_chunk()), C = T << log_n;
  const size_t S = pn_slice_items(log_n, flags, T, slice);  // items of the largest table
  pipe_.begin(cs);  // the working, table and level buffers of the previous call
  const uint8_t *tw = twiddles(cs, log_n);
  x_.ensure(C * XYZZ);
  xz_.ensure(std::max((size_t)PM_ROWS * S, C) * XYZZ);
  if (S) rows_.ensure((size_t)PM_ROWS * S * ROW);
  lv_.ensure(std::max(ta_level_elems((size_t)PM_ROWS * S), ta_level_elems(C)) * ELEM);
  if (!src_dev) in_.ensure(C * AFF);
  if (!dst_dev) out_.ensure(C * AFF);
  auto pend = pipe_.pending([&](int slot, size_t off, size_t cnt) {
    memcpy(static_cast<uint8_t *>(dst) + off * AFF, out_.pin[slot], cnt * AFF);
  });
  size_t k = 0;
  for (size_t t0 = 0; t0 < batch; t0 += T, ++k) {
    const size_t tc = std::min(T, batch - t0), c0 = t0 << log_n, cnt = tc << log_n;
    const int slot = (int)(k & 1);
    const void *d_src;
    void *d_dst;
    if (!src_dev) {
      pipe_.upload(cs, slot, [&] { memcpy(in_.pin[slot], static_cast<const uint8_t *>(src) + c0 * AFF, cnt * AFF); },
                   {{in_, slot, cnt * AFF}});
      d_src = in_.dev[slot].p;
    } else {
      d_src = static_cast<const uint8_t *>(src) + c0 * AFF;
    }
    if (!dst_dev) {
      pipe_.out_open(cs, slot);
      d_dst = out_.dev[slot].p;
    } else {
      d_dst = static_cast<uint8_t *>(dst) + c0 * AFF;
    }
    chunk(cs, d_src, d_dst, log_n, tc, flags, tw, slice);
    pipe_.computed(cs, slot);
    if (!dst_dev) pipe_.download(cs, slot, pend, c0, cnt, {{out_, slot, cnt * AFF}});
  }
  pend.flush();
  pipe_.finish(cs);
}

template class PointsNtt<MSM_GROUP>;

}  // namespace msm
