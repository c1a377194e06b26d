// points_mult.hip -- bulk scalar multiplication out[i] = [k_i] P_i on one MI355X
// (replaces a loop over the reference's one-point blst_p{1,2}_mult: ref
// src/e1.c:505-533, src/e2.c, src/ec_mult.h).
//
// A fixed-window ladder over signed 4-bit digits, the same for every lane:
//   k_pm_table   point t -> its multiples 1P .. 8P: 1P as an affine row, 2P .. 8P
//                as xyzz points by a chain of xyzz_madd (which takes the doubling
//                branch for 2P and restarts from P after a multiple that is
//                infinity, so points of small order need no care)
//   (ta_tree)    the 7 xyzz multiples of every point -> affine rows, through the
//                batch-inversion tree of to_affine.hip (TA_XYZZ_ROWS)
//   k_pm_ladder  from the top window down: four doublings, then the row
//                |digit| of the lane's own point added or subtracted
//                (xyzz_madd).  Every lane runs the same windows and the same
//                doublings; a zero digit or an all-zero row (infinity) is
//                skipped under a predicate.  The rows are read from HBM by a
//                lane-varying index (a register array indexed that way would
//                be scratch), row m of point t at rows[(m - 1) np + t].
//   (ta_tree)    the ladder's xyzz results -> blst affine output (TA_XYZZ_BLST)
//
// Digits (Booth): window w looks at bits 4w - 1 .. 4w + 3 of the scalar (bit -1
// and bits >= nbits are zero), d = b[4w-1] + b[4w] + 2 b[4w+1] + 4 b[4w+2] - 8 b[4w+3]
// in [-8, 8]; sum d_w 16^w = k over nbits / 4 + 1 windows, no carry chain, so a
// lane reads two scalar bytes per window and the ladder can start at the top.
//
// The result is [k]P for every point of the curve, in the subgroup or not (the
// contract of blst_p{1,2}_unchecked_mult): no endomorphism is used.
//
// G1 runs one lane per point, G2 one lane PAIR per point (Fp2L, fp2l.hpp).  Both
// lanes of a pair hold the same digit and the same zero tests (f_is_zero_exact
// combines the pair), so every branch is taken by whole pairs and a DPP swap
// never reads a switched-off partner.
//
// Products per point as built at nbits = 255 (an fp_mul2 priced 1.5 Fp products,
// an fp_mul4 2.5; tools/points_mult_timing.py): 64 windows, 252 doublings of 8.5
// and 60 mixed additions of 9.5 (a digit is zero with probability 1/16) = 2712;
// table 2 + 12.5 + 6 x 9.5 = 71.5, its rows 7 x 8.6 = 60, the output 9.7:
// G1 2853; G2, both lanes, 7814.  One-point mode drops the table and the rows.
#include "points_mult.hpp"

#include <cstring>

#include "pair_kernels.hpp"
#include "pm_common.hpp"
#include "to_affine.hpp"

#ifndef MSM_GROUP
#error "define MSM_GROUP (1 or 2)"
#endif

namespace msm {

// (PmLane, pm_ld / pm_st, pm_digit and k_pm_table: pm_common.hpp, shared with
// point_segments.hip)

// lane (pair) t < n: out[t] = [k_t] P, P = point t (np == n) or point 0 (np == 1) of the rows
template <int G>
static __global__ void __launch_bounds__(128, 2)
    k_pm_ladder(const Aff<typename FieldOf<G>::F> *__restrict__ rows, size_t np, const uint8_t *__restrict__ sc,
                size_t stride, int nbits, Xyzz<typename FieldOf<G>::F> *__restrict__ out, size_t n) {
  typedef typename PmLane<G>::LF LF;
  const size_t tt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int comp = G == 2 ? (int)(tt & 1) : 0;
  const size_t t = G == 2 ? tt >> 1 : tt;
  if (t >= n) return;  // whole pairs only
  const uint8_t *k = sc + t * stride;
  const Aff<typename FieldOf<G>::F> *mine = rows + (np == 1 ? 0 : t);
  Xyzz<LF> acc;
  pm_ladder_loop<G>(acc, mine, np, k, nbits, comp);  // (pm_common.hpp)
  pm_st_xyzz(&out[t], acc, comp);
}

template <int G>
void PointsMult<G>::table(hipStream_t s, const void *d_points, size_t np) {
  typedef typename FieldOf<G>::F SF;
  static_assert(sizeof(Aff<SF>) == ROW && sizeof(Xyzz<SF>) == XYZZ && sizeof(SF) == ELEM, "stored sizes");
  const size_t nx = (size_t)(PM_ROWS - 1) * np;
  if (PM_ROWS * np * ROW > rows_.bytes || nx * XYZZ > xz_.bytes) throw std::runtime_error("points_mult: table buffer too small");
  const unsigned B = 128;
  hipLaunchKernelGGL(k_pm_table<G>, dim3(nblk(np * G, B)), dim3(B), 0, s, static_cast<const uint64_t *>(d_points), np,
                     rows_.as<Aff<SF>>(), xz_.as<Xyzz<SF>>());
  MSM_HIP_CHECK(hipGetLastError());
  ta_tree<G>(s, lv_.p, lv_.bytes, TA_XYZZ_ROWS, xz_.p, rows_.as<Aff<SF>>() + np, nx);
}

template <int G>
void PointsMult<G>::ladder(hipStream_t s, size_t np, const uint8_t *d_scalars, void *d_dst, size_t n, int nbits,
                           size_t stride) {
  typedef typename FieldOf<G>::F SF;
  if (n * XYZZ > xz_.bytes) throw std::runtime_error("points_mult: result buffer too small");
  const unsigned B = 128;
  hipLaunchKernelGGL(k_pm_ladder<G>, dim3(nblk(n * G, B)), dim3(B), 0, s, (const Aff<SF> *)rows_.as<Aff<SF>>(), np,
                     d_scalars, stride, nbits, xz_.as<Xyzz<SF>>(), n);
  MSM_HIP_CHECK(hipGetLastError());
  ta_tree<G>(s, lv_.p, lv_.bytes, TA_XYZZ_BLST, xz_.p, d_dst, n);
}

template <int G>
void PointsMult<G>::run(hipStream_t cs, const void *points, const uint8_t *scalars, void *dst, size_t n, int nbits,
                        size_t stride, bool one_point, bool src_dev, bool dst_dev) {
  if (!n) return;
  if (nbits < 1 || nbits > 256 || stride < (size_t)(nbits + 7) / 8) throw std::runtime_error("points_mult: bad nbits / stride");
  DeviceGuard g(dev_);
  const size_t nb = (size_t)(nbits + 7) / 8;
  const size_t C = std::min(n, pm_chunk());
  const size_t T = one_point ? 1 : C;                // points of a table
  const size_t PB = T * AFF;                         // their bytes in a staged slot; the scalars follow
  const size_t IN = PB + C * nb;                     // (staged scalars are packed: nb bytes apart)
  rows_.ensure(PM_ROWS * T * ROW);
  xz_.ensure(std::max((size_t)(PM_ROWS - 1) * T, C) * XYZZ);
  lv_.ensure(std::max(ta_level_elems((size_t)(PM_ROWS - 1) * T), ta_level_elems(C)) * ELEM);
  if (!src_dev) in_.ensure(IN);
  if (!dst_dev) out_.ensure(C * AFF);
  pipe_.begin(cs);  // the table and level buffers of the previous call
  auto pend = pipe_.pending([&](int slot, size_t off, size_t cnt) {
    memcpy(static_cast<uint8_t *>(dst) + off * AFF, out_.pin[slot], cnt * AFF);
  });
  size_t k = 0;
  for (size_t c0 = 0; c0 < n; c0 += C, ++k) {
    const size_t cnt = std::min(C, n - c0);
    const int slot = (int)(k & 1);
    const size_t np = one_point ? 1 : cnt;
    const uint8_t *d_pts, *d_sc;
    size_t d_stride = stride;
    void *d_dst;
    if (!src_dev) {
      pipe_.upload(cs, slot, [&] {
        uint8_t *w = static_cast<uint8_t *>(in_.pin[slot]);
        memcpy(w, static_cast<const uint8_t *>(points) + (one_point ? 0 : c0 * AFF), np * AFF);
        const uint8_t *sc = scalars + c0 * stride;
        if (stride == nb) memcpy(w + PB, sc, cnt * nb);
        else  // only the nb bytes of each scalar: nothing past the last one is read, and the slot stays small
          for (size_t i = 0; i < cnt; ++i) memcpy(w + PB + i * nb, sc + i * stride, nb);
      }, {{in_, slot, PB + cnt * nb}});
      d_stride = nb;
      d_pts = in_.dev[slot].as<uint8_t>();
      d_sc = d_pts + PB;
    } else {
      d_pts = static_cast<const uint8_t *>(points) + (one_point ? 0 : c0 * AFF);
      d_sc = scalars + c0 * stride;
    }
    if (!dst_dev) {
      pipe_.out_open(cs, slot);
      d_dst = out_.dev[slot].p;
    } else {
      d_dst = static_cast<uint8_t *>(dst) + c0 * AFF;
    }
    if (!one_point || k == 0) table(cs, d_pts, np);  // one point: its rows serve every chunk
    ladder(cs, np, d_sc, d_dst, cnt, nbits, d_stride);
    pipe_.computed(cs, slot);
    if (!dst_dev) pipe_.download(cs, slot, pend, c0, cnt, {{out_, slot, cnt * AFF}});
  }
  pend.flush();
  pipe_.finish(cs);
}

template class PointsMult<MSM_GROUP>;

}  // namespace msm
