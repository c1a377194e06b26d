// point_segments.hip -- segmented sums and MSMs on one MI355X:
// dst[j] = sum over offsets[j] <= i < offsets[j + 1] of [k_i] P_i for k point
// sets in one call (replaces a host loop over the reference's
// blst_p{1,2}s_mult_pippenger / blst_p{1,2}s_add, one call per set: ref
// src/multi_scalar.c:581-607, src/bulk_addition.c:145-164).
//
// The host cuts the points into pieces of at most L consecutive points of one
// segment (segments_plan.hpp); one lane (G2: one lane pair, fp2l.hpp) sums one
// piece:
//   k_pm_table   point t -> its multiples 1P .. 8P (pm_common.hpp, the kernel of
//   (ta_tree)    points_mult.hip) and their affine rows (TA_XYZZ_ROWS); plain
//                sums need neither
//   k_ps_straus  a Straus ladder over signed 4-bit digits (pm_digit), from the
//                top window down: four doublings of the accumulator, then for
//                each point of the piece the row |digit| of that point added or
//                subtracted (xyzz_madd).  The doublings are paid once per piece
//                and window, not once per point as in k_pm_ladder.  A zero digit
//                or an all-zero row (infinity) is skipped under a predicate.
//                G1: the row of the first point is asked for before the doublings
//                and the row of point i + 1 before the addition of point i.  G2
//                has no registers for a row in flight and keeps only the next
//                digit ahead.
//   k_ps_sum     plain sums (no scalars): one pass of xyzz_madd over the piece
//   k_ps_merge   the partials of one segment lie side by side; a strided
//                pairwise tree sums them: at step s = 1, 2, 4, .. the partial at
//                position r of its run, r a multiple of 2 s, takes in the one at
//                r + s.  ceil(log2(run)) dependent steps, run - 1 additions.
//   k_ps_gather  the sum of every segment that ends in this chunk (infinity for
//                an empty one), side by side
//   (ta_tree)    those xyzz sums -> blst affine output (TA_XYZZ_BLST)
//
// A chunk boundary may fall inside a segment: the sum of the open segment so
// far is carried into the next chunk as one more partial, in front of that
// chunk's pieces.  A segment is written once it is complete.
//
// The result is exact for every point of the curve, in the subgroup or not: the
// xyzz formulas of ec.hpp take their doubling and infinity branches where the
// operands ask for them, and no endomorphism is used.
//
// Lanes of a wave hold pieces of different lengths (the last piece of a segment
// is short), so the point loop diverges between lanes; the loop bounds, the
// digit and every zero test are the same in both lanes of a G2 pair
// (f_is_zero_exact combines the pair), so a DPP swap never reads a switched-off
// partner.
#include "point_segments.hpp"

#include <cstring>

#include "pair_kernels.hpp"
#include "pm_common.hpp"
#include "to_affine.hpp"

#ifndef MSM_GROUP
#error "define MSM_GROUP (1 or 2)"
#endif

namespace msm {

// the row |d| of the point whose 1P row is at `mine` (all zero for d == 0)
template <class LF, class SF>
__device__ __forceinline__ void ps_row(Aff<LF> &row, const Aff<SF> *mine, size_t np, int d, int comp) {
  const uint32_t m = (uint32_t)(d < 0 ? -d : d);
  f_zero(row.x);
  f_zero(row.y);
  if (m) {
    const Aff<SF> *r = mine + (size_t)(m - 1) * np;
    pm_ld(row.x, &r->x, comp);
    pm_ld(row.y, &r->y, comp);
  }
}

// lane (pair) t < npieces: out[t] = sum over the points of piece t of [k_i] P_i;
// row m of chunk point i at rows[(m - 1) np + i], its scalar at sc + i stride
template <int G>
static __global__ void __launch_bounds__(128, 2)
    k_ps_straus(const Aff<typename FieldOf<G>::F> *__restrict__ rows, size_t np, const uint8_t *__restrict__ sc,
                size_t stride, int nbits, const SegMeta *__restrict__ meta,
                Xyzz<typename FieldOf<G>::F> *__restrict__ out, size_t npieces) {
  typedef typename PmLane<G>::LF LF;
  const size_t tt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int comp = G == 2 ? (int)(tt & 1) : 0;
  const size_t t = G == 2 ? tt >> 1 : tt;
  if (t >= npieces) return;  // whole pairs only
  const uint32_t s0 = meta[t].start, cnt = meta[t].count;  // the same in both lanes of a pair
  const uint8_t *k = sc + (size_t)s0 * stride;
  const Aff<typename FieldOf<G>::F> *mine = rows + s0;
  const int nw = nbits / 4 + 1;
  Xyzz<LF> acc;
  xyzz_set_inf(acc);
#pragma unroll 1
  for (int w = nw - 1; w >= 0; --w) {
    // G1: the first row is asked for before the doublings, which hide its latency,
    // and the row of point i + 1 before the addition of point i.  G2: a row that
    // stays live across the doublings, or a second row in flight, does not fit at
    // two waves per SIMD (4 and 6 VGPRs spilled to scratch), so every row is
    // loaded where it is used.
    // A row's address waits for its digit, a load of its own: the digit is read
    // one step ahead of the row (dn), so the two latencies do not add up.
    int d = 0, dn = pm_digit(k, w, nbits);
    Aff<LF> row;
    if constexpr (G == 1) {
      d = dn;
      ps_row(row, mine, np, d, comp);
      if (cnt > 1) dn = pm_digit(k + stride, w, nbits);
    }
    if (w != nw - 1) {
#pragma unroll 1
      for (int j = 0; j < 4; ++j) {
        Xyzz<LF> tmp = acc;
        xyzz_dbl(acc, tmp);
      }
    }
#pragma unroll 1
    for (uint32_t i = 0; i < cnt; ++i) {
      if constexpr (G == 1) {
        const Aff<LF> cur = row;
        const bool neg = d < 0;
        if (i + 1 < cnt) {
          d = dn;
          ps_row(row, mine + i + 1, np, d, comp);
          if (i + 2 < cnt) dn = pm_digit(k + (size_t)(i + 2) * stride, w, nbits);
        }
        const bool zx = f_is_zero_exact(cur.x), zy = f_is_zero_exact(cur.y);
        if (!(zx & zy)) xyzz_madd(acc, cur, neg);  // (a zero digit left the row zero)
      } else {
        d = dn;
        ps_row(row, mine + i, np, d, comp);
        if (i + 1 < cnt) dn = pm_digit(k + (size_t)(i + 1) * stride, w, nbits);
        const bool zx = f_is_zero_exact(row.x), zy = f_is_zero_exact(row.y);
        if (!(zx & zy)) xyzz_madd(acc, row, d < 0);
      }
    }
  }
  pm_st_xyzz(&out[t], acc, comp);
}

// lane (pair) t < npieces: out[t] = the sum of the points of piece t (blst affine points at pts)
template <int G>
static __global__ void __launch_bounds__(128, 2)
    k_ps_sum(const uint64_t *__restrict__ pts, const SegMeta *__restrict__ meta,
             Xyzz<typename FieldOf<G>::F> *__restrict__ out, size_t npieces) {
  typedef typename PmLane<G>::LF LF;
  const size_t tt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int comp = G == 2 ? (int)(tt & 1) : 0;
  const size_t t = G == 2 ? tt >> 1 : tt;
  if (t >= npieces) return;  // whole pairs only
  const uint32_t cnt = meta[t].count;  // the same in both lanes of a pair
  const uint64_t *src = pts + (size_t)meta[t].start * 12 * G;
  Xyzz<LF> acc;
  xyzz_set_inf(acc);
#pragma unroll 1
  for (uint32_t i = 0; i < cnt; ++i, src += 12 * G) {
    Aff<LF> p;
    fp_from_blst(pm_c(p.x), src + 6 * comp);
    fp_from_blst(pm_c(p.y), src + 6 * G + 6 * comp);
    const bool zx = f_is_zero_exact(p.x), zy = f_is_zero_exact(p.y);
    if (!(zx & zy)) xyzz_madd(acc, p, false);
  }
  pm_st_xyzz(&out[t], acc, comp);
}

// lane (pair) t < np: one step of the pairwise tree over the run of partial t
template <int G>
static __global__ void __launch_bounds__(128, 2)
    k_ps_merge(Xyzz<typename FieldOf<G>::F> *__restrict__ part, const SegMeta *__restrict__ meta, size_t np,
               uint32_t step) {
  typedef typename PmLane<G>::LF LF;
  const size_t tt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int comp = G == 2 ? (int)(tt & 1) : 0;
  const size_t t = G == 2 ? tt >> 1 : tt;
  if (t >= np) return;  // whole pairs only
  const uint32_t rel = meta[t].rel, len = meta[t].len;  // the same in both lanes of a pair
  if ((rel & (2 * step - 1)) != 0 || rel + step >= len) return;
  Xyzz<LF> a, b;
  pm_ld_xyzz(a, &part[t], comp);
  pm_ld_xyzz(b, &part[t + step], comp);
  xyzz_add(a, b);
  pm_st_xyzz(&part[t], a, comp);
}

// lane (pair) t < nseg: res[t] = part[src[t]], or infinity where src[t] is ~0
template <int G>
static __global__ void __launch_bounds__(128)
    k_ps_gather(const Xyzz<typename FieldOf<G>::F> *__restrict__ part, const uint32_t *__restrict__ src,
                Xyzz<typename FieldOf<G>::F> *__restrict__ res, size_t nseg) {
  typedef typename PmLane<G>::LF LF;
  const size_t tt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int comp = G == 2 ? (int)(tt & 1) : 0;
  const size_t t = G == 2 ? tt >> 1 : tt;
  if (t >= nseg) return;
  const uint32_t s = src[t];
  Xyzz<LF> a;
  if (s == ~0u) xyzz_set_inf(a);
  else pm_ld_xyzz(a, &part[s], comp);
  pm_st_xyzz(&res[t], a, comp);
}

template <int G>
void PointSegments<G>::run(hipStream_t cs, const void *points, const uint8_t *scalars, const size_t *o, size_t k,
                           void *dst, int nbits, size_t stride, bool src_dev, bool dst_dev) {
  typedef typename FieldOf<G>::F SF;
  static_assert(sizeof(Aff<SF>) == ROW && sizeof(Xyzz<SF>) == XYZZ && sizeof(SF) == ELEM, "stored sizes");
  static_assert(sizeof(SegMeta) == 16, "plan entry");
  if (!k) return;
  const bool msm = scalars != nullptr;
  if (msm && (nbits < 1 || nbits > 256 || stride < (size_t)(nbits + 7) / 8))
    throw std::runtime_error("point_segments: bad nbits / stride");
  DeviceGuard g(dev_);
  const size_t nb = msm ? (size_t)(nbits + 7) / 8 : 0;
  const size_t total = o[k] - o[0];
  const SegSizes z = seg_sizes(total, k, seg_chunk(G));
  const size_t C = z.C, CP = z.CP, pmax = z.pmax;
  const size_t L = seg_piece_len(CP, G);
  const size_t PB = CP * AFF;      // the points in a staged slot; the scalars follow
  const size_t IN = PB + CP * nb;  // (staged scalars are packed: nb bytes apart)
  if (msm) rows_.ensure(PM_ROWS * CP * ROW);
  xz_.ensure(std::max(msm ? (size_t)(PM_ROWS - 1) * CP : 0, pmax) * XYZZ);
  res_.ensure(C * XYZZ);
  lv_.ensure(std::max(msm ? ta_level_elems((size_t)(PM_ROWS - 1) * CP) : 0, ta_level_elems(C)) * ELEM);
  carry_.ensure(XYZZ);
  plan_lane_.ensure(z);
  if (!src_dev && total) in_.ensure(IN);
  if (!dst_dev) out_.ensure(C * AFF);
  pipe_.begin(cs);  // the table, partial and level buffers of the previous call
  auto pend = pipe_.pending([&](int slot, size_t off, size_t cnt) {  // (a chunk may write no segment: cnt 0)
    if (cnt) memcpy(static_cast<uint8_t *>(dst) + off * AFF, out_.pin[slot], cnt * AFF);
  });
  const unsigned B = 128;
  Xyzz<SF> *part = xz_.as<Xyzz<SF>>();
  plan_.begin(o, k, z, L, "point_segments");
  for (size_t ck = 0; plan_.next(); ++ck) {
    // this chunk: points [i, i + cnt), segments [j, j + nseg) end in it; np partials, the carried one (pc) first
    const size_t i = plan_.i, cnt = plan_.cnt(), j = plan_.j, nseg = plan_.nseg();
    const size_t np = plan_.np(), npieces = plan_.npieces(), pc = plan_.pc;
    const int slot = (int)(ck & 1);
    // ---- the plan and the sources go up ----
    plan_lane_.send(cs, slot, plan_);
    const SegMeta *d_meta = plan_lane_.d_meta();
    const uint32_t *d_src = plan_lane_.d_src();
    const uint8_t *d_pts = nullptr, *d_sc = nullptr;
    size_t d_stride = stride;
    if (cnt) {
      if (!src_dev) {
        pipe_.upload(cs, slot, [&] {
          uint8_t *w = static_cast<uint8_t *>(in_.pin[slot]);
          memcpy(w, static_cast<const uint8_t *>(points) + i * AFF, cnt * AFF);
          if (msm) {
            const uint8_t *sc = scalars + i * stride;
            if (stride == nb) memcpy(w + PB, sc, cnt * nb);
            else  // only the nb bytes of each scalar: nothing past the last one is read, and the slot stays small
              for (size_t q = 0; q < cnt; ++q) memcpy(w + PB + q * nb, sc + q * stride, nb);
          }
        }, {{in_, slot, PB + cnt * nb}});
        if (msm) d_stride = nb;
        d_pts = in_.dev[slot].as<uint8_t>();
        d_sc = d_pts + PB;
      } else {
        d_pts = static_cast<const uint8_t *>(points) + i * AFF;
        d_sc = msm ? scalars + i * stride : nullptr;
      }
    }
    void *d_dst = nullptr;
    if (!dst_dev) {
      pipe_.out_open(cs, slot);
      d_dst = out_.dev[slot].p;
    } else {
      d_dst = static_cast<uint8_t *>(dst) + j * AFF;
    }
    // ---- the kernels ----
    if (npieces) {
      if (msm) {
        hipLaunchKernelGGL(k_pm_table<G>, dim3(nblk(cnt * G, B)), dim3(B), 0, cs, reinterpret_cast<const uint64_t *>(d_pts),
                           cnt, rows_.as<Aff<SF>>(), part);
        MSM_HIP_CHECK(hipGetLastError());
        ta_tree<G>(cs, lv_.p, lv_.bytes, TA_XYZZ_ROWS, xz_.p, rows_.as<Aff<SF>>() + cnt, (size_t)(PM_ROWS - 1) * cnt);
      }
      // (the partials overwrite the xyzz multiples, which the rows no longer need)
      if (pc) MSM_HIP_CHECK(hipMemcpyAsync(part, carry_.p, XYZZ, hipMemcpyDeviceToDevice, cs));
      if (msm)
        hipLaunchKernelGGL(k_ps_straus<G>, dim3(nblk(npieces * G, B)), dim3(B), 0, cs,
                           (const Aff<SF> *)rows_.as<Aff<SF>>(), cnt, d_sc, d_stride, nbits, d_meta + pc, part + pc,
                           npieces);
      else
        hipLaunchKernelGGL(k_ps_sum<G>, dim3(nblk(npieces * G, B)), dim3(B), 0, cs,
                           reinterpret_cast<const uint64_t *>(d_pts), d_meta + pc, part + pc, npieces);
      MSM_HIP_CHECK(hipGetLastError());
      for (size_t step = 1; step < plan_.maxrun; step *= 2) {
        hipLaunchKernelGGL(k_ps_merge<G>, dim3(nblk(np * G, B)), dim3(B), 0, cs, part, d_meta, np, (uint32_t)step);
        MSM_HIP_CHECK(hipGetLastError());
      }
    }
    if (nseg) {
      hipLaunchKernelGGL(k_ps_gather<G>, dim3(nblk(nseg * G, B)), dim3(B), 0, cs, (const Xyzz<SF> *)part, d_src,
                         res_.as<Xyzz<SF>>(), nseg);
      MSM_HIP_CHECK(hipGetLastError());
      ta_tree<G>(cs, lv_.p, lv_.bytes, TA_XYZZ_BLST, res_.p, d_dst, nseg);
    }
    // a segment stays open: what this chunk summed of it goes into the next one
    if (plan_.carry()) MSM_HIP_CHECK(hipMemcpyAsync(carry_.p, part + plan_.open_src, XYZZ, hipMemcpyDeviceToDevice, cs));
    pipe_.computed(cs, slot);
    if (!dst_dev) pipe_.download(cs, slot, pend, j, nseg, {{out_, slot, nseg * AFF}});
  }
  pend.flush();  // (nothing is held where no chunk ran)
  pipe_.finish(cs);
}

template class PointSegments<MSM_GROUP>;

}  // namespace msm
