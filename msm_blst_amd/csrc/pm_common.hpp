// pm_common.hpp -- device code shared by the per-point ladder (points_mult.hip)
// and the segmented Straus sums (point_segments.hip): the lane type of a group,
// loads and stores of stored field elements, the signed 4-bit digit rule and the
// kernel that builds the multiples 1P .. 8P of every point.  Included by .hip
// files only.
#pragma once
#include "pair_kernels.hpp"
#include "points_mult.hpp"

namespace msm {

template <int G>
struct PmLane;
template <>
struct PmLane<1> {
  typedef Fp LF;
};
template <>
struct PmLane<2> {
  typedef Fp2L LF;
};

// stored elements (internal limbs, 56 B per component, 8-B aligned)
__device__ __forceinline__ void pm_ld(Fp &r, const Fp *p, int) {
  const uint2 *s = reinterpret_cast<const uint2 *>(p);
#pragma unroll
  for (int i = 0; i < NL / 2; ++i) {
    const uint2 v = s[i];
    r.v[2 * i] = v.x;
    r.v[2 * i + 1] = v.y;
  }
}
__device__ __forceinline__ void pm_ld(Fp2L &r, const Fp2 *p, int comp) { ld_comp(r.c, p, comp); }
__device__ __forceinline__ void pm_st(Fp *p, const Fp &a, int) {
  uint2 *d = reinterpret_cast<uint2 *>(p);
#pragma unroll
  for (int i = 0; i < NL / 2; ++i) d[i] = make_uint2(a.v[2 * i], a.v[2 * i + 1]);
}
__device__ __forceinline__ void pm_st(Fp2 *p, const Fp2L &a, int comp) { st_comp(p, a.c, comp); }
template <class LF, class SF>
__device__ __forceinline__ void pm_st_xyzz(Xyzz<SF> *p, const Xyzz<LF> &a, int comp) {
  pm_st(&p->x, a.x, comp);
  pm_st(&p->y, a.y, comp);
  pm_st(&p->zzz, a.zzz, comp);
  pm_st(&p->zz, a.zz, comp);
}
template <class LF, class SF>
__device__ __forceinline__ void pm_ld_xyzz(Xyzz<LF> &a, const Xyzz<SF> *p, int comp) {
  pm_ld(a.x, &p->x, comp);
  pm_ld(a.y, &p->y, comp);
  pm_ld(a.zzz, &p->zzz, comp);
  pm_ld(a.zz, &p->zz, comp);
}
__device__ __forceinline__ Fp &pm_c(Fp &a) { return a; }
__device__ __forceinline__ Fp &pm_c(Fp2L &a) { return a.c; }

// the signed digit of window w (see the head of points_mult.hip); k: the lane's
// scalar, only bytes below (nbits + 7) / 8 are read.  w is uniform.
__device__ __forceinline__ int pm_digit(const uint8_t *k, int w, int nbits) {
  const int lo = 4 * w - 1;  // the lowest of the five bits
  const int nb = (nbits + 7) >> 3;
  uint32_t v = 0;
  if (w == 0) {
    if (nb > 0) v = (uint32_t)k[0] << 1;
  } else {
    const int q = lo >> 3;
    if (q < nb) v = k[q];
    if (q + 1 < nb) v |= (uint32_t)k[q + 1] << 8;
    v >>= (lo & 7);
  }
  v &= 31u;
  const int valid = nbits - lo;  // bits of the five below nbits
  if (valid < 5) v &= valid > 0 ? (1u << valid) - 1u : 0u;
  return (int)(v & 1u) + (int)((v >> 1) & 7u) - 8 * (int)(v >> 4);
}

// The window loop of a ladder (the head of points_mult.hip), shared by k_pm_ladder
// and the NTT over points (points_ntt.hip): acc = [k] P for the lane (pair) whose
// rows are mine[(m - 1) np], m = 1 .. 8, and whose scalar is k.  Every lane of a
// wave runs the same windows and doublings; a zero digit or an all-zero row is
// skipped under a predicate taken by whole pairs.
template <int G>
__device__ __forceinline__ void pm_ladder_loop(Xyzz<typename PmLane<G>::LF> &acc,
                                               const Aff<typename FieldOf<G>::F> *__restrict__ mine, size_t np,
                                               const uint8_t *__restrict__ k, int nbits, int comp) {
  typedef typename PmLane<G>::LF LF;
  const int nw = nbits / 4 + 1;
  xyzz_set_inf(acc);
#pragma unroll 1
  for (int w = nw - 1; w >= 0; --w) {
    const int d = pm_digit(k, w, nbits);
    const uint32_t m = (uint32_t)(d < 0 ? -d : d);
    // the row is asked for before the doublings, which hide its latency
    Aff<LF> row;
    f_zero(row.x);
    f_zero(row.y);
    if (m) {
      const Aff<typename FieldOf<G>::F> *r = mine + (size_t)(m - 1) * np;
      pm_ld(row.x, &r->x, comp);
      pm_ld(row.y, &r->y, comp);
    }
    if (w != nw - 1) {
#pragma unroll 1
      for (int j = 0; j < 4; ++j) {
        Xyzz<LF> tmp = acc;
        xyzz_dbl(acc, tmp);
      }
    }
    const bool zx = f_is_zero_exact(row.x), zy = f_is_zero_exact(row.y);
    if (!(zx & zy)) xyzz_madd(acc, row, d < 0);  // (a zero digit left the row zero)
  }
}

// lane (pair) t < n: rows[t] = P_t (canonical internal limbs; infinity all zero),
// xz[(m - 2) n + t] = [m] P_t for m = 2 .. 8
template <int G>
static __global__ void __launch_bounds__(128)
    k_pm_table(const uint64_t *__restrict__ pts, size_t n, Aff<typename FieldOf<G>::F> *__restrict__ rows,
               Xyzz<typename FieldOf<G>::F> *__restrict__ xz) {
  typedef typename PmLane<G>::LF LF;
  const size_t tt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int comp = G == 2 ? (int)(tt & 1) : 0;
  const size_t t = G == 2 ? tt >> 1 : tt;
  if (t >= n) return;  // whole pairs only
  const uint64_t *src = pts + t * 12 * G;
  Aff<LF> p;
  fp_from_blst(pm_c(p.x), src + 6 * comp);
  fp_from_blst(pm_c(p.y), src + 6 * G + 6 * comp);
  const bool zx = f_is_zero_exact(p.x), zy = f_is_zero_exact(p.y);
  const bool inf = zx & zy;  // uniform over a pair
  pm_st(&rows[t].x, p.x, comp);
  pm_st(&rows[t].y, p.y, comp);
  Xyzz<LF> q;
  if (inf) xyzz_set_inf(q);
  else xyzz_from_aff(q, p, false);
#pragma unroll 1
  for (int m = 2; m <= PM_ROWS; ++m) {
    if (!inf) xyzz_madd(q, p, false);
    pm_st_xyzz(&xz[(size_t)(m - 2) * n + t], q, comp);
  }
}

}  // namespace msm
