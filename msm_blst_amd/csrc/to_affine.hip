// to_affine.hip -- bulk Jacobian -> affine normalisation on one MI355X
// (replaces ref src/multi_scalar.c:17-62, blst_p{1,2}s_to_affine; declared at
// ref bindings/blst.h:222-223, :362; used by bindings/blst.hpp:389,406,438).
//
// The reference shares one inversion over a stride of 1536 / 768 points with a
// serial prefix-product walk.  Here the whole chunk shares the inversions of
// its top level (at most TA_LEAF), through a tree of products (to_affine.hpp:
// TA_K = 8 elements per group):
//   k_ta_up    lane t: level[l+1][t] = prod of level[l][8t .. 8t+7]
//   k_ta_leaf  one Fermat inversion per element of the top level
//   k_ta_down  lane t: from 1 / level[l+1][t] and its group's 8 elements, every
//              element's inverse (prefix products recomputed into registers,
//              then back-substitution), written in place over level[l]
// Level 0 is the Z coordinates, read straight from the blst Jacobians, and the
// level-0 k_ta_down writes the blst affine output.  The same tree normalises
// xyzz points in internal form (ta_tree with TA_XYZZ_BLST / TA_XYZZ_ROWS, used by
// points_mult.hip): level 0 is then ZZZ, and from 1 / ZZZ the level-0 k_ta_down
// forms 1 / Z = ZZ / ZZZ, 1 / ZZ = (1 / Z)^2, x = X / ZZ, y = Y / ZZZ (4 products).
// The bulk encoder (encode.hip) runs the tree with TA_JAC_ENC_C / TA_JAC_ENC_S:
// the level-0 k_ta_down then hands x and y to the encoder's tail (encode_dev.hpp)
// and writes ZCash entries, with no affine array in between.
//
// No layout conversion per coordinate: the stored limbs of a blst coordinate
// (v 2^384 mod p) are used AS the internal value (internal Montgomery R =
// 2^392, so they stand for v 2^-8).  The tree then yields (Z 2^-8)^-1; one
// product with 2^-8 (FROMINT28) gives zi = 1/Z in internal form, and
// fp_mul(X limbs, zi^2) = X zi^2 2^384 is already the blst form of x.
// Products per point: 1 (up) + 1 (prefix) + 2 (back-substitution) + 1 (2^-8)
// + 4 (zi^2, zi^3, x, y) = 9 at level 0, plus 4 / 7 for the levels above
// (4 per element, n / 7 elements) and 570 / 8^levels for the leaves: ~9.7.
//
// A zero Z (infinity, whatever X and Y hold) enters the products as one and
// its output is the all-zero point; no other output is affected.  (The
// reference multiplies the zero into the shared product and corrupts the
// whole stride, ref multi_scalar.c:14-16.)
//
// G2 runs on lane pairs (Fp2L, fp2l.hpp; as k_ches_table2p / k_wbits_table2p):
// the seven prefix products alone are 7 x 28 = 196 registers for a one-lane
// Fp2, before the operands and temporaries of an Fp2 product (the one-lane
// k_wbits_table<2> spilled with far less live state); a lane of a pair holds
// one component, the register use of the G1 kernel.
#include "to_affine.hpp"

#include <cstring>
#include <type_traits>

#include "encode_dev.hpp"
#include "pair_kernels.hpp"

#ifndef MSM_GROUP
#error "define MSM_GROUP (1 or 2)"
#endif

namespace msm {

template <int G>
struct TaLane;
template <>
struct TaLane<1> {
  typedef Fp LF;
};
template <>
struct TaLane<2> {
  typedef Fp2L LF;
};

// level elements (internal limbs, 56 B per component, 8-B aligned)
__device__ __forceinline__ void ta_ld(Fp &r, const Fp *p, int) {
  const uint2 *s = reinterpret_cast<const uint2 *>(p);
#pragma unroll
  for (int i = 0; i < NL / 2; ++i) {
    const uint2 v = s[i];
    r.v[2 * i] = v.x;
    r.v[2 * i + 1] = v.y;
  }
}
__device__ __forceinline__ void ta_ld(Fp2L &r, const Fp2 *p, int comp) { ld_comp(r.c, p, comp); }
__device__ __forceinline__ void ta_st(Fp *p, const Fp &a, int) {
  uint2 *d = reinterpret_cast<uint2 *>(p);
#pragma unroll
  for (int i = 0; i < NL / 2; ++i) d[i] = make_uint2(a.v[2 * i], a.v[2 * i + 1]);
}
__device__ __forceinline__ void ta_st(Fp2 *p, const Fp2L &a, int comp) { st_comp(p, a.c, comp); }
// one blst coordinate (6 G limbs of 64 bits), limbs taken as they are
__device__ __forceinline__ void ta_ld_raw(Fp &r, const uint64_t *l, int) { unpack384(r, l); }
__device__ __forceinline__ void ta_ld_raw(Fp2L &r, const uint64_t *l, int comp) { unpack384(r.c, l + 6 * comp); }
__device__ __forceinline__ void ta_st_raw(uint64_t *l, const Fp &a, int) { pack384(l, a); }
__device__ __forceinline__ void ta_st_raw(uint64_t *l, const Fp2L &a, int comp) { pack384(l + 6 * comp, a.c); }
// a 2^-8 (the internal form of 2^-8 is 2^384 mod p = FROMINT28)
__device__ __forceinline__ void ta_mulk(Fp &r, const Fp &a) {
  Fp k;
  fp_set(k, FROMINT28);
  fp_mul(r, a, k);
}
__device__ __forceinline__ void ta_mulk(Fp2L &r, const Fp2L &a) { ta_mulk(r.c, a.c); }
__device__ __forceinline__ void ta_sel(Fp &r, bool c, const Fp &a) {  // r = c ? a : r
#pragma unroll
  for (int i = 0; i < NL; ++i) r.v[i] = c ? a.v[i] : r.v[i];
}
__device__ __forceinline__ void ta_sel(Fp2L &r, bool c, const Fp2L &a) { ta_sel(r.c, c, a.c); }
__device__ __forceinline__ const Fp &ta_c(const Fp &a) { return a; }
__device__ __forceinline__ const Fp &ta_c(const Fp2L &a) { return a.c; }

template <int J, int N, class Fn>
__device__ __forceinline__ void ta_static_for(Fn &&f) {
  if constexpr (J < N) {
    f(std::integral_constant<int, J>{});
    ta_static_for<J + 1, N>(f);
  }
}

// the kinds whose level 0 is the Z of blst Jacobians
constexpr bool ta_is_jac(int src) { return src == TA_JAC || src == TA_JAC_ENC_C || src == TA_JAC_ENC_S; }

// element j of a level: a Jacobian kind the Z of Jacobian j, an xyzz source the
// ZZZ of xyzz point j (zero -> one, `zero` set; uniform over a lane pair), else
// level element j
template <int G, int SRC>
__device__ __forceinline__ void ta_elem(typename TaLane<G>::LF &r, const void *lvl, size_t j, int comp, bool &zero) {
  typedef typename TaLane<G>::LF LF;
  if (SRC != TA_LEVEL) {
    if (ta_is_jac(SRC)) ta_ld_raw(r, static_cast<const uint64_t *>(lvl) + j * 18 * G + 12 * G, comp);
    else ta_ld(r, &(static_cast<const Xyzz<typename FieldOf<G>::F> *>(lvl) + j)->zzz, comp);
    zero = f_is_zero_exact(r);
    LF one;
    f_one(one);
    ta_sel(r, zero, one);
  } else {
    ta_ld(r, static_cast<const typename FieldOf<G>::F *>(lvl) + j, comp);
    zero = false;
  }
}

// lane (pair) t < n_dst: dst[t] = prod src[8t .. min(8t + 8, n_src))
template <int G, int SRC>
static __global__ void __launch_bounds__(128)
    k_ta_up(const void *__restrict__ src, size_t n_src, typename FieldOf<G>::F *__restrict__ dst, size_t n_dst) {
  typedef typename TaLane<G>::LF LF;
  const size_t tt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int comp = G == 2 ? (int)(tt & 1) : 0;
  const size_t t = G == 2 ? tt >> 1 : tt;
  if (t >= n_dst) return;  // whole pairs only
  const size_t j0 = t * TA_K;
  const size_t cnt = min((size_t)TA_K, n_src - j0);
  bool z;
  LF acc;
  ta_elem<G, SRC>(acc, src, j0, comp, z);
  for (size_t j = 1; j < cnt; ++j) {
    LF e;
    ta_elem<G, SRC>(e, src, j0 + j, comp, z);
    f_mul_bs(acc, acc, e);
  }
  ta_st(dst + t, acc, comp);
}

// top level, in place: top[t] = 1 / top[t]
template <int G>
static __global__ void __launch_bounds__(64) k_ta_leaf(typename FieldOf<G>::F *top, size_t m) {
  typedef typename TaLane<G>::LF LF;
  const size_t tt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int comp = G == 2 ? (int)(tt & 1) : 0;
  const size_t t = G == 2 ? tt >> 1 : tt;
  if (t >= m) return;
  LF a, r;
  ta_ld(a, top + t, comp);
  f_inv(r, a);
  ta_st(top + t, r, comp);
}

// lane (pair) t < n_up: inv_up[t] = 1 / prod lvl[8t ..]; every element of the
// group is replaced by its inverse (a point source: the affine point of point j
// is written to out instead, lvl = the points, read only; TA_XYZZ_ROWS writes
// canonical internal limbs, Aff<F>, the others blst limbs)
template <int G, int SRC>
static __global__ void __launch_bounds__(128)
    k_ta_down(const typename FieldOf<G>::F *__restrict__ inv_up, size_t n_up, void *lvl, size_t n_lvl,
              void *out) {
  typedef typename TaLane<G>::LF LF;
  typedef typename FieldOf<G>::F SF;
  const size_t tt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int comp = G == 2 ? (int)(tt & 1) : 0;
  const size_t t = G == 2 ? tt >> 1 : tt;
  if (t >= n_up) return;
  const size_t j0 = t * TA_K;
  const int cnt = (int)min((size_t)TA_K, n_lvl - j0);
  LF I;
  ta_ld(I, inv_up + t, comp);
  bool z;
  LF pre[TA_K - 1];  // pre[j] = e_0 .. e_j
  ta_elem<G, SRC>(pre[0], lvl, j0, comp, z);
  // (compile-time steps: a `#pragma unroll` loop guarded by j < cnt is turned
  // into a loop of cnt trips, not unrolled, and pre[] lands in scratch)
  ta_static_for<1, (int)TA_K - 1>([&](auto jc) __attribute__((always_inline)) {
    constexpr int j = decltype(jc)::value;
    if (j < cnt) {
      LF e;
      ta_elem<G, SRC>(e, lvl, j0 + j, comp, z);
      f_mul_bs(pre[j], pre[j - 1], e);
    }
  });
  ta_static_for<0, (int)TA_K>([&](auto jc) __attribute__((always_inline)) {
    constexpr int j = (int)TA_K - 1 - decltype(jc)::value;
    if (j < cnt) {
      LF e, ij;
      ta_elem<G, SRC>(e, lvl, j0 + j, comp, z);
      if constexpr (j > 0) {
        f_mul_bs(ij, I, pre[j - 1]);  // 1 / e_j = (1 / (e_0 .. e_j)) (e_0 .. e_{j-1})
        f_mul_bs(I, I, e);
      } else {
        ij = I;
      }
      if constexpr (SRC == TA_JAC) {
        const uint64_t *P = static_cast<const uint64_t *>(lvl) + (j0 + j) * 18 * G;
        uint64_t *o = static_cast<uint64_t *>(out) + (j0 + j) * 12 * G;
        LF zi, zi2, zi3, X, Y, zero;
        ta_mulk(zi, ij);
        f_sqr(zi2, zi);
        f_mul_bs(zi3, zi2, zi);
        ta_ld_raw(X, P, comp);
        ta_ld_raw(Y, P + 6 * G, comp);
        f_mul_bs(X, X, zi2);
        f_mul_bs(Y, Y, zi3);
        f_csub(X);
        f_csub(Y);
        f_zero(zero);
        ta_sel(X, z, zero);
        ta_sel(Y, z, zero);
        ta_st_raw(o, X, comp);
        ta_st_raw(o + 6 * G, Y, comp);
      } else if constexpr (ta_is_jac(SRC)) {  // the encoded kinds: the same x, y, then the encoder's tail
        constexpr bool SER = SRC == TA_JAC_ENC_S;
        const uint64_t *P = static_cast<const uint64_t *>(lvl) + (j0 + j) * 18 * G;
        LF zi, zi2, zi3, X, Y;
        ta_mulk(zi, ij);
        f_sqr(zi2, zi);
        f_mul_bs(zi3, zi2, zi);
        ta_ld_raw(X, P, comp);
        ta_ld_raw(Y, P + 6 * G, comp);
        f_mul_bs(X, X, zi2);
        f_mul_bs(Y, Y, zi3);
        f_csub(X);  // the canonical blst limbs the reference's own normalisation hands its encoder
        f_csub(Y);
        enc_entry<G, SER>(static_cast<uint8_t *>(out) + (j0 + j) * (SER ? 96 : 48) * G, ta_c(X), ta_c(Y), z, comp);
      } else if constexpr (SRC != TA_LEVEL) {
        const Xyzz<SF> *P = static_cast<const Xyzz<SF> *>(lvl) + j0 + j;
        LF zi, izz, X, Y, zero;
        ta_ld(zi, &P->zz, comp);
        ta_ld(X, &P->x, comp);
        ta_ld(Y, &P->y, comp);
        f_mul_bs(zi, zi, ij);  // 1 / Z = ZZ / ZZZ
        f_sqr(izz, zi);
        f_mul_bs(X, X, izz);
        f_mul_bs(Y, Y, ij);
        if constexpr (SRC == TA_XYZZ_BLST) {  // internal -> blst limbs
          ta_mulk(X, X);
          ta_mulk(Y, Y);
        }
        f_csub(X);
        f_csub(Y);
        f_zero(zero);
        ta_sel(X, z, zero);
        ta_sel(Y, z, zero);
        if constexpr (SRC == TA_XYZZ_BLST) {
          uint64_t *o = static_cast<uint64_t *>(out) + (j0 + j) * 12 * G;
          ta_st_raw(o, X, comp);
          ta_st_raw(o + 6 * G, Y, comp);
        } else {
          Aff<SF> *o = static_cast<Aff<SF> *>(out) + j0 + j;
          ta_st(&o->x, X, comp);
          ta_st(&o->y, Y, comp);
        }
      } else {
        ta_st(static_cast<SF *>(lvl) + j0 + j, ij, comp);
      }
    }
  });
}

// the tree over n points at d_src (kind: every point source of to_affine.hpp), all
// in device memory; lv holds ta_level_elems(n) elements
template <int G, int SRC>
static void ta_tree_k(hipStream_t s, void *lv, size_t lv_bytes, const void *d_src, void *d_dst, size_t n) {
  typedef typename FieldOf<G>::F SF;
  const std::vector<size_t> lvs = ta_levels(n);
  std::vector<SF *> L(lvs.size());
  size_t off = 0;
  for (size_t i = 0; i < lvs.size(); ++i) {
    L[i] = static_cast<SF *>(lv) + off;
    off += lvs[i];
  }
  if (off * sizeof(SF) > lv_bytes) throw std::runtime_error("to_affine: level buffer too small");
  const unsigned B = 128;
  constexpr int UP = ta_is_jac(SRC) ? (int)TA_JAC : SRC;  // the way up reads Z alone
  hipLaunchKernelGGL((k_ta_up<G, UP>), dim3(nblk(lvs[0] * G, B)), dim3(B), 0, s, d_src, n, L[0], lvs[0]);
  MSM_HIP_CHECK(hipGetLastError());
  for (size_t i = 1; i < lvs.size(); ++i) {
    hipLaunchKernelGGL((k_ta_up<G, TA_LEVEL>), dim3(nblk(lvs[i] * G, B)), dim3(B), 0, s, (const void *)L[i - 1],
                       lvs[i - 1], L[i], lvs[i]);
    MSM_HIP_CHECK(hipGetLastError());
  }
  const size_t top = lvs.size() - 1;
  hipLaunchKernelGGL(k_ta_leaf<G>, dim3(nblk(lvs[top] * G, 64)), dim3(64), 0, s, L[top], lvs[top]);
  MSM_HIP_CHECK(hipGetLastError());
  for (size_t i = top; i >= 1; --i) {
    hipLaunchKernelGGL((k_ta_down<G, TA_LEVEL>), dim3(nblk(lvs[i] * G, B)), dim3(B), 0, s, (const SF *)L[i], lvs[i],
                       (void *)L[i - 1], lvs[i - 1], (void *)nullptr);
    MSM_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL((k_ta_down<G, SRC>), dim3(nblk(lvs[0] * G, B)), dim3(B), 0, s, (const SF *)L[0], lvs[0],
                     const_cast<void *>(d_src), n, d_dst);
  MSM_HIP_CHECK(hipGetLastError());
}

template <int G>
void ta_tree(hipStream_t s, void *lv, size_t lv_bytes, int kind, const void *d_src, void *d_dst, size_t n) {
  if (!n) return;
  if (kind == TA_JAC) ta_tree_k<G, TA_JAC>(s, lv, lv_bytes, d_src, d_dst, n);
  else if (kind == TA_XYZZ_BLST) ta_tree_k<G, TA_XYZZ_BLST>(s, lv, lv_bytes, d_src, d_dst, n);
  else if (kind == TA_XYZZ_ROWS) ta_tree_k<G, TA_XYZZ_ROWS>(s, lv, lv_bytes, d_src, d_dst, n);
  else if (kind == TA_JAC_ENC_C) ta_tree_k<G, TA_JAC_ENC_C>(s, lv, lv_bytes, d_src, d_dst, n);
  else if (kind == TA_JAC_ENC_S) ta_tree_k<G, TA_JAC_ENC_S>(s, lv, lv_bytes, d_src, d_dst, n);
  else throw std::runtime_error("to_affine: unknown source kind");
}
template void ta_tree<MSM_GROUP>(hipStream_t, void *, size_t, int, const void *, void *, size_t);

// one chunk, device to device: n <= the chunk the level buffer was sized for
template <int G>
void ToAffine<G>::kernels(hipStream_t s, const void *d_src, void *d_dst, size_t n) {
  ta_tree<G>(s, lv_.p, lv_.bytes, TA_JAC, d_src, d_dst, n);
}

template <int G>
void ToAffine<G>::run(hipStream_t cs, const void *src_dev_ptr, const std::vector<Run> &runs, void *dst, size_t n,
                      bool src_dev, bool dst_dev) {
  typedef typename FieldOf<G>::F SF;
  static_assert(sizeof(SF) == ELEM, "level element size");
  if (!n) return;
  DeviceGuard g(dev_);
  const size_t C = std::min(n, ta_chunk());
  size_t elems = 0;
  for (size_t v : ta_levels(C)) elems += v;
  lv_.ensure(elems * ELEM);
  if (!src_dev) in_.ensure(C * JAC);
  if (!dst_dev) out_.ensure(C * AFF);
  pipe_.begin(cs);          // the level buffers of the previous call
  size_t ri = 0, roff = 0;  // gather cursor: run, point within it
  auto pend = pipe_.pending([&](int slot, size_t off, size_t cnt) {
    memcpy(static_cast<uint8_t *>(dst) + off * AFF, out_.pin[slot], cnt * AFF);
  });
  size_t k = 0;
  for (size_t c0 = 0; c0 < n; c0 += C, ++k) {
    const size_t cnt = std::min(C, n - c0);
    const int slot = (int)(k & 1);
    const void *d_src;
    void *d_dst;
    if (!src_dev) {
      pipe_.upload(cs, slot, [&] {
        uint8_t *w = static_cast<uint8_t *>(in_.pin[slot]);
        for (size_t left = cnt; left;) {  // the gather writes straight into pinned memory
          if (ri >= runs.size()) throw std::runtime_error("to_affine: pointer runs do not cover the points");
          const size_t take = std::min(left, runs[ri].count - roff);
          memcpy(w, runs[ri].p + roff * JAC, take * JAC);
          w += take * JAC, left -= take, roff += take;
          if (roff == runs[ri].count) ++ri, roff = 0;
        }
      }, {{in_, slot, cnt * JAC}});
      d_src = in_.dev[slot].p;
    } else {
      d_src = static_cast<const uint8_t *>(src_dev_ptr) + c0 * JAC;
    }
    if (!dst_dev) {
      pipe_.out_open(cs, slot);
      d_dst = out_.dev[slot].p;
    } else {
      d_dst = static_cast<uint8_t *>(dst) + c0 * AFF;
    }
    kernels(cs, d_src, d_dst, cnt);
    pipe_.computed(cs, slot);
    if (!dst_dev) pipe_.download(cs, slot, pend, c0, cnt, {{out_, slot, cnt * AFF}});
  }
  pend.flush();
  pipe_.finish(cs);
}

template class ToAffine<MSM_GROUP>;

}  // namespace msm
