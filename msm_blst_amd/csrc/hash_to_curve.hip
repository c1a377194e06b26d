// hash_to_curve.hip -- bulk hash-to-curve for BLS12-381 on one MI355X (replaces
// a loop over the reference's blst_hash_to_g{1,2} / blst_encode_to_g{1,2} /
// blst_map_to_g{1,2}: ref src/map_to_g1.c:285-453, src/map_to_g2.c:173-401,
// src/hash_to_field.c:51-154; RFC 9380).
//
//   k_h2c_expand  message i -> the uniform bytes of its count G elements: one lane per
//                 message runs expand_message_xmd over SHA-256 (h2c_sha_block: a
//                 rolling 16-word schedule in registers), streaming aug || msg ||
//                 tail byte by byte from the state after Z_pad, then the b_i
//                 blocks from the host's template: 64 uniform bytes per element
//   k_h2c_reduce  element e: its 64 bytes -> blst layout by one two-product
//                 Montgomery reduction (2^256 < p)
//   k_h2c_sswu    element e -> a point of the isogenous curve E' (xyzz, internal
//                 form): the straight-line simplified SWU map with the xd == 0
//                 replacement; G1 one lane and one (p-3)/4 chain per element, G2
//                 one lane PAIR per element (fp2l.hpp) and four chains (1 / gxd,
//                 the quadratic character of the norm, the Fp2 square root);
//                 the sign of y follows sgn0 of the plain values
//   k_h2c_iso     point i: the sum of its two images on E' (general formulas
//                 with A', the doubling u == v and the inverse u == -v included),
//                 then the 11- / 3-isogeny by Horner over the __constant__ table,
//                 evaluated homogeneously (no inversion)
//   k_h2c_clear   point i: G1 [1 - z]P by double-and-add; G2 Budroni-Pintore,
//                 Psi^2(2P) - P - Psi(P) + [-z]([-z]P + P - Psi(P)), two 64-bit
//                 ladders, with one partial sum parked in memory so that at most
//                 two points are live
// and the batch inversion of to_affine.hip (ta_tree, TA_XYZZ_BLST) writes the
// affine points.  The affine form of a point is unique, so the output is bit for
// bit the reference's although the formulas differ (xyzz instead of Jacobian,
// homogeneous Horner instead of stored powers of Z^2).
//
// Every value between products is kept in range class S (fp.hpp): h_add / h_sub
// reduce after each sum, so no lazy-range bookkeeping is needed here.
#define MSM_H2C_DEVICE_TU
#define H2C_HD_CONST __device__ constexpr
#define H2C_FN __device__ __forceinline__
#include "fp.hpp"

#include "hash_to_curve.hpp"

#include <algorithm>
#include <cstring>

#include "decode_dev.hpp"
#include "pm_common.hpp"
#include "to_affine.hpp"

#ifndef MSM_GROUP
#error "define MSM_GROUP (1 or 2)"
#endif

namespace msm {

// ------------------------------------------------------------ expand ----
// lane e < n: the 64 big-endian bytes at raw + 16 e (words, the most significant
// first) -> the canonical blst element out + 6 e.  A kernel of its own: beside the
// SHA rounds its 42 uniform constants do not fit the scalar registers.
static __global__ void __launch_bounds__(128)
    k_h2c_reduce(const uint32_t *__restrict__ raw, size_t n, uint64_t *__restrict__ out) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const uint4 *s = reinterpret_cast<const uint4 *>(raw + 16 * e);
  const uint4 h0 = s[0], h1 = s[1], l0 = s[2], l1 = s[3];
  const uint32_t hi[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
  const uint32_t lo[8] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w};
  uint64_t lh[6], ll[6];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    lh[i] = ((uint64_t)hi[6 - 2 * i] << 32) | hi[7 - 2 * i];
    ll[i] = ((uint64_t)lo[6 - 2 * i] << 32) | lo[7 - 2 * i];
  }
  lh[4] = lh[5] = ll[4] = ll[5] = 0;
  Fp a, b, ka, kb, r;
  unpack384(a, ll);
  unpack384(b, lh);
  fp_set(ka, H2C_RED_LO);
  fp_set(kb, H2C_RED_HI);
  fp_mul2(r, a, ka, b, kb);  // (lo 2^776 + hi 2^1032) / 2^392 < 2p
  fp_csub_p(r);
  pack384(out + 6 * e, r);
}

// lane t < n: message t -> the 64 nelem uniform bytes at out + t nelem 16 (big-endian
// words).  Message t is
// msgs[offs[t] - bias .. offs[t + 1] - bias), or the msg_len bytes at msgs + t
// msg_len when offs is NULL; aug (or NULL): aug_len bytes per message, hashed first.
static __global__ void __launch_bounds__(128)
    k_h2c_expand(const uint8_t *__restrict__ msgs, const size_t *__restrict__ offs, size_t bias, size_t msg_len,
                 const uint8_t *__restrict__ aug, size_t aug_len, size_t n, const H2cTemplate *__restrict__ tp,
                 int nelem, uint32_t *__restrict__ out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint8_t *m;
  size_t ml;
  if (offs) {
    m = msgs + (offs[t] - bias);
    ml = offs[t + 1] - offs[t];
  } else {
    m = msgs + t * msg_len;
    ml = msg_len;
  }
  // (32-bit lengths: abi.cpp bounds every message and aug_len)
  const uint32_t al = aug ? (uint32_t)aug_len : 0u;
  const uint8_t *a = aug + t * (size_t)al;
  const uint32_t tail_len = tp->tail_len;
  const uint32_t body = al + (uint32_t)ml, total = body + tail_len;  // what follows Z_pad
  const uint64_t bits = ((uint64_t)total + 64) * 8;
  const uint32_t len = (total + 1 + 8 + 63) & ~63u;  // with the SHA padding
  uint32_t b0[8], w[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) b0[i] = H2C_SHA_ZPAD[i];
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = 0;
  uint32_t cur = 0;
#pragma unroll 1
  for (uint32_t j = 0; j < len; ++j) {
    // the byte at j: aug, msg, tail, then 0x80, zeros and the bit length (selects, one load)
    const uint8_t *src = j < al ? a + j : j < body ? m + (j - al) : tp->tail + (j - body);
    const uint32_t pad = j == total ? 0x80u : j + 8 < len ? 0u : (uint32_t)(bits >> (8 * (len - 1 - j))) & 0xffu;
    const uint32_t b = j < total ? (uint32_t)*src : pad;
    cur = (cur << 8) | b;
    if ((j & 3) == 3) {
#pragma unroll
      for (int i = 0; i < 15; ++i) w[i] = w[i + 1];
      w[15] = cur;
      if ((j & 63) == 63) h2c_sha_block(b0, w);
    }
  }
  // b_i = H(strxor(b_0, b_(i-1)) || i || DST_prime), i = 1 .. 2 nelem; two of them make an element
  const int nblk = (int)tp->nblk;
  uint32_t prev[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) prev[i] = 0;
  uint4 *o = reinterpret_cast<uint4 *>(out + t * (size_t)nelem * 16);
#pragma unroll 1
  for (int i = 1; i <= 2 * nelem; ++i) {
    uint32_t h[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) h[k] = H2C_SHA_H0[k];
#pragma unroll 1
    for (int blk = 0; blk < nblk; ++blk) {
#pragma unroll
      for (int k = 0; k < 16; ++k) w[k] = tp->blk[blk * 16 + k];
      if (blk == 0) {
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = b0[k] ^ prev[k];
        w[8] |= (uint32_t)i << 24;
      }
      h2c_sha_block(h, w);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) prev[k] = h[k];
    o[2 * (i - 1)] = make_uint4(h[0], h[1], h[2], h[3]);
    o[2 * (i - 1) + 1] = make_uint4(h[4], h[5], h[6], h[7]);
  }
}

// ------------------------------------------------------ field helpers ----
// sums reduced to class S at once (a, b in S)
template <class F>
__device__ __forceinline__ void h_add(F &r, const F &a, const F &b) {
  f_add(r, a, b);
  f_nred(r);
}
template <class F>
__device__ __forceinline__ void h_sub(F &r, const F &a, const F &b) {
  f_sub4(r, a, b);
  f_nred(r);
}
template <class F>
__device__ __forceinline__ void h_mul(F &r, const F &a, const F &b) {
  f_mul_bs(r, a, b);
}
template <class F>
__device__ __forceinline__ void h_sqr(F &r, const F &a) {
  f_sqr(r, a);
}
// a constant of hash_to_curve_consts.hpp: G1 the first row, G2 the lane's component
__device__ __forceinline__ void h_const(Fp &r, const uint32_t (*k)[NL]) { fp_set(r, k[0]); }
__device__ __forceinline__ void h_const(Fp2L &r, const uint32_t (*k)[NL]) {
  Fp c0, c1;
  fp_set(c0, k[0]);
  fp_set(c1, k[1]);
  pair_sel(r.c, pair_odd(), c1, c0);
}
template <class F>
__device__ __forceinline__ void h_sel(F &r, bool c, const F &a) {  // r = c ? a : r, c uniform over a pair
  dec_sel(dec_c(r), c, dec_c(a));
}
// -a for a in S (an exact zero stays zero)
template <class F>
__device__ __forceinline__ void h_cneg(F &a, bool neg) {
  fp_cneg4(dec_c(a), dec_c(a), neg);
  f_nred(a);
}
// sgn0 of RFC 9380 on the plain value: the parity of c0, of c1 when c0 is zero
template <int G>
__device__ __forceinline__ bool h_sgn0(const typename DecLane<G>::LF &a) {
  Fp v;
  dec_plain(v, dec_c(a));
  const uint32_t own = (v.v[0] & 1u) | (fp_is_zero_exact(v) ? 2u : 0u);
  if constexpr (G == 1) {
    return (own & 1u) != 0;
  } else {
    const uint32_t par = pair_swap(own);
    const uint32_t re = pair_odd() ? par : own, im = pair_odd() ? own : par;
    return ((re & 1u) | ((re >> 1) & im & 1u)) != 0;
  }
}

// --------------------------------------------------------------- sswu ----
// lane (pair) e < n: element e of u -> out[e] on E', as (xn xd, y xd^3, xd^3, xd^2)
template <int G>
static __global__ void __launch_bounds__(128)
    k_h2c_sswu(const uint64_t *__restrict__ u_in, size_t n, Xyzz<typename FieldOf<G>::F> *__restrict__ out) {
  typedef typename DecLane<G>::LF LF;
  const size_t tt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int comp = G == 2 ? (int)(tt & 1) : 0;
  const size_t t = G == 2 ? tt >> 1 : tt;
  if (t >= n) return;  // whole pairs only
  LF u, uu, zuu, tv2, x1n, xd, k, one;
  fp_from_blst(dec_c(u), u_in + t * 6 * G + 6 * comp);
  h_sqr(uu, u);
  h_const(k, H2C_Z);
  h_mul(zuu, uu, k);
  h_sqr(tv2, zuu);
  h_add(tv2, tv2, zuu);  // Z^2 u^4 + Z u^2
  f_one(one);
  h_add(x1n, tv2, one);
  h_const(k, H2C_B);
  h_mul(x1n, x1n, k);  // x1n = (tv2 + 1) B
  h_const(k, H2C_MINUS_A);
  h_mul(xd, tv2, k);  // xd = -A tv2
  const bool e1 = f_is_zero_S(xd);
  h_const(k, H2C_ZA);
  h_sel(xd, e1, k);  // xd == 0: xd = Z A
  LF xd2, gxd, gx1, t1;
  h_sqr(xd2, xd);
  h_mul(gxd, xd2, xd);
  h_const(k, H2C_A);
  h_mul(t1, xd2, k);
  h_sqr(gx1, x1n);
  h_add(gx1, gx1, t1);
  h_mul(gx1, gx1, x1n);
  h_const(k, H2C_B);
  h_mul(t1, gxd, k);
  h_add(gx1, gx1, t1);  // gx1 = x1n^3 + A x1n xd^2 + B xd^3
  LF y;
  bool e2;  // gx1 / gxd is a square: x = x1n / xd, else x = Z u^2 x1n / xd
#if MSM_GROUP == 1
  {
    // y1 = (gx1 gxd^3)^((p-3)/4) gx1 gxd = sqrt(+-gx1 / gxd); the sign is the character of gx1 gxd^3
    Fp tv4, r, chi, onev, y2;
    h_mul(tv2, gx1, gxd);
    h_sqr(tv4, gxd);
    h_mul(tv4, tv4, tv2);
    dec_pow_pm3d4(r, tv4);
    fp_mul(y, r, tv2);
    fp_sqr(chi, r);
    fp_mul(chi, chi, tv4);  // tv4^((p-1)/2)
    fp_one(onev);
    e2 = dec_eq(chi, onev) || fp_is_zero_lt2p(tv4);
    h_const(k, H2C_C2);
    h_mul(y2, y, k);  // y2 = y1 sqrt(-Z^3) u^3
    h_mul(y2, y2, uu);
    h_mul(y2, y2, u);
    h_sel(y, !e2, y2);
  }
#else
  {
    LF ginv, a, az, z3;
    f_inv(ginv, gxd);
    h_mul(a, gx1, ginv);  // g(x1)
    Fp own = a.c, sq, psq, nrm, r, chi, onev;
    fp_sqr(sq, own);
    pair_swap(psq, sq);
    fp_add(nrm, sq, psq);
    fp_nred(nrm);  // the norm: a is a square in Fp2 iff it is one in Fp
    dec_pow_pm3d4(r, nrm);
    fp_sqr(chi, r);
    fp_mul(chi, chi, nrm);
    fp_one(onev);
    e2 = dec_eq(chi, onev) || fp_is_zero_lt2p(nrm);
    h_sqr(z3, zuu);
    h_mul(z3, z3, zuu);
    h_mul(az, a, z3);  // g(x2) = (Z u^2)^3 g(x1)
    h_sel(a, !e2, az);
    dec_sqrt(y, a);
  }
#endif
  LF x2n;
  h_mul(x2n, zuu, x1n);
  h_sel(x1n, !e2, x2n);
  const bool flip = h_sgn0<G>(u) != h_sgn0<G>(y);
  h_cneg(y, flip);
  Xyzz<LF> q;
  h_mul(q.x, x1n, xd);
  h_sqr(q.zz, xd);
  h_mul(q.zzz, q.zz, xd);
  h_mul(q.y, y, q.zzz);
  pm_st_xyzz(&out[t], q, comp);
}

// ------------------------------------------------------- add, isogeny ----
// 2p on y^2 = x^3 + A x + B (dbl-2008-s-1 with the a ZZ^2 term), p in S
template <class F>
__device__ __forceinline__ void h2c_dbl_a(Xyzz<F> &r, const Xyzz<F> &p, const F &A) {
  F U, V, W, S, M, t, X3, Y3;
  h_add(U, p.y, p.y);
  h_sqr(V, U);
  h_mul(W, V, U);
  h_mul(S, p.x, V);
  h_sqr(M, p.x);
  h_add(t, M, M);
  h_add(M, t, M);
  h_sqr(t, p.zz);
  h_mul(t, t, A);
  h_add(M, M, t);  // M = 3 X^2 + A ZZ^2
  h_sqr(X3, M);
  h_sub(X3, X3, S);
  h_sub(X3, X3, S);
  h_sub(t, S, X3);
  h_mul(t, t, M);
  h_mul(Y3, W, p.y);
  h_sub(Y3, t, Y3);
  h_mul(r.zz, V, p.zz);
  h_mul(r.zzz, W, p.zzz);
  r.x = X3;
  r.y = Y3;
}
// p += q on E' (add-2008-s); neither is infinity, both in S
template <int G>
__device__ __forceinline__ void h2c_add_a(Xyzz<typename DecLane<G>::LF> &p, const Xyzz<typename DecLane<G>::LF> &q) {
  typedef typename DecLane<G>::LF LF;
  LF U1, U2, S1, S2, Pd, R;
  h_mul(U1, p.x, q.zz);
  h_mul(U2, q.x, p.zz);
  h_mul(S1, p.y, q.zzz);
  h_mul(S2, q.y, p.zzz);
  h_sub(Pd, U2, U1);
  h_sub(R, S2, S1);
  if (f_is_zero_S(Pd)) {
    if (f_is_zero_S(R)) {  // u == v: the doubling needs A'
      LF A;
      h_const(A, H2C_A);
      const Xyzz<LF> d = p;
      h2c_dbl_a(p, d, A);
    } else {  // u == -v
      xyzz_set_inf(p);
    }
    return;
  }
  LF PP, PPP, Q, X3, Y3, t;
  h_sqr(PP, Pd);
  h_mul(PPP, PP, Pd);
  h_mul(Q, U1, PP);
  h_sqr(X3, R);
  h_sub(X3, X3, PPP);
  h_sub(X3, X3, Q);
  h_sub(X3, X3, Q);
  h_sub(t, Q, X3);
  h_mul(t, t, R);
  h_mul(S1, S1, PPP);
  h_sub(Y3, t, S1);
  h_mul(p.zz, p.zz, q.zz);
  h_mul(p.zz, p.zz, PP);
  h_mul(p.zzz, p.zzz, q.zzz);
  h_mul(p.zzz, p.zzz, PPP);
  p.x = X3;
  p.y = Y3;
}
// sum_i c_i X^i ZZ^(deg - i) for the coefficients H2C_ISO[off .. off + deg]
template <int G>
__device__ __forceinline__ void h2c_poly(typename DecLane<G>::LF &acc, const Xyzz<typename DecLane<G>::LF> &p, int off,
                                         int deg) {
  typename DecLane<G>::LF zp = p.zz, c, t;
  h_const(acc, H2C_ISO[off + deg]);
#pragma unroll 1
  for (int i = deg - 1; i >= 0; --i) {
    h_mul(acc, acc, p.x);
    h_const(c, H2C_ISO[off + i]);
    h_mul(t, zp, c);
    h_add(acc, acc, t);
    if (i) h_mul(zp, zp, p.zz);
  }
}
// the isogeny E' -> E on an xyzz point in S: x = xn / (xd ZZ), y = Y yn / (ZZZ yd)
// with the homogeneous polynomials; the result is (XN XD YD^2, YN XD^3 YD^2, Z^3, Z^2), Z = XD YD
template <int G>
__device__ __forceinline__ void h2c_iso(Xyzz<typename DecLane<G>::LF> &p) {
  typedef typename DecLane<G>::LF LF;
  const bool inf = xyzz_is_inf(p);
  LF xn, xd, yn, yd, Z, zz;
  h2c_poly<G>(xn, p, H2C_OXN, H2C_DXN);
  h2c_poly<G>(xd, p, H2C_OXD, H2C_DXD);
  h2c_poly<G>(yn, p, H2C_OYN, H2C_DYN);
  h2c_poly<G>(yd, p, H2C_OYD, H2C_DYD);
  h_mul(xd, xd, p.zz);
  h_mul(yn, yn, p.y);
  h_mul(yd, yd, p.zzz);
  h_mul(Z, xd, yd);
  const bool z0 = f_is_zero_S(Z);  // a point of the kernel
  h_sqr(zz, Z);
  h_mul(xn, xn, yd);
  h_mul(p.x, xn, Z);
  h_mul(yn, yn, xd);
  h_mul(p.y, yn, zz);
  h_mul(p.zzz, zz, Z);
  p.zz = zz;
  if (inf || z0) xyzz_set_inf(p);
}

// lane (pair) t < n: out[t] = iso(e[t count] (+ e[t count + 1]))
template <int G>
static __global__ void __launch_bounds__(128)
    k_h2c_iso(const Xyzz<typename FieldOf<G>::F> *__restrict__ e, size_t n, int count,
              Xyzz<typename FieldOf<G>::F> *__restrict__ out) {
  typedef typename DecLane<G>::LF LF;
  const size_t tt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int comp = G == 2 ? (int)(tt & 1) : 0;
  const size_t t = G == 2 ? tt >> 1 : tt;
  if (t >= n) return;  // whole pairs only
  Xyzz<LF> p;
  pm_ld_xyzz(p, &e[t * (size_t)count], comp);
  if (count == 2) {
    Xyzz<LF> q;
    pm_ld_xyzz(q, &e[t * 2 + 1], comp);
    h2c_add_a<G>(p, q);
  }
  h2c_iso<G>(p);
  pm_st_xyzz(&out[t], p, comp);
}

// ------------------------------------------------------------ cofactor ----
constexpr uint64_t H2C_Z_ABS = DEC_Z_ABS;  // the curve parameter is -|z|

// The general add of the clearing kernel: the 13-reduction form (ec.hpp
// xyzz_add).  k_h2c_clear holds two ladders and five adds in one body; with the
// regrouped add it went from 246 to 301 registers (G1, two waves to one) and
// spilled (G2).
template <class F>
__device__ __forceinline__ void h2c_add(Xyzz<F> &acc, const Xyzz<F> &b) {
  xyzz_add<F, false>(acc, b);
}

// acc = [k] base for a constant k with bit 63 set; acc enters as base
template <class F>
__device__ __forceinline__ void h2c_times(Xyzz<F> &acc, const Xyzz<F> &base, uint64_t k) {
#pragma unroll 1
  for (int b = 62; b >= 0; --b) {
    const Xyzz<F> tmp = acc;
    xyzz_dbl(acc, tmp);
    if ((k >> b) & 1) h2c_add(acc, base);  // uniform: k is a constant
  }
}
template <class F>
__device__ __forceinline__ void h2c_negate(Xyzz<F> &p) {
  if (!xyzz_is_inf(p)) h_cneg(p.y, true);
}
// psi(x, y) = (conj(x) cx, conj(y) cy) on an xyzz point (conjugation is a field
// automorphism: ZZ and ZZZ are conjugated too); constants as in k_decode_group
__device__ __forceinline__ void h2c_psi(Xyzz<Fp2L> &p) {
  const bool inf = xyzz_is_inf(p);
  const bool odd = pair_odd();
  f_nred(p.x);  // class X -> S
  h_cneg(p.x, odd);
  h_cneg(p.y, odd);
  h_cneg(p.zzz, odd);
  h_cneg(p.zz, odd);
  Fp2L cx, cy;
  Fp k;
  fp_zero(cx.c);
  fp_set(k, DEC_PSI_CX1);
  dec_sel(cx.c, odd, k);
  fp_set(cy.c, DEC_PSI_CY0);
  fp_set(k, DEC_PSI_CY1);
  dec_sel(cy.c, odd, k);
  f_mul_bs(p.x, p.x, cx);
  f_mul_bs(p.y, p.y, cy);
  if (inf) xyzz_set_inf(p);
}

// lane (pair) t < n: pts[t] = the cleared image of pts[t]; G2 parks a partial sum in tmp[t stride]
template <int G>
static __global__ void __launch_bounds__(128)
    k_h2c_clear(Xyzz<typename FieldOf<G>::F> *__restrict__ pts, size_t n, Xyzz<typename FieldOf<G>::F> *__restrict__ tmp,
                int stride) {
  typedef typename DecLane<G>::LF LF;
  const size_t tt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int comp = G == 2 ? (int)(tt & 1) : 0;
  const size_t t = G == 2 ? tt >> 1 : tt;
  if (t >= n) return;  // whole pairs only
  Xyzz<LF> P, A;
  pm_ld_xyzz(P, &pts[t], comp);
  if constexpr (G == 1) {
    A = P;
    h2c_times(A, P, H2C_Z_ABS + 1);  // [1 - z]P
  } else {
    Xyzz<typename FieldOf<G>::F> *park = &tmp[t * (size_t)stride];
    {  // Psi^2(2P) - P - Psi(P), formed as -((P - Psi^2(2P)) + Psi(P))
      const Xyzz<LF> c = P;
      xyzz_dbl(A, c);
    }
    h2c_psi(A);
    h2c_psi(A);
    h2c_negate(A);
    h2c_add(A, P);
    h2c_psi(P);
    h2c_add(A, P);
    h2c_negate(A);
    f_nred(A.x);
    pm_st_xyzz(park, A, comp);
    // t0 = [-z]P + P - Psi(P)
    pm_ld_xyzz(P, &pts[t], comp);
    A = P;
    h2c_times(A, P, H2C_Z_ABS);
    h2c_add(A, P);
    h2c_psi(P);
    h2c_negate(P);
    h2c_add(A, P);
    // [-z] t0 = [z^2 - z]P + [z]Psi(P), plus the parked sum
    P = A;
    h2c_times(A, P, H2C_Z_ABS);
    pm_ld_xyzz(P, park, comp);
    h2c_add(A, P);
  }
  pm_st_xyzz(&pts[t], A, comp);
}

// -------------------------------------------------------------- engine ----
// one chunk of the map, device to device: n * count elements at d_u -> n affine points at d_dst
template <int G>
void HashToCurve<G>::map_kernels(hipStream_t s, const void *d_u, void *d_dst, size_t n, int count) {
  typedef Xyzz<typename FieldOf<G>::F> XZ;
  const unsigned B = 128;
  hipLaunchKernelGGL(k_h2c_sswu<G>, dim3(nblk(n * count * G, B)), dim3(B), 0, s, static_cast<const uint64_t *>(d_u),
                     n * count, e_.as<XZ>());
  MSM_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_h2c_iso<G>, dim3(nblk(n * G, B)), dim3(B), 0, s, e_.as<XZ>(), n, count, x_.as<XZ>());
  MSM_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_h2c_clear<G>, dim3(nblk(n * G, B)), dim3(B), 0, s, x_.as<XZ>(), n, e_.as<XZ>(), count);
  MSM_HIP_CHECK(hipGetLastError());
  ta_tree<G>(s, lv_.p, lv_.bytes, TA_XYZZ_BLST, x_.p, d_dst, n);
}

template <int G>
void HashToCurve<G>::run(hipStream_t cs, int mode, const void *u, const H2cMsgs &m, const H2cTemplate *tmpl, void *dst,
                         size_t n, int count, bool src_dev, bool dst_dev) {
  if (!n) return;
  DeviceGuard g(dev_);
  const bool hashing = mode != H2C_MAP, mapping = mode != H2C_FIELD;
  const size_t C = std::min(n, h2c_chunk());
  const size_t UB = (size_t)count * ELEM;      // bytes of the elements of an entry
  const size_t OUT = mapping ? AFF : UB;       // bytes of an entry of dst
  const bool offs_up = hashing && m.offsets;   // the offsets are host memory whatever the source is
  const bool stage = !src_dev || offs_up;
  auto msg_begin = [&](size_t i) { return m.offsets ? m.offsets[i] : i * m.msg_len; };
  // the previous call has finished: its chunk buffers and its template are free
  pipe_.begin_on_host();
  if (mapping) {
    e_.ensure(C * count * XYZZ);
    x_.ensure(C * XYZZ);
    lv_.ensure(ta_level_elems(C) * 56 * G);
  }
  if (mode == H2C_HASH) u_.ensure(C * UB);
  if (hashing) r_.ensure(C * count * G * 64);
  if (!src_dev) {
    size_t in = 1;
    if (!hashing) in = C * UB;
    else
      for (size_t c0 = 0; c0 < n; c0 += C) in = std::max(in, msg_begin(std::min(n, c0 + C)) - msg_begin(c0));
    in_.ensure(in);
    if (hashing && m.aug && m.aug_len) aug_.ensure(C * m.aug_len);
  }
  if (offs_up) off_.ensure((C + 1) * sizeof(size_t));
  if (!dst_dev) out_.ensure(C * OUT);
  if (hashing) {
    tp_.ensure(sizeof(H2cTemplate));
    tpl_.ensure(sizeof(H2cTemplate), false);
    memcpy(tpl_.pin[0], tmpl, sizeof(H2cTemplate));
    MSM_HIP_CHECK(hipMemcpyAsync(tp_.p, tpl_.pin[0], sizeof(H2cTemplate), hipMemcpyHostToDevice, cs));
  }
  auto pend = pipe_.pending([&](int slot, size_t off, size_t cnt) {
    memcpy(static_cast<uint8_t *>(dst) + off * OUT, out_.pin[slot], cnt * OUT);
  });
  const bool has_aug = hashing && m.aug && m.aug_len;
  size_t k = 0;
  for (size_t c0 = 0; c0 < n; c0 += C, ++k) {
    const size_t cnt = std::min(C, n - c0);
    const int slot = (int)(k & 1);
    const size_t b0 = hashing ? msg_begin(c0) : 0, b1 = hashing ? msg_begin(c0 + cnt) : 0;
    if (stage) {
      // the bytes of the three upload lanes (one event for them); a chunk of empty messages sends none
      const size_t in = src_dev ? 0 : hashing ? b1 - b0 : cnt * UB;
      const size_t ab = !src_dev && has_aug ? cnt * m.aug_len : 0, ob = offs_up ? (cnt + 1) * sizeof(size_t) : 0;
      pipe_.upload(cs, slot, [&] {
        if (in) memcpy(in_.pin[slot], hashing ? m.msgs + b0 : static_cast<const uint8_t *>(u) + c0 * UB, in);
        if (ab) memcpy(aug_.pin[slot], m.aug + c0 * m.aug_len, ab);
        if (ob) memcpy(off_.pin[slot], m.offsets + c0, ob);
      }, {{in_, slot, in}, {aug_, slot, ab}, {off_, slot, ob}});
    }
    if (!dst_dev) pipe_.out_open(cs, slot);
    void *d_out = dst_dev ? static_cast<void *>(static_cast<uint8_t *>(dst) + c0 * OUT) : out_.dev[slot].p;
    const void *d_u = src_dev ? static_cast<const void *>(static_cast<const uint8_t *>(u) + c0 * UB) : in_.dev[slot].p;
    if (hashing) {
      // offsets index the caller's array (bias 0) or the staged bytes of this chunk (bias b0)
      const uint8_t *d_msgs = src_dev ? (m.offsets ? m.msgs : m.msgs + b0) : in_.dev[slot].as<uint8_t>();
      const size_t bias = src_dev ? 0 : b0;
      const uint8_t *d_aug = !has_aug ? nullptr : src_dev ? m.aug + c0 * m.aug_len : aug_.dev[slot].as<uint8_t>();
      const size_t *d_off = m.offsets ? off_.dev[slot].as<size_t>() : nullptr;
      void *d_el = mapping ? u_.p : d_out;
      const size_t nel = cnt * count * G;
      hipLaunchKernelGGL(k_h2c_expand, dim3(nblk(cnt, 128)), dim3(128), 0, cs, d_msgs, d_off, bias, m.msg_len, d_aug,
                         m.aug_len, cnt, tp_.as<H2cTemplate>(), count * G, r_.as<uint32_t>());
      MSM_HIP_CHECK(hipGetLastError());
      hipLaunchKernelGGL(k_h2c_reduce, dim3(nblk(nel, 128)), dim3(128), 0, cs, r_.as<uint32_t>(), nel,
                         static_cast<uint64_t *>(d_el));
      MSM_HIP_CHECK(hipGetLastError());
      d_u = d_el;
    }
    if (mapping) map_kernels(cs, d_u, d_out, cnt, count);
    pipe_.computed(cs, slot);
    if (!dst_dev) pipe_.download(cs, slot, pend, c0, cnt, {{out_, slot, cnt * OUT}});
  }
  pend.flush();
  pipe_.finish(cs);
}

template class HashToCurve<MSM_GROUP>;

}  // namespace msm
