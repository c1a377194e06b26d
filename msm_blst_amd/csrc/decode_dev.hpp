// decode_dev.hpp -- device helpers of the bulk point decoding that other kernels
// share (decode.hip, hash_to_curve.hip, sig_verify.hip): the constants of the
// square-root chain, of the sign rule and of the endomorphisms, a^((p-3)/4) by
// fixed 2-bit windows, square roots in Fp and, on lane pairs, in Fp2, the sign
// of y, and the subgroup test.  Included by .hip files only.
#pragma once
#include "pair_kernels.hpp"

namespace msm {

// (p - 3) / 4, the exponent of the square-root chain: a^((p-3)/4) a = a^((p+1)/4)
__device__ constexpr uint64_t PM3D4[6] = {0xee7fbfffffffeaaaull, 0x07aaffffac54ffffull, 0xd9cc34a83dac3d89ull,
                                          0xd91dd2e13ce144afull, 0x92c6e9ed90d2eb35ull, 0x0680447a8e5ff9a6ull};
// 2^784 mod p: integer limbs -> internal form (R = 2^392) in one product
MSM_CONST uint32_t DEC_R2[NL] = {0x10370ed, 0x6d1c345, 0xe243d62, 0xec45c53, 0x3b1d65a, 0x093317d, 0xb4f36a0,
                                 0x5d74088, 0xc10ea72, 0x865d118, 0x7320a75, 0xfd5cd50, 0xcc8a759, 0x000c8d4};
// 1/2 and 4 in internal form; b = 4 (G1), 4 + 4i (G2)
MSM_CONST uint32_t DEC_HALF[NL] = {0x1a3fe5c, 0xec00000, 0x001588c, 0x066f369, 0x6390970, 0xc1d1048, 0x01bb34f,
                                   0x6d07b9f, 0x4d84da1, 0x894bdd8, 0x28aecc7, 0x009653e, 0x32cfe7d, 0x0002bbd};
MSM_CONST uint32_t DEC_FOUR[NL] = {0xd1ff2e0, 0x6000000, 0x00ac467, 0x3379b48, 0x1c84b80, 0x0e88243, 0x0dd9a7e,
                                   0x683dcf8, 0x6c26d0b, 0x4a5eec2, 0x457663c, 0x04b29f1, 0x967f3e8, 0x0015de9};
// (p - 1) / 2, plain integer
MSM_CONST uint32_t DEC_PM1H[NL] = {0xfffd555, 0xff7ffff, 0x9ffffdc, 0xffff58a, 0xb120f55, 0x507b587, 0xfb39869,
                                   0x79c2895, 0x23ba5c2, 0xa5d66bb, 0xdd3db21, 0xf34d258, 0x8f51cbf, 0x000d008};
// sigma^2(x, y) = (beta x, y): the cube root of unity with [z^2]P = (beta x, -y) on G1 (internal form)
MSM_CONST uint32_t DEC_BETA[NL] = {0xa75929a, 0x681b798, 0x22a3e9d, 0xabc02bf, 0x4e5bb45, 0x55e6e7e, 0x4814117,
                                   0x6d04f1b, 0xae3387d, 0x54acb0c, 0x0a4c74b, 0x56138b5, 0xb64e066, 0x00076f2};
// psi(x, y) = (conj(x) cx, conj(y) cy), cx = (1 + i)^-((p-1)/3) = cx1 i, cy = (1 + i)^-((p-1)/2) (internal form)
MSM_CONST uint32_t DEC_PSI_CX1[NL] = {0x58a1811, 0x96e4867, 0x1d5c11c, 0x543e856, 0x13e6366, 0x4b0fc91, 0xae5efbb,
                                      0x8680210, 0x9941307, 0xf700269, 0xb02eef7, 0x9086bfc, 0x6855919, 0x001291e};
MSM_CONST uint32_t DEC_PSI_CY0[NL] = {0xcc17b84, 0xcc5da55, 0x1835de7, 0x3e1e677, 0x9e4ae31, 0x9b9a07a, 0xd662557,
                                      0xb7f1997, 0x71cc4da, 0xa667f92, 0x65115fe, 0x4a3370c, 0xe5b746a, 0x000d16d};
MSM_CONST uint32_t DEC_PSI_CY1[NL] = {0x33e2f27, 0x32a25aa, 0x27ca1d2, 0xc1e049e, 0xc3f707a, 0x055ca94, 0x2010b7b,
                                      0x3b93794, 0xd5a86aa, 0xa544de3, 0x556a044, 0x9c66da5, 0x38ec515, 0x000cea3};
constexpr uint64_t DEC_Z_ABS = 0xd201000000010000ull;

template <int G>
struct DecLane;
template <>
struct DecLane<1> {
  typedef Fp LF;
};
template <>
struct DecLane<2> {
  typedef Fp2L LF;
};
__device__ __forceinline__ Fp &dec_c(Fp &a) { return a; }
__device__ __forceinline__ Fp &dec_c(Fp2L &a) { return a.c; }
__device__ __forceinline__ const Fp &dec_c(const Fp &a) { return a; }
__device__ __forceinline__ const Fp &dec_c(const Fp2L &a) { return a.c; }

// a value over the lanes of a point: G1 the lane's own, G2 combined with the partner's
template <int G>
__device__ __forceinline__ uint32_t dec_or(uint32_t v) {
  return G == 2 ? (v | pair_swap(v)) : v;
}
template <int G>
__device__ __forceinline__ uint32_t dec_swap(uint32_t v) {
  return G == 2 ? pair_swap(v) : v;
}
template <int G>
__device__ __forceinline__ bool dec_all(bool b) {
  const uint32_t v = b ? 1u : 0u;
  return (G == 2 ? (v & pair_swap(v)) : v) != 0;
}

// 48 big-endian bytes at s (4-byte aligned) -> integer limbs.  top = the three
// flag bits of byte 0; nz = OR of the words (the flag bits left out when
// `mask`, which also clears them in the value).
__device__ __forceinline__ void dec_ld_be(Fp &r, uint32_t &top, uint32_t &nz, const uint32_t *s, bool mask) {
  uint64_t l[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    uint32_t lo = __builtin_bswap32(s[11 - 2 * i]), hi = __builtin_bswap32(s[10 - 2 * i]);
    if (i == 5) {
      top = hi >> 29;
      hi = mask ? (hi & 0x1fffffffu) : hi;
    }
    l[i] = ((uint64_t)hi << 32) | lo;
  }
  uint64_t o = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) o |= l[i];
  nz = (uint32_t)o | (uint32_t)(o >> 32);
  unpack384(r, l);
}
// a >= p for normalized integer limbs
__device__ __forceinline__ bool dec_ge_p(const Fp &a) {
  int32_t br = 0;
#pragma unroll
  for (int i = 0; i < NL; ++i) br = ((int32_t)a.v[i] - (int32_t)P28[i] + br) >> 28;
  return br == 0;
}
// a > (p - 1) / 2 for a canonical plain integer
__device__ __forceinline__ bool dec_gt_half(const Fp &a) {
  int32_t br = 0;
#pragma unroll
  for (int i = 0; i < NL; ++i) br = ((int32_t)DEC_PM1H[i] - (int32_t)a.v[i] + br) >> 28;
  return br != 0;
}
__device__ __forceinline__ void dec_mulk(Fp &r, const Fp &a, const uint32_t *c) {
  Fp k;
  fp_set(k, c);
  fp_mul(r, a, k);
}
// the plain integer of an internal value (any lazy class), canonical
__device__ __forceinline__ void dec_plain(Fp &r, const Fp &a) {
  Fp one;
  fp_zero(one);
  one.v[0] = 1;
  fp_mul(r, a, one);
  fp_csub_p(r);
}
// a == b mod p; a normalized < 10p (class S or X), b in S
__device__ __forceinline__ bool dec_eq(const Fp &a, const Fp &b) {
  Fp d, c;
  fp_sub<4>(d, a, b);  // a + 4p - b < 14p
  fp_canon(c, d);
  return fp_is_zero_exact(c);
}
// a + b == 0 mod p; a, b in S
__device__ __forceinline__ bool dec_sum_is_zero(const Fp &a, const Fp &b) {
  Fp d, c;
  fp_add(d, a, b);
  fp_canon(c, d);
  return fp_is_zero_exact(c);
}
__device__ __forceinline__ void dec_sel(Fp &r, bool c, const Fp &a) {  // r = c ? a : r
#pragma unroll
  for (int i = 0; i < NL; ++i) r.v[i] = c ? a.v[i] : r.v[i];
}

// a^((p-3)/4): fixed 2-bit windows of a constant exponent (uniform control
// flow), as fp_inv (fp2l_mem.hpp).  Input any lazy value, output S.
__device__ __forceinline__ void dec_pow_pm3d4(Fp &r, const Fp &a) {
  Fp a1 = a, a2, a3, acc;
  fp_norm(a1);
  fp_sqr(a2, a1);
  fp_mul(a3, a2, a1);
  fp_one(acc);
  for (int k = 189; k >= 0; --k) {  // 2-bit windows of (p - 3) / 4 (379 bits), from the top
    if (k != 189) {
      fp_sqr(acc, acc);
      fp_sqr(acc, acc);
    }
    const uint32_t w = (uint32_t)(PM3D4[k >> 5] >> ((k & 31) * 2)) & 3u;
    if (w) {
      const uint32_t m1 = 0u - (uint32_t)(w == 1), m2 = 0u - (uint32_t)(w == 2), m3 = 0u - (uint32_t)(w == 3);
      Fp t;
#pragma unroll
      for (int i = 0; i < NL; ++i) t.v[i] = (a1.v[i] & m1) | (a2.v[i] & m2) | (a3.v[i] & m3);
      fp_mul(acc, acc, t);
    }
  }
  r = acc;
}

// a candidate root of a (in S); the caller verifies y^2 == a
__device__ __forceinline__ void dec_sqrt(Fp &y, const Fp &a) {
  Fp r;
  dec_pow_pm3d4(r, a);
  fp_mul(y, r, a);
}
// Fp2 through the norm: with n = sqrt(a0^2 + a1^2), t = (a0 + n) / 2 (or
// (a0 - n) / 2 when that is zero), r = t^((p-3)/4), c = r t, d = a1 r / 2:
//   c^2 == t   ->  y = c + d i        (r = 1 / c)
//   c^2 == -t  ->  y = -d + c i       (r = -1 / c; the other of the two t has the root)
// Every value is formed on both lanes; each keeps its own component.  A
// non-square a gives a y that fails the caller's y^2 == a.
__device__ __forceinline__ void dec_sqrt(Fp2L &y, const Fp2L &a) {
  const bool odd = pair_odd();
  Fp par, a0, a1, n, s, t1, t2, r, c, d, c2;
  pair_swap(par, a.c);
  pair_sel(a0, odd, par, a.c);
  pair_sel(a1, odd, a.c, par);
  fp_sqr(n, a0);
  fp_sqr(s, a1);
  fp_add(n, n, s);  // < 4p lazy
  dec_pow_pm3d4(r, n);
  fp_norm(n);
  fp_mul(s, r, n);  // sqrt of the norm, S
  fp_add(t1, a0, s);
  fp_sub<4>(t2, a0, s);
  dec_mulk(t1, t1, DEC_HALF);
  dec_mulk(t2, t2, DEC_HALF);
  dec_sel(t1, fp_is_zero_lt2p(t1), t2);
  dec_pow_pm3d4(r, t1);
  fp_mul(c, r, t1);
  fp_mul(d, a1, r);
  dec_mulk(d, d, DEC_HALF);
  fp_sqr(c2, c);
  const bool good = dec_eq(c2, t1);
  Fp nd;
  fp_neg<4>(nd, d);
  fp_nred(nd);
  pair_sel(y.c, odd, d, c);     // good: even c, odd d
  pair_sel(nd, odd, c, nd);     // else: even -d, odd c
  dec_sel(y.c, !good, nd);
}

// the 0x20 flag of y (internal form): y > (p - 1) / 2, for Fp2 decided by the
// imaginary part unless it is zero (ref sgn0_pty_mont_384x >> 1)
__device__ __forceinline__ bool dec_sign(const Fp &y) {
  Fp v;
  dec_plain(v, y);
  return dec_gt_half(v);
}
__device__ __forceinline__ bool dec_sign(const Fp2L &y) {
  Fp v;
  dec_plain(v, y.c);
  const uint32_t own = (dec_gt_half(v) ? 1u : 0u) | (fp_is_zero_exact(v) ? 2u : 0u);
  const uint32_t par = pair_swap(own);
  const uint32_t im = pair_odd() ? own : par, re = pair_odd() ? par : own;
  return ((im & 2u) ? (re & 1u) : (im & 1u)) != 0;
}

// r = [k] p for the constant k = hi 2^64 + lo of `bits` bits (top bit set), p
// affine and not infinity; r enters as p
template <class F>
__device__ __forceinline__ void dec_times(Xyzz<F> &r, const Aff<F> &p, uint64_t hi, uint64_t lo, int bits) {
  for (int b = bits - 2; b >= 0; --b) {
    Xyzz<F> tmp = r;
    xyzz_dbl(r, tmp);
    if (((b >= 64 ? hi >> (b - 64) : lo >> b) & 1) != 0) xyzz_madd(r, p, false);  // uniform: k is a constant
  }
}
constexpr unsigned __int128 DEC_ZZ = (unsigned __int128)DEC_Z_ABS * DEC_Z_ABS;  // z^2, 128 bits
constexpr uint64_t DEC_ZZ_HI = (uint64_t)(DEC_ZZ >> 64), DEC_ZZ_LO = (uint64_t)DEC_ZZ;
static_assert((DEC_ZZ_HI >> 63) == 1 && (DEC_Z_ABS >> 63) == 1, "top bits");

// The reference's endomorphism tests (Scott, eprint 2021/1130) on an affine point
// of the curve that is not infinity: G1 [z^2]P == -sigma^2(P), G2 [|z|]P ==
// -psi(P), on ec.hpp's xyzz formulas.  G2: both lanes of the pair get the
// verdict.  (k_decode_group of decode.hip and k_sig_screen of sig_verify.hip;
// the all-zero point runs through the same instructions and its verdict is
// not used.)
template <int G>
__device__ __forceinline__ bool dec_in_group(const Aff<typename DecLane<G>::LF> &p) {
  typedef typename DecLane<G>::LF LF;
  Xyzz<LF> q;
  xyzz_from_aff(q, p, false);
  LF ex, ey;  // [k]P must equal (ex, -ey), affine
  if constexpr (G == 1) {
    dec_times(q, p, DEC_ZZ_HI, DEC_ZZ_LO, 128);
    ey = p.y;
    dec_mulk(ex, p.x, DEC_BETA);
  } else {
    dec_times(q, p, 0, DEC_Z_ABS, 64);
    // psi: conjugate, then the constants (cx = cx1 i)
    const bool odd = pair_odd();
    LF cx, cy, t1, t2;
    fp_zero(cx.c);
    Fp k;
    fp_set(k, DEC_PSI_CX1);
    dec_sel(cx.c, odd, k);
    fp_set(cy.c, DEC_PSI_CY0);
    fp_set(k, DEC_PSI_CY1);
    dec_sel(cy.c, odd, k);
    fp_cneg4(t1.c, p.x.c, odd);
    fp_cneg4(t2.c, p.y.c, odd);
    f_mul(ex, t1, cx);
    f_mul(ey, t2, cy);
  }
  // q == (ex, -ey):  X == ex ZZ,  Y + ey ZZZ == 0
  LF u, v;
  f_mul_bs(u, ex, q.zz);
  f_mul_bs(v, ey, q.zzz);
  const bool eq_x = dec_eq(dec_c(q.x), dec_c(u)), eq_y = dec_sum_is_zero(dec_c(q.y), dec_c(v));
  bool ok = eq_x & eq_y;
  const bool q_inf = xyzz_is_inf(q);
  return dec_all<G>(ok) && !q_inf;
}

}  // namespace msm
