// fr_quot.hpp -- the per-element steps of msm_fr_eval_quotient (fr_poly.hip) on
// fr.hpp: a polynomial f given by its values f_i on the domain x_i = omega_n^i is
// evaluated at z and divided by (X - z) without leaving the evaluation form.
// Compiles for the host under MSM_FP_HOST_TEST (tests/test_kzg_host.py), with the
// range checks of fp.hpp armed, like fr_elem.
//
// With d_i = 1 / (z - x_i) (0 where z = x_i), S = sum f_i x_i d_i, T = sum x_i d_i:
//   z outside the domain:  y = (z^n - 1) n^-1 S,  q_i = (y - f_i) d_i
//   z = x_m:               y = f_m,  q_i as above for i != m,  q_m = z^-1 (S - y T)
// (the zero d_m drops term m out of both sums).
//
// Forms.  The 2^261 Montgomery form of fr.hpp reads a blst_fr a as
// a / 32, so f, y and q travel as "value / 32", which is invisible to the sums.  z is
// lifted once to its exact value (fq_point), the domain points come exact from the
// power tables, and so the d_i are exact.  Under MSM_FR_DST_SCALAR the inverse of
// a workgroup's product is multiplied by 2^-256 once, which every d_i inherits: the
// product (y - f_i) d_i then IS the blst_scalar of q_i, and fq_finish undoes the
// factor on the two sums.
//
// Classes: every Fr that leaves a function here is class S or canonical; the lazy
// values (fr_sub4, fr_add) live inside one function and enter a product as its first
// operand or fr_nred at once, as fr.hpp allows.
#pragma once
#include "fr.hpp"

namespace msm {

MSM_FN bool fr_eq_exact(const Fr &a, const Fr &b) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < FR_NL; ++i) o |= a.v[i] ^ b.v[i];
  return o == 0;
}

// the blst_fr z -> its exact value, canonical
MSM_FN void fq_point(Fr &zt, const Fr &z) {
  fr_mulc(zt, z, FR_C266);
  fr_csub(zt);
}

// u = z - x (class S); where z = x, u = 1 and true.  zt, x canonical.
MSM_FN bool fq_diff(Fr &u, const Fr &zt, const Fr &x) {
  const bool zero = fr_eq_exact(zt, x);
  Fr one;
  fr_one(one);
  fr_sub4(u, zt, x);
  fr_nred(u);
  fr_sel(u, zero, one);
  return zero;
}

// a^-1 (Fermat, r - 2 a word at a time); a class S, nonzero -> class S
MSM_FN void fq_inv(Fr &r, const Fr &a) {
  fr_one(r);
#pragma unroll 1
  for (int w = 3; w >= 0; --w) {
    const uint64_t word = w == 3   ? 0x73eda753299d7d48ull
                          : w == 2 ? 0x3339d80809a1d805ull
                          : w == 1 ? 0x53bda402fffe5bfeull
                                   : 0xfffffffeffffffffull;
#pragma unroll 1
    for (int i = 63; i >= 0; --i) {
      fr_mul(r, r, r);
      if ((word >> i) & 1) fr_mul(r, r, a);
    }
  }
}

// S += f x d and T += x d with x = z - u; S, T, u class S, d and f canonical.  A
// zero d (z = x, or a lane past the tile) adds nothing whatever u holds.
MSM_FN void fq_term(Fr &S, Fr &T, const Fr &zt, const Fr &u, const Fr &d, const Fr &f) {
  Fr x, a;
  fr_sub4(x, zt, u);  // lazy
  fr_mul(a, x, d);
  fr_add(T, T, a);
  fr_nred(T);
  fr_mul(a, a, f);
  fr_add(S, S, a);
  fr_nred(S);
}

// a + b of two class S sums -> class S
MSM_FN void fq_sum(Fr &a, const Fr &b) {
  fr_add(a, a, b);
  fr_nred(a);
}

// One polynomial's y (a blst_fr) and q_m (a blst_fr, or a blst_scalar with `scalar`;
// zero when z is outside the domain) from its sums.  zt canonical; S, T class S; fm
// the blst_fr f_m, read only when z^n = 1; ninv the constant 1 / n.
MSM_FN void fq_finish(Fr &y, Fr &qm, const Fr &zt, Fr S, Fr T, const Fr &fm, const Fr &ninv, int log_n, bool scalar) {
  if (scalar) {  // the sums carry the 2^-256 of the d_i
    fr_mulc(S, S, FR_K517);
    fr_mulc(T, T, FR_K517);
  }
  Fr zn = zt, one;
  for (int i = 0; i < log_n; ++i) fr_sqr(zn, zn);
  fr_csub(zn);
  fr_one(one);
  if (!fr_eq_exact(zn, one)) {
    Fr w;
    fr_sub4(w, zn, one);
    fr_mul(w, w, ninv);
    fr_mul(y, w, S);
    fr_csub(y);
    fr_zero(qm);
  } else {
    Fr t, zi;
    y = fm;
    fr_mul(t, T, y);
    fr_sub4(t, S, t);
    fq_inv(zi, zt);
    fr_mul(qm, t, zi);
    if (scalar) fr_mulc(qm, qm, FR_C32);
    fr_csub(qm);
  }
}

// q_i = (y - f_i) d_i, or q_m where d_i is zero.  y, f, d, qm canonical.
MSM_FN void fq_quot(Fr &q, const Fr &y, const Fr &f, const Fr &d, const Fr &qm) {
  const bool m = fr_is_zero_exact(d);
  fr_sub4(q, y, f);
  fr_mul(q, q, d);
  fr_csub(q);
  fr_sel(q, m, qm);
}

}  // namespace msm
