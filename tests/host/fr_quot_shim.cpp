// fr_quot_shim.cpp -- host (g++) build of the per-element header of
// msm_fr_eval_quotient (msm_blst_amd/csrc/fr_quot.hpp on fr.hpp) with every range
// check enabled (MSM_FP_HOST_TEST: a wrapping column, a wrapping or negative limb or a
// negative reduced value sets msm_fp_overflow).  h_fq_poly runs one whole polynomial
// through the steps in the order of the kernels (fr_poly.hip): the differences and
// their running product, ONE inversion, the way back down with the two sums, the
// finish, the quotient.  TEST INFRASTRUCTURE ONLY: loaded by tests/test_kzg_host.py
// through ctypes; the same header text is compiled for gfx950 in the product.
#define MSM_FP_HOST_TEST 1
#include <string.h>

#include <vector>

#include "../../msm_blst_amd/csrc/fr_quot.hpp"
#include "../../msm_blst_amd/csrc/host_fr.hpp"

extern "C" {
int msm_fp_overflow = 0;

using namespace msm;

int h_fq_overflow(int clear) {
  int v = msm_fp_overflow;
  if (clear) msm_fp_overflow = 0;
  return v;
}

static Fr rest(const uint8_t *p) {  // 32 bytes at rest -> limbs
  uint32_t w[8];
  memcpy(w, p, 32);
  Fr r;
  fr_unpack(r, w);
  return r;
}
static void to_rest(uint8_t *p, const Fr &a) {
  uint32_t w[8];
  fr_pack(w, a);
  memcpy(p, w, 32);
}
// the constant x 2^261 mod r of the blst_fr x (what the power tables hold)
static Fr constant(const uint8_t *p) {
  hfr::Fr x;
  memcpy(&x, p, 32);
  const hfr::Fr v = hfr::mul(x, hfr::from_u64(32));
  return rest(reinterpret_cast<const uint8_t *>(&v));
}

// f, x: n blst_fr (the values and the domain points, in the same order); z, ninv: one
// blst_fr each -> y (blst_fr) and q (n elements; blst_scalar bytes with `scalar`)
void h_fq_poly(uint8_t *y, uint8_t *q, const uint8_t *f, const uint8_t *x, const uint8_t *z, const uint8_t *ninv,
               size_t n, int log_n, int scalar) {
  Fr zt;
  fq_point(zt, rest(z));
  std::vector<Fr> u(n), p(n), d(n);
  std::vector<char> zf(n);
  for (size_t i = 0; i < n; ++i) {
    zf[i] = fq_diff(u[i], zt, constant(x + 32 * i));
    if (i == 0) p[0] = u[0];
    else fr_mul(p[i], p[i - 1], u[i]);
  }
  Fr I, S, T, fm, zero;
  fq_inv(I, p[n - 1]);
  if (scalar) fr_mulc(I, I, FR_C32);
  fr_zero(S);
  fr_zero(T);
  fr_zero(fm);
  fr_zero(zero);
  for (size_t i = n; i-- > 0;) {
    if (i > 0) {
      fr_mul(d[i], I, p[i - 1]);
      fr_mul(I, I, u[i]);
    } else {
      d[i] = I;
    }
    fr_csub(d[i]);
    fr_sel(d[i], zf[i] != 0, zero);
    const Fr fi = rest(f + 32 * i);
    if (zf[i]) fm = fi;
    fq_term(S, T, zt, u[i], d[i], fi);
  }
  Fr yy, qm;
  fq_finish(yy, qm, zt, S, T, fm, constant(ninv), log_n, scalar != 0);
  to_rest(y, yy);
  for (size_t i = 0; i < n; ++i) {
    Fr r;
    fq_quot(r, yy, rest(f + 32 * i), d[i], qm);
    to_rest(q + 32 * i, r);
  }
}
}
