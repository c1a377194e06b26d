// single_chain_shim.cpp -- host (g++) build of fp.hpp / ec.hpp with every range
// check enabled (MSM_FP_HOST_TEST), exposing each Montgomery product and the G1
// xyzz formulas in both column forms: form 0 = MulSplit (the untagged functions),
// form 1 = MulChain (single-chain columns).  TEST INFRASTRUCTURE ONLY: loaded by
// tests/test_single_chain_host.py through ctypes.
#define MSM_FP_HOST_TEST 1
#include <string.h>

#include "../../msm_blst_amd/csrc/ec.hpp"

extern "C" {
int msm_fp_overflow = 0;
}
using namespace msm;

static Fp ld(const uint32_t *p) {
  Fp r;
  memcpy(r.v, p, sizeof r.v);
  return r;
}

template <class CF>
static void fp_op(int op, Fp &R, const uint32_t *const *x) {
  switch (op) {
    case 0: fp_mul(R, ld(x[0]), ld(x[1]), CF{}); break;
    case 1: fp_sqr(R, ld(x[0]), CF{}); break;
    case 2: fp_mul2(R, ld(x[0]), ld(x[1]), ld(x[2]), ld(x[3]), CF{}); break;
    case 3: fp_mul4(R, ld(x[0]), ld(x[1]), ld(x[2]), ld(x[3]), ld(x[4]), ld(x[5]), ld(x[6]), ld(x[7]), CF{}); break;
    case 4: f_mul_sub(R, ld(x[0]), ld(x[1]), ld(x[2]), ld(x[3]), CF{}); break;
  }
}
// op 0: madd (other = affine row, flags bit 0 = neg, bit 1 = acc_affine), 1: add, 2: dbl
template <class CF>
static void xyzz_op(int op, Xyzz<Fp> &A, const uint32_t *other, int flags) {
  if (op == 0) {
    Aff<Fp> p;
    memcpy(&p, other, sizeof p);
    xyzz_madd<Fp, CF>(A, p, (flags & 1) != 0, (flags & 2) != 0);
  } else if (op == 1) {
    Xyzz<Fp> B;
    memcpy(&B, other, sizeof B);
    xyzz_add<Fp, true, CF>(A, B);
  } else {
    Xyzz<Fp> B = A;
    xyzz_dbl<Fp, CF>(A, B);
  }
}

extern "C" {
int h_overflow(int clear) {
  int v = msm_fp_overflow;
  if (clear) msm_fp_overflow = 0;
  return v;
}
// x: 8 operand pointers (unused ones null)
void h_sc_fp(int form, int op, uint32_t *r, const uint32_t *const *x) {
  Fp R;
  if (form) fp_op<MulChain>(op, R, x);
  else fp_op<MulSplit>(op, R, x);
  memcpy(r, R.v, sizeof R.v);
}
// acc: xyzz (x | y | zzz | zz), in place
void h_sc_xyzz(int form, int op, uint32_t *acc, const uint32_t *other, int flags) {
  Xyzz<Fp> A;
  memcpy(&A, acc, sizeof A);
  if (form) xyzz_op<MulChain>(op, A, other, flags);
  else xyzz_op<MulSplit>(op, A, other, flags);
  memcpy(acc, &A, sizeof A);
}
}
