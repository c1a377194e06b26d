// fp_ops_test.hpp -- msm_test_fp_ops of the C ABI (include/msm_mi355x.h): one
// operation of fp.hpp / fp2l.hpp / ec.hpp / coop.hpp per launch on raw stored
// limbs, so that the device code runs at the range-class bounds the host proof
// covers (tests/test_gpu_fp_ops.py).  Diagnostic only: no product
// path calls it.  Host-visible part: the numbering, what each op reads and
// writes, and the two launchers (fp_ops_test.hip; the cooperative add in
// ches.hip, where coop.hpp is compiled).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace msm {

enum { TEST_FIELD_FP = 0, TEST_FIELD_FP2 = 1, TEST_FIELD_FP2L = 2 };
enum { TEST_FORM_SPLIT = 0, TEST_FORM_CHAIN = 1 };
enum {
  TEST_F_MUL = 0,
  TEST_F_MUL_BS = 1,
  TEST_F_SQR = 2,
  TEST_F_MUL_SUB = 3,
  TEST_F_MUL_SUB_BS = 4,
  TEST_F_ADD = 5,
  TEST_F_SUB4 = 6,
  TEST_F_SUB16 = 7,
  TEST_F_SUB8 = 8,
  TEST_F_SUB32 = 9,
  TEST_F_SUB_2X = 10,
  TEST_F_NEG4 = 11,
  TEST_F_MUL3 = 12,
  TEST_F_NORM = 13,
  TEST_F_NRED = 14,
  TEST_F_ONE = 15,
  TEST_F_IS_ZERO_EXACT = 16,
  TEST_F_IS_ZERO_S = 17,
  TEST_FP_MUL2 = 18,
  TEST_FP_MUL4 = 19,
  TEST_FP_RED = 20,
  TEST_FP_CNEG4 = 21,
  TEST_FP_CANON = 22,
  TEST_FP_CSUB_P = 23,
  TEST_XYZZ_MADD = 24,
  TEST_XYZZ_ADD = 25,
  TEST_XYZZ_ADD_U1S1 = 26,
  TEST_XYZZ_DBL = 27,
  TEST_COOP_ADD = 28,
  TEST_FP_OPS_COUNT = 29
};
enum { TEST_FLAG_NEG = 1, TEST_FLAG_ACC_AFFINE = 2, TEST_FLAG_ACC_NEG = 4 };

struct TestFpOp {
  int nin;      // field elements read per value
  int nout;     // field elements written per value; 0: one 32-bit word (the zero tests)
  bool fp_only;
  bool forms;   // has a MulChain form (over Fp)
  bool flags;   // reads the per-value flag word
};
// nullptr: no such op
inline const TestFpOp *test_fp_op(int op) {
  static const TestFpOp T[TEST_FP_OPS_COUNT] = {
      {2, 1, false, true, false},   // f_mul
      {2, 1, false, true, false},   // f_mul_bs
      {1, 1, false, true, false},   // f_sqr
      {4, 1, false, true, false},   // f_mul_sub
      {4, 1, false, true, false},   // f_mul_sub_bs
      {2, 1, false, false, false},  // f_add
      {2, 1, false, false, false},  // f_sub4
      {2, 1, false, false, false},  // f_sub16
      {2, 1, false, false, false},  // fp_sub<8>
      {2, 1, false, false, false},  // fp_sub<32>
      {3, 1, false, false, false},  // f_sub_2x
      {1, 1, false, false, false},  // f_neg4
      {1, 1, false, false, false},  // f_mul3
      {1, 1, false, false, false},  // f_norm
      {1, 1, false, false, false},  // f_nred
      {0, 1, false, false, false},  // f_one
      {1, 0, false, false, false},  // f_is_zero_exact
      {1, 0, false, false, false},  // f_is_zero_S
      {4, 1, true, true, false},    // fp_mul2
      {8, 1, true, true, false},    // fp_mul4
      {1, 1, true, false, false},   // fp_red
      {1, 1, true, false, true},    // fp_cneg4
      {1, 1, true, false, false},   // fp_canon
      {1, 1, true, false, false},   // fp_csub_p
      {6, 4, false, true, true},    // xyzz_madd
      {8, 4, false, true, false},   // xyzz_add
      {8, 4, false, true, false},   // xyzz_add_u1s1
      {4, 4, false, true, false},   // xyzz_dbl
      {8, 4, false, false, false},  // cooperative add (Fp, Fp2L)
  };
  return op >= 0 && op < TEST_FP_OPS_COUNT ? &T[op] : nullptr;
}
// 32-bit words of one stored element of the field kind
inline size_t test_fp_words(int field) { return field == TEST_FIELD_FP ? 14 : 28; }

// every op but the cooperative add; in: n x nin elements, out: cap >= n slots of
// nout elements (or one word), uploaded, run over the first n, downloaded whole
void test_fp_ops(int field, int form, int op, const uint32_t *in, const uint32_t *flags, uint32_t *out, size_t n,
                 size_t cap);
// the cooperative add through k_pair_step_c<1> (G = 1) / k_pair_step_c2p (G = 2):
// in: 2 n stored xyzz points, out: cap >= n
template <int G>
void test_coop_pair_add(const uint32_t *in, uint32_t *out, size_t n, size_t cap);

}  // namespace msm
