// first_pair_shim.cpp -- host (g++) run of a bucket's first two entries as the
// accumulation kernels run them (kernels.hpp accumulate_bucket, pair_kernels.hpp
// accumulate_pair): xyzz_from_aff of the first row, then xyzz_madd of the second
// with acc_affine set (ec.hpp: the four products by ZZ1 = ZZZ1 = 1 skipped) or
// clear (the generic formula, the comparison).  Every range check of fp.hpp is
// enabled as in fp_host_shim.cpp, whose loaders and lane-pair harness this file
// reuses.  TEST INFRASTRUCTURE ONLY: loaded by tests/test_first_pair_bounds.py.
#include "fp_host_shim.cpp"

// rows: 2 affine points (x | y each); out: xyzz (x | y | zzz | zz)
template <class F>
static void first_pair_io(uint32_t *out, const uint32_t *rows, int neg1, int neg2, int affine) {
  Aff<F> p1, p2;
  memcpy(&p1, rows, sizeof p1);
  memcpy(&p2, rows + sizeof(p1) / 4, sizeof p2);
  Xyzz<F> A;
  xyzz_set_inf(A);
  xyzz_madd(A, p1, neg1 != 0);  // infinity: xyzz_from_aff
  xyzz_madd(A, p2, neg2 != 0, affine != 0);
  memcpy(out, &A, sizeof A);
}

// group 1: Fp, 2: Fp2 on one lane, 3: Fp2 on a lane pair (fp2l.hpp)
extern "C" void h_first_pair(int group, uint32_t *out, const uint32_t *rows, int neg1, int neg2, int affine) {
  if (group == 1) {
    first_pair_io<Fp>(out, rows, neg1, neg2, affine);
  } else if (group == 2) {
    first_pair_io<Fp2>(out, rows, neg1, neg2, affine);
  } else {
    pair_run([&](int lane) {
      Aff<Fp2L> p1, p2;
      ldl(&p1.x, rows, 1, lane);
      ldl(&p1.y, rows + 2 * NL, 1, lane);
      ldl(&p2.x, rows + 4 * NL, 1, lane);
      ldl(&p2.y, rows + 6 * NL, 1, lane);
      Xyzz<Fp2L> A;
      xyzz_set_inf(A);
      xyzz_madd(A, p1, neg1 != 0);
      xyzz_madd(A, p2, neg2 != 0, affine != 0);
      stl(out, &A.x, 1, lane);
      stl(out + 2 * NL, &A.y, 1, lane);
      stl(out + 4 * NL, &A.zzz, 1, lane);
      stl(out + 6 * NL, &A.zz, 1, lane);
    });
  }
}
