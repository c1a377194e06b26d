// fp12_host_shim.cpp -- host (g++) build of the Fp12 tower and the Miller loop's
// line functions (msm_blst_amd/csrc/fp12l.hpp, on fp2l.hpp / fp2l_mem.hpp) with
// every range check of fp.hpp enabled, as in fp_host_shim.cpp, whose loaders
// and two-thread lane-pair harness this file reuses: lane 0 holds and touches
// component c0 of every Fp2 of a stored value, lane 1 component c1.  The same
// header text is compiled for gfx950 in the product.  TEST INFRASTRUCTURE ONLY:
// loaded by tests/test_fp12_bounds.py.
#define __constant__  // pairing_consts.hpp: the Frobenius table is plain host data here
#include "fp_host_shim.cpp"

#include "../../msm_blst_amd/csrc/fp12l.hpp"

// One operation on stored values (Fp12S: six Fp2, c0 | c1 each, 168 words).
// op as msm_test_fp12 of the C ABI: 0 mul, 1 sqr, 2 sparse (x, y, z = coefficients
// 0, 1, 4 of b), 3 conj, 4 Frobenius k, 5 inverse, 6 k cyclotomic squarings held in
// registers, 7 / 8 the doubling / addition line: a = (X, Y, Z, qx, qy, unused),
// out = (X3, Y3, Z3, l0, l1, l2).  alias 1: the destination is a, 2: it is b.
extern "C" int h_fp12_op(int op, int k, int alias, uint32_t *out, const uint32_t *a, const uint32_t *b) {
  Fp12S A, B, D;
  memcpy(&A, a, sizeof A);
  if (b) memcpy(&B, b, sizeof B);
  memset(&D, 0xff, sizeof D);  // a destination of its own starts out of every class
  Fp12S *d = alias == 1 ? &A : alias == 2 ? &B : &D;
  if (op < 0 || op > 8 || ((op == 0 || op == 2) && !b)) return -1;
  pair_run([&](int comp) {
    switch (op) {
      case 0: t_mul12(d, &A, &B, comp); break;
      case 1: t_sqr12(d, &A, comp); break;
      case 2: {
        Fp2L x, y, z;
        ld_comp(x.c, &B.c[0], comp);
        ld_comp(y.c, &B.c[1], comp);
        ld_comp(z.c, &B.c[4], comp);
        t_mul12_sparse(d, &A, x, y, z, comp);
        break;
      }
      case 3: t_conj12(d, &A, comp); break;
      case 4: t_frob12(d, &A, k, comp); break;
      case 5: t_inv12(d, &A, comp); break;
      case 6: {
        F12L v;
        t_ld12(v, &A, comp);
        for (int i = 0; i < k; ++i) t_cyc_sqr12(v);
        t_st12(d, v, comp);
        break;
      }
      default: {
        Fp2L X, Y, Z, l0, l1, l2;
        ld_comp(X.c, &A.c[0], comp);
        ld_comp(Y.c, &A.c[1], comp);
        ld_comp(Z.c, &A.c[2], comp);
        if (op == 8) {
          Fp2L qx, qy;
          ld_comp(qx.c, &A.c[3], comp);
          ld_comp(qy.c, &A.c[4], comp);
          pair_line_add(X, Y, Z, qx, qy, l0, l1, l2);
        } else {
          pair_line_dbl(X, Y, Z, l0, l1, l2);
        }
        st_comp(&d->c[0], X.c, comp);
        st_comp(&d->c[1], Y.c, comp);
        st_comp(&d->c[2], Z.c, comp);
        st_comp(&d->c[3], l0.c, comp);
        st_comp(&d->c[4], l1.c, comp);
        st_comp(&d->c[5], l2.c, comp);
        break;
      }
    }
  });
  memcpy(out, d, sizeof D);
  return 0;
}

// The Fp2 primitives of the tower on one value each (c0 | c1, 28 words): 0 t_add,
// 1 t_sub, 2 t_dbl, 3 t_neg, 4 t_conj, 5 t_xi, 6 t_mul, 7 t_sqr, 8 f_inv, and
// 9 t_scale by the Fp value at b (the same in both lanes)
extern "C" void h_tower_fp2(int op, uint32_t *r, const uint32_t *a, const uint32_t *b) {
  pair_run([&](int lane) {
    Fp2L A, B, R;
    ldl(&A, a, 1, lane);
    if (b && op != 9) ldl(&B, b, 1, lane);
    switch (op) {
      case 0: t_add(R, A, B); break;
      case 1: t_sub(R, A, B); break;
      case 2: t_dbl(R, A); break;
      case 3: t_neg(R, A); break;
      case 4: t_conj(R, A); break;
      case 5: t_xi(R, A); break;
      case 6: t_mul(R, A, B); break;
      case 7: t_sqr(R, A); break;
      case 8: f_inv(R, A); break;
      default: t_scale(R, A, ld(b)); break;
    }
    stl(r, &R, 1, lane);
  });
}
