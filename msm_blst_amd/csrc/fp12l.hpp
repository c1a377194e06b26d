// fp12l.hpp -- the Fp6 / Fp12 tower of BLS12-381 on lane pairs (device code;
// replaces the reference's src/fp12_tower.c for the bulk pairings):
//   Fp6 = Fp2[v] / (v^3 - xi),  Fp12 = Fp6[w] / (w^2 - v),  xi = 1 + u,
// over the lane-pair Fp2L of fp2l.hpp: the even lane of a pair holds the real
// parts of all six Fp2 coefficients of a value, the odd lane the imaginary
// parts (84 registers per lane and value).
//
// An Fp12 value at rest is an Fp12S: six stored Fp2 in blst's order
// (a00, a01, a02, a10, a11, a12), internal limbs, 672 bytes.  A lane reads and
// writes only its own component of a stored value; the partner's component
// reaches it through the DPP swaps inside the Fp2L products.  So the Fp12
// operations below work from memory to memory (every load before the first
// store: the destination may be an operand), reload an operand rather than keep
// it in registers across an Fp6 product, and need no barrier.
//
// Ranges: every value between products is kept in class S;
// t_add / t_sub reduce after each sum as h_add / h_sub of hash_to_curve.hip do,
// so no lazy-range bookkeeping is needed and the proven bounds carry over: the
// rows "Fp12 tower" of DESIGN.md 21 (tests/fp_bounds.py prove_tower) prove it,
// and tests/host/fp12_host_shim.cpp runs this header's text on the host with
// every range check armed (MSM_FP_HOST_TEST; tests/test_fp12_bounds.py).
#pragma once
#ifdef MSM_FP_HOST_TEST
#include "fp2l_mem.hpp"
#else
#include "pair_kernels.hpp"
#endif
#include "pairing_consts.hpp"

namespace msm {

struct Fp12S {
  Fp2 c[6];
};
struct F6L {
  Fp2L c[3];
};
struct F12L {
  Fp2L c[6];
};

// ------------------------------------------------------------------ Fp2 ----
MSM_FN void t_add(Fp2L &r, const Fp2L &a, const Fp2L &b) {
  f_add(r, a, b);
  f_nred(r);
}
MSM_FN void t_sub(Fp2L &r, const Fp2L &a, const Fp2L &b) {
  f_sub4(r, a, b);
  f_nred(r);
}
MSM_FN void t_dbl(Fp2L &r, const Fp2L &a) { t_add(r, a, a); }
// Every Fp2 product is a scheduling region of its own: with 512 registers to
// spend (one wave per SIMD) the scheduler otherwise interleaves the independent
// products of a Karatsuba step and moves loads far ahead, and the kernels that
// hold whole Fp12 values spill (tests/test_kernel_resources.py).
#ifdef MSM_FP_HOST_TEST
MSM_FN void t_fence() {}
#else
MSM_FN void t_fence() { __builtin_amdgcn_sched_barrier(0); }
#endif
MSM_FN void t_mul(Fp2L &r, const Fp2L &a, const Fp2L &b) {
  f_mul_bs(r, a, b);
  t_fence();
}
MSM_FN void t_sqr(Fp2L &r, const Fp2L &a) {
  f_sqr(r, a);
  t_fence();
}
MSM_FN void t_neg(Fp2L &r, const Fp2L &a) {
  f_neg4(r, a);
  f_nred(r);
}
// conj(a): the imaginary part negated
MSM_FN void t_conj(Fp2L &r, const Fp2L &a) {
  fp_cneg4(r.c, a.c, pair_odd());
  f_nred(r);
}
// a (1 + u) = (a0 - a1) + (a0 + a1) u
MSM_FN void t_xi(Fp2L &r, const Fp2L &a) {
  Fp par, s, d;
  pair_swap(par, a.c);
  fp_add(s, a.c, par);      // odd: a1 + a0
  fp_sub<4>(d, a.c, par);   // even: a0 + 4p - a1
  pair_sel(r.c, pair_odd(), s, d);
  f_nred(r);
}
// a k for k in Fp (the same value in both lanes)
MSM_FN void t_scale(Fp2L &r, const Fp2L &a, const Fp &k) { fp_mul(r.c, a.c, k); }
MSM_FN void t_const(Fp2L &r, const uint32_t (*k)[NL]) {
  Fp c0, c1;
  fp_set(c0, k[0]);
  fp_set(c1, k[1]);
  pair_sel(r.c, pair_odd(), c1, c0);
}
MSM_FN void t_sel(Fp2L &r, bool c, const Fp2L &a) {  // r = c ? a : r, c uniform over a pair
#pragma unroll
  for (int i = 0; i < NL; ++i) r.c.v[i] = c ? a.c.v[i] : r.c.v[i];
}

// ------------------------------------------------------------------ Fp6 ----
MSM_FN void t_ld6(F6L &r, const Fp2 *p, int comp) {
#pragma unroll
  for (int j = 0; j < 3; ++j) ld_comp(r.c[j].c, p + j, comp);
}
MSM_FN void t_st6(Fp2 *p, const F6L &a, int comp) {
#pragma unroll
  for (int j = 0; j < 3; ++j) st_comp(p + j, a.c[j].c, comp);
}
MSM_FN void t_add6(F6L &r, const F6L &a, const F6L &b) {
#pragma unroll
  for (int j = 0; j < 3; ++j) t_add(r.c[j], a.c[j], b.c[j]);
}
MSM_FN void t_sub6(F6L &r, const F6L &a, const F6L &b) {
#pragma unroll
  for (int j = 0; j < 3; ++j) t_sub(r.c[j], a.c[j], b.c[j]);
}
MSM_FN void t_neg6(F6L &r, const F6L &a) {
#pragma unroll
  for (int j = 0; j < 3; ++j) t_neg(r.c[j], a.c[j]);
}
// a v = xi a2 + a0 v + a1 v^2
MSM_FN void t_mulv6(F6L &r, const F6L &a) {
  Fp2L t;
  t_xi(t, a.c[2]);
  r.c[2] = a.c[1];
  r.c[1] = a.c[0];
  r.c[0] = t;
}
// Karatsuba: six Fp2 products.  r is neither a nor b.
MSM_FN void t_mul6(F6L &r, const F6L &a, const F6L &b) {
  Fp2L t0, t1, t2, s, u, m;
  t_mul(t0, a.c[0], b.c[0]);
  t_mul(t1, a.c[1], b.c[1]);
  t_mul(t2, a.c[2], b.c[2]);
  t_add(s, a.c[1], a.c[2]);
  t_add(u, b.c[1], b.c[2]);
  t_mul(m, s, u);
  t_sub(m, m, t1);
  t_sub(m, m, t2);
  t_xi(m, m);
  t_add(r.c[0], m, t0);  // (a1 b2 + a2 b1) xi + a0 b0
  t_add(s, a.c[0], a.c[1]);
  t_add(u, b.c[0], b.c[1]);
  t_mul(m, s, u);
  t_sub(m, m, t0);
  t_sub(m, m, t1);
  t_xi(s, t2);
  t_add(r.c[1], m, s);  // a0 b1 + a1 b0 + a2 b2 xi
  t_add(s, a.c[0], a.c[2]);
  t_add(u, b.c[0], b.c[2]);
  t_mul(m, s, u);
  t_sub(m, m, t0);
  t_sub(m, m, t2);
  t_add(r.c[2], m, t1);  // a0 b2 + a2 b0 + a1 b1
}
// a (x + y v): five products.  r is not a.
MSM_FN void t_mul6_xy0(F6L &r, const F6L &a, const Fp2L &x, const Fp2L &y) {
  Fp2L m0, m1, m, s, u;
  t_mul(m0, a.c[0], x);
  t_mul(m1, a.c[1], y);
  t_mul(m, a.c[2], y);
  t_xi(m, m);
  t_add(r.c[0], m, m0);  // a0 x + a2 y xi
  t_add(s, a.c[0], a.c[1]);
  t_add(u, x, y);
  t_mul(m, s, u);
  t_sub(m, m, m0);
  t_sub(r.c[1], m, m1);  // a0 y + a1 x
  t_mul(m, a.c[2], x);
  t_add(r.c[2], m, m1);  // a2 x + a1 y
}
// a (z v): three products.  r is not a.
MSM_FN void t_mul6_0y0(F6L &r, const F6L &a, const Fp2L &z) {
  t_mul(r.c[0], a.c[2], z);
  t_xi(r.c[0], r.c[0]);
  t_mul(r.c[1], a.c[0], z);
  t_mul(r.c[2], a.c[1], z);
}
// the cofactors c of a and its norm n to Fp2: 1 / a = c / n
MSM_FN void t_cof6(F6L &c, Fp2L &n, const F6L &a) {
  Fp2L t, s;
  t_sqr(c.c[0], a.c[0]);
  t_mul(t, a.c[1], a.c[2]);
  t_xi(t, t);
  t_sub(c.c[0], c.c[0], t);  // a0^2 - a1 a2 xi
  t_sqr(c.c[1], a.c[2]);
  t_xi(c.c[1], c.c[1]);
  t_mul(t, a.c[0], a.c[1]);
  t_sub(c.c[1], c.c[1], t);  // a2^2 xi - a0 a1
  t_sqr(c.c[2], a.c[1]);
  t_mul(t, a.c[0], a.c[2]);
  t_sub(c.c[2], c.c[2], t);  // a1^2 - a0 a2
  t_mul(t, c.c[1], a.c[2]);
  t_mul(s, c.c[2], a.c[1]);
  t_add(t, t, s);
  t_xi(t, t);
  t_mul(s, c.c[0], a.c[0]);
  t_add(n, t, s);  // (a2 c1 + a1 c2) xi + a0 c0
}

// ----------------------------------------------------------------- Fp12 ----
MSM_FN void t_ld12(F12L &r, const Fp12S *p, int comp) {
#pragma unroll
  for (int j = 0; j < 6; ++j) ld_comp(r.c[j].c, &p->c[j], comp);
}
MSM_FN void t_st12(Fp12S *p, const F12L &a, int comp) {
#pragma unroll
  for (int j = 0; j < 6; ++j) st_comp(&p->c[j], a.c[j].c, comp);
}
MSM_FN void t_one12(Fp12S *p, int comp) {
  Fp2L one, zero;
  f_one(one);
  f_zero(zero);
  st_comp(&p->c[0], one.c, comp);
#pragma unroll
  for (int j = 1; j < 6; ++j) st_comp(&p->c[j], zero.c, comp);
}
// the low half c0 = t0 + t1 v of a product whose Fp6 parts are t0 = a0 b0, t1 = a1 b1
MSM_FN void t_low12(F6L &r, const F6L &t0, const F6L &t1) {
  F6L w;
  t_mulv6(w, t1);
  t_add6(r, t0, w);
}
// The compiler may not carry a loaded value across this point: what is needed
// again is loaded again, which is cheaper than the registers it would hold.
MSM_FN void t_reload() { asm volatile("" ::: "memory"); }
// d = a b: Karatsuba over Fp6, 18 Fp2 products
MSM_FN void t_mul12(Fp12S *d, const Fp12S *a, const Fp12S *b, int comp) {
  F6L x, y, t0, t1, t2;
  t_ld6(x, a->c, comp);
  t_ld6(y, b->c, comp);
  t_mul6(t0, x, y);
  t_ld6(x, a->c + 3, comp);
  t_ld6(y, b->c + 3, comp);
  t_mul6(t1, x, y);
  t_reload();
  t_ld6(t2, a->c, comp);
  t_add6(x, x, t2);
  t_ld6(t2, b->c, comp);
  t_add6(y, y, t2);
  t_mul6(t2, x, y);
  t_sub6(t2, t2, t0);
  t_sub6(t2, t2, t1);  // a0 b1 + a1 b0
  t_low12(x, t0, t1);
  t_st6(d->c, x, comp);
  t_st6(d->c + 3, t2, comp);
}
// d = a^2: (a0 + a1)(a0 + a1 v) - a0 a1 - a0 a1 v and 2 a0 a1, 12 Fp2 products
MSM_FN void t_sqr12(Fp12S *d, const Fp12S *a, int comp) {
  F6L a0, a1, t0, t1;
  t_ld6(a0, a->c, comp);
  t_ld6(a1, a->c + 3, comp);
  {
    F6L s, w;
    t_add6(s, a0, a1);
    t_mulv6(w, a1);
    t_add6(w, a0, w);
    t_mul6(t0, s, w);
  }
  t_reload();
  t_ld6(a0, a->c, comp);
  t_ld6(a1, a->c + 3, comp);
  t_mul6(t1, a0, a1);
  t_sub6(t0, t0, t1);
  t_mulv6(a0, t1);
  t_sub6(t0, t0, a0);
  t_add6(t1, t1, t1);
  t_st6(d->c, t0, comp);
  t_st6(d->c + 3, t1, comp);
}
// d = a (x + y v + z v w): the sparse form of a line, 13 Fp2 products
MSM_FN void t_mul12_sparse(Fp12S *d, const Fp12S *a, const Fp2L &x, const Fp2L &y, const Fp2L &z, int comp) {
  F6L a0, a1, t0, t1, t2;
  Fp2L yz;
  t_ld6(a0, a->c, comp);
  t_ld6(a1, a->c + 3, comp);
  t_mul6_xy0(t0, a0, x, y);
  t_mul6_0y0(t1, a1, z);
  t_add6(a0, a0, a1);
  t_add(yz, y, z);
  t_mul6_xy0(t2, a0, x, yz);
  t_sub6(t2, t2, t0);
  t_sub6(t2, t2, t1);
  t_low12(a0, t0, t1);
  t_st6(d->c, a0, comp);
  t_st6(d->c + 3, t2, comp);
}
// d = conj(a) = a0 - a1 w
MSM_FN void t_conj12(Fp12S *d, const Fp12S *a, int comp) {
  F6L a0, a1;
  t_ld6(a0, a->c, comp);
  t_ld6(a1, a->c + 3, comp);
  t_neg6(a1, a1);
  t_st6(d->c, a0, comp);
  t_st6(d->c + 3, a1, comp);
}
// d = a^(p^k), k = 1 .. 3: coefficient j conjugated k times, times PAIR_FROB[6 (k - 1) + j]
MSM_FN void t_frob12(Fp12S *d, const Fp12S *a, int k, int comp) {
#pragma unroll 1
  for (int j = 0; j < 6; ++j) {
    Fp2L c, g;
    ld_comp(c.c, &a->c[j], comp);
    fp_cneg4(c.c, c.c, (k & 1) != 0 && pair_odd());
    f_nred(c);
    t_const(g, PAIR_FROB[6 * (k - 1) + j]);
    t_mul(c, c, g);
    st_comp(&d->c[j], c.c, comp);
  }
}
// d = 1 / a: the norm to Fp6, its norm to Fp2, and one Fp2 inversion (itself one Fp
// inversion, f_inv).  d is not a: it parks the cofactors, so that nothing but the
// norm is live across the Fermat chain.
MSM_FN void t_inv12(Fp12S *d, const Fp12S *a, int comp) {
  Fp2L n, s;
  {
    F6L a0, t0, t1;
    t_ld6(a0, a->c, comp);
    t_mul6(t0, a0, a0);
    t_ld6(a0, a->c + 3, comp);
    t_mul6(t1, a0, a0);
    t_mulv6(t1, t1);
    t_sub6(t0, t0, t1);  // a0^2 - a1^2 v
    t_cof6(t1, n, t0);
    t_st6(d->c, t1, comp);
  }
  t_reload();
  f_inv(s, n);
  t_fence();
  t_reload();
  F6L r, x, y;
  t_ld6(x, d->c, comp);
  t_mul(r.c[0], x.c[0], s);  // 1 / (a0^2 - a1^2 v)
  t_mul(r.c[1], x.c[1], s);
  t_mul(r.c[2], x.c[2], s);
  t_ld6(x, a->c, comp);
  t_mul6(y, x, r);
  t_st6(d->c, y, comp);
  t_reload();
  t_ld6(x, a->c + 3, comp);
  t_mul6(y, x, r);
  t_neg6(y, y);
  t_st6(d->c + 3, y, comp);
}
// (a + b s)^2 in Fp4 = Fp2[s] / (s^2 - xi): r0 = a^2 + b^2 xi, r1 = 2 a b
MSM_FN void t_sqr4(Fp2L &r0, Fp2L &r1, const Fp2L &a, const Fp2L &b) {
  Fp2L t0, t1, s;
  t_sqr(t0, a);
  t_sqr(t1, b);
  t_add(s, a, b);
  t_sqr(s, s);
  t_sub(s, s, t0);
  t_sub(r1, s, t1);
  t_xi(t1, t1);
  t_add(r0, t1, t0);
}
// 3 t - 2 c and 3 t + 2 c
MSM_FN void t_cyc_lo(Fp2L &c, const Fp2L &t) {
  Fp2L d;
  t_sub(d, t, c);
  t_dbl(d, d);
  t_add(c, d, t);
}
MSM_FN void t_cyc_hi(Fp2L &c, const Fp2L &t) {
  Fp2L d;
  t_add(d, t, c);
  t_dbl(d, d);
  t_add(c, d, t);
}
// a = a^2 for a in the cyclotomic subgroup (Granger-Scott: three squarings in Fp4, 9 Fp2 squarings)
MSM_FN void t_cyc_sqr12(F12L &a) {
  Fp2L t00, t01, t10, t11, t20, t21;
  t_sqr4(t00, t01, a.c[0], a.c[4]);
  t_sqr4(t10, t11, a.c[3], a.c[2]);
  t_sqr4(t20, t21, a.c[1], a.c[5]);
  t_cyc_lo(a.c[0], t00);
  t_cyc_lo(a.c[1], t10);
  t_cyc_lo(a.c[2], t20);
  t_xi(t21, t21);
  t_cyc_hi(a.c[3], t21);
  t_cyc_hi(a.c[4], t01);
  t_cyc_hi(a.c[5], t11);
}

// ---------------------------------------------------------------- lines ----
// The Miller loop's two steps (pairing.hip k_pair_miller): the Jacobian doubling
// dbl-2009-alnr and the mixed addition madd-2007-bl with the lines of eprint
// 2010/354, before the factors -2 x_P and 2 y_P.  T and Q in S; everything
// that comes out is in S.
// T = 2 T and the line through T: l0 = 6 X^3 - 4 Y^2, l1 = 3 X^2 Z^2, l2 = Z3 Z^2
MSM_FN void pair_line_dbl(Fp2L &X, Fp2L &Y, Fp2L &Z, Fp2L &l0, Fp2L &l1, Fp2L &l2) {
  Fp2L A, B, ZZ, C, D, E, F, X3, Z3, t;
  t_sqr(A, X);
  t_sqr(B, Y);
  t_sqr(ZZ, Z);
  t_sqr(C, B);
  t_add(D, X, B);
  t_sqr(D, D);
  t_sub(D, D, A);
  t_sub(D, D, C);
  t_dbl(D, D);  // 2 ((X + B)^2 - A - C)
  t_dbl(E, A);
  t_add(E, E, A);  // 3 A
  t_sqr(F, E);
  t_sub(X3, F, D);
  t_sub(X3, X3, D);
  t_add(Z3, Y, Z);
  t_sqr(Z3, Z3);
  t_sub(Z3, Z3, B);
  t_sub(Z3, Z3, ZZ);
  t_add(l0, E, X);
  t_sqr(l0, l0);
  t_sub(l0, l0, A);
  t_sub(l0, l0, F);
  t_dbl(t, B);
  t_dbl(t, t);
  t_sub(l0, l0, t);
  t_mul(l1, E, ZZ);
  t_mul(l2, Z3, ZZ);
  t_dbl(C, C);
  t_dbl(C, C);
  t_dbl(C, C);
  t_sub(t, D, X3);
  t_mul(t, t, E);
  t_sub(Y, t, C);  // E (D - X3) - 8 C
  X = X3;
  Z = Z3;
}
// T = T + Q and the line through T and Q: l0 = 2 (r x_Q - y_Q Z3), l1 = r, l2 = Z3
MSM_FN void pair_line_add(Fp2L &X, Fp2L &Y, Fp2L &Z, const Fp2L &qx, const Fp2L &qy, Fp2L &l0, Fp2L &l1,
                          Fp2L &l2) {
  Fp2L ZZ, U2, S2, H, HH, I, J, r, V, X3, Z3, t;
  t_sqr(ZZ, Z);
  t_mul(U2, qx, ZZ);
  t_mul(S2, qy, Z);
  t_mul(S2, S2, ZZ);
  t_sub(H, U2, X);
  t_sqr(HH, H);
  t_dbl(I, HH);
  t_dbl(I, I);
  t_mul(J, H, I);
  t_sub(r, S2, Y);
  t_dbl(r, r);
  t_mul(V, X, I);
  t_sqr(X3, r);
  t_sub(X3, X3, J);
  t_sub(X3, X3, V);
  t_sub(X3, X3, V);
  t_add(Z3, Z, H);
  t_sqr(Z3, Z3);
  t_sub(Z3, Z3, ZZ);
  t_sub(Z3, Z3, HH);
  t_mul(J, J, Y);
  t_sub(t, V, X3);
  t_mul(t, t, r);
  t_sub(t, t, J);
  t_sub(Y, t, J);  // r (V - X3) - 2 Y J
  t_mul(l0, r, qx);
  t_mul(t, qy, Z3);
  t_sub(l0, l0, t);
  t_dbl(l0, l0);
  l1 = r;
  l2 = Z3;
  X = X3;
  Z = Z3;
}

}  // namespace msm
