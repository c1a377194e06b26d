// ec.hpp -- BLS12-381 point arithmetic in xyzz coordinates for gfx950,
// generic over the base field (G1: Fp, G2: Fp2).
//
// Replaces the reference's bucket formulas (src/ec_ops.h:642-785):
//   xyzz_madd  <- POINTonE1xyzz_dadd_affine (ec_ops.h:710-769), madd-2008-s
//                 with the sign twist and the mdbl-2008-s-1 doubling branch
//   xyzz_add   <- POINTonE1xyzz_dadd (ec_ops.h:642-702), add-2008-s /
//                 dbl-2008-s-1
//   xyzz_dbl   <- the doubling branch of the above, used by the reductions
// An xyzz point (X, Y, ZZZ, ZZ) stands for (X/ZZ, Y/ZZZ); infinity is ZZ == 0
// (set exactly, never produced by a product).  Every coordinate leaving these
// functions is in range class S (normalized, < 2p per component; fp.hpp)
// except x, which is left in class X (normalized, < 10p): it only enters
// products and the subtrahend of f_sub16, so its reduction is skipped.
// Branches for the rare cases (P == +-bucket, infinity) are data-dependent
// and divergent; random inputs never take them, the parity tests force them.
#pragma once
#include "fp.hpp"

namespace msm {

template <class F>
struct Aff {
  F x, y;
};
template <class F>
struct Xyzz {
  F x, y, zzz, zz;
};

template <class F>
MSM_FN bool xyzz_is_inf(const Xyzz<F> &a) {
  return f_is_zero_exact(a.zz);
}
template <class F>
MSM_FN void xyzz_set_inf(Xyzz<F> &a) {
  f_zero(a.x);
  f_zero(a.y);
  f_zero(a.zzz);
  f_zero(a.zz);
}
// bucket := +-P   (ZZ = ZZZ = 1, Y negated instead of ZZZ; same point as the
// reference's (X, Y, -1, 1) representative of ec_ops.h:720-724)
template <class F>
MSM_FN void xyzz_from_aff(Xyzz<F> &r, const Aff<F> &p, bool neg) {
  r.x = p.x;
  if (neg) {
    f_neg4(r.y, p.y);
    f_nred(r.y);
  } else {
    r.y = p.y;
  }
  f_one(r.zzz);
  f_one(r.zz);
}

// doubling of an xyzz point given in S (dbl-2008-s-1):
//   U = 2Y, V = U^2, W = U V, S = X V, M = 3 X^2 (+ a ZZ^2, a = 0)
//   X3 = M^2 - 2S, Y3 = M (S - X3) - W Y, ZZ3 = V ZZ, ZZZ3 = W ZZZ
template <class F, class CF = MulSplit>
MSM_FN void xyzz_dbl(Xyzz<F> &r, const Xyzz<F> &a) {
  if (xyzz_is_inf(a)) {
    r = a;
    return;
  }
  // ordered so that each input coordinate dies at its last use (ZZ3, ZZZ3
  // first; r may alias a).  Round 3 reverted this order because compiled into
  // the one-lane G2 table kernel (256 VGPR + 256 AGPR + 1.5 KB scratch) it gave
  // wrong rows on the device only: 2Q right, then Q itself corrupted across
  // the call (3Q and every later row wrong; tests/test_gpu_table_rows.py).  The
  // lane-pair table kernel has no spills and builds correct rows with it
  // (DESIGN 11).
  F U, V, W, S, M, t, X3;
  f_add(U, a.y, a.y);      // < 4p lazy
  f_sqr(V, U, CF{});             // S
  f_mul(W, V, U, CF{});          // S
  f_mul(S, a.x, V, CF{});        // S
  f_mul(r.zz, V, a.zz, CF{});    // ZZ3 = V ZZ (V, ZZ die)
  f_mul(r.zzz, W, a.zzz, CF{});  // ZZZ3 = W ZZZ
  f_sqr(M, a.x, CF{});           // S (X dies)
  f_mul3(M, M);            // < 6p lazy
  f_sqr(X3, M, CF{});            // S
  F z;
  f_zero(z);
  f_sub_2x(X3, X3, z, S);  // M^2 + 8p - 2S   < 10p
  f_norm(X3);              // X
  f_sub16(t, S, X3);       // < 18p
  f_mul_sub(r.y, t, M, W, a.y, CF{});  // Y3 = M (S - X3) - W Y   S (one reduction)
  r.x = X3;
}

// acc += (neg ? -P : P); P affine, canonical, not infinity (callers skip the
// all-zero affine point, as ec_ops.h:717 does).
// acc_affine: acc is exactly what xyzz_from_aff left (ZZ1 = ZZZ1 = 1, a
// bucket's first entry), so the four products by one are skipped: U2 := X2,
// S2 := +-Y2, ZZ3 := PP, ZZZ3 := PPP -- 5 reductions instead of 9 for every
// bucket's first add.  The flag may differ between the lanes of a wave (it
// must not differ inside a G2 lane pair; a pair shares its bucket); the skips
// are branches around the products of the one madd body, not a second copy of
// it.  A negated Y2 is reduced as xyzz_from_aff reduces it: the generic path
// reduces it in the product S2 = Y2 ZZZ1, and left lazy (< 4p) it would put R
// at 8p, past the < 6p f_sqr and f_mul_sub are proven for
// (tests/test_first_pair_bounds.py).  X2 and +-Y2 are in class S like the
// products they replace, so every later range is the generic path's.
template <class F, class CF = MulSplit>
MSM_FN void xyzz_madd(Xyzz<F> &acc, const Aff<F> &p, bool neg, bool acc_affine = false) {
  if (xyzz_is_inf(acc)) {
    xyzz_from_aff(acc, p, neg);
    return;
  }
  F y2, P, R, PP, PPP, t;
  if (neg) {
    f_neg4(y2, p.y);       // < 4p, limbs < 2^29
  } else {
    y2 = p.y;
  }
  if (acc_affine) {
    P = p.x;                    // U2 = X2              canonical
    if (neg) f_nred(y2);        // S2 = +-Y2            S
    R = y2;
  } else {
    f_mul_bs(P, p.x, acc.zz, CF{});   // U2 = X2 ZZ1          S
    f_mul_bs(R, y2, acc.zzz, CF{});   // S2 = Y2 ZZZ1         S
  }
  f_sub16(P, P, acc.x);    // P = U2 - X1          < 18p lazy
  f_sub4(R, R, acc.y);     // R = S2 - Y1          < 6p lazy
  f_sqr(PP, P, CF{});            // PP                   S
  if (__builtin_expect(f_is_zero_S(PP), 0)) {
    // X1 == X2: either P == bucket (double it) or P == -bucket (infinity)
    F RR;
    f_sqr(RR, R, CF{});
    if (f_is_zero_S(RR)) {
      // +-P equals the bucket: double the bucket itself (still untouched
      // here), so the affine operand dies after U2 and S2 instead of staying
      // live through the whole madd for this branch
      Xyzz<F> b = acc;
      xyzz_dbl<F, CF>(acc, b);
    } else {
      xyzz_set_inf(acc);
    }
    return;
  }
  // ordered so that ZZ1, P, X1 and PP die as early as possible (register
  // pressure: 8-10 live field elements; G2 elements are 28 VGPRs each);
  // f_mul_bs: second operand normalized (every S value here)
  // (only where the flag is a run-time value: every other caller's madd
  // compiles to what it was)
  if (!__builtin_constant_p(acc_affine)) f_pin(PP);
  if (acc_affine) {
    acc.zz = PP;                     // ZZ3 = PP             S
  } else {
    f_mul_bs(acc.zz, acc.zz, PP, CF{});    // ZZ3 = ZZ1 PP         S
  }
  f_mul_bs(PPP, P, PP, CF{});         // S
  f_mul_bs(acc.x, acc.x, PP, CF{});      // Q = X1 PP  (in place of X1)   S
  if (acc_affine) {
    acc.zzz = PPP;                   // ZZZ3 = PPP           S
  } else {
    f_mul_bs(acc.zzz, acc.zzz, PPP, CF{}); // ZZZ3 = ZZZ1 PPP      S
  }
  F X3;
  f_sqr(X3, R, CF{});            // R^2                  S
  f_sub_2x(X3, X3, PPP, acc.x);  // R^2 + 8p - PPP - 2Q   < 10p
  f_norm(X3);              // X3 = R^2 - PPP - 2Q  X
  f_sub16(t, acc.x, X3);   // Q - X3  < 18p
  f_mul_sub(acc.y, t, R, acc.y, PPP, CF{});  // Y3 = R (Q - X3) - Y1 PPP   S (one reduction)
  acc.x = X3;
}

// acc += b, both xyzz in S: the 13-reduction form (U1 = X1 ZZ2 and S1 = Y1 ZZZ2
// reduced on their own).  Kept for the one-lane Fp2 and for hash_to_curve.hip,
// see xyzz_add.
template <class F, class CF = MulSplit>
MSM_FN void xyzz_add_u1s1(Xyzz<F> &acc, const Xyzz<F> &b) {
  // Computed in place so that b dies early and at most ~8 field elements are
  // live (G2: 28 VGPRs each): acc is first rewritten as the representative
  // (U1, S1, ZZZ1 ZZZ2, ZZ1 ZZ2) of the same point, which is also what the
  // doubling branch doubles.
  F P, R, PP, PPP, t;
  f_mul_bs(acc.x, acc.x, b.zz, CF{});    // U1 = X1 ZZ2          S
  f_mul_bs(acc.y, acc.y, b.zzz, CF{});   // S1 = Y1 ZZZ2         S
  f_mul_bs(P, b.x, acc.zz, CF{});        // U2 = X2 ZZ1          S
  f_sub4(P, P, acc.x);          // P = U2 - U1          < 6p
  f_mul_bs(R, b.y, acc.zzz, CF{});       // S2 = Y2 ZZZ1         S
  f_sub4(R, R, acc.y);          // R = S2 - S1          < 6p
  f_mul_bs(acc.zz, acc.zz, b.zz, CF{});
  f_mul_bs(acc.zzz, acc.zzz, b.zzz, CF{});
  f_sqr(PP, P, CF{});
  if (__builtin_expect(f_is_zero_S(PP), 0)) {
    F RR;
    f_sqr(RR, R, CF{});
    if (f_is_zero_S(RR)) {
      Xyzz<F> a = acc;
      xyzz_dbl<F, CF>(acc, a);
    } else {
      xyzz_set_inf(acc);
    }
    return;
  }
  f_mul_bs(acc.zz, acc.zz, PP, CF{});    // ZZ3 = ZZ1 ZZ2 PP
  f_mul_bs(PPP, P, PP, CF{});
  f_mul_bs(acc.x, acc.x, PP, CF{});      // Q = U1 PP  (in place of U1)
  f_mul_bs(acc.zzz, acc.zzz, PPP, CF{}); // ZZZ3 = ZZZ1 ZZZ2 PPP
  F X3;
  f_sqr(X3, R, CF{});
  f_sub_2x(X3, X3, PPP, acc.x);
  f_norm(X3);                   // X3 = R^2 - PPP - 2Q  X
  f_sub16(t, acc.x, X3);
  f_mul_sub(acc.y, t, R, acc.y, PPP, CF{});  // Y3 = R (Q - X3) - S1 PPP   S (one reduction)
  acc.x = X3;
}

// Which fields take the regrouped add below.  The one-lane Fp2 does not: its
// kernels sit at the 512 registers of a one-wave kernel, and with P and R as
// four-product sums (fp_mul4: eight operands live at once) k_wbits_pairs<2>
// spilled VGPRs, which no product kernel may (tests/test_kernel_resources.py;
// DESIGN 11 has the history).  The range proof holds for it all the same
// (tests/test_xyzz_add_bounds.py); none of these kernels is on a batch's
// critical path.
template <class F>
struct AddRegrouped {
  static constexpr bool value = true;
};
template <>
struct AddRegrouped<Fp2> {
  static constexpr bool value = false;
};

// the regrouped add of two finite points
template <class F, class CF = MulSplit>
MSM_FN void xyzz_add_regrouped(Xyzz<F> &acc, const Xyzz<F> &b) {
  // 12 products and 2 squares with 11 Montgomery reductions instead of 13
  // (DESIGN 23): U1 = X1 ZZ2 and S1 = Y1 ZZZ2 are never reduced on their own.
  // P and R are each one two-product difference (f_mul_sub), and the later
  // uses of U1 and S1 are regrouped around V = ZZ2 PP and W = ZZZ2 PPP, which
  // ZZ3 and ZZZ3 need anyway:  Q = U1 PP = X1 V,  S1 PPP = Y1 W.
  // Ordered so that b dies early (b.x, b.y in P and R, b.zz in V, b.zzz in W);
  // at most nine field elements are live, at R (G2: 28 VGPRs each).
  // f_mul_sub takes X1 and X2 in class X here (normalized, < 10p): a b + c
  // (4p - d) < 10p 2p + 10p 4p = 60 p^2 and every column stays below 2^64
  // (tests/test_xyzz_add_bounds.py).
  F P, R, PP, PPP, V, W, t;
  f_mul_sub_bs(P, b.x, acc.zz, acc.x, b.zz, CF{});    // P = X2 ZZ1 - X1 ZZ2     S
  f_mul_sub_bs(R, b.y, acc.zzz, acc.y, b.zzz, CF{});  // R = Y2 ZZZ1 - Y1 ZZZ2   S
  f_sqr(PP, P, CF{});                              // PP                      S
  if (__builtin_expect(f_is_zero_S(PP), 0)) {
    F RR;
    f_sqr(RR, R, CF{});
    if (f_is_zero_S(RR)) {
      // b equals acc: double acc itself, which is still the untouched input
      Xyzz<F> a = acc;
      xyzz_dbl<F, CF>(acc, a);
    } else {
      xyzz_set_inf(acc);
    }
    return;
  }
  f_mul_bs(V, b.zz, PP, CF{});           // V = ZZ2 PP           S  (ZZ2 dies)
  f_mul_bs(acc.zz, acc.zz, V, CF{});     // ZZ3 = ZZ1 V          S
  f_mul_bs(acc.x, acc.x, V, CF{});       // Q = X1 V  (in place of X1)   S  (V dies)
  f_mul_bs(PPP, P, PP, CF{});            // PPP                  S  (P, PP die)
  f_mul_bs(W, b.zzz, PPP, CF{});         // W = ZZZ2 PPP         S  (ZZZ2 dies)
  f_mul_bs(acc.zzz, acc.zzz, W, CF{});   // ZZZ3 = ZZZ1 W        S
  F X3;
  f_sqr(X3, R, CF{});
  f_sub_2x(X3, X3, PPP, acc.x);
  f_norm(X3);                   // X3 = R^2 - PPP - 2Q  X
  f_sub16(t, acc.x, X3);
  f_mul_sub_bs(acc.y, t, R, acc.y, W, CF{});  // Y3 = R (Q - X3) - Y1 W   S (one reduction; R is S here)
  acc.x = X3;
}

// acc += b, both xyzz in S.  REGROUP = false asks for the 13-reduction form
// (xyzz_add<F, false>(acc, b)): the cofactor-clearing kernel of
// hash_to_curve.hip, two ladders and five adds in one body, lost a wave (G1) and
// spilled (G2) with the regrouped one.
template <class F, bool REGROUP = AddRegrouped<F>::value, class CF = MulSplit>
MSM_FN void xyzz_add(Xyzz<F> &acc, const Xyzz<F> &b) {
  if (xyzz_is_inf(b)) return;
  if (xyzz_is_inf(acc)) {
    acc = b;
    return;
  }
  if constexpr (REGROUP) xyzz_add_regrouped<F, CF>(acc, b);
  else xyzz_add_u1s1<F, CF>(acc, b);
}

}  // namespace msm
