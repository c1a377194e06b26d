// fr.hpp -- BLS12-381 scalar-field arithmetic (mod the group order r) for
// gfx950, kept in registers.  The device twin of the reference's Fr routines
// (ref src/exports.c blst_fr_*, src/vect.h mul_mont_sparse_256 and kin).
//
// Form: 9 limbs of 29 bits (261 bits, radix 2^29, Montgomery
// R' = 2^261), chosen by the same count as fp.hpp's 14 x 28: one v_mad_u64_u32
// per limb product and no carry inside a column.  A column holds at most 9
// a_i b_j and 9 m_i r_j, so with limb products below 2^60.6 it fits 64 bits;
// 81 + 81 mads and ~4 ops per column for a product (10 x 28 would issue 100 +
// 100, and 8 x 32 needs a carry chain after every mad).  fp.hpp's column
// templates (MulChain) are written for NL = 14 and P28; nothing of them is
// generic in the limb count, so the product below is its own short FIPS loop
// on fp.hpp's mad64 / top32 (and their host-build range checks).
//
// At rest an element is 32 bytes, the 4 x 64-bit limbs of blst_fr (a 2^256 mod
// r, canonical).  Those limbs are used AS the internal value: with R' = 2^261
// they stand for a 2^-5, which is invisible to everything linear (add, sub,
// the NTT butterflies, products by constants held as c 2^261).  Only a product
// of two data operands, and the two changes of form, pay one extra product by
// a constant (FR_C266, FR_C251, FR_K517, 32).
//
// Range classes (all values non-negative; tests/test_fr_bounds.py):
//   C : canonical, normalized limbs (< 2^29), value < r.  Everything at rest.
//   S : normalized limbs, value < 2r.  Every fr_mul and fr_nred output.
//   lazy : fr_add(S, S) < 4r, limbs < 2^30; fr_sub4(S, S) = a + 4r - b < 6r,
//          limbs < 2^29 + 2^30.  Legal first operand of fr_mul when the second
//          is normalized (limb products < 2^59.6), legal fr_nred input.
#pragma once
#include "fp.hpp"

namespace msm {

constexpr int FR_NL = 9;
constexpr int FR_B = 29;
constexpr uint32_t FR_MASK = 0x1fffffffu;
// -r^-1 mod 2^29 is 2^29 - 1 (r = 1 mod 2^32): m = -acc mod 2^29

// r in radix 2^29
MSM_CONST uint32_t FR_R29[FR_NL] = {0x1, 0x1ffffff8, 0x1f96ffbf, 0x1b4805ff, 0x1d80553b,
                                    0xc0404d0, 0x1520cce7, 0xa6533af, 0x73eda7};
// 4r with limbs borrow-adjusted so limbs 0..7 are >= 2^29 - 1 (subtrahend headroom)
MSM_CONST uint32_t FR_SUB4R[FR_NL] = {0x20000004, 0x3fffffdf, 0x3e5bfefe, 0x2d2017fe, 0x360154ee,
                                      0x30101342, 0x3483339c, 0x2994cebd, 0x1cfb69c};
// 2^261 mod r (one), 2^517 mod r (blst_scalar -> blst_fr), 2^266 mod r (after a
// product of two blst_fr), 2^251 mod r (after an inversion of a blst_fr)
MSM_CONST uint32_t FR_ONE[FR_NL] = {0x1fffffba, 0x22f, 0x1cb61180, 0xa4e5c00, 0xee8b1a2,
                                    0x16e6aedf, 0x1907f8bb, 0x853ddf7, 0x4d043f};
MSM_CONST uint32_t FR_K517[FR_NL] = {0x1e538d9e, 0x19e99103, 0x13b31ecc, 0x4e2d5e4, 0x181dac62,
                                     0x115f1ba1, 0x1e414fbb, 0x11b3009c, 0x13fec};
MSM_CONST uint32_t FR_C266[FR_NL] = {0x1ffff72b, 0x46a7, 0x1f5f3540, 0xce3021c, 0x118f3661,
                                     0x8176cb, 0x54e487c, 0x102e8190, 0x1e092e};
MSM_CONST uint32_t FR_C251[FR_NL] = {0, 0, 0, 0, 0, 0, 0, 0, 0x80000};
// blst_fr -> blst_scalar: a 2^256 times 32 / 2^261
MSM_CONST uint32_t FR_C32[FR_NL] = {32, 0, 0, 0, 0, 0, 0, 0, 0};

struct Fr {
  uint32_t v[FR_NL];
};

// Montgomery product a b / 2^261 mod r, FIPS.  Inputs: limb products a_i b_j <
// 2^60.6 (e.g. a lazy, b normalized; or both limbs < 2^30), a b < 2^261 r.
// Output: class S.  r may alias a or b.
MSM_FN void fr_mul(Fr &r, const Fr &a, const Fr &b) {
  uint32_t m[FR_NL];
  uint64_t acc = 0;
#pragma unroll
  for (int k = 0; k < FR_NL; ++k) {
#pragma unroll
    for (int i = 0; i <= k; ++i) acc = mad64(a.v[i], b.v[k - i], acc);
#pragma unroll
    for (int i = 0; i < k; ++i) acc = mad64(m[i], FR_R29[k - i], acc);
    m[k] = (0u - (uint32_t)acc) & FR_MASK;
    acc = mad64(m[k], FR_R29[0], acc);
    acc >>= FR_B;
  }
  uint32_t t[FR_NL];
#pragma unroll
  for (int k = FR_NL; k < 2 * FR_NL - 1; ++k) {
#pragma unroll
    for (int i = k - FR_NL + 1; i < FR_NL; ++i) acc = mad64(a.v[i], b.v[k - i], acc);
#pragma unroll
    for (int i = k - FR_NL + 1; i < FR_NL; ++i) acc = mad64(m[i], FR_R29[k - i], acc);
    t[k - FR_NL] = (uint32_t)acc & FR_MASK;
    acc >>= FR_B;
  }
  t[FR_NL - 1] = top32(acc);
#pragma unroll
  for (int i = 0; i < FR_NL; ++i) r.v[i] = t[i];
}
MSM_FN void fr_sqr(Fr &r, const Fr &a) { fr_mul(r, a, a); }

// lazy add: no carry propagation
MSM_FN void fr_add(Fr &r, const Fr &a, const Fr &b) {
#pragma unroll
  for (int i = 0; i < FR_NL; ++i) {
    MSM_CHECK((uint64_t)a.v[i] + b.v[i] <= 0xffffffffull);
    r.v[i] = a.v[i] + b.v[i];
  }
}
// a + 4r - b, b in S (normalized, top limb below the adjusted top limb of 4r)
MSM_FN void fr_sub4(Fr &r, const Fr &a, const Fr &b) {
#pragma unroll
  for (int i = 0; i < FR_NL; ++i) {
    MSM_CHECK((uint64_t)a.v[i] + FR_SUB4R[i] <= 0xffffffffull && a.v[i] + FR_SUB4R[i] >= b.v[i]);
    r.v[i] = a.v[i] + FR_SUB4R[i] - b.v[i];
  }
}
MSM_FN void fr_neg4(Fr &r, const Fr &a) {
#pragma unroll
  for (int i = 0; i < FR_NL; ++i) {
    MSM_CHECK(FR_SUB4R[i] >= a.v[i]);
    r.v[i] = FR_SUB4R[i] - a.v[i];
  }
}
// carry propagation -> limbs < 2^29 below the top limb (value unchanged)
MSM_FN void fr_norm(Fr &a) {
#pragma unroll
  for (int i = 0; i < FR_NL - 1; ++i) {
    MSM_CHECK((uint64_t)a.v[i + 1] + (a.v[i] >> FR_B) <= 0xffffffffull);
    a.v[i + 1] += a.v[i] >> FR_B;
    a.v[i] &= FR_MASK;
  }
}
// normalized v < 16r -> class S: quotient estimate from the top limb,
// q = floor(v8 floor(2^44 / (r8 + 1)) / 2^44) <= floor(v / r), and v - q r <
// 1.001 r (bounded over the top limb: tests/test_fr_bounds.py)
constexpr uint32_t FR_RED_MAG = 0x235509;  // floor(2^44 / (r8 + 1)), r8 = 0x73eda7
MSM_FN void fr_red(Fr &a) {
  const uint32_t q = (uint32_t)(((uint64_t)a.v[FR_NL - 1] * FR_RED_MAG) >> 44);
  int64_t c = 0;
#pragma unroll
  for (int i = 0; i < FR_NL; ++i) {
    const int64_t t = (int64_t)a.v[i] - (int64_t)((uint64_t)q * FR_R29[i]) + c;
    a.v[i] = (uint32_t)t & FR_MASK;
    c = t >> FR_B;
  }
  MSM_CHECK(c == 0);
}
MSM_FN void fr_nred(Fr &a) {
  fr_norm(a);
  fr_red(a);
}
// class S -> canonical
MSM_FN void fr_csub(Fr &a) {
  uint32_t t[FR_NL];
  int32_t br = 0;
#pragma unroll
  for (int i = 0; i < FR_NL; ++i) {
    const int32_t d = (int32_t)a.v[i] - (int32_t)FR_R29[i] + br;
    br = d >> FR_B;  // 0 or -1
    t[i] = (uint32_t)d & FR_MASK;
  }
  const bool ge = br == 0;
#pragma unroll
  for (int i = 0; i < FR_NL; ++i) a.v[i] = ge ? t[i] : a.v[i];
}
MSM_FN void fr_set(Fr &r, const uint32_t *c) {
#pragma unroll
  for (int i = 0; i < FR_NL; ++i) r.v[i] = c[i];
}
MSM_FN void fr_zero(Fr &r) {
#pragma unroll
  for (int i = 0; i < FR_NL; ++i) r.v[i] = 0;
}
MSM_FN void fr_one(Fr &r) { fr_set(r, FR_ONE); }
MSM_FN bool fr_is_zero_exact(const Fr &a) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < FR_NL; ++i) o |= a.v[i];
  return o == 0;
}
MSM_FN void fr_sel(Fr &r, bool c, const Fr &a) {  // r = c ? a : r
#pragma unroll
  for (int i = 0; i < FR_NL; ++i) r.v[i] = c ? a.v[i] : r.v[i];
}
// a times a constant held as c 2^261 (a table entry, FR_*): a c, class S
MSM_FN void fr_mulc(Fr &r, const Fr &a, const uint32_t *c) {
  Fr k;
  fr_set(k, c);
  fr_mul(r, a, k);
}

// 256 bits at rest (eight 32-bit words, little-endian: the limbs of a blst_fr or
// the bytes of a blst_scalar) <-> nine 29-bit limbs, in registers.  Any 256-bit
// value unpacks to normalized limbs; a value < 2^256 with normalized limbs packs.
MSM_FN void fr_unpack(Fr &r, const uint32_t (&w)[8]) {
#pragma unroll
  for (int i = 0; i < FR_NL; ++i) {
    const int j = (FR_B * i) / 32, off = (FR_B * i) % 32;
    const uint64_t two = ((uint64_t)(j + 1 < 8 ? w[j + 1] : 0u) << 32) | w[j];
    r.v[i] = (uint32_t)(two >> off) & FR_MASK;
  }
}
MSM_FN void fr_pack(uint32_t (&w)[8], const Fr &a) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int i = (32 * j) / FR_B, s = (32 * j) % FR_B;  // s <= 21: two limbs cover the word
    MSM_CHECK(a.v[i] <= FR_MASK && (i + 1 == FR_NL - 1 ? a.v[i + 1] < (1u << 24) : a.v[i + 1] <= FR_MASK));
    w[j] = (uint32_t)((((uint64_t)a.v[i + 1] << FR_B) | a.v[i]) >> s);
  }
}

// One elementwise operation on blst_fr limbs (msm_fr_op; OP is the MSM_FR_* value:
// 0 add, 1 sub, 2 mul, 3 sqr, 4 neg, 6 from_scalar, 7 to_scalar; the inversion is a
// tree, fr_ntt.hip).  x, y canonical (6: x any 256-bit value) -> x canonical.
template <int OP>
MSM_FN void fr_elem(Fr &x, const Fr &y) {
  if constexpr (OP == 0) {
    fr_add(x, x, y);
    fr_norm(x);  // < 2r
  } else if constexpr (OP == 1) {
    fr_sub4(x, x, y);
    fr_nred(x);
  } else if constexpr (OP == 2) {
    fr_mul(x, x, y);  // a b 2^251
    fr_mulc(x, x, FR_C266);
  } else if constexpr (OP == 3) {
    fr_sqr(x, x);
    fr_mulc(x, x, FR_C266);
  } else if constexpr (OP == 4) {
    fr_neg4(x, x);
    fr_nred(x);
  } else if constexpr (OP == 6) {
    fr_mulc(x, x, FR_K517);
  } else {
    static_assert(OP == 7, "unknown elementwise op");
    fr_mulc(x, x, FR_C32);
  }
  fr_csub(x);
}

}  // namespace msm
