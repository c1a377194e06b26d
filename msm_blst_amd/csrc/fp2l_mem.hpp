// fp2l_mem.hpp -- what the lane-pair code needs besides fp2l.hpp's arithmetic
// and that compiles for the device and for the host range-check build alike
// (MSM_FP_HOST_TEST, tests/host/fp12_host_shim.cpp): the loads and stores of
// one component of a stored Fp2, the Fermat inversion in Fp and the Fp2
// inversion on a lane pair.  Included by ches_kernels.hpp / pair_kernels.hpp
// (the kernels) and by fp12l.hpp (the tower).
#pragma once
#ifdef MSM_FP_HOST_TEST
#include <string.h>
#endif
#include "fp2l.hpp"

namespace msm {

// component `comp` of an Fp2 stored at p (14 limbs, 8-B aligned: 56-B components)
MSM_FN void ld_comp(Fp &r, const Fp2 *p, int comp) {
#ifdef MSM_FP_HOST_TEST
  memcpy(r.v, reinterpret_cast<const uint8_t *>(p) + comp * sizeof(Fp), sizeof(Fp));
#else
  const uint2 *s = reinterpret_cast<const uint2 *>(reinterpret_cast<const uint8_t *>(p) + comp * sizeof(Fp));
#pragma unroll
  for (int i = 0; i < NL / 2; ++i) {
    uint2 v = s[i];
    r.v[2 * i] = v.x;
    r.v[2 * i + 1] = v.y;
  }
#endif
}
MSM_FN void st_comp(Fp2 *p, const Fp &a, int comp) {
#ifdef MSM_FP_HOST_TEST
  memcpy(reinterpret_cast<uint8_t *>(p) + comp * sizeof(Fp), a.v, sizeof(Fp));
#else
  uint2 *d = reinterpret_cast<uint2 *>(reinterpret_cast<uint8_t *>(p) + comp * sizeof(Fp));
#pragma unroll
  for (int i = 0; i < NL / 2; ++i) d[i] = make_uint2(a.v[2 * i], a.v[2 * i + 1]);
#endif
}

// ---------------------------------------------------------------- inversion --
// a^(p-2) mod p (Fermat), fixed 2-bit windows, input any lazy value, output S.
// Inlined and register-lean (a, a^2, a^3 and the accumulator: ~60 VGPRs): the
// earlier 4-bit version kept a 16-entry table in scratch (912 B/lane) and was
// a call -- the table kernels that use it are now scratch-free.
// One inversion per lane amortises over the lane's 3h table rows, so its ~570
// products (vs ~490 with 4-bit windows) do not matter.
MSM_CONST uint64_t PM2[6] = {0xb9feffffffffaaa9ull, 0x1eabfffeb153ffffull, 0x6730d2a0f6b0f624ull,
                             0x64774b84f38512bfull, 0x4b1ba7b6434bacd7ull, 0x1a0111ea397fe69aull};
MSM_FN void fp_inv(Fp &r, const Fp &a) {
  Fp a1 = a, a2, a3, acc;
  fp_norm(a1);
  fp_sqr(a2, a1);
  fp_mul(a3, a2, a1);
  fp_one(acc);
  for (int k = 190; k >= 0; --k) {  // 2-bit windows of p - 2 (381 bits), from the top
    if (k != 190) {
      fp_sqr(acc, acc);
      fp_sqr(acc, acc);
    }
    const uint32_t w = (uint32_t)(PM2[k >> 5] >> ((k & 31) * 2)) & 3u;  // uniform: the exponent is a constant
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

// 1 / (a0 + a1 i) = (a0 - a1 i) / (a0^2 + a1^2) on a lane pair: both lanes form
// the norm a0^2 + a1^2 (own square + partner's square) and invert it (the same
// instructions on both lanes), then scale their own (negated on odd lanes)
// component.  a in S.
MSM_FN void f_inv(Fp2L &r, const Fp2L &a) {
  Fp own = a.c, sq, psq, d, neg, x;
  fp_norm(own);
  fp_sqr(sq, own);
  pair_swap(psq, sq);
  fp_add(d, sq, psq);  // < 4p lazy
  fp_inv(d, d);
  fp_neg<4>(neg, own);
  pair_sel(x, pair_odd(), neg, own);
  fp_mul(r.c, x, d);
}

}  // namespace msm
