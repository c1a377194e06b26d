// encode_dev.hpp -- the tail of the bulk encoder: two coordinates of a finite or
// infinite point -> one ZCash entry (ref src/e1.c:139-234, src/e2.c the G2
// twins).  Device code, shared by k_encode (encode.hip, affine source) and the
// level-0 k_ta_down of the encoded tree kinds (to_affine.hip, Jacobian source).
#pragma once
#include "fp2l.hpp"
#include "kernels.hpp"

namespace msm {

// (p - 1) / 2, plain integer
MSM_CONST uint32_t ENC_PM1H[NL] = {0xfffd555, 0xff7ffff, 0x9ffffdc, 0xffff58a, 0xb120f55, 0x507b587, 0xfb39869,
                                   0x79c2895, 0x23ba5c2, 0xa5d66bb, 0xdd3db21, 0xf34d258, 0x8f51cbf, 0x000d008};

// The plain integer of a blst coordinate.  The limbs l (normalized, l < 2^384:
// stored limbs, canonical or not) stand for v 2^384; fp_mul(l, 2^8) = l 2^8 /
// 2^392 = v mod p.  l 2^8 < 2^392, so the product is at most p, and it is p
// exactly when l is a non-zero multiple of p -- as the reference's own
// Montgomery reduction of l before its last subtraction.  fp_csub_p then makes
// the value canonical.
__device__ __forceinline__ void enc_plain_le_p(Fp &r, const Fp &l) {
  Fp k;
  fp_zero(k);
  k.v[0] = 1u << 8;
  fp_mul(r, l, k);
}
// a > (p - 1) / 2 for a plain integer a <= p
__device__ __forceinline__ bool enc_gt_half(const Fp &a) {
  int32_t br = 0;
#pragma unroll
  for (int i = 0; i < NL; ++i) br = ((int32_t)ENC_PM1H[i] - (int32_t)a.v[i] + br) >> 28;
  return br != 0;
}
// a canonical plain integer -> 48 big-endian bytes at d (4-byte aligned), `top` ORed into byte 0
__device__ __forceinline__ void enc_st_be(uint32_t *d, const Fp &a, uint32_t top) {
  uint64_t l[6];
  pack384(l, a);
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    uint32_t hi = (uint32_t)(l[5 - i] >> 32);
    const uint32_t lo = (uint32_t)l[5 - i];
    if (i == 0) hi |= top << 24;
    d[2 * i] = __builtin_bswap32(hi);
    d[2 * i + 1] = __builtin_bswap32(lo);
  }
}

// One entry at e (48 G bytes, SER: 96 G).  x, y: this lane's component of the
// coordinates as blst limbs (see enc_plain_le_p); inf: the point is infinity (the
// same on both lanes of a pair).  G2: lane comp of a pair writes its component,
// the imaginary lane the first 48 bytes of a coordinate and the flag bits.
// Every lane runs the same instructions, and the pair swap sits outside every
// lane-dependent choice (a DPP move under a divergent branch reads zero from the
// lanes the branch switched off).  2 G products.
template <int G, bool SER>
__device__ __forceinline__ void enc_entry(uint8_t *e, const Fp &x, const Fp &y, bool inf, int comp) {
  Fp xi, yi;
  enc_plain_le_p(xi, x);
  enc_plain_le_p(yi, y);
  // the 0x20 flag: y > (p - 1) / 2, for Fp2 decided by the imaginary part unless
  // it is zero.  Taken before the last subtraction, as the reference does
  // (sgn0_pty_mont_384[x]): stored y limbs that are a non-zero multiple of p
  // count as p, non-zero and above the half, though the bytes written are zero.
  const uint32_t own = (enc_gt_half(yi) ? 1u : 0u) | (fp_is_zero_exact(yi) ? 2u : 0u);
  fp_csub_p(xi);
  fp_csub_p(yi);
  uint32_t sign = own & 1u;
  if (G == 2) {
    const uint32_t par = pair_swap(own);
    const uint32_t im = comp ? own : par, re = comp ? par : own;
    sign = (im & 2u) ? (re & 1u) : (im & 1u);
  }
  const bool lead = G == 1 || comp == 1;
  uint32_t top = SER ? (inf ? 0x40u : 0u) : (inf ? 0xc0u : (0x80u | (sign << 5)));
  top = lead ? top : 0u;
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    xi.v[i] = inf ? 0u : xi.v[i];
    yi.v[i] = inf ? 0u : yi.v[i];
  }
  uint32_t *d = reinterpret_cast<uint32_t *>(e) + (lead ? 0 : 12);
  enc_st_be(d, xi, top);
  if (SER) enc_st_be(d + 12 * G, yi, 0u);
}

}  // namespace msm
