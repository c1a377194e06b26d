// fr_mem.hpp -- what the Fr kernels of fr_ntt.hip and fr_poly.hip share beside
// fr.hpp: an element at rest (32 bytes, 8-byte aligned) to and from registers, an
// Fr as a kernel argument and the host's way to one.  Device code (HIP).
#pragma once
#include "fr.hpp"
#include "host_fr.hpp"

namespace msm {

struct FrK {  // an Fr as a kernel argument
  uint32_t v[FR_NL];
};

// ---- at rest: 32 bytes, 8-byte aligned ----
__device__ __forceinline__ void fr_ld(Fr &r, const uint32_t *p) {
  const uint2 *s = reinterpret_cast<const uint2 *>(p);
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const uint2 v = s[i];
    w[2 * i] = v.x;
    w[2 * i + 1] = v.y;
  }
  fr_unpack(r, w);
}
__device__ __forceinline__ void fr_st(uint32_t *p, const Fr &a) {
  uint32_t w[8];
  fr_pack(w, a);
  uint2 *d = reinterpret_cast<uint2 *>(p);
#pragma unroll
  for (int i = 0; i < 4; ++i) d[i] = make_uint2(w[2 * i], w[2 * i + 1]);
}
__device__ __forceinline__ void fr_arg(Fr &r, const FrK &k) { fr_set(r, k.v); }

// ---- host side ----
// a 256-bit value as nine 29-bit limbs
inline void fr_limbs29(uint32_t out[FR_NL], const hfr::Fr &v) {
  for (int i = 0; i < FR_NL; ++i) {
    const int bit = FR_B * i, j = bit / 64, off = bit % 64;
    uint64_t w = v.l[j] >> off;
    if (off && j + 1 < 4) w |= v.l[j + 1] << (64 - off);
    out[i] = (uint32_t)w & FR_MASK;
  }
}
// the field element with blst_fr x, as the constant x 2^261 mod r the kernels multiply by
inline FrK fr_internal(const hfr::Fr &x) {
  FrK k;
  fr_limbs29(k.v, hfr::mul(x, hfr::from_u64(32)));
  return k;
}

}  // namespace msm
