// host_fr.hpp -- host twin of the Fr layer (fr.hpp), plain C++ with no HIP
// include, as host_fp.hpp is for Fp.  Elements are blst_fr: four little-endian
// 64-bit limbs of a 2^256 mod r, canonical (ref src/exports.c blst_fr_*).
// Used by the NTT plan's constants (roots of unity, 1 / n, shift powers), the
// C ABI's host-only calls and the tests.
#pragma once
#include <stdint.h>
#include <string.h>

namespace hfr {

struct Fr {
  uint64_t l[4];
};

constexpr Fr R = {{0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull}};
constexpr uint64_t N0 = 0xfffffffeffffffffull;  // -r^-1 mod 2^64
constexpr Fr ONE = {{0x00000001fffffffeull, 0x5884b7fa00034802ull, 0x998c4fefecbc4ff5ull, 0x1824b159acc5056full}};
constexpr Fr RR = {{0xc999e990f3f29c6dull, 0x2b6cedcb87925c23ull, 0x05d314967254398full, 0x0748d9d99f59ff11ull}};
// omega = 7^((r - 1) / 2^32), of order 2^32 (omega^(2^31) = r - 1), Montgomery form
constexpr Fr OMEGA = {{0xb9b58d8c5f0e466aull, 0x5b1b4c801819d7ecull, 0x0af53ae352a31e64ull, 0x5bf3adda19e9b27bull}};

inline bool geq_r(const uint64_t *a) {
  for (int i = 3; i >= 0; --i)
    if (a[i] != R.l[i]) return a[i] > R.l[i];
  return true;
}
inline void sub_r(uint64_t *a) {
  unsigned __int128 br = 0;
  for (int i = 0; i < 4; ++i) {
    const unsigned __int128 d = (unsigned __int128)a[i] - R.l[i] - br;
    a[i] = (uint64_t)d;
    br = (d >> 64) & 1;
  }
}
inline bool is_zero(const Fr &a) { return (a.l[0] | a.l[1] | a.l[2] | a.l[3]) == 0; }
inline bool eq(const Fr &a, const Fr &b) { return memcmp(&a, &b, sizeof a) == 0; }

// a b / 2^256 mod r (CIOS); any a < 2^256 with b < r gives a canonical result
inline Fr mul(const Fr &a, const Fr &b) {
  uint64_t t[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; ++i) {
    unsigned __int128 c = 0;
    for (int j = 0; j < 4; ++j) {
      c += (unsigned __int128)a.l[j] * b.l[i] + t[j];
      t[j] = (uint64_t)c;
      c >>= 64;
    }
    c += t[4];
    t[4] = (uint64_t)c;
    t[5] = (uint64_t)(c >> 64);
    const uint64_t m = t[0] * N0;
    c = (unsigned __int128)m * R.l[0] + t[0];
    c >>= 64;
    for (int j = 1; j < 4; ++j) {
      c += (unsigned __int128)m * R.l[j] + t[j];
      t[j - 1] = (uint64_t)c;
      c >>= 64;
    }
    c += t[4];
    t[3] = (uint64_t)c;
    t[4] = t[5] + (uint64_t)(c >> 64);
  }
  if (t[4] || geq_r(t)) sub_r(t);
  Fr r;
  memcpy(r.l, t, sizeof r.l);
  return r;
}
inline Fr sqr(const Fr &a) { return mul(a, a); }
inline Fr add(const Fr &a, const Fr &b) {
  uint64_t t[4];
  unsigned __int128 c = 0;
  for (int i = 0; i < 4; ++i) {
    c += (unsigned __int128)a.l[i] + b.l[i];
    t[i] = (uint64_t)c;
    c >>= 64;
  }
  if (c || geq_r(t)) sub_r(t);
  Fr r;
  memcpy(r.l, t, sizeof r.l);
  return r;
}
inline Fr neg(const Fr &a) {
  if (is_zero(a)) return a;
  Fr r = R;
  unsigned __int128 br = 0;
  for (int i = 0; i < 4; ++i) {
    const unsigned __int128 d = (unsigned __int128)r.l[i] - a.l[i] - br;
    r.l[i] = (uint64_t)d;
    br = (d >> 64) & 1;
  }
  return r;
}
inline Fr sub(const Fr &a, const Fr &b) { return add(a, neg(b)); }
// a^e, e a plain 256-bit exponent (little-endian limbs)
inline Fr pow(const Fr &a, const uint64_t e[4]) {
  Fr r = ONE;
  for (int i = 255; i >= 0; --i) {
    r = sqr(r);
    if ((e[i / 64] >> (i % 64)) & 1) r = mul(r, a);
  }
  return r;
}
inline Fr pow2k(Fr a, unsigned k) {  // a^(2^k)
  while (k--) a = sqr(a);
  return a;
}
inline Fr inverse(const Fr &a) {  // Fermat; 0 -> 0
  const uint64_t e[4] = {R.l[0] - 2, R.l[1], R.l[2], R.l[3]};
  return pow(a, e);
}
// the two byte forms: blst_scalar (32 little-endian bytes of a, any 256-bit
// value taken mod r) <-> blst_fr
inline Fr from_scalar(const uint8_t s[32]) {
  Fr a;
  for (int i = 0; i < 4; ++i) {
    uint64_t w = 0;
    for (int j = 7; j >= 0; --j) w = (w << 8) | s[8 * i + j];
    a.l[i] = w;
  }
  return mul(a, RR);
}
inline void to_scalar(uint8_t s[32], const Fr &a) {
  const Fr one = {{1, 0, 0, 0}};
  const Fr v = mul(a, one);
  for (int i = 0; i < 32; ++i) s[i] = (uint8_t)(v.l[i / 8] >> (8 * (i % 8)));
}
inline Fr from_u64(uint64_t v) {
  const Fr a = {{v, 0, 0, 0}};
  return mul(a, RR);
}
// omega_n for n = 2^log_n, log_n <= 32
inline Fr root_of_unity(unsigned log_n) { return pow2k(OMEGA, 32 - log_n); }

}  // namespace hfr
