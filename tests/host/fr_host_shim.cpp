// fr_host_shim.cpp -- host (g++) build of the engine's Fr header
// (msm_blst_amd/csrc/fr.hpp) with every range check enabled (MSM_FP_HOST_TEST:
// a wrapping 64-bit column, a wrapping or negative limb, or a negative reduced
// value sets msm_fp_overflow), and of its plain host twin (host_fr.hpp).  TEST
// INFRASTRUCTURE ONLY: loaded by tests/test_fr_bounds.py through ctypes; the
// same header text is compiled for gfx950 in the product.
#define MSM_FP_HOST_TEST 1
#include <string.h>

#include "../../msm_blst_amd/csrc/fr.hpp"
#include "../../msm_blst_amd/csrc/host_fr.hpp"

extern "C" {
int msm_fp_overflow = 0;

using namespace msm;

static Fr ld(const uint32_t *p) {
  Fr r;
  memcpy(r.v, p, sizeof r.v);
  return r;
}

int h_fr_overflow(int clear) {
  int v = msm_fp_overflow;
  if (clear) msm_fp_overflow = 0;
  return v;
}

// limb-level primitives: 0 mul, 1 add, 2 sub4, 3 nred, 4 csub, 5 neg4, 6 norm
void h_fr_prim(int op, uint32_t *r, const uint32_t *a, const uint32_t *b) {
  Fr R = ld(a);
  switch (op) {
    case 0: fr_mul(R, ld(a), ld(b)); break;
    case 1: fr_add(R, ld(a), ld(b)); break;
    case 2: fr_sub4(R, ld(a), ld(b)); break;
    case 3: fr_nred(R); break;
    case 4: fr_csub(R); break;
    case 5: fr_neg4(R, ld(a)); break;
    case 6: fr_norm(R); break;
  }
  memcpy(r, R.v, sizeof R.v);
}

// the butterfly of the transform kernels: (a + b reduced, (a - b) w), w a table entry
void h_fr_bfly(uint32_t *ra, uint32_t *rb, const uint32_t *a, const uint32_t *b, const uint32_t *w) {
  Fr s, d;
  fr_add(s, ld(a), ld(b));
  fr_sub4(d, ld(a), ld(b));
  fr_nred(s);
  fr_mul(d, d, ld(w));
  memcpy(ra, s.v, sizeof s.v);
  memcpy(rb, d.v, sizeof d.v);
}

void h_fr_unpack(uint32_t *limbs, const uint32_t *w) {
  uint32_t t[8];
  memcpy(t, w, sizeof t);
  Fr r;
  fr_unpack(r, t);
  memcpy(limbs, r.v, sizeof r.v);
}
void h_fr_pack(uint32_t *w, const uint32_t *limbs) {
  uint32_t t[8];
  fr_pack(t, ld(limbs));
  memcpy(w, t, sizeof t);
}

// msm_fr_op's element formulas on the 32 bytes at rest (op: the MSM_FR_* value, not 5)
void h_fr_elem(int op, uint8_t *out, const uint8_t *a, const uint8_t *b) {
  uint32_t wa[8], wb[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  memcpy(wa, a, 32);
  if (b) memcpy(wb, b, 32);
  Fr x, y;
  fr_unpack(x, wa);
  fr_unpack(y, wb);
  switch (op) {
    case 0: fr_elem<0>(x, y); break;
    case 1: fr_elem<1>(x, y); break;
    case 2: fr_elem<2>(x, y); break;
    case 3: fr_elem<3>(x, y); break;
    case 4: fr_elem<4>(x, y); break;
    case 6: fr_elem<6>(x, y); break;
    default: fr_elem<7>(x, y); break;
  }
  fr_pack(wa, x);
  memcpy(out, wa, 32);
}

// the host twin (op: the MSM_FR_* value)
void h_fr_host(int op, uint8_t *out, const uint8_t *a, const uint8_t *b) {
  hfr::Fr x, y = {{0, 0, 0, 0}}, r;
  memcpy(&x, a, 32);
  if (b) memcpy(&y, b, 32);
  switch (op) {
    case 0: r = hfr::add(x, y); break;
    case 1: r = hfr::sub(x, y); break;
    case 2: r = hfr::mul(x, y); break;
    case 3: r = hfr::sqr(x); break;
    case 4: r = hfr::neg(x); break;
    case 5: r = hfr::inverse(x); break;
    case 6: r = hfr::from_scalar(a); break;
    default: hfr::to_scalar(out, x); return;
  }
  memcpy(out, &r, 32);
}
// a^e for a 32-byte little-endian exponent
void h_fr_host_pow(uint8_t *out, const uint8_t *a, const uint8_t *e) {
  hfr::Fr x;
  uint64_t ex[4];
  memcpy(&x, a, 32);
  memcpy(ex, e, 32);
  const hfr::Fr r = hfr::pow(x, ex);
  memcpy(out, &r, 32);
}
}
