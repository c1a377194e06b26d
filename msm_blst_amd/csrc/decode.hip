// decode.hip -- bulk decoding of ZCash-encoded BLS12-381 points on one MI355X
// (replaces ref src/e1.c:236-351 blst_p1_uncompress / _deserialize,
// src/e2.c:279-410 the G2 twins, src/map_to_g1.c:531-559 and
// src/map_to_g2.c:403-443 blst_p{1,2}_affine_in_g{1,2}).
//
//   k_decode        entry i -> affine point i (blst layout) + status byte:
//                   parse (big-endian bytes -> 28-bit limbs, range check
//                   against p, one product with 2^784 -> internal form),
//                   a = x^3 + b, y = a^((p+1)/4) by a fixed 2-bit-window chain
//                   (G2: two such chains over Fp, through the norm), y^2 == a,
//                   sign from the canonical y against (p-1)/2; serialized
//                   entries check y^2 == a on the given y instead
//   k_decode_group  status-0 points only: the reference's endomorphism tests
//                   (Scott, eprint 2021/1130): G1 [z^2]P == -sigma^2(P), G2
//                   [|z|]P == -psi(P), |z| = 0xd201000000010000, on ec.hpp's
//                   xyzz formulas; a failing point gets status 3 and is zeroed
//
// Lanes of a wave hold different statuses: every lane runs the same chains and
// the results are selected at the end (the only wave-level branch skips the
// square root of a serialized array when no lane of the wave holds a compressed
// entry).  The output of every failed entry is the all-zero point.
//
// G1 runs one lane per point, G2 one lane PAIR per point (Fp2L, fp2l.hpp): a
// lane holds one component, so both kernels have the register use of G1.  The
// Fp2 square root needs both components in both lanes (the norm a0^2 + a1^2
// and the two Fp chains are the same instructions on both lanes).
//
// Products per point as built (an fp_mul2 priced 1.5 Fp products, an fp_mul4
// 2.5; tools/decode_timing.py): G1 decode 546 (the chain: 378 squarings + 159
// products), group check 1238.5 (127 doublings, 16 mixed additions); G2, both
// lanes, 2185 and 1604.
#include "decode.hpp"

#include <cstring>

#include "decode_dev.hpp"
#include "pair_kernels.hpp"

#ifndef MSM_GROUP
#error "define MSM_GROUP (1 or 2)"
#endif

namespace msm {

// lane (pair) t < n: entry t of src -> out[t], status[t]
template <int G, bool SER>
static __global__ void __launch_bounds__(128)
    k_decode(const uint8_t *__restrict__ src, size_t n, uint64_t *__restrict__ out, uint8_t *__restrict__ status) {
  typedef typename DecLane<G>::LF LF;
  const size_t tt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int comp = G == 2 ? (int)(tt & 1) : 0;
  const size_t t = G == 2 ? tt >> 1 : tt;
  if (t >= n) return;  // whole pairs only
  // the imaginary part comes first and carries the flags
  const bool lead = G == 1 || comp == 1;
  const uint32_t *e = reinterpret_cast<const uint32_t *>(src + t * (SER ? 96 : 48) * G) + (lead ? 0 : 12);
  Fp xi;
  uint32_t top, nzo;
  dec_ld_be(xi, top, nzo, e, lead);
  // (the swap outside the lane-dependent choice: a DPP move under a divergent
  // branch reads zero from the lanes the branch switched off)
  const uint32_t ptop = dec_swap<G>(top);
  const uint32_t flags = lead ? top : ptop;
  const bool fc = (flags & 4u) != 0, finf = (flags & 2u) != 0, fsgn = (flags & 1u) != 0;
  const bool x_zero = dec_or<G>(nzo) == 0;
  const bool x_bad = dec_or<G>(dec_ge_p(xi) ? 1u : 0u) != 0;
  LF x, a, y;
  dec_mulk(dec_c(x), xi, DEC_R2);  // S
  {
    LF t2;
    Fp four;
    f_sqr(t2, x);
    f_mul(a, t2, x);
    fp_set(four, DEC_FOUR);
    fp_add(dec_c(a), dec_c(a), four);
    fp_nred(dec_c(a));  // a = x^3 + b, S
  }
  bool root_ok = false;
  f_zero(y);
  if (!SER || __builtin_amdgcn_ballot_w64(fc) != 0) {
    LF y2;
    dec_sqrt(y, a);
    f_sqr(y2, y);
    root_ok = dec_all<G>(dec_eq(dec_c(y2), dec_c(a)));
    const bool neg = dec_sign(y) != fsgn;
    fp_cneg4(dec_c(y), dec_c(y), neg);  // < 4p lazy
  }
  uint32_t st;
  bool inf = false;
  if (SER && flags == 0) {
    Fp yi;
    uint32_t ytop, ynz;
    dec_ld_be(yi, ytop, ynz, e + 12 * G, false);
    const bool y_bad = dec_or<G>(dec_ge_p(yi) ? 1u : 0u) != 0;
    LF ys, y2;
    dec_mulk(dec_c(ys), yi, DEC_R2);
    f_sqr(y2, ys);
    const bool on_curve = dec_all<G>(dec_eq(dec_c(y2), dec_c(a)));
    st = (x_bad || y_bad) ? 1u : !on_curve ? 2u : (G == 1 && x_zero) ? 3u : 0u;
    y = ys;
  } else if (fc) {
    if (finf) {
      inf = !fsgn && x_zero;
      st = inf ? 0u : 1u;
    } else {
      st = x_bad ? 1u : !root_ok ? 2u : (G == 1 && x_zero) ? 3u : 0u;
    }
  } else if (SER && finf) {
    Fp yi;
    uint32_t ytop, ynz;
    dec_ld_be(yi, ytop, ynz, e + 12 * G, false);
    inf = !fsgn && x_zero && dec_or<G>(ynz) == 0;
    st = inf ? 0u : 1u;
  } else {
    st = 1u;
  }
  Fp xo, yo, zero;
  dec_mulk(xo, dec_c(x), FROMINT28);
  dec_mulk(yo, dec_c(y), FROMINT28);
  fp_csub_p(xo);
  fp_csub_p(yo);
  fp_zero(zero);
  dec_sel(xo, st != 0 || inf, zero);
  dec_sel(yo, st != 0 || inf, zero);
  uint64_t *o = out + t * 12 * G;
  pack384(o + 6 * comp, xo);
  pack384(o + 6 * G + 6 * comp, yo);
  if (comp == 0) status[t] = (uint8_t)st;
}

// lane (pair) t < n: a status-0 point outside the prime-order subgroup gets
// status 3 and the all-zero output; everything else stays as it is
template <int G>
static __global__ void __launch_bounds__(128, 2) k_decode_group(uint64_t *out, uint8_t *status, size_t n) {
  typedef typename DecLane<G>::LF LF;
  const size_t tt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int comp = G == 2 ? (int)(tt & 1) : 0;
  const size_t t = G == 2 ? tt >> 1 : tt;
  if (t >= n) return;  // whole pairs only
  uint64_t *o = out + t * 12 * G;
  Aff<LF> p;
  fp_from_blst(dec_c(p.x), o + 6 * comp);
  fp_from_blst(dec_c(p.y), o + 6 * G + 6 * comp);
  const bool zx = f_is_zero_exact(p.x), zy = f_is_zero_exact(p.y);
  const bool skip = status[t] != 0 || (zx && zy);
  const bool ok = dec_in_group<G>(p);  // (decode_dev.hpp)
  if (!skip && !ok) {
    Fp zero;
    fp_zero(zero);
    pack384(o + 6 * comp, zero);
    pack384(o + 6 * G + 6 * comp, zero);
    if (comp == 0) status[t] = 3;
  }
}

// one chunk, device to device
template <int G>
void Decode<G>::kernels(hipStream_t s, const void *d_src, void *d_dst, uint8_t *d_status, size_t n, bool serialized,
                        bool check_group) {
  const unsigned B = 128;
  const dim3 grid(nblk(n * G, B));
  if (serialized)
    hipLaunchKernelGGL((k_decode<G, true>), grid, dim3(B), 0, s, static_cast<const uint8_t *>(d_src), n,
                       static_cast<uint64_t *>(d_dst), d_status);
  else
    hipLaunchKernelGGL((k_decode<G, false>), grid, dim3(B), 0, s, static_cast<const uint8_t *>(d_src), n,
                       static_cast<uint64_t *>(d_dst), d_status);
  MSM_HIP_CHECK(hipGetLastError());
  if (check_group) {
    hipLaunchKernelGGL(k_decode_group<G>, grid, dim3(B), 0, s, static_cast<uint64_t *>(d_dst), d_status, n);
    MSM_HIP_CHECK(hipGetLastError());
  }
}

template <int G>
void Decode<G>::run(hipStream_t cs, const void *src, void *dst, uint8_t *status, size_t n, bool serialized,
                    bool check_group, bool src_dev, bool dst_dev) {
  if (!n) return;
  DeviceGuard g(dev_);
  const size_t ENC = serialized ? 2 * COMP : COMP;
  const size_t C = std::min(n, dec_chunk());
  const bool out_host = !dst_dev || status;  // something comes back per chunk
  dst_[0].ensure(C);
  dst_[1].ensure(C);
  if (!src_dev) in_.ensure(C * ENC);
  if (!dst_dev) out_.ensure(C * AFF);
  if (status) st_.ensure(C, false);
  pipe_.begin(cs);  // the status buffers of the previous call
  auto pend = pipe_.pending([&](int slot, size_t off, size_t cnt) {
    if (!dst_dev) memcpy(static_cast<uint8_t *>(dst) + off * AFF, out_.pin[slot], cnt * AFF);
    if (status) memcpy(status + off, st_.pin[slot], cnt);
  });
  size_t k = 0;
  for (size_t c0 = 0; c0 < n; c0 += C, ++k) {
    const size_t cnt = std::min(C, n - c0);
    const int slot = (int)(k & 1);
    const void *d_src;
    void *d_dst;
    if (!src_dev) {
      pipe_.upload(cs, slot, [&] { memcpy(in_.pin[slot], static_cast<const uint8_t *>(src) + c0 * ENC, cnt * ENC); },
                   {{in_, slot, cnt * ENC}});
      d_src = in_.dev[slot].p;
    } else {
      d_src = static_cast<const uint8_t *>(src) + c0 * ENC;
    }
    if (out_host) pipe_.out_open(cs, slot);  // (guards dst_[slot] as well as the output slot)
    d_dst = dst_dev ? static_cast<void *>(static_cast<uint8_t *>(dst) + c0 * AFF) : out_.dev[slot].p;
    kernels(cs, d_src, d_dst, dst_[slot].as<uint8_t>(), cnt, serialized, check_group);
    pipe_.computed(cs, slot);
    if (out_host)
      pipe_.download(cs, slot, pend, c0, cnt,
                     {{out_, slot, dst_dev ? 0 : cnt * AFF}, {st_.pin[slot], dst_[slot].p, status ? cnt : 0}});
  }
  pend.flush();
  pipe_.finish(cs);
}

template class Decode<MSM_GROUP>;

}  // namespace msm
