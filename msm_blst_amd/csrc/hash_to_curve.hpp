// hash_to_curve.hpp -- bulk hash-to-curve on the GPU (replaces the reference's
// one-message calls blst_hash_to_g{1,2}, blst_encode_to_g{1,2} and
// blst_map_to_g{1,2}: ref src/map_to_g1.c:285-453, src/map_to_g2.c:173-401,
// src/hash_to_field.c:51-154; kernels and orchestration in hash_to_curve.hip,
// DESIGN.md section 19).
//
// The first part is free of HIP: SHA-256 (one block function shared by the
// host and the device, a small streaming wrapper for the host) and the
// per-call template the host prepares from the DST.  tests/host/h2c_host.cpp
// compiles it alone (MSM_H2C_HOST_ONLY) under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "env_size.hpp"
#include "hash_to_curve_consts.hpp"

#ifndef H2C_FN
#define H2C_FN inline
#endif

namespace msm {

H2C_FN uint32_t h2c_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// One SHA-256 block.  The message schedule is a rolling window of 16 words in
// w (consumed); fully unrolled, every index is a constant, so on the device h
// and w stay in registers.
H2C_FN void h2c_sha_block(uint32_t (&h)[8], uint32_t (&w)[16]) {
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    if (i >= 16) {
      const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
      const uint32_t s0 = h2c_rotr(w15, 7) ^ h2c_rotr(w15, 18) ^ (w15 >> 3);
      const uint32_t s1 = h2c_rotr(w2, 17) ^ h2c_rotr(w2, 19) ^ (w2 >> 10);
      w[i & 15] += s0 + w[(i + 9) & 15] + s1;
    }
    const uint32_t t1 = hh + (h2c_rotr(e, 6) ^ h2c_rotr(e, 11) ^ h2c_rotr(e, 25)) + ((e & f) ^ (~e & g)) +
                        H2C_SHA_K[i] + w[i & 15];
    const uint32_t t2 = (h2c_rotr(a, 2) ^ h2c_rotr(a, 13) ^ h2c_rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
    hh = g;
    g = f;
    f = e;
    e = d + t1;
    d = c;
    c = b;
    b = a;
    a = t1 + t2;
  }
  h[0] += a;
  h[1] += b;
  h[2] += c;
  h[3] += d;
  h[4] += e;
  h[5] += f;
  h[6] += g;
  h[7] += hh;
}

constexpr size_t H2C_CHUNK_DEFAULT = (size_t)1 << 18;
constexpr size_t H2C_DST_PRIME_MAX = 256;  // 255 bytes of DST and its length byte

// What the host prepares once per call from the DST and the output length:
//   tail  what follows aug || msg in the b_0 hash: I2OSP(len_in_bytes, 2) || I2OSP(0, 1) || DST_prime
//   blk   the b_i message strxor(b_0, b_(i-1)) || I2OSP(i, 1) || DST_prime with its SHA padding,
//         as big-endian words; the first 32 bytes and the counter byte are left zero for the kernel
struct H2cTemplate {
  uint32_t blk[80];
  uint32_t nblk;      // SHA blocks of blk in use (1 .. 5)
  uint32_t tail_len;  // bytes of tail in use (4 .. 259)
  uint8_t tail[264];
};

// ---- host side (left out of the translation unit of the kernels, MSM_H2C_DEVICE_TU,
// where the SHA constants are device variables) ----
#ifndef MSM_H2C_DEVICE_TU
struct H2cSha {
  uint32_t h[8];
  uint8_t buf[64];
  uint64_t n = 0;
  H2cSha() {
    for (int i = 0; i < 8; ++i) h[i] = H2C_SHA_H0[i];
  }
  void block() {
    uint32_t w[16];
    for (int i = 0; i < 16; ++i)
      w[i] = ((uint32_t)buf[4 * i] << 24) | ((uint32_t)buf[4 * i + 1] << 16) | ((uint32_t)buf[4 * i + 2] << 8) |
             buf[4 * i + 3];
    h2c_sha_block(h, w);
  }
  void update(const uint8_t *p, size_t len) {
    for (size_t i = 0; i < len; ++i) {
      buf[n++ & 63] = p[i];
      if ((n & 63) == 0) block();
    }
  }
  void final(uint8_t out[32]) {
    const uint64_t bits = n * 8;
    const uint8_t one = 0x80, zero = 0;
    update(&one, 1);
    while ((n & 63) != 56) update(&zero, 1);
    for (int i = 7; i >= 0; --i) {
      const uint8_t b = (uint8_t)(bits >> (8 * i));
      update(&b, 1);
    }
    for (int i = 0; i < 8; ++i)
      for (int k = 0; k < 4; ++k) out[4 * i + k] = (uint8_t)(h[i] >> (24 - 8 * k));
  }
};

// DST_prime = DST || I2OSP(len(DST), 1), a DST of more than 255 bytes first
// replaced by SHA-256("H2C-OVERSIZE-DST-" || DST) (RFC 9380 5.3.3; ref hash_to_field.c:65-71).
// out holds H2C_DST_PRIME_MAX bytes; returns the length.
inline size_t h2c_dst_prime(uint8_t *out, const uint8_t *dst, size_t dst_len) {
  if (dst_len > 255) {
    H2cSha s;
    s.update(reinterpret_cast<const uint8_t *>("H2C-OVERSIZE-DST-"), 17);
    s.update(dst, dst_len);
    s.final(out);
    dst_len = 32;
  } else if (dst_len) {
    memcpy(out, dst, dst_len);
  }
  out[dst_len] = (uint8_t)dst_len;
  return dst_len + 1;
}

inline void h2c_make_template(H2cTemplate &t, const uint8_t *dst, size_t dst_len, unsigned len_in_bytes) {
  uint8_t dp[H2C_DST_PRIME_MAX];
  const size_t dpl = h2c_dst_prime(dp, dst, dst_len);
  memset(&t, 0, sizeof t);
  t.tail[0] = (uint8_t)(len_in_bytes >> 8);
  t.tail[1] = (uint8_t)len_in_bytes;
  t.tail[2] = 0;
  memcpy(t.tail + 3, dp, dpl);
  t.tail_len = (uint32_t)(3 + dpl);
  uint8_t b[320];
  memset(b, 0, sizeof b);
  memcpy(b + 33, dp, dpl);
  const size_t len = 33 + dpl;  // the b_i message
  b[len] = 0x80;
  const size_t total = (len + 1 + 8 + 63) & ~(size_t)63;
  const uint64_t bits = (uint64_t)len * 8;
  for (int i = 0; i < 8; ++i) b[total - 1 - i] = (uint8_t)(bits >> (8 * i));
  t.nblk = (uint32_t)(total / 64);
  for (size_t i = 0; i < total / 4; ++i)
    t.blk[i] = ((uint32_t)b[4 * i] << 24) | ((uint32_t)b[4 * i + 1] << 16) | ((uint32_t)b[4 * i + 2] << 8) | b[4 * i + 3];
}

#endif  // !MSM_H2C_DEVICE_TU

// entries per chunk: MSM_H2C_CHUNK=<entries> overrides the default, read at each call
inline size_t h2c_chunk() {
  const size_t e = env_size("MSM_H2C_CHUNK");
  return e ? e : H2C_CHUNK_DEFAULT;
}

}  // namespace msm

#ifndef MSM_H2C_HOST_ONLY
#include <vector>

#include "chunk_pipe.hpp"

namespace msm {

// What one call does
enum {
  H2C_MAP = 0,    // field elements -> points
  H2C_FIELD = 1,  // messages -> field elements
  H2C_HASH = 2,   // messages -> points
};

// The messages of a call: `offsets` (host, n + 1 values) or fixed `msg_len`;
// msgs and aug in the same memory space.
struct H2cMsgs {
  const uint8_t *msgs = nullptr;
  const size_t *offsets = nullptr;
  size_t msg_len = 0;
  const uint8_t *aug = nullptr;
  size_t aug_len = 0;
};

// One engine: the device buffers of a chunk (field elements, the images on the
// isogenous curve, the points before the batch inversion, its levels, the
// template) and for host memory staging lanes on the shared chunk pipe
// (chunk_pipe.hpp): messages or elements, aug and offsets up, results down,
// and a pinned lane for the template.
template <int G>
class HashToCurve {
 public:
  static constexpr size_t AFF = 96 * G, ELEM = 48 * G, XYZZ = 224 * G;
  explicit HashToCurve(int device) : dev_(device), pipe_(device) {}
  // mode H2C_MAP: n * count field elements at u -> n affine points at dst;
  // H2C_FIELD: n messages -> n * count elements at dst; H2C_HASH: n messages
  // -> n affine points.  `cs` orders the kernels (the caller's stream when a
  // side is device memory, else the engine's).  Returns with the work queued
  // on cs when dst is device memory, otherwise with dst written.
  void run(hipStream_t cs, int mode, const void *u, const H2cMsgs &m, const H2cTemplate *tmpl, void *dst, size_t n,
           int count, bool src_dev, bool dst_dev);
  size_t device_bytes() const {
    return r_.bytes + u_.bytes + e_.bytes + x_.bytes + lv_.bytes + tp_.bytes + in_.device_bytes() +
           aug_.device_bytes() + off_.device_bytes() + out_.device_bytes();
  }
  int device() const { return dev_; }

 private:
  int dev_;
  DevBuf r_, u_, e_, x_, lv_, tp_;  // uniform bytes, elements, images on E', points (xyzz), inversion levels, the template
  Stage in_, aug_, off_, out_, tpl_;
  // tpl_: pinned only, slot 0 goes into tp_ on the compute stream; the pipe comes
  // last: it waits for the queued work before the buffers go
  ChunkPipe pipe_;
  void map_kernels(hipStream_t s, const void *d_u, void *d_dst, size_t n, int count);
};

}  // namespace msm
#endif  // !MSM_H2C_HOST_ONLY
