// h2c_host.cpp -- the HIP-free host part of csrc/hash_to_curve.hpp (SHA-256, the
// DST_prime rule, the per-call template) as a stand-alone program, built by
// tests/test_hash_to_curve_host.py with -fsanitize=address,undefined.
//
//   h2c_host sha <hex>...        SHA-256 of each argument, one digest per line
//   h2c_host dstprime <hex>...   DST_prime of each argument
//   h2c_host bi <hex dst> <len_in_bytes> <hex b0> <i>
//                                the digest of the template's b_i message with
//                                its first 32 bytes set to b0 and its counter to
//                                i, hashed block by block as the kernel does
//   h2c_host tail <hex dst> <len_in_bytes>   the template's tail bytes
#define MSM_H2C_HOST_ONLY
#include "../../msm_blst_amd/csrc/hash_to_curve.hpp"

#include <cstdio>
#include <string>
#include <vector>

using namespace msm;

static std::vector<uint8_t> unhex(const char *s) {
  std::vector<uint8_t> out;
  const std::string h(s);
  if (h == "-") return out;  // the empty string
  for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)std::stoul(h.substr(i, 2), nullptr, 16));
  return out;
}
static void put(const uint8_t *p, size_t n) {
  for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
  printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  const std::string mode = argv[1];
  if (mode == "sha" || mode == "dstprime") {
    for (int k = 2; k < argc; ++k) {
      const std::vector<uint8_t> in = unhex(argv[k]);
      if (mode == "sha") {
        H2cSha s;
        uint8_t d[32];
        s.update(in.data(), in.size());
        s.final(d);
        put(d, 32);
      } else {
        uint8_t dp[H2C_DST_PRIME_MAX];
        put(dp, h2c_dst_prime(dp, in.data(), in.size()));
      }
    }
    return 0;
  }
  if ((mode == "bi" && argc == 6) || (mode == "tail" && argc == 4)) {
    const std::vector<uint8_t> dst = unhex(argv[2]);
    H2cTemplate t;
    h2c_make_template(t, dst.data(), dst.size(), (unsigned)atoi(argv[3]));
    if (mode == "tail") {
      put(t.tail, t.tail_len);
      return 0;
    }
    const std::vector<uint8_t> b0 = unhex(argv[4]);
    if (b0.size() != 32) return 2;
    uint32_t h[8];
    for (int i = 0; i < 8; ++i) h[i] = H2C_SHA_H0[i];
    for (uint32_t blk = 0; blk < t.nblk; ++blk) {
      uint32_t w[16];
      for (int k = 0; k < 16; ++k) w[k] = t.blk[blk * 16 + k];
      if (blk == 0) {
        for (int k = 0; k < 8; ++k)
          w[k] = ((uint32_t)b0[4 * k] << 24) | ((uint32_t)b0[4 * k + 1] << 16) | ((uint32_t)b0[4 * k + 2] << 8) | b0[4 * k + 3];
        w[8] |= (uint32_t)atoi(argv[5]) << 24;
      }
      h2c_sha_block(h, w);
    }
    uint8_t d[32];
    for (int i = 0; i < 8; ++i)
      for (int k = 0; k < 4; ++k) d[4 * i + k] = (uint8_t)(h[i] >> (24 - 8 * k));
    put(d, 32);
    return 0;
  }
  return 2;
}
