// decode.hpp -- bulk decoding of ZCash-encoded points on the GPU
// (replaces the reference's one-point calls blst_p{1,2}_uncompress,
// blst_p{1,2}_deserialize and blst_p{1,2}_affine_in_g{1,2}: ref src/e1.c:236-351,
// src/e2.c:279-410, src/map_to_g1.c:531-559, src/map_to_g2.c:403-443; kernels
// and orchestration in decode.hip).  This header is host-only.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "engine.hpp"

namespace msm {

constexpr size_t DEC_CHUNK_DEFAULT = (size_t)1 << 18;

// entries per chunk: MSM_DECODE_CHUNK=<entries> overrides the default, read at each call
inline size_t dec_chunk() {
  const char *e = getenv("MSM_DECODE_CHUNK");
  if (e && *e) {
    const long long v = atoll(e);
    if (v > 0) return (size_t)v;
  }
  return DEC_CHUNK_DEFAULT;
}

// One engine: a status buffer per slot, and for host memory two pinned + two
// device staging buffers per direction with their own copy streams.
template <int G>
class Decode {
 public:
  static constexpr size_t AFF = 96 * G, COMP = 48 * G;
  explicit Decode(int device);
  ~Decode();
  Decode(const Decode &) = delete;
  Decode &operator=(const Decode &) = delete;
  // n entries of COMP (compressed) or 2 COMP (serialized) bytes at src -> n
  // affine points at dst (host or device, flat) and, when status is not NULL,
  // n status bytes in host memory.  `cs` orders the kernels (the caller's
  // stream when a side is device memory, else the engine's).  Returns with the
  // work queued on cs when dst is device memory and status is NULL; otherwise
  // with dst (host) and status written.
  void run(hipStream_t cs, const void *src, void *dst, uint8_t *status, size_t n, bool serialized, bool check_group,
           bool src_dev, bool dst_dev);
  size_t device_bytes() const {
    return din_[0].bytes + din_[1].bytes + dout_[0].bytes + dout_[1].bytes + dst_[0].bytes + dst_[1].bytes;
  }
  int device() const { return dev_; }

 private:
  int dev_;
  DevBuf din_[2], dout_[2], dst_[2];  // staged input, staged output, status bytes
  void *pin_in_[2] = {nullptr, nullptr}, *pin_out_[2] = {nullptr, nullptr}, *pin_st_[2] = {nullptr, nullptr};
  size_t pin_in_bytes_ = 0, pin_out_bytes_ = 0, pin_st_bytes_ = 0;
  hipStream_t h2d_ = nullptr, d2h_ = nullptr;
  hipEvent_t ev_h2d_[2] = {nullptr, nullptr}, ev_comp_[2] = {nullptr, nullptr}, ev_d2h_[2] = {nullptr, nullptr};
  hipEvent_t ev_busy_ = nullptr;  // the last kernel of the previous call (the status buffers are reused)
  void ensure_pinned(void **slots, size_t &have, size_t bytes);
  void kernels(hipStream_t s, const void *d_src, void *d_dst, uint8_t *d_status, size_t n, bool serialized,
               bool check_group);
};

}  // namespace msm
