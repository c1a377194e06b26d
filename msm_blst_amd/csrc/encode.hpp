// encode.hpp -- bulk ZCash encoding of points on the GPU
// (replaces a loop over the reference's one-point calls blst_p{1,2}_affine_compress,
// _affine_serialize, _compress and _serialize: ref src/e1.c:139-234 and the
// src/e2.c twins; kernels and orchestration in encode.hip, the tail shared with
// the inversion tree in encode_dev.hpp).  This header is host-only.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "engine.hpp"

namespace msm {

constexpr size_t ENC_CHUNK_DEFAULT = (size_t)1 << 18;

// points per chunk: MSM_ENCODE_CHUNK=<points> overrides the default, read at each call
inline size_t enc_chunk() {
  const char *e = getenv("MSM_ENCODE_CHUNK");
  if (e && *e) {
    const long long v = atoll(e);
    if (v > 0) return (size_t)v;
  }
  return ENC_CHUNK_DEFAULT;
}

// One engine: the level buffer of the inversion tree (Jacobian sources,
// to_affine.hpp), and for host memory two pinned + two device staging buffers
// per direction with their own copy streams.
template <int G>
class Encode {
 public:
  static constexpr size_t AFF = 96 * G, JAC = 144 * G, COMP = 48 * G, ELEM = 56 * G;
  explicit Encode(int device);
  ~Encode();
  Encode(const Encode &) = delete;
  Encode &operator=(const Encode &) = delete;
  // n affine points (AFF bytes) or Jacobians (JAC bytes, `jacobian`) at src -> n
  // entries of COMP (compressed) or 2 COMP (serialized) bytes at dst; each side
  // flat, host or device.  `cs` orders the kernels (the caller's stream when a
  // side is device memory, else the engine's).  Device destination: returns with
  // the work queued on cs; host destination: returns with the data in dst.
  void run(hipStream_t cs, const void *src, void *dst, size_t n, bool jacobian, bool serialized, bool src_dev,
           bool dst_dev);
  size_t device_bytes() const { return lv_.bytes + din_[0].bytes + din_[1].bytes + dout_[0].bytes + dout_[1].bytes; }
  int device() const { return dev_; }

 private:
  int dev_;
  DevBuf lv_, din_[2], dout_[2];
  void *pin_in_[2] = {nullptr, nullptr}, *pin_out_[2] = {nullptr, nullptr};
  size_t pin_in_bytes_ = 0, pin_out_bytes_ = 0;
  hipStream_t h2d_ = nullptr, d2h_ = nullptr;
  hipEvent_t ev_h2d_[2] = {nullptr, nullptr}, ev_comp_[2] = {nullptr, nullptr}, ev_d2h_[2] = {nullptr, nullptr};
  hipEvent_t ev_busy_ = nullptr;  // the last kernel of the previous call (the level buffer is reused)
  void ensure_pinned(void **slots, size_t &have, size_t bytes);
  void kernels(hipStream_t s, const void *d_src, void *d_dst, size_t n, bool jacobian, bool serialized);
};

}  // namespace msm
