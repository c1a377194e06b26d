// encode.hpp -- bulk ZCash encoding of points on the GPU
// (replaces a loop over the reference's one-point calls blst_p{1,2}_affine_compress,
// _affine_serialize, _compress and _serialize: ref src/e1.c:139-234 and the
// src/e2.c twins; kernels and orchestration in encode.hip, the tail shared with
// the inversion tree in encode_dev.hpp).  This header is host-only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "chunk_pipe.hpp"

namespace msm {

constexpr size_t ENC_CHUNK_DEFAULT = (size_t)1 << 18;

// points per chunk: MSM_ENCODE_CHUNK=<points> overrides the default, read at each call
inline size_t enc_chunk() {
  const size_t e = env_size("MSM_ENCODE_CHUNK");
  return e ? e : ENC_CHUNK_DEFAULT;
}

// One engine: the level buffer of the inversion tree (Jacobian sources,
// to_affine.hpp), and for host memory a staging lane per direction on the
// shared chunk pipe (chunk_pipe.hpp).
template <int G>
class Encode {
 public:
  static constexpr size_t AFF = 96 * G, JAC = 144 * G, COMP = 48 * G, ELEM = 56 * G;
  explicit Encode(int device) : dev_(device), pipe_(device) {}
  // n affine points (AFF bytes) or Jacobians (JAC bytes, `jacobian`) at src -> n
  // entries of COMP (compressed) or 2 COMP (serialized) bytes at dst; each side
  // flat, host or device.  `cs` orders the kernels (the caller's stream when a
  // side is device memory, else the engine's).  Device destination: returns with
  // the work queued on cs; host destination: returns with the data in dst.
  void run(hipStream_t cs, const void *src, void *dst, size_t n, bool jacobian, bool serialized, bool src_dev,
           bool dst_dev);
  size_t device_bytes() const { return lv_.bytes + in_.device_bytes() + out_.device_bytes(); }
  int device() const { return dev_; }

 private:
  int dev_;
  DevBuf lv_;
  Stage in_, out_;
  ChunkPipe pipe_;  // (last: it waits for the queued work before the buffers go)
  void kernels(hipStream_t s, const void *d_src, void *d_dst, size_t n, bool jacobian, bool serialized);
};

}  // namespace msm
