// decode.hpp -- bulk decoding of ZCash-encoded points on the GPU
// (replaces the reference's one-point calls blst_p{1,2}_uncompress,
// blst_p{1,2}_deserialize and blst_p{1,2}_affine_in_g{1,2}: ref src/e1.c:236-351,
// src/e2.c:279-410, src/map_to_g1.c:531-559, src/map_to_g2.c:403-443; kernels
// and orchestration in decode.hip).  This header is host-only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "chunk_pipe.hpp"

namespace msm {

constexpr size_t DEC_CHUNK_DEFAULT = (size_t)1 << 18;

// entries per chunk: MSM_DECODE_CHUNK=<entries> overrides the default, read at each call
inline size_t dec_chunk() {
  const size_t e = env_size("MSM_DECODE_CHUNK");
  return e ? e : DEC_CHUNK_DEFAULT;
}

// One engine: a status buffer per slot, and for host memory a staging lane per
// direction and a pinned lane for the status bytes on the shared chunk pipe
// (chunk_pipe.hpp).
template <int G>
class Decode {
 public:
  static constexpr size_t AFF = 96 * G, COMP = 48 * G;
  explicit Decode(int device) : dev_(device), pipe_(device) {}
  // n entries of COMP (compressed) or 2 COMP (serialized) bytes at src -> n
  // affine points at dst (host or device, flat) and, when status is not NULL,
  // n status bytes in host memory.  `cs` orders the kernels (the caller's
  // stream when a side is device memory, else the engine's).  Returns with the
  // work queued on cs when dst is device memory and status is NULL; otherwise
  // with dst (host) and status written.
  void run(hipStream_t cs, const void *src, void *dst, uint8_t *status, size_t n, bool serialized, bool check_group,
           bool src_dev, bool dst_dev);
  // one chunk, device to device, queued on s: the kernels alone, with the status
  // bytes left in device memory at d_status (sig_verify.hip reads them there)
  void kernels(hipStream_t s, const void *d_src, void *d_dst, uint8_t *d_status, size_t n, bool serialized,
               bool check_group);
  size_t device_bytes() const { return in_.device_bytes() + out_.device_bytes() + dst_[0].bytes + dst_[1].bytes; }
  int device() const { return dev_; }

 private:
  int dev_;
  DevBuf dst_[2];        // status bytes of a slot
  Stage in_, out_, st_;  // st_: the status bytes' pinned slots (they come down from dst_)
  ChunkPipe pipe_;       // (last: it waits for the queued work before the buffers go)
};

}  // namespace msm
