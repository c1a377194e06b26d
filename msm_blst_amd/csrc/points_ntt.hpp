// points_ntt.hpp -- batched NTTs over group elements on the GPU (msm_points_ntt;
// kernels and orchestration in points_ntt.hip, the schedule in
// points_ntt_plan.hpp).  This header is host-only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <map>

#include "chunk_pipe.hpp"
#include "points_mult.hpp"
#include "points_ntt_plan.hpp"

namespace msm {

// One engine: the working array of a chunk (xyzz), the table of a slice (xyzz
// multiples, also the gathered result of the chunk; then their affine rows),
// the level buffer of the shared inversion tree (to_affine.hpp), the twiddle
// tables by log_n, and for host memory a staging lane per direction on the
// shared chunk pipe (chunk_pipe.hpp).
template <int G>
class PointsNtt {
 public:
  static constexpr size_t AFF = 96 * G, ROW = 112 * G, XYZZ = 224 * G, ELEM = 56 * G;
  explicit PointsNtt(int device) : dev_(device), pipe_(device) {}
  // `batch` transforms of 2^log_n affine points each, src -> dst (flat, host or
  // device; dst may be src); flags: PN_INVERSE | PN_BITREV.  `cs` orders the
  // kernels (the caller's stream when a side is device memory, else the
  // engine's).  Device destination: returns with the work queued on cs; host
  // destination: returns with the data in dst.
  void run(hipStream_t cs, const void *src, void *dst, int log_n, size_t batch, int flags, bool src_dev, bool dst_dev);
  size_t device_bytes() const {
    size_t b = x_.bytes + xz_.bytes + rows_.bytes + lv_.bytes + in_.device_bytes() + out_.device_bytes();
    for (const auto &t : tw_) b += t.second.bytes;
    return b;
  }
  int device() const { return dev_; }

 private:
  int dev_;
  DevBuf x_, xz_, rows_, lv_;
  std::map<int, DevBuf> tw_;  // log_n -> pn_twiddles(log_n) scalars of 32 little-endian bytes
  Stage in_, out_;
  ChunkPipe pipe_;  // (last: it waits for the queued work before the buffers go)
  const uint8_t *twiddles(hipStream_t cs, int log_n);
  // one chunk of `tc` transforms, device to device
  void chunk(hipStream_t cs, const void *d_src, void *d_dst, int log_n, size_t tc, int flags, const uint8_t *tw,
             size_t slice);
};

}  // namespace msm
