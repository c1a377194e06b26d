// points_mult.hpp -- bulk scalar multiplication out[i] = [k_i] P_i on the GPU
// (replaces a loop over the reference's one-point blst_p{1,2}_mult /
// _unchecked_mult: ref src/e1.c:505-533, src/e2.c, src/ec_mult.h; kernels and
// orchestration in points_mult.hip).  This header is host-only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "chunk_pipe.hpp"

namespace msm {

constexpr size_t PM_CHUNK_DEFAULT = (size_t)1 << 18;
constexpr int PM_ROWS = 8;  // 1P .. 8P: signed 4-bit windows

// points per chunk: MSM_POINTS_MULT_CHUNK=<points> overrides the default, read at each call
inline size_t pm_chunk() {
  const size_t e = env_size("MSM_POINTS_MULT_CHUNK");
  return e ? e : PM_CHUNK_DEFAULT;
}

// One engine: the table of a chunk (xyzz multiples, then their affine rows),
// the level buffer of the shared inversion tree (to_affine.hpp), and for host
// memory a staging lane per direction on the shared chunk pipe
// (chunk_pipe.hpp).  A staged input slot holds the points followed by the
// scalars, packed (nbits + 7) / 8 bytes apart.
template <int G>
class PointsMult {
 public:
  static constexpr size_t AFF = 96 * G, ROW = 112 * G, XYZZ = 224 * G, ELEM = 56 * G;
  explicit PointsMult(int device) : dev_(device), pipe_(device) {}
  // dst[i] = [k_i] P_i for i < n, k_i = the low nbits bits of the little-endian
  // scalar at scalars + i stride (0 < nbits <= 256, stride >= (nbits + 7) / 8).
  // one_point: `points` holds one point, used for every scalar.  points and
  // scalars are both host or both device memory (src_dev); dst is flat, host or
  // device.  `cs` orders the kernels (the caller's stream when a side is device
  // memory, else the engine's).  Device destination: returns with the work
  // queued on cs; host destination: returns with the data in dst.
  void run(hipStream_t cs, const void *points, const uint8_t *scalars, void *dst, size_t n, int nbits, size_t stride,
           bool one_point, bool src_dev, bool dst_dev);
  size_t device_bytes() const { return xz_.bytes + rows_.bytes + lv_.bytes + in_.device_bytes() + out_.device_bytes(); }
  int device() const { return dev_; }

 private:
  int dev_;
  DevBuf xz_, rows_, lv_;  // xyzz multiples / ladder results, affine rows, tree levels
  Stage in_, out_;
  ChunkPipe pipe_;  // (last: it waits for the queued work before the buffers go)
  // the rows of `np` points (row m of point t at rows_[(m - 1) np + t])
  void table(hipStream_t s, const void *d_points, size_t np);
  // one chunk, device to device, on a table of np rows per multiple (np == 1: every lane reads point 0's)
  void ladder(hipStream_t s, size_t np, const uint8_t *d_scalars, void *d_dst, size_t n, int nbits, size_t stride);
};

}  // namespace msm
