// to_affine.hpp -- bulk Jacobian -> affine normalisation on the GPU
// (replaces ref src/multi_scalar.c:17-62, blst_p{1,2}s_to_affine; kernels and
// orchestration in to_affine.hip).  This header is host-only: the plan (level
// sizes, chunk size) is shared with abi.cpp's msm_to_affine_levels().
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "chunk_pipe.hpp"

namespace msm {

// Hierarchical Montgomery batch inversion: a lane of k_ta_up multiplies TA_K
// consecutive elements of a level into one element of the next, until a level
// has at most TA_LEAF elements; those are inverted one per lane (k_ta_leaf)
// and k_ta_down walks back.  K = 8 keeps the K - 1 prefix products of a group
// in registers (7 x 14 VGPRs; K = 16 would need 210 and spill).
// Level sizes for one default chunk of 2^18 points: 32768, 4096, 512, 64
// (4 levels); a 2^20 input is four such chunks.
constexpr size_t TA_K = 8;
constexpr size_t TA_LEAF = 256;
constexpr size_t TA_CHUNK_DEFAULT = (size_t)1 << 18;

// points per chunk: MSM_TO_AFFINE_CHUNK=<points> overrides the default, read at each call
inline size_t ta_chunk() {
  const size_t e = env_size("MSM_TO_AFFINE_CHUNK");
  return e ? e : TA_CHUNK_DEFAULT;
}

// sizes of the levels above n points (at least one level for n >= 1)
inline std::vector<size_t> ta_levels(size_t n) {
  std::vector<size_t> lv;
  while (n) {
    n = (n + TA_K - 1) / TA_K;
    lv.push_back(n);
    if (n <= TA_LEAF) break;
  }
  return lv;
}

// total elements of the levels above n points (the size of a level buffer)
inline size_t ta_level_elems(size_t n) {
  size_t e = 0;
  for (size_t v : ta_levels(n)) e += v;
  return e;
}

// what level 0 of a tree reads and its last kernel writes
enum {
  TA_LEVEL = 0,      // (inside the tree: a level above the points)
  TA_JAC = 1,        // blst Jacobians -> blst affine points
  TA_XYZZ_BLST = 2,  // xyzz points in internal form (ec.hpp, Xyzz<F>) -> blst affine points
  TA_XYZZ_ROWS = 3,  // the same -> canonical affine points in internal form (Aff<F>, 112 G bytes)
  TA_JAC_ENC_C = 4,  // blst Jacobians -> compressed ZCash entries (48 G bytes, encode_dev.hpp)
  TA_JAC_ENC_S = 5,  // blst Jacobians -> serialized ZCash entries (96 G bytes)
};
// The whole tree, device to device, on stream s: n points of `kind` at d_src ->
// n affine points at d_dst; lv: a device buffer of at least ta_level_elems(n)
// elements of 56 G bytes.  Infinity (Z / ZZZ zero) gives the all-zero point
// (the encoded kinds: the infinity entry, c0 00.. / 40 00..; d_dst 4-byte aligned).
// Defined in to_affine.hip for the group it is compiled for.
template <int G>
void ta_tree(hipStream_t s, void *lv, size_t lv_bytes, int kind, const void *d_src, void *d_dst, size_t n);

// One engine: level buffers, and for host memory a staging lane per direction
// on the shared chunk pipe (chunk_pipe.hpp).
template <int G>
class ToAffine {
 public:
  static constexpr size_t JAC = 144 * G, AFF = 96 * G, ELEM = 56 * G;
  // runs [first index, pointer, count] of a blst pointer array (ptr_walk.hpp)
  struct Run {
    size_t first;
    const uint8_t *p;
    size_t count;
  };
  explicit ToAffine(int device) : dev_(device), pipe_(device) {}
  // n Jacobians -> n affine points.  src: device memory (src_dev), or host
  // memory named by `runs` (ascending, covering [0, n)).  dst: flat, host or
  // device.  `cs` orders the kernels (the caller's stream when a side is device
  // memory, else the engine's).  Device destination: returns with the work
  // queued on cs; host destination: returns with the data in dst.
  void run(hipStream_t cs, const void *src_dev_ptr, const std::vector<Run> &runs, void *dst, size_t n, bool src_dev,
           bool dst_dev);
  size_t device_bytes() const { return lv_.bytes + in_.device_bytes() + out_.device_bytes(); }
  int device() const { return dev_; }

 private:
  int dev_;
  DevBuf lv_;
  Stage in_, out_;
  ChunkPipe pipe_;  // (last: it waits for the queued work before the buffers go)
  void kernels(hipStream_t s, const void *d_src, void *d_dst, size_t n);
};

}  // namespace msm
