// fr_poly.hpp -- evaluation-form polynomials over Fr on the GPU: the value at an
// arbitrary point and the quotient by (X - z), many polynomials per call
// (msm_fr_eval_quotient; kernels and orchestration in fr_poly.hip, the per-element
// steps in fr_quot.hpp).  Host-only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <map>

#include "chunk_pipe.hpp"
#include "env_size.hpp"

namespace msm {

enum { POLYF_DST_SCALAR = 4, POLYF_BITREV = 8 };  // the values of include/msm_mi355x.h
constexpr int POLY_MAX_LOG = 26;
constexpr int POLY_TILE_DEFAULT = 10, POLY_TILE_MIN = 2, POLY_TILE_MAX = 10;
constexpr size_t POLY_CHUNK_DEFAULT = (size_t)1 << 20;  // elements (32 MiB) per chunk
constexpr size_t POLY_CHUNK_MAX = (size_t)1 << 30;      // (the grid of the smallest tile stays below 2^31)

// log2 of the elements one workgroup inverts together: MSM_POLY_TILE=<log2> in 2..10
// overrides the default, read at each call
inline int poly_tile() {
  const size_t e = env_size("MSM_POLY_TILE");
  return e >= (size_t)POLY_TILE_MIN && e <= (size_t)POLY_TILE_MAX ? (int)e : POLY_TILE_DEFAULT;
}
// elements per chunk (whole polynomials; a longer polynomial is a chunk of its own):
// MSM_POLY_CHUNK=<elements> overrides the default, read at each call
inline size_t poly_chunk() {
  const size_t e = env_size("MSM_POLY_CHUNK");
  return std::min(e ? e : POLY_CHUNK_DEFAULT, POLY_CHUNK_MAX);
}

// One engine: the inverses d_i of a chunk, the partial sums of its tiles, the
// per-polynomial f_m and q_m, the domain tables (cached by log_n) and, for host
// memory, staging lanes on the shared chunk pipe.
class FrPoly {
 public:
  static constexpr size_t EL = 32;
  explicit FrPoly(int device) : dev_(device), pipe_(device) {}
  // `count` polynomials of 2^log_n blst_fr at polys and their points at z (the same
  // side) -> y (count blst_fr) and, unless q is NULL, the quotients (q == polys
  // allowed); y and q on the same side.  `cs` orders the kernels.  Device
  // destination: returns with the work queued on cs; host: with the data in place.
  void run(hipStream_t cs, const void *polys, const void *z, void *y, void *q, int log_n, size_t count, int flags,
           bool src_dev, bool dst_dev);
  size_t device_bytes() const;
  int device() const { return dev_; }

 private:
  struct Table {  // omega_n^e = lo[e & (2^lb - 1)] hi[e >> lb] for e < n (hi NULL: lo alone)
    DevBuf buf;
    const uint32_t *lo = nullptr, *hi = nullptr;
    int lb = 0;
  };
  int dev_;
  DevBuf d_, part_, fm_, qm_;
  std::map<int, Table> tw_;
  Stage in_, inz_, outq_, outy_;
  ChunkPipe pipe_;  // (last: it waits for the queued work before the buffers go)
  const Table &table(hipStream_t s, int log_n);
  void kernels(hipStream_t s, const void *d_f, const void *d_z, void *d_y, void *d_q, int log_n, size_t count,
               int flags);
};

}  // namespace msm
