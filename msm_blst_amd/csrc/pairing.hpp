// pairing.hpp -- bulk pairings on the GPU:
//   dst[j] = fe(prod over offsets[j] <= i < offsets[j + 1] of ml(P_i, Q_i))
// (replaces a host loop over the reference's blst_miller_loop / blst_fp12_mul /
// blst_final_exp, one call per pair: ref src/pairing.c:181-262 and 371-404;
// kernels and orchestration in pairing.hip, the tower in fp12l.hpp, the host
// plan in segments_plan.hpp).  This header is host-only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "chunk_pipe.hpp"
#include "point_segments.hpp"
#include "segments_plan.hpp"

namespace msm {

constexpr size_t PAIR_CHUNK_DEFAULT = (size_t)1 << 16;
constexpr size_t PAIR_PIECE_MAX = 64;
// lane pairs that are resident at once at the register budget of the Miller
// kernel (one wave per SIMD): 256 CUs x 4 SIMDs x 64 lanes / 2
constexpr size_t PAIR_LANE_PAIRS = (size_t)256 * 4 * 64 / 2;

// pairs (and segments written) per chunk: MSM_PAIRING_CHUNK=<pairs> overrides
// the default, read at each call
inline size_t pair_chunk() {
  const size_t e = env_size("MSM_PAIRING_CHUNK");
  return e ? e : PAIR_CHUNK_DEFAULT;
}

// The piece length for m pairs in flight.  A piece of L pairs pays the Fp12
// squaring of a step once instead of L times, but the chip wants a piece for
// every resident lane pair: L is the longest that still leaves one, clamped to
// [1, PAIR_PIECE_MAX] (the rule of seg_piece_len).  MSM_PAIRING_PIECE=<pairs>
// overrides it, read at each call.
inline size_t pair_piece_len(size_t m) {
  const size_t e = env_size("MSM_PAIRING_PIECE");
  if (e) return std::min(e, PAIR_PIECE_MAX);
  return std::min(std::max(m / PAIR_LANE_PAIRS, (size_t)1), PAIR_PIECE_MAX);
}

// One engine: the per-pair records of a chunk (the running point T, Q and the
// two factors of P), the partial Miller values (one per piece, and the value
// carried from one chunk into the next), the segment values, the five working
// values of the final exponentiation per segment, the verdict bytes, the plan
// of a chunk (two pinned slots with events of their own, one device copy), and
// for host memory staging lanes on the shared chunk pipe (chunk_pipe.hpp): P
// and Q up under one upload event, values and verdicts down.
class Pairing {
 public:
  static constexpr size_t P_AFF = 96, Q_AFF = 192, GT = 576, FP12S = 672, REC = 680;
  static constexpr int FE_SLOTS = 5;
  explicit Pairing(int device) : dev_(device), plan_lane_(device), pipe_(device) {}
  // dst[j] = E(segment j) for j < k, o = offsets (host, k + 1 values,
  // non-decreasing); with final_exp false the product of the Miller values.
  // p and q are both host or both device memory (src_dev) and are indexed from
  // pair 0.  dst (k values of 576 bytes, host or device) may be NULL when only
  // the verdicts are wanted; is_one: k host bytes or NULL (final_exp only).
  // `cs` orders the kernels.  Returns with the work queued on cs when dst is
  // device memory and is_one is NULL, otherwise with dst / is_one written.
  void run(hipStream_t cs, const void *p, const void *q, const size_t *offsets, size_t k, void *dst, uint8_t *is_one,
           bool final_exp, bool src_dev, bool dst_dev);
  // dst[i] = fe(src[i]) for i < n (blst Fp12 values)
  void run_final_exp(hipStream_t cs, const void *src, size_t n, void *dst, uint8_t *is_one, bool src_dev, bool dst_dev);
  size_t device_bytes() const {
    return rec_.bytes + part_.bytes + res_.bytes + ws_.bytes + carry_.bytes + plan_lane_.device_bytes() +
           st_dev_[0].bytes + st_dev_[1].bytes + in_p_.device_bytes() + in_q_.device_bytes() + out_.device_bytes();
  }
  int device() const { return dev_; }

 private:
  int dev_;
  DevBuf rec_, part_, res_, ws_, carry_, st_dev_[2];
  Stage in_p_, in_q_, out_, st_;  // st_: pinned only
  SegPlanner plan_;               // the plan of the chunk being queued (segments_plan.hpp)
  SegPlanLane plan_lane_;         // and its way to the device (point_segments.hpp)
  ChunkPipe pipe_;                // (last: it waits for the queued work before the buffers go)
  // values res_[0 .. n) -> dst / verdicts (device pointers, either may be NULL)
  void finish_kernels(hipStream_t s, size_t n, void *d_dst, uint8_t *d_st, bool final_exp);
};

// One tower operation on n values, device 0, synchronous (msm_test_fp12 of the C
// ABI, which checks the arguments; test entry, not on any product path).  raw:
// the 672-byte stored form in and out, else blst Fp12 values.  alias 1 / 2: the
// destination is operand a / b.
enum {
  TEST_FP12_MUL = 0,
  TEST_FP12_SQR = 1,
  TEST_FP12_SPARSE = 2,
  TEST_FP12_CONJ = 3,
  TEST_FP12_FROB = 4,
  TEST_FP12_INV = 5,
  TEST_FP12_CSQR = 6,
  TEST_FP12_LINE_DBL = 7,
  TEST_FP12_LINE_ADD = 8
};
void test_fp12(int op, int k, int alias, bool raw, const void *a, const void *b, void *out, size_t n);

}  // namespace msm
