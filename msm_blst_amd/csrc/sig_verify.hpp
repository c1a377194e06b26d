// sig_verify.hpp -- bulk BLS signature verification on the GPU (replaces a host
// loop over the reference's blst_core_verify_pk_in_g{1,2} and its
// blst_pairing_chk_n_aggr_* / chk_n_mul_n_aggr_* / commit / finalverify
// sequences: ref src/aggregate.c:98-339, 390-501, 625-673; kernels and
// orchestration in sig_verify.hip, the host plan in sig_plan.hpp, DESIGN.md
// section 24).  This header is host-only.
//
// Every check is the equation  e(-g, S_j) prod_i e(PK'_i, H_i) == 1  (min-sig:
// the sides swapped).  The engine orchestrates the other bulk engines on one
// stream, with every intermediate in device memory: Decode (encoded inputs),
// the screen, PointSegments (sums of keys, sums of signatures), PointsMult
// (the weights of a batch, on the G1 side of every tuple), HashToCurve and
// Pairing::run with one segment per check, verdicts only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <memory>
#include <vector>

#include "chunk_pipe.hpp"
#include "decode.hpp"
#include "hash_to_curve.hpp"
#include "pairing.hpp"
#include "point_segments.hpp"
#include "points_mult.hpp"
#include "sig_plan.hpp"

namespace msm {

// What one call verifies.  keys, sigs, the messages and the scalars are in one
// memory space (src_dev); o, pk and the template are host memory.
struct SigCall {
  int mode = SIG_VERIFY;
  bool encoded = false;  // keys and signatures are compressed ZCash entries
  int count = 2;         // field elements per message: 2 hash, 1 encode
  const void *keys = nullptr, *sigs = nullptr;
  const uint8_t *scalars = nullptr;  // SIG_BATCH; NULL (or nbits 0): unweighted
  int nbits = 0;
  size_t stride = 0;
  H2cMsgs m;
  const H2cTemplate *tmpl = nullptr;
  const size_t *o = nullptr;   // SIG_AGGREGATE, SIG_BATCH: k + 1 offsets
  const size_t *pk = nullptr;  // SIG_VERIFY: k + 1 offsets of the key sets, or NULL
  size_t k = 0;                // checks
  bool src_dev = false;
};

// PKG: the group of the public keys (1: min-pk, 2: min-sig)
template <int PKG>
class SigVerify {
 public:
  static constexpr int SG = 3 - PKG;  // the group of the signatures and the hashes
  static constexpr size_t KAFF = 96 * PKG, SAFF = 96 * SG, KENC = 48 * PKG, SENC = 48 * SG;
  explicit SigVerify(int device)
      : dev_(device), dec_k_(device), dec_s_(device), sum_k_(device), sum_s_(device), mult_(device), h2c_(device),
        pair_(device), ev_codes_(device), pipe_(device) {}
  // status[j] for j < k (host memory); returns with them written
  void run(hipStream_t cs, const SigCall &c, uint8_t *status);
  size_t device_bytes() const {
    size_t b = dec_k_.device_bytes() + dec_s_.device_bytes() + sum_k_.device_bytes() + sum_s_.device_bytes() +
               mult_.device_bytes() + h2c_.device_bytes() + pair_.device_bytes();
    for (const DevBuf *d : {&kaff_, &saff_, &kcode_, &scode_, &cc_, &late_, &ksum_, &ssum_, &hash_, &g1w_, &ent_, &p_, &q_})
      b += d->bytes;
    return b + in_k_.device_bytes() + in_s_.device_bytes() + in_w_.device_bytes();
  }
  int device() const { return dev_; }

 private:
  int dev_;
  Decode<PKG> dec_k_;
  Decode<SG> dec_s_;
  PointSegments<PKG> sum_k_;
  PointSegments<SG> sum_s_;
  PointsMult<1> mult_;
  HashToCurve<SG> h2c_;
  Pairing pair_;
  // decoded keys and signatures, their codes, the codes of the checks, the late
  // codes (a key sum that is infinite), the key sums, the signature sums, the
  // hashes, the weighted G1 side, the rows' plan, the P and Q arrays
  DevBuf kaff_, saff_, kcode_, scode_, cc_, late_, ksum_, ssum_, hash_, g1w_, ent_, p_, q_;
  Stage in_k_, in_s_, in_w_;     // keys, signatures and scalars of a chunk in host memory
  Stage codes_, plan_;            // pinned only: codes down, the plan and the checks' codes up
  SigChunkPlan pl_;
  std::vector<uint8_t> cch_;
  EventPair ev_codes_;  // [0]: the codes of the chunk's points have reached their pinned slot
  ChunkPipe pipe_;      // (last: it waits for the queued work before the buffers go)
};

// The screen alone: in_group[i] = blst_p{1,2}_affine_in_g{1,2}(P_i)
template <int G>
class GroupScreen {
 public:
  static constexpr size_t AFF = 96 * G;
  explicit GroupScreen(int device) : dev_(device), pipe_(device) {}
  // n affine points at src (host or device) -> n host bytes, 1 in the group (infinity passes)
  void run(hipStream_t cs, const void *src, uint8_t *in_group, size_t n, bool src_dev);
  size_t device_bytes() const { return in_.device_bytes() + code_.bytes; }
  int device() const { return dev_; }

 private:
  int dev_;
  DevBuf code_;
  Stage in_, out_;  // out_: pinned only
  ChunkPipe pipe_;
};

}  // namespace msm
