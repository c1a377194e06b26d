// kzg.hpp -- KZG commitments, openings and verification over one Lagrange-basis SRS
// (msm_kzg_*; kzg.cpp).  Host-only.  Nothing here is a kernel: the context owns an
// msm_ctx over the SRS and chains the library's own bulk calls on the caller's
// stream -- msm_fr_op / msm_fr_eval_quotient produce the scalars on the device,
// msm_ctx_mult_batch sums them, msm_points_msm_segments and msm_pairing_segments
// check the openings.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/msm_mi355x.h"
#include "engine.hpp"

namespace msm {

constexpr int KZG_MAX_LOG = 20;

class Kzg {
 public:
  // window: the bucket window of the Pippenger context
  Kzg(int device, int log_n, int flags, int window);
  ~Kzg();
  Kzg(const Kzg &) = delete;
  Kzg &operator=(const Kzg &) = delete;
  // Every call returns an MSM_* code; the message of a failed inner call stays in
  // msm_last_error().  HIP failures of the copies made here throw.
  int set_srs(const void *srs, bool on_device, const void *tau_g2, hipStream_t s);
  int commit(void *dst, const void *polys, size_t count, bool src_dev, bool dst_dev, hipStream_t s);
  int open(void *proofs, void *y, const void *polys, const void *z, size_t count, bool src_dev, bool dst_dev,
           hipStream_t s);
  // weights NULL: `count` verdicts, one per tuple.  Else nbatches verdicts over the tuples
  // bo[0] .. bo[nbatches] (bo a checked host array).
  int verify(uint8_t *ok, size_t *nfail, const void *commitments, const void *z, const void *y, const void *proofs,
             size_t count, const uint8_t *weights, size_t nbits, size_t stride, const size_t *bo, size_t nbatches,
             bool src_dev, hipStream_t s);
  int device() const { return dev_; }
  int log_n() const { return log_n_; }

 private:
  int dev_, log_n_, flags_;
  msm_ctx *ctx_ = nullptr;
  uint8_t g1_[96], neg_g2_[192], tau_g2_[192];
  DevBuf scal_, ybuf_, pts_, sc_, sums_, p_, q_;
  // the scalars at d_scalars (nb sets of n blst_scalar) summed over the SRS -> dst (affine)
  int sums(void *dst, const void *d_scalars, size_t nb, bool dst_dev, hipStream_t s);
};

}  // namespace msm
