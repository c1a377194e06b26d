// kzg.cpp -- the KZG context (kzg.hpp): commit, open and verify as chains of the
// library's bulk calls.
//
// verify.  With A_j = C_j - [y_j]G1 + [z_j]pi_j a tuple holds iff
//   e(A_j, -G2) e(pi_j, [tau]G2) = 1,
// and a batch with weights r_j iff the same holds for A = sum r_j A_j and B = sum r_j
// pi_j.  A_j is the MSM of the three points (C_j, G1, pi_j) by (r_j, -r_j y_j, r_j z_j):
// one segment of msm_points_msm_segments per tuple, or one segment of 3 len points per
// batch plus one of len points for B.  The three scalars of a tuple are Fr work done
// HERE ON THE HOST (host_fr.hpp; three products per tuple, against two Miller loops
// per check on the device); device-resident z and y are fetched for it.
#include "kzg.hpp"

#include <string.h>

#include <algorithm>
#include <stdexcept>

#include "fr_poly.hpp"
#include "host_fp.hpp"
#include "host_fr.hpp"

namespace msm {

namespace {
#define KZG_TRY(call)           \
  do {                          \
    const int rc_ = (call);     \
    if (rc_ != MSM_OK) return rc_; \
  } while (0)

constexpr size_t P1 = 96, P2 = 192, EL = 32;
constexpr size_t HOST_AFFINE_MAX = 1024;  // sums normalised on the host up to this many (about a microsecond each)

void copy2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t rows, bool src_dev, hipStream_t s) {
  if (!rows) return;
  if (src_dev) MSM_HIP_CHECK(hipMemcpy2DAsync(dst, dpitch, src, spitch, P1, rows, hipMemcpyDeviceToDevice, s));
  else MSM_HIP_CHECK(hipMemcpy2D(dst, dpitch, src, spitch, P1, rows, hipMemcpyHostToDevice));
}
}  // namespace

Kzg::Kzg(int device, int log_n, int flags, int window) : dev_(device), log_n_(log_n), flags_(flags) {
  if (msm_ctx_create(&ctx_, 1, device, window) != MSM_OK) throw std::runtime_error(msm_last_error());
  const hfp::Jac<hfp::Fp> g1 = hfp::g1_generator();
  const hfp::Jac<hfp::Fp2> g2 = hfp::g2_generator();
  const hfp::Aff<hfp::Fp> a1{g1.x, g1.y};
  const hfp::Aff<hfp::Fp2> a2{g2.x, hfp::neg(g2.y)};
  memcpy(g1_, &a1, P1);
  memcpy(neg_g2_, &a2, P2);
  memset(tau_g2_, 0, P2);
}

Kzg::~Kzg() { msm_ctx_destroy(ctx_); }

int Kzg::set_srs(const void *srs, bool on_device, const void *tau_g2, hipStream_t s) {
  memcpy(tau_g2_, tau_g2, P2);
  return msm_ctx_set_points(ctx_, srs, (size_t)1 << log_n_, on_device ? 1 : 0, s);
}

int Kzg::sums(void *dst, const void *d_scalars, size_t nb, bool dst_dev, hipStream_t s) {
  const size_t n = (size_t)1 << log_n_;
  std::vector<uint8_t> jac(nb * 144);
  KZG_TRY(msm_ctx_mult_batch(ctx_, jac.data(), static_cast<const byte *>(d_scalars), EL, n * EL, 255, nb, 1, s));
  if (nb > HOST_AFFINE_MAX) return msm_points_to_affine(1, dev_, dst, jac.data(), nb, 0, dst_dev ? 1 : 0, s);
  // not many sums: the device's batch inversion is a Fermat chain in Fp whatever the count
  // and its Jacobians come from the host anyway (a millisecond and more, measured); the
  // host's batch inversion takes microseconds
  std::vector<hfp::Aff<hfp::Fp>> aff(nb);
  hfp::to_affine_batch(aff.data(), reinterpret_cast<const hfp::Jac<hfp::Fp> *>(jac.data()), nb);
  if (!dst_dev) {
    memcpy(dst, aff.data(), nb * P1);
    return MSM_OK;
  }
  MSM_HIP_CHECK(hipMemcpyAsync(dst, aff.data(), nb * P1, hipMemcpyHostToDevice, s));
  MSM_HIP_CHECK(hipStreamSynchronize(s));
  return MSM_OK;
}

int Kzg::commit(void *dst, const void *polys, size_t count, bool src_dev, bool dst_dev, hipStream_t s) {
  DeviceGuard g(dev_);
  const size_t n = (size_t)1 << log_n_, per = std::min(count, std::max<size_t>(1, poly_chunk() >> log_n_));
  scal_.ensure(per * n * EL);
  for (size_t c0 = 0; c0 < count; c0 += per) {
    const size_t nb = std::min(per, count - c0);
    KZG_TRY(msm_fr_op(dev_, MSM_FR_TO_SCALAR, scal_.p, static_cast<const uint8_t *>(polys) + c0 * n * EL, nullptr,
                      nb * n, 0, src_dev ? 1 : 0, 1, s));
    KZG_TRY(sums(static_cast<uint8_t *>(dst) + c0 * P1, scal_.p, nb, dst_dev, s));
  }
  return MSM_OK;
}

int Kzg::open(void *proofs, void *y, const void *polys, const void *z, size_t count, bool src_dev, bool dst_dev,
              hipStream_t s) {
  DeviceGuard g(dev_);
  const size_t n = (size_t)1 << log_n_, per = std::min(count, std::max<size_t>(1, poly_chunk() >> log_n_));
  scal_.ensure(per * n * EL);
  ybuf_.ensure(per * EL);
  for (size_t c0 = 0; c0 < count; c0 += per) {
    const size_t nb = std::min(per, count - c0);
    // the quotient's scalars never leave the device; y comes back beside them
    KZG_TRY(msm_fr_eval_quotient(dev_, ybuf_.p, scal_.p, static_cast<const uint8_t *>(polys) + c0 * n * EL,
                                 static_cast<const uint8_t *>(z) + c0 * EL, (size_t)log_n_, nb,
                                 MSM_FR_DST_SCALAR | (flags_ & MSM_POLY_BITREV), src_dev ? 1 : 0, 1, s));
    MSM_HIP_CHECK(hipMemcpyAsync(static_cast<uint8_t *>(y) + c0 * EL, ybuf_.p, nb * EL,
                                 dst_dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
    KZG_TRY(sums(static_cast<uint8_t *>(proofs) + c0 * P1, scal_.p, nb, dst_dev, s));
  }
  if (!dst_dev) MSM_HIP_CHECK(hipStreamSynchronize(s));
  return MSM_OK;
}

int Kzg::verify(uint8_t *ok, size_t *nfail, const void *commitments, const void *z, const void *y,
                const void *proofs, size_t count, const uint8_t *weights, size_t nbits, size_t stride,
                const size_t *bo, size_t nbatches, bool src_dev, hipStream_t s) {
  DeviceGuard g(dev_);
  const bool weighted = weights != nullptr;
  const size_t one_batch[2] = {0, count};
  if (weighted && !bo) bo = one_batch, nbatches = 1;
  const size_t t0 = weighted ? bo[0] : 0, m = weighted ? bo[nbatches] - t0 : count;  // the tuples read
  const size_t nchk = weighted ? nbatches : count;
  const uint8_t *C = static_cast<const uint8_t *>(commitments) + t0 * P1;
  const uint8_t *PI = static_cast<const uint8_t *>(proofs) + t0 * P1;

  // ---- z, y on the host; the three scalars of every tuple ----
  std::vector<hfr::Fr> zy(2 * m);
  if (m) {
    const uint8_t *zs = static_cast<const uint8_t *>(z) + t0 * EL, *ys = static_cast<const uint8_t *>(y) + t0 * EL;
    if (src_dev) {
      MSM_HIP_CHECK(hipMemcpyAsync(zy.data(), zs, m * EL, hipMemcpyDeviceToHost, s));
      MSM_HIP_CHECK(hipMemcpyAsync(zy.data() + m, ys, m * EL, hipMemcpyDeviceToHost, s));
      MSM_HIP_CHECK(hipStreamSynchronize(s));
    } else {
      memcpy(zy.data(), zs, m * EL);
      memcpy(zy.data() + m, ys, m * EL);
    }
  }
  const size_t npts = 3 * m + (weighted ? m : 0);
  std::vector<uint8_t> sc(npts * EL), gens(m * P1);
  const size_t wb = (nbits + 7) / 8;
  for (size_t j = 0; j < m; ++j) {
    hfr::Fr r = hfr::ONE;
    if (weighted) {
      uint8_t w[32] = {0};
      memcpy(w, weights + (t0 + j) * stride, wb);
      if (nbits & 7) w[wb - 1] &= (uint8_t)((1u << (nbits & 7)) - 1);
      r = hfr::from_scalar(w);
    }
    uint8_t *o = sc.data() + 3 * j * EL;
    hfr::to_scalar(o, r);
    hfr::to_scalar(o + EL, hfr::neg(hfr::mul(r, zy[m + j])));
    hfr::to_scalar(o + 2 * EL, hfr::mul(r, zy[j]));
    if (weighted) memcpy(sc.data() + (3 * m + j) * EL, o, EL);
    memcpy(gens.data() + j * P1, g1_, P1);
  }

  // ---- the points (C_j, G1, pi_j) per tuple, then every pi_j again under weights ----
  pts_.ensure(std::max<size_t>(npts, 1) * P1);
  sc_.ensure(std::max<size_t>(npts, 1) * EL);
  uint8_t *pts = pts_.as<uint8_t>();
  copy2d(pts, 3 * P1, C, P1, m, src_dev, s);
  copy2d(pts + P1, 3 * P1, gens.data(), P1, m, false, s);
  copy2d(pts + 2 * P1, 3 * P1, PI, P1, m, src_dev, s);
  if (weighted) copy2d(pts + 3 * m * P1, P1, PI, P1, m, src_dev, s);
  if (npts) MSM_HIP_CHECK(hipMemcpy(sc_.p, sc.data(), npts * EL, hipMemcpyHostToDevice));
  const size_t nseg = weighted ? 2 * nbatches : count;
  std::vector<size_t> off(nseg + 1);
  if (weighted) {
    for (size_t b = 0; b <= nbatches; ++b) off[b] = 3 * (bo[b] - t0), off[nbatches + b] = 3 * m + (bo[b] - t0);
  } else {
    for (size_t j = 0; j <= count; ++j) off[j] = 3 * j;
  }
  sums_.ensure(nseg * P1);
  KZG_TRY(msm_points_msm_segments(1, dev_, sums_.p, pts, sc_.as<byte>(), off.data(), nseg, 255, EL, 0, 1, 1, s));

  // ---- per check the pairs (A, -G2), (B, [tau]G2) ----
  p_.ensure(nchk * 2 * P1);
  q_.ensure(nchk * 2 * P2);
  uint8_t *p = p_.as<uint8_t>();
  copy2d(p, 2 * P1, sums_.p, P1, nchk, true, s);
  if (weighted) copy2d(p + P1, 2 * P1, sums_.as<uint8_t>() + nbatches * P1, P1, nchk, true, s);
  else copy2d(p + P1, 2 * P1, pts + 2 * P1, 3 * P1, nchk, true, s);
  std::vector<uint8_t> qs(nchk * 2 * P2);
  std::vector<size_t> off2(nchk + 1);
  for (size_t c = 0; c < nchk; ++c) {
    memcpy(qs.data() + 2 * c * P2, neg_g2_, P2);
    memcpy(qs.data() + (2 * c + 1) * P2, tau_g2_, P2);
  }
  for (size_t c = 0; c <= nchk; ++c) off2[c] = 2 * c;
  MSM_HIP_CHECK(hipMemcpy(q_.p, qs.data(), qs.size(), hipMemcpyHostToDevice));
  return msm_pairing_segments(dev_, nullptr, ok, nfail, p, q_.p, off2.data(), nchk, 0, 1, 0, s);
}

}  // namespace msm
