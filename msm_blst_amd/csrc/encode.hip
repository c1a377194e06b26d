// encode.hip -- bulk ZCash encoding of BLS12-381 points on one MI355X
// (replaces a loop over ref src/e1.c:139-234 blst_p1_affine_compress /
// _affine_serialize / _compress / _serialize and the src/e2.c twins; DESIGN.md
// section 17).  The mirror of decode.hip.
//
//   k_encode   affine point i (blst layout) -> entry i: the stored limbs of a
//              coordinate (v 2^384) are used as they are, one product with 2^8
//              gives the plain integer v mod p, a conditional subtraction makes
//              it canonical, the 14 limbs of 28 bits are repacked into twelve
//              32-bit words, byte-swapped and stored big-endian; the sign flag
//              comes from the canonical y against (p-1)/2 (encode_dev.hpp)
//   Jacobians  the inversion tree of to_affine.hip with TA_JAC_ENC_C / _S: its
//              level-0 kernel forms x = X zi^2, y = Y zi^3 and runs the same
//              tail, so no affine array and no second pass
//
// Nothing is validated and nothing can fail: like the reference, the encoder
// writes whatever coordinates it is given.  Infinity is the all-zero affine
// point / a zero Z; limbs in [p, 2^384) encode their value mod p (the product
// with 2^8 reduces them, as the reference's from_fp does).
//
// G1 runs one lane per point, G2 one lane PAIR per point (fp2l.hpp): each lane
// encodes its own component, the imaginary lane writes the first 48 bytes of a
// coordinate and the flags.  Products per entry: 2 (G1), 4 (G2, both lanes),
// in either encoding; the Jacobian kinds add them to the tree's ~9.7.
#include "encode.hpp"

#include <cstring>

#include "encode_dev.hpp"
#include "to_affine.hpp"

#ifndef MSM_GROUP
#error "define MSM_GROUP (1 or 2)"
#endif

namespace msm {

// lane (pair) t < n: affine point t of src -> entry t of dst
template <int G, bool SER>
static __global__ void __launch_bounds__(128)
    k_encode(const uint64_t *__restrict__ src, size_t n, uint8_t *__restrict__ dst) {
  const size_t tt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int comp = G == 2 ? (int)(tt & 1) : 0;
  const size_t t = G == 2 ? tt >> 1 : tt;
  if (t >= n) return;  // whole pairs only
  const uint64_t *P = src + t * 12 * G;
  Fp x, y;
  unpack384(x, P + 6 * comp);
  unpack384(y, P + 6 * G + 6 * comp);
  // infinity: all 12 G limbs zero (X zero with Y non-zero is a finite entry)
  uint32_t nz = (fp_is_zero_exact(x) && fp_is_zero_exact(y)) ? 0u : 1u;
  if (G == 2) nz |= pair_swap(nz);
  enc_entry<G, SER>(dst + t * (SER ? 96 : 48) * G, x, y, nz == 0, comp);
}

// one chunk, device to device: n <= the chunk the level buffer was sized for
template <int G>
void Encode<G>::kernels(hipStream_t s, const void *d_src, void *d_dst, size_t n, bool jacobian, bool serialized) {
  if (jacobian) {
    ta_tree<G>(s, lv_.p, lv_.bytes, serialized ? TA_JAC_ENC_S : TA_JAC_ENC_C, d_src, d_dst, n);
    return;
  }
  const unsigned B = 128;
  const dim3 grid(nblk(n * G, B));
  if (serialized)
    hipLaunchKernelGGL((k_encode<G, true>), grid, dim3(B), 0, s, static_cast<const uint64_t *>(d_src), n,
                       static_cast<uint8_t *>(d_dst));
  else
    hipLaunchKernelGGL((k_encode<G, false>), grid, dim3(B), 0, s, static_cast<const uint64_t *>(d_src), n,
                       static_cast<uint8_t *>(d_dst));
  MSM_HIP_CHECK(hipGetLastError());
}

template <int G>
void Encode<G>::run(hipStream_t cs, const void *src, void *dst, size_t n, bool jacobian, bool serialized, bool src_dev,
                    bool dst_dev) {
  if (!n) return;
  DeviceGuard g(dev_);
  const size_t PT = jacobian ? JAC : AFF, ENC = serialized ? 2 * COMP : COMP;
  const size_t C = std::min(n, enc_chunk());
  if (jacobian) lv_.ensure(ta_level_elems(C) * ELEM);
  if (!src_dev) in_.ensure(C * PT);
  if (!dst_dev) out_.ensure(C * ENC);
  pipe_.begin(cs);  // the level buffer of the previous call
  auto pend = pipe_.pending([&](int slot, size_t off, size_t cnt) {
    memcpy(static_cast<uint8_t *>(dst) + off * ENC, out_.pin[slot], cnt * ENC);
  });
  size_t k = 0;
  for (size_t c0 = 0; c0 < n; c0 += C, ++k) {
    const size_t cnt = std::min(C, n - c0);
    const int slot = (int)(k & 1);
    const void *d_src;
    void *d_dst;
    if (!src_dev) {
      pipe_.upload(cs, slot, [&] { memcpy(in_.pin[slot], static_cast<const uint8_t *>(src) + c0 * PT, cnt * PT); },
                   {{in_, slot, cnt * PT}});
      d_src = in_.dev[slot].p;
    } else {
      d_src = static_cast<const uint8_t *>(src) + c0 * PT;
    }
    if (!dst_dev) {
      pipe_.out_open(cs, slot);
      d_dst = out_.dev[slot].p;
    } else {
      d_dst = static_cast<uint8_t *>(dst) + c0 * ENC;
    }
    kernels(cs, d_src, d_dst, cnt, jacobian, serialized);
    pipe_.computed(cs, slot);
    if (!dst_dev) pipe_.download(cs, slot, pend, c0, cnt, {{out_, slot, cnt * ENC}});
  }
  pend.flush();
  pipe_.finish(cs);
}

template class Encode<MSM_GROUP>;

}  // namespace msm
