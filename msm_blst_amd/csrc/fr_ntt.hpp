// fr_ntt.hpp -- bulk scalar-field arithmetic and batched NTTs on the GPU
// (msm_fr_ntt, msm_fr_op; kernels and orchestration in fr_ntt.hip, the pass
// plan in ntt_plan.hpp, the field layer in fr.hpp / host_fr.hpp).  Host-only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <map>

#include "chunk_pipe.hpp"
#include "host_fr.hpp"
#include "ntt_plan.hpp"

namespace msm {

// ops and flags: the values of include/msm_mi355x.h
enum { FR_ADD = 0, FR_SUB, FR_MUL, FR_SQR, FR_NEG, FR_INV, FR_FROM_SCALAR, FR_TO_SCALAR, FR_NOPS };
enum { FRF_INVERSE = 1, FRF_SRC_SCALAR = 2, FRF_DST_SCALAR = 4 };
enum { FRF_B_ONE = 1 };
inline bool fr_op_binary(int op) { return op == FR_ADD || op == FR_SUB || op == FR_MUL; }

// One engine: the pass buffers, the twiddle tables (cached by log_n), the
// levels of the inversion tree and, for host memory, staging lanes on the
// shared chunk pipe (chunk_pipe.hpp).  Elements are 32 bytes everywhere.
class FrNtt {
 public:
  static constexpr size_t EL = 32;
  explicit FrNtt(int device) : dev_(device), pipe_(device) {}
  // `batch` transforms of 2^log_n elements, src -> dst (host or device each;
  // dst == src allowed).  shift: NULL or a blst_scalar, 0 < s < r (checked by
  // the caller).  `cs` orders the kernels.  Device destination: returns with the
  // work queued on cs; host destination: returns with the data in dst.
  void ntt(hipStream_t cs, const void *src, void *dst, int log_n, size_t batch, const uint8_t *shift, int flags,
           bool src_dev, bool dst_dev);
  // dst[i] = a[i] op b[i] (b_one: b[0]); a and b on the same side
  void op(hipStream_t cs, int op, void *dst, const void *a, const void *b, size_t n, bool b_one, bool src_dev,
          bool dst_dev);
  size_t device_bytes() const;
  int device() const { return dev_; }

 private:
  struct Tables {  // omega_n^e for e < n / 2 as lo[e & (2^lb - 1)] hi[e >> lb], and omega_R^x = in[x << in_shift(R)]
    DevBuf buf;
    const uint32_t *lo = nullptr, *hi = nullptr, *in = nullptr;
    int lb = 0, in_log = 0;
  };
  int dev_;
  DevBuf ta_, tb_, lv_, sh_;
  std::map<int, Tables> tw_;
  Stage in_, inb_, out_;
  ChunkPipe pipe_;  // (last: it waits for the queued work before the buffers go)
  const Tables &tables(hipStream_t s, int log_n);
  void passes(hipStream_t s, const void *d_src, void *d_dst, int log_n, size_t batch, int flags, bool shifted);
  void op_kernels(hipStream_t s, int op, void *d_dst, const void *d_a, const void *d_b, size_t n, bool b_one);
};

// out[t] = mult base^t for t < count, as the constants c 2^261 mod r the kernels multiply
// by (canonical, 32 bytes each), queued on s: the power tables of the Fr engines
void fr_pow_table(hipStream_t s, uint32_t *out, size_t count, const hfr::Fr &base, const hfr::Fr &mult);

// register-resident Fr products per second on `device` (out[0]) and the ms spent (out[1])
void fr_probe(int device, double out[2]);

}  // namespace msm
