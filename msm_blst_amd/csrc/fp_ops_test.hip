// fp_ops_test.hip -- the kernels of msm_test_fp_ops (include/msm_mi355x.h,
// fp_ops_test.hpp; tests/test_gpu_fp_ops.py): ONE operation of fp.hpp, fp2l.hpp
// or ec.hpp per launch, on raw stored limbs, so the caller puts each operand at
// the bound of its range class and reads the representative that comes back.
// The host build of the same headers (tests/test_fp_bounds.py) shares none of
// what differs on the device: the v_mad_u64_u32 columns, pair_swap as a DPP move
// under a partial EXEC mask, the pins of MulChain, the selects, the register
// allocation.
//
// One kernel per (field kind, column form, op), so each holds the registers of
// its own op only and none spills (tests/test_kernel_resources.py).  Lane
// mapping as in the product kernels: Fp and Fp2 one lane per value, Fp2L value i
// on lanes 2i (c0) and 2i + 1 (c1) of a 64-thread block; the last block runs
// with whole pairs (lanes) missing.  The cooperative add is not here: it runs
// through the reductions' own kernels (test_coop_pair_add, ches.hip).
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include "ec.hpp"
#include "engine.hpp"
#include "fp2l.hpp"
#include "fp_ops_test.hpp"

namespace msm {
namespace {

// stored element <-> registers; comp: the lane's component (Fp2L), else unused
__device__ __forceinline__ void t_ld(Fp &r, const uint32_t *p) {
#pragma unroll
  for (int i = 0; i < NL; ++i) r.v[i] = p[i];
}
__device__ __forceinline__ void t_st(uint32_t *p, const Fp &a) {
#pragma unroll
  for (int i = 0; i < NL; ++i) p[i] = a.v[i];
}
__device__ __forceinline__ void t_ld(Fp &r, const uint32_t *p, int) { t_ld(r, p); }
__device__ __forceinline__ void t_st(uint32_t *p, const Fp &a, int) { t_st(p, a); }
__device__ __forceinline__ void t_ld(Fp2 &r, const uint32_t *p, int) {
  t_ld(r.c0, p);
  t_ld(r.c1, p + NL);
}
__device__ __forceinline__ void t_st(uint32_t *p, const Fp2 &a, int) {
  t_st(p, a.c0);
  t_st(p + NL, a.c1);
}
__device__ __forceinline__ void t_ld(Fp2L &r, const uint32_t *p, int comp) { t_ld(r.c, p + comp * NL); }
__device__ __forceinline__ void t_st(uint32_t *p, const Fp2L &a, int comp) { t_st(p + comp * NL, a.c); }

template <class F>
struct Words {
  static constexpr int value = sizeof(F) / 4;
};
template <>
struct Words<Fp2L> {
  static constexpr int value = 2 * NL;
};
template <class F>
struct Lanes {
  static constexpr int value = 1;
};
template <>
struct Lanes<Fp2L> {
  static constexpr int value = 2;
};

// fp_sub<K> per component (fp.hpp names K = 4 and 16 only)
template <int K>
__device__ __forceinline__ void t_sub(Fp &r, const Fp &a, const Fp &b) { fp_sub<K>(r, a, b); }
template <int K>
__device__ __forceinline__ void t_sub(Fp2 &r, const Fp2 &a, const Fp2 &b) {
  fp_sub<K>(r.c0, a.c0, b.c0);
  fp_sub<K>(r.c1, a.c1, b.c1);
}
template <int K>
__device__ __forceinline__ void t_sub(Fp2L &r, const Fp2L &a, const Fp2L &b) { fp_sub<K>(r.c, a.c, b.c); }

// value index and component of this lane; false: the lane has no value
template <class F>
__device__ __forceinline__ bool t_lane(size_t n, size_t &i, int &comp) {
  const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
  i = t / Lanes<F>::value;
  comp = (int)(t % Lanes<F>::value);
  return i < n;  // Fp2L: whole pairs only
}

// field ops 0 .. 15: in n x NIN elements, out n elements
template <class F, class CF, int OP>
__global__ void __launch_bounds__(64) k_fpt_field(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t n) {
  constexpr int W = Words<F>::value;
  constexpr int NIN = OP == TEST_F_MUL_SUB || OP == TEST_F_MUL_SUB_BS ? 4
                      : OP == TEST_F_SUB_2X                            ? 3
                      : OP == TEST_F_ONE                               ? 0
                      : OP <= TEST_F_MUL_BS || (OP >= TEST_F_ADD && OP <= TEST_F_SUB32) ? 2
                                                                                        : 1;
  size_t i;
  int comp;
  if (!t_lane<F>(n, i, comp)) return;
  F x[NIN > 0 ? NIN : 1], r;
#pragma unroll
  for (int j = 0; j < NIN; ++j) t_ld(x[j], in + (i * NIN + j) * W, comp);
  if constexpr (OP == TEST_F_MUL) f_mul(r, x[0], x[1], CF{});
  else if constexpr (OP == TEST_F_MUL_BS) f_mul_bs(r, x[0], x[1], CF{});
  else if constexpr (OP == TEST_F_SQR) f_sqr(r, x[0], CF{});
  else if constexpr (OP == TEST_F_MUL_SUB) f_mul_sub(r, x[0], x[1], x[2], x[3], CF{});
  else if constexpr (OP == TEST_F_MUL_SUB_BS) f_mul_sub_bs(r, x[0], x[1], x[2], x[3], CF{});
  else if constexpr (OP == TEST_F_ADD) f_add(r, x[0], x[1]);
  else if constexpr (OP == TEST_F_SUB4) f_sub4(r, x[0], x[1]);
  else if constexpr (OP == TEST_F_SUB16) f_sub16(r, x[0], x[1]);
  else if constexpr (OP == TEST_F_SUB8) t_sub<8>(r, x[0], x[1]);
  else if constexpr (OP == TEST_F_SUB32) t_sub<32>(r, x[0], x[1]);
  else if constexpr (OP == TEST_F_SUB_2X) f_sub_2x(r, x[0], x[1], x[2]);
  else if constexpr (OP == TEST_F_NEG4) f_neg4(r, x[0]);
  else if constexpr (OP == TEST_F_MUL3) f_mul3(r, x[0]);
  else if constexpr (OP == TEST_F_NORM) {
    r = x[0];
    f_norm(r);
  } else if constexpr (OP == TEST_F_NRED) {
    r = x[0];
    f_nred(r);
  } else {
    static_assert(OP == TEST_F_ONE, "field op");
    f_one(r);
  }
  t_st(out + i * W, r, comp);
}

// the zero tests: one word per value (Fp2L: written by the even lane; the verdict
// is the pair's, both lanes compute it)
template <class F, int OP>
__global__ void __launch_bounds__(64) k_fpt_zero(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, size_t n) {
  size_t i;
  int comp;
  if (!t_lane<F>(n, i, comp)) return;
  F x;
  t_ld(x, in + i * Words<F>::value, comp);
  const bool z = OP == TEST_F_IS_ZERO_EXACT ? f_is_zero_exact(x) : f_is_zero_S(x);
  if (comp == 0) out[i] = z ? 1u : 0u;
}

// the Fp-only ops
template <class CF, int OP>
__global__ void __launch_bounds__(64)
    k_fpt_fp(const uint32_t *__restrict__ in, const uint32_t *__restrict__ flags, uint32_t *__restrict__ out, size_t n) {
  constexpr int NIN = OP == TEST_FP_MUL2 ? 4 : OP == TEST_FP_MUL4 ? 8 : 1;
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  Fp x[NIN], r;
#pragma unroll
  for (int j = 0; j < NIN; ++j) t_ld(x[j], in + (i * NIN + j) * NL);
  if constexpr (OP == TEST_FP_MUL2) fp_mul2(r, x[0], x[1], x[2], x[3], CF{});
  else if constexpr (OP == TEST_FP_MUL4) fp_mul4(r, x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], CF{});
  else if constexpr (OP == TEST_FP_RED) {
    r = x[0];
    fp_red(r);
  } else if constexpr (OP == TEST_FP_CNEG4) fp_cneg4(r, x[0], (flags[i] & TEST_FLAG_NEG) != 0);
  else if constexpr (OP == TEST_FP_CANON) fp_canon(r, x[0]);
  else {
    static_assert(OP == TEST_FP_CSUB_P, "Fp op");
    r = x[0];
    fp_csub_p(r);
  }
  t_st(out + i * NL, r);
}

// the point formulas: points as stored (x, y, zzz, zz)
template <class F>
__device__ __forceinline__ void t_ld_xyzz(Xyzz<F> &r, const uint32_t *p, int comp) {
  constexpr int W = Words<F>::value;
  t_ld(r.x, p, comp);
  t_ld(r.y, p + W, comp);
  t_ld(r.zzz, p + 2 * W, comp);
  t_ld(r.zz, p + 3 * W, comp);
}
// The one-lane Fp2 (28 registers an element) reads its operands where the formula
// uses them, from memory, and xyzz_dbl writes its result there: with every
// operand loaded up front those two kernels spilled VGPRs.  The stored layout is
// the struct's (x, y, zzz, zz; c0 | c1).
// xyzz_madd takes its affine operand from memory over Fp as well.  Loaded into
// registers up front, the MulChain madd with a run-time acc_affine was compiled
// wrongly (boundary execution on the device): at the join of the
// skipped and the computed U2 / S2, P = U2 - X1 was written over nine limbs of
// S2 before R = S2 - Y1 read them, so x and y came out wrong and the doubling
// branch was never taken.  k_accumulate<1>, the one product kernel with that
// madd, does not have the overlap in its code.
template <class F, class CF, int OP>
__global__ void __launch_bounds__(64)
    k_fpt_curve(const uint32_t *__restrict__ in, const uint32_t *__restrict__ flags, uint32_t *__restrict__ out, size_t n) {
  constexpr int W = Words<F>::value;
  constexpr bool mem = std::is_same<F, Fp2>::value, mem_aff = !std::is_same<F, Fp2L>::value;
  size_t i;
  int comp;
  if (!t_lane<F>(n, i, comp)) return;
  Xyzz<F> acc;
  if constexpr (OP == TEST_XYZZ_MADD) {
    const uint32_t *p = in + i * 6 * W;
    const uint32_t fl = flags[i];
    const bool first = (fl & TEST_FLAG_ACC_AFFINE) != 0, neg = (fl & TEST_FLAG_NEG) != 0;
    if (first) {  // a bucket's first entry, as the accumulation builds it
      Aff<F> q;
      t_ld(q.x, p, comp);
      t_ld(q.y, p + W, comp);
      xyzz_from_aff(acc, q, (fl & TEST_FLAG_ACC_NEG) != 0);
    } else {
      t_ld_xyzz(acc, p, comp);
    }
    if constexpr (mem_aff) {
      xyzz_madd<F, CF>(acc, *reinterpret_cast<const Aff<F> *>(p + 4 * W), neg, first);
    } else {
      Aff<F> a;
      t_ld(a.x, p + 4 * W, comp);
      t_ld(a.y, p + 5 * W, comp);
      xyzz_madd<F, CF>(acc, a, neg, first);
    }
  } else if constexpr (OP == TEST_XYZZ_DBL) {
    if constexpr (mem) {
      xyzz_dbl<F, CF>(*reinterpret_cast<Xyzz<F> *>(out + i * 4 * W), *reinterpret_cast<const Xyzz<F> *>(in + i * 4 * W));
      return;
    } else {
      t_ld_xyzz(acc, in + i * 4 * W, comp);
      const Xyzz<F> a = acc;  // as the doubling branches of ec.hpp call it
      xyzz_dbl<F, CF>(acc, a);
    }
  } else {
    Xyzz<F> b;
    t_ld_xyzz(acc, in + i * 8 * W, comp);
    t_ld_xyzz(b, in + (i * 8 + 4) * W, comp);
    if constexpr (OP == TEST_XYZZ_ADD) xyzz_add<F, AddRegrouped<F>::value, CF>(acc, b);
    else xyzz_add_u1s1<F, CF>(acc, b);
  }
  uint32_t *o = out + i * 4 * W;
  t_st(o, acc.x, comp);
  t_st(o + W, acc.y, comp);
  t_st(o + 2 * W, acc.zzz, comp);
  t_st(o + 3 * W, acc.zz, comp);
}

template <int LO, int... I, class Fn>
bool op_case(int op, std::integer_sequence<int, I...>, Fn fn) {
  return ((op == LO + I ? (fn(std::integral_constant<int, LO + I>{}), true) : false) || ...);
}
// fn(integral_constant<int, op>) for LO <= op <= HI
template <int LO, int HI, class Fn>
bool by_op(int op, Fn fn) {
  return op_case<LO>(op, std::make_integer_sequence<int, HI - LO + 1>{}, fn);
}

template <class F, class CF>
void launch(int op, const uint32_t *in, const uint32_t *flags, uint32_t *out, size_t n) {
  const dim3 grid(nblk(n * Lanes<F>::value, 64)), block(64);
  // MulChain: only the ops that have the form (the caller has checked op against it)
  constexpr bool chain = std::is_same<CF, MulChain>::value;
  auto field_op = [&](auto o) {
    hipLaunchKernelGGL((k_fpt_field<F, CF, decltype(o)::value>), grid, block, 0, 0, in, out, n);
  };
  bool ok = by_op<TEST_F_MUL, TEST_F_MUL_SUB>(op, field_op);
  // fp.hpp has no f_mul_sub_bs over the one-lane Fp2 (its add is the u1s1 form, ec.hpp)
  if constexpr (!std::is_same<F, Fp2>::value) ok = ok || by_op<TEST_F_MUL_SUB_BS, TEST_F_MUL_SUB_BS>(op, field_op);
  if constexpr (!chain) ok = ok || by_op<TEST_F_ADD, TEST_F_ONE>(op, field_op);
  if constexpr (!chain)
    ok = ok || by_op<TEST_F_IS_ZERO_EXACT, TEST_F_IS_ZERO_S>(op, [&](auto o) {
           hipLaunchKernelGGL((k_fpt_zero<F, decltype(o)::value>), grid, block, 0, 0, in, out, n);
         });
  if constexpr (std::is_same<F, Fp>::value)
    ok = ok || by_op<TEST_FP_MUL2, chain ? TEST_FP_MUL4 : TEST_FP_CSUB_P>(op, [&](auto o) {
           hipLaunchKernelGGL((k_fpt_fp<CF, decltype(o)::value>), grid, block, 0, 0, in, flags, out, n);
         });
  ok = ok || by_op<TEST_XYZZ_MADD, TEST_XYZZ_DBL>(op, [&](auto o) {
         hipLaunchKernelGGL((k_fpt_curve<F, CF, decltype(o)::value>), grid, block, 0, 0, in, flags, out, n);
       });
  if (!ok) throw std::runtime_error("test_fp_ops: no kernel for this field / op");
  MSM_HIP_CHECK(hipGetLastError());
}

}  // namespace

void test_fp_ops(int field, int form, int op, const uint32_t *in, const uint32_t *flags, uint32_t *out, size_t n,
                 size_t cap) {
  const TestFpOp *d = test_fp_op(op);
  if (!n || !d) return;
  DeviceGuard g(0);
  const size_t w = test_fp_words(field) * 4;  // bytes of an element
  const size_t in_bytes = n * d->nin * w, out_bytes = cap * (d->nout ? d->nout * w : 4);
  DevBuf din, dfl, dout;
  if (in_bytes) {
    din.ensure(in_bytes);
    MSM_HIP_CHECK(hipMemcpy(din.p, in, in_bytes, hipMemcpyHostToDevice));
  }
  if (d->flags) {
    dfl.ensure(n * 4);
    MSM_HIP_CHECK(hipMemcpy(dfl.p, flags, n * 4, hipMemcpyHostToDevice));
  }
  dout.ensure(out_bytes);
  MSM_HIP_CHECK(hipMemcpy(dout.p, out, out_bytes, hipMemcpyHostToDevice));
  const uint32_t *I = din.as<uint32_t>(), *FL = dfl.as<uint32_t>();
  uint32_t *O = dout.as<uint32_t>();
  if (field == TEST_FIELD_FP) {
    if (form == TEST_FORM_CHAIN) launch<Fp, MulChain>(op, I, FL, O, n);
    else launch<Fp, MulSplit>(op, I, FL, O, n);
  } else if (field == TEST_FIELD_FP2) {
    launch<Fp2, MulSplit>(op, I, FL, O, n);
  } else {
    launch<Fp2L, MulSplit>(op, I, FL, O, n);
  }
  MSM_HIP_CHECK(hipDeviceSynchronize());
  MSM_HIP_CHECK(hipMemcpy(out, dout.p, out_bytes, hipMemcpyDeviceToHost));
}

}  // namespace msm
