// pairing.hip -- bulk pairings for BLS12-381 on one MI355X (replaces a host loop
// over the reference's blst_miller_loop / blst_fp12_mul / blst_final_exp: ref
// src/pairing.c:181-262 and 371-404, src/fp12_tower.c).
//
// The host cuts the pairs into pieces of at most L consecutive pairs of one
// segment (segments_plan.hpp); one lane pair (fp2l.hpp, fp12l.hpp) runs the
// Miller loop of one piece:
//   k_pair_init       pair i -> its record: T = Q (Jacobian, Z = 1), Q, -2 x_P,
//                     2 y_P and the skip flag (P or Q the all-zero point)
//   k_pair_miller     piece t: f = 1; over the bits of |z| from the top, f = f^2
//                     once per step and piece, then per pair of the piece the
//                     doubling (and on a set bit the addition) of T with its line
//                     and f = f line (sparse); T is reloaded from and parked in
//                     the record.  A skipped pair multiplies by the line (1, 0, 0):
//                     a select that is the same in both lanes of the pair.  The
//                     conjugate (z < 0) of the piece's value is stored.
//   k_pair_merge      the partial values of one segment lie side by side; a
//                     strided pairwise tree multiplies them (the shape of k_ps_merge)
//   k_pair_gather     the value of every segment that ends in this chunk (one for
//                     an empty segment), side by side
//   k_pair_fe_inv     value t: 1 / f, through the norms down to one Fp inversion
//   k_pair_final_exp  value t: the easy part (conjugate, the inverse, Frobenius
//                     2), the hard part on cyclotomic squarings with the reference's
//                     chain (its exponent is pinned by the tests), canonical blst
//                     bytes and the is_one byte; with an empty program it only
//                     stores the bytes (MSM_PAIRING_MILLER_ONLY)
//   k_pair_load       blst Fp12 values -> stored internal form (msm_fp12_final_exp)
//
// The raw Miller value is not pinned to the reference's bytes, only its final
// exponentiation is; the line functions here are the Jacobian doubling
// dbl-2009-alnr and mixed addition madd-2007-bl with the lines of eprint
// 2010/354, the factors -2 x_P and 2 y_P applied to the line afterwards.
//
// Values at rest (f, the five working values of the final exponentiation, T) live
// in HBM and are touched only by the lane pair that owns them, each lane its own
// component: no barrier, no LDS, and no Fp12 value held in registers across an
// operation (only the cyclotomic squarings of a run keep theirs).
//
// A chunk boundary may fall inside a segment: the product of the open segment
// so far is carried into the next chunk as one more partial, in front of that
// chunk's pieces.  A segment is written once it is complete.
#include "pairing.hpp"

#include <cstring>

#include "fp12l.hpp"
#include "pm_common.hpp"

namespace msm {

struct PairRec {
  Fp2 X, Y, Z;  // T
  Fp2 qx, qy;   // Q
  Fp px, py;    // -2 x_P, 2 y_P
  uint32_t skip, pad;
};
static_assert(sizeof(PairRec) == Pairing::REC && sizeof(Fp12S) == Pairing::FP12S, "stored sizes");
static_assert(sizeof(SegMeta) == 16, "plan entry");

constexpr uint64_t PAIR_Z_ABS = 0xd201000000010000ull;  // the curve parameter is -|z|

#define PAIR_LANE()                                                         \
  const size_t tt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;          \
  const int comp = (int)(tt & 1);                                           \
  const size_t t = tt >> 1

// lane pair t < n: rec[t] from P_t (96 B) and Q_t (192 B), blst affine
static __global__ void __launch_bounds__(128)
    k_pair_init(const uint64_t *__restrict__ p, const uint64_t *__restrict__ q, size_t n, PairRec *__restrict__ rec) {
  PAIR_LANE();
  if (t >= n) return;  // whole pairs only
  Fp x, y;
  fp_from_blst(x, p + t * 12);
  fp_from_blst(y, p + t * 12 + 6);
  Fp2L qx, qy, one;
  fp_from_blst(qx.c, q + t * 24 + 6 * comp);
  fp_from_blst(qy.c, q + t * 24 + 12 + 6 * comp);
  const bool pz = fp_is_zero_exact(x) && fp_is_zero_exact(y);
  const bool qzx = f_is_zero_exact(qx), qzy = f_is_zero_exact(qy);
  const bool skip = pz || (qzx && qzy);  // the same in both lanes
  Fp px, py;
  fp_add(px, x, x);
  fp_nred(px);
  fp_neg<4>(px, px);
  fp_nred(px);
  fp_add(py, y, y);
  fp_nred(py);
  f_one(one);
  PairRec *r = &rec[t];
  st_comp(&r->X, qx.c, comp);
  st_comp(&r->Y, qy.c, comp);
  st_comp(&r->Z, one.c, comp);
  st_comp(&r->qx, qx.c, comp);
  st_comp(&r->qy, qy.c, comp);
  if (comp == 0) {
    pm_st(&r->px, px, 0);
    pm_st(&r->py, py, 0);
    r->skip = skip ? 1u : 0u;
    r->pad = 0;
  }
}

// (pair_line_dbl / pair_line_add, the two line functions: fp12l.hpp)

// lane pair t < npieces: out[t] = conj(prod over the pairs of piece t of the Miller function)
static __global__ void __launch_bounds__(128)
    k_pair_miller(PairRec *__restrict__ rec, const SegMeta *__restrict__ meta, Fp12S *__restrict__ out, size_t npieces) {
  PAIR_LANE();
  if (t >= npieces) return;  // whole pairs only
  const uint32_t s0 = meta[t].start, cnt = meta[t].count;  // the same in both lanes of a pair
  Fp12S *f = &out[t];
  t_one12(f, comp);
#pragma unroll 1
  for (int b = 62; b >= 0; --b) {
    if (b != 62) t_sqr12(f, f, comp);
    const int nph = (int)((PAIR_Z_ABS >> b) & 1) + 1;  // uniform: the doubling, and on a set bit the addition
#pragma unroll 1
    for (int ph = 0; ph < nph; ++ph) {
#pragma unroll 1
      for (uint32_t i = 0; i < cnt; ++i) {
        PairRec *r = rec + s0 + i;
        Fp2L X, Y, Z, l0, l1, l2;
        ld_comp(X.c, &r->X, comp);
        ld_comp(Y.c, &r->Y, comp);
        ld_comp(Z.c, &r->Z, comp);
        if (ph == 0) {
          pair_line_dbl(X, Y, Z, l0, l1, l2);
        } else {
          Fp2L qx, qy;
          ld_comp(qx.c, &r->qx, comp);
          ld_comp(qy.c, &r->qy, comp);
          pair_line_add(X, Y, Z, qx, qy, l0, l1, l2);
        }
        st_comp(&r->X, X.c, comp);
        st_comp(&r->Y, Y.c, comp);
        st_comp(&r->Z, Z.c, comp);
        Fp k;
        pm_ld(k, &r->px, 0);
        t_scale(l1, l1, k);
        pm_ld(k, &r->py, 0);
        t_scale(l2, l2, k);
        const bool skip = r->skip != 0;  // the same in both lanes: the line becomes one
        Fp2L one, zero;
        f_one(one);
        f_zero(zero);
        t_sel(l0, skip, one);
        t_sel(l1, skip, zero);
        t_sel(l2, skip, zero);
        t_mul12_sparse(f, f, l0, l1, l2, comp);
      }
    }
  }
  t_conj12(f, f, comp);
}

// lane pair t < np: one step of the pairwise tree over the run of partial t
static __global__ void __launch_bounds__(128)
    k_pair_merge(Fp12S *__restrict__ part, const SegMeta *__restrict__ meta, size_t np, uint32_t step) {
  PAIR_LANE();
  if (t >= np) return;  // whole pairs only
  const uint32_t rel = meta[t].rel, len = meta[t].len;  // the same in both lanes of a pair
  if ((rel & (2 * step - 1)) != 0 || rel + step >= len) return;
  t_mul12(&part[t], &part[t], &part[t + step], comp);
}

// lane pair t < nseg: res[t] = part[src[t]], or one where src[t] is ~0
static __global__ void __launch_bounds__(128)
    k_pair_gather(const Fp12S *__restrict__ part, const uint32_t *__restrict__ src, Fp12S *__restrict__ res,
                  size_t nseg) {
  PAIR_LANE();
  if (t >= nseg) return;
  const uint32_t s = src[t];
  if (s == ~0u) {
    t_one12(&res[t], comp);
  } else {
    F12L a;
    t_ld12(a, &part[s], comp);
    t_st12(&res[t], a, comp);
  }
}

// lane pair t < n: res[t] = the blst Fp12 value at src + 72 t
static __global__ void __launch_bounds__(128)
    k_pair_load(const uint64_t *__restrict__ src, size_t n, Fp12S *__restrict__ res) {
  PAIR_LANE();
  if (t >= n) return;
#pragma unroll 1
  for (int j = 0; j < 6; ++j) {
    Fp c;
    fp_from_blst(c, src + t * 72 + j * 12 + 6 * comp);
    st_comp(&res[t].c[j], c, comp);
  }
}

// ---- the final exponentiation as a program over stored values ----
// One instruction: op | d << 4 | a << 8 | b << 12 | n << 16 on the slots R, Y0 .. Y3
// (working values) and F (the input, read only).  Every lane pair runs the same
// program, so the control flow is uniform and each operation is compiled once.
enum { FE_MUL = 0, FE_CSQR = 1, FE_CONJ = 2, FE_FROB = 3 };
enum { FE_R = 0, FE_Y0 = 1, FE_Y1 = 2, FE_Y2 = 3, FE_Y3 = 4, FE_F = 5 };
#define FE_OP(op, d, a, b, n) \
  ((uint32_t)(op) | ((uint32_t)(d) << 4) | ((uint32_t)(a) << 8) | ((uint32_t)(b) << 12) | ((uint32_t)(n) << 16))
#define FE_MULS(d, a, b) FE_OP(FE_MUL, d, a, b, 0)
#define FE_SQRS(d, a, n) FE_OP(FE_CSQR, d, a, 0, n)
#define FE_CONJS(d, a) FE_OP(FE_CONJ, d, a, 0, 0)
#define FE_FROBS(d, a, k) FE_OP(FE_FROB, d, a, 0, k)
// d = a^(|z| / 2) conjugated (z < 0): five multiply-and-square runs over the bits of |z|; d is not a
#define FE_ZHALF(d, a)                                                                                       \
  FE_SQRS(d, a, 1), FE_MULS(d, d, a), FE_SQRS(d, d, 2), FE_MULS(d, d, a), FE_SQRS(d, d, 3), FE_MULS(d, d, a), \
      FE_SQRS(d, d, 9), FE_MULS(d, d, a), FE_SQRS(d, d, 32), FE_MULS(d, d, a), FE_SQRS(d, d, 15), FE_CONJS(d, d)
#define FE_Z(d, a) FE_ZHALF(d, a), FE_SQRS(d, d, 1)
static __constant__ uint32_t PAIR_FE_PROG[] = {
    // the easy part: R = f^((p^6 - 1)(p^2 + 1)); k_pair_fe_inv has left 1 / f in Y2
    FE_CONJS(FE_Y1, FE_F), FE_MULS(FE_R, FE_Y1, FE_Y2), FE_FROBS(FE_Y2, FE_R, 2), FE_MULS(FE_R, FE_R, FE_Y2),
    // the hard part, the chain of ref pairing.c:382-403
    FE_SQRS(FE_Y0, FE_R, 1), FE_Z(FE_Y1, FE_Y0), FE_ZHALF(FE_Y2, FE_Y1), FE_CONJS(FE_Y3, FE_R),
    FE_MULS(FE_Y1, FE_Y1, FE_Y3), FE_CONJS(FE_Y1, FE_Y1), FE_MULS(FE_Y1, FE_Y1, FE_Y2), FE_Z(FE_Y2, FE_Y1),
    FE_Z(FE_Y3, FE_Y2), FE_CONJS(FE_Y1, FE_Y1), FE_MULS(FE_Y3, FE_Y3, FE_Y1), FE_CONJS(FE_Y1, FE_Y1),
    FE_FROBS(FE_Y1, FE_Y1, 3), FE_FROBS(FE_Y2, FE_Y2, 2), FE_MULS(FE_Y1, FE_Y1, FE_Y2), FE_Z(FE_Y2, FE_Y3),
    FE_MULS(FE_Y2, FE_Y2, FE_Y0), FE_MULS(FE_Y2, FE_Y2, FE_R), FE_MULS(FE_Y1, FE_Y1, FE_Y2),
    FE_FROBS(FE_Y2, FE_Y3, 1), FE_MULS(FE_R, FE_Y1, FE_Y2)};
constexpr int PAIR_FE_LEN = (int)(sizeof(PAIR_FE_PROG) / sizeof(uint32_t));

// lane pair t < n: slot Y2 of value t = 1 / src[t].  A kernel of its own: beside the
// products of the program the inversion does not fit the registers without spills.
static __global__ void __launch_bounds__(128)
    k_pair_fe_inv(const Fp12S *__restrict__ src, size_t n, Fp12S *__restrict__ ws) {
  PAIR_LANE();
  if (t >= n) return;  // whole pairs only
  t_inv12(&ws[(size_t)FE_Y2 * n + t], &src[t], comp);
}

// lane pair t < n: the first nprog instructions on src[t] (slot s of value t at ws[s n + t]),
// then the result (src[t] itself when nprog is 0) as blst bytes at dst + 72 t (unless
// NULL) and is_one[t] = the result is one (unless NULL)
static __global__ void __launch_bounds__(128)
    k_pair_final_exp(const Fp12S *__restrict__ src, size_t n, Fp12S *__restrict__ ws, uint64_t *__restrict__ dst,
                     uint8_t *__restrict__ is_one, int nprog) {
  PAIR_LANE();
  if (t >= n) return;  // whole pairs only
  Fp12S *in = const_cast<Fp12S *>(&src[t]);  // (never a destination)
  auto slot = [&](uint32_t s) { return s == FE_F ? in : &ws[(size_t)s * n + t]; };
#pragma unroll 1
  for (int pc = 0; pc < nprog; ++pc) {
    const uint32_t w = PAIR_FE_PROG[pc];
    const uint32_t op = w & 15u, cnt = w >> 16;
    Fp12S *d = slot((w >> 4) & 15u);
    const Fp12S *a = slot((w >> 8) & 15u), *b = slot((w >> 12) & 15u);
    switch (op) {
      case FE_MUL:
        t_mul12(d, a, b, comp);
        break;
      case FE_CSQR: {
        F12L v;
        t_ld12(v, a, comp);
#pragma unroll 1
        for (uint32_t i = 0; i < cnt; ++i) t_cyc_sqr12(v);
        t_st12(d, v, comp);
        break;
      }
      case FE_CONJ:
        t_conj12(d, a, comp);
        break;
      default:
        t_frob12(d, a, (int)cnt, comp);
        break;
    }
  }
  const Fp12S *r = nprog ? slot(FE_R) : in;
  uint32_t same = 1;
#pragma unroll 1
  for (int j = 0; j < 6; ++j) {
    Fp c, v, want;
    ld_comp(c, &r->c[j], comp);
    fp_canon(v, c);
    fp_zero(want);
    if (j == 0 && comp == 0) fp_one(want);
    uint32_t x = 0;
#pragma unroll
    for (int i = 0; i < NL; ++i) x |= v.v[i] ^ want.v[i];
    same &= x == 0 ? 1u : 0u;
    if (dst) fp_to_blst(dst + t * 72 + j * 12 + 6 * comp, v);
  }
  same &= pair_swap(same);
  if (is_one && comp == 0) is_one[t] = (uint8_t)same;
}

// -------------------------------------------------------------- engine ----
void Pairing::finish_kernels(hipStream_t s, size_t n, void *d_dst, uint8_t *d_st, bool final_exp) {
  if (final_exp) {
    hipLaunchKernelGGL(k_pair_fe_inv, dim3(nblk(n * 2, 128)), dim3(128), 0, s, (const Fp12S *)res_.as<Fp12S>(), n,
                       ws_.as<Fp12S>());
    MSM_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_pair_final_exp, dim3(nblk(n * 2, 128)), dim3(128), 0, s, (const Fp12S *)res_.as<Fp12S>(), n,
                     ws_.as<Fp12S>(), static_cast<uint64_t *>(d_dst), d_st, final_exp ? PAIR_FE_LEN : 0);
  MSM_HIP_CHECK(hipGetLastError());
}

void Pairing::run(hipStream_t cs, const void *p, const void *q, const size_t *o, size_t k, void *dst, uint8_t *is_one,
                  bool final_exp, bool src_dev, bool dst_dev) {
  if (!k) return;
  DeviceGuard g(dev_);
  const size_t total = o[k] - o[0];
  const SegSizes z = seg_sizes(total, k, pair_chunk());
  const size_t C = z.C, CP = z.CP, pmax = z.pmax;
  const size_t L = pair_piece_len(CP);
  const bool host_out = dst && !dst_dev, back = host_out || is_one;  // something comes back per chunk
  rec_.ensure(CP * REC);
  part_.ensure(pmax * FP12S);
  res_.ensure(C * FP12S);
  if (final_exp) ws_.ensure((size_t)FE_SLOTS * C * FP12S);
  carry_.ensure(FP12S);
  plan_lane_.ensure(z);
  if (!src_dev && total) {
    in_p_.ensure(CP * P_AFF);
    in_q_.ensure(CP * Q_AFF);
  }
  if (host_out) out_.ensure(C * GT);
  if (is_one) {
    st_.ensure(C, false);
    st_dev_[0].ensure(C);
    st_dev_[1].ensure(C);
  }
  pipe_.begin(cs);  // the record, partial, working and verdict buffers of the previous call
  auto pend = pipe_.pending([&](int slot, size_t off, size_t cnt) {  // (a chunk may write no segment: cnt 0)
    if (host_out && cnt) memcpy(static_cast<uint8_t *>(dst) + off * GT, out_.pin[slot], cnt * GT);
    if (is_one && cnt) memcpy(is_one + off, st_.pin[slot], cnt);
  });
  const unsigned B = 128;
  Fp12S *part = part_.as<Fp12S>();
  plan_.begin(o, k, z, L, "pairing");
  for (size_t ck = 0; plan_.next(); ++ck) {
    // this chunk: pairs [i, i + cnt), segments [j, j + nseg) end in it; np partials, the carried one (pc) first
    const size_t i = plan_.i, cnt = plan_.cnt(), j = plan_.j, nseg = plan_.nseg();
    const size_t np = plan_.np(), npieces = plan_.npieces(), pc = plan_.pc;
    const int slot = (int)(ck & 1);
    // ---- the plan and the sources go up ----
    plan_lane_.send(cs, slot, plan_);
    const SegMeta *d_meta = plan_lane_.d_meta();
    const uint32_t *d_src = plan_lane_.d_src();
    const uint8_t *d_p = nullptr, *d_q = nullptr;
    if (cnt) {
      if (!src_dev) {
        pipe_.upload(cs, slot, [&] {
          memcpy(in_p_.pin[slot], static_cast<const uint8_t *>(p) + i * P_AFF, cnt * P_AFF);
          memcpy(in_q_.pin[slot], static_cast<const uint8_t *>(q) + i * Q_AFF, cnt * Q_AFF);
        }, {{in_p_, slot, cnt * P_AFF}, {in_q_, slot, cnt * Q_AFF}});  // (one event for the two lanes)
        d_p = in_p_.dev[slot].as<uint8_t>();
        d_q = in_q_.dev[slot].as<uint8_t>();
      } else {
        d_p = static_cast<const uint8_t *>(p) + i * P_AFF;
        d_q = static_cast<const uint8_t *>(q) + i * Q_AFF;
      }
    }
    if (back) pipe_.out_open(cs, slot);  // (guards st_dev_[slot] as well as the output slot)
    void *d_dst = !dst ? nullptr : dst_dev ? static_cast<void *>(static_cast<uint8_t *>(dst) + j * GT) : out_.dev[slot].p;
    uint8_t *d_st = is_one ? st_dev_[slot].as<uint8_t>() : nullptr;
    // ---- the kernels ----
    if (npieces) {
      hipLaunchKernelGGL(k_pair_init, dim3(nblk(cnt * 2, B)), dim3(B), 0, cs, reinterpret_cast<const uint64_t *>(d_p),
                         reinterpret_cast<const uint64_t *>(d_q), cnt, rec_.as<PairRec>());
      MSM_HIP_CHECK(hipGetLastError());
      if (pc) MSM_HIP_CHECK(hipMemcpyAsync(part, carry_.p, FP12S, hipMemcpyDeviceToDevice, cs));
      hipLaunchKernelGGL(k_pair_miller, dim3(nblk(npieces * 2, B)), dim3(B), 0, cs, rec_.as<PairRec>(), d_meta + pc,
                         part + pc, npieces);
      MSM_HIP_CHECK(hipGetLastError());
      for (size_t step = 1; step < plan_.maxrun; step *= 2) {
        hipLaunchKernelGGL(k_pair_merge, dim3(nblk(np * 2, B)), dim3(B), 0, cs, part, d_meta, np, (uint32_t)step);
        MSM_HIP_CHECK(hipGetLastError());
      }
    }
    if (nseg) {
      hipLaunchKernelGGL(k_pair_gather, dim3(nblk(nseg * 2, B)), dim3(B), 0, cs, (const Fp12S *)part, d_src,
                         res_.as<Fp12S>(), nseg);
      MSM_HIP_CHECK(hipGetLastError());
      finish_kernels(cs, nseg, d_dst, d_st, final_exp);
    }
    // a segment stays open: what this chunk multiplied of it goes into the next one
    if (plan_.carry()) MSM_HIP_CHECK(hipMemcpyAsync(carry_.p, part + plan_.open_src, FP12S, hipMemcpyDeviceToDevice, cs));
    pipe_.computed(cs, slot);
    if (back)
      pipe_.download(cs, slot, pend, j, nseg,
                     {{out_, slot, host_out ? nseg * GT : 0}, {st_.pin[slot], st_dev_[slot].p, is_one ? nseg : 0}});
  }
  pend.flush();  // (nothing is held where no chunk ran)
  pipe_.finish(cs);
}

void Pairing::run_final_exp(hipStream_t cs, const void *src, size_t n, void *dst, uint8_t *is_one, bool src_dev,
                            bool dst_dev) {
  if (!n) return;
  DeviceGuard g(dev_);
  const size_t C = std::min(n, pair_chunk());
  const bool host_out = dst && !dst_dev, back = host_out || is_one;
  res_.ensure(C * FP12S);
  ws_.ensure((size_t)FE_SLOTS * C * FP12S);
  if (!src_dev) in_q_.ensure(C * GT);
  if (host_out) out_.ensure(C * GT);
  if (is_one) {
    st_.ensure(C, false);
    st_dev_[0].ensure(C);
    st_dev_[1].ensure(C);
  }
  pipe_.begin(cs);
  auto pend = pipe_.pending([&](int slot, size_t off, size_t cnt) {
    if (host_out) memcpy(static_cast<uint8_t *>(dst) + off * GT, out_.pin[slot], cnt * GT);
    if (is_one) memcpy(is_one + off, st_.pin[slot], cnt);
  });
  size_t ck = 0;
  for (size_t c0 = 0; c0 < n; c0 += C, ++ck) {
    const size_t cnt = std::min(C, n - c0);
    const int slot = (int)(ck & 1);
    const void *d_src;
    if (!src_dev) {
      pipe_.upload(cs, slot, [&] { memcpy(in_q_.pin[slot], static_cast<const uint8_t *>(src) + c0 * GT, cnt * GT); },
                   {{in_q_, slot, cnt * GT}});
      d_src = in_q_.dev[slot].p;
    } else {
      d_src = static_cast<const uint8_t *>(src) + c0 * GT;
    }
    if (back) pipe_.out_open(cs, slot);
    void *d_dst = !dst ? nullptr : dst_dev ? static_cast<void *>(static_cast<uint8_t *>(dst) + c0 * GT) : out_.dev[slot].p;
    hipLaunchKernelGGL(k_pair_load, dim3(nblk(cnt * 2, 128)), dim3(128), 0, cs, static_cast<const uint64_t *>(d_src), cnt,
                       res_.as<Fp12S>());
    MSM_HIP_CHECK(hipGetLastError());
    finish_kernels(cs, cnt, d_dst, is_one ? st_dev_[slot].as<uint8_t>() : nullptr, true);
    pipe_.computed(cs, slot);
    if (back)
      pipe_.download(cs, slot, pend, c0, cnt,
                     {{out_, slot, host_out ? cnt * GT : 0}, {st_.pin[slot], st_dev_[slot].p, is_one ? cnt : 0}});
  }
  pend.flush();
  pipe_.finish(cs);
}

// ------------------------------------------------ per-operation test entry ----
// msm_test_fp12 (include/msm_mi355x.h; tests/test_gpu_fp12_tower.py): one tower
// operation per lane pair on stored values, with the lane mapping, the launch
// bounds and the memory-to-memory forms of the kernels above.  The inversion has
// a kernel of its own as k_pair_fe_inv has, and so have the two line functions,
// which keep their point and line in registers.  The destination may be an
// operand (the host passes the same pointer), hence no __restrict__.
static __global__ void __launch_bounds__(128)
    k_test_fp12(int op, int k, Fp12S *d, const Fp12S *a, const Fp12S *b, size_t n) {
  PAIR_LANE();
  if (t >= n) return;  // whole pairs only
  switch (op) {
    case TEST_FP12_MUL:
      t_mul12(&d[t], &a[t], &b[t], comp);
      break;
    case TEST_FP12_SQR:
      t_sqr12(&d[t], &a[t], comp);
      break;
    case TEST_FP12_SPARSE: {
      Fp2L x, y, z;
      ld_comp(x.c, &b[t].c[0], comp);
      ld_comp(y.c, &b[t].c[1], comp);
      ld_comp(z.c, &b[t].c[4], comp);
      t_mul12_sparse(&d[t], &a[t], x, y, z, comp);
      break;
    }
    case TEST_FP12_CONJ:
      t_conj12(&d[t], &a[t], comp);
      break;
    case TEST_FP12_FROB:
      t_frob12(&d[t], &a[t], k, comp);
      break;
    default: {  // TEST_FP12_CSQR: k squarings held in registers, as FE_CSQR
      F12L v;
      t_ld12(v, &a[t], comp);
#pragma unroll 1
      for (int i = 0; i < k; ++i) t_cyc_sqr12(v);
      t_st12(&d[t], v, comp);
      break;
    }
  }
}
static __global__ void __launch_bounds__(128) k_test_fp12_inv(Fp12S *d, const Fp12S *a, size_t n) {
  PAIR_LANE();
  if (t >= n) return;
  t_inv12(&d[t], &a[t], comp);
}
// a[t]: X, Y, Z, qx, qy (the sixth slot is not read); d[t]: X3, Y3, Z3, l0, l1, l2
static __global__ void __launch_bounds__(128) k_test_fp12_line(int add, Fp12S *d, const Fp12S *a, size_t n) {
  PAIR_LANE();
  if (t >= n) return;
  Fp2L X, Y, Z, l0, l1, l2;
  ld_comp(X.c, &a[t].c[0], comp);
  ld_comp(Y.c, &a[t].c[1], comp);
  ld_comp(Z.c, &a[t].c[2], comp);
  if (add) {
    Fp2L qx, qy;
    ld_comp(qx.c, &a[t].c[3], comp);
    ld_comp(qy.c, &a[t].c[4], comp);
    pair_line_add(X, Y, Z, qx, qy, l0, l1, l2);
  } else {
    pair_line_dbl(X, Y, Z, l0, l1, l2);
  }
  st_comp(&d[t].c[0], X.c, comp);
  st_comp(&d[t].c[1], Y.c, comp);
  st_comp(&d[t].c[2], Z.c, comp);
  st_comp(&d[t].c[3], l0.c, comp);
  st_comp(&d[t].c[4], l1.c, comp);
  st_comp(&d[t].c[5], l2.c, comp);
}

void test_fp12(int op, int k, int alias, bool raw, const void *a, const void *b, void *out, size_t n) {
  if (!n) return;
  DeviceGuard g(0);
  constexpr size_t GT = Pairing::GT, S = Pairing::FP12S;
  const dim3 grid(nblk(n * 2, 128)), block(128);
  DevBuf da, db, dd, io;
  da.ensure(n * S);
  if (b) db.ensure(n * S);
  if (!alias) dd.ensure(n * S);
  if (!raw) io.ensure(n * GT);
  auto up = [&](DevBuf &dst, const void *src) {
    if (raw) {
      MSM_HIP_CHECK(hipMemcpy(dst.p, src, n * S, hipMemcpyHostToDevice));
    } else {  // the arithmetic of msm_fp12_final_exp's way in
      MSM_HIP_CHECK(hipMemcpy(io.p, src, n * GT, hipMemcpyHostToDevice));
      hipLaunchKernelGGL(k_pair_load, grid, block, 0, 0, (const uint64_t *)io.as<uint64_t>(), n, dst.as<Fp12S>());
      MSM_HIP_CHECK(hipGetLastError());
    }
  };
  up(da, a);
  if (b) up(db, b);
  Fp12S *A = da.as<Fp12S>(), *B = b ? db.as<Fp12S>() : nullptr;
  Fp12S *D = alias == 1 ? A : alias == 2 ? B : dd.as<Fp12S>();
  if (op == TEST_FP12_INV)
    hipLaunchKernelGGL(k_test_fp12_inv, grid, block, 0, 0, D, (const Fp12S *)A, n);
  else if (op == TEST_FP12_LINE_DBL || op == TEST_FP12_LINE_ADD)
    hipLaunchKernelGGL(k_test_fp12_line, grid, block, 0, 0, op == TEST_FP12_LINE_ADD ? 1 : 0, D, (const Fp12S *)A, n);
  else
    hipLaunchKernelGGL(k_test_fp12, grid, block, 0, 0, op, k, D, (const Fp12S *)A, (const Fp12S *)B, n);
  MSM_HIP_CHECK(hipGetLastError());
  if (raw) {
    MSM_HIP_CHECK(hipMemcpy(out, D, n * S, hipMemcpyDeviceToHost));
  } else {  // its way out: the tail of k_pair_final_exp (an empty program)
    hipLaunchKernelGGL(k_pair_final_exp, grid, block, 0, 0, (const Fp12S *)D, n, (Fp12S *)nullptr, io.as<uint64_t>(),
                       (uint8_t *)nullptr, 0);
    MSM_HIP_CHECK(hipGetLastError());
    MSM_HIP_CHECK(hipMemcpy(out, io.p, n * GT, hipMemcpyDeviceToHost));
  }
}

}  // namespace msm
