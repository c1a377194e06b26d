// fr_ntt.hip -- bulk Fr arithmetic and batched NTTs on one MI355X (msm_fr_ntt,
// msm_fr_op; the device side of the reference's blst_fr_* loops, ref
// src/exports.c, and of the transforms a prover builds on them).
//
// k_fr_ntt_pass is one Stockham pass of ntt_plan.hpp.  A workgroup of 256
// lanes fills its tile in LDS (first pass: the change of form and the coset
// powers ride on the load), runs the log2(R) butterfly levels there as in-place
// decimation in frequency -- a radix-2 step when log2(R) is odd, then radix-4
// steps, each lane holding its four elements and three twiddles in registers
// between the two levels -- and writes the tile back through the bit reversal
// of the row index with the inter-pass twiddle applied (last pass: 1 / n, the
// coset powers, the index reversal of an inverse transform and the change of
// form ride on the store).  An inverse transform is the forward one written to
// index (n - k) mod n, so one set of twiddles serves both directions.
//
// LDS layout: planar, limb l of element e at word l LS + e + (e >> 5).  Lanes
// that walk consecutive elements hit consecutive banks; the skew of one word
// per 32 elements spreads the power-of-two strides of the last radix-4 steps
// and of the bit-reversed read.
//
// Twiddles: per log_n, omega_n^e for e < n / 2 as lo[e mod 2^12] hi[e >> 12]
// (one product per inter-pass twiddle; n <= 2^13 needs no hi), and for the
// butterflies inside a tile a direct table of omega_2048^x (n <= 2^13: lo
// itself).  All entries are c 2^261 mod r, 32 bytes, so a product with one
// leaves the data in the form it came in.
//
// k_fr_op is the elementwise call; MSM_FR_INV is the product tree of
// to_affine.hip (its level plan, to_affine.hpp ta_levels, is shared) over Fr:
// k_fr_up / k_fr_leaf / k_fr_down.  A zero enters the products as one and
// comes out as zero.
#include "fr_ntt.hpp"

#include <cstring>
#include <type_traits>

#include "fr_mem.hpp"
#include "to_affine.hpp"

namespace msm {

namespace {

// ---- LDS: planar with a skew ----
__device__ __forceinline__ uint32_t lds_at(uint32_t e) { return e + (e >> 5); }
__device__ __forceinline__ void lds_ld(Fr &r, const uint32_t *lds, uint32_t ls, uint32_t e) {
  const uint32_t p = lds_at(e);
#pragma unroll
  for (int l = 0; l < FR_NL; ++l) r.v[l] = lds[l * ls + p];
}
__device__ __forceinline__ void lds_st(uint32_t *lds, uint32_t ls, uint32_t e, const Fr &a) {
  const uint32_t p = lds_at(e);
#pragma unroll
  for (int l = 0; l < FR_NL; ++l) lds[l * ls + p] = a.v[l];
}

enum {
  NP_LAST = 1,       // the last pass: no inter-pass twiddle
  NP_REVERSE = 2,    // store to index (n - k) mod n (the last pass of an inverse transform)
  NP_IN_CONST = 4,   // multiply every loaded element by cin
  NP_IN_TABLE = 8,   // ... by sh_lo[j mod 2^slb] sh_hi[j >> slb], j its index in the transform
  NP_OUT_CONST = 16,  // the same on the store, by cout / the table at the output index
  NP_OUT_TABLE = 32,
};

struct NttArgs {
  const uint32_t *src;
  uint32_t *dst;
  size_t slots;                         // tiles of R x C elements in the call
  int log_n, log_r, log_c, log_s, log_t;  // s: the product of the earlier radices; 2^log_t slots per workgroup
  int flags;
  const uint32_t *tw_lo, *tw_hi, *tw_in;
  int lb, in_log;
  const uint32_t *sh_lo, *sh_hi;
  int slb;
  FrK cin, cout;
};

__device__ __forceinline__ void sh_lookup(Fr &w, const NttArgs &A, uint32_t j) {
  fr_ld(w, A.sh_lo + (size_t)(j & ((1u << A.slb) - 1)) * 8);
  if (A.sh_hi) {
    Fr h;
    fr_ld(h, A.sh_hi + (size_t)(j >> A.slb) * 8);
    fr_mul(w, w, h);
  }
}

// a' = a + b, b' = a - b (not yet multiplied): class S and lazy
__device__ __forceinline__ void bfly(Fr &a, Fr &b) {
  Fr s;
  fr_add(s, a, b);
  fr_sub4(b, a, b);
  fr_nred(s);
  a = s;
}

static __global__ void __launch_bounds__(256) k_fr_ntt_pass(const NttArgs A) {
  extern __shared__ uint32_t lds[];
  const int lr = A.log_r, lc = A.log_c;
  const uint32_t E = 1u << (A.log_t + lr + lc), LS = E + (E >> 5) + 1;
  const uint32_t R = 1u << lr, C = 1u << lc;
  const size_t slot0 = (size_t)blockIdx.x << A.log_t;
  const int lspt = A.log_n - lr - lc;  // log2 of the slots of one transform
  const uint32_t tid = threadIdx.x;

  // ---- load: columns fastest (runs of C elements), rows n / R apart ----
  for (uint32_t e = tid; e < E; e += 256) {
    const uint32_t sl = e >> (lr + lc), i = (e >> lc) & (R - 1), c = e & (C - 1);
    const size_t slot = slot0 + sl;
    if (slot < A.slots) {
      const size_t b = slot >> lspt;
      const uint32_t g = (((uint32_t)slot & ((1u << lspt) - 1)) << lc) + c;
      const uint32_t j = g + (i << (A.log_n - lr));
      Fr x;
      fr_ld(x, A.src + ((b << A.log_n) + j) * 8);
      if (A.flags & NP_IN_CONST) {
        Fr k;
        fr_arg(k, A.cin);
        fr_mul(x, x, k);
      } else if (A.flags & NP_IN_TABLE) {
        Fr w;
        sh_lookup(w, A, j);
        fr_mul(x, x, w);
      }
      lds_st(lds, LS, e, x);
    }
  }
  __syncthreads();

  // ---- the butterfly levels, in place, decimation in frequency ----
  uint32_t L = R;  // size of the sub-transforms still to do
  int ll = lr;
  if (lr & 1) {
    const uint32_t h = R >> 1;
    for (uint32_t pid = tid; pid < (E >> 1); pid += 256) {
      const uint32_t c = pid & (C - 1), t = (pid >> lc) & (h - 1), sl = pid >> (lc + lr - 1);
      if (slot0 + sl < A.slots) {
        const uint32_t i0 = (sl << (lr + lc)) + (t << lc) + c, i1 = i0 + (h << lc);
        Fr a, b;
        lds_ld(a, lds, LS, i0);
        lds_ld(b, lds, LS, i1);
        bfly(a, b);
        if (h > 1) {
          Fr w;
          fr_ld(w, A.tw_in + ((size_t)t << (A.in_log - lr)) * 8);
          fr_mul(b, b, w);
        } else {
          fr_nred(b);
        }
        lds_st(lds, LS, i0, a);
        lds_st(lds, LS, i1, b);
      }
    }
    L = h;
    ll = lr - 1;
    __syncthreads();
  }
  while (L >= 4) {
    const uint32_t q = L >> 2;
    const int lq = ll - 2, sh = A.in_log - ll;  // omega_L^x = tw_in[x << sh]
    for (uint32_t qd = tid; qd < (E >> 2); qd += 256) {
      const uint32_t c = qd & (C - 1), jj = (qd >> lc) & ((R >> 2) - 1), sl = qd >> (lc + lr - 2);
      if (slot0 + sl < A.slots) {
        const uint32_t t = jj & (q - 1), u = ((jj >> lq) << (lq + 2)) + t;
        const uint32_t base = (sl << (lr + lc)) + (u << lc) + c, step = q << lc;
        Fr e0, e1, e2, e3;
        lds_ld(e0, lds, LS, base);
        lds_ld(e1, lds, LS, base + step);
        lds_ld(e2, lds, LS, base + 2 * step);
        lds_ld(e3, lds, LS, base + 3 * step);
        bfly(e0, e2);  // level of size L: (e0, e2) and (e1, e3)
        bfly(e1, e3);
        Fr w;
        if (L > 4) {
          fr_ld(w, A.tw_in + ((size_t)t << sh) * 8);
          fr_mul(e2, e2, w);
        } else {
          fr_nred(e2);
        }
        fr_ld(w, A.tw_in + ((size_t)(t + q) << sh) * 8);
        fr_mul(e3, e3, w);
        bfly(e0, e1);  // level of size L / 2: (e0, e1) and (e2, e3)
        bfly(e2, e3);
        if (L > 4) {
          fr_ld(w, A.tw_in + ((size_t)(2 * t) << sh) * 8);
          fr_mul(e1, e1, w);
          fr_mul(e3, e3, w);
        } else {
          fr_nred(e1);
          fr_nred(e3);
        }
        lds_st(lds, LS, base, e0);
        lds_st(lds, LS, base + step, e1);
        lds_st(lds, LS, base + 2 * step, e2);
        lds_st(lds, LS, base + 3 * step, e3);
      }
    }
    L = q;
    ll -= 2;
    __syncthreads();
  }

  // ---- store: row k sits at the bit reversal of k; y[q + s (R p + k)] ----
  const bool k_fast = A.log_s < lc;  // the first pass of several: a column's outputs are adjacent
  const uint32_t n = 1u << A.log_n;
  for (uint32_t e = tid; e < E; e += 256) {
    const uint32_t sl = e >> (lr + lc);
    const uint32_t k = k_fast ? e & (R - 1) : (e >> lc) & (R - 1);
    const uint32_t c = k_fast ? (e >> lr) & (C - 1) : e & (C - 1);
    const size_t slot = slot0 + sl;
    if (slot < A.slots) {
      const uint32_t kb = lr ? __brev(k) >> (32 - lr) : 0;
      Fr x;
      lds_ld(x, lds, LS, (sl << (lr + lc)) + (kb << lc) + c);
      const size_t b = slot >> lspt;
      const uint32_t g = (((uint32_t)slot & ((1u << lspt) - 1)) << lc) + c;
      const uint32_t qq = g & ((1u << A.log_s) - 1), p = g >> A.log_s;
      if (!(A.flags & NP_LAST)) {
        const uint32_t ex = (p * k) << A.log_s;  // omega_n^ex = omega_(n/s)^(p k), ex < n
        if (ex) {
          const uint32_t e2 = ex & ((n >> 1) - 1);
          Fr w;
          fr_ld(w, A.tw_lo + (size_t)(e2 & ((1u << A.lb) - 1)) * 8);
          if (A.tw_hi) {
            Fr h;
            fr_ld(h, A.tw_hi + (size_t)(e2 >> A.lb) * 8);
            fr_mul(w, w, h);
          }
          if (ex >> (A.log_n - 1)) fr_neg4(w, w);  // omega^(n/2) = -1
          fr_mul(x, x, w);
        }
      }
      uint32_t o = qq + (((p << lr) + k) << A.log_s);
      if (A.flags & NP_REVERSE) o = (n - o) & (n - 1);
      if (A.flags & NP_OUT_CONST) {
        Fr kc;
        fr_arg(kc, A.cout);
        fr_mul(x, x, kc);
      } else if (A.flags & NP_OUT_TABLE) {
        Fr w;
        sh_lookup(w, A, o);
        fr_mul(x, x, w);
      }
      fr_csub(x);
      fr_st(A.dst + ((b << A.log_n) + o) * 8, x);
    }
  }
}

// out[t] = mult base^t, t < count (all c 2^261 mod r; canonical)
static __global__ void __launch_bounds__(256) k_fr_pow_table(uint32_t *out, uint32_t count, const FrK base,
                                                             const FrK mult) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  Fr acc, b;
  fr_arg(acc, mult);
  fr_arg(b, base);
  for (uint32_t rest = t; rest; rest >>= 1) {
    if (rest & 1) fr_mul(acc, acc, b);
    fr_mul(b, b, b);
  }
  fr_csub(acc);
  fr_st(out + (size_t)t * 8, acc);
}

// ---- elementwise ----
template <int OP>
static __global__ void __launch_bounds__(256)
    k_fr_op(uint32_t *dst, const uint32_t *a, const uint32_t *b, size_t n, size_t b_stride) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fr x, y;
  fr_ld(x, a + i * 8);
  if constexpr (OP == FR_ADD || OP == FR_SUB || OP == FR_MUL) fr_ld(y, b + i * b_stride * 8);
  fr_elem<OP>(x, y);
  fr_st(dst + i * 8, x);
}

// ---- the inversion tree (to_affine.hip's, over Fr; TA_K elements per group) ----
template <int J, int N, class Fn>
__device__ __forceinline__ void fr_static_for(Fn &&f) {
  if constexpr (J < N) {
    f(std::integral_constant<int, J>{});
    fr_static_for<J + 1, N>(f);
  }
}
// element j of a level; at level 0 (DATA) a zero is taken as one, `zero` set
template <bool DATA>
__device__ __forceinline__ void inv_elem(Fr &r, const uint32_t *lvl, size_t j, bool &zero) {
  fr_ld(r, lvl + j * 8);
  zero = false;
  if (DATA) {
    zero = fr_is_zero_exact(r);
    Fr one;
    fr_one(one);
    fr_sel(r, zero, one);
  }
}
template <bool DATA>
static __global__ void __launch_bounds__(128) k_fr_up(const uint32_t *src, size_t n_src, uint32_t *dst, size_t n_dst) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_dst) return;
  const size_t j0 = t * TA_K, cnt = min((size_t)TA_K, n_src - j0);
  bool z;
  Fr acc;
  inv_elem<DATA>(acc, src, j0, z);
  for (size_t j = 1; j < cnt; ++j) {
    Fr e;
    inv_elem<DATA>(e, src, j0 + j, z);
    fr_mul(acc, acc, e);
  }
  fr_csub(acc);
  fr_st(dst + t * 8, acc);
}
// top[t] = 1 / top[t] (Fermat, in the 2^261 domain)
static __global__ void __launch_bounds__(64) k_fr_leaf(uint32_t *top, size_t m) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= m) return;
  Fr a, r;
  fr_ld(a, top + t * 8);
  fr_one(r);
  for (int w = 3; w >= 0; --w) {  // r - 2, a word at a time (selects, no indexed array)
    const uint64_t word = w == 3 ? 0x73eda753299d7d48ull
                          : w == 2 ? 0x3339d80809a1d805ull
                          : w == 1 ? 0x53bda402fffe5bfeull
                                   : 0xfffffffeffffffffull;
    for (int i = 63; i >= 0; --i) {
      fr_mul(r, r, r);
      if ((word >> i) & 1) fr_mul(r, r, a);
    }
  }
  fr_csub(r);
  fr_st(top + t * 8, r);
}
// from 1 / (product of group t) every element's inverse; level 0 (DATA) writes
// the blst_fr of 1 / a to out (lvl = the data, read only unless out == lvl)
template <bool DATA>
static __global__ void __launch_bounds__(128)
    k_fr_down(const uint32_t *inv_up, size_t n_up, uint32_t *lvl, size_t n_lvl, uint32_t *out) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_up) return;
  const size_t j0 = t * TA_K;
  const int cnt = (int)min((size_t)TA_K, n_lvl - j0);
  Fr I;
  fr_ld(I, inv_up + t * 8);
  bool z;
  Fr pre[TA_K - 1];  // pre[j] = e_0 .. e_j
  inv_elem<DATA>(pre[0], lvl, j0, z);
  fr_static_for<1, (int)TA_K - 1>([&](auto jc) __attribute__((always_inline)) {
    constexpr int j = decltype(jc)::value;
    if (j < cnt) {
      Fr e;
      inv_elem<DATA>(e, lvl, j0 + j, z);
      fr_mul(pre[j], pre[j - 1], e);
    }
  });
  fr_static_for<0, (int)TA_K>([&](auto jc) __attribute__((always_inline)) {
    constexpr int j = (int)TA_K - 1 - decltype(jc)::value;
    if (j < cnt) {
      Fr e, ij;
      inv_elem<DATA>(e, lvl, j0 + j, z);
      if constexpr (j > 0) {
        fr_mul(ij, I, pre[j - 1]);
        fr_mul(I, I, e);
      } else {
        ij = I;
      }
      if constexpr (DATA) {
        Fr zero;
        fr_mulc(ij, ij, FR_C251);  // (a 2^-5)^-1 in the 2^261 domain -> a^-1 2^256
        fr_csub(ij);
        fr_zero(zero);
        fr_sel(ij, z, zero);
        fr_st(out + (j0 + j) * 8, ij);
      } else {
        fr_csub(ij);
        fr_st(lvl + (j0 + j) * 8, ij);
      }
    }
  });
}

static __global__ void __launch_bounds__(256) k_fr_probe(uint32_t *out, int iters) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  Fr x, y;
  fr_one(x);
  fr_set(y, FR_C266);
  x.v[0] ^= t & 0xffff;
  for (int i = 0; i < iters; ++i) {
    fr_mul(x, x, y);
    fr_mul(y, y, x);
  }
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < FR_NL; ++i) o ^= x.v[i] ^ y.v[i];
  out[t] = o;
}

// ---- host side ----
FrK internal(const hfr::Fr &x) { return fr_internal(x); }
const hfr::Fr kPlainOne = {{1, 0, 0, 0}};  // the blst_fr of 2^-256

}  // namespace

void fr_pow_table(hipStream_t s, uint32_t *out, size_t count, const hfr::Fr &base, const hfr::Fr &mult) {
  hipLaunchKernelGGL(k_fr_pow_table, dim3(nblk(count, 256)), dim3(256), 0, s, out, (uint32_t)count, internal(base),
                     internal(mult));
  MSM_HIP_CHECK(hipGetLastError());
}

size_t FrNtt::device_bytes() const {
  size_t b = ta_.bytes + tb_.bytes + lv_.bytes + sh_.bytes + in_.device_bytes() + inb_.device_bytes() +
             out_.device_bytes();
  for (const auto &kv : tw_) b += kv.second.buf.bytes;
  return b;
}

const FrNtt::Tables &FrNtt::tables(hipStream_t s, int log_n) {
  auto it = tw_.find(log_n);
  if (it != tw_.end()) return it->second;
  Tables t;
  t.lb = std::min(log_n - 1, 12);
  const size_t n_lo = (size_t)1 << t.lb, n_hi = (size_t)1 << (log_n - 1 - t.lb);
  const size_t n_in = log_n > 13 ? 1024 : 0;
  t.buf.ensure((n_lo + (n_hi > 1 ? n_hi : 0) + n_in) * EL);
  uint32_t *p = t.buf.as<uint32_t>();
  const hfr::Fr w = hfr::root_of_unity((unsigned)log_n);
  fr_pow_table(s, p, n_lo, w, hfr::ONE);
  t.lo = p;
  p += n_lo * 8;
  if (n_hi > 1) {
    fr_pow_table(s, p, n_hi, hfr::pow2k(w, (unsigned)t.lb), hfr::ONE);
    t.hi = p;
    p += n_hi * 8;
  }
  if (n_in) {
    fr_pow_table(s, p, n_in, hfr::root_of_unity(11), hfr::ONE);
    t.in = p, t.in_log = 11;
  } else {
    t.in = t.lo, t.in_log = log_n;
  }
  return tw_.emplace(log_n, std::move(t)).first->second;
}

// one chunk of whole transforms, device to device
void FrNtt::passes(hipStream_t s, const void *d_src, void *d_dst, int log_n, size_t batch, int flags, bool shifted) {
  const int tile = ntt_tile();
  std::vector<int> plan = ntt_plan(log_n, tile);
  if (plan.empty()) plan.push_back(0);  // log_n = 0: a copy, or a change of form
  const size_t np = plan.size();
  NttArgs A;
  memset(&A, 0, sizeof A);
  A.log_n = log_n;
  if (log_n > 0) {
    const Tables &t = tables(s, log_n);
    A.tw_lo = t.lo, A.tw_hi = t.hi, A.tw_in = t.in, A.lb = t.lb, A.in_log = t.in_log;
  }
  // what rides on the first load and the last store
  const bool inverse = (flags & FRF_INVERSE) != 0;
  hfr::Fr yin = hfr::ONE, yout = hfr::ONE;
  bool has_in = false, has_out = false;
  if (flags & FRF_SRC_SCALAR) yin = hfr::RR, has_in = true;  // the blst_fr of 2^256
  if (inverse && log_n > 0) yout = hfr::inverse(hfr::from_u64((uint64_t)1 << log_n)), has_out = true;
  if (flags & FRF_DST_SCALAR) yout = hfr::mul(yout, kPlainOne), has_out = true;
  int first = 0, last = NP_LAST | (inverse ? NP_REVERSE : 0);
  if (shifted) {  // (the tables of this call: FrNtt::ntt built them with yin / yout folded in)
    A.slb = std::min(log_n, 13);
    A.sh_lo = sh_.as<uint32_t>();
    A.sh_hi = log_n > A.slb ? A.sh_lo + ((size_t)8 << A.slb) : nullptr;
    if (inverse) last |= NP_OUT_TABLE;
    else first |= NP_IN_TABLE;
  }
  if (has_in && !(first & NP_IN_TABLE)) first |= NP_IN_CONST, A.cin = internal(yin);
  if (has_out && !(last & NP_OUT_TABLE)) last |= NP_OUT_CONST, A.cout = internal(yout);

  const void *cur = d_src;
  int log_s = 0;
  for (size_t i = 0; i < np; ++i) {
    void *out = i + 1 == np ? d_dst : (i & 1) ? tb_.p : ta_.p;
    A.src = static_cast<const uint32_t *>(cur);
    A.dst = static_cast<uint32_t *>(out);
    A.log_r = plan[i];
    A.log_c = np == 1 ? 0 : std::min(ntt_cols_log(tile), log_n - A.log_r);
    A.log_s = log_s;
    A.slots = batch << (log_n - A.log_r - A.log_c);
    A.log_t = std::max(0, tile - A.log_r - A.log_c);
    while (A.log_t > 0 && ((size_t)1 << (A.log_t - 1)) >= A.slots) --A.log_t;
    A.flags = (i == 0 ? first : 0) | (i + 1 == np ? last : 0);
    const size_t E = (size_t)1 << (A.log_t + A.log_r + A.log_c);
    const size_t lds = FR_NL * (E + (E >> 5) + 1) * sizeof(uint32_t);
    if (lds > 64 * 1024)
      MSM_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(k_fr_ntt_pass),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const size_t grid = (A.slots + ((size_t)1 << A.log_t) - 1) >> A.log_t;
    hipLaunchKernelGGL(k_fr_ntt_pass, dim3((unsigned)grid), dim3(256), lds, s, A);
    MSM_HIP_CHECK(hipGetLastError());
    cur = out;
    log_s += A.log_r;
  }
}

void FrNtt::ntt(hipStream_t cs, const void *src, void *dst, int log_n, size_t batch, const uint8_t *shift, int flags,
                bool src_dev, bool dst_dev) {
  if (!batch) return;
  DeviceGuard g(dev_);
  const size_t per = std::min(batch, std::max<size_t>(1, ntt_chunk() >> log_n));  // transforms per chunk
  const size_t C = per << log_n;
  const size_t np = std::max<size_t>(1, ntt_plan(log_n, ntt_tile()).size());
  if (np >= 2) ta_.ensure(C * EL);
  if (np >= 3) tb_.ensure(C * EL);
  if (!src_dev) in_.ensure(C * EL);
  if (!dst_dev) out_.ensure(C * EL);
  if (shift) sh_.ensure((((size_t)1 << std::min(log_n, 13)) + ((size_t)1 << std::max(0, log_n - 13))) * EL);
  pipe_.begin(cs);  // the pass buffers and tables of the previous call
  if (shift) {      // s^j (forward: times what the load applies; inverse: s^-j times what the store applies)
    const bool inverse = (flags & FRF_INVERSE) != 0;
    hfr::Fr base = hfr::from_scalar(shift), mult = hfr::ONE;
    if (inverse) {
      base = hfr::inverse(base);
      if (log_n > 0) mult = hfr::inverse(hfr::from_u64((uint64_t)1 << log_n));
      if (flags & FRF_DST_SCALAR) mult = hfr::mul(mult, kPlainOne);
    } else if (flags & FRF_SRC_SCALAR) {
      mult = hfr::RR;
    }
    const int slb = std::min(log_n, 13);
    fr_pow_table(cs, sh_.as<uint32_t>(), (size_t)1 << slb, base, mult);
    if (log_n > slb)
      fr_pow_table(cs, sh_.as<uint32_t>() + ((size_t)8 << slb), (size_t)1 << (log_n - slb),
                   hfr::pow2k(base, (unsigned)slb), hfr::ONE);
  }
  auto pend = pipe_.pending([&](int slot, size_t off, size_t cnt) {
    memcpy(static_cast<uint8_t *>(dst) + off * EL, out_.pin[slot], cnt * EL);
  });
  size_t k = 0;
  for (size_t c0 = 0; c0 < batch; c0 += per, ++k) {
    const size_t nb = std::min(per, batch - c0), cnt = nb << log_n, off = c0 << log_n;
    const int slot = (int)(k & 1);
    const void *d_src;
    void *d_dst;
    if (!src_dev) {
      pipe_.upload(cs, slot, [&] { memcpy(in_.pin[slot], static_cast<const uint8_t *>(src) + off * EL, cnt * EL); },
                   {{in_, slot, cnt * EL}});
      d_src = in_.dev[slot].p;
    } else {
      d_src = static_cast<const uint8_t *>(src) + off * EL;
    }
    if (!dst_dev) {
      pipe_.out_open(cs, slot);
      d_dst = out_.dev[slot].p;
    } else {
      d_dst = static_cast<uint8_t *>(dst) + off * EL;
    }
    passes(cs, d_src, d_dst, log_n, nb, flags, shift != nullptr);
    pipe_.computed(cs, slot);
    if (!dst_dev) pipe_.download(cs, slot, pend, off, cnt, {{out_, slot, cnt * EL}});
  }
  pend.flush();
  pipe_.finish(cs);
}

template <int OP>
static void launch_op(hipStream_t s, void *d_dst, const void *d_a, const void *d_b, size_t n, bool b_one) {
  hipLaunchKernelGGL(k_fr_op<OP>, dim3(nblk(n, 256)), dim3(256), 0, s, static_cast<uint32_t *>(d_dst),
                     static_cast<const uint32_t *>(d_a), static_cast<const uint32_t *>(d_b), n,
                     (size_t)(b_one ? 0 : 1));
  MSM_HIP_CHECK(hipGetLastError());
}

void FrNtt::op_kernels(hipStream_t s, int op, void *d_dst, const void *d_a, const void *d_b, size_t n, bool b_one) {
  switch (op) {
    case FR_ADD: return launch_op<FR_ADD>(s, d_dst, d_a, d_b, n, b_one);
    case FR_SUB: return launch_op<FR_SUB>(s, d_dst, d_a, d_b, n, b_one);
    case FR_MUL: return launch_op<FR_MUL>(s, d_dst, d_a, d_b, n, b_one);
    case FR_SQR: return launch_op<FR_SQR>(s, d_dst, d_a, d_b, n, b_one);
    case FR_NEG: return launch_op<FR_NEG>(s, d_dst, d_a, d_b, n, b_one);
    case FR_FROM_SCALAR: return launch_op<FR_FROM_SCALAR>(s, d_dst, d_a, d_b, n, b_one);
    case FR_TO_SCALAR: return launch_op<FR_TO_SCALAR>(s, d_dst, d_a, d_b, n, b_one);
    case FR_INV: break;
    default: throw std::runtime_error("fr_op: unknown op");
  }
  // one batch inversion over the chunk: the tree of to_affine.hip
  const std::vector<size_t> lvs = ta_levels(n);
  std::vector<uint32_t *> L(lvs.size());
  size_t off = 0;
  for (size_t i = 0; i < lvs.size(); ++i) {
    L[i] = lv_.as<uint32_t>() + off * 8;
    off += lvs[i];
  }
  if (off * EL > lv_.bytes) throw std::runtime_error("fr_op: level buffer too small");
  const unsigned B = 128;
  const uint32_t *a = static_cast<const uint32_t *>(d_a);
  hipLaunchKernelGGL(k_fr_up<true>, dim3(nblk(lvs[0], B)), dim3(B), 0, s, a, n, L[0], lvs[0]);
  MSM_HIP_CHECK(hipGetLastError());
  for (size_t i = 1; i < lvs.size(); ++i) {
    hipLaunchKernelGGL(k_fr_up<false>, dim3(nblk(lvs[i], B)), dim3(B), 0, s, (const uint32_t *)L[i - 1], lvs[i - 1],
                       L[i], lvs[i]);
    MSM_HIP_CHECK(hipGetLastError());
  }
  const size_t top = lvs.size() - 1;
  hipLaunchKernelGGL(k_fr_leaf, dim3(nblk(lvs[top], 64)), dim3(64), 0, s, L[top], lvs[top]);
  MSM_HIP_CHECK(hipGetLastError());
  for (size_t i = top; i >= 1; --i) {
    hipLaunchKernelGGL(k_fr_down<false>, dim3(nblk(lvs[i], B)), dim3(B), 0, s, (const uint32_t *)L[i], lvs[i],
                       L[i - 1], lvs[i - 1], (uint32_t *)nullptr);
    MSM_HIP_CHECK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_fr_down<true>, dim3(nblk(lvs[0], B)), dim3(B), 0, s, (const uint32_t *)L[0], lvs[0],
                     const_cast<uint32_t *>(a), n, static_cast<uint32_t *>(d_dst));
  MSM_HIP_CHECK(hipGetLastError());
}

void FrNtt::op(hipStream_t cs, int op, void *dst, const void *a, const void *b, size_t n, bool b_one, bool src_dev,
               bool dst_dev) {
  if (!n) return;
  DeviceGuard g(dev_);
  const bool two = fr_op_binary(op);
  const size_t C = std::min(n, ntt_chunk());
  if (op == FR_INV) lv_.ensure(ta_level_elems(C) * EL);
  if (!src_dev) in_.ensure(C * EL);
  if (!src_dev && two) inb_.ensure(b_one ? EL : C * EL);
  if (!dst_dev) out_.ensure(C * EL);
  pipe_.begin(cs);
  auto pend = pipe_.pending([&](int slot, size_t off, size_t cnt) {
    memcpy(static_cast<uint8_t *>(dst) + off * EL, out_.pin[slot], cnt * EL);
  });
  size_t k = 0;
  for (size_t c0 = 0; c0 < n; c0 += C, ++k) {
    const size_t cnt = std::min(C, n - c0);
    const int slot = (int)(k & 1);
    const void *d_a, *d_b = nullptr;
    void *d_dst;
    if (!src_dev) {
      const size_t bb = !two ? 0 : b_one ? EL : cnt * EL;  // bytes of the second operand
      pipe_.upload(cs, slot, [&] {
        memcpy(in_.pin[slot], static_cast<const uint8_t *>(a) + c0 * EL, cnt * EL);
        if (two) memcpy(inb_.pin[slot], static_cast<const uint8_t *>(b) + (b_one ? 0 : c0 * EL), bb);
      }, {{in_, slot, cnt * EL}, {inb_, slot, bb}});
      d_a = in_.dev[slot].p;
      if (two) d_b = inb_.dev[slot].p;
    } else {
      d_a = static_cast<const uint8_t *>(a) + c0 * EL;
      if (two) d_b = static_cast<const uint8_t *>(b) + (b_one ? 0 : c0 * EL);
    }
    if (!dst_dev) {
      pipe_.out_open(cs, slot);
      d_dst = out_.dev[slot].p;
    } else {
      d_dst = static_cast<uint8_t *>(dst) + c0 * EL;
    }
    op_kernels(cs, op, d_dst, d_a, d_b, cnt, b_one);
    pipe_.computed(cs, slot);
    if (!dst_dev) pipe_.download(cs, slot, pend, c0, cnt, {{out_, slot, cnt * EL}});
  }
  pend.flush();
  pipe_.finish(cs);
}

void fr_probe(int device, double out[2]) {
  DeviceGuard g(device);
  const unsigned blocks = 256 * 8, threads = 256;
  const int iters = 2048;
  DevBuf buf;
  buf.ensure((size_t)blocks * threads * sizeof(uint32_t));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipStream_t s = nullptr;
  try {
    MSM_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    MSM_HIP_CHECK(hipEventCreate(&e0));
    MSM_HIP_CHECK(hipEventCreate(&e1));
    hipLaunchKernelGGL(k_fr_probe, dim3(blocks), dim3(threads), 0, s, buf.as<uint32_t>(), 16);  // warm-up
    MSM_HIP_CHECK(hipEventRecord(e0, s));
    hipLaunchKernelGGL(k_fr_probe, dim3(blocks), dim3(threads), 0, s, buf.as<uint32_t>(), iters);
    MSM_HIP_CHECK(hipGetLastError());
    MSM_HIP_CHECK(hipEventRecord(e1, s));
    MSM_HIP_CHECK(hipEventSynchronize(e1));
    float ms = 0;
    MSM_HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
    out[0] = 2.0 * iters * blocks * threads / (ms * 1e-3);
    out[1] = ms;
  } catch (...) {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (s) (void)hipStreamDestroy(s);
    throw;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipStreamSynchronize(s);
  (void)hipStreamDestroy(s);
}

}  // namespace msm
