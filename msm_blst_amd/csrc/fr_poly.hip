// fr_poly.hip -- msm_fr_eval_quotient on one MI355X: y_j = f_j(z_j) and the
// quotient (f_j - y_j) / (X - z_j) of many polynomials held as their values on the
// domain of the NTT (the step between "evaluations" and "the scalars of a KZG
// proof"; formulas and forms in fr_quot.hpp).
//
// Three kernels per chunk of whole polynomials:
//   k_poly_partial  one workgroup of 256 lanes per TILE of 2^t elements (t = 10: four
//                   per lane).  The n inversions d_i = 1 / (z - x_i) are one batch
//                   inversion per tile: per-lane prefix products, a binary product
//                   tree over the lanes in LDS, ONE Fermat chain per workgroup, and
//                   the way back down.  The tiles of all polynomials of the chunk are
//                   one grid, so the dependent Fermat chains of different workgroups
//                   overlap (no launch waits for a leaf, as the chunks of MSM_FR_INV
//                   do).  Each tile leaves its partial sums S, T, and its d_i when a
//                   quotient is wanted.
//   k_poly_finish   one workgroup per polynomial adds the partial sums of its tiles
//                   and one lane forms y and q_m (fq_finish).
//   k_poly_quot     elementwise q_i = (y - f_i) d_i, the byte form already in d_i.
// Domain points come from power tables built by fr_ntt.hip's k_fr_pow_table.
#include "fr_poly.hpp"

#include <cstring>
#include <type_traits>

#include "fr_mem.hpp"
#include "fr_ntt.hpp"
#include "fr_quot.hpp"

namespace msm {

namespace {

constexpr int EPL = 4;         // elements per lane (256 lanes x 4 = the largest tile)
constexpr uint32_t LDS_N = 512;  // nodes of the product tree (511 used); later the two sum trees

struct PolyArgs {
  const uint32_t *f, *z;  // the polynomials and points of the chunk
  uint32_t *d;            // the inverses, or NULL (no quotient wanted)
  uint32_t *part;         // per tile: S, T
  uint32_t *fm;           // per polynomial: f_m, written by the lane that meets z = x_m
  const uint32_t *lo, *hi;
  int lb, log_n, log_t, flags;
};

// planar LDS: limb l of node e at l LDS_N + e
__device__ __forceinline__ void node_ld(Fr &r, const uint32_t *lds, uint32_t e) {
#pragma unroll
  for (int l = 0; l < FR_NL; ++l) r.v[l] = lds[l * LDS_N + e];
}
__device__ __forceinline__ void node_st(uint32_t *lds, uint32_t e, const Fr &a) {
#pragma unroll
  for (int l = 0; l < FR_NL; ++l) lds[l * LDS_N + e] = a.v[l];
}
// keeps a value that is uniform over the workgroup (z_j, a kernel argument) in vector
// registers, so the field arithmetic on it is not moved to the scalar unit
__device__ __forceinline__ void fr_vec(Fr &a) {
#pragma unroll
  for (int i = 0; i < FR_NL; ++i) asm volatile("" : "+v"(a.v[i]));
}
// first node of level l of the tree over 256 lanes (level l has 256 >> l nodes)
__device__ __forceinline__ uint32_t lvl_at(int l) { return LDS_N - (LDS_N >> l); }

// x_i: the domain point at position i of a polynomial, exact and canonical
__device__ __forceinline__ void dom_point(Fr &x, const PolyArgs &A, uint32_t i) {
  uint32_t e = i;
  if (A.flags & POLYF_BITREV) e = A.log_n ? __brev(i) >> (32 - A.log_n) : 0;
  fr_ld(x, A.lo + (size_t)(e & ((1u << A.lb) - 1)) * 8);
  if (A.hi) {
    Fr h;
    fr_ld(h, A.hi + (size_t)(e >> A.lb) * 8);
    fr_mul(x, x, h);
    fr_csub(x);
  }
}

// the sums of 256 lanes: S in nodes 0..255, T in nodes 256..511 -> lane 0's S, T
__device__ __forceinline__ void sum_lanes(uint32_t *lds, Fr &S, Fr &T, uint32_t tid) {
  node_st(lds, tid, S);
  node_st(lds, 256 + tid, T);
  __syncthreads();
#pragma unroll 1
  for (uint32_t s = 128; s >= 1; s >>= 1) {
    if (tid < s) {
      Fr a, b;
      node_ld(a, lds, tid);
      node_ld(b, lds, tid + s);
      fq_sum(a, b);
      node_st(lds, tid, a);
      node_ld(a, lds, 256 + tid);
      node_ld(b, lds, 256 + tid + s);
      fq_sum(a, b);
      node_st(lds, 256 + tid, a);
    }
    __syncthreads();
  }
  node_ld(S, lds, 0);
  node_ld(T, lds, 256);
  fr_vec(S);
  fr_vec(T);
}

static __global__ void __launch_bounds__(256) k_poly_partial(const PolyArgs A) {
  __shared__ uint32_t lds[FR_NL * LDS_N];
  const uint32_t tid = threadIdx.x;
  const int lt = A.log_t, ltp = A.log_n - lt;  // log2 of the tile, of the tiles of a polynomial
  const uint32_t E = 1u << lt;
  const size_t tile = blockIdx.x, j = tile >> ltp;
  const uint32_t base = ((uint32_t)tile & ((1u << ltp) - 1)) << lt;  // the tile's first position

  Fr zt;
  fr_ld(zt, A.z + j * 8);
  fr_vec(zt);
  fq_point(zt, zt);

  // ---- u_k = z - x_k (1 where it is zero, and past the tile) and their prefix products ----
  Fr u[EPL], p[EPL];
  uint32_t zmask = 0;
#pragma unroll
  for (int k = 0; k < EPL; ++k) {
    const uint32_t l = k * 256 + tid;
    if (l < E) {
      Fr x;
      dom_point(x, A, base + l);
      if (fq_diff(u[k], zt, x)) zmask |= 1u << k;
    } else {
      fr_one(u[k]);
      zmask |= 1u << k;
    }
    if (k == 0) p[0] = u[0];
    else fr_mul(p[k], p[k - 1], u[k]);
  }

  // ---- the product tree over the lanes, one inversion, and back down ----
  node_st(lds, tid, p[EPL - 1]);
  __syncthreads();
#pragma unroll 1
  for (int l = 1; l <= 8; ++l) {
    if (tid < (256u >> l)) {
      Fr a, b;
      node_ld(a, lds, lvl_at(l - 1) + 2 * tid);
      node_ld(b, lds, lvl_at(l - 1) + 2 * tid + 1);
      fr_mul(a, a, b);
      node_st(lds, lvl_at(l) + tid, a);
    }
    __syncthreads();
  }
  if (tid == 0) {
    Fr a, r;
    node_ld(a, lds, lvl_at(8));
    fr_vec(a);
    fq_inv(r, a);
    if (A.flags & POLYF_DST_SCALAR) fr_mulc(r, r, FR_C32);  // every d_i inherits the 2^-256
    node_st(lds, lvl_at(8), r);
  }
  __syncthreads();
#pragma unroll 1
  for (int l = 8; l >= 1; --l) {
    if (tid < (256u >> l)) {
      Fr I, a, b;
      node_ld(I, lds, lvl_at(l) + tid);
      node_ld(a, lds, lvl_at(l - 1) + 2 * tid);
      node_ld(b, lds, lvl_at(l - 1) + 2 * tid + 1);
      fr_mul(b, I, b);
      fr_mul(a, I, a);
      node_st(lds, lvl_at(l - 1) + 2 * tid, b);
      node_st(lds, lvl_at(l - 1) + 2 * tid + 1, a);
    }
    __syncthreads();
  }
  Fr I;
  node_ld(I, lds, tid);
  __syncthreads();  // (the sums reuse the nodes)

  // ---- d_k from the lane's inverse, the two sums ----
  Fr S, T;
  fr_zero(S);
  fr_zero(T);
  const auto term = [&](auto kc) __attribute__((always_inline)) {
    constexpr int k = decltype(kc)::value;
    Fr d, zero;
    if constexpr (k > 0) {
      fr_mul(d, I, p[k - 1]);
      fr_mul(I, I, u[k]);
    } else {
      d = I;
    }
    fr_csub(d);
    fr_zero(zero);
    const bool isz = (zmask >> k) & 1;
    fr_sel(d, isz, zero);
    const uint32_t l = k * 256 + tid;
    if (l < E) {
      const size_t at = ((j << A.log_n) + base + l) * 8;
      Fr f;
      fr_ld(f, A.f + at);
      if (isz) fr_st(A.fm + j * 8, f);  // z = x_m: at most one lane of the polynomial
      fq_term(S, T, zt, u[k], d, f);
      if (A.d) fr_st(A.d + at, d);
    }
  };
  static_assert(EPL == 4, "the terms below");
  term(std::integral_constant<int, 3>{});
  term(std::integral_constant<int, 2>{});
  term(std::integral_constant<int, 1>{});
  term(std::integral_constant<int, 0>{});
  sum_lanes(lds, S, T, tid);
  if (tid == 0) {
    fr_csub(S);
    fr_csub(T);
    fr_st(A.part + tile * 16, S);
    fr_st(A.part + tile * 16 + 8, T);
  }
}

// y[j], qm[j] of polynomial j = blockIdx.x from the partial sums of its 2^ltp tiles
static __global__ void __launch_bounds__(256)
    k_poly_finish(uint32_t *y, uint32_t *qm, const uint32_t *part, const uint32_t *fm, const uint32_t *z, int log_n,
                  int ltp, const FrK ninv, int scalar) {
  __shared__ uint32_t lds[FR_NL * LDS_N];
  const uint32_t tid = threadIdx.x;
  const size_t j = blockIdx.x, nt = (size_t)1 << ltp;
  Fr S, T;
  fr_zero(S);
  fr_zero(T);
  for (size_t t = tid; t < nt; t += 256) {
    Fr a;
    fr_ld(a, part + ((j << ltp) + t) * 16);
    fq_sum(S, a);
    fr_ld(a, part + ((j << ltp) + t) * 16 + 8);
    fq_sum(T, a);
  }
  sum_lanes(lds, S, T, tid);
  if (tid == 0) {
    Fr zt, f, k, yy, q;
    fr_ld(zt, z + j * 8);
    fr_vec(zt);
    fq_point(zt, zt);
    fr_ld(f, fm + j * 8);  // (meaningful only when z is in the domain)
    fr_vec(f);
    fr_arg(k, ninv);
    fr_vec(k);
    fq_finish(yy, q, zt, S, T, f, k, log_n, scalar != 0);
    fr_st(y + j * 8, yy);
    fr_st(qm + j * 8, q);
  }
}

static __global__ void __launch_bounds__(256)
    k_poly_quot(uint32_t *q, const uint32_t *f, const uint32_t *d, const uint32_t *y, const uint32_t *qm, int log_n,
                size_t total) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const size_t j = i >> log_n;
  Fr yy, ff, dd, mm, r;
  fr_ld(yy, y + j * 8);
  fr_ld(mm, qm + j * 8);
  fr_ld(ff, f + i * 8);
  fr_ld(dd, d + i * 8);
  fq_quot(r, yy, ff, dd, mm);
  fr_st(q + i * 8, r);
}

}  // namespace

size_t FrPoly::device_bytes() const {
  size_t b = d_.bytes + part_.bytes + fm_.bytes + qm_.bytes + in_.device_bytes() + inz_.device_bytes() +
             outq_.device_bytes() + outy_.device_bytes();
  for (const auto &kv : tw_) b += kv.second.buf.bytes;
  return b;
}

const FrPoly::Table &FrPoly::table(hipStream_t s, int log_n) {
  auto it = tw_.find(log_n);
  if (it != tw_.end()) return it->second;
  Table t;
  t.lb = std::min(log_n, 12);
  const size_t n_lo = (size_t)1 << t.lb, n_hi = (size_t)1 << (log_n - t.lb);
  t.buf.ensure((n_lo + (n_hi > 1 ? n_hi : 0)) * EL);
  uint32_t *p = t.buf.as<uint32_t>();
  const hfr::Fr w = hfr::root_of_unity((unsigned)log_n);
  fr_pow_table(s, p, n_lo, w, hfr::ONE);
  t.lo = p;
  if (n_hi > 1) {
    fr_pow_table(s, p + n_lo * 8, n_hi, hfr::pow2k(w, (unsigned)t.lb), hfr::ONE);
    t.hi = p + n_lo * 8;
  }
  return tw_.emplace(log_n, std::move(t)).first->second;
}

// one chunk of whole polynomials, device to device
void FrPoly::kernels(hipStream_t s, const void *d_f, const void *d_z, void *d_y, void *d_q, int log_n, size_t count,
                     int flags) {
  const Table &t = table(s, log_n);
  PolyArgs A;
  memset(&A, 0, sizeof A);
  A.f = static_cast<const uint32_t *>(d_f);
  A.z = static_cast<const uint32_t *>(d_z);
  A.d = d_q ? d_.as<uint32_t>() : nullptr;
  A.part = part_.as<uint32_t>();
  A.fm = fm_.as<uint32_t>();
  A.lo = t.lo, A.hi = t.hi, A.lb = t.lb;
  A.log_n = log_n;
  A.log_t = std::min(poly_tile(), log_n);
  A.flags = flags;
  const int ltp = log_n - A.log_t;
  const size_t tiles = count << ltp, total = count << log_n;
  if (tiles * 2 * EL > part_.bytes || count * EL > fm_.bytes || (d_q && total * EL > d_.bytes))
    throw std::runtime_error("fr_eval_quotient: chunk buffers too small");
  hipLaunchKernelGGL(k_poly_partial, dim3((unsigned)tiles), dim3(256), 0, s, A);
  MSM_HIP_CHECK(hipGetLastError());
  const hfr::Fr ninv = hfr::inverse(hfr::from_u64((uint64_t)1 << log_n));
  hipLaunchKernelGGL(k_poly_finish, dim3((unsigned)count), dim3(256), 0, s, static_cast<uint32_t *>(d_y),
                     qm_.as<uint32_t>(), (const uint32_t *)A.part, (const uint32_t *)A.fm, A.z, log_n, ltp,
                     fr_internal(ninv), (flags & POLYF_DST_SCALAR) ? 1 : 0);
  MSM_HIP_CHECK(hipGetLastError());
  if (d_q) {
    hipLaunchKernelGGL(k_poly_quot, dim3(nblk(total, 256)), dim3(256), 0, s, static_cast<uint32_t *>(d_q), A.f,
                       (const uint32_t *)A.d, (const uint32_t *)d_y, (const uint32_t *)qm_.as<uint32_t>(), log_n,
                       total);
    MSM_HIP_CHECK(hipGetLastError());
  }
}

void FrPoly::run(hipStream_t cs, const void *polys, const void *z, void *y, void *q, int log_n, size_t count,
                 int flags, bool src_dev, bool dst_dev) {
  if (!count) return;
  DeviceGuard g(dev_);
  const size_t per = std::min(count, std::max<size_t>(1, poly_chunk() >> log_n));  // polynomials per chunk
  const size_t C = per << log_n;
  const int ltp = log_n - std::min(poly_tile(), log_n);
  if (q) d_.ensure(C * EL);
  part_.ensure((per << ltp) * 2 * EL);
  fm_.ensure(per * EL);
  qm_.ensure(per * EL);
  if (!src_dev) in_.ensure(C * EL), inz_.ensure(per * EL);
  if (!dst_dev) outy_.ensure(per * EL);
  if (!dst_dev && q) outq_.ensure(C * EL);
  pipe_.begin(cs);  // the chunk buffers and tables of the previous call
  auto pend = pipe_.pending([&](int slot, size_t c0, size_t nb) {
    memcpy(static_cast<uint8_t *>(y) + c0 * EL, outy_.pin[slot], nb * EL);
    if (q) memcpy(static_cast<uint8_t *>(q) + (c0 << log_n) * EL, outq_.pin[slot], (nb << log_n) * EL);
  });
  size_t k = 0;
  for (size_t c0 = 0; c0 < count; c0 += per, ++k) {
    const size_t nb = std::min(per, count - c0), cnt = nb << log_n, off = c0 << log_n;
    const int slot = (int)(k & 1);
    const void *d_f, *d_z;
    void *d_y, *d_q = nullptr;
    if (!src_dev) {
      pipe_.upload(cs, slot, [&] {
        memcpy(in_.pin[slot], static_cast<const uint8_t *>(polys) + off * EL, cnt * EL);
        memcpy(inz_.pin[slot], static_cast<const uint8_t *>(z) + c0 * EL, nb * EL);
      }, {{in_, slot, cnt * EL}, {inz_, slot, nb * EL}});
      d_f = in_.dev[slot].p;
      d_z = inz_.dev[slot].p;
    } else {
      d_f = static_cast<const uint8_t *>(polys) + off * EL;
      d_z = static_cast<const uint8_t *>(z) + c0 * EL;
    }
    if (!dst_dev) {
      pipe_.out_open(cs, slot);
      d_y = outy_.dev[slot].p;
      if (q) d_q = outq_.dev[slot].p;
    } else {
      d_y = static_cast<uint8_t *>(y) + c0 * EL;
      if (q) d_q = static_cast<uint8_t *>(q) + off * EL;
    }
    kernels(cs, d_f, d_z, d_y, d_q, log_n, nb, flags);
    pipe_.computed(cs, slot);
    if (!dst_dev) pipe_.download(cs, slot, pend, c0, nb, {{outy_, slot, nb * EL}, {outq_, slot, q ? cnt * EL : 0}});
  }
  pend.flush();
  pipe_.finish(cs);
}

}  // namespace msm
