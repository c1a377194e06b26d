// abi.cpp -- extern "C" boundary of libmsm_mi355x.so (include/msm_mi355x.h).
//
// The blst-named entry points reproduce the reference's calling convention
// (ref src/multi_scalar.c:581-607: arrays of pointers with the {ptr, NULL}
// flat shortcut, scalars packed with stride (nbits+7)/8) and run the MSM on
// the GPU; the msm_* functions expose device-resident contexts.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/msm_mi355x.h"
#include "decode.hpp"
#include "encode.hpp"
#include "engine.hpp"
#include "fr_ntt.hpp"
#include "fp_ops_test.hpp"
#include "fr_poly.hpp"
#include "hash_to_curve.hpp"
#include "host_fr.hpp"
#include "kzg.hpp"
#include "multi.hpp"
#include "pairing.hpp"
#include "point_segments.hpp"
#include "points_mult.hpp"
#include "points_ntt.hpp"
#include "points_ntt_model.hpp"
#include "pool.hpp"
#include "ptr_walk.hpp"
#include "sig_verify.hpp"
#include "table_registry.hpp"
#include "to_affine.hpp"

using namespace msm;

namespace {
thread_local std::string g_err;

int fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}

// window of the blst drop-in's plain Pippenger: the fastest c measured on
// MI355X per n (tools/window_sweep.py, profiles/archive_r01_r04.txt (r03_window_sweep.json); blst's
// own rule, multi_scalar.c:268-275, picks smaller windows: CPU buckets are
// cache-bound, GPU lanes want enough buckets to fill the chip)
int auto_window(size_t n) {
  int lg = 0;
  while (((size_t)1 << (lg + 1)) <= n) ++lg;
  if (lg <= 8) return 8;
  if (lg <= 10) return 10;
  if (lg <= 12) return 12;
  if (lg == 13) return 13;
  if (lg <= 16) return 14;
  if (lg <= 21) return 16;
  return 17;
}

// Failure inside a void blst-named entry point.  Default: print and abort (a
// wrong answer is never returned silently).  With msm_set_abort_on_error(0) the
// call instead returns with `ret` set to the all-zero point (infinity), the
// message in msm_last_error() and msm_error_pending() raised for the caller.
std::atomic<int> g_abort_on_error{1};
thread_local int g_pending = 0;
void die(const char *where, const std::exception &e, void *ret = nullptr, size_t ret_bytes = 0) {
  if (g_abort_on_error.load()) {
    fprintf(stderr, "msm_mi355x: %s failed: %s\n", where, e.what());
    fflush(stderr);
    abort();
  }
  g_err = std::string(where) + " failed: " + e.what();
  g_pending = 1;
  if (ret) memset(ret, 0, ret_bytes);
}

// ---- what the entry points share ----
// body() -> int under the boundary's catch: a std::exception becomes `code` (the
// entry point's own: most give MSM_E_HIP, a few MSM_E_ARG) with its message in
// msm_last_error(), after on_throw() has done the call's own clean-up.
template <class Body, class OnThrow>
int guarded(int code, Body body, OnThrow on_throw) {
  try {
    return body();
  } catch (const std::exception &e) {
    on_throw();
    return fail(code, e.what());
  }
}
template <class Body>
int guarded(int code, Body body) {
  return guarded(code, body, [] {});
}

// the same for a void blst-named entry point; `where` is its exported name
template <class Body>
void blst_guarded(const char *where, void *ret, size_t ret_bytes, Body body) {
  try {
    body();
  } catch (const std::exception &e) {
    die(where, e, ret, ret_bytes);
  }
}

// f(std::integral_constant<int, G>{}) for the group G.  A group other than 1 runs
// as 2, as in the if / else pairs this replaces; most callers checked it before.
template <class F>
decltype(auto) by_group(int group, F f) {
  if (group == 1) return f(std::integral_constant<int, 1>{});
  return f(std::integral_constant<int, 2>{});
}

bool device_ok(int dev) {
  const int ndev = msm_device_count();
  return dev >= 0 && dev < ndev;
}
int no_device() { return fail(MSM_E_NODEV, "no such HIP device"); }

// on_throw of the bulk calls: a host destination is never left half written
void zero_host(void *dst, size_t bytes, bool dst_dev) {
  if (dst && !dst_dev) memset(dst, 0, bytes);
}

// The status bytes of n items of a bulk call that also counts its failures: the
// caller's, or a buffer of our own when the caller gave none and wants the count.
struct StatusBytes {
  std::vector<uint8_t> own;
  uint8_t *p;
  StatusBytes(uint8_t *status, size_t n, bool counted) : p(status) {
    if (!p && counted) {
      own.resize(n);
      p = own.data();
    }
  }
  size_t count_not(size_t n, uint8_t good) const { return n - (size_t)std::count(p, p + n, good); }
};

template <int G>
std::unique_ptr<typename EnginePool<Pippenger<G>>::Lease> pippenger_engine(int window) {
  int dev = 0;
  MSM_HIP_CHECK(hipGetDevice(&dev));
  return EnginePool<Pippenger<G>>::get().lease(dev, window,
                                               [&] { return std::make_unique<Pippenger<G>>(dev, window); });
}

// The device rows of n points at `pts` when a registered host table holds all
// of them (msm_register_host_table; table_registry.hpp), else nullptr.  `hold`
// keeps the table alive for the call.
template <int G>
const void *registered_rows(const uint8_t *pts, size_t n, std::shared_ptr<HostTable> &hold) {
  int dev = 0;
  MSM_HIP_CHECK(hipGetDevice(&dev));
  std::shared_ptr<HostTable> t = TableRegistry::get().find(G, dev, pts);
  if (!t) return nullptr;
  const size_t off = (size_t)(pts - t->base) / (96 * G);
  if (off + n > t->nrows) return nullptr;
  t = fresh<G>(t, off, off + n - 1);  // rows edited since registration: re-uploaded
  if (!t) return nullptr;
  hold = t;
  return t->rows.template as<uint8_t>() + off * t->row_bytes;
}

template <int G>
void mult_pippenger(void *ret, const void *const *points, size_t n, const byte *const *scalars, size_t nbits) {
  typedef typename HostField<G>::F HF;
  hfp::Jac<HF> out;
  if (n == 0) {
    memset(&out, 0, sizeof out);
    memcpy(ret, &out, sizeof out);
    return;
  }
  const size_t nb = (nbits + 7) / 8;
  std::vector<uint8_t> pbuf, sbuf;
  const uint8_t *pts = contiguous(pbuf, points, n, 96 * G);
  const uint8_t *sc = contiguous(sbuf, (const void *const *)scalars, n, nb);
  std::shared_ptr<HostTable> hold;
  const void *rows = registered_rows<G>(pts, n, hold);  // points registered once: no upload
  auto eng = pippenger_engine<G>(auto_window(n));
  (*eng)->run_host(eng->stream(), pts, n, sc, nb, (int)nbits, &out, nullptr, rows);
  memcpy(ret, &out, sizeof out);
}

// one blst window tile (ref multi_scalar.c:383-419, 587-600): sum_i d_i P_i with
// d_i the Booth digit of scalar i at [bit0, bit0+wbits) (lookback bit bit0-1),
// digits and signs computed on the device (k_tile_booth)
template <int G>
void tile_pippenger(void *ret, const void *const *points, size_t n, const byte *const *scalars, size_t nbits,
                    size_t bit0, size_t window) {
  typedef typename HostField<G>::F HF;
  hfp::Jac<HF> out;
  memset(&out, 0, sizeof out);
  // bit0 == nbits is legal: the top tile of nbits = 256 with 8-bit windows holds
  // only the Booth carry of bit 255 (wbits = 0, cbits = 1; ref multi_scalar.c:596-599)
  if (n == 0) {
    memcpy(ret, &out, sizeof out);
    return;
  }
  if (bit0 > nbits || window == 0 || window > 24) throw std::runtime_error("tile outside the scalar bits");
  TileSpec t;
  t.bit0 = (int)bit0;
  if (bit0 + window > nbits) {
    t.wbits = (int)(nbits - bit0);
    t.cbits = t.wbits + 1;
  } else {
    t.wbits = t.cbits = (int)window;
  }
  const size_t nb = (nbits + 7) / 8;
  std::vector<uint8_t> pbuf, sbuf;
  const uint8_t *pts = contiguous(pbuf, points, n, 96 * G);
  const uint8_t *sc = contiguous(sbuf, (const void *const *)scalars, n, nb);
  std::shared_ptr<HostTable> hold;
  const void *rows = registered_rows<G>(pts, n, hold);
  auto eng = pippenger_engine<G>(8);
  (*eng)->run_host(eng->stream(), pts, n, sc, nb, (int)nbits, &out, &t, rows);
  memcpy(ret, &out, sizeof out);
}

// ---- blst-level CHES / BGMW95 tiles (ref multi_scalar.c:421-547, 671-744) ----
constexpr uint32_t kNone = 0xffffffffu;  // entry skipped (bucket sort key)

// The pointer-array tiles below hand the entries to entry_msm_ptrs (compat.hip):
// keys / vals are filled by the host worker pool straight into pinned memory
// and the n pointed-to rows are gathered chunk-wise through a pinned ring, so
// the host work runs in parallel and overlaps the DMA (at 2^20 CHES one call
// moves 12.6 M rows, 1.2 GB).
struct TileFill {
  const int *scalars;
  const unsigned char *signs;
  const int *v2i;    // d_CHES: bucket value -> index (0 = skipped)
  size_t nb;         // noindex / BGMW95: bucket range check
  int mode;          // 0 d_CHES, 1 noindexhash, 2 BGMW95
};
void tile_fill(void *ctx, size_t t0, size_t t1, uint32_t *keys, uint32_t *vals) {
  const TileFill &f = *static_cast<const TileFill *>(ctx);
  for (size_t t = t0; t < t1; ++t) {
    const int v = f.scalars[t];
    uint32_t key;
    if (f.mode == 0) {  // ref multi_scalar.c:421-463: entry t -> bucket v2i[scalars[t]]
      const int idx = f.v2i[v];
      key = idx > 0 ? (uint32_t)idx : kNone;
    } else if (f.mode == 1) {  // ref multi_scalar.c:466-503: buckets indexed by value
      if (v < 0 || (size_t)v >= f.nb) throw std::runtime_error("bucket value outside the bucket set range");
      key = v > 0 ? (uint32_t)v : kNone;
    } else {  // ref multi_scalar.c:506-547: value v in [1, q/2] -> bucket v - 1
      if (v < 0 || (size_t)v > f.nb) throw std::runtime_error("BGMW95 digit outside [0, q/2]");
      key = v > 0 ? (uint32_t)(v - 1) : kNone;
    }
    keys[t - t0] = key;
    vals[t - t0] = (uint32_t)t | ((uint32_t)(f.signs[t] != 0) << 31);
  }
}

// ref multi_scalar.c:421-463: entry t -> bucket v2i[scalars[t]] (0 = skipped),
// weight of bucket k = bucket_set_ascend[k]
template <int G>
void tile_d_ches(void *ret, const void *const *points, size_t n, const int *scalars, const unsigned char *signs,
                 void *buckets, const int *B, const int *v2i, size_t bsize) {
  std::vector<uint32_t> w(bsize);
  for (size_t k = 0; k < bsize; ++k) w[k] = (uint32_t)std::max(B[k], 0);
  TileFill f{scalars, signs, v2i, bsize, 0};
  entry_msm_ptrs<G>(ret, points, n, tile_fill, &f, bsize, w.data(), buckets);
}

// ref multi_scalar.c:466-503: buckets indexed by value; weight v for v in B, else 0
template <int G>
void tile_d_ches_noindex(void *ret, const void *const *points, size_t n, const int *scalars,
                         const unsigned char *signs, void *buckets, const int *B, size_t bsize) {
  if (bsize == 0) throw std::runtime_error("empty bucket set");
  const size_t nb = (size_t)B[bsize - 1] + 1;
  std::vector<uint32_t> w(nb, 0);
  for (size_t k = 1; k < bsize; ++k) w[B[k]] = (uint32_t)B[k];
  TileFill f{scalars, signs, nullptr, nb, 1};
  entry_msm_ptrs<G>(ret, points, n, tile_fill, &f, nb, w.data(), buckets);
}

// ref multi_scalar.c:671-744: standard q-ary digits, hash lookup and carry
// (written back into scalars[t + 1]) here, table slots 3 t + m - 1
template <int G>
void tile_ches_std(void *ret, const void *table, size_t n, int *scalars, const digit_decomposition *H, void *buckets,
                   const int *B, const int *v2i, size_t bsize) {
  std::vector<uint32_t> keys(n), vals(n), w(bsize);
  for (size_t t = 0; t < n; ++t) {
    const digit_decomposition d = H[scalars[t]];
    if (d.alpha) ++scalars[t + 1];
    int idx = v2i[d.b];
    keys[t] = idx > 0 ? (uint32_t)idx : kNone;
    vals[t] = (uint32_t)(3 * t + d.m - 1) | ((uint32_t)(d.alpha != 0) << 31);
  }
  for (size_t k = 0; k < bsize; ++k) w[k] = (uint32_t)std::max(B[k], 0);
  entry_msm<G>(ret, table, 3 * n, keys.data(), vals.data(), n, bsize, w.data(), buckets);
}

// ref multi_scalar.c:506-547: bucket value v in [1, q/2] -> bucket v - 1 of weight v
template <int G>
void tile_bgmw95(void *ret, const void *const *points, size_t n, const int *scalars, const unsigned char *signs,
                 void *buckets, size_t q_exp) {
  if (q_exp < 2 || q_exp > 26) throw std::runtime_error("q_exponent out of range");
  const size_t nb = (size_t)1 << (q_exp - 1);
  std::vector<uint32_t> w(nb);
  for (size_t k = 0; k < nb; ++k) w[k] = (uint32_t)(k + 1);
  TileFill f{scalars, signs, nullptr, nb, 2};
  entry_msm_ptrs<G>(ret, points, n, tile_fill, &f, nb, w.data(), nullptr);
  // the reference's integrate_buckets leaves buckets[0 .. q/2] zeroed
  if (buckets) memset(buckets, 0, (nb + 1) * 192 * G);
}

// sum_i P_i on the GPU: entries spread over up to 4096 buckets of weight 1
// (one lane accumulates each bucket), then the weighted reduction sums them
template <int G>
void points_add(void *ret, const void *const *points, size_t n) {
  std::vector<uint8_t> buf;
  const uint8_t *flat = contiguous(buf, points, n, 96 * G);
  const size_t nb = std::max<size_t>(1, std::min<size_t>(n, 4096));
  std::vector<uint32_t> keys(n), vals(n), w(nb, 1);
  for (size_t i = 0; i < n; ++i) {
    keys[i] = (uint32_t)(i % nb);
    vals[i] = (uint32_t)i;
  }
  entry_msm<G>(ret, flat, n, keys.data(), vals.data(), n, nb, w.data(), nullptr);
}

// ---- fixed-window MSM with a precomputed table (ref multi_scalar.c:63-261) ----
template <int G>
std::unique_ptr<typename EnginePool<Wbits<G>>::Lease> wbits_engine(int wbits) {
  int dev = 0;
  MSM_HIP_CHECK(hipGetDevice(&dev));
  return EnginePool<Wbits<G>>::get().lease(dev, wbits, [&] { return std::make_unique<Wbits<G>>(dev, wbits); });
}

// all points are read (pointer rule of ref multi_scalar.c:136: a NULL entry
// continues after the previous point) before the table is written, so the
// binding's in-place call (points at the end of the table, blst.hpp:383-393) works
template <int G>
void wbits_precompute(void *table, size_t wbits, const void *const *points, size_t n) {
  if (!n) return;
  std::vector<uint8_t> buf;
  const uint8_t *flat = contiguous(buf, points, n, 96 * G);
  auto eng = wbits_engine<G>((int)wbits);
  (*eng)->precompute(flat, n, false, eng->stream());
  (*eng)->get_table(table, 0, (*eng)->table_rows(), eng->stream());
}

// scalar pointer rule of ref multi_scalar.c:165,191: the first pointer is
// taken, then NULL continues after the previous scalar (stride (nbits+7)/8)
template <int G>
void wbits_mult(void *ret, const void *table, size_t wbits, size_t n, const byte *const *scalars, size_t nbits) {
  typedef typename HostField<G>::F HF;
  hfp::Jac<HF> out;
  memset(&out, 0, sizeof out);
  if (n && nbits) {
    const size_t nb = (nbits + 7) / 8;
    std::vector<uint8_t> buf;
    const uint8_t *sc = contiguous(buf, (const void *const *)scalars, n, nb);
    auto eng = wbits_engine<G>((int)wbits);
    hipStream_t s = eng->stream();
    (*eng)->set_table(table, n, false, s);
    (*eng)->upload_scalars(sc, n * nb, s);
    (*eng)->run(s, nullptr, nb, (int)nbits, &out);
  }
  memcpy(ret, &out, sizeof out);
}

// ---- the bulk point operations (engines on the chunk pipe, chunk_pipe.hpp) ----
// What their calls share: run(engine, cs) on a leased engine E (pool key
// `group`) of device `dev`.  cs orders the kernels: the caller's stream when a
// side is device memory, else the leased engine's own.
template <class E, class Run>
void bulk_run(int dev, int group, bool src_dev, bool dst_dev, hipStream_t user, Run run) {
  DeviceGuard g(dev);
  // work queued earlier on the caller's stream may still be writing the source:
  // device sources are read by kernels ordered on that stream; host sources are
  // read by this thread, so the stream is drained first
  if (!src_dev && user) MSM_HIP_CHECK(hipStreamSynchronize(user));
  auto eng = EnginePool<E>::get().lease(dev, group, [&] { return std::make_unique<E>(dev); });
  const bool on_user = src_dev || dst_dev;
  hipStream_t cs = on_user ? user : eng->stream();
  run(**eng, cs);
  // the legacy default stream gives the caller nothing to wait on: finish here
  if (on_user && !user && dst_dev) MSM_HIP_CHECK(hipStreamSynchronize(cs));
}

// the result of a bulk call whose every output is the point at infinity, in the place of bulk_run
void zero_fill(int dev, void *dst, size_t bytes, bool src_dev, bool dst_dev, hipStream_t user) {
  DeviceGuard g(dev);
  if (!src_dev && user) MSM_HIP_CHECK(hipStreamSynchronize(user));  // (as bulk_run does)
  if (dst_dev) MSM_HIP_CHECK(hipMemsetAsync(dst, 0, bytes, user));
  else memset(dst, 0, bytes);
  if (dst_dev && !user) MSM_HIP_CHECK(hipStreamSynchronize(user));
}

// ---- bulk Jacobian -> affine (ref multi_scalar.c:17-62) ----
constexpr int kCurrentDevice = -0x7fffffff;  // the blst-style calls: hipGetDevice

bool ranges_overlap(const void *a, size_t an, const void *b, size_t bn) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bn && y < x + an;
}

// runs: the host source as runs of adjacent points (ptr_walk.hpp), or empty
// with src_dev set.
template <int G>
int points_to_affine_checked(int dev, void *dst, const void *src_flat, const void *const *ptrs, size_t n,
                             bool src_dev, bool dst_dev, hipStream_t user) {
  typedef typename ToAffine<G>::Run Run;
  std::vector<Run> runs;
  if (!src_dev) {
    if (ptrs) walk_runs(ptrs, n, 144 * G, [&](size_t i, const uint8_t *p, size_t k) { runs.push_back(Run{i, p, k}); });
    else runs.push_back(Run{0, (const uint8_t *)src_flat, n});
    for (const Run &r : runs) {
      if (!r.p) return fail(MSM_E_ARG, "null point pointer");
      if (!dst_dev && ranges_overlap(r.p, r.count * 144 * G, dst, n * 96 * G))
        return fail(MSM_E_ARG, "source and destination overlap");
    }
  } else if (((uintptr_t)src_flat & 7) != 0) {
    return fail(MSM_E_ARG, "device source not 8-byte aligned");
  }
  if (dst_dev && ((uintptr_t)dst & 7) != 0) return fail(MSM_E_ARG, "device destination not 8-byte aligned");
  if (dev == kCurrentDevice ? msm_device_count() < 1 : !device_ok(dev)) return no_device();
  const auto on_throw = [&] { zero_host(dst, n * 96 * G, dst_dev); };
  return guarded(MSM_E_HIP, [&] {
    if (dev == kCurrentDevice) MSM_HIP_CHECK(hipGetDevice(&dev));
    bulk_run<ToAffine<G>>(dev, G, src_dev, dst_dev, user, [&](ToAffine<G> &e, hipStream_t cs) {
      e.run(cs, src_flat, runs, dst, n, src_dev, dst_dev);
    });
    return MSM_OK;
  }, on_throw);
}

// ---- bulk point decoding (ref e1.c:236-351, e2.c:279-410, map_to_g{1,2}.c in_g{1,2}) ----
// status: n host bytes or NULL.
int points_decode_checked(int group, int dev, void *dst, uint8_t *status, size_t *nbad, const void *src, size_t n,
                          int encoding, int flags, bool src_dev, bool dst_dev, hipStream_t user) {
  if (group != 1 && group != 2) return fail(MSM_E_ARG, "group must be 1 or 2");
  if (encoding != MSM_ENC_COMPRESSED && encoding != MSM_ENC_SERIALIZED) return fail(MSM_E_ARG, "unknown encoding");
  if (flags & ~MSM_DECODE_CHECK_GROUP) return fail(MSM_E_ARG, "unknown flag bits");
  if (n == 0) return MSM_OK;  // nothing touched
  if (!dst || !src) return fail(MSM_E_ARG, "null dst / src");
  if (n > ((size_t)1 << 40)) return fail(MSM_E_ARG, "npoints out of range");
  const bool ser = encoding == MSM_ENC_SERIALIZED;
  const size_t enc = (size_t)(ser ? 96 : 48) * group, aff = (size_t)96 * group;
  if (!src_dev && !dst_dev && ranges_overlap(src, n * enc, dst, n * aff))
    return fail(MSM_E_ARG, "source and destination overlap");
  if (status && ((!src_dev && ranges_overlap(src, n * enc, status, n)) ||
                 (!dst_dev && ranges_overlap(dst, n * aff, status, n))))
    return fail(MSM_E_ARG, "status overlaps the source or the destination");
  if (src_dev && ((uintptr_t)src & 3) != 0) return fail(MSM_E_ARG, "device source not 4-byte aligned");
  if (dst_dev && ((uintptr_t)dst & 7) != 0) return fail(MSM_E_ARG, "device destination not 8-byte aligned");
  if (!device_ok(dev)) return no_device();
  const auto on_throw = [&] {
    zero_host(dst, n * aff, dst_dev);
    if (status) memset(status, 1, n);
    if (nbad) *nbad = n;
  };
  return guarded(MSM_E_HIP, [&] {
    StatusBytes st(status, n, nbad != nullptr);
    by_group(group, [&](auto g) {
      constexpr int G = decltype(g)::value;
      bulk_run<Decode<G>>(dev, G, src_dev, dst_dev, user, [&](Decode<G> &e, hipStream_t cs) {
        e.run(cs, src, dst, st.p, n, ser, (flags & MSM_DECODE_CHECK_GROUP) != 0, src_dev, dst_dev);
      });
    });
    if (nbad) *nbad = st.count_not(n, 0);
    return MSM_OK;
  }, on_throw);
}

// ---- bulk point encoding (a loop over ref e1.c:139-234 and the e2.c twins) ----
int points_encode_checked(int group, int dev, void *dst, const void *src, size_t n, int src_form, int encoding,
                          int flags, bool src_dev, bool dst_dev, hipStream_t user) {
  if (group != 1 && group != 2) return fail(MSM_E_ARG, "group must be 1 or 2");
  if (src_form != MSM_SRC_AFFINE && src_form != MSM_SRC_JACOBIAN) return fail(MSM_E_ARG, "unknown source form");
  if (encoding != MSM_ENC_COMPRESSED && encoding != MSM_ENC_SERIALIZED) return fail(MSM_E_ARG, "unknown encoding");
  if (flags != 0) return fail(MSM_E_ARG, "unknown flag bits");
  if (n == 0) return MSM_OK;  // nothing touched
  if (!dst || !src) return fail(MSM_E_ARG, "null dst / src");
  if (n > ((size_t)1 << 40)) return fail(MSM_E_ARG, "npoints out of range");
  const bool jac = src_form == MSM_SRC_JACOBIAN, ser = encoding == MSM_ENC_SERIALIZED;
  const size_t pt = (size_t)(jac ? 144 : 96) * group, enc = (size_t)(ser ? 96 : 48) * group;
  if (!src_dev && !dst_dev && ranges_overlap(src, n * pt, dst, n * enc))
    return fail(MSM_E_ARG, "source and destination overlap");
  if (src_dev && ((uintptr_t)src & 7) != 0) return fail(MSM_E_ARG, "device source not 8-byte aligned");
  if (dst_dev && ((uintptr_t)dst & 3) != 0) return fail(MSM_E_ARG, "device destination not 4-byte aligned");
  if (!device_ok(dev)) return no_device();
  const auto on_throw = [&] { zero_host(dst, n * enc, dst_dev); };
  return guarded(MSM_E_HIP, [&] {
    by_group(group, [&](auto g) {
      constexpr int G = decltype(g)::value;
      bulk_run<Encode<G>>(dev, G, src_dev, dst_dev, user, [&](Encode<G> &e, hipStream_t cs) {
        e.run(cs, src, dst, n, jac, ser, src_dev, dst_dev);
      });
    });
    return MSM_OK;
  }, on_throw);
}

// ---- bulk scalar multiplication (a loop over ref e1.c:505-533 blst_p1_mult, e2.c, ec_mult.h) ----
template <int G>
void points_mult(int dev, void *dst, const void *points, const uint8_t *scalars, size_t n, int nbits, size_t stride,
                 bool one_point, bool src_dev, bool dst_dev, hipStream_t user) {
  if (nbits == 0) return zero_fill(dev, dst, n * 96 * G, src_dev, dst_dev, user);  // every scalar is zero
  bulk_run<PointsMult<G>>(dev, G, src_dev, dst_dev, user, [&](PointsMult<G> &e, hipStream_t cs) {
    e.run(cs, points, scalars, dst, n, nbits, stride, one_point, src_dev, dst_dev);
  });
}

int points_mult_checked(int group, int dev, void *dst, const void *points, const byte *scalars, size_t n, size_t nbits,
                        size_t stride, int flags, bool src_dev, bool dst_dev, hipStream_t user) {
  if (group != 1 && group != 2) return fail(MSM_E_ARG, "group must be 1 or 2");
  if (nbits > 256) return fail(MSM_E_ARG, "nbits must be at most 256");
  if (stride < (nbits + 7) / 8) return fail(MSM_E_ARG, "scalar_stride shorter than (nbits + 7) / 8");
  if (flags & ~MSM_MULT_ONE_POINT) return fail(MSM_E_ARG, "unknown flag bits");
  if (n == 0) return MSM_OK;  // nothing touched
  if (!dst || !points || !scalars) return fail(MSM_E_ARG, "null dst / points / scalars");
  if (n > ((size_t)1 << 40) || stride > ((size_t)1 << 20)) return fail(MSM_E_ARG, "npoints / scalar_stride out of range");
  const bool one = (flags & MSM_MULT_ONE_POINT) != 0;
  const size_t aff = (size_t)96 * group, pbytes = (one ? 1 : n) * aff, sbytes = (n - 1) * stride + (nbits + 7) / 8;
  if (!src_dev && !dst_dev && (ranges_overlap(points, pbytes, dst, n * aff) || ranges_overlap(scalars, sbytes, dst, n * aff)))
    return fail(MSM_E_ARG, "source and destination overlap");
  if (src_dev && ((uintptr_t)points & 7) != 0) return fail(MSM_E_ARG, "device points not 8-byte aligned");
  if (dst_dev && ((uintptr_t)dst & 7) != 0) return fail(MSM_E_ARG, "device destination not 8-byte aligned");
  if (!device_ok(dev)) return no_device();
  const auto on_throw = [&] { zero_host(dst, n * aff, dst_dev); };
  return guarded(MSM_E_HIP, [&] {
    by_group(group, [&](auto g) {
      points_mult<decltype(g)::value>(dev, dst, points, scalars, n, (int)nbits, stride, one, src_dev, dst_dev, user);
    });
    return MSM_OK;
  }, on_throw);
}

// ---- NTTs over group elements (csrc/points_ntt.hip) ----
int points_ntt_checked(int group, int dev, void *dst, const void *src, size_t log_n, size_t batch, int flags,
                       bool src_dev, bool dst_dev, hipStream_t user) {
  if (group != 1 && group != 2) return fail(MSM_E_ARG, "group must be 1 or 2");
  if (log_n > (size_t)PN_MAX_LOG) return fail(MSM_E_ARG, "log_n above 24");
  if (flags & ~(MSM_NTT_INVERSE | MSM_POLY_BITREV)) return fail(MSM_E_ARG, "unknown flag bits");
  if (batch == 0) return MSM_OK;  // nothing touched
  if (!dst || !src) return fail(MSM_E_ARG, "null dst / src");
  if (batch > (((size_t)1 << 40) >> log_n)) return fail(MSM_E_ARG, "batch out of range");
  const size_t bytes = (batch << log_n) * 96 * group;
  if (src_dev == dst_dev && dst != src && ranges_overlap(src, bytes, dst, bytes))
    return fail(MSM_E_ARG, "source and destination overlap");
  if (src_dev && ((uintptr_t)src & 7) != 0) return fail(MSM_E_ARG, "device source not 8-byte aligned");
  if (dst_dev && ((uintptr_t)dst & 7) != 0) return fail(MSM_E_ARG, "device destination not 8-byte aligned");
  if (!device_ok(dev)) return no_device();
  const auto on_throw = [&] { zero_host(dst, bytes, dst_dev); };
  return guarded(MSM_E_HIP, [&] {
    by_group(group, [&](auto g) {
      constexpr int G = decltype(g)::value;
      bulk_run<PointsNtt<G>>(dev, G, src_dev, dst_dev, user, [&](PointsNtt<G> &e, hipStream_t cs) {
        e.run(cs, src, dst, (int)log_n, batch, flags, src_dev, dst_dev);
      });
    });
    return MSM_OK;
  }, on_throw);
}

// ---- segmented sums and MSMs (a loop over ref multi_scalar.c:581-607 / bulk_addition.c:145-164 per point set) ----
template <int G>
void points_segments(int dev, void *dst, const void *points, const uint8_t *scalars, const size_t *offsets, size_t k,
                     int nbits, size_t stride, bool src_dev, bool dst_dev, hipStream_t user) {
  if ((scalars && nbits == 0) || offsets[k] == offsets[0])  // every scalar is zero, or every segment is empty
    return zero_fill(dev, dst, k * 96 * G, src_dev, dst_dev, user);
  bulk_run<PointSegments<G>>(dev, G, src_dev, dst_dev, user, [&](PointSegments<G> &e, hipStream_t cs) {
    e.run(cs, points, scalars, offsets, k, dst, nbits, stride, src_dev, dst_dev);
  });
}

int points_segments_checked(int group, int dev, void *dst, const void *points, const byte *scalars,
                            const size_t *offsets, size_t k, size_t nbits, size_t stride, int flags, bool src_dev,
                            bool dst_dev, hipStream_t user) {
  if (group != 1 && group != 2) return fail(MSM_E_ARG, "group must be 1 or 2");
  if (scalars) {
    if (nbits > 256) return fail(MSM_E_ARG, "nbits must be at most 256");
    if (stride < (nbits + 7) / 8) return fail(MSM_E_ARG, "scalar_stride shorter than (nbits + 7) / 8");
    if (stride > ((size_t)1 << 20)) return fail(MSM_E_ARG, "scalar_stride out of range");
  }
  if (flags != 0) return fail(MSM_E_ARG, "unknown flag bits");
  if (k == 0) return MSM_OK;  // nothing touched
  if (!dst || !points || !offsets) return fail(MSM_E_ARG, "null dst / points / offsets");
  if (k > ((size_t)1 << 40)) return fail(MSM_E_ARG, "nsegments out of range");
  if (!seg_offsets_ok(offsets, k)) return fail(MSM_E_ARG, "offsets decrease");
  const size_t n = offsets[k];
  if (n > ((size_t)1 << 40)) return fail(MSM_E_ARG, "offsets out of range");
  const size_t aff = (size_t)96 * group;
  if (!src_dev && !dst_dev && n > offsets[0] &&
      (ranges_overlap(points, n * aff, dst, k * aff) ||
       (scalars && nbits && ranges_overlap(scalars, (n - 1) * stride + (nbits + 7) / 8, dst, k * aff))))
    return fail(MSM_E_ARG, "source and destination overlap");
  if (src_dev && ((uintptr_t)points & 7) != 0) return fail(MSM_E_ARG, "device points not 8-byte aligned");
  if (dst_dev && ((uintptr_t)dst & 7) != 0) return fail(MSM_E_ARG, "device destination not 8-byte aligned");
  if (!device_ok(dev)) return no_device();
  const auto on_throw = [&] { zero_host(dst, k * aff, dst_dev); };
  return guarded(MSM_E_HIP, [&] {
    by_group(group, [&](auto g) {
      points_segments<decltype(g)::value>(dev, dst, points, scalars, offsets, k, (int)nbits, stride, src_dev, dst_dev,
                                          user);
    });
    return MSM_OK;
  }, on_throw);
}

// ---- bulk hash-to-curve (a loop over ref map_to_g{1,2}.c hash / encode / map, hash_to_field.c) ----
int hash_to_curve_checked(int group, int dev, int mode, void *dst, const void *u, const void *msgs,
                          const size_t *offsets, size_t msg_len, const void *aug, size_t aug_len, size_t n,
                          const byte *DST, size_t DST_len, int count, bool src_dev, bool dst_dev, hipStream_t user) {
  if (group != 1 && group != 2) return fail(MSM_E_ARG, "group must be 1 or 2");
  if (count != 1 && count != 2) return fail(MSM_E_ARG, "count must be 1 or 2");
  if (n == 0) return MSM_OK;  // nothing touched
  if (!dst) return fail(MSM_E_ARG, "null dst");
  if (n > ((size_t)1 << 40)) return fail(MSM_E_ARG, "npoints out of range");
  const size_t elem = (size_t)48 * group;
  const size_t out_bytes = n * (mode == H2C_FIELD ? count * elem : 2 * elem);
  H2cMsgs m;
  H2cTemplate tmpl;
  if (mode == H2C_MAP) {
    if (!u) return fail(MSM_E_ARG, "null u");
    if (src_dev && ((uintptr_t)u & 7) != 0) return fail(MSM_E_ARG, "device source not 8-byte aligned");
    if (!src_dev && !dst_dev && ranges_overlap(u, n * count * elem, dst, out_bytes))
      return fail(MSM_E_ARG, "source and destination overlap");
  } else {
    if (DST_len && !DST) return fail(MSM_E_ARG, "null DST");
    if (offsets && !seg_offsets_ok(offsets, n)) return fail(MSM_E_ARG, "offsets decrease");
    if (offsets)  // the kernel counts the bytes of a message in 32 bits
      for (size_t i = 0; i < n; ++i)
        if (offsets[i + 1] - offsets[i] > ((size_t)1 << 30)) return fail(MSM_E_ARG, "a message longer than 2^30 bytes");
    const size_t first = offsets ? offsets[0] : 0, last = offsets ? offsets[n] : n * msg_len;
    if (!offsets && msg_len > ((size_t)1 << 30)) return fail(MSM_E_ARG, "msg_len out of range");
    if (last > first && !msgs) return fail(MSM_E_ARG, "null msgs");
    if (aug_len > ((size_t)1 << 30)) return fail(MSM_E_ARG, "aug_len out of range");
    if (!src_dev && !dst_dev &&
        ((last > first && ranges_overlap((const uint8_t *)msgs + first, last - first, dst, out_bytes)) ||
         (aug && aug_len && ranges_overlap(aug, n * aug_len, dst, out_bytes))))
      return fail(MSM_E_ARG, "source and destination overlap");
    m.msgs = (const uint8_t *)msgs;
    m.offsets = offsets;
    m.msg_len = msg_len;
    m.aug = aug_len ? (const uint8_t *)aug : nullptr;
    m.aug_len = aug ? aug_len : 0;
    h2c_make_template(tmpl, DST, DST_len, (unsigned)(64 * count * group));
  }
  if (dst_dev && ((uintptr_t)dst & 7) != 0) return fail(MSM_E_ARG, "device destination not 8-byte aligned");
  if (!device_ok(dev)) return no_device();
  const auto on_throw = [&] { zero_host(dst, out_bytes, dst_dev); };
  return guarded(MSM_E_HIP, [&] {
    by_group(group, [&](auto g) {
      constexpr int G = decltype(g)::value;
      bulk_run<HashToCurve<G>>(dev, G, src_dev, dst_dev, user, [&](HashToCurve<G> &e, hipStream_t cs) {
        e.run(cs, mode, u, m, &tmpl, dst, n, count, src_dev, dst_dev);
      });
    });
    return MSM_OK;
  }, on_throw);
}

// ---- bulk pairings (a loop over ref pairing.c:181-262 miller_loop_n and 371-404 final_exp per pair) ----
// src: the Fp12 values of msm_fp12_final_exp (then p, q and offsets are unused), else NULL.
int pairing_checked(int dev, void *dst, uint8_t *is_one, size_t *nfail, const void *p, const void *q, const void *src,
                    const size_t *offsets, size_t k, int flags, bool fe_only, bool src_dev, bool dst_dev,
                    hipStream_t user) {
  if (flags & ~MSM_PAIRING_MILLER_ONLY) return fail(MSM_E_ARG, "unknown flag bits");
  const bool fe = !(flags & MSM_PAIRING_MILLER_ONLY);
  if (!fe && (is_one || nfail)) return fail(MSM_E_ARG, "is_one / nfail under MSM_PAIRING_MILLER_ONLY");
  if (k == 0) return MSM_OK;  // nothing touched
  if (!dst && !is_one && !nfail) return fail(MSM_E_ARG, "null dst without is_one / nfail");
  if (k > ((size_t)1 << 40)) return fail(MSM_E_ARG, "nsegments out of range");
  if (!dst) dst_dev = false;
  const size_t GT = Pairing::GT;
  size_t first = 0, last = k;  // the pairs read
  if (fe_only) {
    if (!src) return fail(MSM_E_ARG, "null src");
    if (!src_dev && dst && !dst_dev && ranges_overlap(src, k * GT, dst, k * GT))
      return fail(MSM_E_ARG, "source and destination overlap");
    if (src_dev && ((uintptr_t)src & 7) != 0) return fail(MSM_E_ARG, "device source not 8-byte aligned");
  } else {
    if (offsets) {
      if (!seg_offsets_ok(offsets, k)) return fail(MSM_E_ARG, "offsets decrease");
      first = offsets[0], last = offsets[k];
      if (last > ((size_t)1 << 40)) return fail(MSM_E_ARG, "offsets out of range");
    }
    if (last > first && (!p || !q)) return fail(MSM_E_ARG, "null p / q");
    if (!src_dev && dst && !dst_dev && last > first &&
        (ranges_overlap(p, last * Pairing::P_AFF, dst, k * GT) || ranges_overlap(q, last * Pairing::Q_AFF, dst, k * GT)))
      return fail(MSM_E_ARG, "source and destination overlap");
    if (src_dev && last > first && ((((uintptr_t)p) | ((uintptr_t)q)) & 7) != 0)
      return fail(MSM_E_ARG, "device points not 8-byte aligned");
  }
  if (dst_dev && ((uintptr_t)dst & 7) != 0) return fail(MSM_E_ARG, "device destination not 8-byte aligned");
  if (!device_ok(dev)) return no_device();
  const auto on_throw = [&] {
    zero_host(dst, k * GT, dst_dev);
    if (is_one) memset(is_one, 0, k);
    if (nfail) *nfail = k;
  };
  return guarded(MSM_E_HIP, [&] {
    StatusBytes st(is_one, k, nfail != nullptr);
    std::vector<size_t> single;  // offsets == NULL: one pair per segment
    if (!fe_only && !offsets) {
      single.resize(k + 1);
      for (size_t i = 0; i <= k; ++i) single[i] = i;
      offsets = single.data();
    }
    bulk_run<Pairing>(dev, 0, src_dev, dst_dev, user, [&](Pairing &e, hipStream_t cs) {
      if (fe_only) e.run_final_exp(cs, src, k, dst, st.p, src_dev, dst_dev);
      else e.run(cs, p, q, offsets, k, dst, st.p, fe, src_dev, dst_dev);
    });
    if (nfail) *nfail = st.count_not(k, 1);
    return MSM_OK;
  }, on_throw);
}

// ---- bulk signature verification (a loop over ref aggregate.c: core_verify, and the
// pairing_chk_n_[mul_n_]aggr / commit / finalverify sequence per check) ----
struct SigArgs {
  int mode, scheme, dev;
  uint8_t *status;
  size_t *nfail;
  const void *pks, *sigs, *msgs, *aug;
  const size_t *pk_offsets, *msg_offsets, *offsets;
  size_t msg_len, aug_len, k;
  const byte *scalars;
  size_t nbits, stride;
  const byte *DST;
  size_t DST_len;
  int flags;
  bool src_dev;
  hipStream_t user;
};

int sigs_checked(const SigArgs &a) {
  if (a.scheme != MSM_SIG_MIN_PK && a.scheme != MSM_SIG_MIN_SIG) return fail(MSM_E_ARG, "unknown scheme");
  if (a.flags & ~(MSM_H2C_ENCODE | MSM_SIG_ENCODED)) return fail(MSM_E_ARG, "unknown flag bits");
  const bool weighted = a.mode == SIG_BATCH && a.scalars && a.nbits;
  if (a.mode == SIG_BATCH && a.scalars) {
    if (a.nbits > 256) return fail(MSM_E_ARG, "nbits must be at most 256");
    if (a.stride < (a.nbits + 7) / 8) return fail(MSM_E_ARG, "scalar_stride shorter than (nbits + 7) / 8");
    if (a.stride > ((size_t)1 << 20)) return fail(MSM_E_ARG, "scalar_stride out of range");
  }
  const size_t k = a.k;
  if (k == 0) return MSM_OK;  // nothing touched
  if (!a.status && !a.nfail) return fail(MSM_E_ARG, "null status and nfail");
  if (k > ((size_t)1 << 40)) return fail(MSM_E_ARG, "nchecks out of range");
  if (a.mode != SIG_VERIFY) {
    if (!a.offsets) return fail(MSM_E_ARG, "null offsets");
    if (!seg_offsets_ok(a.offsets, k)) return fail(MSM_E_ARG, "offsets decrease");
    if (a.offsets[k] > ((size_t)1 << 40)) return fail(MSM_E_ARG, "offsets out of range");
  } else if (a.pk_offsets) {
    if (!seg_offsets_ok(a.pk_offsets, k)) return fail(MSM_E_ARG, "pk_offsets decrease");
    if (a.pk_offsets[k] > ((size_t)1 << 40)) return fail(MSM_E_ARG, "pk_offsets out of range");
  }
  const size_t r0 = sig_row_begin(a.mode, a.offsets, 0), r1 = sig_row_begin(a.mode, a.offsets, k);
  const size_t k0 = sig_key_begin(a.mode, a.offsets, a.pk_offsets, 0), k1 = sig_key_begin(a.mode, a.offsets, a.pk_offsets, k);
  const size_t s0 = sig_sig_begin(a.mode, a.offsets, 0), s1 = sig_sig_begin(a.mode, a.offsets, k);
  if (k1 > k0 && !a.pks) return fail(MSM_E_ARG, "null public keys");
  if (s1 > s0 && !a.sigs) return fail(MSM_E_ARG, "null signatures");
  if (a.DST_len && !a.DST) return fail(MSM_E_ARG, "null DST");
  if (a.aug_len > ((size_t)1 << 30)) return fail(MSM_E_ARG, "aug_len out of range");
  if (a.msg_offsets) {
    if (!seg_offsets_ok(a.msg_offsets, r1)) return fail(MSM_E_ARG, "message offsets decrease");
    for (size_t i = r0; i < r1; ++i)
      if (a.msg_offsets[i + 1] - a.msg_offsets[i] > ((size_t)1 << 30)) return fail(MSM_E_ARG, "a message longer than 2^30 bytes");
    if (a.msg_offsets[r1] > a.msg_offsets[r0] && !a.msgs) return fail(MSM_E_ARG, "null msgs");
  } else {
    if (a.msg_len > ((size_t)1 << 30)) return fail(MSM_E_ARG, "msg_len out of range");
    if (r1 > r0 && a.msg_len && !a.msgs) return fail(MSM_E_ARG, "null msgs");
  }
  const bool enc = (a.flags & MSM_SIG_ENCODED) != 0;
  if (a.src_dev && (((uintptr_t)a.pks | (uintptr_t)a.sigs) & (enc ? 3 : 7)) != 0)
    return fail(MSM_E_ARG, enc ? "device keys / signatures not 4-byte aligned" : "device keys / signatures not 8-byte aligned");
  if (!device_ok(a.dev)) return no_device();
  const auto on_throw = [&] {
    if (a.status) memset(a.status, SIG_VERIFY_FAIL, k);
    if (a.nfail) *a.nfail = k;
  };
  return guarded(MSM_E_HIP, [&] {
    StatusBytes st(a.status, k, true);  // (no status: nfail was asked for)
    SigCall c;
    c.mode = a.mode;
    c.encoded = enc;
    c.count = (a.flags & MSM_H2C_ENCODE) ? 1 : 2;
    c.keys = a.pks, c.sigs = a.sigs;
    c.scalars = weighted ? a.scalars : nullptr;
    c.nbits = weighted ? (int)a.nbits : 0;
    c.stride = a.stride;
    c.m.msgs = (const uint8_t *)a.msgs;
    c.m.offsets = a.msg_offsets;
    c.m.msg_len = a.msg_len;
    c.m.aug = a.aug_len ? (const uint8_t *)a.aug : nullptr;
    c.m.aug_len = a.aug ? a.aug_len : 0;
    H2cTemplate tmpl;
    const int hg = a.scheme == MSM_SIG_MIN_PK ? 2 : 1;  // the group of the hashes
    h2c_make_template(tmpl, a.DST, a.DST_len, (unsigned)(64 * c.count * hg));
    c.tmpl = &tmpl;
    c.o = a.offsets, c.pk = a.pk_offsets, c.k = k, c.src_dev = a.src_dev;
    static_assert(MSM_SIG_MIN_PK == 1 && MSM_SIG_MIN_SIG == 2, "SigVerify<G>: G is the group of the public keys");
    by_group(a.scheme, [&](auto g) {
      typedef SigVerify<decltype(g)::value> E;
      bulk_run<E>(a.dev, a.scheme, a.src_dev, false, a.user, [&](E &e, hipStream_t cs) { e.run(cs, c, st.p); });
    });
    if (a.nfail) *a.nfail = st.count_not(k, 0);
    return MSM_OK;
  }, on_throw);
}

int points_in_group_checked(int group, int dev, uint8_t *in_group, const void *points, size_t n, bool src_dev,
                            hipStream_t user) {
  if (group != 1 && group != 2) return fail(MSM_E_ARG, "group must be 1 or 2");
  if (n == 0) return MSM_OK;  // nothing touched
  if (!in_group || !points) return fail(MSM_E_ARG, "null in_group / points");
  if (n > ((size_t)1 << 40)) return fail(MSM_E_ARG, "npoints out of range");
  if (src_dev && ((uintptr_t)points & 7) != 0) return fail(MSM_E_ARG, "device points not 8-byte aligned");
  if (!device_ok(dev)) return no_device();
  const auto on_throw = [&] { memset(in_group, 0, n); };
  return guarded(MSM_E_HIP, [&] {
    by_group(group, [&](auto g) {
      constexpr int G = decltype(g)::value;
      bulk_run<GroupScreen<G>>(dev, G, src_dev, false, user, [&](GroupScreen<G> &e, hipStream_t cs) {
        e.run(cs, points, in_group, n, src_dev);
      });
    });
    return MSM_OK;
  }, on_throw);
}

size_t blst_window(size_t n) {  // ref multi_scalar.c:268-275
  size_t w = 0;
  while (n >>= 1) ++w;
  return w > 12 ? w - 3 : (w > 4 ? w - 2 : (w ? 2 : 1));
}

// What the four context kinds share: the engine E<group> of one group on `device`.
template <template <int> class E>
struct GroupCtx {
  int group = 1;
  int device = 0;      // (CHES: the first shard's device)
  bool ready = false;  // a table was built / set / loaded (mult before that: MSM_E_STATE)
  std::unique_ptr<E<1>> g1;
  std::unique_ptr<E<2>> g2;
  // f(engine of the context's group)
  template <class F>
  decltype(auto) with(F f) const {
    if (group == 1) return f(*g1);
    return f(*g2);
  }
};
}  // namespace

template <class F>
void fixed_points(hfp::Aff<F> *out, size_t n, hfp::Jac<F> g) {
  std::vector<hfp::Jac<F>> j(n);
  for (size_t i = 0; i < n; ++i) {
    g = hfp::dbl(g);
    j[i] = g;
  }
  hfp::to_affine_batch(out, j.data(), n);
}

// the C tags of include/msm_mi355x.h
struct msm_ches_ctx : GroupCtx<ChesMulti> {};  // one shard per device (multi.hpp); one shard = one device

struct msm_bgmw_ctx : GroupCtx<Bgmw> {
  DevBuf scalars;
};

struct msm_wbits_ctx : GroupCtx<Wbits> {
  DevBuf scalars;
};

struct msm_ctx : GroupCtx<Pippenger> {  // (`ready` unused: a context without points multiplies nothing)
  DevBuf scalars;
  DevBuf decoded;  // msm_ctx_set_points_encoded: the decoded affine points
};

struct msm_kzg_ctx {
  Kzg k;
  msm_kzg_ctx(int device, int log_n, int flags, int window) : k(device, log_n, flags, window) {}
};

namespace {
// ---------------- table file cache ----------------
// file = 64-byte header + rows in blst affine layout (canonical Montgomery,
// byte-identical to the reference's PRECOMPUTATION_POINTS_LIST_3nh / _BGMW95)
struct TableFileHeader {
  char magic[8];  // "MSMTBL01"
  int32_t group, method, q_exp, h;  // method: 1 CHES (3 rows per digit), 2 BGMW95 (1 row)
  uint64_t npoints, rows;
  uint8_t pad[24];
};
static_assert(sizeof(TableFileHeader) == 64, "header");
static const size_t kTableChunk = (size_t)1 << 20;  // rows per I/O chunk

template <class E>
static int save_table_file(E &eng, int group, int method, int q_exp, int h, const char *path) {
  FILE *f = fopen(path, "wb");
  if (!f) return fail(MSM_E_ARG, std::string("cannot open ") + path);
  TableFileHeader hd;
  memset(&hd, 0, sizeof hd);
  memcpy(hd.magic, "MSMTBL01", 8);
  hd.group = group, hd.method = method, hd.q_exp = q_exp, hd.h = h;
  hd.npoints = eng.npoints(), hd.rows = eng.table_rows();
  bool ok = fwrite(&hd, sizeof hd, 1, f) == 1;
  std::vector<uint8_t> buf(std::min<size_t>(kTableChunk, std::max<size_t>(hd.rows, 1)) * 96 * group);
  for (size_t r0 = 0; ok && r0 < hd.rows; r0 += kTableChunk) {
    size_t cnt = std::min(kTableChunk, (size_t)hd.rows - r0);
    eng.get_table(buf.data(), r0, cnt, (hipStream_t)0);
    ok = fwrite(buf.data(), 96 * group, cnt, f) == cnt;
  }
  ok = (fclose(f) == 0) && ok;
  return ok ? MSM_OK : fail(MSM_E_ARG, std::string("write failed: ") + path);
}

template <class E>
static int load_table_file(E &eng, int group, int method, int q_exp, int h, const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) return fail(MSM_E_ARG, std::string("cannot open ") + path);
  TableFileHeader hd;
  if (fread(&hd, sizeof hd, 1, f) != 1 || memcmp(hd.magic, "MSMTBL01", 8) != 0) {
    fclose(f);
    return fail(MSM_E_ARG, "not a table file");
  }
  if (hd.group != group || hd.method != method || hd.q_exp != q_exp || hd.h != h) {
    fclose(f);
    return fail(MSM_E_ARG, "table file was written for other parameters");
  }
  // validate everything the header claims before the engine is touched: the
  // row count must be the method's (3 h per point for CHES, h for BGMW95) and
  // the file must hold exactly header + rows * affine bytes
  const uint64_t per_point = (uint64_t)(method == 1 ? 3 : 1) * (uint64_t)h;
  const uint64_t row_bytes = 96ull * (uint64_t)group;
  if (hd.npoints >= (1ull << 31) || hd.rows != per_point * hd.npoints) {
    fclose(f);
    return fail(MSM_E_ARG, "table file row count does not match its point count");
  }
  if (fseek(f, 0, SEEK_END) != 0 || (uint64_t)ftell(f) != sizeof hd + hd.rows * row_bytes ||
      fseek(f, (long)sizeof hd, SEEK_SET) != 0) {
    fclose(f);
    return fail(MSM_E_ARG, std::string("table file size does not match its header: ") + path);
  }
  bool ok = true;
  try {
    eng.reserve_table((size_t)hd.npoints);
    std::vector<uint8_t> buf(std::min<size_t>(kTableChunk, std::max<size_t>(hd.rows, 1)) * row_bytes);
    for (size_t r0 = 0; ok && r0 < hd.rows; r0 += kTableChunk) {
      size_t cnt = std::min(kTableChunk, (size_t)hd.rows - r0);
      ok = fread(buf.data(), row_bytes, cnt, f) == cnt;
      if (ok) eng.put_table(buf.data(), r0, cnt, false, (hipStream_t)0);
    }
  } catch (...) {
    fclose(f);
    eng.reserve_table(0);  // no half-loaded table: the context has no points until a good load/build
    throw;
  }
  fclose(f);
  if (!ok) {
    eng.reserve_table(0);
    return fail(MSM_E_ARG, std::string("short read: ") + path);
  }
  return MSM_OK;
}

// ---------------- what the context entry points share ----------------
// The tail of every *_create: a context C of `group` on `device` around the
// engine make(integral_constant<G>) builds.  *ctx is written on success only;
// `code` is what a throwing constructor gives.
template <class C, class Make>
int create_ctx(C **ctx, int group, int device, int code, Make make) {
  return guarded(code, [&] {
    auto c = std::make_unique<C>();
    c->group = group;
    c->device = device;
    if (group == 1) c->g1 = make(std::integral_constant<int, 1>{});
    else c->g2 = make(std::integral_constant<int, 2>{});
    *ctx = c.release();
    return MSM_OK;
  });
}

// build_table / set_table / precompute: set(engine) with the context not ready
// while it runs, and ready after it only if it did not throw
template <class C, class Set>
int set_table_ctx(C *ctx, Set set) {
  return guarded(MSM_E_HIP, [&] {
    ctx->ready = false;
    ctx->with(set);
    ctx->ready = true;
    return MSM_OK;
  });
}

template <class C>
int get_table_ctx(C *ctx, void *out, size_t first, size_t count, int code) {
  if (!ctx || (!out && count)) return fail(MSM_E_ARG, "bad args");
  return guarded(code, [&] {
    ctx->with([&](auto &e) { e.get_table(out, first, count, (hipStream_t)0); });
    return MSM_OK;
  });
}

// save_table / load_table: `method` and qh(engine) = {q_exp, h} go into / are
// checked against the file's header
template <class C, class QH>
int save_table_ctx(C *ctx, const char *path, int method, QH qh) {
  if (!ctx || !path) return fail(MSM_E_ARG, "bad args");
  return guarded(MSM_E_HIP, [&] {
    DeviceGuard g(ctx->device);
    return ctx->with([&](auto &e) {
      const std::pair<int, int> p = qh(e);
      return save_table_file(e, ctx->group, method, p.first, p.second, path);
    });
  });
}
template <class C, class QH>
int load_table_ctx(C *ctx, const char *path, int method, QH qh) {
  if (!ctx || !path) return fail(MSM_E_ARG, "bad args");
  return guarded(MSM_E_HIP, [&] {
    DeviceGuard g(ctx->device);
    ctx->ready = false;
    const int rc = ctx->with([&](auto &e) {
      const std::pair<int, int> p = qh(e);
      return load_table_file(e, ctx->group, method, p.first, p.second, path);
    });
    ctx->ready = rc == MSM_OK;
    return rc;
  });
}

// `count` results of the engine's group: run(out) fills blst Jacobians, which
// are then copied to the caller's ret
template <template <int> class E, int G, class Run>
void mult_out(E<G> &, void *ret, size_t count, Run run) {
  typedef hfp::Jac<typename HostField<G>::F> J;
  J one;
  std::vector<J> many(count > 1 ? count : 0);  // (one result: no allocation)
  J *out = count > 1 ? many.data() : &one;
  run(out);
  memcpy(ret, out, count * sizeof(J));
}

// the scalars of a single-set mult on the device: host scalars are copied to
// the context's buffer on `s`, device scalars pass through
const uint8_t *stage_scalars(DevBuf &buf, const byte *scalars, size_t bytes, bool on_device, hipStream_t s) {
  if (on_device || !bytes) return scalars;
  buf.ensure(bytes + 16);
  MSM_HIP_CHECK(hipMemcpyAsync(buf.p, scalars, bytes, hipMemcpyHostToDevice, s));
  return buf.as<uint8_t>();
}

void phase_times_out(const PhaseTimes &t, float out[6]) {
  const float v[6] = {t.digits, t.sort, t.accumulate, t.reduce, t.finalize, t.total};
  memcpy(out, v, sizeof v);
}

}  // namespace

extern "C" {

size_t blst_p1s_mult_pippenger_scratch_sizeof(size_t npoints) { return sizeof(blst_p1xyzz) << (blst_window(npoints) - 1); }
size_t blst_p2s_mult_pippenger_scratch_sizeof(size_t npoints) { return sizeof(blst_p2xyzz) << (blst_window(npoints) - 1); }

#define MSM_PIPPENGER_ENTRIES(g)                                                                                  \
  void blst_p##g##s_mult_pippenger(blst_p##g *ret, const blst_p##g##_affine *const points[], size_t npoints,      \
                                   const byte *const scalars[], size_t nbits, limb_t *scratch) {                  \
    (void)scratch;                                                                                                \
    blst_guarded("blst_p" #g "s_mult_pippenger", ret, sizeof(*ret),                                               \
                 [&] { mult_pippenger<g>(ret, (const void *const *)points, npoints, scalars, nbits); });          \
  }                                                                                                               \
  void blst_p##g##s_tile_pippenger(blst_p##g *ret, const blst_p##g##_affine *const points[], size_t npoints,      \
                                   const byte *const scalars[], size_t nbits, limb_t *scratch, size_t bit0,       \
                                   size_t window) {                                                               \
    (void)scratch;                                                                                                \
    blst_guarded("blst_p" #g "s_tile_pippenger", ret, sizeof(*ret), [&] {                                         \
      tile_pippenger<g>(ret, (const void *const *)points, npoints, scalars, nbits, bit0, window);                 \
    });                                                                                                           \
  }
MSM_PIPPENGER_ENTRIES(1)
MSM_PIPPENGER_ENTRIES(2)
#undef MSM_PIPPENGER_ENTRIES

// ---- blst-level CHES / BGMW95 entry points ----
size_t blst_p1s_mult_pippenger_scratch_sizeof_CHES(size_t window) { return sizeof(blst_p1xyzz) * (window / 2); }
size_t blst_p2s_mult_pippenger_scratch_sizeof_CHES(size_t window) { return sizeof(blst_p2xyzz) * (window / 2); }

#define MSM_XYZZ_HELPERS(g, F)                                                                                   \
  void blst_p##g##xyzz_dadd_affine(blst_p##g##xyzz *out, const blst_p##g##xyzz *in, const blst_p##g##_affine *p, \
                                   unsigned char booth_sign) {                                                   \
    *reinterpret_cast<hfp::Xyzz<F> *>(out) = hfp::xyzz_madd(*reinterpret_cast<const hfp::Xyzz<F> *>(in),         \
                                                            *reinterpret_cast<const hfp::Aff<F> *>(p),           \
                                                            booth_sign != 0);                                    \
  }                                                                                                              \
  void blst_p##g##xyzz_dadd(blst_p##g##xyzz *p3, const blst_p##g##xyzz *p1, const blst_p##g##xyzz *p2) {         \
    *reinterpret_cast<hfp::Xyzz<F> *>(p3) = hfp::xyzz_add(*reinterpret_cast<const hfp::Xyzz<F> *>(p1),           \
                                                          *reinterpret_cast<const hfp::Xyzz<F> *>(p2));          \
  }                                                                                                              \
  void blst_p##g##xyzz_to_Jacobian(blst_p##g *out, const blst_p##g##xyzz *in) {                                  \
    *reinterpret_cast<hfp::Jac<F> *>(out) = hfp::xyzz_to_jac(*reinterpret_cast<const hfp::Xyzz<F> *>(in));       \
  }                                                                                                              \
  void blst_p##g##_to_xyzz(blst_p##g##xyzz *out, blst_p##g *in) {                                                \
    *reinterpret_cast<hfp::Xyzz<F> *>(out) = hfp::jac_to_xyzz(*reinterpret_cast<const hfp::Jac<F> *>(in));       \
  }                                                                                                              \
  void blst_p##g##_prefetch_CHES(const blst_p##g##xyzz buckets[], size_t booth_idx) {                            \
    (void)buckets;                                                                                               \
    (void)booth_idx;                                                                                             \
  }                                                                                                              \
  void blst_p##g##_bucket_CHES(blst_p##g##xyzz buckets[], int booth_idx, const blst_p##g##_affine *p,            \
                               unsigned char booth_sign) {                                                       \
    blst_p##g##xyzz_dadd_affine(&buckets[booth_idx], &buckets[booth_idx], p, booth_sign);                        \
  }
MSM_XYZZ_HELPERS(1, hfp::Fp)
MSM_XYZZ_HELPERS(2, hfp::Fp2)
#undef MSM_XYZZ_HELPERS

#define MSM_CHES_ENTRIES(g)                                                                                        \
  void blst_p##g##_integrate_buckets_accumulation_d_CHES(blst_p##g *out, blst_p##g##xyzz buckets[],              \
                                                         int bucket_set_ascend[], size_t bucket_set_size,         \
                                                         int d_max) {                                             \
    (void)d_max;                                                                                                  \
    blst_guarded("blst_p" #g "_integrate_buckets_accumulation_d_CHES", out, sizeof(*out), [&] {                   \
      std::vector<uint32_t> w(bucket_set_size);                                                                   \
      for (size_t k = 0; k < bucket_set_size; ++k) w[k] = (uint32_t)std::max(bucket_set_ascend[k], 0);           \
      weighted_bucket_sum<g>(out, buckets, bucket_set_size, w.data());                                            \
    });                                                                                                           \
  }                                                                                                               \
  void blst_p##g##_construct_nh_scalars_nh_points(int nh_scalars[], unsigned char booth_signs[],                  \
                                                  blst_p##g##_affine *nh_points_ptr[], const size_t npoints,     \
                                                  blst_p##g##_affine table[], const digit_decomposition H[]) {   \
    for (size_t i = 0; i < npoints; ++i) {                                                                        \
      const digit_decomposition d = H[nh_scalars[i]];                                                             \
      nh_scalars[i] = d.b;                                                                                        \
      booth_signs[i] = (unsigned char)d.alpha;                                                                    \
      if (d.alpha && i + 1 < npoints) ++nh_scalars[i + 1];                                                        \
      nh_points_ptr[i] = table + 3 * i + d.m - 1;                                                                 \
    }                                                                                                             \
  }                                                                                                               \
  void blst_p##g##_tile_pippenger_d_CHES(blst_p##g *ret, const blst_p##g##_affine *const points[], size_t npoints, \
                                         const int scalars[], const unsigned char booth_signs[],                  \
                                         blst_p##g##xyzz buckets[], int bucket_set_ascend[],                      \
                                         int bucket_value_to_its_index[], size_t bucket_set_size, int d_max) {    \
    (void)d_max;                                                                                                  \
    blst_guarded("blst_p" #g "_tile_pippenger_d_CHES", ret, sizeof(*ret), [&] {                                   \
      tile_d_ches<g>(ret, (const void *const *)points, npoints, scalars, booth_signs, buckets, bucket_set_ascend, \
                     bucket_value_to_its_index, bucket_set_size);                                                 \
    });                                                                                                           \
  }                                                                                                               \
  void blst_p##g##_tile_pippenger_d_CHES_noindexhash(                                                             \
      blst_p##g *ret, const blst_p##g##_affine *const points[], size_t npoints, const int scalars[],               \
      const unsigned char booth_signs[], blst_p##g##xyzz buckets[], int bucket_set_ascend[],                      \
      size_t bucket_set_size, int d_max) {                                                                        \
    (void)d_max;                                                                                                  \
    blst_guarded("blst_p" #g "_tile_pippenger_d_CHES_noindexhash", ret, sizeof(*ret), [&] {                       \
      tile_d_ches_noindex<g>(ret, (const void *const *)points, npoints, scalars, booth_signs, buckets,            \
                             bucket_set_ascend, bucket_set_size);                                                 \
    });                                                                                                           \
  }                                                                                                               \
  void blst_p##g##_tile_pippenger_CHES_prefetch_2step_ahead_input_std_scalar(                                     \
      blst_p##g *ret, const blst_p##g##_affine table[], size_t npoints, int scalars[],                            \
      digit_decomposition H[], blst_p##g##xyzz buckets[], int bucket_set_ascend[],                                \
      int bucket_value_to_its_index[], size_t bucket_set_size, int d_max) {                                       \
    (void)d_max;                                                                                                  \
    blst_guarded("blst_p" #g "_tile_pippenger_CHES_prefetch_2step_ahead_input_std_scalar", ret, sizeof(*ret), [&] { \
      tile_ches_std<g>(ret, table, npoints, scalars, H, buckets, bucket_set_ascend, bucket_value_to_its_index,    \
                       bucket_set_size);                                                                          \
    });                                                                                                           \
  }                                                                                                               \
  void blst_p##g##_tile_pippenger_BGMW95(blst_p##g *ret, const blst_p##g##_affine *const points[], size_t npoints, \
                                         const int scalars[], const unsigned char booth_signs[],                  \
                                         blst_p##g##xyzz buckets[], size_t q_exponent) {                          \
    blst_guarded("blst_p" #g "_tile_pippenger_BGMW95", ret, sizeof(*ret), [&] {                                   \
      tile_bgmw95<g>(ret, (const void *const *)points, npoints, scalars, booth_signs, buckets, q_exponent);       \
    });                                                                                                           \
  }
MSM_CHES_ENTRIES(1)
MSM_CHES_ENTRIES(2)
#undef MSM_CHES_ENTRIES

// ---- sum of affine points (replaces ref src/bulk_addition.c:145-164) ----
// point pointer rule of bulk_addition.c:155: a NULL entry continues right after
// the previous point
#define MSM_POINTS_ADD(g)                                                                                         \
  void blst_p##g##s_add(blst_p##g *ret, const blst_p##g##_affine *const points[], size_t npoints) {             \
    blst_guarded("blst_p" #g "s_add", ret, sizeof(*ret),                                                          \
                 [&] { points_add<g>(ret, (const void *const *)points, npoints); });                              \
  }
MSM_POINTS_ADD(1)
MSM_POINTS_ADD(2)
#undef MSM_POINTS_ADD

// ---- fixed-window MSM with a precomputed table (replaces ref multi_scalar.c:63-261) ----
#define MSM_WBITS_ENTRIES(g, scratch_pts)                                                                         \
  size_t blst_p##g##s_mult_wbits_precompute_sizeof(size_t wbits, size_t npoints) {                              \
    return (sizeof(blst_p##g##_affine) * npoints) << (wbits - 1);                                                 \
  }                                                                                                               \
  void blst_p##g##s_mult_wbits_precompute(blst_p##g##_affine table[], size_t wbits,                              \
                                          const blst_p##g##_affine *const points[], size_t npoints) {            \
    /* no half-written table: all of it is zeroed (no points: nothing is written and nothing throws) */          \
    blst_guarded("blst_p" #g "s_mult_wbits_precompute", table,                                                    \
                 npoints ? blst_p##g##s_mult_wbits_precompute_sizeof(wbits, npoints) : 0,                         \
                 [&] { wbits_precompute<g>(table, wbits, (const void *const *)points, npoints); });               \
  }                                                                                                               \
  size_t blst_p##g##s_mult_wbits_scratch_sizeof(size_t npoints) {                                                \
    return sizeof(blst_p##g) * (npoints < scratch_pts ? npoints : scratch_pts);                                   \
  }                                                                                                               \
  void blst_p##g##s_mult_wbits(blst_p##g *ret, const blst_p##g##_affine table[], size_t wbits, size_t npoints,   \
                               const byte *const scalars[], size_t nbits, limb_t *scratch) {                      \
    (void)scratch;                                                                                                \
    blst_guarded("blst_p" #g "s_mult_wbits", ret, sizeof(*ret),                                                   \
                 [&] { wbits_mult<g>(ret, table, wbits, npoints, scalars, nbits); });                             \
  }
MSM_WBITS_ENTRIES(1, 8192)  /* SCRATCH_SZ of ref multi_scalar.c:78 */
MSM_WBITS_ENTRIES(2, 4096)
#undef MSM_WBITS_ENTRIES

// ---- bulk Jacobian -> affine (replaces ref multi_scalar.c:17-62) ----
// pointer rule of multi_scalar.c:30 (walk_runs, ptr_walk.hpp); current device
#define MSM_PS_TO_AFFINE(g)                                                                                       \
  int msm_p##g##s_to_affine(blst_p##g##_affine dst[], const blst_p##g *const points[], size_t npoints) {        \
    if (npoints == 0) return MSM_OK;                                                                              \
    if (!dst || !points || !points[0]) return fail(MSM_E_ARG, "null dst / points");                               \
    return points_to_affine_checked<g>(kCurrentDevice, dst, nullptr, (const void *const *)points, npoints, false, \
                                       false, nullptr);                                                           \
  }
MSM_PS_TO_AFFINE(1)
MSM_PS_TO_AFFINE(2)
#undef MSM_PS_TO_AFFINE

int msm_points_to_affine(int group, int device, void *dst, const void *src, size_t npoints, int src_on_device,
                         int dst_on_device, void *hip_stream) {
  if (group != 1 && group != 2) return fail(MSM_E_ARG, "group must be 1 or 2");
  if (npoints == 0) return MSM_OK;
  if (!dst || !src) return fail(MSM_E_ARG, "null dst / src");
  if (npoints > ((size_t)1 << 40)) return fail(MSM_E_ARG, "npoints out of range");
  if (device == kCurrentDevice) return no_device();
  return by_group(group, [&](auto g) {
    return points_to_affine_checked<decltype(g)::value>(device, dst, src, nullptr, npoints, src_on_device != 0,
                                                        dst_on_device != 0, (hipStream_t)hip_stream);
  });
}

int msm_to_affine_levels(size_t npoints) { return (int)ta_levels(std::min(npoints, ta_chunk())).size(); }

// ---- bulk Fr arithmetic and NTTs (csrc/fr_ntt.hip) ----
int msm_fr_ntt(int device, void *dst, const void *src, size_t log_n, size_t batch, const byte *shift, int flags,
               int src_on_device, int dst_on_device, void *hip_stream) {
  const bool src_dev = src_on_device != 0, dst_dev = dst_on_device != 0;
  if (log_n > (size_t)NTT_MAX_LOG) return fail(MSM_E_ARG, "log_n above 26");
  if (flags & ~(MSM_NTT_INVERSE | MSM_FR_SRC_SCALAR | MSM_FR_DST_SCALAR)) return fail(MSM_E_ARG, "unknown flag bits");
  if (batch == 0) return MSM_OK;  // nothing touched
  if (!dst || !src) return fail(MSM_E_ARG, "null dst / src");
  if (batch > (((size_t)1 << 40) >> log_n)) return fail(MSM_E_ARG, "batch out of range");
  const size_t bytes = (batch << log_n) * 32;
  if (shift) {
    uint64_t w[4];
    memcpy(w, shift, 32);  // (little-endian host, as the blst limbs everywhere here)
    if (!(w[0] | w[1] | w[2] | w[3]) || hfr::geq_r(w)) return fail(MSM_E_ARG, "shift must be in (0, r)");
  }
  if (src_dev == dst_dev && dst != src && ranges_overlap(src, bytes, dst, bytes))
    return fail(MSM_E_ARG, "source and destination overlap");
  if (src_dev && ((uintptr_t)src & 7) != 0) return fail(MSM_E_ARG, "device source not 8-byte aligned");
  if (dst_dev && ((uintptr_t)dst & 7) != 0) return fail(MSM_E_ARG, "device destination not 8-byte aligned");
  if (!device_ok(device)) return no_device();
  const auto on_throw = [&] { zero_host(dst, bytes, dst_dev); };
  return guarded(MSM_E_HIP, [&] {
    bulk_run<FrNtt>(device, 0, src_dev, dst_dev, (hipStream_t)hip_stream, [&](FrNtt &e, hipStream_t cs) {
      e.ntt(cs, src, dst, (int)log_n, batch, shift, flags, src_dev, dst_dev);
    });
    return MSM_OK;
  }, on_throw);
}

int msm_fr_op(int device, int op, void *dst, const void *a, const void *b, size_t n, int flags, int src_on_device,
              int dst_on_device, void *hip_stream) {
  const bool src_dev = src_on_device != 0, dst_dev = dst_on_device != 0;
  if (op < 0 || op >= FR_NOPS) return fail(MSM_E_ARG, "unknown op");
  if (flags & ~MSM_FR_B_ONE) return fail(MSM_E_ARG, "unknown flag bits");
  if (n == 0) return MSM_OK;
  const bool two = fr_op_binary(op), b_one = (flags & MSM_FR_B_ONE) != 0;
  if (!dst || !a || (two && !b)) return fail(MSM_E_ARG, "null dst / a / b");
  if (n > ((size_t)1 << 40)) return fail(MSM_E_ARG, "n out of range");
  const size_t bytes = n * 32, b_bytes = b_one ? 32 : bytes;
  if (src_dev == dst_dev && ((dst != a && ranges_overlap(a, bytes, dst, bytes)) ||
                             (two && !(dst == b && !b_one) && ranges_overlap(b, b_bytes, dst, bytes))))
    return fail(MSM_E_ARG, "source and destination overlap");
  if (src_dev && ((((uintptr_t)a) | (two ? (uintptr_t)b : 0)) & 7) != 0)
    return fail(MSM_E_ARG, "device source not 8-byte aligned");
  if (dst_dev && ((uintptr_t)dst & 7) != 0) return fail(MSM_E_ARG, "device destination not 8-byte aligned");
  if (!device_ok(device)) return no_device();
  const auto on_throw = [&] { zero_host(dst, bytes, dst_dev); };
  return guarded(MSM_E_HIP, [&] {
    bulk_run<FrNtt>(device, 0, src_dev, dst_dev, (hipStream_t)hip_stream, [&](FrNtt &e, hipStream_t cs) {
      e.op(cs, op, dst, a, two ? b : nullptr, n, b_one, src_dev, dst_dev);
    });
    return MSM_OK;
  }, on_throw);
}

// ---- evaluation-form polynomials: value at a point and quotient (csrc/fr_poly.hip) ----
int msm_fr_eval_quotient(int device, void *y, void *q, const void *polys, const void *z, size_t log_n, size_t count,
                         int flags, int src_on_device, int dst_on_device, void *hip_stream) {
  const bool src_dev = src_on_device != 0, dst_dev = dst_on_device != 0;
  if (log_n > (size_t)POLY_MAX_LOG) return fail(MSM_E_ARG, "log_n above 26");
  if (flags & ~(MSM_FR_DST_SCALAR | MSM_POLY_BITREV)) return fail(MSM_E_ARG, "unknown flag bits");
  if (count == 0) return MSM_OK;  // nothing touched
  if (!y || !polys || !z) return fail(MSM_E_ARG, "null y / polys / z");
  if (count > (((size_t)1 << 40) >> log_n)) return fail(MSM_E_ARG, "count out of range");
  const size_t bytes = (count << log_n) * 32, ybytes = count * 32;
  if (q && src_dev == dst_dev && q != polys && ranges_overlap(polys, bytes, q, bytes))
    return fail(MSM_E_ARG, "q overlaps polys without being equal to it");
  if (src_dev == dst_dev && (ranges_overlap(polys, bytes, y, ybytes) || ranges_overlap(z, ybytes, y, ybytes) ||
                             (q && (ranges_overlap(q, bytes, y, ybytes) || ranges_overlap(z, ybytes, q, bytes)))))
    return fail(MSM_E_ARG, "y or z overlaps another array");
  if (src_dev && ((((uintptr_t)polys) | ((uintptr_t)z)) & 7) != 0)
    return fail(MSM_E_ARG, "device source not 8-byte aligned");
  if (dst_dev && ((((uintptr_t)y) | ((uintptr_t)q)) & 7) != 0)
    return fail(MSM_E_ARG, "device destination not 8-byte aligned");
  if (!device_ok(device)) return no_device();
  const auto on_throw = [&] {
    zero_host(y, ybytes, dst_dev);
    zero_host(q, bytes, dst_dev);
  };
  return guarded(MSM_E_HIP, [&] {
    bulk_run<FrPoly>(device, 0, src_dev, dst_dev, (hipStream_t)hip_stream, [&](FrPoly &e, hipStream_t cs) {
      e.run(cs, polys, z, y, q, (int)log_n, count, flags, src_dev, dst_dev);
    });
    return MSM_OK;
  }, on_throw);
}

int msm_fr_root_of_unity(size_t log_n, blst_fr *out) {
  if (log_n > 32 || !out) return fail(MSM_E_ARG, "log_n above 32 / null out");
  const hfr::Fr w = hfr::root_of_unity((unsigned)log_n);
  memcpy(out, &w, sizeof w);
  return MSM_OK;
}

int msm_ntt_plan(size_t log_n, int *npasses, int log_radix[], int capacity) {
  if (log_n > (size_t)NTT_MAX_LOG || !npasses) return fail(MSM_E_ARG, "log_n above 26 / null npasses");
  const std::vector<int> plan = ntt_plan((int)log_n, ntt_tile());
  *npasses = (int)plan.size();
  for (int i = 0; log_radix && i < capacity && i < (int)plan.size(); ++i) log_radix[i] = plan[i];
  return MSM_OK;
}

int msm_fr_probe(int device, double out[2]) {
  if (!out) return fail(MSM_E_ARG, "null out");
  if (!device_ok(device)) return no_device();
  return guarded(MSM_E_HIP, [&] {
    fr_probe(device, out);
    return MSM_OK;
  });
}

int msm_points_decode(int group, int device, void *dst, uint8_t *status, size_t *nbad, const void *src, size_t npoints,
                      int encoding, int flags, int src_on_device, int dst_on_device, void *hip_stream) {
  return points_decode_checked(group, device, dst, status, nbad, src, npoints, encoding, flags, src_on_device != 0,
                               dst_on_device != 0, (hipStream_t)hip_stream);
}

int msm_points_mult(int group, int device, void *dst, const void *points, const byte *scalars, size_t npoints,
                    size_t nbits, size_t scalar_stride, int flags, int src_on_device, int dst_on_device,
                    void *hip_stream) {
  return points_mult_checked(group, device, dst, points, scalars, npoints, nbits, scalar_stride, flags,
                             src_on_device != 0, dst_on_device != 0, (hipStream_t)hip_stream);
}

int msm_points_ntt(int group, int device, void *dst_affine, const void *src_affine, size_t log_n, size_t batch,
                   int flags, int src_on_device, int dst_on_device, void *hip_stream) {
  return points_ntt_checked(group, device, dst_affine, src_affine, log_n, batch, flags, src_on_device != 0,
                            dst_on_device != 0, (hipStream_t)hip_stream);
}

int msm_points_ntt_model(size_t log_n, int flags, blst_fr *dst, const blst_fr *src) {
  if (log_n > 16) return fail(MSM_E_ARG, "log_n above 16");
  if (flags & ~(MSM_NTT_INVERSE | MSM_POLY_BITREV)) return fail(MSM_E_ARG, "unknown flag bits");
  if (!dst || !src) return fail(MSM_E_ARG, "null dst / src");
  static_assert(sizeof(blst_fr) == sizeof(hfr::Fr), "blst_fr");
  return guarded(MSM_E_ARG, [&] {
    pn_model((int)log_n, flags, 1, reinterpret_cast<hfr::Fr *>(dst), reinterpret_cast<const hfr::Fr *>(src), pn_chunk(),
             pn_slice());
    return MSM_OK;
  });
}

int msm_points_encode(int group, int device, void *dst, const void *src, size_t npoints, int src_form, int encoding,
                      int flags, int src_on_device, int dst_on_device, void *hip_stream) {
  return points_encode_checked(group, device, dst, src, npoints, src_form, encoding, flags, src_on_device != 0,
                               dst_on_device != 0, (hipStream_t)hip_stream);
}

int msm_points_msm_segments(int group, int device, void *dst_affine, const void *points_affine, const byte *scalars,
                            const size_t *offsets, size_t nsegments, size_t nbits, size_t scalar_stride, int flags,
                            int src_on_device, int dst_on_device, void *hip_stream) {
  return points_segments_checked(group, device, dst_affine, points_affine, scalars, offsets, nsegments, nbits,
                                 scalar_stride, flags, src_on_device != 0, dst_on_device != 0, (hipStream_t)hip_stream);
}

size_t msm_segments_piece(int group, size_t npoints) {
  if (group != 1 && group != 2) return 0;
  return seg_piece_len(std::min(npoints, seg_chunk(group)), group);
}

int msm_segments_plan(const size_t *offsets, size_t nsegments, size_t piece, size_t *npieces, size_t *start,
                      size_t *count, size_t *segment, size_t capacity) {
  if (!npieces || piece == 0 || (nsegments && !offsets)) return fail(MSM_E_ARG, "null npieces / offsets or piece == 0");
  if (!seg_offsets_ok(offsets, nsegments)) return fail(MSM_E_ARG, "offsets decrease");
  size_t w = 0;
  *npieces = nsegments ? seg_cut(offsets, nsegments, piece, offsets[0], offsets[nsegments], 0,
                                 [&](size_t s, size_t c, size_t j) {
                                   if (w < capacity) {
                                     if (start) start[w] = s;
                                     if (count) count[w] = c;
                                     if (segment) segment[w] = j;
                                   }
                                   ++w;
                                 })
                       : 0;
  return MSM_OK;
}

int msm_points_map(int group, int device, void *dst_affine, const void *u, size_t npoints, int count,
                   int src_on_device, int dst_on_device, void *hip_stream) {
  return hash_to_curve_checked(group, device, H2C_MAP, dst_affine, u, nullptr, nullptr, 0, nullptr, 0, npoints, nullptr,
                               0, count, src_on_device != 0, dst_on_device != 0, (hipStream_t)hip_stream);
}

int msm_hash_to_field(int group, int device, void *dst_elems, const void *msgs, const size_t *offsets, size_t msg_len,
                      const void *aug, size_t aug_len, size_t npoints, const byte *DST, size_t DST_len, int count,
                      int src_on_device, int dst_on_device, void *hip_stream) {
  return hash_to_curve_checked(group, device, H2C_FIELD, dst_elems, nullptr, msgs, offsets, msg_len, aug, aug_len,
                               npoints, DST, DST_len, count, src_on_device != 0, dst_on_device != 0,
                               (hipStream_t)hip_stream);
}

int msm_points_hash(int group, int device, void *dst_affine, const void *msgs, const size_t *offsets, size_t msg_len,
                    const void *aug, size_t aug_len, size_t npoints, const byte *DST, size_t DST_len, int flags,
                    int src_on_device, int dst_on_device, void *hip_stream) {
  if (flags & ~MSM_H2C_ENCODE) return fail(MSM_E_ARG, "unknown flag bits");
  return hash_to_curve_checked(group, device, H2C_HASH, dst_affine, nullptr, msgs, offsets, msg_len, aug, aug_len,
                               npoints, DST, DST_len, (flags & MSM_H2C_ENCODE) ? 1 : 2, src_on_device != 0,
                               dst_on_device != 0, (hipStream_t)hip_stream);
}

int msm_h2c_dst_prime(byte *out, size_t *out_len, const byte *DST, size_t DST_len) {
  if (!out || !out_len || (DST_len && !DST)) return fail(MSM_E_ARG, "null out / out_len / DST");
  *out_len = h2c_dst_prime(out, DST, DST_len);
  return MSM_OK;
}

int msm_pairing_segments(int device, void *dst_fp12, uint8_t *is_one, size_t *nfail, const void *p_affine,
                         const void *q_affine, const size_t *offsets, size_t nsegments, int flags, int src_on_device,
                         int dst_on_device, void *hip_stream) {
  return pairing_checked(device, dst_fp12, is_one, nfail, p_affine, q_affine, nullptr, offsets, nsegments, flags, false,
                         src_on_device != 0, dst_on_device != 0, (hipStream_t)hip_stream);
}

int msm_fp12_final_exp(int device, void *dst_fp12, uint8_t *is_one, size_t *nfail, const void *src_fp12, size_t n,
                       int src_on_device, int dst_on_device, void *hip_stream) {
  return pairing_checked(device, dst_fp12, is_one, nfail, nullptr, nullptr, src_fp12, nullptr, n, 0, true,
                         src_on_device != 0, dst_on_device != 0, (hipStream_t)hip_stream);
}

size_t msm_pairing_piece(size_t npairs) { return pair_piece_len(std::min(std::max(npairs, (size_t)1), pair_chunk())); }

int msm_sigs_verify(int scheme, int device, uint8_t *status, size_t *nfail, const void *pks, const size_t *pk_offsets,
                    const void *sigs, const void *msgs, const size_t *msg_offsets, size_t msg_len, const void *aug,
                    size_t aug_len, size_t nchecks, const byte *DST, size_t DST_len, int flags, int src_on_device,
                    void *hip_stream) {
  return sigs_checked(SigArgs{SIG_VERIFY, scheme, device, status, nfail, pks, sigs, msgs, aug, pk_offsets, msg_offsets,
                              nullptr, msg_len, aug_len, nchecks, nullptr, 0, 0, DST, DST_len, flags,
                              src_on_device != 0, (hipStream_t)hip_stream});
}

int msm_sigs_aggregate_verify(int scheme, int device, uint8_t *status, size_t *nfail, const void *pks, const void *sigs,
                              const void *msgs, const size_t *msg_offsets, size_t msg_len, const void *aug,
                              size_t aug_len, const size_t *offsets, size_t nchecks, const byte *DST, size_t DST_len,
                              int flags, int src_on_device, void *hip_stream) {
  return sigs_checked(SigArgs{SIG_AGGREGATE, scheme, device, status, nfail, pks, sigs, msgs, aug, nullptr, msg_offsets,
                              offsets, msg_len, aug_len, nchecks, nullptr, 0, 0, DST, DST_len, flags,
                              src_on_device != 0, (hipStream_t)hip_stream});
}

int msm_sigs_batch_verify(int scheme, int device, uint8_t *status, size_t *nfail, const void *pks, const void *sigs,
                          const byte *scalars, size_t nbits, size_t scalar_stride, const void *msgs,
                          const size_t *msg_offsets, size_t msg_len, const void *aug, size_t aug_len,
                          const size_t *offsets, size_t nchecks, const byte *DST, size_t DST_len, int flags,
                          int src_on_device, void *hip_stream) {
  return sigs_checked(SigArgs{SIG_BATCH, scheme, device, status, nfail, pks, sigs, msgs, aug, nullptr, msg_offsets,
                              offsets, msg_len, aug_len, nchecks, scalars, nbits, scalar_stride, DST, DST_len, flags,
                              src_on_device != 0, (hipStream_t)hip_stream});
}

int msm_points_in_group(int group, int device, uint8_t *in_group, const void *points_affine, size_t npoints,
                        int src_on_device, void *hip_stream) {
  return points_in_group_checked(group, device, in_group, points_affine, npoints, src_on_device != 0,
                                 (hipStream_t)hip_stream);
}

size_t msm_sigs_chunk(void) { return sig_chunk(); }

int msm_sigs_plan(int mode, const size_t *offsets, const size_t *pk_offsets, size_t nchecks, size_t c0, size_t chunk,
                  size_t *c1, size_t counts[4], uint32_t *ent_check, uint32_t *ent_src, size_t *pair_off,
                  size_t *key_off, size_t *sig_off, size_t capacity) {
  if (mode < SIG_VERIFY || mode > SIG_BATCH || !c1 || !counts || chunk == 0 || c0 >= nchecks)
    return fail(MSM_E_ARG, "bad mode / null c1 / counts / chunk 0 / c0 past the checks");
  if (mode != SIG_VERIFY && (!offsets || !seg_offsets_ok(offsets, nchecks))) return fail(MSM_E_ARG, "null or decreasing offsets");
  if (mode == SIG_VERIFY && pk_offsets && !seg_offsets_ok(pk_offsets, nchecks)) return fail(MSM_E_ARG, "pk_offsets decrease");
  SigChunkPlan pl;
  *c1 = sig_chunk_end(mode, offsets, pk_offsets, nchecks, c0, chunk);
  sig_plan_chunk(pl, mode, offsets, pk_offsets, c0, *c1);
  counts[0] = pl.nrows, counts[1] = pl.nkeys, counts[2] = pl.nsigs, counts[3] = pl.ent.size();
  for (size_t i = 0; i < pl.ent.size() && i < capacity; ++i) {
    if (ent_check) ent_check[i] = pl.ent[i].check;
    if (ent_src) ent_src[i] = pl.ent[i].src;
  }
  for (size_t i = 0; i < pl.pair_off.size() && i < capacity; ++i)
    if (pair_off) pair_off[i] = pl.pair_off[i];
  for (size_t i = 0; i < pl.key_off.size() && i < capacity; ++i)
    if (key_off) key_off[i] = pl.key_off[i];
  for (size_t i = 0; i < pl.sig_off.size() && i < capacity; ++i)
    if (sig_off) sig_off[i] = pl.sig_off[i];
  return MSM_OK;
}

int msm_sigs_reduce(int mode, const size_t *offsets, const size_t *pk_offsets, size_t c0, size_t c1,
                    const uint8_t *sig_codes, const uint8_t *key_codes, const uint8_t *late, const uint8_t *is_one,
                    uint8_t *status) {
  if (mode < SIG_VERIFY || mode > SIG_BATCH || c1 < c0 || !status || !is_one || (mode != SIG_VERIFY && !offsets))
    return fail(MSM_E_ARG, "bad mode / range / null status / is_one / offsets");
  SigChunkPlan pl;
  sig_plan_chunk(pl, mode, offsets, pk_offsets, c0, c1);
  std::vector<uint8_t> cc(c1 - c0);
  sig_reduce(pl, mode, offsets, pk_offsets, sig_codes, key_codes, cc.data());
  for (size_t j = 0; j < c1 - c0; ++j)
    status[j] = sig_status(cc[j], late && late[j], is_one[j] == 1, pl.pair_off[j + 1] - pl.pair_off[j] - 1);
  return MSM_OK;
}

const char *msm_last_error(void) { return g_err.c_str(); }

int msm_set_abort_on_error(int on) { return g_abort_on_error.exchange(on != 0 ? 1 : 0); }

int msm_error_pending(void) {
  const int p = g_pending;
  g_pending = 0;
  return p;
}

void msm_release_engine_cache(void) {
  PoolStats st;
  PoolRegistry::get().visit(st, true);
}

void msm_engine_cache_stats(size_t out[3]) {
  PoolStats st;
  PoolRegistry::get().visit(st, false);
  out[0] = st.live, out[1] = st.idle, out[2] = st.idle_bytes;
}

size_t msm_set_engine_cache_limit(size_t bytes) {
  const size_t prev = PoolRegistry::get().idle_budget.exchange(bytes);
  PoolStats st;  // a lowered limit trims the engines already idle
  PoolRegistry::get().visit(st, false);
  return prev;
}

int msm_register_host_table(int group, const void *rows, size_t nrows) {
  if ((group != 1 && group != 2) || !rows || !nrows) return fail(MSM_E_ARG, "bad group / rows");
  return guarded(MSM_E_HIP, [&] {
    by_group(group, [&](auto g) { register_host_table<decltype(g)::value>(rows, nrows); });
    return MSM_OK;
  });
}

int msm_unregister_host_table(const void *rows) {
  if (!rows) return fail(MSM_E_ARG, "null rows");
  return TableRegistry::get().remove(rows) ? MSM_OK : fail(MSM_E_ARG, "table not registered");
}

int msm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int msm_valu_probe(int device, double out[4]) {
  if (!out) return fail(MSM_E_ARG, "null out");
  if (!device_ok(device)) return no_device();
  return guarded(MSM_E_HIP, [&] {
    valu_probe(device, out);
    return MSM_OK;
  });
}

int msm_fp_form_ops(int device, int form, const uint32_t *in, size_t lanes, uint32_t *out) {
  if (!in || !out || !lanes || (form != 0 && form != 1)) return fail(MSM_E_ARG, "bad in / out / lanes / form");
  if (!device_ok(device)) return no_device();
  return guarded(MSM_E_HIP, [&] {
    form_ops(device, form, in, lanes, out);
    return MSM_OK;
  });
}

int msm_ctx_create(msm_ctx **ctx, int group, int device, int window_bits) {
  if (!ctx || (group != 1 && group != 2)) return fail(MSM_E_ARG, "bad ctx/group");
  if (!device_ok(device)) return no_device();
  const int wb = window_bits > 0 ? window_bits : 16;
  return create_ctx(ctx, group, device, MSM_E_HIP,
                    [&](auto g) { return std::make_unique<Pippenger<decltype(g)::value>>(device, wb); });
}

int msm_ctx_set_points(msm_ctx *ctx, const void *points, size_t n, int on_device, void *stream) {
  if (!ctx || (!points && n)) return fail(MSM_E_ARG, "bad args");
  return guarded(MSM_E_HIP, [&] {
    ctx->with([&](auto &e) { e.set_points(points, n, on_device != 0, (hipStream_t)stream); });
    return MSM_OK;
  });
}

int msm_ctx_set_points_encoded(msm_ctx *ctx, const void *src, size_t n, int encoding, int flags, int src_on_device,
                               size_t *first_bad, void *stream) {
  if (!ctx || (!src && n)) return fail(MSM_E_ARG, "bad args");
  if (n == 0) return msm_ctx_set_points(ctx, nullptr, 0, 1, stream);
  std::vector<uint8_t> st;
  const int allocated = guarded(MSM_E_HIP, [&] {
    DeviceGuard g(ctx->device);
    st.resize(n);
    ctx->decoded.ensure(n * 96 * (size_t)ctx->group);
    return MSM_OK;
  });
  if (allocated != MSM_OK) return allocated;
  const int rc = points_decode_checked(ctx->group, ctx->device, ctx->decoded.p, st.data(), nullptr, src, n, encoding,
                                       flags, src_on_device != 0, true, (hipStream_t)stream);
  if (rc != MSM_OK) return rc;
  for (size_t i = 0; i < n; ++i)
    if (st[i]) {  // the context keeps its previous points
      if (first_bad) *first_bad = i;
      return fail(MSM_E_ARG, "encoded point " + std::to_string(i) + " rejected: status " + std::to_string((int)st[i]));
    }
  return msm_ctx_set_points(ctx, ctx->decoded.p, n, 1, stream);
}

int msm_ctx_mult(msm_ctx *ctx, void *ret, const byte *scalars, size_t stride, size_t nbits, int on_device,
                 void *stream) {
  if (!ctx || !ret || nbits == 0 || nbits > 256 || stride < (nbits + 7) / 8) return fail(MSM_E_ARG, "bad args");
  return guarded(MSM_E_HIP, [&] {
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    ctx->with([&](auto &e) {
      const uint8_t *d = stage_scalars(ctx->scalars, scalars, e.npoints() * stride, on_device != 0, s);
      mult_out(e, ret, 1, [&](auto *out) { e.run(s, d, stride, (int)nbits, out); });
    });
    return MSM_OK;
  });
}

int msm_ctx_mult_batch(msm_ctx *ctx, void *rets, const byte *scalars, size_t stride, size_t set_stride, size_t nbits,
                       size_t count, int on_device, void *stream) {
  if (!ctx || (!rets && count) || nbits == 0 || nbits > 256 || stride < (nbits + 7) / 8)
    return fail(MSM_E_ARG, "bad args");
  return guarded(MSM_E_HIP, [&] {
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t n = ctx->with([](auto &e) { return e.npoints(); });
    const uint8_t *d = scalars;
    if (!on_device && n && count) {  // the sets, packed, in one upload
      ctx->scalars.ensure(count * n * stride + 16);
      for (size_t k = 0; k < count; ++k)
        MSM_HIP_CHECK(hipMemcpyAsync(ctx->scalars.as<uint8_t>() + k * n * stride, scalars + k * set_stride,
                                     n * stride, hipMemcpyHostToDevice, s));
      d = ctx->scalars.as<uint8_t>();
      set_stride = n * stride;
    }
    ctx->with([&](auto &e) {
      mult_out(e, rets, count, [&](auto *out) { e.run_batch(s, d, stride, set_stride, count, (int)nbits, out); });
    });
    return MSM_OK;
  });
}

int msm_ctx_set_profiling(msm_ctx *ctx, int on) {
  if (!ctx) return fail(MSM_E_ARG, "null ctx");
  ctx->with([&](auto &e) { e.set_profiling(on != 0); });
  return MSM_OK;
}

int msm_ctx_phase_times(const msm_ctx *ctx, float out[6]) {
  if (!ctx || !out) return fail(MSM_E_ARG, "null");
  phase_times_out(ctx->with([](auto &e) -> const PhaseTimes & { return e.times(); }), out);
  return MSM_OK;
}

void msm_ctx_destroy(msm_ctx *ctx) { delete ctx; }

// ---------------- KZG contexts (csrc/kzg.cpp) ----------------
int msm_kzg_ctx_create(msm_kzg_ctx **ctx, int device, size_t log_n, const void *srs_lagrange_g1, int srs_on_device,
                       const void *tau_g2, int flags, void *hip_stream) {
  if (!ctx || !srs_lagrange_g1 || !tau_g2) return fail(MSM_E_ARG, "null ctx / srs / tau_g2");
  if (log_n > (size_t)KZG_MAX_LOG) return fail(MSM_E_ARG, "log_n above 20");
  if (flags & ~MSM_POLY_BITREV) return fail(MSM_E_ARG, "unknown flag bits");
  if (srs_on_device && ((uintptr_t)srs_lagrange_g1 & 7) != 0) return fail(MSM_E_ARG, "device srs not 8-byte aligned");
  if (!device_ok(device)) return no_device();
  int rc = MSM_OK;
  const int thrown = guarded(MSM_E_HIP, [&] {
    auto c = std::make_unique<msm_kzg_ctx>(device, (int)log_n, flags, auto_window((size_t)1 << log_n));
    rc = c->k.set_srs(srs_lagrange_g1, srs_on_device != 0, tau_g2, (hipStream_t)hip_stream);
    if (rc == MSM_OK) *ctx = c.release();
    return MSM_OK;
  });
  return thrown != MSM_OK ? thrown : rc;
}

void msm_kzg_ctx_destroy(msm_kzg_ctx *ctx) { delete ctx; }

int msm_kzg_ctx_create_monomial(msm_kzg_ctx **ctx, int device, size_t log_n, const void *srs_monomial_g1,
                                int srs_on_device, const void *tau_g2, int flags, void *hip_stream) {
  if (!ctx || !srs_monomial_g1 || !tau_g2) return fail(MSM_E_ARG, "null ctx / srs / tau_g2");
  if (log_n > (size_t)KZG_MAX_LOG) return fail(MSM_E_ARG, "log_n above 20");
  if (flags & ~MSM_POLY_BITREV) return fail(MSM_E_ARG, "unknown flag bits");
  if (srs_on_device && ((uintptr_t)srs_monomial_g1 & 7) != 0) return fail(MSM_E_ARG, "device srs not 8-byte aligned");
  if (!device_ok(device)) return no_device();
  int rc = MSM_OK;
  const int thrown = guarded(MSM_E_HIP, [&] {
    // the Lagrange SRS: the inverse transform of the monomial one, device to device on the caller's stream
    DeviceGuard g(device);
    DevBuf lag;
    lag.ensure(((size_t)96) << log_n);
    rc = points_ntt_checked(1, device, lag.p, srs_monomial_g1, log_n, 1, MSM_NTT_INVERSE | (flags & MSM_POLY_BITREV),
                            srs_on_device != 0, true, (hipStream_t)hip_stream);
    if (rc != MSM_OK) return MSM_OK;
    auto c = std::make_unique<msm_kzg_ctx>(device, (int)log_n, flags, auto_window((size_t)1 << log_n));
    rc = c->k.set_srs(lag.p, true, tau_g2, (hipStream_t)hip_stream);
    MSM_HIP_CHECK(hipStreamSynchronize((hipStream_t)hip_stream));  // `lag` is freed here
    if (rc == MSM_OK) *ctx = c.release();
    return MSM_OK;
  });
  return thrown != MSM_OK ? thrown : rc;
}

int msm_kzg_commit(msm_kzg_ctx *ctx, void *dst_affine, const void *polys, size_t count, int src_on_device,
                   int dst_on_device, void *hip_stream) {
  if (!ctx) return fail(MSM_E_ARG, "null ctx");
  if (count == 0) return MSM_OK;  // nothing touched
  if (!dst_affine || !polys) return fail(MSM_E_ARG, "null dst / polys");
  if (count > (((size_t)1 << 40) >> ctx->k.log_n())) return fail(MSM_E_ARG, "count out of range");
  const bool src_dev = src_on_device != 0, dst_dev = dst_on_device != 0;
  if (src_dev && ((uintptr_t)polys & 7) != 0) return fail(MSM_E_ARG, "device source not 8-byte aligned");
  if (dst_dev && ((uintptr_t)dst_affine & 7) != 0) return fail(MSM_E_ARG, "device destination not 8-byte aligned");
  const auto on_throw = [&] { zero_host(dst_affine, count * 96, dst_dev); };
  int rc = MSM_OK;
  const int thrown = guarded(MSM_E_HIP, [&] {
    rc = ctx->k.commit(dst_affine, polys, count, src_dev, dst_dev, (hipStream_t)hip_stream);
    return MSM_OK;
  }, on_throw);
  if (thrown == MSM_OK && rc != MSM_OK) on_throw();
  return thrown != MSM_OK ? thrown : rc;
}

int msm_kzg_open(msm_kzg_ctx *ctx, void *proofs_affine, void *y, const void *polys, const void *z, size_t count,
                 int src_on_device, int dst_on_device, void *hip_stream) {
  if (!ctx) return fail(MSM_E_ARG, "null ctx");
  if (count == 0) return MSM_OK;  // nothing touched
  if (!proofs_affine || !y || !polys || !z) return fail(MSM_E_ARG, "null proofs / y / polys / z");
  if (count > (((size_t)1 << 40) >> ctx->k.log_n())) return fail(MSM_E_ARG, "count out of range");
  const bool src_dev = src_on_device != 0, dst_dev = dst_on_device != 0;
  if (src_dev && ((((uintptr_t)polys) | ((uintptr_t)z)) & 7) != 0)
    return fail(MSM_E_ARG, "device source not 8-byte aligned");
  if (dst_dev && ((((uintptr_t)proofs_affine) | ((uintptr_t)y)) & 7) != 0)
    return fail(MSM_E_ARG, "device destination not 8-byte aligned");
  const auto on_throw = [&] {
    zero_host(proofs_affine, count * 96, dst_dev);
    zero_host(y, count * 32, dst_dev);
  };
  int rc = MSM_OK;
  const int thrown = guarded(MSM_E_HIP, [&] {
    rc = ctx->k.open(proofs_affine, y, polys, z, count, src_dev, dst_dev, (hipStream_t)hip_stream);
    return MSM_OK;
  }, on_throw);
  if (thrown == MSM_OK && rc != MSM_OK) on_throw();
  return thrown != MSM_OK ? thrown : rc;
}

int msm_kzg_verify(msm_kzg_ctx *ctx, uint8_t *ok, size_t *nfail, const void *commitments, const void *z,
                   const void *y, const void *proofs, size_t count, const byte *weights, size_t nbits,
                   size_t weight_stride, const size_t *batch_offsets, size_t nbatches, int src_on_device,
                   void *hip_stream) {
  if (weights) {
    if (nbits > 256) return fail(MSM_E_ARG, "nbits must be at most 256");
    if (weight_stride < (nbits + 7) / 8) return fail(MSM_E_ARG, "weight_stride shorter than (nbits + 7) / 8");
    if (weight_stride > ((size_t)1 << 20)) return fail(MSM_E_ARG, "weight_stride out of range");
    if (batch_offsets) {
      if (nbatches > ((size_t)1 << 32)) return fail(MSM_E_ARG, "nbatches out of range");
      if (!seg_offsets_ok(batch_offsets, nbatches)) return fail(MSM_E_ARG, "batch offsets decrease");
      if (batch_offsets[nbatches] > count) return fail(MSM_E_ARG, "batch offsets past the tuples");
    }
  }
  if (!ctx) return fail(MSM_E_ARG, "null ctx");
  if (count == 0) return MSM_OK;  // nothing touched
  if (!ok && !nfail) return fail(MSM_E_ARG, "null ok and nfail");
  if (!commitments || !z || !y || !proofs) return fail(MSM_E_ARG, "null commitments / z / y / proofs");
  if (count > ((size_t)1 << 32)) return fail(MSM_E_ARG, "count out of range");
  const bool src_dev = src_on_device != 0;
  if (src_dev && ((((uintptr_t)commitments) | ((uintptr_t)z) | ((uintptr_t)y) | ((uintptr_t)proofs)) & 7) != 0)
    return fail(MSM_E_ARG, "device source not 8-byte aligned");
  const size_t nchk = weights ? (batch_offsets ? nbatches : 1) : count;
  if (nchk == 0) return MSM_OK;
  const auto on_throw = [&] {
    if (ok) memset(ok, 0, nchk);
    if (nfail) *nfail = nchk;
  };
  int rc = MSM_OK;
  const int thrown = guarded(MSM_E_HIP, [&] {
    rc = ctx->k.verify(ok, nfail, commitments, z, y, proofs, count, weights, nbits, weight_stride, batch_offsets,
                       nbatches, src_dev, (hipStream_t)hip_stream);
    return MSM_OK;
  }, on_throw);
  if (thrown == MSM_OK && rc != MSM_OK) on_throw();
  return thrown != MSM_OK ? thrown : rc;
}

// ---------------- CHES contexts ----------------
static void params_out(const ChesParams &p, int out[9]) {
  const int v[9] = {p.n_exp, p.beta, p.q_exp, p.h, p.a_h, p.d_max, p.b_size, p.q_exp_bgmw, p.h_bgmw};
  memcpy(out, v, sizeof v);
}

int msm_ches_params(int n_exp, int beta, int out[9]) {
  ChesParams p;
  if (!out || !ches_params_for(n_exp, beta, &p)) return fail(MSM_E_ARG, "no CHES configuration for n_exp/beta");
  params_out(p, out);
  return MSM_OK;
}

// The tail of the CHES creates: one shard per entry of devices[0 .. ndev); the
// context's device is the first.
static int ches_create(msm_ches_ctx **ctx, int group, const int *devices, int ndev, const int v[9]) {
  const ChesParams p{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8]};
  return create_ctx(ctx, group, devices[0], MSM_E_HIP, [&](auto g) {
    return std::make_unique<ChesMulti<decltype(g)::value>>(std::vector<int>(devices, devices + ndev), p);
  });
}

int msm_ches_ctx_create_params(msm_ches_ctx **ctx, int group, int device, const int v[9]) {
  if (!ctx || !v || (group != 1 && group != 2)) return fail(MSM_E_ARG, "bad ctx/group/params");
  if (!device_ok(device)) return no_device();
  return ches_create(ctx, group, &device, 1, v);
}

int msm_ches_ctx_create(msm_ches_ctx **ctx, int group, int device, int n_exp, int beta) {
  int v[9];
  int rc = msm_ches_params(n_exp, beta, v);
  if (rc) return rc;
  return msm_ches_ctx_create_params(ctx, group, device, v);
}

int msm_ches_ctx_create_multi(msm_ches_ctx **ctx, int group, const int *devices, int ndev, int n_exp, int beta) {
  if (!ctx || !devices || ndev < 1 || (group != 1 && group != 2)) return fail(MSM_E_ARG, "bad ctx/group/devices");
  int v[9];
  int rc = msm_ches_params(n_exp, beta, v);
  if (rc) return rc;
  for (int i = 0; i < ndev; ++i)
    if (!device_ok(devices[i])) return no_device();
  return ches_create(ctx, group, devices, ndev, v);
}

int msm_ches_ctx_shards(const msm_ches_ctx *ctx) {
  return ctx ? (int)ctx->with([](auto &e) { return e.nshards(); }) : 0;
}

int msm_ches_ctx_rccl_exchange(const msm_ches_ctx *ctx) {
  return ctx ? (int)ctx->with([](auto &e) { return e.rccl_exchange(); }) : 0;
}

// several engines take host memory only (each device gets its own slice); shards
// merged into one engine on one device (multi.hpp) take device memory like a
// single-device context
static bool multi_device_arg(const msm_ches_ctx *ctx, int on_device) {
  return on_device && ctx->with([](auto &e) { return e.engines(); }) > 1;
}

int msm_ches_ctx_build_table(msm_ches_ctx *ctx, const void *pts, size_t n, int on_device, void *stream) {
  if (!ctx || (!pts && n)) return fail(MSM_E_ARG, "bad args");
  if (multi_device_arg(ctx, on_device)) return fail(MSM_E_ARG, "a multi-device context takes host points");
  return set_table_ctx(ctx, [&](auto &e) { e.build_table(pts, n, on_device != 0, (hipStream_t)stream); });
}

int msm_ches_ctx_set_table(msm_ches_ctx *ctx, const void *tab, size_t n, int on_device, void *stream) {
  if (!ctx || (!tab && n)) return fail(MSM_E_ARG, "bad args");
  if (multi_device_arg(ctx, on_device)) return fail(MSM_E_ARG, "a multi-device context takes a host table");
  return set_table_ctx(ctx, [&](auto &e) { e.set_table(tab, n, on_device != 0, (hipStream_t)stream); });
}

int msm_ches_ctx_get_table(msm_ches_ctx *ctx, void *out, size_t first, size_t count) {
  return get_table_ctx(ctx, out, first, count, MSM_E_HIP);
}

// (the CHES mults hand the scalars to the engine where they are: host scalars
// are staged per shard, or set by set inside the pipeline, Ches::run_batch)
int msm_ches_ctx_mult(msm_ches_ctx *ctx, void *ret, const byte *scalars, size_t stride, int on_device,
                      void *stream) {
  if (!ctx || !ret || stride < 32) return fail(MSM_E_ARG, "bad args (stride must be >= 32)");
  if (!ctx->ready) return fail(MSM_E_STATE, "no table: build_table, set_table or load_table first");
  if (multi_device_arg(ctx, on_device)) return fail(MSM_E_ARG, "a multi-device context takes host scalars");
  return guarded(MSM_E_HIP, [&] {
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    ctx->with([&](auto &e) {
      mult_out(e, ret, 1, [&](auto *out) { e.run(s, scalars, stride, on_device != 0, out); });
    });
    return MSM_OK;
  });
}

int msm_ches_ctx_mult_batch(msm_ches_ctx *ctx, void *rets, const byte *scalars, size_t stride, size_t set_stride,
                            size_t count, int on_device, void *stream) {
  if (!ctx || (!rets && count) || stride < 32) return fail(MSM_E_ARG, "bad args (stride must be >= 32)");
  if (!ctx->ready) return fail(MSM_E_STATE, "no table: build_table, set_table or load_table first");
  if (multi_device_arg(ctx, on_device)) return fail(MSM_E_ARG, "a multi-device context takes host scalars");
  return guarded(MSM_E_HIP, [&] {
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    const bool on_host = !on_device;
    ctx->with([&](auto &e) {
      mult_out(e, rets, count, [&](auto *out) { e.run_batch(s, scalars, stride, set_stride, count, out, on_host); });
    });
    return MSM_OK;
  });
}

int msm_ches_ctx_set_profiling(msm_ches_ctx *ctx, int on) {
  if (!ctx) return fail(MSM_E_ARG, "null ctx");
  ctx->with([&](auto &e) { e.set_profiling(on != 0); });
  return MSM_OK;
}

int msm_ches_ctx_phase_times(const msm_ches_ctx *ctx, float out[6]) {
  if (!ctx || !out) return fail(MSM_E_ARG, "null");
  phase_times_out(ctx->with([](auto &e) -> const PhaseTimes & { return e.front().times(); }), out);
  return MSM_OK;
}

size_t msm_ches_ctx_bucket_count(const msm_ches_ctx *ctx) {
  return ctx ? ctx->with([](auto &e) { return e.front().bucket_count(); }) : 0;
}

int msm_ches_ctx_batch_lanes(const msm_ches_ctx *ctx) {
  return ctx ? ctx->with([](auto &e) { return e.front().batch_lanes(); }) : 0;
}

int msm_ches_ctx_time_accumulation(msm_ches_ctx *ctx, const byte *scalars, size_t set_stride, int nsets, int reps,
                                   float *ms) {
  if (!ctx || !scalars || !ms || nsets < 1 || reps < 1) return fail(MSM_E_ARG, "bad args");
  if (!ctx->ready) return fail(MSM_E_STATE, "no table");
  if (ctx->with([](auto &e) { return e.engines(); }) != 1) return fail(MSM_E_ARG, "single-device contexts only");
  return guarded(MSM_E_HIP, [&] {
    DeviceGuard g(ctx->device);
    *ms = ctx->with([&](auto &e) {
      return e.front().time_accumulation((hipStream_t)0, scalars, set_stride, nsets, reps);
    });
    return MSM_OK;
  });
}

void msm_ches_ctx_destroy(msm_ches_ctx *ctx) { delete ctx; }

// ---------------- BGMW95 contexts ----------------
// (a throwing Bgmw / Wbits constructor, and a throwing Wbits::get_table, give MSM_E_ARG
// where the other families give MSM_E_HIP: kept as the callers have seen it)
int msm_bgmw_ctx_create(msm_bgmw_ctx **ctx, int group, int device, int q_exp, int h) {
  if (!ctx || (group != 1 && group != 2)) return fail(MSM_E_ARG, "bad ctx/group");
  if (!device_ok(device)) return no_device();
  return create_ctx(ctx, group, device, MSM_E_ARG,
                    [&](auto g) { return std::make_unique<Bgmw<decltype(g)::value>>(device, q_exp, h); });
}

int msm_bgmw_ctx_build_table(msm_bgmw_ctx *ctx, const void *pts, size_t n, int on_device, void *stream) {
  if (!ctx || (!pts && n)) return fail(MSM_E_ARG, "bad args");
  return set_table_ctx(ctx, [&](auto &e) { e.build_table(pts, n, on_device != 0, (hipStream_t)stream); });
}

int msm_bgmw_ctx_set_table(msm_bgmw_ctx *ctx, const void *tab, size_t n, int on_device, void *stream) {
  if (!ctx || (!tab && n)) return fail(MSM_E_ARG, "bad args");
  return set_table_ctx(ctx, [&](auto &e) { e.set_table(tab, n, on_device != 0, (hipStream_t)stream); });
}

int msm_bgmw_ctx_get_table(msm_bgmw_ctx *ctx, void *out, size_t first, size_t count) {
  return get_table_ctx(ctx, out, first, count, MSM_E_HIP);
}

int msm_bgmw_ctx_mult(msm_bgmw_ctx *ctx, void *ret, const byte *scalars, size_t stride, int on_device,
                      void *stream) {
  if (!ctx || !ret || stride < 32) return fail(MSM_E_ARG, "bad args (stride must be >= 32)");
  if (!ctx->ready) return fail(MSM_E_STATE, "no table: build_table, set_table or load_table first");
  return guarded(MSM_E_HIP, [&] {
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    ctx->with([&](auto &e) {
      const uint8_t *d = stage_scalars(ctx->scalars, scalars, e.npoints() * stride, on_device != 0, s);
      mult_out(e, ret, 1, [&](auto *out) { e.run(s, d, stride, out); });
    });
    return MSM_OK;
  });
}

int msm_bgmw_ctx_set_profiling(msm_bgmw_ctx *ctx, int on) {
  if (!ctx) return fail(MSM_E_ARG, "null ctx");
  ctx->with([&](auto &e) { e.set_profiling(on != 0); });
  return MSM_OK;
}

int msm_bgmw_ctx_phase_times(const msm_bgmw_ctx *ctx, float out[6]) {
  if (!ctx || !out) return fail(MSM_E_ARG, "null");
  phase_times_out(ctx->with([](auto &e) -> const PhaseTimes & { return e.times(); }), out);
  return MSM_OK;
}

size_t msm_bgmw_ctx_bucket_count(const msm_bgmw_ctx *ctx) {
  return ctx ? ctx->with([](auto &e) { return e.bucket_count(); }) : 0;
}

void msm_bgmw_ctx_destroy(msm_bgmw_ctx *ctx) { delete ctx; }

// ---------------- table files (method 1: CHES, 2: BGMW95) ----------------
static const auto ches_qh = [](auto &e) { return std::make_pair(e.params().q_exp, e.params().h); };
static const auto bgmw_qh = [](auto &e) { return std::make_pair(e.q_exp(), e.h()); };

int msm_ches_ctx_save_table(msm_ches_ctx *ctx, const char *path) { return save_table_ctx(ctx, path, 1, ches_qh); }
int msm_ches_ctx_load_table(msm_ches_ctx *ctx, const char *path) { return load_table_ctx(ctx, path, 1, ches_qh); }
int msm_bgmw_ctx_save_table(msm_bgmw_ctx *ctx, const char *path) { return save_table_ctx(ctx, path, 2, bgmw_qh); }
int msm_bgmw_ctx_load_table(msm_bgmw_ctx *ctx, const char *path) { return load_table_ctx(ctx, path, 2, bgmw_qh); }

size_t msm_ches_bucket_set(int q, int a_h, int *out, size_t cap) {
  if (q < 4 || a_h < 0) return 0;
  std::vector<int> B = ches_bucket_set(q, a_h);
  if (out) memcpy(out, B.data(), std::min(cap, B.size()) * sizeof(int));
  return B.size();
}

int msm_ches_digit_table(int q, int a_h, digit_decomposition *out) {
  if (q < 4 || a_h < 0 || !out) return fail(MSM_E_ARG, "bad args");
  return guarded(MSM_E_ARG, [&]() -> int {  // (MSM_E_ARG: host work only, what throws here is q / a_h)
    // decoded from the compact device tables (code + rank, ches_kernels.hpp)
    // with the device's arithmetic, so the golden digit-table hashes pin them
    std::vector<int> B = ches_bucket_set(q, a_h);
    std::vector<uint32_t> code, rank;
    ches_digit_code(B, q, code, rank);
    for (size_t d = 0; d <= (size_t)q; ++d) {
      const uint32_t c = (code[d >> 3] >> (4 * (d & 7))) & 15u, m = (c & 3u) + 1, alpha = (c >> 2) & 1u;
      int b = 0;
      if (!(c & 8u)) {
        const uint32_t v = (alpha ? (uint32_t)q - (uint32_t)d : (uint32_t)d) / m;
        const uint32_t bits = rank[2 * (v >> 5)], idx = rank[2 * (v >> 5) + 1] +
                                                        (uint32_t)__builtin_popcount(bits & ((1u << (v & 31)) - 1u));
        if (!((bits >> (v & 31)) & 1u)) return fail(MSM_E_ARG, "digit code names a value outside B");
        b = B[idx];
      }
      out[d].m = (int)m;
      out[d].b = b;
      out[d].alpha = (int)alpha;
    }
    return MSM_OK;
  });
}

// ---------------- boundary helpers ----------------
static uint64_t splitmix64(uint64_t *s) {
  uint64_t z = (*s += 0x9e3779b97f4a7c15ULL);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}
void msm_gen_scalars(byte *out, size_t n, uint64_t seed) {
  static const uint64_t R[4] = {0xffffffff00000001ULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL,
                                0x73eda753299d7d48ULL};
  uint64_t st = seed;
  for (size_t i = 0; i < n; ++i) {
    uint64_t a[4];
    for (;;) {
      for (int k = 0; k < 4; ++k) a[k] = splitmix64(&st);
      a[3] >>= 1;
      bool lt = false;
      for (int k = 3; k >= 0; --k) {
        if (a[k] != R[k]) {
          lt = a[k] < R[k];
          break;
        }
      }
      if (lt) break;
    }
    for (int k = 0; k < 32; ++k) out[32 * i + k] = (uint8_t)(a[k / 8] >> (8 * (k % 8)));
  }
}

void msm_p1_fixed_points(blst_p1_affine *out, size_t n) { msm_p1_fixed_points_range(out, 0, n); }
void msm_p2_fixed_points(blst_p2_affine *out, size_t n) { msm_p2_fixed_points_range(out, 0, n); }
void msm_p1_fixed_points_range(blst_p1_affine *out, size_t start, size_t n) {
  hfp::Jac<hfp::Fp> g = hfp::g1_generator();
  for (size_t i = 0; i < start; ++i) g = hfp::dbl(g);
  fixed_points<hfp::Fp>(reinterpret_cast<hfp::Aff<hfp::Fp> *>(out), n, g);
}
void msm_p2_fixed_points_range(blst_p2_affine *out, size_t start, size_t n) {
  hfp::Jac<hfp::Fp2> g = hfp::g2_generator();
  for (size_t i = 0; i < start; ++i) g = hfp::dbl(g);
  fixed_points<hfp::Fp2>(reinterpret_cast<hfp::Aff<hfp::Fp2> *>(out), n, g);
}
void msm_p1_to_affine(blst_p1_affine *out, const blst_p1 *in) {
  *reinterpret_cast<hfp::Aff<hfp::Fp> *>(out) = hfp::to_affine(*reinterpret_cast<const hfp::Jac<hfp::Fp> *>(in));
}
void msm_p2_to_affine(blst_p2_affine *out, const blst_p2 *in) {
  *reinterpret_cast<hfp::Aff<hfp::Fp2> *>(out) = hfp::to_affine(*reinterpret_cast<const hfp::Jac<hfp::Fp2> *>(in));
}
void msm_p1_compress(byte out[48], const blst_p1 *in) {
  hfp::compress(out, hfp::to_affine(*reinterpret_cast<const hfp::Jac<hfp::Fp> *>(in)));
}
void msm_p2_compress(byte out[96], const blst_p2 *in) {
  hfp::compress(out, hfp::to_affine(*reinterpret_cast<const hfp::Jac<hfp::Fp2> *>(in)));
}
void msm_p1_add(blst_p1 *out, const blst_p1 *a, const blst_p1 *b) {
  *reinterpret_cast<hfp::Jac<hfp::Fp> *>(out) = hfp::addj(*reinterpret_cast<const hfp::Jac<hfp::Fp> *>(a),
                                                          *reinterpret_cast<const hfp::Jac<hfp::Fp> *>(b));
}
void msm_p2_add(blst_p2 *out, const blst_p2 *a, const blst_p2 *b) {
  *reinterpret_cast<hfp::Jac<hfp::Fp2> *>(out) = hfp::addj(*reinterpret_cast<const hfp::Jac<hfp::Fp2> *>(a),
                                                           *reinterpret_cast<const hfp::Jac<hfp::Fp2> *>(b));
}

int msm_test_field(int group, int op, const limb_t *a, const limb_t *b, limb_t *out, size_t n) {
  return guarded(MSM_E_HIP, [&] {
    by_group(group, [&](auto g) { test_field<decltype(g)::value>(op, a, b, out, n); });
    return MSM_OK;
  });
}
int msm_test_xyzz(int group, const void *pts, size_t npts, const uint32_t *ops, int len, size_t nseq, void *out) {
  return guarded(MSM_E_HIP, [&] {
    by_group(group, [&](auto g) {
      test_xyzz<decltype(g)::value>((const uint64_t *)pts, npts, ops, len, nseq, (uint64_t *)out);
    });
    return MSM_OK;
  });
}
int msm_test_fp12(int op, int k, int alias, int raw, const void *a, const void *b, void *out, size_t n) {
  if (op < TEST_FP12_MUL || op > TEST_FP12_LINE_ADD) return fail(MSM_E_ARG, "unknown op");
  if (op == TEST_FP12_FROB && (k < 1 || k > 3)) return fail(MSM_E_ARG, "Frobenius power outside 1..3");
  if (op == TEST_FP12_CSQR && (k < 1 || k > 64)) return fail(MSM_E_ARG, "squaring count outside 1..64");
  const bool binary = op == TEST_FP12_MUL || op == TEST_FP12_SPARSE;
  // d == a wherever the operation works from memory to memory and allows it; d == b for the product only
  const bool alias_ok = alias == 0 || (alias == 1 && op <= TEST_FP12_CSQR && op != TEST_FP12_INV) ||
                        (alias == 2 && op == TEST_FP12_MUL);
  if (!alias_ok || (raw != 0 && raw != 1)) return fail(MSM_E_ARG, "bad alias / raw");
  if (n && (!a || !out || (binary && !b))) return fail(MSM_E_ARG, "null operand");
  if (!n) return MSM_OK;
  if (!device_ok(0)) return no_device();
  return guarded(MSM_E_HIP, [&] {
    test_fp12(op, k, alias, raw != 0, a, binary ? b : nullptr, out, n);
    return MSM_OK;
  });
}
int msm_test_fp_ops(int field, int form, int op, const uint32_t *in, const uint32_t *flags, uint32_t *out, size_t n,
                    size_t cap) {
  const TestFpOp *d = test_fp_op(op);
  if (!d) return fail(MSM_E_ARG, "unknown op");
  if (field < TEST_FIELD_FP || field > TEST_FIELD_FP2L) return fail(MSM_E_ARG, "unknown field");
  if (form != TEST_FORM_SPLIT && form != TEST_FORM_CHAIN) return fail(MSM_E_ARG, "unknown form");
  if (form == TEST_FORM_CHAIN && (!d->forms || field != TEST_FIELD_FP))
    return fail(MSM_E_ARG, "no single-chain form of this op on this field");
  if (d->fp_only && field != TEST_FIELD_FP) return fail(MSM_E_ARG, "an Fp-only op");
  if ((op == TEST_COOP_ADD || op == TEST_F_MUL_SUB_BS) && field == TEST_FIELD_FP2)
    return fail(MSM_E_ARG, "the one-lane Fp2 has no f_mul_sub_bs and no cooperative kernel");
  if (cap < n) return fail(MSM_E_ARG, "cap < n");
  if (n && ((d->nin && !in) || (d->flags && !flags) || !out)) return fail(MSM_E_ARG, "null operand");
  if (!n) return MSM_OK;
  if (!device_ok(0)) return no_device();
  return guarded(MSM_E_HIP, [&] {
    if (op != TEST_COOP_ADD) test_fp_ops(field, form, op, in, flags, out, n, cap);
    else if (field == TEST_FIELD_FP) test_coop_pair_add<1>(in, out, n, cap);
    else test_coop_pair_add<2>(in, out, n, cap);
    return MSM_OK;
  });
}

// ---------------- fixed-window (wbits) contexts ----------------
int msm_wbits_ctx_create(msm_wbits_ctx **ctx, int group, int device, int wbits) {
  if (!ctx || (group != 1 && group != 2)) return fail(MSM_E_ARG, "bad ctx/group");
  if (!device_ok(device)) return no_device();
  return create_ctx(ctx, group, device, MSM_E_ARG,
                    [&](auto g) { return std::make_unique<Wbits<decltype(g)::value>>(device, wbits); });
}

int msm_wbits_ctx_precompute(msm_wbits_ctx *ctx, const void *pts, size_t n, int on_device, void *stream) {
  if (!ctx || (!pts && n)) return fail(MSM_E_ARG, "bad args");
  return set_table_ctx(ctx, [&](auto &e) { e.precompute(pts, n, on_device != 0, (hipStream_t)stream); });
}

int msm_wbits_ctx_set_table(msm_wbits_ctx *ctx, const void *tab, size_t n, int on_device, void *stream) {
  if (!ctx || (!tab && n)) return fail(MSM_E_ARG, "bad args");
  return set_table_ctx(ctx, [&](auto &e) { e.set_table(tab, n, on_device != 0, (hipStream_t)stream); });
}

int msm_wbits_ctx_get_table(msm_wbits_ctx *ctx, void *out, size_t first, size_t count) {
  return get_table_ctx(ctx, out, first, count, MSM_E_ARG);
}

int msm_wbits_ctx_mult(msm_wbits_ctx *ctx, void *ret, const byte *scalars, size_t stride, size_t nbits,
                       int on_device, void *stream) {
  if (!ctx || !ret || stride == 0 || (nbits + 7) / 8 > stride) return fail(MSM_E_ARG, "bad args (stride < nbits/8)");
  if (!ctx->ready) return fail(MSM_E_STATE, "no table: precompute or set_table first");
  return guarded(MSM_E_HIP, [&] {
    DeviceGuard g(ctx->device);
    hipStream_t s = (hipStream_t)stream;
    ctx->with([&](auto &e) {
      const uint8_t *d = stage_scalars(ctx->scalars, scalars, e.npoints() * stride, on_device != 0, s);
      mult_out(e, ret, 1, [&](auto *out) { e.run(s, d, stride, (int)nbits, out); });
    });
    return MSM_OK;
  });
}

size_t msm_wbits_ctx_table_rows(const msm_wbits_ctx *ctx) {
  return ctx ? ctx->with([](auto &e) { return e.table_rows(); }) : 0;
}

void msm_wbits_ctx_destroy(msm_wbits_ctx *ctx) { delete ctx; }

}  // extern "C"
