// points_ntt_model.hpp -- the plan of points_ntt_plan.hpp run on the host with Fr
// elements in place of points (the group Z_r: a "scalar multiplication" is a
// product), and the twiddle table both the model and the engine use.  Plain C++,
// no HIP: msm_points_ntt_model (abi.cpp) and the stand-alone sanitizer program of
// the tests include it.  The loops are the engine's: chunks of whole transforms,
// passes, slices, items; only the element type differs.
#pragma once
#include <vector>

#include "host_fr.hpp"
#include "points_ntt_plan.hpp"

namespace msm {

// omega_n^e for e < n / 2, then n^-1 (Montgomery form)
inline std::vector<hfr::Fr> pn_twiddle_table(int log_n) {
  const size_t half = ((size_t)1 << log_n) >> 1;
  std::vector<hfr::Fr> tw(pn_twiddles(log_n));
  const hfr::Fr w = hfr::root_of_unity((unsigned)log_n);
  hfr::Fr p = hfr::ONE;
  for (size_t e = 0; e < half; ++e) {
    tw[e] = p;
    p = hfr::mul(p, w);
  }
  tw[half] = hfr::inverse(hfr::from_u64((uint64_t)1 << log_n));
  return tw;
}

// `batch` transforms, dst may be src.  chunk / slice: pn_chunk() / pn_slice() of the caller.
inline void pn_model(int log_n, int flags, size_t batch, hfr::Fr *dst, const hfr::Fr *src, size_t chunk,
                     size_t slice) {
  const size_t n = (size_t)1 << log_n;
  const std::vector<hfr::Fr> tw = pn_twiddle_table(log_n);
  const size_t T = pn_chunk_transforms(log_n, batch, chunk);
  std::vector<hfr::Fr> x(T * n), tab(pn_slice_items(log_n, flags, T, slice));
  for (size_t t0 = 0; t0 < batch; t0 += T) {
    const size_t tc = batch - t0 < T ? batch - t0 : T, cnt = tc << log_n;
    const hfr::Fr *s = src + (t0 << log_n);
    hfr::Fr *d = dst + (t0 << log_n);
    for (size_t i = 0; i < cnt; ++i) x[i] = s[((i >> log_n) << log_n) + pn_in_map(log_n, flags, i & (n - 1))];  // k_pn_load
    for (int p = 0; p < pn_passes(log_n, flags); ++p) {
      const int il = pn_items_log(log_n, p);
      const size_t items = tc << il;
      const bool level = !pn_is_scale(log_n, p), mult = pn_laddered(log_n, p);
      for (size_t g0 = 0; g0 < items; g0 += slice) {
        const size_t sc = items - g0 < slice ? items - g0 : slice;
        for (size_t u = 0; u < sc; ++u) {  // k_pn_bfly, k_pn_table
          const size_t g = g0 + u, base = (g >> il) << log_n;
          const PnItem it = pn_item(log_n, p, g & (((size_t)1 << il) - 1));
          if (level) {
            const hfr::Fr a = x[base + it.a], b = x[base + it.b];
            x[base + it.a] = hfr::add(a, b);
            x[base + it.b] = hfr::sub(a, b);
          }
          if (mult) tab[u] = x[base + it.b];
        }
        for (size_t u = 0; mult && u < sc; ++u) {  // k_pn_ladder
          const size_t g = g0 + u, base = (g >> il) << log_n;
          const PnItem it = pn_item(log_n, p, g & (((size_t)1 << il) - 1));
          x[base + it.b] = hfr::mul(tab[u], tw[it.e]);
        }
      }
    }
    std::vector<hfr::Fr> y(cnt);
    for (size_t i = 0; i < cnt; ++i) y[i] = x[((i >> log_n) << log_n) + pn_out_map(log_n, flags, i & (n - 1))];  // k_pn_store
    for (size_t i = 0; i < cnt; ++i) d[i] = y[i];
  }
}

}  // namespace msm
