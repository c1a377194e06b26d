// sig_verify.hip -- bulk BLS signature verification on one MI355X (replaces a
// host loop over the reference's blst_core_verify_pk_in_g{1,2} and the
// blst_pairing_* aggregation sequences: ref src/aggregate.c).
//
// The engine queues the other bulk engines on one stream (sig_verify.hpp); its
// own device code is small:
//   k_sig_screen  point i (blst affine, left alone) -> a code byte: the status
//                 it came with (a failed decode), else SIG_INF for the all-zero
//                 point, else 0 in the prime-order subgroup and 3 outside it;
//                 the test is decode_dev.hpp's dec_in_group, the one k_decode_group
//                 runs.  G1 a lane per point, G2 a lane pair.
//   k_sig_pairs   the P (96-byte rows) and Q (192-byte rows) arrays of the pairing
//                 call: per check a row per tuple and the row (-g, S_j), at the
//                 positions of the host plan; every row of a check whose code is
//                 non-zero is all zero, so that no point outside the subgroups
//                 reaches k_pair_miller.  A lane per 48-byte coordinate.  In
//                 SIG_VERIFY the lane of a row's first coordinate also reports a
//                 key sum that is infinite.
//
// Per chunk the codes of the points come down once, the host reduces them to a
// code per check (sig_plan.hpp) and sends those up with the rows' plan -- while
// the sums, the hashes and the weights, which do not depend on them, run; the
// verdicts of the pairing call end the chunk.
#include "sig_verify.hpp"

#include <cstring>

#include "decode_dev.hpp"

namespace msm {

// -g1 and -g2, blst affine
static __constant__ uint64_t SIG_NEG_G1[12] = {
    0x5cb38790fd530c16ull, 0x7817fc679976fff5ull, 0x154f95c7143ba1c1ull, 0xf0ae6acdf3d0e747ull,
    0xedce6ecc21dbf440ull, 0x120177419e0bfb75ull, 0xff526c2af318883aull, 0x92899ce4383b0270ull,
    0x89d7738d9fa9d055ull, 0x12caf35ba344c12aull, 0x3cff1b76964b5317ull, 0x0e44d2ede9774430ull};
static __constant__ uint64_t SIG_NEG_G2[24] = {
    0xf5f28fa202940a10ull, 0xb3f5fb2687b4961aull, 0xa1a893b53e2ae580ull, 0x9894999d1a3caee9ull,
    0x6f67b7631863366bull, 0x058191924350bcd7ull, 0xa5a9c0759e23f606ull, 0xaaa0c59dbccd60c3ull,
    0x3bb17e18e2867806ull, 0x1b1ab6cc8541b367ull, 0xc2b6ed0ef2158547ull, 0x11922a097360edf3ull,
    0x6d8bf5079fb65e61ull, 0xc52f05df531d63a5ull, 0x7f4a4d344ca692c9ull, 0xa887959b8577c95full,
    0x4347fe40525c8734ull, 0x197d145bbaff0bb5ull, 0x0c3e036d209afa4eull, 0x0601d8f4863f9e23ull,
    0xe0832636bacc0a84ull, 0xeb2def362a476f84ull, 0x64044f659f0ee1e9ull, 0x0ed54f48d5a1caa7ull};

// lane (pair) t < n: code[t] of point t; st_in (may be NULL): the status of a decode
template <int G>
static __global__ void __launch_bounds__(128, 2)
    k_sig_screen(const uint64_t *__restrict__ pts, const uint8_t *st_in, uint8_t *code, size_t n) {  // (st_in may be code)
  typedef typename DecLane<G>::LF LF;
  const size_t tt = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int comp = G == 2 ? (int)(tt & 1) : 0;
  const size_t t = G == 2 ? tt >> 1 : tt;
  if (t >= n) return;  // whole pairs only
  const uint64_t *o = pts + t * 12 * G;
  Aff<LF> p;
  fp_from_blst(dec_c(p.x), o + 6 * comp);
  fp_from_blst(dec_c(p.y), o + 6 * G + 6 * comp);
  const bool zx = f_is_zero_exact(p.x), zy = f_is_zero_exact(p.y);
  const bool ok = dec_in_group<G>(p);
  const uint8_t st = st_in ? st_in[t] : (uint8_t)0;
  if (comp == 0) code[t] = st ? st : (zx && zy) ? SIG_INF : ok ? SIG_OK : SIG_NOT_IN_GROUP;
}

// lane tid < 6 nent: coordinate tid % 6 (x_P, y_P, then the four of Q) of row tid / 6
static __global__ void __launch_bounds__(256)
    k_sig_pairs(const SigEntry *__restrict__ ent, size_t nent, const uint8_t *__restrict__ cc,
                const uint64_t *__restrict__ g1rows, const uint64_t *__restrict__ g2rows,
                const uint64_t *__restrict__ sigrows, int pkg, uint8_t *__restrict__ late, uint64_t *__restrict__ P,
                uint64_t *__restrict__ Q) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t e = tid / 6;
  const int w = (int)(tid % 6);
  if (e >= nent) return;
  const SigEntry en = ent[e];
  const bool sigrow = en.src == SIG_ROW_SIG, zero = cc[en.check] != 0, g1side = w < 2;
  const int v = g1side ? w : w - 2;  // the coordinate within its point
  // the generator's side of a signature row is a constant, everything else a row in device memory
  const bool gen = sigrow && (g1side == (pkg == 1));
  const uint64_t *src = nullptr;
  if (!sigrow) src = g1side ? g1rows + (size_t)en.src * 12 : g2rows + (size_t)en.src * 24;
  else if (!gen) src = sigrows + (size_t)en.check * (g1side ? 12 : 24);
  uint64_t *dst = g1side ? P + e * 12 + 6 * v : Q + e * 24 + 6 * v;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    uint64_t x;
    if (gen) x = g1side ? SIG_NEG_G1[6 * v + i] : SIG_NEG_G2[6 * v + i];
    else x = src[6 * v + i];
    dst[i] = zero ? 0 : x;
  }
  if (late && !sigrow && w == 0) {  // SIG_VERIFY: the sum of the keys is infinite
    const uint64_t *k = pkg == 1 ? g1rows + (size_t)en.src * 12 : g2rows + (size_t)en.src * 24;
    uint64_t acc = 0;
    for (int i = 0; i < 12 * pkg; ++i) acc |= k[i];
    late[en.check] = acc == 0 ? 1 : 0;
  }
}

template <int G>
static void screen(hipStream_t s, const void *d_pts, const uint8_t *d_st, uint8_t *d_code, size_t n) {
  if (!n) return;
  hipLaunchKernelGGL(k_sig_screen<G>, dim3(nblk(n * G, 128)), dim3(128), 0, s, static_cast<const uint64_t *>(d_pts),
                     d_st, d_code, n);
  MSM_HIP_CHECK(hipGetLastError());
}

// -------------------------------------------------------------- engine ----
template <int PKG>
void SigVerify<PKG>::run(hipStream_t cs, const SigCall &c, uint8_t *status) {
  if (!c.k) return;
  DeviceGuard g(dev_);
  const int mode = c.mode;
  const bool weighted = mode == SIG_BATCH && c.scalars && c.nbits > 0;
  const size_t nb = weighted ? ((size_t)c.nbits + 7) / 8 : 0;
  const size_t KIN = c.encoded ? KENC : KAFF, SIN = c.encoded ? SENC : SAFF;
  const size_t C = sig_chunk();
  const uint8_t *keys = static_cast<const uint8_t *>(c.keys), *sigs = static_cast<const uint8_t *>(c.sigs);
  std::vector<uint8_t> verdict;
  pipe_.begin(cs);
  for (size_t c0 = 0; c0 < c.k;) {
    const size_t c1 = sig_chunk_end(mode, c.o, c.pk, c.k, c0, C);
    sig_plan_chunk(pl_, mode, c.o, c.pk, c0, c1);
    const size_t nc = c1 - c0, nk = pl_.nkeys, ns = pl_.nsigs, nr = pl_.nrows, nent = pl_.ent.size();
    if (nent >= SIG_ROW_SIG) throw std::runtime_error("sig_verify: a check of 2^31 tuples or more");  // (SigEntry is 32-bit)
    // ---- the sources: where they lie, or through the staging lanes ----
    const uint8_t *d_kin = keys + pl_.k0 * KIN, *d_sin = sigs + pl_.s0 * SIN;
    const uint8_t *d_w = weighted ? c.scalars + pl_.r0 * c.stride : nullptr;
    size_t wstride = c.stride;
    if (!c.src_dev) {
      if (nk) in_k_.ensure(nk * KIN);
      if (ns) in_s_.ensure(ns * SIN);
      if (weighted && nr) in_w_.ensure(nr * nb);
      pipe_.upload(cs, 0, [&] {
        if (nk) memcpy(in_k_.pin[0], d_kin, nk * KIN);
        if (ns) memcpy(in_s_.pin[0], d_sin, ns * SIN);
        if (weighted)
          for (size_t i = 0; i < nr; ++i) memcpy(static_cast<uint8_t *>(in_w_.pin[0]) + i * nb, d_w + i * c.stride, nb);
      }, {{in_k_, 0, nk * KIN}, {in_s_, 0, ns * SIN}, {in_w_, 0, nr * nb}});  // (nb is 0 unless weighted)
      d_kin = in_k_.dev[0].as<uint8_t>(), d_sin = in_s_.dev[0].as<uint8_t>();
      if (weighted) d_w = in_w_.dev[0].as<uint8_t>(), wstride = nb;
    }
    // ---- decode and screen ----
    kcode_.ensure(std::max(nk, (size_t)1));
    scode_.ensure(std::max(ns, (size_t)1));
    const uint8_t *d_k = d_kin, *d_s = d_sin;
    if (c.encoded) {
      if (nk) {
        kaff_.ensure(nk * KAFF);
        dec_k_.kernels(cs, d_kin, kaff_.p, kcode_.as<uint8_t>(), nk, false, false);
        d_k = kaff_.as<uint8_t>();
      }
      if (ns) {
        saff_.ensure(ns * SAFF);
        dec_s_.kernels(cs, d_sin, saff_.p, scode_.as<uint8_t>(), ns, false, false);
        d_s = saff_.as<uint8_t>();
      }
    }
    screen<PKG>(cs, d_k, c.encoded ? kcode_.as<uint8_t>() : nullptr, kcode_.as<uint8_t>(), nk);
    screen<SG>(cs, d_s, c.encoded ? scode_.as<uint8_t>() : nullptr, scode_.as<uint8_t>(), ns);
    // ---- the codes start down; everything up to the rows is queued without waiting for them ----
    const size_t PLAN = nent * sizeof(SigEntry) + nc;
    codes_.ensure(std::max(nk + ns, nc) + 1, false);
    plan_.ensure(PLAN, false);
    uint8_t *hc = static_cast<uint8_t *>(codes_.pin[0]);
    if (nk) MSM_HIP_CHECK(hipMemcpyAsync(hc, kcode_.p, nk, hipMemcpyDeviceToHost, cs));
    if (ns) MSM_HIP_CHECK(hipMemcpyAsync(hc + nk, scode_.p, ns, hipMemcpyDeviceToHost, cs));
    MSM_HIP_CHECK(hipEventRecord(ev_codes_[0], cs));
    // ---- the key of every row: the key itself, or the sum of its set ----
    const uint8_t *d_rowkey = d_k;
    if (mode == SIG_VERIFY && c.pk) {
      ksum_.ensure(nc * KAFF);
      if (nk) sum_k_.run(cs, d_k, nullptr, pl_.key_off.data(), nc, ksum_.p, 0, 0, true, true);
      else MSM_HIP_CHECK(hipMemsetAsync(ksum_.p, 0, nc * KAFF, cs));
      d_rowkey = ksum_.as<uint8_t>();
    }
    // ---- the hashes ----
    const uint8_t *d_hash = nullptr;
    if (nr) {
      hash_.ensure(nr * SAFF);
      H2cMsgs m = c.m;
      if (m.offsets) m.offsets += pl_.r0;
      else if (m.msgs) m.msgs += pl_.r0 * m.msg_len;
      if (m.aug) m.aug += pl_.r0 * m.aug_len;
      h2c_.run(cs, H2C_HASH, nullptr, m, c.tmpl, hash_.p, nr, c.count, c.src_dev, true);
      d_hash = hash_.as<uint8_t>();
    }
    // ---- a batch: the weights on the G1 side of every tuple, and the weighted sums of the signatures ----
    const uint8_t *d_g1 = PKG == 1 ? d_rowkey : d_hash, *d_g2 = PKG == 1 ? d_hash : d_rowkey;
    if (weighted && nr) {
      g1w_.ensure(nr * 96);
      mult_.run(cs, d_g1, d_w, g1w_.p, nr, c.nbits, wstride, false, true, true);
      d_g1 = g1w_.as<uint8_t>();
    }
    const uint8_t *d_sigrow = d_s;
    if (mode == SIG_BATCH) {
      ssum_.ensure(nc * SAFF);
      if (ns) sum_s_.run(cs, d_s, weighted ? d_w : nullptr, pl_.sig_off.data(), nc, ssum_.p, c.nbits, wstride, true, true);
      else MSM_HIP_CHECK(hipMemsetAsync(ssum_.p, 0, nc * SAFF, cs));
      d_sigrow = ssum_.as<uint8_t>();
    }
    // ---- the checks' codes (the host's reduction) and the rows' plan go up, behind the work queued above ----
    MSM_HIP_CHECK(hipEventSynchronize(ev_codes_[0]));
    cch_.assign(nc, 0);
    sig_reduce(pl_, mode, c.o, c.pk, hc + nk, hc, cch_.data());
    uint8_t *hp = static_cast<uint8_t *>(plan_.pin[0]);
    memcpy(hp, pl_.ent.data(), nent * sizeof(SigEntry));
    memcpy(hp + nent * sizeof(SigEntry), cch_.data(), nc);
    ent_.ensure(PLAN);
    MSM_HIP_CHECK(hipMemcpyAsync(ent_.p, hp, PLAN, hipMemcpyHostToDevice, cs));
    const SigEntry *d_ent = ent_.as<SigEntry>();
    const uint8_t *d_cc = ent_.as<uint8_t>() + nent * sizeof(SigEntry);
    // ---- the rows and the pairing products ----
    p_.ensure(nent * Pairing::P_AFF);
    q_.ensure(nent * Pairing::Q_AFF);
    late_.ensure(nc);
    uint8_t *d_late = mode == SIG_VERIFY ? late_.as<uint8_t>() : nullptr;
    hipLaunchKernelGGL(k_sig_pairs, dim3(nblk(nent * 6, 256)), dim3(256), 0, cs, d_ent, nent, d_cc,
                       reinterpret_cast<const uint64_t *>(d_g1), reinterpret_cast<const uint64_t *>(d_g2),
                       reinterpret_cast<const uint64_t *>(d_sigrow), PKG, d_late, p_.as<uint64_t>(), q_.as<uint64_t>());
    MSM_HIP_CHECK(hipGetLastError());
    // (the late bytes are on the host before the verdicts, which pair_.run waits for, are)
    if (d_late) MSM_HIP_CHECK(hipMemcpyAsync(hc, d_late, nc, hipMemcpyDeviceToHost, cs));
    verdict.assign(nc, 0);
    pair_.run(cs, p_.p, q_.p, pl_.pair_off.data(), nc, nullptr, verdict.data(), true, true, false);
    pipe_.computed(cs, 0);
    for (size_t j = 0; j < nc; ++j)
      status[c0 + j] = sig_status(cch_[j], d_late && hc[j], verdict[j] == 1,
                                  pl_.pair_off[j + 1] - pl_.pair_off[j] - 1);
    c0 = c1;
  }
  pipe_.finish(cs);
}

template <int G>
void GroupScreen<G>::run(hipStream_t cs, const void *src, uint8_t *in_group, size_t n, bool src_dev) {
  if (!n) return;
  DeviceGuard g(dev_);
  const size_t C = std::min(n, dec_chunk());
  code_.ensure(C);
  out_.ensure(C, false);
  if (!src_dev) in_.ensure(C * AFF);
  pipe_.begin(cs);
  for (size_t c0 = 0; c0 < n; c0 += C) {
    const size_t cnt = std::min(C, n - c0);
    const void *d_src = static_cast<const uint8_t *>(src) + c0 * AFF;
    if (!src_dev) {
      pipe_.upload(cs, 0, [&] { memcpy(in_.pin[0], d_src, cnt * AFF); }, {{in_, 0, cnt * AFF}});
      d_src = in_.dev[0].p;
    }
    screen<G>(cs, d_src, nullptr, code_.as<uint8_t>(), cnt);
    pipe_.computed(cs, 0);
    MSM_HIP_CHECK(hipMemcpyAsync(out_.pin[0], code_.p, cnt, hipMemcpyDeviceToHost, cs));
    MSM_HIP_CHECK(hipStreamSynchronize(cs));
    const uint8_t *h = static_cast<const uint8_t *>(out_.pin[0]);
    for (size_t i = 0; i < cnt; ++i) in_group[c0 + i] = h[i] == SIG_NOT_IN_GROUP ? 0 : 1;
  }
  pipe_.finish(cs);
}

template class SigVerify<1>;
template class SigVerify<2>;
template class GroupScreen<1>;
template class GroupScreen<2>;

}  // namespace msm
