// sig_plan.hpp -- the host plan of the bulk signature verification
// (sig_verify.hpp).  Plain C++, no HIP:
// tests/test_sigs_host.py compiles it alone under the sanitizers.
//
// A call holds k checks.  What a check owns, by mode (o = the caller's offsets):
//   SIG_VERIFY     signature j, message j, the keys pk[j] .. pk[j + 1] (pk NULL:
//                  key j); one pairing row (sum of the keys, H(message j))
//   SIG_AGGREGATE  signature j, the (key, message) tuples o[j] .. o[j + 1]; a
//                  row per tuple
//   SIG_BATCH      the (key, message, signature, scalar) tuples o[j] .. o[j + 1];
//                  a row per tuple
// and after its rows every check has one signature row: (-g, S_j).
//
// For a chunk of whole checks the plan gives the position of every row in the
// P and Q arrays of the pairing call, the pairing offsets, the segment offsets
// of the key sums and of the signature sums, and the reduction of the per-point
// codes and the pairing verdicts to one status per check.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "env_size.hpp"

namespace msm {

enum { SIG_VERIFY = 0, SIG_AGGREGATE = 1, SIG_BATCH = 2 };

// the code bytes of the screen: a BLST_ERROR value, or the marker of infinity
// (which is an error for a key and a skip for a signature)
constexpr uint8_t SIG_OK = 0, SIG_BAD_ENCODING = 1, SIG_NOT_ON_CURVE = 2, SIG_NOT_IN_GROUP = 3, SIG_VERIFY_FAIL = 5,
                  SIG_PK_IS_INFINITY = 6, SIG_INF = 0x80;

constexpr size_t SIG_CHUNK_DEFAULT = (size_t)1 << 16;
constexpr uint32_t SIG_ROW_SIG = 0x80000000u;  // SigEntry::src: the signature row of the check

// tuples per chunk: MSM_SIGS_CHUNK=<tuples> overrides the default, read at each call
inline size_t sig_chunk() {
  const size_t e = env_size("MSM_SIGS_CHUNK");
  return e ? e : SIG_CHUNK_DEFAULT;
}

// first row (tuple) of check j
inline size_t sig_row_begin(int mode, const size_t *o, size_t j) { return mode == SIG_VERIFY ? j : o[j]; }
// first key of check j
inline size_t sig_key_begin(int mode, const size_t *o, const size_t *pk, size_t j) {
  return mode == SIG_VERIFY ? (pk ? pk[j] : j) : o[j];
}
// first signature of check j
inline size_t sig_sig_begin(int mode, const size_t *o, size_t j) { return mode == SIG_BATCH ? o[j] : j; }

// The chunk that starts at check c0: the checks [c0, return value).  Chunks are
// cut at check boundaries and hold at most C tuples (in SIG_VERIFY also at
// most C keys); a check longer than that is a chunk of its own.
inline size_t sig_chunk_end(int mode, const size_t *o, const size_t *pk, size_t k, size_t c0, size_t C) {
  size_t c1 = c0;
  while (c1 < k) {
    const size_t rows = sig_row_begin(mode, o, c1 + 1) - sig_row_begin(mode, o, c0);
    const size_t keys = sig_key_begin(mode, o, pk, c1 + 1) - sig_key_begin(mode, o, pk, c0);
    if (c1 > c0 && (rows > C || keys > C || c1 - c0 >= C)) break;
    ++c1;
  }
  return c1;
}

// one row of the pairing call: the check it belongs to (relative to the chunk)
// and where its points come from (the row's index relative to the chunk, or
// SIG_ROW_SIG: the check's signature row)
struct SigEntry {
  uint32_t check, src;
};

struct SigChunkPlan {
  size_t c0 = 0, c1 = 0;              // the checks
  size_t r0 = 0, nrows = 0;           // first row (message) and their number
  size_t k0 = 0, nkeys = 0;           // first key and their number
  size_t s0 = 0, nsigs = 0;           // first signature and their number
  std::vector<SigEntry> ent;          // per row of the pairing call, in position order
  std::vector<size_t> pair_off;       // the pairing offsets, checks + 1 values
  std::vector<size_t> key_off;        // SIG_VERIFY with key sets: the keys of each check, from 0
  std::vector<size_t> sig_off;        // SIG_BATCH: the signatures of each check, from 0
};

inline void sig_plan_chunk(SigChunkPlan &pl, int mode, const size_t *o, const size_t *pk, size_t c0, size_t c1) {
  const size_t nc = c1 - c0;
  pl.c0 = c0, pl.c1 = c1;
  pl.r0 = sig_row_begin(mode, o, c0), pl.nrows = sig_row_begin(mode, o, c1) - pl.r0;
  pl.k0 = sig_key_begin(mode, o, pk, c0), pl.nkeys = sig_key_begin(mode, o, pk, c1) - pl.k0;
  pl.s0 = sig_sig_begin(mode, o, c0), pl.nsigs = sig_sig_begin(mode, o, c1) - pl.s0;
  pl.ent.clear();
  pl.pair_off.assign(nc + 1, 0);
  pl.key_off.clear();
  pl.sig_off.clear();
  for (size_t j = c0; j < c1; ++j) {
    pl.pair_off[j - c0] = pl.ent.size();
    for (size_t r = sig_row_begin(mode, o, j); r < sig_row_begin(mode, o, j + 1); ++r)
      pl.ent.push_back(SigEntry{(uint32_t)(j - c0), (uint32_t)(r - pl.r0)});
    pl.ent.push_back(SigEntry{(uint32_t)(j - c0), SIG_ROW_SIG});
  }
  pl.pair_off[nc] = pl.ent.size();
  if (mode == SIG_VERIFY && pk)
    for (size_t j = c0; j <= c1; ++j) pl.key_off.push_back(pk[j] - pl.k0);
  if (mode == SIG_BATCH)
    for (size_t j = c0; j <= c1; ++j) pl.sig_off.push_back(o[j] - pl.s0);
}

// the code of one step: infinity is an error for a key and a skip for a signature
inline uint8_t sig_step_code(uint8_t code, bool is_key) {
  if (code == SIG_INF) return is_key ? SIG_PK_IS_INFINITY : SIG_OK;
  return code;
}

// cc[j - c0] = the code of the first step of check j that fails, 0 when none
// does.  scode / kcode: the screen's bytes of the chunk's signatures and keys.
// The order: per tuple the signature, then its key(s); SIG_VERIFY and
// SIG_AGGREGATE have one signature, in front of everything.  A check without
// tuples runs no step.
inline void sig_reduce(const SigChunkPlan &pl, int mode, const size_t *o, const size_t *pk, const uint8_t *scode,
                       const uint8_t *kcode, uint8_t *cc) {
  for (size_t j = pl.c0; j < pl.c1; ++j) {
    uint8_t c = 0;
    const size_t kb = sig_key_begin(mode, o, pk, j) - pl.k0, ke = sig_key_begin(mode, o, pk, j + 1) - pl.k0;
    if (mode == SIG_BATCH) {
      for (size_t t = kb; t < ke && !c; ++t) {
        c = sig_step_code(scode[t], false);
        if (!c) c = sig_step_code(kcode[t], true);
      }
    } else if (mode == SIG_VERIFY || ke > kb) {
      c = sig_step_code(scode[j - pl.s0], false);
      for (size_t t = kb; t < ke && !c; ++t) c = sig_step_code(kcode[t], true);
    }
    cc[j - pl.c0] = c;
  }
}

// the status of a check: its code; for a set of keys whose sum is infinite
// (late, SIG_VERIFY) 6; else the verdict of the pairing product.  A check
// without tuples (rows == 0) fails: the reference's finalverify returns 0 when
// nothing was aggregated.
inline uint8_t sig_status(uint8_t cc, bool late_inf, bool is_one, size_t rows) {
  if (rows == 0) return SIG_VERIFY_FAIL;
  if (cc) return cc;
  if (late_inf) return SIG_PK_IS_INFINITY;
  return is_one ? SIG_OK : SIG_VERIFY_FAIL;
}

}  // namespace msm
