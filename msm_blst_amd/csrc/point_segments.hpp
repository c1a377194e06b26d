// point_segments.hpp -- segmented sums and MSMs on the GPU:
// dst[j] = sum over offsets[j] <= i < offsets[j + 1] of [k_i] P_i
// (replaces a host loop over the reference's blst_p{1,2}s_mult_pippenger /
// blst_p{1,2}s_add, one call per point set: ref src/multi_scalar.c:581-607,
// src/bulk_addition.c:145-164; kernels and orchestration in point_segments.hip,
// the host plan in segments_plan.hpp).  This header is host-only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cstring>

#include "chunk_pipe.hpp"
#include "segments_plan.hpp"

namespace msm {

// The lane of a chunk's plan (SegPlanner), shared with pairing.hip: two pinned
// slots with events of their own, and one device copy, written on the compute
// stream in front of the chunk's kernels.
class SegPlanLane {
 public:
  explicit SegPlanLane(int device) : ev_(device) {}
  void ensure(const SegSizes &z) {
    dmeta_.ensure(z.META);
    pin_.ensure(z.META, false);
    src_at_ = z.pmax * sizeof(SegMeta);
  }
  // the plan of the chunk in `slot` goes up on cs
  void send(hipStream_t cs, int slot, const SegPlanner &pl) {
    const size_t mb = pl.np() * sizeof(SegMeta), sb = pl.nseg() * sizeof(uint32_t);
    MSM_HIP_CHECK(hipEventSynchronize(ev_[slot]));  // chunk k - 2's plan has left the pinned slot
    uint8_t *pm = static_cast<uint8_t *>(pin_.pin[slot]);
    if (mb) memcpy(pm, pl.meta.data(), mb);
    if (sb) memcpy(pm + src_at_, pl.src.data(), sb);
    if (mb) MSM_HIP_CHECK(hipMemcpyAsync(dmeta_.p, pm, mb, hipMemcpyHostToDevice, cs));
    if (sb) MSM_HIP_CHECK(hipMemcpyAsync(dmeta_.as<uint8_t>() + src_at_, pm + src_at_, sb, hipMemcpyHostToDevice, cs));
    MSM_HIP_CHECK(hipEventRecord(ev_[slot], cs));
  }
  const SegMeta *d_meta() const { return dmeta_.as<SegMeta>(); }
  const uint32_t *d_src() const { return reinterpret_cast<const uint32_t *>(dmeta_.as<uint8_t>() + src_at_); }
  size_t device_bytes() const { return dmeta_.bytes; }

 private:
  DevBuf dmeta_;
  Stage pin_;          // pinned only
  size_t src_at_ = 0;  // the sources follow the pmax entries of the call
  EventPair ev_;       // (last: it waits for the copies before the slots go)
};

// One engine: the table of a chunk (xyzz multiples, then their affine rows; the
// partial sums reuse the xyzz buffer), the segment results, the level buffer of
// the shared inversion tree (to_affine.hpp), the partial carried from one chunk
// into the next, the plan of a chunk (two pinned slots with events of their
// own, one device copy), and for host memory a staging lane per direction on
// the shared chunk pipe (chunk_pipe.hpp).  A staged input slot holds the
// points followed by the scalars, packed (nbits + 7) / 8 bytes apart.
template <int G>
class PointSegments {
 public:
  static constexpr size_t AFF = 96 * G, ROW = 112 * G, XYZZ = 224 * G, ELEM = 56 * G;
  explicit PointSegments(int device) : dev_(device), plan_lane_(device), pipe_(device) {}
  // dst[j] = sum_{o[j] <= i < o[j + 1]} [k_i] P_i for j < k, o = offsets (host,
  // k + 1 values, non-decreasing).  k_i = the low nbits bits of the
  // little-endian scalar at scalars + i stride (0 < nbits <= 256, stride >=
  // (nbits + 7) / 8), or 1 when scalars is NULL.  points and scalars are both
  // host or both device memory (src_dev) and are indexed from point 0; dst is
  // flat, host or device.  `cs` orders the kernels (the caller's stream when a
  // side is device memory, else the engine's).  Device destination: returns
  // with the work queued on cs; host destination: returns with the data in dst.
  void run(hipStream_t cs, const void *points, const uint8_t *scalars, const size_t *offsets, size_t k, void *dst,
           int nbits, size_t stride, bool src_dev, bool dst_dev);
  size_t device_bytes() const {
    return xz_.bytes + rows_.bytes + res_.bytes + lv_.bytes + carry_.bytes + plan_lane_.device_bytes() +
           in_.device_bytes() + out_.device_bytes();
  }
  int device() const { return dev_; }

 private:
  int dev_;
  DevBuf xz_, rows_, res_, lv_, carry_;
  Stage in_, out_;
  SegPlanner plan_;        // the plan of the chunk being queued
  SegPlanLane plan_lane_;  // and its way to the device
  ChunkPipe pipe_;         // (last: it waits for the queued work before the buffers go)
};

}  // namespace msm
