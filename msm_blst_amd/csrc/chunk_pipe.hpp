// chunk_pipe.hpp -- the double-buffered chunk pipeline of the bulk engines
// (to_affine, decode, encode, points_mult, point_segments, hash_to_curve,
// pairing, sig_verify, fr_ntt, fr_poly).
// Host-only.  A call is cut into chunks; chunk k uses slot k & 1 of every
// staging lane, so chunk k + 1 is filled and uploaded while chunk k computes
// and chunk k - 1 is copied back and drained.  The pipe owns the copy streams
// and the events and the slot protocol; the loop, the sizes, the fill, the
// lanes and the kernels stay with the engine.
//
// The steps of chunk k in slot s, in the order an engine issues them, what
// each does, and the buffer each wait guards:
//   upload(cs, s, fill, lanes)
//       host waits ev_h2d[s]:   chunk k - 2 has left the pinned input slot
//       fill()                  the engine fills the pinned slot(s)
//       h2d waits ev_comp[s]:   chunk k - 2's kernels have read the device input slot
//       pinned -> device on h2d, one copy per lane in the order given
//       record ev_h2d[s] on h2d; cs waits for it
//   out_open(cs, s)
//       cs waits ev_d2h[s]:     chunk k - 2 has left the device output slot
//   (the engine queues its kernels on cs)
//   computed(cs, s)
//       record ev_comp[s] on cs
//   download(cs, s, pend, off, cnt, lanes)
//       d2h waits ev_comp[s]
//       device -> pinned on d2h, one copy per lane in the order given
//       record ev_d2h[s] on d2h
//       pend.push(s, off, cnt): host waits ev_d2h of chunk k - 1 and takes it out of its pinned slot
// A lane of zero bytes issues no copy.  out_open and computed stand alone: an
// engine whose source is device memory skips upload, one whose destination is
// device memory skips out_open and download, and computed is never skipped.
// begin(cs) / finish(cs) bracket a call: ev_busy is the last kernel of the
// previous call, which may still use the buffers an engine keeps per call
// (levels, tables, status), whatever stream that call was ordered on.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>
#include <utility>

#include "engine.hpp"
#include "env_size.hpp"

namespace msm {

// One staging lane: two pinned host slots and, unless the lane is pinned only
// (the status bytes of decode, the plan of point_segments, the template of
// hash_to_curve), two device slots.
struct Stage {
  void *pin[2] = {nullptr, nullptr};
  size_t pin_bytes = 0;
  DevBuf dev[2];
  Stage() = default;
  Stage(const Stage &) = delete;
  Stage &operator=(const Stage &) = delete;
  ~Stage() { free_pinned(); }
  // at least `bytes` per slot; a lane that grows frees both pinned slots, then allocates both
  void ensure(size_t bytes, bool device = true) {
    if (bytes > pin_bytes) {
      free_pinned();  // (waits for the copies that use them)
      for (int i = 0; i < 2; ++i) MSM_HIP_CHECK(hipHostMalloc(&pin[i], bytes, hipHostMallocDefault));
      pin_bytes = bytes;
    }
    if (device) {
      dev[0].ensure(bytes);
      dev[1].ensure(bytes);
    }
  }
  size_t device_bytes() const { return dev[0].bytes + dev[1].bytes; }

 private:
  void free_pinned() {
    for (int i = 0; i < 2; ++i) {
      if (pin[i]) (void)hipHostFree(pin[i]);
      pin[i] = nullptr;
    }
    pin_bytes = 0;
  }
};

// Two events, one per slot, for a lane with an order of its own (the plan of
// point_segments).  Destroyed after the queued work that records them is done.
class EventPair {
 public:
  explicit EventPair(int device) : dev_(device) {
    try {
      DeviceGuard g(dev_);
      for (int i = 0; i < 2; ++i) MSM_HIP_CHECK(hipEventCreateWithFlags(&ev_[i], hipEventDisableTiming));
    } catch (...) {
      destroy();
      throw;
    }
  }
  ~EventPair() { destroy(); }
  EventPair(const EventPair &) = delete;
  EventPair &operator=(const EventPair &) = delete;
  hipEvent_t operator[](int slot) const { return ev_[slot]; }

 private:
  int dev_;
  hipEvent_t ev_[2] = {nullptr, nullptr};
  void destroy() noexcept {
    int prev = -1;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(dev_);
    for (int i = 0; i < 2; ++i) {
      if (ev_[i]) (void)hipEventSynchronize(ev_[i]);
      if (ev_[i]) (void)hipEventDestroy(ev_[i]);
      ev_[i] = nullptr;
    }
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

class ChunkPipe {
 public:
  explicit ChunkPipe(int device) : dev_(device) {
    try {
      DeviceGuard g(dev_);
      MSM_HIP_CHECK(hipStreamCreateWithFlags(&h2d_, hipStreamNonBlocking));
      MSM_HIP_CHECK(hipStreamCreateWithFlags(&d2h_, hipStreamNonBlocking));
      for (int i = 0; i < 2; ++i) {
        MSM_HIP_CHECK(hipEventCreateWithFlags(&ev_h2d_[i], hipEventDisableTiming));
        MSM_HIP_CHECK(hipEventCreateWithFlags(&ev_comp_[i], hipEventDisableTiming));
        MSM_HIP_CHECK(hipEventCreateWithFlags(&ev_d2h_[i], hipEventDisableTiming));
      }
      MSM_HIP_CHECK(hipEventCreateWithFlags(&ev_busy_, hipEventDisableTiming));
    } catch (...) {
      destroy();  // what was made before the failure
      throw;
    }
  }
  // An engine declares its pipe after its buffers and lanes, so that this runs
  // (and waits for the queued work that uses them) before they are freed.
  ~ChunkPipe() { destroy(); }
  ChunkPipe(const ChunkPipe &) = delete;
  ChunkPipe &operator=(const ChunkPipe &) = delete;

  // ---- a call ----
  // cs waits for the last kernel of the previous call / the host does
  void begin(hipStream_t cs) { MSM_HIP_CHECK(hipStreamWaitEvent(cs, ev_busy_, 0)); }
  void begin_on_host() { MSM_HIP_CHECK(hipEventSynchronize(ev_busy_)); }
  void finish(hipStream_t cs) { MSM_HIP_CHECK(hipEventRecord(ev_busy_, cs)); }

  // One copy of a composite step: `bytes` between a pinned and a device
  // address (the status bytes of decode and of pairing come down from a buffer
  // that is no Stage), or slot `slot` of a Stage.  Zero bytes: no copy.
  struct Lane {
    void *pin;
    void *dev;
    size_t bytes;
    Lane(void *pinned, void *device, size_t n) : pin(pinned), dev(device), bytes(n) {}
    Lane(const Stage &st, int slot, size_t n) : pin(st.pin[slot]), dev(st.dev[slot].p), bytes(n) {}
  };

  // ---- a chunk goes up: fill() writes the pinned slots, the lanes carry them to the device ----
  template <class Fill>
  void upload(hipStream_t cs, int slot, Fill fill, std::initializer_list<Lane> lanes) {
    MSM_HIP_CHECK(hipEventSynchronize(ev_h2d_[slot]));
    fill();
    MSM_HIP_CHECK(hipStreamWaitEvent(h2d_, ev_comp_[slot], 0));
    for (const Lane &l : lanes)
      if (l.bytes) MSM_HIP_CHECK(hipMemcpyAsync(l.dev, l.pin, l.bytes, hipMemcpyHostToDevice, h2d_));
    MSM_HIP_CHECK(hipEventRecord(ev_h2d_[slot], h2d_));
    MSM_HIP_CHECK(hipStreamWaitEvent(cs, ev_h2d_[slot], 0));
  }

  // ---- its kernels ----
  void out_open(hipStream_t cs, int slot) { MSM_HIP_CHECK(hipStreamWaitEvent(cs, ev_d2h_[slot], 0)); }
  void computed(hipStream_t cs, int slot) { MSM_HIP_CHECK(hipEventRecord(ev_comp_[slot], cs)); }

  // ---- the results come down; the chunk before is drained while this one runs ----
  template <class Pend>
  void download(hipStream_t /* cs: the copies wait for computed(cs, slot) */, int slot, Pend &pend, size_t off,
                size_t cnt, std::initializer_list<Lane> lanes) {
    MSM_HIP_CHECK(hipStreamWaitEvent(d2h_, ev_comp_[slot], 0));
    for (const Lane &l : lanes)
      if (l.bytes) MSM_HIP_CHECK(hipMemcpyAsync(l.pin, l.dev, l.bytes, hipMemcpyDeviceToHost, d2h_));
    MSM_HIP_CHECK(hipEventRecord(ev_d2h_[slot], d2h_));
    pend.push(slot, off, cnt);
  }
  void out_wait(int slot) { MSM_HIP_CHECK(hipEventSynchronize(ev_d2h_[slot])); }

  // The one chunk whose results are on their way back.  push(slot, off, cnt)
  // at the end of download drains the chunk before (while this one runs) and
  // holds this one; flush() after the loop drains the last.  take(slot, off, cnt)
  // copies a drained chunk out of its pinned slot(s).
  template <class Take>
  class Pending {
   public:
    Pending(ChunkPipe &pipe, Take take) : pipe_(pipe), take_(std::move(take)) {}
    void push(int slot, size_t off, size_t cnt) {
      flush();
      slot_ = slot, off_ = off, cnt_ = cnt, held_ = true;
    }
    void flush() {
      if (!held_) return;
      held_ = false;
      pipe_.out_wait(slot_);
      take_(slot_, off_, cnt_);
    }

   private:
    ChunkPipe &pipe_;
    Take take_;
    bool held_ = false;
    int slot_ = 0;
    size_t off_ = 0, cnt_ = 0;
  };
  template <class Take>
  Pending<Take> pending(Take take) {
    return Pending<Take>(*this, std::move(take));
  }

 private:
  int dev_;
  hipStream_t h2d_ = nullptr, d2h_ = nullptr;
  hipEvent_t ev_h2d_[2] = {nullptr, nullptr}, ev_comp_[2] = {nullptr, nullptr}, ev_d2h_[2] = {nullptr, nullptr};
  hipEvent_t ev_busy_ = nullptr;  // the last kernel of the previous call
  void destroy() noexcept {
    int prev = -1;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(dev_);
    // queued work may still read the staging buffers and what the engine keeps per call
    if (ev_busy_) (void)hipEventSynchronize(ev_busy_);
    if (h2d_) (void)hipStreamSynchronize(h2d_);
    if (d2h_) (void)hipStreamSynchronize(d2h_);
    for (int i = 0; i < 2; ++i) {
      if (ev_comp_[i]) (void)hipEventSynchronize(ev_comp_[i]);
      if (ev_h2d_[i]) (void)hipEventDestroy(ev_h2d_[i]);
      if (ev_comp_[i]) (void)hipEventDestroy(ev_comp_[i]);
      if (ev_d2h_[i]) (void)hipEventDestroy(ev_d2h_[i]);
    }
    if (ev_busy_) (void)hipEventDestroy(ev_busy_);
    if (h2d_) (void)hipStreamDestroy(h2d_);
    if (d2h_) (void)hipStreamDestroy(d2h_);
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

}  // namespace msm
