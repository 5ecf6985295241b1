// Owning types for the host code's HIP resources: device and pinned buffers,
// streams, events, and the fixed ring of staging slots that the signature units
// share.  All of them are move-only, release what they hold in their destructor,
// and make no HIP call while empty.
//
// Two rules for their users:
//   * a stream is drained before the buffers its queued work reads are released
//     (Lane's destructor, StageSlot's destructor, SlotRing's guard);
//   * state that lives as long as the process is never destroyed (a heap object
//     that is never deleted): its owners would otherwise call into a HIP runtime
//     that static destruction may already have torn down.
#pragma once
#include <hip/hip_runtime.h>
#include <string.h>
#include <algorithm>
#include <condition_variable>
#include <mutex>
#include <utility>

namespace fts {

struct DevMem {
  static hipError_t alloc(void** p, size_t n) { return hipMalloc(p, n); }
  static void free(void* p) { (void)hipFree(p); }
};
struct PinMem {
  static hipError_t alloc(void** p, size_t n) { return hipHostMalloc(p, n, hipHostMallocDefault); }
  static void free(void* p) { (void)hipHostFree(p); }
};

// One allocation and its capacity.  Re-allocation frees first (the contents are
// never carried over) and a failed one leaves the buffer empty.
template <class Mem>
struct OwnedBuf {
  void* p = nullptr;
  size_t cap = 0;
  OwnedBuf() = default;
  OwnedBuf(OwnedBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  OwnedBuf& operator=(OwnedBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = std::exchange(o.p, nullptr);
      cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~OwnedBuf() { release(); }
  // exactly `bytes` when the buffer holds fewer; false when the allocation fails
  bool reserve(size_t bytes) {
    if (bytes <= cap) return true;
    release();
    if (Mem::alloc(&p, bytes) != hipSuccess) return p = nullptr, false;
    cap = bytes;
    return true;
  }
  // grows geometrically: hipFree synchronises the whole device (stalling every
  // other lane's pass), so a buffer must not be re-allocated on every slightly
  // larger batch
  bool grow(size_t bytes, size_t floor = 256) {
    return bytes <= cap || reserve(std::max(std::max(bytes, cap + cap / 2), floor));
  }
  void release() {
    if (p) Mem::free(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};
using DevBuf = OwnedBuf<DevMem>;
using PinBuf = OwnedBuf<PinMem>;

// a stream or event handle; converts to the raw handle at launch sites
template <class H, hipError_t (*Destroy)(H)>
struct Handle {
  H h = nullptr;
  Handle() = default;
  Handle(Handle&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
  Handle& operator=(Handle&& o) noexcept {
    if (this != &o) {
      release();
      h = std::exchange(o.h, nullptr);
    }
    return *this;
  }
  ~Handle() { release(); }
  void release() {
    if (h) (void)Destroy(h);
    h = nullptr;
  }
  operator H() const { return h; }
};

struct Stream : Handle<hipStream_t, hipStreamDestroy> {
  // non-blocking (never ordered against the null stream)
  hipError_t create() {
    release();
    return hipStreamCreateWithFlags(&h, hipStreamNonBlocking);
  }
  hipError_t create(int priority) {
    release();
    return hipStreamCreateWithPriority(&h, hipStreamNonBlocking, priority);
  }
};

struct Event : Handle<hipEvent_t, hipEventDestroy> {
  hipError_t create(unsigned flags = hipEventDefault) {
    release();
    return hipEventCreateWithFlags(&h, flags);
  }
};

// Wipes a signing call's secrets from its staging slot on every way out of the call:
// the device region by a memset on the slot's stream (behind the last kernel), the
// pinned region after the stream has drained.  A call that has queued the device
// memset itself clears `dev`; one that has wiped the pinned region clears `host`.
struct SecretWipe {
  hipStream_t stream;
  void* dev = nullptr;
  void* host = nullptr;
  size_t bytes = 0;
  explicit SecretWipe(hipStream_t s) : stream(s) {}
  SecretWipe(const SecretWipe&) = delete;
  ~SecretWipe() {
    if (dev) (void)hipMemsetAsync(dev, 0, bytes, stream);
    if (dev || host) (void)hipStreamSynchronize(stream);
    if (host) memset(host, 0, bytes);
  }
};

// N staging slots shared by concurrent callers.  Slot has a `stream` member.
// acquire() blocks for a free slot; the guard it returns gives the slot back.
template <class Slot, int N>
struct SlotRing {
  std::mutex mu;
  std::condition_variable cv;
  Slot slot[N];
  bool busy[N] = {};
  SlotRing() = default;
  ~SlotRing() {  // before the slots' buffers go
    for (Slot& s : slot)
      if (s.stream) (void)hipStreamSynchronize(s.stream);
  }

  template <class Publish>
  struct Guard {
    SlotRing& r;
    int k;
    Publish publish;
    Guard(SlotRing& rr, int kk, Publish p) : r(rr), k(kk), publish(std::move(p)) {}
    Guard(const Guard&) = delete;
    Slot& slot() const { return r.slot[k]; }
    ~Guard() {
      // an error path may leave a copy or kernel queued on the slot's stream that
      // still reads its pinned staging / device buffers: drain it before the next
      // caller may reuse (or re-allocate) them
      if (r.slot[k].stream) (void)hipStreamSynchronize(r.slot[k].stream);
      std::lock_guard<std::mutex> l(r.mu);
      publish(r.slot[k]);
      r.busy[k] = false;
      r.cv.notify_one();
    }
  };

  // publish(slot) runs under the ring's lock when the guard dies: it copies the
  // call's timings to wherever the "last call" getters read them (under `mu`)
  template <class Publish>
  Guard<Publish> acquire(Publish publish) {
    std::unique_lock<std::mutex> l(mu);
    int k = -1;
    cv.wait(l, [&] {
      for (int j = 0; j < N && k < 0; j++)
        if (!busy[j]) k = j;
      return k >= 0;
    });
    busy[k] = true;
    return Guard<Publish>(*this, k, std::move(publish));
  }
};

}  // namespace fts
