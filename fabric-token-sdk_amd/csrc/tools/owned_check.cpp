// Stand-alone check of host/hip_owned.hpp.  Assumes nothing about a device: with
// none, every HIP allocation fails and the failure paths are what runs; with one,
// the success paths run too.  Ownership bookkeeping (moves, exactly-once frees)
// is checked on OwnedBuf over a counting host allocator, which behaves the same
// everywhere.  Exit status 0 iff every check holds.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "../host/hip_owned.hpp"

using namespace fts;

static int g_failed = 0;
#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      fprintf(stderr, "owned_check: %s (line %d)\n", #x, __LINE__); \
      g_failed++;                                                 \
    }                                                             \
  } while (0)

struct CountMem {
  static int allocs, frees;
  static bool fail;
  static hipError_t alloc(void** p, size_t n) {
    if (fail) return hipErrorOutOfMemory;
    allocs++;
    *p = malloc(n);
    return hipSuccess;
  }
  static void free(void* p) {
    frees++;
    ::free(p);
  }
};
int CountMem::allocs = 0, CountMem::frees = 0;
bool CountMem::fail = false;
using CountBuf = OwnedBuf<CountMem>;

static void check_counting() {
  {
    CountBuf e;
    CHECK(!e.p && e.cap == 0);
  }
  CHECK(CountMem::allocs == 0 && CountMem::frees == 0);  // empty: the allocator is never called
  {
    CountBuf a;
    CHECK(a.grow(100) && a.cap == 256);  // the default floor
    void* p0 = a.p;
    CHECK(a.grow(200) && a.p == p0 && a.reserve(10) && a.p == p0);  // a smaller request keeps the pointer
    CHECK(a.grow(257) && a.cap == 384);                             // 1.5x headroom
    CHECK(a.grow(1000) && a.cap == 1000);
    CHECK(a.reserve(1001) && a.cap == 1001);  // reserve: exactly what was asked
    CHECK(CountMem::allocs == 4 && CountMem::frees == 3);
    CountMem::fail = true;
    CHECK(!a.grow(5000) && !a.p && a.cap == 0);  // frees first, stays empty
    CHECK(!a.reserve(1) && !a.p && a.cap == 0);
    CountMem::fail = false;
    CHECK(CountMem::frees == 4);
    CountBuf z;
    CHECK(z.grow(10, 0) && z.cap == 10);  // no floor
  }
  CHECK(CountMem::allocs == 5 && CountMem::frees == 5);
  {
    CountBuf a, b;
    CHECK(a.reserve(64) && b.reserve(32));
    void* pa = a.p;
    const int f0 = CountMem::frees;
    CountBuf c(std::move(a));  // move construction: nothing freed, the source empty
    CHECK(c.p == pa && c.cap == 64 && !a.p && a.cap == 0 && CountMem::frees == f0);
    b = std::move(c);  // move assignment: the destination's old allocation freed once
    CHECK(b.p == pa && b.cap == 64 && !c.p && c.cap == 0 && CountMem::frees == f0 + 1);
    CountBuf& self = b;
    b = std::move(self);  // self-assignment keeps the allocation
    CHECK(b.p == pa && CountMem::frees == f0 + 1);
  }
  CHECK(CountMem::allocs == 7 && CountMem::frees == 7);
}

template <class Buf>
static void check_hip_buf(const char* what) {
  Buf b;
  CHECK(!b.p && b.cap == 0);
  const bool ok = b.grow(1000, 4096);
  if (ok) {
    CHECK(b.p && b.cap >= 1000);
    void* p0 = b.p;
    CHECK(b.reserve(512) && b.p == p0 && b.grow(4096) && b.p == p0);
    Buf c(std::move(b));
    CHECK(!b.p && b.cap == 0 && c.p == p0);
    c.release();
    CHECK(!c.p && c.cap == 0);
  } else {
    CHECK(!b.p && b.cap == 0);
    CHECK(!b.reserve(64) && !b.p && b.cap == 0);
  }
  printf("owned_check: %s allocation %s\n", what, ok ? "succeeded" : "failed (no device): failure path checked");
}

static void check_handles() {
  Stream s;
  Event e;
  CHECK(!s && !e);  // empty: their destructors make no HIP call
  if (s.create() == hipSuccess) {
    CHECK((hipStream_t)s != nullptr);
    hipStream_t raw = s;
    Stream t(std::move(s));
    CHECK(!s && (hipStream_t)t == raw);
    CHECK(e.create(hipEventDisableTiming) == hipSuccess && (hipEvent_t)e != nullptr);
    Event f;
    f = std::move(e);
    CHECK(!e && (hipEvent_t)f != nullptr);
  } else {
    CHECK(!s);
  }
}

struct TestSlot {
  Stream stream;  // stays empty: the guard then skips the drain
  int published = 0;
};

static void check_ring() {
  constexpr int N = 3;
  SlotRing<TestSlot, N> ring;
  std::atomic<bool> locked_in_publish{false};
  auto publish = [&](TestSlot& sl) {
    sl.published++;
    // another thread cannot take the ring's lock while publish runs
    std::thread([&] {
      const bool got = ring.mu.try_lock();
      if (got) ring.mu.unlock();
      locked_in_publish = !got;
    }).join();
  };
  auto* g0 = new auto(ring.acquire(publish));
  auto* g1 = new auto(ring.acquire(publish));
  auto* g2 = new auto(ring.acquire(publish));
  CHECK(&g0->slot() != &g1->slot() && &g1->slot() != &g2->slot() && &g0->slot() != &g2->slot());
  std::atomic<bool> got{false};
  TestSlot* fourth = nullptr;
  std::thread waiter([&] {
    auto g = ring.acquire(publish);
    fourth = &g.slot();
    got = true;
  });
  std::this_thread::sleep_for(std::chrono::milliseconds(50));
  CHECK(!got);  // every slot busy: the fourth acquirer blocks
  TestSlot* freed = &g1->slot();
  delete g1;
  waiter.join();
  CHECK(got && fourth == freed);
  CHECK(locked_in_publish);
  CHECK(freed->published == 2);  // g1's guard, then the waiter's
  delete g0;
  delete g2;
  for (int j = 0; j < N; j++) CHECK(!ring.busy[j]);
}

int main() {
  check_counting();
  check_hip_buf<DevBuf>("device");
  check_hip_buf<PinBuf>("pinned");
  check_handles();
  check_ring();
  if (g_failed) {
    fprintf(stderr, "owned_check: %d check(s) failed\n", g_failed);
    return 1;
  }
  printf("owned_check: ok\n");
  return 0;
}
