// Stand-alone check of host/table_cache.hpp over host memory (no HIP call, no
// device): single flight, failed builds, release order, private entries and
// concurrent builds of distinct keys.  Built with the host address / undefined-
// behaviour sanitizers, so a double free, a leak or a read of a freed table
// aborts it.  Exit status 0 iff every check holds.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../host/table_cache.hpp"

using namespace fts;

static std::atomic<int> g_failed{0};
#define CHECK(x)                                                        \
  do {                                                                  \
    if (!(x)) {                                                         \
      fprintf(stderr, "table_cache_check: %s (line %d)\n", #x, __LINE__); \
      g_failed++;                                                       \
    }                                                                   \
  } while (0)

// host memory that counts: what a device policy does with hipMalloc / hipFree
struct HostMem {
  static std::atomic<int> allocs, frees, last_free_device;
  static std::atomic<bool> fail;
  static void* alloc(int device, size_t bytes) {
    if (fail) return nullptr;
    allocs++;
    return malloc(bytes);
  }
  static void free(int device, void* p) {
    frees++;
    last_free_device = device;
    ::free(p);
  }
};
std::atomic<int> HostMem::allocs{0}, HostMem::frees{0}, HostMem::last_free_device{-1};
std::atomic<bool> HostMem::fail{false};
using Cache = TableCache<HostMem>;

static const size_t BYTES = 1 << 16;

static TableKey key_of(int device, int width, uint8_t tag) {
  uint8_t bases[3 * 64];
  for (size_t i = 0; i < sizeof bases; i++) bases[i] = (uint8_t)(tag + i);
  return TableKey::of(device, width, bases, 3);
}
static void fill(void* p, uint8_t tag) { memset(p, tag, BYTES); }
static bool filled(const Cache::Ref& r, uint8_t tag) {
  if (!r || !r->p || r->bytes != BYTES) return false;
  for (size_t i = 0; i < BYTES; i++)
    if (r->as<uint8_t>()[i] != tag) return false;
  return true;
}
static void nap(int ms) { std::this_thread::sleep_for(std::chrono::milliseconds(ms)); }

// every thread of a test has reached its acquire() before a build ends
struct Gate {
  std::atomic<int> arrived{0};
  void arrive() { arrived++; }
  void wait_for(int n) {
    while (arrived < n) std::this_thread::yield();
    nap(20);  // ... and has had the time to find the entry building
  }
};

// 16 threads, one key: one build, 15 hits, one buffer, all see the built contents
static void check_single_flight() {
  Cache c;
  const TableKey k = key_of(0, 16, 1);
  const int T = 16;
  std::atomic<int> builds{0};
  Gate gate;
  std::vector<Cache::Ref> refs(T);
  std::vector<char> built(T, 0);
  const int a0 = HostMem::allocs;
  std::vector<std::thread> th;
  for (int t = 0; t < T; t++)
    th.emplace_back([&, t]() {
      bool b = false;
      gate.arrive();
      refs[t] = c.acquire(
          k, BYTES,
          [&](void* p) {
            builds++;
            gate.wait_for(T);
            fill(p, 0xA1);
            return true;
          },
          &b);
      built[t] = b;
    });
  for (auto& x : th) x.join();
  int nbuilt = 0;
  for (int t = 0; t < T; t++) {
    nbuilt += built[t];
    CHECK(filled(refs[t], 0xA1));
    CHECK(refs[t] && refs[t]->id == refs[0]->id && refs[t]->p == refs[0]->p);
  }
  CHECK(builds == 1 && nbuilt == 1 && HostMem::allocs - a0 == 1);
  TableCacheStats s = c.stats(0);
  CHECK(s.builds == 1 && s.hits == (uint64_t)T - 1 && s.entries == 1 && s.resident_bytes == BYTES);
  CHECK(Cache::refs(refs[0]) == (uint32_t)T && c.has(k));
  CHECK(c.stats(1).entries == 0 && c.stats(1).builds == 0);  // per device
  const int f0 = HostMem::frees;
  for (int t = 0; t < T - 1; t++) refs[t].reset();
  CHECK(HostMem::frees == f0 && filled(refs[T - 1], 0xA1));  // the last user still reads it
  refs[T - 1].reset();
  s = c.stats(0);
  CHECK(HostMem::frees == f0 + 1 && s.entries == 0 && s.resident_bytes == 0 && !c.has(k));
  CHECK(s.builds == 1 && s.hits == (uint64_t)T - 1);  // counters are since the start
}

// the first build fails with waiters queued: they are woken, exactly one of them builds
// again, and nobody is handed an entry that was not built
static void check_failed_build() {
  Cache c;
  const TableKey k = key_of(0, 20, 2);
  const int T = 8;
  std::atomic<int> attempts{0};
  Gate gate;
  std::vector<Cache::Ref> refs(T);
  std::vector<char> built(T, 0);
  const int a0 = HostMem::allocs, f0 = HostMem::frees;
  std::vector<std::thread> th;
  for (int t = 0; t < T; t++)
    th.emplace_back([&, t]() {
      bool b = false;
      gate.arrive();
      refs[t] = c.acquire(
          k, BYTES,
          [&](void* p) {
            const int a = attempts++;
            gate.wait_for(T);
            if (a == 0) return false;  // half-written: must never be seen
            fill(p, 0xB2);
            return true;
          },
          &b);
      built[t] = b;
    });
  for (auto& x : th) x.join();
  int nnull = 0, nbuilt = 0;
  uint64_t id = 0;
  for (int t = 0; t < T; t++) {
    if (!refs[t]) {
      nnull++;
      CHECK(!built[t]);
      continue;
    }
    nbuilt += built[t];
    CHECK(filled(refs[t], 0xB2));
    CHECK(id == 0 || refs[t]->id == id);
    id = refs[t]->id;
  }
  CHECK(attempts == 2 && nnull == 1 && nbuilt == 1);
  CHECK(HostMem::allocs - a0 == 2 && HostMem::frees - f0 == 1);  // the failed buffer went at once
  TableCacheStats s = c.stats(0);
  CHECK(s.builds == 1 && s.hits == (uint64_t)T - 2 && s.entries == 1 && s.resident_bytes == BYTES);
  for (auto& r : refs) r.reset();
  CHECK(HostMem::frees - f0 == 2 && c.stats(0).entries == 0 && c.stats(0).resident_bytes == 0);
  // a failed allocation: nothing is built, nothing stays behind, the next call builds
  HostMem::fail = true;
  bool b = true, ran = false;
  Cache::Ref r = c.acquire(k, BYTES, [&](void*) { return ran = true; }, &b);
  CHECK(!r && !b && !ran && !c.has(k) && c.stats(0).entries == 0);
  CHECK(!c.make_private(k, BYTES, [&](void*) { return ran = true; }) && !ran);
  HostMem::fail = false;
  r = c.acquire(k, BYTES, [&](void* p) { return fill(p, 0xB3), true; }, &b);
  CHECK(b && filled(r, 0xB3) && c.stats(0).builds == 2);
}

// builder first, builder last: the table lives until the last user lets go, is
// freed exactly once (on its device), and the books return to zero
static void check_release_order(bool builder_first) {
  Cache c;
  const TableKey k = key_of(3, 22, 4);
  bool ba = false, bb = true;
  const int f0 = HostMem::frees;
  Cache::Ref a = c.acquire(k, BYTES, [&](void* p) { return fill(p, 0xC3), true; }, &ba);
  int second_builds = 0;
  Cache::Ref b = c.acquire(k, BYTES, [&](void*) { return second_builds++, false; }, &bb);
  CHECK(second_builds == 0);
  CHECK(ba && !bb && a && b && a->id == b->id && Cache::refs(a) == 2 && Cache::refs(b) == 2);
  (builder_first ? a : b).reset();
  Cache::Ref& rest = builder_first ? b : a;
  CHECK(HostMem::frees == f0 && filled(rest, 0xC3) && Cache::refs(rest) == 1);
  CHECK(c.stats(3).entries == 1 && c.stats(3).resident_bytes == BYTES && c.has(k));
  rest.reset();
  CHECK(HostMem::frees == f0 + 1 && HostMem::last_free_device == 3);
  CHECK(c.stats(3).entries == 0 && c.stats(3).resident_bytes == 0 && !c.has(k));
  // nothing is kept alive: the same key builds again, under a new id
  Cache::Ref again = c.acquire(k, BYTES, [&](void* p) { return fill(p, 0xC4), true; }, &ba);
  CHECK(ba && filled(again, 0xC4) && c.stats(3).builds == 2 && c.stats(3).hits == 1);
}

// keys differ by device, width and bases; private entries stay out of the books
static void check_keys_and_private() {
  Cache c;
  const TableKey k = key_of(0, 20, 5);
  std::vector<Cache::Ref> r;
  for (const TableKey& q : {k, key_of(1, 20, 5), key_of(0, 22, 5), key_of(0, 20, 6)}) {
    bool b = false;
    r.push_back(c.acquire(q, BYTES, [&](void* p) { return fill(p, 0xD5), true; }, &b));
    CHECK(b && r.back());
  }
  for (size_t i = 0; i < r.size(); i++)
    for (size_t j = i + 1; j < r.size(); j++) CHECK(r[i]->id != r[j]->id && r[i]->p != r[j]->p);
  CHECK(c.stats(0).entries == 3 && c.stats(1).entries == 1 && c.stats(0).resident_bytes == 3 * BYTES);
  const TableCacheStats s0 = c.stats(0);
  const int f0 = HostMem::frees;
  Cache::Ref p1 = c.make_private(k, BYTES, [&](void* p) { return fill(p, 0xD6), true; });
  Cache::Ref p2 = c.make_private(k, BYTES, [&](void* p) { return fill(p, 0xD7), true; });
  CHECK(filled(p1, 0xD6) && filled(p2, 0xD7) && filled(r[0], 0xD5));
  CHECK(p1->id != p2->id && p1->id != r[0]->id && p1->p != r[0]->p && Cache::refs(p1) == 1);
  const TableCacheStats s1 = c.stats(0);
  CHECK(s1.entries == s0.entries && s1.resident_bytes == s0.resident_bytes && s1.builds == s0.builds && s1.hits == s0.hits);
  p1.reset();
  p2.reset();
  CHECK(HostMem::frees == f0 + 2 && c.stats(0).entries == 3 && c.has(k) && filled(r[0], 0xD5));
}

// two keys build at the same time: each build waits (bounded) for the other to have
// started, which a cache that serialised builds could never satisfy
static void check_concurrent_keys() {
  Cache c;
  std::atomic<int> started{0};
  std::atomic<bool> overlapped[2] = {{false}, {false}};
  Cache::Ref r[2];
  std::vector<std::thread> th;
  for (int t = 0; t < 2; t++)
    th.emplace_back([&, t]() {
      bool b = false;
      r[t] = c.acquire(
          key_of(0, 20, (uint8_t)(7 + t)), BYTES,
          [&](void* p) {
            started++;
            const auto until = std::chrono::steady_clock::now() + std::chrono::seconds(10);
            while (started < 2 && std::chrono::steady_clock::now() < until) std::this_thread::yield();
            overlapped[t] = started == 2;
            fill(p, (uint8_t)(0xE0 + t));
            return true;
          },
          &b);
      CHECK(b);
    });
  for (auto& x : th) x.join();
  CHECK(overlapped[0] && overlapped[1]);
  CHECK(filled(r[0], 0xE0) && filled(r[1], 0xE1) && c.stats(0).builds == 2 && c.stats(0).hits == 0);
}

int main() {
  check_single_flight();
  check_failed_build();
  check_release_order(true);
  check_release_order(false);
  check_keys_and_private();
  check_concurrent_keys();
  CHECK(HostMem::allocs == HostMem::frees);  // every cache above is gone: so is every table
  if (g_failed) {
    fprintf(stderr, "table_cache_check: %d check(s) failed\n", g_failed.load());
    return 1;
  }
  printf("table_cache_check: ok\n");
  return 0;
}
