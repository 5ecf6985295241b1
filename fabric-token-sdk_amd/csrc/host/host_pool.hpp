// The process's host worker pool for the batch loops (DER parsing, staging,
// signature packing) and the host clock of the phase timings.  The pool
// singleton is defined once, in api_ctx.cpp: one pool per process.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>

namespace fts {

// host worker threads for batch parsing: the CPUs this process may actually
// use (cgroup v2 cpu.max quota, else the hardware count), at most 16
inline unsigned host_threads() {
  static const unsigned n = [] {
    unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
      char q[32] = {0};
      long long period = 0;
      if (fscanf(f, "%31s %lld", q, &period) == 2 && strcmp(q, "max") != 0 && period > 0)
        hw = std::min<unsigned>(hw, (unsigned)std::max(1LL, atoll(q) / period));
      fclose(f);
    }
    return std::min(16u, hw);
  }();
  return n;
}

// Fork-join pool of host_threads() - 1 persistent workers for the host loops
// (DER parsing, staging): spawning host_threads() std::threads per loop cost
// ~0.5 ms per loop, twice per action call, with several calls in flight.
// Every caller works on its own job too, so concurrent callers always progress.
class HostPool {
 public:
  static HostPool& get();  // the process's pool (api_ctx.cpp); never destroyed: workers may outlive static destructors
  void run(size_t n, const std::function<void(size_t)>& f) {
    auto j = std::make_shared<Job>();
    j->n = n;
    j->f = &f;
    // items are claimed in chunks: one atomic claim and one completion count per
    // chunk, not per item (per-item counters bounced one cache line between every
    // worker: ~0.8 us of overhead per parsed action with 8 threads)
    j->grain = std::max<size_t>(1, std::min<size_t>(32, n / (8 * (size_t)host_threads())));
    {
      std::lock_guard<std::mutex> l(mu_);
      q_.push_back(j);
    }
    cv_.notify_all();
    work(*j);
    std::unique_lock<std::mutex> l(j->m);
    j->cv.wait(l, [&] { return j->done.load() == j->n; });
  }

 private:
  struct Job {
    size_t n = 0, grain = 1;
    const std::function<void(size_t)>* f = nullptr;
    std::atomic<size_t> next{0}, done{0};
    std::mutex m;
    std::condition_variable cv;
  };
  HostPool() {
    const unsigned nw = host_threads() > 1 ? host_threads() - 1 : 0;
    for (unsigned t = 0; t < nw; t++) std::thread([this] { loop(); }).detach();
  }
  static void work(Job& j) {
    for (size_t i0; (i0 = j.next.fetch_add(j.grain)) < j.n;) {
      const size_t i1 = std::min(j.n, i0 + j.grain);
      for (size_t i = i0; i < i1; i++) (*j.f)(i);
      if ((j.done += i1 - i0) == j.n) {
        std::lock_guard<std::mutex> l(j.m);
        j.cv.notify_all();
      }
    }
  }
  void loop() {
    for (;;) {
      std::shared_ptr<Job> j;
      {
        std::unique_lock<std::mutex> l(mu_);
        cv_.wait(l, [&] { return !q_.empty(); });
        j = q_.front();
        if (j->next.load() >= j->n) {  // exhausted: drop it and look again
          q_.pop_front();
          continue;
        }
      }
      work(*j);
    }
  }
  std::mutex mu_;
  std::condition_variable cv_;
  std::deque<std::shared_ptr<Job>> q_;
};

// run f(i) for i in [0, n) on the host pool (inline when small)
template <class F>
void parallel_for(size_t n, size_t min_parallel, F&& f) {
  if (n < min_parallel || host_threads() <= 1) {
    for (size_t i = 0; i < n; i++) f(i);
    return;
  }
  const std::function<void(size_t)> fn = std::ref(f);
  HostPool::get().run(n, fn);
}
// the same pool for the signature batches' packing loops (ecdsa_kernels.hip,
// api_idemix.cpp)
void host_parallel_for(size_t n, const std::function<void(size_t)>& f);

inline double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace fts
