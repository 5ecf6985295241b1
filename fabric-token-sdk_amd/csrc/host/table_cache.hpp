// Process-wide cache of fixed-base tables, shared between the contexts of one
// device.  A table set is a pure function of its generator
// bytes, so contexts with the same bases read one device buffer instead of
// building and holding a copy each.
//
//   key        (device, window width, SHA-256 of the base array as uploaded)
//   single     the first creator of a key inserts a `building` entry, builds
//   flight     outside the cache's lock and publishes it; concurrent creators
//              of the same key wait and allocate nothing.  A failed build
//              removes the entry and wakes the waiters; the first of them to
//              find the key gone becomes the next builder.
//   lifetime   every user holds a std::shared_ptr to the entry, the cache only
//              a weak one: the last user to let go frees the buffer, and the
//              cache keeps nothing alive by itself.
//   read-only  a published entry is never written again.
//
// The cache makes no HIP call of its own: `Policy` allocates and frees
//   static void* Policy::alloc(int device, size_t bytes);   // nullptr: failed
//   static void  Policy::free(int device, void* p);
// and the caller of acquire() passes the build step (bool build(void* p):
// fill p, drain the work, true on success).  tools/table_cache_check.cpp runs
// it over host memory.
#pragma once
#include <stdint.h>
#include <string.h>
#include <atomic>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>

#include "../common/sha256.hpp"

namespace fts {

struct TableKey {
  int device = 0;
  int width = 0;  // window bits of the table set
  uint8_t digest[32] = {};
  // key of the table set of `nbases` bases, 64 bytes each, exactly as uploaded
  static TableKey of(int device, int width, const void* bases, size_t nbases) {
    TableKey k;
    k.device = device, k.width = width;
    sha256(static_cast<const uint8_t*>(bases), nbases * 64, k.digest);
    return k;
  }
  bool operator<(const TableKey& o) const {
    if (device != o.device) return device < o.device;
    if (width != o.width) return width < o.width;
    return memcmp(digest, o.digest, 32) < 0;
  }
};

struct TableCacheStats {
  uint64_t resident_bytes = 0;  // bytes of the device's published entries
  uint32_t entries = 0;         // their number
  uint64_t builds = 0, hits = 0;  // since process start
};

template <class Policy>
class TableCache {
 public:
  struct Entry {
    TableKey key;
    uint64_t id = 0;  // unique in the process: equal ids = the same buffer
    void* p = nullptr;
    size_t bytes = 0;
    template <class T>
    const T* as() const {
      return reinterpret_cast<const T*>(p);
    }

   private:
    friend class TableCache;
    enum State { BUILDING, READY, FAILED };
    State state = BUILDING;     // under the cache's lock
    TableCache* cache = nullptr;  // null: private (never in the map)
  };
  using Ref = std::shared_ptr<const Entry>;

  // The entry of `key`: found ready (after waiting for its builder, if one is at
  // work), or allocated and built by this call.  *built tells which.  Null when
  // this call's own allocation or build failed; nothing is left behind then.
  template <class Build>
  Ref acquire(const TableKey& key, size_t bytes, Build&& build, bool* built) {
    if (built) *built = false;
    std::shared_ptr<Entry> mine;
    {
      std::unique_lock<std::mutex> lk(mu_);
      for (;;) {
        auto it = map_.find(key);
        if (it != map_.end()) {
          if (std::shared_ptr<Entry> e = it->second.lock()) {
            if (e->state == Entry::READY) {
              dev_[key.device].hits++;
              return e;
            }
            // building: its builder holds it, so letting go here frees nothing
            e.reset();
            cv_.wait(lk);
            continue;
          }
          map_.erase(it);  // its last user is letting go right now
        }
        mine = make_entry(key, this);
        map_[key] = mine;
        break;
      }
    }
    void* p = Policy::alloc(key.device, bytes);
    const bool ok = p && build(p);
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (ok) {
        mine->p = p, mine->bytes = bytes;
        mine->state = Entry::READY;
        TableCacheStats& s = dev_[key.device];
        s.resident_bytes += bytes, s.entries++, s.builds++;
      } else {
        mine->state = Entry::FAILED;
        map_.erase(key);  // still this entry: nobody replaces a live one
      }
    }
    cv_.notify_all();
    if (!ok) {
      if (p) Policy::free(key.device, p);
      return nullptr;  // `mine` goes outside the lock
    }
    if (built) *built = true;
    return mine;
  }

  // A table set of one user alone: never in the map, not counted in the stats.
  template <class Build>
  Ref make_private(const TableKey& key, size_t bytes, Build&& build) {
    std::shared_ptr<Entry> e = make_entry(key, nullptr);
    void* p = Policy::alloc(key.device, bytes);
    if (!p) return nullptr;
    if (!build(p)) {
      Policy::free(key.device, p);
      return nullptr;
    }
    e->p = p, e->bytes = bytes, e->state = Entry::READY;
    return e;
  }

  // a ready or building entry of `key` exists
  bool has(const TableKey& key) {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = map_.find(key);
    return it != map_.end() && !it->second.expired();
  }

  TableCacheStats stats(int device) {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = dev_.find(device);
    return it == dev_.end() ? TableCacheStats() : it->second;
  }

  // users holding the entry now
  static uint32_t refs(const Ref& r) { return r ? (uint32_t)r.use_count() : 0; }

 private:
  static std::shared_ptr<Entry> make_entry(const TableKey& key, TableCache* cache) {
    static std::atomic<uint64_t> next_id{1};
    Entry* e = new Entry();
    e->key = key, e->cache = cache;
    e->id = next_id.fetch_add(1, std::memory_order_relaxed);
    return std::shared_ptr<Entry>(e, &TableCache::drop);
  }
  // the last user let go: out of the books first, then the buffer
  static void drop(Entry* e) {
    if (e->cache && e->state == Entry::READY) {
      TableCache& c = *e->cache;
      std::lock_guard<std::mutex> lk(c.mu_);
      TableCacheStats& s = c.dev_[e->key.device];
      s.resident_bytes -= e->bytes, s.entries--;
      auto it = c.map_.find(e->key);
      if (it != c.map_.end() && it->second.expired()) c.map_.erase(it);  // not a successor's
    }
    if (e->p) Policy::free(e->key.device, e->p);
    delete e;
  }

  std::mutex mu_;
  std::condition_variable cv_;
  std::map<TableKey, std::weak_ptr<Entry>> map_;
  std::map<int, TableCacheStats> dev_;
};

}  // namespace fts
