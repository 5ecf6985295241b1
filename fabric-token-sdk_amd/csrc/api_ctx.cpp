// C-ABI (include/fts_gpu.h): context creation from the public parameters
// (setup.go:319-372) with its knobs and fixed-base tables, the multi-device
// layer, context information and the last run's timings.  Also the definitions
// shared by every unit of the library: the host pool and the timeline's names.
#include "host/api_internal.hpp"

namespace fts {
// "fb:" + nm, interned (Timeline marks after fallback())
const char* fallback_name(const char* nm) {
  static std::mutex mu;
  static std::deque<std::string> names;  // stable storage (deque never moves elements)
  std::lock_guard<std::mutex> g(mu);
  const std::string want = std::string("fb:") + nm;
  for (const std::string& x : names)
    if (x == want) return x.c_str();
  names.push_back(want);
  return names.back().c_str();
}
}  // namespace fts

namespace fts {
// the process's one host pool (host/host_pool.hpp)
HostPool& HostPool::get() {
  static HostPool* p = new HostPool();  // never destroyed: workers may outlive static destructors
  return *p;
}
void host_parallel_for(size_t n, const std::function<void(size_t)>& f) { parallel_for(n, 2, f); }
}  // namespace fts

// the process's one table cache (host/table_cache.hpp); never destroyed, like the host
// pool.  Its entries are owned by the contexts, not by it.
DevTableCache& table_cache() {
  static DevTableCache* t = new DevTableCache();
  return *t;
}

namespace fts {
namespace host {
void build_prover_tables(const PublicParams& pp, int n, ProverTables& t) {
  t.n = n;
  std::vector<G1A> bases;
  for (int i = 0; i < n; i++) bases.push_back(pp.left[i]);
  for (int i = 0; i < n; i++) bases.push_back(pp.right[i]);
  for (int i = 0; i < 3; i++) bases.push_back(pp.ped[i]);
  bases.push_back(pp.P);
  bases.push_back(pp.Q);
  t.fb.resize(bases.size());
  std::atomic<size_t> next{0};
  unsigned nth = host_threads();
  std::vector<std::thread> th;
  for (unsigned w = 0; w < nth; w++)
    th.emplace_back([&]() {
      for (size_t i; (i = next++) < bases.size();) t.fb[i].build(bases[i]);
    });
  for (auto& x : th) x.join();
}
}  // namespace host
}  // namespace fts

static int ctx_create(const uint8_t* pp_bytes, size_t pp_len, uint32_t bits, int device, fts_ctx** out,
                      const fts_ctx_opts* opts = nullptr) {
  if (!pp_bytes || !out) return FTS_API_EINVAL;
  *out = nullptr;
  std::unique_ptr<fts_ctx> c(new fts_ctx());  // released (on its device) by every failing exit
  std::string err;
  if (!parse_public_params(pp_bytes, pp_len, c->pp, err)) {
    fprintf(stderr, "fts_gpu: public parameters rejected: %s\n", err.c_str());
    return FTS_API_EPP;
  }
  if (bits) {
    if (bits > c->pp.bit_length || (bits & (bits - 1)) || bits < 2) return FTS_API_ESIZE;
    c->pp.left.resize(bits);
    c->pp.right.resize(bits);
    c->pp.bit_length = bits;
    c->pp.rounds = 63 - __builtin_clzll(bits);
    c->pp.max_token = bits == 64 ? ~0ULL : ((1ULL << bits) - 1);
    c->pp.precision = bits;
  }
  c->n = (int)c->pp.bit_length;
  c->k = (int)c->pp.rounds;
  if (device == FTS_DEVICE_NONE) {  // host-only context: parsing + prover, no GPU
    c->device = FTS_DEVICE_NONE;
    *out = c.release();
    return FTS_API_OK;
  }
  if (device < 0) {
    if (hipGetDevice(&device) != hipSuccess) device = 0;
  }
  c->device = device;
  if (hipSetDevice(device) != hipSuccess) return FTS_API_EDEVICE;
  int nl = 4;  // lanes (FTS_LANES): 4 beat 5 and 3 on the burst and the steady state (s20_sweep4.sh)
  if (const char* e = getenv("FTS_LANES")) nl = std::max(1, std::min(16, atoi(e)));
  if (opts && opts->lanes > 0) nl = std::min(16, opts->lanes);
  c->nlanes = nl;
  if (const char* e = getenv("FTS_COALESCE_MAX")) c->coalesce_max = (size_t)std::max(0L, atol(e));
  c->gather_target = c->coalesce_max / 2;
  if (const char* e = getenv("FTS_GATHER_TARGET")) c->gather_target = (size_t)std::max(1L, atol(e));
  if (const char* e = getenv("FTS_GATHER_US")) c->gather_us = std::max(0, atoi(e));
  if (const char* e = getenv("FTS_IDLE_GATHER_US")) c->idle_gather_us = std::max(0, atoi(e));
  if (const char* e = getenv("FTS_IDLE_QUIET_US")) c->idle_quiet_us = std::max(0, atoi(e));
  if (const char* e = getenv("FTS_IDLE_FIRST_US")) c->idle_first_us = std::max(0, atoi(e));
  if (const char* e = getenv("FTS_COM_FIXED_MAX")) c->com_fixed_max = (size_t)std::max(0L, atol(e));
  if (const char* e = getenv("FTS_RLC_FORK")) c->rlc_fork = std::max(0, std::min(4, atoi(e)));
  if (const char* e = getenv("FTS_X0_SPLIT")) c->x0_split = std::max(0, std::min(3, atoi(e)));
  if (const char* e = getenv("FTS_MSM_SORT")) c->msm_sort = atoi(e) != 0;
  if (const char* e = getenv("FTS_MAIN_GROUPS")) c->main_groups = atoi(e) != 0;
  if (const char* e = getenv("FTS_FX_SERIAL")) c->fx_serial = atoi(e) != 0;
  {  // process-wide, like the priority table: every context sets it (the last one wins)
    const char* e = getenv("FTS_WORK_BS");
    g_work_bs.store(e && atoi(e) == 256 ? 256 : 64, std::memory_order_relaxed);
  }
  if (const char* e = getenv("FTS_GT1")) c->gt1 = std::max(8, std::min(1024, atoi(e)));
  if (const char* e = getenv("FTS_GT2_MIN")) c->gt2_min = std::max(0, atoi(e));
  if (const char* e = getenv("FTS_GT_ADAPT")) c->gt_adapt = atoi(e) != 0;
  if (const char* e = getenv("FTS_LOCATE")) c->locate = atoi(e) != 0;
  if (const char* e = getenv("FTS_MSM_MAXC")) c->msm_maxc = std::max(8, std::min(16, atoi(e)));
  // FTS_WAVE_PRIO: one digit 0-3 per PrioSlot (device/wave_prio.hpp), e.g.
  // 022113313133; the table is per device and process: every context uploads its
  // own (the default without the variable), the last one created on a device wins
  {
    int pr[PS_N] = FTS_WAVE_PRIO_DEFAULT;
    if (const char* e = getenv("FTS_WAVE_PRIO"))
      for (int i = 0; i < PS_N && e[i]; i++)
        if (e[i] >= '0' && e[i] <= '3') pr[i] = e[i] - '0';
    if (set_wave_prio(pr) != hipSuccess) return FTS_API_EDEVICE;
  }
  // the batch check's stream (s3: RLC weights + MSM, the longest chain of a small
  // pass) gets the device's highest stream priority, so its few waves are
  // dispatched ahead of the exact phase's wide fixed-base launches
  int prio_lo = 0, prio_hi = 0;
  if (hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi) != hipSuccess) prio_lo = prio_hi = 0;
  for (int i = 0; i < nl; i++) {
    c->lanes.emplace_back(new Lane());
    c->lanes.back()->id = i;
    c->free_lanes.push_back(i);
    if (int rc = c->lanes.back()->create(prio_hi)) return rc;
  }
  hipStream_t s0 = c->lanes[0]->s;
  const int n = c->n;
  // fixed bases in table order (rp_kernels.hpp tb_*)
  std::vector<G1A> bases;
  for (int i = 0; i < n; i++) bases.push_back(c->pp.left[i]);
  for (int i = 0; i < n; i++) bases.push_back(c->pp.right[i]);
  bases.push_back(c->pp.ped[1]);
  bases.push_back(c->pp.ped[2]);
  bases.push_back(c->pp.P);
  bases.push_back(c->pp.Q);
  G1J K = jac_identity();
  for (int i = 0; i < n; i++) {
    K = jadd_aff(K, c->pp.right[i]);
    K = jadd_aff(K, aff_neg(c->pp.left[i]));
  }
  bases.push_back(to_aff(K));
  bases.push_back(c->pp.ped[0]);
  const int nb = (int)bases.size();
  std::vector<uint32_t> hb((size_t)nb * 16, 0);
  for (int b = 0; b < nb; b++)
    if (!bases[b].inf) {
      memcpy(&hb[b * 16], bases[b].x.v, 32);  // 4x64 LE == 8x32 LE Montgomery form
      memcpy(&hb[b * 16 + 8], bases[b].y.v, 32);
    }
  // The tables come from the device's table cache (host/table_cache.hpp, DESIGN.md
  // §4.1): built by this call only when no live context on the device has the same
  // bases at the same width.  FTS_TABLE_SHARE=0: private tables, as before the cache.
  bool share = true;
  if (const char* e = getenv("FTS_TABLE_SHARE")) share = atoi(e) != 0;
  DevTableCache& cache = table_cache();
  int build_rc = FTS_API_OK;  // why a build step failed (the cache reports only that it did)
  const auto take = [&](const TableKey& key, size_t bytes, const std::function<bool(void*)>& build, TableRef& ref) {
    bool built = true;
    ref.e = share ? cache.acquire(key, bytes, build, &built) : cache.make_private(key, bytes, build);
    ref.built = built;
    return ref.e != nullptr;
  };
  // A build step uploads the bases, fills the entry's buffer on s0 and drains s0 before
  // it returns: the entry is published (visible to other contexts' streams) only after
  // that host-side synchronisation, and the step's temporaries go after it too.
  c->table_bytes = (size_t)nb * fb_words_per_base() * 4;
  const auto build_narrow = [&](void* p) {
    DevBuf bases_buf, scr_buf;
    const int chunk = std::min(nb, 16);  // bases per build pass (bounds the Jacobian scratch)
    if (!bases_buf.reserve(hb.size() * 4) || !scr_buf.reserve(table_build_scratch_bytes(chunk))) {
      (void)hipGetLastError();
      build_rc = FTS_API_ENOMEM;
      return false;
    }
    uint32_t* const d_bases = bases_buf.as<uint32_t>();
    hipMemcpyAsync(d_bases, hb.data(), hb.size() * 4, hipMemcpyHostToDevice, s0);
    for (int b0 = 0; b0 < nb; b0 += chunk)
      launch_build_tables(d_bases + (size_t)b0 * 16, std::min(chunk, nb - b0),
                          static_cast<uint32_t*>(p) + (size_t)b0 * fb_words_per_base(), scr_buf.as<uint32_t>(), s0);
    if (hipStreamSynchronize(s0) != hipSuccess) {
      build_rc = FTS_API_EDEVICE;
      return false;
    }
    return true;
  };
  const int narrow_bits = 16;  // FB_W (device/fixed_base.hpp): the narrow set has one width
  if (!take(TableKey::of(device, narrow_bits, hb.data(), nb), c->table_bytes, build_narrow, c->d_tables))
    return build_rc != FTS_API_OK ? build_rc : FTS_API_ENOMEM;
  // wide tables of the per-proof bases H_i, K, P (same build, wider windows):
  // 22-bit windows (one mixed addition fewer per product: -8 % of the pass's
  // largest kernel) when the free HBM holds them with room to spare for the lanes'
  // workspace (~7 GB each at n = 64) and other contexts (160 GiB: at n = 64 only the
  // first context on an empty MI355X takes them); else, or when the allocation
  // fails, 20-bit
  {
    const int nw = n + 2;
    std::vector<uint32_t> hw((size_t)nw * 16, 0);
    for (int i = 0; i < nw; i++) {
      const int src = i < n ? n + i : (i == n ? 2 * n + 4 : 2 * n + 2);  // H_i, K, P in `bases`
      memcpy(&hw[(size_t)i * 16], &hb[(size_t)src * 16], 64);
    }
    // the wide key leaves the Pedersen generators out: public parameters that differ
    // only in them share this set
    const auto wide_key = [&](int wbits) { return TableKey::of(device, wbits, hw.data(), nw); };
    {
      // explicit width (fts_ctx_opts.wide_bits, else FTS_WIDE_BITS), else the budget:
      // 22-bit only when the whole context's tables fit the caller's table_budget
      // (fts_ctx_opts, counted against the bytes the context reads, shared or not) or,
      // without one, when a live context on the device already has (or is building)
      // these bases' 22-bit set -- sharing it costs nothing -- or when the free HBM
      // keeps every lane's workspace (~8 GiB each for 81,920-proof passes at n = 64)
      // and 128 GiB for other contexts and processes on the device
      int wb = 20, forced = 0;
      if (opts && (opts->wide_bits == 20 || opts->wide_bits == 22)) {
        wb = opts->wide_bits, forced = 1;
      } else if (const char* e = getenv("FTS_WIDE_BITS")) {
        wb = atoi(e) == 22 ? 22 : 20, forced = 1;
      } else {
        size_t fr = 0, tot = 0;
        const size_t need22 = (size_t)nw * fbw_words_per_base(22) * 4;
        if (opts && opts->table_budget) {
          if (c->table_bytes + need22 <= opts->table_budget) wb = 22;
        } else if (share && cache.has(wide_key(22))) {
          wb = 22;
        } else if (hipMemGetInfo(&fr, &tot) == hipSuccess &&
                   fr > need22 + (size_t)nl * ((size_t)8 << 30) + ((size_t)128 << 30)) {
          wb = 22;
        }
      }
      c->wbits = wb;
      c->wbits_forced = forced;
    }
    const auto build_wide = [&](void* p) {
      DevBuf wb_buf, wscr_buf;
      const int wchunk = std::min(nw, c->wbits == 22 ? 1 : 4);  // bounds the Jacobian build scratch (2.4 / 1.6 GB)
      if (!wb_buf.reserve(hw.size() * 4) || !wscr_buf.reserve(wide_build_scratch_bytes(wchunk, c->wbits))) {
        (void)hipGetLastError();
        build_rc = FTS_API_ENOMEM;
        return false;
      }
      uint32_t* const d_wb = wb_buf.as<uint32_t>();
      hipMemcpyAsync(d_wb, hw.data(), hw.size() * 4, hipMemcpyHostToDevice, s0);
      for (int b0 = 0; b0 < nw; b0 += wchunk)
        launch_build_wide_tables(d_wb + (size_t)b0 * 16, std::min(wchunk, nw - b0),
                                 static_cast<uint32_t*>(p) + (size_t)b0 * fbw_words_per_base(c->wbits),
                                 wscr_buf.as<uint32_t>(), s0, c->wbits);
      if (hipStreamSynchronize(s0) != hipSuccess) {
        build_rc = FTS_API_EDEVICE;
        return false;
      }
      return true;
    };
    for (;;) {  // 22-bit tables that do not fit after all (other contexts' lanes): 20-bit, which may be a hit
      build_rc = FTS_API_OK;
      if (take(wide_key(c->wbits), (size_t)nw * fbw_words_per_base(c->wbits) * 4, build_wide, c->d_wtables)) break;
      if (build_rc == FTS_API_EDEVICE) return FTS_API_EDEVICE;
      if (c->wbits == 22 && !c->wbits_forced) {
        c->wbits = 20;
        continue;
      }
      return FTS_API_ENOMEM;
    }
    c->table_bytes += (size_t)nw * fbw_words_per_base(c->wbits) * 4;
  }
  // constant part of the x0 transcript: hex(G_i) "||" ... hex(Q) "||"
  std::string xc;
  for (int i = 0; i <= n; i++) {
    uint8_t b[64];
    g1_to_bytes(i < n ? c->pp.left[i] : c->pp.Q, b);
    xc += hex_of(b, 64);
    xc += "||";
  }
  if (!c->d_x0const.reserve(xc.size())) return FTS_API_ENOMEM;
  hipMemcpyAsync(c->d_x0const.p, xc.data(), xc.size(), hipMemcpyHostToDevice, s0);
  // block-aligned template of the fully constant SHA-256 blocks of the x0 message
  std::string xt(64u * (x0_cb1(n) - x0_cb0(n)), '\0');
  for (size_t j = 0; j < xt.size(); j++) xt[j] = xc[64u * x0_cb0(n) + j - x0_const_off(n)];
  if (!c->d_x0tmpl.reserve(xt.size())) return FTS_API_ENOMEM;
  hipMemcpyAsync(c->d_x0tmpl.p, xt.data(), xt.size(), hipMemcpyHostToDevice, s0);
  hipError_t e = hipStreamSynchronize(s0);
  if (e != hipSuccess) {
    fprintf(stderr, "fts_gpu: table build failed: %s\n", hipGetErrorString(e));
    return FTS_API_EDEVICE;
  }
  *out = c.release();
  return FTS_API_OK;
}

// ------------------------------------------------------ multi-device layer
// A context over several devices (fts_ctx_create_devices / _mask) owns one
// child context per device -- its own lanes, streams and workspace, and the
// device's fixed-base tables (shared by the children on one device) -- and parses the public parameters itself as a host-only context
// (host provers, commitments).  Each batch entry point splits the caller's
// batch into contiguous shards balanced by a cost weight (fts_shard_plan),
// runs shard j on child j from its own host thread, and lets every child write
// its verdicts straight into the caller's arrays at the shard's offset: the
// verdicts come back in caller order.  The reference verifies every action
// independently (core/common/validator.go:215-224), so no data crosses devices;
// each device closes its own random-linear-combination check.
// The device provers, the commit call and the generators split the same way
// (over_devices): the parent checks the batch and makes the call's one RngSource,
// every child proves its slice at the items' indices in the caller's batch, and
// the parent packs once.
extern "C" int fts_shard_plan(size_t n, const double* weights, int nshards, size_t* bounds) {
  if (nshards < 1 || !bounds) return FTS_API_EINVAL;
  double tot = 0;
  for (size_t i = 0; i < n; i++) tot += weights ? std::max(0.0, weights[i]) : 1.0;
  bounds[0] = 0;
  size_t i = 0;
  double acc = 0;
  for (int j = 1; j < nshards; j++) {
    const double target = tot * j / nshards;
    // first index whose prefix weight reaches the target (never behind the previous cut)
    while (i < n && acc + (weights ? std::max(0.0, weights[i]) : 1.0) * 0.5 <= target) {
      acc += weights ? std::max(0.0, weights[i]) : 1.0;
      i++;
    }
    bounds[j] = i;
  }
  bounds[nshards] = n;
  return FTS_API_OK;
}

extern "C" {

int fts_ctx_create_devices(const uint8_t* pp, size_t pp_len, uint32_t bit_length, const int32_t* devices, int ndev,
                           fts_ctx** out) {
  if (!pp || !out || !devices || ndev < 1 || ndev > 64) return FTS_API_EINVAL;
  *out = nullptr;
  fts_ctx* c = nullptr;
  // the parent: parsed parameters, host-only (host provers / commitments run here)
  int rc = fts_ctx_create_bits(pp, pp_len, bit_length, FTS_DEVICE_NONE, &c);
  if (rc != FTS_API_OK) return rc;
  c->shards.assign(ndev, nullptr);
  std::vector<int> crc(ndev, FTS_API_OK);
  // tables of every device built concurrently; shards on one device build each key once
  // and wait for it (the table cache's single flight)
  std::vector<std::thread> th;
  for (int j = 0; j < ndev; j++)
    th.emplace_back([&, j]() { crc[j] = fts_ctx_create_bits(pp, pp_len, bit_length, devices[j], &c->shards[j]); });
  for (auto& t : th) t.join();
  for (int j = 0; j < ndev; j++)
    if (crc[j] != FTS_API_OK) rc = crc[j];
  if (rc != FTS_API_OK) {
    fts_ctx_destroy(c);
    return rc;
  }
  c->device = c->shards[0]->device;
  *out = c;
  return FTS_API_OK;
}

int fts_ctx_create_mask(const uint8_t* pp, size_t pp_len, uint32_t bit_length, uint64_t device_mask, fts_ctx** out) {
  std::vector<int32_t> devs;
  for (int d = 0; d < 64; d++)
    if ((device_mask >> d) & 1u) devs.push_back(d);
  if (devs.empty()) return FTS_API_EINVAL;
  return fts_ctx_create_devices(pp, pp_len, bit_length, devs.data(), (int)devs.size(), out);
}

int fts_ctx_devices(const fts_ctx* c, int32_t* devices, int cap) {
  if (!c) return 0;
  if (c->shards.empty()) {
    if (devices && cap > 0) devices[0] = c->device;
    return c->device == FTS_DEVICE_NONE ? 0 : 1;
  }
  for (int j = 0; j < (int)c->shards.size() && j < cap; j++)
    if (devices) devices[j] = c->shards[j]->device;
  return (int)c->shards.size();
}

}  // extern "C"

extern "C" {

int fts_ctx_create(const uint8_t* pp, size_t pp_len, int device, fts_ctx** out) {
  return ctx_create(pp, pp_len, 0, device, out);
}
int fts_ctx_create_opts(const uint8_t* pp, size_t pp_len, int device, const fts_ctx_opts* opts, fts_ctx** out) {
  return ctx_create(pp, pp_len, opts ? opts->bit_length : 0, device, out, opts);
}
int fts_ctx_create_bits(const uint8_t* pp, size_t pp_len, uint32_t bit_length, int device, fts_ctx** out) {
  return ctx_create(pp, pp_len, bit_length, device, out);
}

void fts_ctx_destroy(fts_ctx* c) { delete c; }

int fts_ctx_info(const fts_ctx* c, fts_pp_info* o) {
  if (!c || !o) return FTS_API_EINVAL;
  if (!c->shards.empty()) {  // device of shard 0; tables summed over the devices
    int rc = fts_ctx_info(c->shards[0], o);
    for (size_t j = 1; j < c->shards.size(); j++) o->table_bytes += c->shards[j]->table_bytes;
    return rc;
  }
  o->bit_length = (uint32_t)c->pp.bit_length;
  o->rounds = (uint32_t)c->pp.rounds;
  o->curve_id = (uint32_t)c->pp.curve_id;
  o->device = c->device;
  o->max_token = c->pp.max_token;
  o->table_bytes = c->table_bytes;
  o->wide_bits = (uint32_t)c->wbits;
  o->lanes = (uint32_t)c->nlanes;
  return FTS_API_OK;
}

int fts_ctx_table_info(const fts_ctx* c, int shard, fts_table_info* o) {
  if (!c || !o) return FTS_API_EINVAL;
  if (!c->shards.empty()) {
    if (shard < 0 || shard >= (int)c->shards.size()) return FTS_API_EINVAL;
    return fts_ctx_table_info(c->shards[shard], 0, o);
  }
  if (shard != 0 || !c->d_tables.e || !c->d_wtables.e) return FTS_API_EINVAL;  // host-only: no tables
  o->narrow_id = c->d_tables.e->id, o->wide_id = c->d_wtables.e->id;
  o->narrow_bytes = c->d_tables.e->bytes, o->wide_bytes = c->d_wtables.e->bytes;
  o->narrow_refs = DevTableCache::refs(c->d_tables.e), o->wide_refs = DevTableCache::refs(c->d_wtables.e);
  o->narrow_built = c->d_tables.built, o->wide_built = c->d_wtables.built;
  return FTS_API_OK;
}

// debug: entries T[w][d - 1] of one base's table as the device holds them (the tables
// are read-only once built, so the copies need no lane), 64-byte X||Y BE each
int fts_debug_table_entries(fts_ctx* c, int wide, int base, size_t count, const uint32_t* w, const uint32_t* d,
                            uint8_t* out64) {
  if (c && !c->shards.empty()) return fts_debug_table_entries(c->shards[0], wide, base, count, w, d, out64);
  if (!c || c->device < 0 || !c->d_tables.e || !c->d_wtables.e) return FTS_API_EINVAL;
  if (count && (!w || !d || !out64)) return FTS_API_EINVAL;
  const int bits = wide ? c->wbits : 16;
  const int nbases = wide ? c->n + 2 : 2 * c->n + 6;
  const size_t nw = (size_t)(255 + bits - 1) / bits, e = (size_t)1 << (bits - 1);
  const size_t per_base = wide ? fbw_words_per_base(bits) : fb_words_per_base();
  if (base < 0 || base >= nbases) return FTS_API_EINVAL;
  for (size_t j = 0; j < count; j++)
    if (w[j] >= nw || d[j] < 1 || d[j] > e) return FTS_API_EINVAL;
  const uint32_t* t = (wide ? c->d_wtables : c->d_tables).as<uint32_t>() + (size_t)base * per_base;
  HIP_OK(hipSetDevice(c->device));
  for (size_t j = 0; j < count; j++) {
    uint32_t m[16];
    HIP_OK(hipMemcpy(m, t + ((size_t)w[j] * e + d[j] - 1) * 16, 64, hipMemcpyDeviceToHost));
    G1A a{};
    memcpy(a.x.v, m, 32);  // 8x32 LE == 4x64 LE Montgomery form
    memcpy(a.y.v, m + 8, 32);
    a.inf = false;
    g1_to_bytes(a, out64 + 64 * j);
  }
  return FTS_API_OK;
}

int fts_debug_shard_work(const fts_ctx* c, int shard, int64_t out[4]) {
  if (!c || !out) return FTS_API_EINVAL;
  if (!c->shards.empty()) {
    if (shard < 0 || shard >= (int)c->shards.size()) return FTS_API_EINVAL;
    return fts_debug_shard_work(c->shards[shard], 0, out);
  }
  if (shard != 0 || c->device < 0) return FTS_API_EINVAL;  // host-only: no device work to count
  out[0] = c->st_pv_proofs, out[1] = c->st_pv_actions, out[2] = c->st_pv_tokens, out[3] = c->st_pv_passes;
  return FTS_API_OK;
}

int fts_debug_shard_timings(const fts_ctx* c, int shard, const char** names, float* ms, int cap) {
  if (!c || shard < 0) return 0;
  if (c->shards.empty()) return shard == 0 ? fts_last_timings_ex(c, names, ms, nullptr, cap) : 0;
  return shard < (int)c->shards.size() ? fts_last_timings_ex(c->shards[shard], names, ms, nullptr, cap) : 0;
}

int fts_table_cache_stats(int device, struct fts_table_cache_stats* o) {
  if (!o) return FTS_API_EINVAL;
  const TableCacheStats s = table_cache().stats(device);
  o->resident_bytes = s.resident_bytes;
  o->entries = s.entries;
  o->builds = s.builds, o->hits = s.hits;
  return FTS_API_OK;
}

const char* fts_status_str(int32_t s) {
  switch (s) {
    case FTS_OK: return "";
    case FTS_E_MALFORMED: return "failed to deserialize proof";
    case FTS_E_RP_NIL: return "invalid range proof: nil elements";
    case FTS_E_RP_INVALID: return "invalid range proof";
    case FTS_E_IPA_NIL: return "invalid IPA proof: nil elements";
    case FTS_E_IPA_LEN: return "invalid IPA proof";
    case FTS_E_IPA_INVALID: return "invalid IPA";
    case FTS_E_RC_COUNT: return "invalid range proof";
    case FTS_E_TAS_INVALID: return "invalid sum and type proof";
    case FTS_E_ST_INVALID: return "invalid same type proof";
    case FTS_E_NOT_RUN: return "not evaluated";
    case FTS_E_ACTION_INVALID: return "invalid action";
    case FTS_E_OPEN_MISMATCH: return "does not match the provided opening";
    case FTS_E_SIG_MALFORMED: return "asn1: signature does not deserialize";
    case FTS_E_SIG_NOT_LOW_S: return "signature is not in lowS";
    case FTS_E_SIG_INVALID: return "signature not valid";
    case FTS_E_NYM_MALFORMED: return "error unmarshalling signature";
    case FTS_E_NYM_BADKEY: return "failed importing nym public key";
    case FTS_E_NYM_INVALID: return "pseudonym signature invalid: zero-knowledge proof is invalid";
    case FTS_E_ID_MALFORMED: return "identity malformed";
    case FTS_E_ID_BADNYM: return "failed to import nym public key";
    case FTS_E_ID_NO_EIDNYM: return "no EidNym provided but ExpectEidNym required";
    case FTS_E_ID_NO_RHNYM: return "no RhNym provided but ExpectEidNymRhNym required";
    case FTS_E_ID_REVOCATION: return "unsupported revocation algorithm";
    case FTS_E_ID_APRIME: return "signature invalid: APrime = 1";
    case FTS_E_ID_PAIRING: return "signature invalid: APrime and ABar don't have the expected structure";
    case FTS_E_ID_ZK: return "signature invalid: zero-knowledge proof is invalid";
    case FTS_E_AUDIT_MALFORMED: return "could not deserialize the identity, its proof or the audit data";
    case FTS_E_AUDIT_NO_EIDNYM: return "error while verifying the nym eid: no EidNym provided";
    case FTS_E_AUDIT_EID_POINT: return "error while verifying the nym eid: invalid EidNym point";
    case FTS_E_AUDIT_EID_MISMATCH: return "error while verifying the nym eid: eid nym does not match";
    case FTS_E_AUDIT_NO_RHNYM: return "error while verifying the nym rh: no RhNym provided";
    case FTS_E_AUDIT_RH_POINT: return "error while verifying the nym rh: invalid RhNym point";
    case FTS_E_AUDIT_RH_MISMATCH: return "error while verifying the nym rh: rh nym does not match";
    case FTS_E_SIGN_BADKEY: return "signing key out of range";
    case FTS_E_CRED_MALFORMED: return "credential malformed";
    case FTS_E_CRED_B: return "b-value from credential does not match the attribute values";
    case FTS_E_CRED_PAIRING: return "credential is not cryptographically valid";
    case FTS_E_CREDREQ_MALFORMED: return "one of the proof values is undefined";
    case FTS_E_CREDREQ_INVALID: return "zero knowledge proof is invalid";
    case FTS_E_IPK_MALFORMED: return "issuer public key malformed";
    case FTS_E_IPK_UNDEFINED: return "some part of the public key is undefined";
    case FTS_E_IPK_PROOF: return "zero knowledge proof in public key invalid";
    default: return "unknown status";
  }
}

int fts_last_timings(const fts_ctx* c, const char** names, float* ms, int cap) {
  return fts_last_timings_ex(c, names, ms, nullptr, cap);
}

int fts_last_timings_ex(const fts_ctx* cc, const char** names, float* ms, double* mads, int cap) {
  if (!cc) return 0;
  if (!cc->shards.empty()) return fts_last_timings_ex(cc->shards[0], names, ms, mads, cap);
  fts_ctx* c = const_cast<fts_ctx*>(cc);
  std::lock_guard<std::mutex> g(c->tim_mu);
  return c->tim.copy_out(names, ms, mads, cap);
}

}  // extern "C"
