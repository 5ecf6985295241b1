// Shared by the units of the C-ABI (include/fts_gpu.h): api_ctx.cpp (contexts,
// multi-device layer), api_rp.cpp (range-proof passes and their dispatcher),
// api_msm.cpp, api_actions.cpp (transfers / issues / requests), api_prove.cpp,
// api_generate.cpp and api_audit.cpp.
//
// Host side of the drop-in boundary: context creation from the public
// parameters (setup.go:319-372), DER decoding of proofs into device records,
// orchestration of the HIP kernels in the rp_*.hip units / sigma_kernels.hip, and
// the reference error-precedence rules (transfer.go:153-197,
// issue/verifier.go:32-57, rangecorrectness.go:137-162).
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <chrono>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <sys/random.h>
#include <vector>

#include "../../../include/fts_gpu.h"
#include "../device/launch.hpp"
#include "../device/rp_kernels.hpp"
#include "../device/sigma.hpp"
#include "../device/prove.hpp"
#include "../device/wave_prio.hpp"
#include "action_stage.hpp"
#include "bn254_host.hpp"
#include "der.hpp"
#include "hip_owned.hpp"
#include "host_pool.hpp"
#include "pp_parse.hpp"
#include "request_parse.hpp"
#include "table_cache.hpp"
#include "proofs.hpp"
#include "prover.hpp"

// internal to the API units, which are written in these namespaces
using namespace fts;
using namespace fts::host;

#define HIP_OK(x)                                                                         \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) {                                                               \
      fprintf(stderr, "fts_gpu: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
      return FTS_API_EDEVICE;                                                             \
    }                                                                                     \
  } while (0)

namespace fts {
namespace host {

struct Workspace {
  DevBuf pts, ch, small, hpj, hpa, hpbe, x0, x0mid, terms, scratch, ypow, svec, zvec, rp_excl;
  // random-linear-combination check + MSM
  DevBuf r_key, r_msc, r_coef, r_colsum, r_fixed, r_flag, r_gcol, r_gfix, r_sel, r_next, r_cnt, m_keys,
      m_counts, m_offsets, m_cursor, m_sorted, m_buckets, m_segs, m_wins, m_out, m_scratch, m_win, m_choff, m_chbkt, m_partials;
  DevBuf r_msel, r_mcol, r_mfix, r_mqfix, r_mflag;  // the per-caller-batch combination of a coalesced pass
  DevBuf r_loc, r_save;  // the single-fault locator: located proof, the failed combination S
  // action (transfer / issue) batches
  DevBuf rp_raw, rp_sc, rp_status, rp_ipa;
  DevBuf s_act, s_raw, s_owner, s_pts, s_sc, s_status, s_work, s_terms, s_aff, s_affoff, s_msgs, s_jac, s_scratch;
  DevBuf open_rec;  // token opening checks: [raw n*64][scalars n*96][status n*4]
  DevBuf pv;        // batched prover: one arena (prove_arena)
  DevBuf sp;        // sigma provers: one arena
};

// timings of one run: kernel spans (with their algorithmic work, in products) and
// host phases
struct TimingRecord {
  int n = 0;
  const char* name[Timeline::CAP];
  float ms[Timeline::CAP];
  double work[Timeline::CAP];
  void add(const char* nm, float t, double w) {
    if (n >= Timeline::CAP) return;
    name[n] = nm, ms[n] = t, work[n] = w;
    n++;
  }
  // the named marks of a finished timeline (fork/join markers skipped)
  void add_marks(const Timeline& tl) {
    for (int i = 0; i < tl.n && n < Timeline::CAP; i++) {
      if (!tl.name[i]) continue;
      const int j = n++;
      name[j] = tl.name[i];
      work[j] = tl.work[i];
      hipEventElapsedTime(&ms[j], tl.ev[tl.start[i]], tl.ev[i + 1]);
    }
  }
  int copy_out(const char** names, float* ms_out, double* mads, int cap) const {
    const int m = std::min(cap, n);
    for (int i = 0; i < m; i++) {
      if (names) names[i] = name[i];
      if (ms_out) ms_out[i] = ms[i];
      if (mads) mads[i] = work[i] * MADS_PER_MUL;
    }
    return m;
  }
};

}  // namespace host
}  // namespace fts

// One execution lane: a main + side stream pair with its own workspace and
// timeline.  Independent batches submitted concurrently (e.g. by the Go shim's
// aggregation goroutines, or bench.py's pipeline) run on different lanes, so
// one batch's latency-bound phases (transcript hashing, doubling chains)
// overlap another batch's throughput-bound kernels.

// pinned window-table slots of Lane::Pinned (msm_prepare_plan)
enum { MSM_SLOT_PASS = 0, MSM_SLOT_RESERVE, MSM_SLOT_GT_BIG, MSM_SLOT_GT_SMALL, MSM_WIN_SLOTS };

struct Lane {
  int id = 0;
  // completion event created with hipEventBlockingSync: waiting on it sleeps
  // instead of spinning (a spinning waiter per lane burns the process's CPU
  // quota; on a CFS-throttled box that stalls every host thread for ~50 ms
  // out of each 100 ms period)
  Event done;
  hipError_t sync() {
    hipError_t e = hipEventRecord(done, s);
    return e == hipSuccess ? hipEventSynchronize(done) : e;
  }
  bool presized = false;  // workspace sized for the context's largest coalesced pass
  // no other pass was running when the current one started (set by the dispatchers):
  // only then does a small pass take the latency path (k_rp_fixed_all), which does
  // more total work than the work path and pays off only on an otherwise idle device
  bool alone = true;
  Stream s, s2;
  Stream s3;  // sigma proofs of action batches (beside the range-proof pass)
  Stream s4;  // the batch check's x0-free columns beside its MSM
  Event ev_a, ev_b, ev_c, ev_d, ev_e;  // cross-stream ordering (no timing)
  Workspace ws;
  Timeline tl;
  float host_prep_ms = 0, host_enqueue_ms = 0, host_wait_ms = 0;  // host wall time of the last run
  float host_parse_ms = 0, host_stage_ms = 0;  // action batches: DER parsing, assembly + upload
  float host_misc_ms = 0, host_total_ms = 0, host_stage_copy_ms = 0;  // action batches: allocation before the parse + verdict assembly / release after the wait
  // pinned host staging (pageable async copies would block the enqueue)
  struct Pinned {
    uint32_t key[8];
    // window tables of the MSM plans uploaded between two syncs of the lane
    // (msm_prepare_plan's `slot`): the group test uploads two plans back to
    // back, and one shared pinned source let the second memcpy overwrite the
    // first before its DMA ran
    MsmWindow win[MSM_WIN_SLOTS][MSM_MAX_WINDOWS];
    int32_t flag;
    int32_t gflag[RP_GATHER_MAX];  // per caller batch of a grouped pass: its combination closed
  }* pin = nullptr;  // view of pin_mem
  PinBuf pin_mem, pin_status;
  int32_t* status_buf(size_t n) {
    return pin_status.reserve(std::max<size_t>(n, 4096) * 4) ? pin_status.as<int32_t>() : nullptr;
  }
  // action batches: pinned staging of the assembled sigma / range-proof inputs
  PinBuf stage;
  uint8_t* stage_buf(size_t bytes) { return stage.grow(bytes, 1 << 20) ? stage.as<uint8_t>() : nullptr; }
  // pinned source of the per-caller-batch slot map (its own buffer: `stage` may still
  // be the source of an action batch's pending uploads)
  PinBuf pin_sel;
  int32_t* sel_buf(size_t n) {
    return pin_sel.reserve(std::max<size_t>(n, 1 << 16) * 4) ? pin_sel.as<int32_t>() : nullptr;
  }
  // streams, completion event, pinned block and timeline; FTS_API_OK or the error
  int create(int prio_hi) {
    if (s.create() != hipSuccess || done.create(hipEventBlockingSync | hipEventDisableTiming) != hipSuccess)
      return FTS_API_EDEVICE;
    if (!pin_mem.reserve(sizeof(Pinned))) return FTS_API_ENOMEM;
    pin = pin_mem.as<Pinned>();
    if (s2.create() != hipSuccess || s4.create() != hipSuccess || s3.create(prio_hi) != hipSuccess) return FTS_API_EDEVICE;
    for (Event* e : {&ev_a, &ev_b, &ev_c, &ev_d, &ev_e})
      if (e->create(hipEventDisableTiming) != hipSuccess) return FTS_API_EDEVICE;
    tl.create();
    return FTS_API_OK;
  }
  Lane() = default;
  // drains the lane's streams before any member (workspace, pinned buffers) is released
  ~Lane() {
    for (hipStream_t x : {(hipStream_t)s, (hipStream_t)s2, (hipStream_t)s4, (hipStream_t)s3})
      if (x) hipStreamSynchronize(x);
    tl.destroy();
  }
};

// Device policy of the table cache: the entry's device is made current before its
// buffer is allocated or freed (the last context to let go may run anywhere).
struct DevTableMem {
  static void* alloc(int device, size_t bytes) {
    void* p = nullptr;
    if (hipSetDevice(device) != hipSuccess || hipMalloc(&p, bytes) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    return p;
  }
  static void free(int device, void* p) {
    (void)hipSetDevice(device);
    (void)hipFree(p);
  }
};
using DevTableCache = TableCache<DevTableMem>;
// the process's one table cache [api_ctx.cpp]
DevTableCache& table_cache();

// a context's reference to one table set
struct TableRef {
  DevTableCache::Ref e;
  bool built = false;  // this context's creation built it (else: found in the cache)
  template <class T>
  const T* as() const {
    return e ? e->as<T>() : nullptr;
  }
};

struct ActSlot;
struct fts_rp_batch {
  int B = 0;
  int device = 0;
  // staged on a multi-device context: one child batch per shard, shard j holds
  // proofs [bounds[j], bounds[j+1]) of the caller's batch
  std::vector<fts_rp_batch*> parts;
  std::vector<fts_ctx*> part_ctx;
  std::vector<size_t> bounds;
  int merged = 1;  // batches in the device pass that verified it last
  bool dense = false;  // its last failed verification found dense bad proofs (FTS_GT_ADAPT)
  int locate_skip = 0, locate_backoff = 8;  // single-fault locator backoff (fts_ctx::locate)
  TimingRecord tim;  // of this batch's last verification
  ~fts_rp_batch() {
    for (fts_rp_batch* q : parts) delete q;
    if (raw_mem.p) hipSetDevice(device);
  }
  // a staged batch owns its records; a staging slot's batch has empty owners and its
  // views below point into the slot's `dev`
  DevBuf raw_mem, sc_mem, status0_mem, status_mem, ipa_mem;
  uint8_t* raw = nullptr;
  uint32_t* sc = nullptr;
  int32_t* status0 = nullptr;  // host-parse verdicts (restored before every run)
  int32_t* status = nullptr;
  int32_t* ipa_flag = nullptr;
};

// One call waiting for (or being served by) a device pass: a staged range-proof
// batch (fts_rp_batch_verify, fts_rp_verify_batch), or an action call (transfers /
// issues / requests) whose range proofs are `b` and whose sigma batch is `act`.
struct RpReq {
  fts_rp_batch* b;
  int32_t* status;  // caller's host status array of b's proofs (may be null)
  ActSlot* act = nullptr;
  int rc = 0;
  bool done = false;
  std::chrono::steady_clock::time_point arrived = std::chrono::steady_clock::now();
  std::condition_variable cv;  // this caller's wake-up (targeted, no thundering herd)
  RpReq(fts_rp_batch* bb, int32_t* st, ActSlot* a = nullptr) : b(bb), status(st), act(a) {}
};

// Staging slot of fts_rp_verify_batch (host DER bytes -> device), and the base of the
// action calls' ActSlot: pinned host records and device input buffers, grown
// geometrically and reused across calls, so a call neither allocates nor frees
// device memory (hipFree synchronises the whole device, stalling every other
// lane's pass)
struct StageSlot {
  std::unique_ptr<fts_rp_batch> b;  // its views point into `dev` (not owned by the batch)
  PinBuf pin;
  DevBuf dev;
  Stream s;
  Event done;  // blocking-sync: the waiting caller sleeps
  bool create(int device) {
    b.reset(new fts_rp_batch());
    b->device = device;
    return s.create() == hipSuccess && done.create(hipEventBlockingSync | hipEventDisableTiming) == hipSuccess;
  }
  bool size(size_t pin_bytes, size_t dev_bytes) { return pin.grow(pin_bytes, 0) && dev.grow(dev_bytes, 0); }
  StageSlot() = default;
  ~StageSlot() {  // the stream may still read pin / dev
    if (s) hipStreamSynchronize(s);
  }
};
using RpSlot = StageSlot;

// An action call staged for the dispatcher (act_stage), pooled per context like
// RpSlot: the call's records parsed straight into pinned host memory in their
// device layout, one upload into `dev`, and the call's sigma workspace behind
// them in `dev`.  Its sigma proofs (TypeAndSum / SameType, independent of the
// range proofs) run at once on the slot's own stream, while the call waits for a
// pass; they also write the V slots of its range proofs.  A device pass then
// verifies the range proofs of several calls as one batch (gathered like staged
// range-proof batches) after the calls' sigma events, so concurrent transfer /
// issue / request calls share passes instead of taking a lane each, and the sigma
// work overlaps other passes instead of sitting on a pass's critical path
// (DESIGN.md §3.4).
struct ActSlot : StageSlot {
  // on s: [0] before the sigma kernels, [1] after decode + primes + V slots, [2] after
  // the sigma equations (the pass waits for it before gathering the range proofs)
  Event ev_sig[3];
  SigBatchDev sd{};            // the call's sigma batch (sd.A == 0: none); rp_raw = the slot's range proofs
  int32_t* sig_res = nullptr;  // pinned: sigma verdicts [sd.A], downloaded by the pass
  std::vector<int32_t> rp_res;  // range-proof verdicts [b->B], scattered by the pass
  std::vector<ActionState> st;
  StageLayout lay;  // the call's record layout (host/action_stage.hpp)
  float parse_ms = 0, stage_ms = 0;
  float phase_ms[3] = {0, 0, 0};  // act_stage's shapes / layout / decode steps of the last call
};

struct fts_ctx {
  int device = 0;
  // multi-device context (fts_ctx_create_devices): one child context per device;
  // batch entry points shard their batch over the children (multi_* below)
  std::vector<fts_ctx*> shards;  // owned (released by the destructor)
  PublicParams pp;
  int n = 0, k = 0;
  // fixed-base tables: counted references to entries of the device's table cache
  // (host/table_cache.hpp; private entries with FTS_TABLE_SHARE=0), read-only once built
  TableRef d_tables;
  TableRef d_wtables;  // wide tables of [H_0 .. H_{n-1}, K, P] (k_rp_fixed_exact)
  // their window width: 22 bits (12 additions per product, 1.5 GiB per base) when the
  // device has the memory at context creation, else 20 (13, 436 MiB); FTS_WIDE_BITS
  int wbits = 20;
  int wbits_forced = 0;  // fts_ctx_opts.wide_bits / FTS_WIDE_BITS: no fallback to 20 bits
  int nlanes = 0;
  DevBuf d_x0const;
  DevBuf d_x0tmpl;  // x0 message blocks [x0_cb0, x0_cb1): shared by every proof
  size_t table_bytes = 0;
  // lane pool
  std::vector<std::unique_ptr<Lane>> lanes;
  std::vector<int> free_lanes;
  std::mutex mu;
  std::condition_variable cv;
  int last_lane = 0;
  // timings of the most recently completed range-proof run
  std::mutex tim_mu;
  TimingRecord tim;
  // batch coalescing (fts_rp_batch_verify): staged batches submitted
  // concurrently are merged into one device pass of up to coalesce_max proofs
  std::deque<RpReq*> rp_pending;
  size_t pending_proofs = 0;  // proofs queued in rp_pending
  // 81,920 proofs (20 batches of 4,096): a burst of batches (the driver's 20-step
  // bench) shares two or three large passes, whose chain kernels (com, the
  // per-proof x0 hash, the MSM's final reduction) run at several waves per SIMD
  // instead of under one (tools/s20_sweep4.sh: 3.0 -> 3.6 M rp64/s at 20 steps,
  // 4.41 -> 4.47 M/s at 512 steps, single-batch latency unchanged)
  size_t coalesce_max = 81920;
  // gather window: while the device is busy and fewer than gather_target proofs
  // are queued, the head request waits up to gather_us for more batches before
  // it takes a lane (a burst of callers then shares a few large passes instead
  // of one lone 4,096-proof pass per free lane); an idle device starts at once
  size_t gather_target = 16384;
  int gather_us = 1000;
  // An idle device's window (FTS_IDLE_GATHER_US / FTS_IDLE_QUIET_US): the head waits
  // while batches keep arriving (each within idle_quiet_us of the last, at most
  // idle_gather_us in all) or until gather_target proofs are queued, and its pass
  // takes at most gather_target proofs.  A burst of 20 callers released together
  // (the driver's 20-step line) becomes two passes of 10 batches whatever the
  // threads' timing (r05: 4.19-4.32 M/s medians with passes of 1 + 10 + 9, formed by
  // arrival luck; 4.35-4.40 with 10 + 10); a lone caller waits idle_quiet_us.
  int idle_gather_us = 1000;
  int idle_quiet_us = 150;
  std::chrono::steady_clock::time_point last_arrival{};
  // FTS_IDLE_FIRST_US: a caller that arrives at an idle device with no other arrival in
  // the last idle_quiet_us (a lone caller, not part of a burst) waits only this long
  // for company -- spinning, not on a condition variable whose wake-up alone cost
  // ~0.1 ms -- and starts at once when nobody comes (round 5 paid the whole quiet gap
  // plus a wake-up: 3.36 vs 2.75-2.86 ms for a lone 4,096-proof batch)
  int idle_first_us = 30;
  std::atomic<uint64_t> arrivals{0};
  // test hook (fts_debug_hold): no pass starts until hold_n requests are queued
  int hold_n = 0;
  // dispatcher counters (fts_debug_dispatch_stats)
  std::atomic<int64_t> st_passes{0}, st_reqs{0}, st_max_merged{0}, st_act_reqs{0};
  // range-proof pass counters (fts_debug_pass_stats): passes finished, passes whose
  // combination did not close, locator hits, proofs given to the per-proof equations
  std::atomic<int64_t> st_rp_passes{0}, st_rp_failed{0}, st_rp_located{0}, st_rp_perproof{0};
  // prover-side work counters (fts_debug_shard_work), bumped next to the launches: range
  // proofs proved, sigma proofs (actions), tokens committed, prover / commit passes started
  std::atomic<int64_t> st_pv_proofs{0}, st_pv_actions{0}, st_pv_tokens{0}, st_pv_passes{0};
  // passes of up to com_fixed_max proofs compute com on the latency path (fixed-base
  // groups, rp_exact.hip k_rp_fixed_all), larger ones on the work path (Horner +
  // joint GLV chains): the same group element either way
  size_t com_fixed_max = 16384;
  // group test: round-1 group size and round-2 threshold (FTS_GT1 / FTS_GT2_MIN).  Larger
  // round-1 groups make the grouped MSM's bucket reduction cheaper (it scales with the
  // group count); the per-proof checks of the failing groups cost one GLV chain of
  // latency whatever their number up to ~8k proofs (tools/gt_sweep.sh, C5 1 % tampered:
  // 64/2048 -> 256/8192 = 485k -> 533k actions/s)
  int gt1 = 256, gt2_min = 8192;
  // FTS_LOCATE: after a failed (ungrouped) batch check whose caller batches are all
  // sparse, first the single-fault locator (rp_locate_single): one index-weighted
  // recombination + a lane per proof, instead of the group test's grouped MSM
  bool locate = true;
  // after a miss (several bad proofs) each caller batch of the pass that holds a bad
  // proof skips the locator in its next locate_backoff failing passes, the backoff
  // doubling per consecutive miss (8 .. 256) and reset by a hit: a stream of
  // multi-fault batches (C5, tampered C2) pays it rarely.  Kept per caller batch
  // (fts_rp_batch::locate_skip), so one caller's multi-fault passes never make
  // another caller's single-fault passes skip the locator
  // action calls (transfer / issue / mixed / request) have no batch object across
  // calls: they share one locator backoff, carried into each call's slot batch and
  // back (a stream of multi-fault calls -- C5 with 1 % tampered actions -- would
  // otherwise pay a missed locator, one extra MSM, on every call)
  std::atomic<int> act_locate_skip{0}, act_locate_backoff{8};
  // FTS_GT_ADAPT: a staged caller batch's round-1 group size follows the bad-proof
  // density of ITS last failed verification (fts_rp_batch::dense; per caller batch,
  // so one caller's tampered batches never change the fallback of another's).
  // Dense (more than half the batch's proofs in failing 256-groups, or more than
  // 2 % in failing 8-groups: ~0.3 % bad proofs and up) starts at groups of 8 on the
  // small-group kernels; a 256-group round there is one whole grouped Pippenger MSM
  // that clears almost nothing (C2 with 1 % tampered, 81,920-proof pass: 51.8 ->
  // 41.4 ms; C5's sparse bad proofs keep 256, where 8 was slower,
  // tools/sweeps/gt1_small.txt).  Action calls have no batch across calls: 256.
  int gt_adapt = 1;
  // FTS_X0_SPLIT: bit 0 the work path hashes the x0 prefix beside the com chain, bit 1
  // the latency path beside com_tree (round 6: a lone 4,096-proof batch 3.15 -> 2.87 ms,
  // profiles/r06_x0_split_ab/); 1 = the work path only (rounds 2-5)
  int x0_split = 3;
  // FTS_MSM_SORT: the MSMs' two-level counting sort (msm.hip k_rs_*; 0: k_msm_digits'
  // device atomics + k_msm_scatter, the round-4 batch-check sort, for A/B)
  int msm_sort = 1;
  // FTS_MSM_MAXC: the widest MSM window this context's plans take (per context: one
  // context's setting never changes another's plans)
  int msm_maxc = 16;
  // FTS_MAIN_GROUPS=1: a coalesced pass checks one random linear combination PER CALLER
  // BATCH (a G-group MSM + per-group column sums), so a bad proof's fallback covers
  // its own batch only.  Default 0 (one combination over the pass): the grouped MSM's
  // extra windows and per-group bucket reductions cost 10-17 % of the clean 512-step
  // rate (4.96 -> 4.47 M rp64/s, gpurun_out/r05b) for +10 % with one bad proof per pass
  int main_groups = 0;
  // FTS_FX_SERIAL: passes' fixed-base launches run one at a time across the lanes
  // (device-side event chain under fx_mu), staggering concurrent passes
  int fx_serial = 0;
  std::mutex fx_mu;
  hipEvent_t fx_last = nullptr;  // (a lane's ev_d, not owned) the fixed-base event of the pass enqueued last
  // FTS_RLC_FORK: the batch check forks after the fixed-base products (1) or after the
  // challenges (0); 2 (default): after the challenges on the latency path (a lone small
  // pass: its MSM chain is the critical path, 3.16 -> 2.98 ms per 4,096-proof batch),
  // after the fixed-base products on the work path (larger passes: 4.69 -> 4.82 M/s at
  // 512 steps; tools/run_lat4k.sh, tools/run_fork.sh)
  int rlc_fork = 2;
  // a lane was freed (call with mu held): the head pending range-proof request
  // becomes the next leader; LaneGuard waiters re-check too
  void wake_lane_waiters() {
    if (!rp_pending.empty()) rp_pending.front()->cv.notify_one();
    cv.notify_all();
  }
  std::once_flag prover_once;
  ProverTables ptab;
  std::mutex slot_mu;
  std::vector<std::unique_ptr<RpSlot>> slots;    // fts_rp_verify_batch staging
  std::vector<std::unique_ptr<ActSlot>> aslots;  // action-call staging
  std::vector<RpSlot*> free_slots;               // the idle ones, under slot_mu
  std::vector<ActSlot*> free_aslots;
  // members are released on the context's device; a host-only context and a
  // multi-device parent own no device resource
  ~fts_ctx() {
    const bool owns_device = shards.empty() && device != FTS_DEVICE_NONE && !lanes.empty();
    for (fts_ctx* ch : shards) delete ch;
    if (owns_device) hipSetDevice(device);
  }
};

// RAII lane acquisition (want < 0: any free lane)
struct LaneGuard {
  fts_ctx* c;
  Lane* L;
  LaneGuard(fts_ctx* cc, int want = -1) : c(cc), L(nullptr) {
    std::unique_lock<std::mutex> lk(c->mu);
    c->cv.wait(lk, [&] {
      if (want < 0) return !c->free_lanes.empty();
      return std::find(c->free_lanes.begin(), c->free_lanes.end(), want) != c->free_lanes.end();
    });
    auto it = want < 0 ? c->free_lanes.end() - 1 : std::find(c->free_lanes.begin(), c->free_lanes.end(), want);
    L = c->lanes[*it].get();
    c->free_lanes.erase(it);
    L->alone = c->free_lanes.size() + 1 == c->lanes.size();
  }
  ~LaneGuard() {
    std::lock_guard<std::mutex> lk(c->mu);
    c->free_lanes.push_back(L->id);
    c->wake_lane_waiters();
  }
};

// ---- functions the units call across (the unit that defines each in brackets)
// DER range proofs -> device input records in caller-provided host memory [api_rp.cpp]
void parse_rp_into(int k, size_t B, const uint8_t* const* der_p, const size_t* der_len, const uint8_t* com64,
                   uint8_t* raw, uint32_t* sc, int32_t* status, int32_t* ipa);
// the lane's timeline + host phases -> the context's record (and b's); sig_ms
// (optional): the k_sig_prep / k_sig_finish spans of an action call's slot [api_rp.cpp]
void collect_timings(fts_ctx* c, Lane& L, fts_rp_batch* b, const float* sig_ms = nullptr);
// MSM plans on a lane's workspace, and the lane's workspace itself [api_rp.cpp]
int msm_prepare_plan(Lane& L, MsmPlan& mp, int slot);
int msm_prepare(Lane& L, int N, MsmPlan& mp, int slot, int ch, bool local_sort, int maxc);
int lane_reserve(fts_ctx* c, Lane& L, int B, bool inputs);
// the work-sharing dispatcher of staged batches and action calls [api_rp.cpp]
int rp_dispatch(fts_ctx* c, RpReq& me);
// the context's host prover tables, built on first use [api_prove.cpp]
const ProverTables& prover_tables(const fts_ctx* cc);
// the argument checks of the action provers on one witness [api_prove.cpp]
bool action_witness_valid(const fts_action_witness& x, int issue);
// A whole transfer (issue = 0) / issue proofs on one device context: w[a] is item g0 + a
// of its call and draws from src.at(g0 + a) -- the index in the caller's batch, never the
// one inside a shard; der[a] <- the proof of fts_transfer_prove / fts_issue_prove.  The
// caller has checked every witness (action_witness_valid / gen_valid) [api_prove.cpp]
int actions_prove_core(fts_ctx* c, size_t g0, size_t A, const fts_action_witness* w, int issue,
                       const RngSource& src, std::string* der);
// n token commitments on one device context: item(i, type, type_len, value, bf32) names
// token i; com64_out[i] <- its 64 bytes [api_generate.cpp]
using CommitItem = std::function<void(size_t, const uint8_t*&, size_t&, uint64_t&, const uint8_t*&)>;
int token_commit_device(fts_ctx* c, size_t n, const CommitItem& item, uint8_t* com64_out);

// run f(j, lo, hi) for every non-empty shard j concurrently; first error wins
template <class F>
int run_shards(const std::vector<size_t>& bnd, F&& f) {
  const int ns = (int)bnd.size() - 1;
  std::vector<int> rc(ns, FTS_API_OK);
  std::vector<std::thread> th;
  for (int j = 0; j < ns; j++)
    if (bnd[j + 1] > bnd[j]) th.emplace_back([&, j]() { rc[j] = f(j, bnd[j], bnd[j + 1]); });
  for (auto& t : th) t.join();
  for (int r : rc)
    if (r != FTS_API_OK) return r;
  return FTS_API_OK;
}
inline std::vector<size_t> plan(size_t n, const std::vector<double>* w, int ns) {
  std::vector<size_t> b(ns + 1);
  fts_shard_plan(n, w ? w->data() : nullptr, ns, b.data());
  return b;
}

// f(child, lo, hi) for the slice [lo, hi) of n items on every child of a multi-device
// context (split by the weights w, NULL: equal), concurrently; f(c, 0, n) on any other
template <class F>
int over_devices(fts_ctx* c, size_t n, const std::vector<double>* w, F&& f) {
  if (c->shards.empty()) return f(c, (size_t)0, n);
  return run_shards(plan(n, w, (int)c->shards.size()),
                    [&](int j, size_t lo, size_t hi) { return f(c->shards[j], lo, hi); });
}

// cost weight of an action: its range proofs (none for a 1-in/1-out transfer) + the sigma proof
inline double action_weight(size_t n_in, size_t n_out, bool transfer) {
  return (transfer && n_in == 1 && n_out == 1 ? 0.0 : (double)n_out) + 0.25;
}

// canonical LE u32 limbs of a BE 32-byte integer reduced mod r (G1.Mul(s) = (s mod r) P)
inline void zr_canon_words(const uint8_t* be32, uint32_t out[8]) {
  uint64_t c[4];
  be32_to_u64(be32, c);
  while (geq_mod<ModR>(c)) sub_mod_raw<ModR>(c);
  for (int i = 0; i < 4; i++) out[2 * i] = (uint32_t)c[i], out[2 * i + 1] = (uint32_t)(c[i] >> 32);
}
inline void fr_canon_words(const Fr& a, uint32_t out[8]) {
  uint64_t c[4];
  from_mont(a, c);
  for (int i = 0; i < 4; i++) out[2 * i] = (uint32_t)c[i], out[2 * i + 1] = (uint32_t)(c[i] >> 32);
}
inline bool fr_arg(const uint8_t* b32, Fr& out) {
  if (!b32) return false;
  out = fr_from_be(b32);
  return true;
}
