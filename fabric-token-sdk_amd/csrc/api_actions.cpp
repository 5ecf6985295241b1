// C-ABI (include/fts_gpu.h): action calls -- transfers, issues, mixed batches and
// raw token requests.  Device half of the staging (host/action_stage.hpp is the
// host half), verdict folding with the reference's precedence, and the entry
// points.
#include "host/api_internal.hpp"

// ------------------------------------------------------- transfers / issues
// One action = a transfer (TypeAndSum + RangeCorrectness on Out_j - CT,
// transfer/transfer.go:49-60,153-197) or an issue (SameType + RangeCorrectness
// on Tok_i - CT, issue/verifier.go:24-57).  An action call is parsed straight into
// a pooled slot's pinned records (act_stage), uploaded once, and verified by the
// range-proof dispatcher (rp_dispatch) together with whatever else is queued.

// an idle action staging slot (or a new one); nullptr on failure
static ActSlot* aslot_acquire(fts_ctx* c) {
  {
    std::lock_guard<std::mutex> g(c->slot_mu);
    if (!c->free_aslots.empty()) {
      ActSlot* sl = c->free_aslots.back();
      c->free_aslots.pop_back();
      return sl;
    }
  }
  std::unique_ptr<ActSlot> sl(new ActSlot());
  bool ok = sl->create(c->device);
  for (Event& e : sl->ev_sig) ok = ok && e.create() == hipSuccess;
  if (!ok) return nullptr;
  std::lock_guard<std::mutex> g(c->slot_mu);
  c->aslots.push_back(std::move(sl));
  return c->aslots.back().get();
}

static void aslot_release(fts_ctx* c, ActSlot* sl) {
  std::lock_guard<std::mutex> g(c->slot_mu);
  c->free_aslots.push_back(sl);
}

// the staging functions' loop: the host pool
static const auto stage_loop = [](size_t n, auto&& f) { parallel_for(n, 2, f); };

// Stage an action call in slot sl: its records parsed (host/action_stage.hpp)
// straight into the slot's pinned buffer in their device layout (no per-action
// host vectors, no second copy), one upload, and the sigma kernels on the slot's
// stream.
static int act_stage(fts_ctx* c, ActSlot* sl, const std::vector<ActionIn>& acts) {
  const double t0 = now_ms();
  const int k = c->k;
  StageLayout& lay = sl->lay;
  stage_layout(k, acts, sl->st, lay, stage_loop);
  if (!sl->size(std::max<size_t>(lay.pin_end, 256), std::max<size_t>(lay.dev_end, 256))) return FTS_API_ENOMEM;
  uint8_t* hp = sl->pin.as<uint8_t>();
  const double t_p2 = now_ms();
  stage_decode(k, acts, sl->st, lay, hp, stage_loop);
  const double t1 = now_ms();
  sl->parse_ms = (float)(t1 - t0);
  sl->phase_ms[0] = (float)(lay.t_shapes - t0);
  sl->phase_ms[1] = (float)(t_p2 - lay.t_shapes);
  sl->phase_ms[2] = (float)(t1 - t_p2);
  // the slot's views: range-proof batch and sigma batch over the device copy
  const int SA = lay.tot.sa, rp_total = lay.tot.rp;
  uint8_t* dv = sl->dev.as<uint8_t>();
  fts_rp_batch* b = sl->b.get();
  b->B = rp_total;
  b->raw = dv + lay.o_rraw;
  b->sc = reinterpret_cast<uint32_t*>(dv + lay.o_rsc);
  b->status0 = reinterpret_cast<int32_t*>(dv + lay.o_rst);
  b->ipa_flag = reinterpret_cast<int32_t*>(dv + lay.o_ripa);
  b->status = nullptr;  // never verified in place: the pass gathers it
  b->dense = false;     // action calls have no batch across calls (FTS_GT_ADAPT: groups of 256)
  b->locate_skip = c->act_locate_skip.load(std::memory_order_relaxed);  // the calls' shared backoff
  b->locate_backoff = c->act_locate_backoff.load(std::memory_order_relaxed);
  b->merged = 1;
  b->tim.n = 0;
  sl->rp_res.assign((size_t)rp_total, FTS_E_NOT_RUN);
  sl->sig_res = reinterpret_cast<int32_t*>(hp + lay.o_res);
  SigBatchDev& sd = sl->sd;
  sd = SigBatchDev{};
  sd.A = SA;
  sd.npts = lay.tot.pt;
  sd.naff = lay.tot.aff;
  sd.nwork = lay.tot.term;
  sd.nfix = lay.tot.nfix;
  sd.act = reinterpret_cast<const SigAction*>(dv + lay.o_act);
  sd.raw = dv + lay.o_raw;
  sd.pt_owner = reinterpret_cast<int32_t*>(dv + lay.o_owner);
  sd.pts = reinterpret_cast<uint32_t*>(dv + lay.w_pts);
  sd.sc = reinterpret_cast<uint32_t*>(dv + lay.o_sc);
  sd.status = reinterpret_cast<int32_t*>(dv + lay.o_sst);
  sd.work = reinterpret_cast<int2*>(dv + lay.o_work);
  sd.terms = reinterpret_cast<uint32_t*>(dv + lay.w_terms);
  sd.aff = reinterpret_cast<uint32_t*>(dv + lay.w_aff);
  sd.aff_off = reinterpret_cast<int32_t*>(dv + lay.o_affoff);
  sd.msgs = dv + lay.w_msgs;
  sd.jac = reinterpret_cast<uint32_t*>(dv + lay.w_jac);
  sd.scratch = reinterpret_cast<uint32_t*>(dv + lay.w_scratch);
  sd.rp_k = k;
  if (SA || rp_total) {
    // upload, then the sigma proofs at once on the slot's stream: decode + primes (and
    // the V slots of the call's own range proofs, before any pass gathers them), the
    // equations and transcripts.  No host wait: the pass waits for ev_sig[2], and the
    // pinned records stay the slot's until the call returns.
    sd.rp_raw = rp_total ? b->raw : nullptr;
    HIP_OK(hipMemcpyAsync(dv, hp, lay.in_end, hipMemcpyHostToDevice, sl->s));
    HIP_OK(hipEventRecord(sl->ev_sig[0], sl->s));
    if (SA) launch_sig_prep(sd, sl->s);
    HIP_OK(hipEventRecord(sl->ev_sig[1], sl->s));
    if (SA) launch_sig_finish(sd, c->d_tables.as<uint32_t>(), c->n, sl->s);
    HIP_OK(hipEventRecord(sl->ev_sig[2], sl->s));
    HIP_OK(hipGetLastError());
  }
  sl->stage_ms = (float)(now_ms() - t1);
  return FTS_API_OK;
}

// the entry points' items as staging inputs (a null proof is an empty one)
static void add_transfers(std::vector<ActionIn>& acts, size_t n, const fts_transfer_item* it) {
  acts.reserve(acts.size() + n);
  for (size_t i = 0; i < n; i++)
    acts.push_back(ActionIn{SIG_TAS, it[i].inputs, it[i].n_in, it[i].outputs, it[i].n_out,
                            der::Span{it[i].proof, it[i].proof ? it[i].proof_len : 0}});
}
static void add_issues(std::vector<ActionIn>& acts, size_t n, const fts_issue_item* it) {
  acts.reserve(acts.size() + n);
  for (size_t i = 0; i < n; i++)
    acts.push_back(ActionIn{SIG_ST, nullptr, 0, it[i].tokens, it[i].n_tok,
                            der::Span{it[i].proof, it[i].proof ? it[i].proof_len : 0}});
}

// Verify an action call: stage it, let the dispatcher verify it (alone or with
// other queued calls), then combine each action's sigma and range-proof verdicts
// with the reference's precedence.
static int act_verify(fts_ctx* c, const std::vector<ActionIn>& acts, int32_t* status, int32_t* fail_index) {
  ActSlot* sl = aslot_acquire(c);
  if (!sl) return FTS_API_ENOMEM;
  int rc = act_stage(c, sl, acts);
  if (rc == FTS_API_OK && sl->b->B) {
    RpReq me(sl->b.get(), sl->rp_res.data(), sl);
    rc = rp_dispatch(c, me);
    c->act_locate_skip.store(sl->b->locate_skip, std::memory_order_relaxed);
    c->act_locate_backoff.store(sl->b->locate_backoff, std::memory_order_relaxed);
  } else if (rc == FTS_API_OK && sl->sd.A) {  // sigma proofs only (1-in/1-out transfers): no pass
    if (hipMemcpyAsync(sl->sig_res, sl->sd.status, (size_t)sl->sd.A * 4, hipMemcpyDeviceToHost, sl->s) != hipSuccess ||
        hipEventRecord(sl->done, sl->s) != hipSuccess || hipEventSynchronize(sl->done) != hipSuccess)
      rc = FTS_API_EDEVICE;
  }
  if (rc == FTS_API_OK) {
    const std::vector<ActionState>& st = sl->st;
    const int32_t* sig_res = sl->sig_res;
    const int32_t* rp_res = sl->rp_res.data();
    for (size_t i = 0; i < acts.size(); i++) {
      const ActionState& s = st[i];
      int32_t out = FTS_OK, idx = -1;
      if (s.host_final >= 0) {
        out = s.host_final;
      } else {
        const int32_t sig = sig_res[s.sig];
        bool malformed = sig == FTS_E_MALFORMED;
        for (int j = 0; j < s.rp_count && s.rp_base >= 0; j++) malformed |= rp_res[s.rp_base + j] == FTS_E_MALFORMED;
        if (malformed) {
          out = FTS_E_MALFORMED;                       // deserialisation precedes verification
        } else if (sig != FTS_OK) {
          out = sig;                                   // TypeAndSum / SameType error wins (transfer.go:192-196)
        } else if (s.rc_applicable) {
          if (s.rc_count_bad) {
            out = FTS_E_RC_COUNT;                      // rangecorrectness.go:138-140
          } else {
            for (int j = 0; j < s.rp_count; j++)       // first failing index wins (:141-160)
              if (rp_res[s.rp_base + j] != FTS_OK) {
                out = rp_res[s.rp_base + j];
                idx = j;
                break;
              }
          }
        }
      }
      status[i] = out;
      if (fail_index) fail_index[i] = idx;
    }
  }
  // an error path may leave the upload or the sigma kernels queued on the slot's
  // stream, still reading its pinned / device buffers: drain it before the next
  // caller may reuse (or re-allocate) them
  if (rc != FTS_API_OK && sl->s) (void)hipStreamSynchronize(sl->s);
  aslot_release(c, sl);
  return rc;
}

// act_verify; on an error every verdict is FTS_E_NOT_RUN
static int act_verify_or_not_run(fts_ctx* c, const std::vector<ActionIn>& acts, int32_t* status, int32_t* fail_index) {
  const int rc = act_verify(c, acts, status, fail_index);
  if (rc != FTS_API_OK) std::fill(status, status + acts.size(), FTS_E_NOT_RUN);
  return rc;
}

// host-side cost of the staging's host half (parse + layout, no device): tools/host_parse_bench.py
extern "C" int fts_debug_stage_actions(fts_ctx* c, size_t n_tr, const fts_transfer_item* transfers, size_t n_is,
                                       const fts_issue_item* issues, int reps, float* ms_avg) {
  if (!c || (n_tr && !transfers) || (n_is && !issues) || reps < 1 || c->device >= 0 || !c->shards.empty())
    return FTS_API_EINVAL;
  std::vector<ActionIn> acts;
  add_transfers(acts, n_tr, transfers);
  add_issues(acts, n_is, issues);
  // the host half alone, into host memory: no slot, no stream, no device
  std::vector<ActionState> st;
  StageLayout lay;
  std::vector<uint8_t> buf;
  double tot[4] = {0, 0, 0, 0};
  for (int r = -1; r < reps; r++) {  // run -1 untimed: the buffers grow (page faults) once
    const double t0 = now_ms();
    stage_layout(c->k, acts, st, lay, stage_loop);
    buf.resize(std::max<size_t>(lay.pin_end, 256));
    const double t_p2 = now_ms();
    stage_decode(c->k, acts, st, lay, buf.data(), stage_loop);
    const double t1 = now_ms();
    if (r < 0) continue;
    tot[0] += (float)(t1 - t0);
    tot[1] += (float)(lay.t_shapes - t0), tot[2] += (float)(t_p2 - lay.t_shapes), tot[3] += (float)(t1 - t_p2);
  }
  if (ms_avg)
    for (int q = 0; q < 4; q++) ms_avg[q] = (float)(tot[q] / reps);
  return FTS_API_OK;
}


extern "C" {

int fts_transfer_verify_batch(fts_ctx* c, size_t n, const fts_transfer_item* items, int32_t* status,
                              int32_t* fail_index) {
  if (!c || !status || (n && !items)) return FTS_API_EINVAL;
  if (!c->shards.empty()) {
    std::vector<double> w(n);
    for (size_t i = 0; i < n; i++) w[i] = action_weight(items[i].n_in, items[i].n_out, true);
    return run_shards(plan(n, &w, (int)c->shards.size()), [&](int j, size_t lo, size_t hi) {
      return fts_transfer_verify_batch(c->shards[j], hi - lo, items + lo, status + lo,
                                       fail_index ? fail_index + lo : nullptr);
    });
  }
  if (c->device < 0) return FTS_API_EDEVICE;
  if (n == 0) return FTS_API_OK;
  std::vector<ActionIn> acts;
  add_transfers(acts, n, items);
  HIP_OK(hipSetDevice(c->device));
  return act_verify_or_not_run(c, acts, status, fail_index);
}

int fts_issue_verify_batch(fts_ctx* c, size_t n, const fts_issue_item* items, int32_t* status, int32_t* fail_index) {
  if (!c || !status || (n && !items)) return FTS_API_EINVAL;
  if (!c->shards.empty()) {
    std::vector<double> w(n);
    for (size_t i = 0; i < n; i++) w[i] = action_weight(0, items[i].n_tok, false);
    return run_shards(plan(n, &w, (int)c->shards.size()), [&](int j, size_t lo, size_t hi) {
      return fts_issue_verify_batch(c->shards[j], hi - lo, items + lo, status + lo, fail_index ? fail_index + lo : nullptr);
    });
  }
  if (c->device < 0) return FTS_API_EDEVICE;
  if (n == 0) return FTS_API_OK;
  std::vector<ActionIn> acts;
  add_issues(acts, n, items);
  HIP_OK(hipSetDevice(c->device));
  return act_verify_or_not_run(c, acts, status, fail_index);
}

// mixed batch (BASELINE config C5): the transfers and issues of many token
// requests verified in ONE device pass (one range-proof batch + one sigma batch)
int fts_actions_verify_batch(fts_ctx* c, size_t n_tr, const fts_transfer_item* transfers, size_t n_is,
                             const fts_issue_item* issues, int32_t* status_tr, int32_t* fail_tr, int32_t* status_is,
                             int32_t* fail_is) {
  if (!c || (n_tr && (!transfers || !status_tr)) || (n_is && (!issues || !status_is))) return FTS_API_EINVAL;
  if (!c->shards.empty()) {  // transfers and issues each split into balanced shards, device j gets part j of both
    const int ns = (int)c->shards.size();
    std::vector<double> wt(n_tr), wi(n_is);
    for (size_t i = 0; i < n_tr; i++) wt[i] = action_weight(transfers[i].n_in, transfers[i].n_out, true);
    for (size_t i = 0; i < n_is; i++) wi[i] = action_weight(0, issues[i].n_tok, false);
    const std::vector<size_t> bt = plan(n_tr, &wt, ns), bi = plan(n_is, &wi, ns);
    std::vector<size_t> all(ns + 1);
    for (int j = 0; j <= ns; j++) all[j] = j;
    return run_shards(all, [&](int j, size_t, size_t) {
      const size_t t0 = bt[j], t1 = bt[j + 1], i0 = bi[j], i1 = bi[j + 1];
      if (t1 == t0 && i1 == i0) return FTS_API_OK;
      return fts_actions_verify_batch(c->shards[j], t1 - t0, transfers + t0, i1 - i0, issues + i0,
                                      status_tr ? status_tr + t0 : nullptr, fail_tr ? fail_tr + t0 : nullptr,
                                      status_is ? status_is + i0 : nullptr, fail_is ? fail_is + i0 : nullptr);
    });
  }
  if (c->device < 0) return FTS_API_EDEVICE;
  const size_t n = n_tr + n_is;
  if (n == 0) return FTS_API_OK;
  std::vector<ActionIn> acts;
  add_transfers(acts, n_tr, transfers);
  add_issues(acts, n_is, issues);
  std::vector<int32_t> st(n, FTS_E_NOT_RUN), fi(n, -1);
  HIP_OK(hipSetDevice(c->device));
  const int rc = act_verify_or_not_run(c, acts, st.data(), fi.data());
  for (size_t i = 0; i < n_tr; i++) {
    status_tr[i] = st[i];
    if (fail_tr) fail_tr[i] = fi[i];
  }
  for (size_t i = 0; i < n_is; i++) {
    status_is[i] = st[n_tr + i];
    if (fail_is) fail_is[i] = fi[n_tr + i];
  }
  return rc;
}

// Raw TokenRequest ingest: decode n requests on the host threads, verify the
// proofs of every action of every request in one device pass, then fold each
// request's action verdicts in the reference's order (issues, then transfers).
int fts_request_verify_batch(fts_ctx* c, size_t n, const uint8_t* const* req, const size_t* req_len,
                             int32_t* status, int32_t* fail_action, int32_t* fail_index) {
  if (!c || !status || (n && (!req || !req_len))) return FTS_API_EINVAL;
  if (!c->shards.empty()) {  // request bytes approximate the proofs they carry
    std::vector<double> w(n);
    for (size_t i = 0; i < n; i++) w[i] = (double)req_len[i] + 64.0;
    return run_shards(plan(n, &w, (int)c->shards.size()), [&](int j, size_t lo, size_t hi) {
      return fts_request_verify_batch(c->shards[j], hi - lo, req + lo, req_len + lo, status + lo,
                                      fail_action ? fail_action + lo : nullptr, fail_index ? fail_index + lo : nullptr);
    });
  }
  if (c->device < 0) return FTS_API_EDEVICE;
  if (n == 0) return FTS_API_OK;
  namespace rq = fts::host::req;
  std::vector<rq::Request> R(n);
  {
    unsigned nth = n >= 64 ? host_threads() : 1u;
    std::atomic<size_t> next{0};
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nth; t++)
      th.emplace_back([&]() {
        for (size_t i; (i = next++) < n;)
          rq::parse_request(req[i], req[i] ? req_len[i] : 0, SIG_TAS, SIG_ST, R[i]);
      });
    for (auto& t : th) t.join();
  }
  // actions that reach the verifier: those before (and excluding) the request's
  // first structurally invalid action
  std::vector<ActionIn> acts;
  std::vector<std::pair<uint32_t, uint32_t>> owner;  // (request, position in acts order)
  for (size_t i = 0; i < n; i++) {
    if (R[i].deser_failed) continue;
    for (size_t j = 0; j < R[i].acts.size(); j++) {
      const rq::Action& a = R[i].acts[j];
      if (a.pre >= 0) break;
      acts.push_back(ActionIn{a.kind, R[i].in(a), a.n_in, R[i].out(a), a.n_out, der::Span{a.proof, a.proof_len}});
      owner.emplace_back((uint32_t)i, (uint32_t)j);
    }
  }
  std::vector<int32_t> st(acts.size(), FTS_OK), fi(acts.size(), -1);
  int rc = FTS_API_OK;
  if (!acts.empty()) {
    HIP_OK(hipSetDevice(c->device));
    rc = act_verify_or_not_run(c, acts, st.data(), fi.data());
  }
  // fold: first failing verified action, else the first structural verdict
  std::vector<int32_t> first(n, -1);  // index into acts of the request's first failing action
  for (size_t q = acts.size(); q-- > 0;)
    if (st[q] != FTS_OK) first[owner[q].first] = (int32_t)q;
  for (size_t i = 0; i < n; i++) {
    const rq::Request& r = R[i];
    int32_t s = r.status, fa = r.fail_action, fx = -1;
    if (rc != FTS_API_OK) {
      s = FTS_E_NOT_RUN, fa = -1;
    } else if (!r.deser_failed) {
      if (first[i] >= 0) {
        const int q = first[i];
        s = st[q], fx = fi[q], fa = r.acts[owner[q].second].index;
      } else {
        for (const rq::Action& a : r.acts)
          if (a.pre >= 0) {
            s = a.pre, fa = a.index;
            break;
          }
      }
    }
    status[i] = s;
    if (fail_action) fail_action[i] = fa;
    if (fail_index) fail_index[i] = fx;
  }
  return rc;
}

int fts_request_inspect(const uint8_t* req, size_t req_len, int32_t* status, int32_t* fail_action, int32_t* n_issue,
                        int32_t* n_transfer, int32_t* pre_status, int32_t* pre_action) {
  if (!status || (req_len && !req)) return FTS_API_EINVAL;
  fts::host::req::Request r;
  fts::host::req::parse_request(req, req ? req_len : 0, SIG_TAS, SIG_ST, r);
  int32_t ni = 0, nt = 0, ps = FTS_OK, pa = -1;
  for (const auto& a : r.acts) {
    (a.transfer ? nt : ni)++;
    if (a.pre >= 0 && pa < 0) ps = a.pre, pa = a.index;
  }
  *status = r.status;
  if (fail_action) *fail_action = r.fail_action;
  if (n_issue) *n_issue = ni;
  if (n_transfer) *n_transfer = nt;
  if (pre_status) *pre_status = ps;
  if (pre_action) *pre_action = pa;
  return FTS_API_OK;
}

}  // extern "C"
