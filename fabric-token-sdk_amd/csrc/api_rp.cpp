// C-ABI (include/fts_gpu.h): range proofs.  One device pass over proofs already
// on the device (rp_enqueue .. rp_finish), the fallbacks of a failed batch check
// (single-fault locator, group test), the work-sharing dispatcher that merges
// staged batches and action calls into passes (rp_dispatch), staged batches,
// fts_rp_verify_batch and the debug hooks.
#include "host/api_internal.hpp"

// ------------------------------------------------------------ range proofs
// host records for B proofs
struct RpHost {
  std::vector<uint8_t> raw;
  std::vector<uint32_t> sc;
  std::vector<int32_t> status, ipa;
};

// DER range proofs -> device input records (raw BE points with the caller's
// commitment in slot V, canonical scalars, host-parse verdicts), written into
// caller-provided host memory (pageable or pinned); parallel over chunks of
// 256 proofs on the host pool
void parse_rp_into(int k, size_t B, const uint8_t* const* der_p, const size_t* der_len, const uint8_t* com64,
                   uint8_t* raw, uint32_t* sc, int32_t* status, int32_t* ipa) {
  const int npts = rp_npts(k);
  constexpr size_t CH = 256;
  parallel_for((B + CH - 1) / CH, 2, [&](size_t c) {
    for (size_t i = c * CH; i < std::min(B, (c + 1) * CH); i++) {
      uint8_t* pts = raw + i * npts * 64;  // every slot written once below (no clearing pass)
      status[i] = 0;
      ipa[i] = 0;
      der::Span s{der_p[i], der_len[i]};
      if (!der_p[i]) s.n = 0;
      parse_range_proof(s, k, pts, sc + i * RP_NSC * 8, status[i], ipa[i]);
      memcpy(pts + RP_PT_V * 64, com64 + i * 64, 64);
    }
  });
}

static void parse_rp_batch(int k, size_t B, const uint8_t* const* der_p, const size_t* der_len, const uint8_t* com64,
                           RpHost& h) {
  const int npts = rp_npts(k);
  h.raw.assign(B * npts * 64, 0);
  h.sc.assign(B * RP_NSC * 8, 0);
  h.status.assign(B, 0);
  h.ipa.assign(B, 0);
  parse_rp_into(k, B, der_p, der_len, com64, h.raw.data(), h.sc.data(), h.status.data(), h.ipa.data());
}

static int multi_rp_verify(fts_ctx* c, size_t n, const uint8_t* const* der, const size_t* len, const uint8_t* com64,
                           int32_t* status) {
  return run_shards(plan(n, nullptr, (int)c->shards.size()), [&](int j, size_t lo, size_t hi) {
    return fts_rp_verify_batch(c->shards[j], hi - lo, der + lo, len + lo, com64 + 64 * lo, status + lo);
  });
}

// sig_ms (optional): the k_sig_prep / k_sig_finish spans of an action call's slot
void collect_timings(fts_ctx* c, Lane& L, fts_rp_batch* b, const float* sig_ms) {
  std::lock_guard<std::mutex> g(c->tim_mu);
  TimingRecord& t = c->tim;
  t.n = 0;
  c->last_lane = L.id;
  for (int q = 0; sig_ms && q < 2; q++) t.add(q ? "k_sig_finish" : "k_sig_prep", sig_ms[q], 0);
  t.add_marks(L.tl);
  const char* hn[8] = {"host_prep", "host_enqueue", "host_wait_flag", "host_parse", "host_stage", "host_misc",
                       "host_total", "host_stage_copy"};
  const float hv[8] = {L.host_prep_ms, L.host_enqueue_ms, L.host_wait_ms, L.host_parse_ms, L.host_stage_ms,
                       L.host_misc_ms, L.host_total_ms, L.host_stage_copy_ms};
  for (int q = 0; q < 8; q++) t.add(hn[q], hv[q], 0);
  if (b) b->tim = t;
}

// MSM plan for N real points on lane L's workspace (buffers grown as needed,
// window table uploaded on L.s).  Returns 0 or FTS_API_ENOMEM.
int msm_prepare(Lane& L, int N, MsmPlan& mp, int slot, int ch, bool local_sort, int maxc) {
  mp = MsmPlan{};
  msm_layout(N, mp, maxc);
  if (ch != MSM_CH) msm_set_chunk(mp, ch);
  mp.local_sort = local_sort;
  return msm_prepare_plan(L, mp, slot);
}
// buffers of an already laid-out plan (msm_layout / msm_layout_groups) on lane L.
// `slot` (< MSM_WIN_SLOTS) is the pinned source of the window-table upload: plans
// uploaded before the lane's next sync must use different slots (MSM_SLOT_*)
int msm_prepare_plan(Lane& L, MsmPlan& mp, int slot) {
  Workspace& w = L.ws;
  if (!w.m_choff.grow((size_t)mp.NB * 4) || !w.m_chbkt.grow((size_t)mp.NC * 4) ||
      !w.m_partials.grow((size_t)mp.NC * 96) || !w.m_keys.grow((size_t)mp.nw * mp.NV * 4) ||
      !w.m_counts.grow((size_t)mp.NB * 4) || !w.m_offsets.grow((size_t)mp.NB * 4) ||
      !w.m_cursor.grow((size_t)mp.nw * mp.NV * 4) || !w.m_sorted.grow((size_t)mp.nw * mp.NV * 4) ||
      !w.m_buckets.grow((size_t)mp.NB * 96) || !w.m_segs.grow((size_t)mp.NS * 96) ||
      !w.m_wins.grow((size_t)(mp.nw + 1) * 96) || !w.m_out.grow((size_t)mp.G * 96) ||
      !w.m_scratch.grow(std::max((size_t)mp.NS * 96, msm_scratch_words(mp) * 4)) || !w.m_win.grow(sizeof(mp.win)))
    return FTS_API_ENOMEM;
  mp.d_win = w.m_win.as<MsmWindow>();
  MsmWindow* src = L.pin->win[slot];
  memcpy(src, mp.win, sizeof(MsmWindow) * mp.nw);
  if (hipMemcpyAsync(mp.d_win, src, sizeof(MsmWindow) * mp.nw, hipMemcpyHostToDevice, L.s) != hipSuccess)
    return FTS_API_EDEVICE;
  mp.keys = w.m_keys.as<int32_t>();
  mp.counts = w.m_counts.as<uint32_t>();
  mp.offsets = w.m_offsets.as<uint32_t>();
  mp.cursor = w.m_cursor.as<uint32_t>();
  mp.sorted = w.m_sorted.as<uint32_t>();
  mp.buckets = w.m_buckets.as<uint32_t>();
  mp.segs = w.m_segs.as<uint32_t>();
  mp.wins = w.m_wins.as<uint32_t>();
  mp.out = w.m_out.as<uint32_t>();
  mp.chunk_off = w.m_choff.as<uint32_t>();
  mp.chunk_bkt = w.m_chbkt.as<int32_t>();
  mp.partials = w.m_partials.as<uint32_t>();
  mp.scratch = w.m_scratch.as<uint32_t>();
  return FTS_API_OK;
}

// workspace of a range-proof pass of B proofs (grow-only).  The pass's INPUT
// buffers (w.rp_* for gathered/action batches) belong to the caller, which
// fills them before rp_pipeline runs: they are never re-allocated here.
static int rp_buffers(fts_ctx* c, Lane& L, int B) {
  const int n = c->n, k = c->k, npts = rp_npts(k), N = B * npts;
  Workspace& w = L.ws;
  if (!w.pts.grow((size_t)B * npts * 64) || !w.ch.grow((size_t)B * rp_nch(k) * 32) ||
      !w.small.grow((size_t)B * (2 + k) * SMALL_SLOT) || !w.hpj.grow((size_t)B * (n + 1) * 96) ||
      !w.hpa.grow((size_t)B * (n + 1) * 64) || !w.hpbe.grow((size_t)B * (n + 1) * 64) ||
      !w.x0.grow((size_t)B * x0_var_bytes(n)) || !w.x0mid.grow((size_t)B * 32) || !w.terms.grow(rp_terms_words(B, n, k) * 4) ||
      !w.scratch.grow(std::max(rp_scratch_words(B, n, k), (size_t)B * 10 * 24) * 4) || !w.r_key.grow(32) ||
      !w.r_msc.grow((size_t)N * 32) || !w.r_coef.grow((size_t)B * RLC_NCOEF * 32) ||
      !w.r_colsum.grow(rlc_ncols(n) * 32 * (1 + 64))  /* + RQ_PARTS partial rows of column Q */ || !w.r_fixed.grow(rlc_ncols(n) * 96) || !w.r_flag.grow(4) || !w.ypow.grow((size_t)B * n * 32) ||
      !w.svec.grow((size_t)B * n * 32) || !w.zvec.grow((size_t)B * n * 32) || !w.rp_excl.grow((size_t)B * 4) ||
      !L.status_buf((size_t)B))
    return FTS_API_ENOMEM;
  return FTS_API_OK;
}

// size lane L's workspace for range-proof passes of up to B proofs; with
// inputs, also the pass-input buffers (w.rp_*) -- never from inside a pass,
// whose caller has already filled them
int lane_reserve(fts_ctx* c, Lane& L, int B, bool inputs) {
  const int npts = rp_npts(c->k);
  MsmPlan big{};
  if (int rc = msm_prepare(L, B * npts, big, MSM_SLOT_RESERVE, MSM_CH, c->msm_sort != 0, c->msm_maxc)) return rc;
  if (int rc = rp_buffers(c, L, B)) return rc;
  Workspace& w = L.ws;
  if (inputs && (!w.rp_raw.grow((size_t)B * npts * 64) || !w.rp_sc.grow((size_t)B * RP_NSC * 32) ||
                 !w.rp_status.grow((size_t)B * 4) || !w.rp_ipa.grow((size_t)B * 4)))
    return FTS_API_ENOMEM;
  L.presized = true;
  return FTS_API_OK;
}

// The batch check failed: find the failing proofs without re-checking the whole
// pass proof by proof ("fall back to per-proof checks
// (bisection)").  Round 1 tests groups of RP_GT1 consecutive proofs that never
// straddle two caller batches (`groups`: the batches' first proofs, the pass's
// end last); if more than RP_GT2_MIN proofs sit in failing groups, round 2 tests
// groups of RP_GT2 among them.  Every group test is ONE grouped MSM over the
// batch check's own weights.  The proofs of groups that do not close get the
// per-proof final equations (bulletproof.go:314-324, ipa.go:254-259), whose
// verdicts are the reference's.  A single bad proof costs one grouped MSM plus
// RP_GT1 per-proof checks, all of them in its own caller batch (RP_GT1, RP_GT2_MIN:
// fts_ctx::gt1, gt2_min).
constexpr int RP_GT2 = 8;
// dense[q] (caller batch q = [groups[q], groups[q+1])): its round-1 groups are of
// RP_GT2 proofs instead of gt1; with FTS_GT_ADAPT the flags are updated from this
// fallback's round-1 failures (a batch's own density).  An empty `dense` = all sparse.
// only (optional): only[q] != 0 for the caller batches whose own combination failed
// (the per-caller-batch main check): the others are decided and stay out of it
static int rp_group_fallback(fts_ctx* c, Lane& L, const RpBatchDev& d, const RlcDev& r,
                             const std::vector<int>& groups, std::vector<uint8_t>& dense,
                             const std::vector<uint8_t>* only = nullptr) {
  const bool adapt = c->gt_adapt && c->gt1 > RP_GT2;
  const int RP_GT2_MIN = c->gt2_min;
  const int B = d.B, n = d.n, npts = rp_npts(d.k);
  const size_t nb = groups.size() > 0 ? groups.size() - 1 : 0;
  dense.resize(nb, 0);
  Workspace& w = L.ws;
  L.tl.fallback();
  // round-1 selections, -1 padded: groups of gt1 over the sparse batches, of RP_GT2 over the dense ones
  std::vector<int32_t> sel_big, sel_small;
  for (size_t q = 0; q < nb; q++) {
    if (only && !(*only)[q]) continue;
    const bool small = adapt && dense[q];
    const int gs = small ? RP_GT2 : c->gt1;
    std::vector<int32_t>& sel = small ? sel_small : sel_big;
    for (int lo = groups[q]; lo < groups[q + 1]; lo += gs)
      for (int j = 0; j < gs; j++) sel.push_back(lo + j < groups[q + 1] ? lo + j : -1);
  }
  const size_t slots = std::max<size_t>(sel_big.size() + sel_small.size(), (size_t)B + RP_GT2);
  // groups of any round: round 1 has sel_big / gt1 + sel_small / RP_GT2, round 2 at most slots / RP_GT2
  const size_t gmax = std::max(sel_big.size() / c->gt1 + sel_small.size() / RP_GT2, (slots + RP_GT2 - 1) / RP_GT2);
  if (!w.r_sel.grow(2 * slots * 4) || !w.r_next.grow(slots * 4) || !w.r_cnt.grow(8) ||
      !w.r_gcol.grow(gmax * rlc_ncols(n) * 32) || !w.r_gfix.grow(gmax * rlc_ncols(n) * 96))
    return FTS_API_ENOMEM;
  uint8_t* hs = L.stage_buf((sel_big.size() + sel_small.size()) * 4);
  if (!hs) return FTS_API_ENOMEM;
  memcpy(hs, sel_big.data(), sel_big.size() * 4);
  memcpy(hs + sel_big.size() * 4, sel_small.data(), sel_small.size() * 4);
  int32_t* cur_big = w.r_sel.as<int32_t>();
  int32_t* cur_small = cur_big + sel_big.size();
  int32_t* nxt = w.r_next.as<int32_t>();
  uint32_t* cnt = w.r_cnt.as<uint32_t>();
  HIP_OK(hipMemcpyAsync(cur_big, hs, (sel_big.size() + sel_small.size()) * 4, hipMemcpyHostToDevice, L.s));
  HIP_OK(hipMemsetAsync(nxt, 0xff, slots * 4, L.s));  // -1: empty slots of the next round
  HIP_OK(hipMemsetAsync(cnt, 0, 4, L.s));
  // one grouped test per group size; both append their failing proofs to nxt
  auto group_test = [&](const int32_t* sel, int G, int gs) -> int {
    if (G == 0) return FTS_API_OK;
    MsmPlan gp{};
    msm_layout_groups(G * gs * npts, G, gs * npts, gp, c->msm_maxc);
    gp.local_sort = c->msm_sort != 0;  // FTS_MSM_SORT covers the group tests' MSMs too
    gp.sel = sel;
    gp.sel_pts = npts;
    if (int rc = msm_prepare_plan(L, gp, gs == RP_GT2 ? MSM_SLOT_GT_SMALL : MSM_SLOT_GT_BIG)) return rc;
    launch_rlc_group_test(d, r, c->d_tables.as<uint32_t>(), gp, sel, G, gs, w.r_gcol.as<uint32_t>(), w.r_gfix.as<uint32_t>(), nxt,
                          cnt, L.s, &L.tl);
    HIP_OK(hipGetLastError());
    return FTS_API_OK;
  };
  if (int rc = group_test(cur_big, (int)(sel_big.size() / c->gt1), c->gt1)) return rc;
  if (int rc = group_test(cur_small, (int)(sel_small.size() / RP_GT2), RP_GT2)) return rc;
  HIP_OK(hipMemcpyAsync(&L.pin->flag, cnt, 4, hipMemcpyDeviceToHost, L.s));
  HIP_OK(L.sync());
  const int nfail = L.pin->flag;
  if (adapt && nfail > 0) {
    // each batch's own density from its failing round-1 proofs
    int32_t* hf = L.status_buf((size_t)nfail);
    if (!hf) return FTS_API_ENOMEM;
    HIP_OK(hipMemcpyAsync(hf, nxt, (size_t)nfail * 4, hipMemcpyDeviceToHost, L.s));
    HIP_OK(L.sync());
    std::vector<int> fails(nb, 0);
    for (int i = 0; i < nfail; i++) {
      const size_t q = (size_t)(std::upper_bound(groups.begin(), groups.end(), hf[i]) - groups.begin()) - 1;
      if (q < nb) fails[q]++;
    }
    for (size_t q = 0; q < nb; q++) {
      const int sz = groups[q + 1] - groups[q];
      if (only && !(*only)[q]) dense[q] = 0;  // its combination closed: no bad proof
      else dense[q] = dense[q] ? fails[q] > 0.02 * sz : fails[q] > 0.5 * sz;
    }
  } else if (adapt) {
    std::fill(dense.begin(), dense.end(), 0);
  }
  if (nfail == 0) return FTS_API_OK;
  // per-proof checks of what is left; a second group test only pays when round 1
  // left many proofs in large groups (the per-proof check's latency is one GLV
  // chain whatever their number, its work grows with it)
  if (sel_big.empty() || nfail <= RP_GT2_MIN) {
    c->st_rp_perproof += nfail;
    launch_rp_fallback(d, c->d_tables.as<uint32_t>(), nxt, nfail, L.s, &L.tl);
    HIP_OK(hipGetLastError());
    return FTS_API_OK;
  }
  int32_t* cur = w.r_sel.as<int32_t>();  // round 2 over the survivors, groups of RP_GT2
  HIP_OK(hipMemcpyAsync(cur, nxt, slots * 4, hipMemcpyDeviceToDevice, L.s));
  HIP_OK(hipMemsetAsync(nxt, 0xff, slots * 4, L.s));
  HIP_OK(hipMemsetAsync(cnt, 0, 4, L.s));
  const int G2 = (nfail + RP_GT2 - 1) / RP_GT2;
  if ((size_t)G2 > gmax) return FTS_API_EINVAL;  // cannot happen: nfail <= B
  if (int rc = group_test(cur, G2, RP_GT2)) return rc;
  HIP_OK(hipMemcpyAsync(&L.pin->flag, cnt, 4, hipMemcpyDeviceToHost, L.s));
  HIP_OK(L.sync());
  const int nfail2 = L.pin->flag;
  if (nfail2 == 0) return FTS_API_OK;
  c->st_rp_perproof += nfail2;
  launch_rp_fallback(d, c->d_tables.as<uint32_t>(), nxt, nfail2, L.s, &L.tl);
  HIP_OK(hipGetLastError());
  return FTS_API_OK;
}

// One range-proof pass enqueued on a lane (rp_enqueue), finished by rp_finish.
struct RpPass {
  RpBatchDev d{};
  RlcDev r{};
  std::vector<int> groups;
  std::vector<uint8_t> dense;  // per caller batch (groups[q] .. groups[q+1]): round-1 groups of 8; updated by the fallback
  double t_start = 0, t_prep = 0, t_enq = 0;
  bool tl_started = false;
  std::vector<fts_rp_batch*> bats;  // the caller batches of the pass (groups order); empty: none
  bool clean = false;               // the combination closed: no fallback ran (rp_finish)
  int located = -1;                 // the locator: 1 hit, 0 missed, -1 not run  // the lane's timeline was begun by the caller (action passes: gather + sigma marks)
};

// Range-proof pipeline on B proofs already on the device: exact phase, RLC
// batch check, and (rp_finish) the group-test fallback when the combination
// fails.  `between` (optional) is launched after the RLC check and before the
// flag sync (the sigma-proof kernels of transfer/issue batches).
// `groups`: first proof of every caller batch in the pass, then B ({0, B}: one batch)
// `pre_rlc` (optional): launched on the batch check's stream (lane s3) right before k_rlc_prep
template <class F>
static int rp_enqueue(fts_ctx* c, Lane& L, int B, uint8_t* d_raw, uint32_t* d_sc, int32_t* d_status, int32_t* d_ipa,
                      F&& between, const std::vector<int>& groups, RpPass& P,
                      void (*pre_rlc)(void*, hipStream_t) = nullptr, void* pre_rlc_arg = nullptr) {
  const int n = c->n, k = c->k, npts = rp_npts(k);
  Workspace& w = L.ws;
  const int N = B * npts;
  P.t_start = now_ms();
  P.groups = groups;
  // first range-proof pass of this lane: size the workspace for the largest
  // coalesced pass at once (no re-allocation, i.e. no device-wide sync, later)
  if (!L.presized && c->coalesce_max > (size_t)B && c->coalesce_max <= (1u << 20))
    if (int rc = lane_reserve(c, L, (int)c->coalesce_max, false)) return rc;
  MsmPlan mp{};
  // the per-caller-batch combination: G groups of gs proof slots (padding -1)
  const int G = (int)groups.size() - 1;
  const bool grouped = c->main_groups && G > 1 && G <= RP_GATHER_MAX && !pre_rlc;
  int gs = 0;
  if (grouped) {
    for (int q = 0; q < G; q++) gs = std::max(gs, groups[q + 1] - groups[q]);
    msm_layout_groups(G * gs * npts, G, gs * npts, mp, c->msm_maxc);
    mp.local_sort = c->msm_sort != 0;
    Workspace& w0 = L.ws;
    const size_t NC = rlc_ncols(n);
    if (!w0.r_msel.grow((size_t)G * gs * 4) || !w0.r_mcol.grow((size_t)G * NC * 32) ||
        !w0.r_mfix.grow((size_t)G * NC * 96) || !w0.r_mqfix.grow((size_t)G * NC * 96) ||
        !w0.r_mflag.grow((size_t)G * 4))
      return FTS_API_ENOMEM;
    int32_t* hs = L.sel_buf((size_t)G * gs);
    if (!hs) return FTS_API_ENOMEM;
    for (int q = 0; q < G; q++)
      for (int j = 0; j < gs; j++) hs[(size_t)q * gs + j] = groups[q] + j < groups[q + 1] ? groups[q] + j : -1;
    HIP_OK(hipMemcpyAsync(w0.r_msel.p, hs, (size_t)G * gs * 4, hipMemcpyHostToDevice, L.s));
    // equal caller batches (the usual coalesced pass): slot = proof, no indirection in
    // the MSM's point gathers
    bool uniform = true;
    for (int q = 0; q < G; q++) uniform = uniform && groups[q] == q * gs;
    mp.sel = uniform && groups[G] == G * gs ? nullptr : w0.r_msel.as<int32_t>();
    mp.sel_pts = npts;
    if (int rc = msm_prepare_plan(L, mp, MSM_SLOT_PASS)) return rc;
  } else if (int rc = msm_prepare(L, N, mp, MSM_SLOT_PASS, MSM_CH, c->msm_sort != 0, c->msm_maxc)) {
    return rc;
  }
  if (int rc = rp_buffers(c, L, B)) return rc;
  RpBatchDev d{B,
               n,
               k,
               d_raw,
               d_sc,
               d_status,
               d_ipa,
               w.pts.as<uint32_t>(),
               w.ch.as<uint32_t>(),
               w.small.as<uint8_t>(),
               w.hpj.as<uint32_t>(),
               w.hpa.as<uint32_t>(),
               w.hpbe.as<uint8_t>(),
               w.x0.as<uint8_t>(),
               w.terms.as<uint32_t>(),
               w.scratch.as<uint32_t>(),
               w.ypow.as<uint32_t>(),
               w.svec.as<uint32_t>(),
               w.zvec.as<uint32_t>(),
               nullptr,
               nullptr,
               (size_t)B <= c->com_fixed_max && L.alone ? 1 : 0};
  d.pre_rlc = pre_rlc;
  d.pre_rlc_arg = pre_rlc_arg;
  // 2 (adaptive): 0 on the latency path, 1 on the work path; 3: 0 on the latency
  // path, on the work path the MSM's sort beside the fixed-base launch
  d.rlc_fork = c->rlc_fork == 2 ? (d.com_fixed ? 0 : 1) : c->rlc_fork >= 3 ? (d.com_fixed ? 0 : c->rlc_fork) : c->rlc_fork;
  d.ev_coef = L.ev_c;
  d.ev_fx = L.ev_d;
  // x0 prefix beside the com chain (work path) or com_tree (latency path; round 2
  // measured that slower, 3.51 vs 3.06 ms, when the normalisation did not yet write
  // the H' records and the prefix waited for a separate build)
  d.x0_mid = (c->x0_split & (d.com_fixed ? 2 : 1)) ? w.x0mid.as<uint32_t>() : nullptr;
  d.excl = pre_rlc ? w.rp_excl.as<int32_t>() : nullptr;
  RlcDev r{w.r_key.as<uint32_t>(), w.r_msc.as<uint32_t>(),   w.r_coef.as<uint32_t>(), w.r_colsum.as<uint32_t>(),
           w.r_fixed.as<uint32_t>(), w.r_flag.as<int32_t>(), w.m_scratch.as<uint32_t>(), mp};
  if (grouped) {
    r.G = G;
    r.gs = gs;
    r.sel = w.r_msel.as<int32_t>();
    r.gcol = w.r_mcol.as<uint32_t>();
    r.gfix = w.r_mfix.as<uint32_t>();
    r.gqfix = w.r_mqfix.as<uint32_t>();
    r.gflag = w.r_mflag.as<int32_t>();
  }
  // fresh RLC weights key (getrandom), unpredictable to the provers
  if (getrandom(L.pin->key, sizeof L.pin->key, 0) != (ssize_t)sizeof L.pin->key) return FTS_API_EDEVICE;
  HIP_OK(hipMemcpyAsync(r.key, L.pin->key, sizeof L.pin->key, hipMemcpyHostToDevice, L.s));
  P.t_prep = now_ms();
  if (!P.tl_started) L.tl.begin(L.s);
  if (c->fx_serial) {
    // the wait, this pass's fixed-base launch and its event record are enqueued in
    // one critical section, so the chain of events follows the enqueue order
    std::lock_guard<std::mutex> g(c->fx_mu);
    d.fx_wait = c->fx_last;
    launch_rp_batch(d, r, c->d_tables.as<uint32_t>(), c->d_wtables.as<uint32_t>(), c->d_x0const.as<uint8_t>(), c->d_x0tmpl.as<uint8_t>(), L.s, L.s2, L.s3, L.s4, &L.tl,
                    c->wbits);
    c->fx_last = d.ev_fx;
  } else {
    launch_rp_batch(d, r, c->d_tables.as<uint32_t>(), c->d_wtables.as<uint32_t>(), c->d_x0const.as<uint8_t>(), c->d_x0tmpl.as<uint8_t>(), L.s, L.s2, L.s3, L.s4, &L.tl,
                    c->wbits);
  }
  between();
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(&L.pin->flag, r.flag, 4, hipMemcpyDeviceToHost, L.s));
  if (grouped) HIP_OK(hipMemcpyAsync(L.pin->gflag, r.gflag, (size_t)G * 4, hipMemcpyDeviceToHost, L.s));
  P.t_enq = now_ms();
  P.d = d;
  P.r = r;
  return FTS_API_OK;
}

// The single-fault locator (rp_rlc.hip k_rlc_locate): S' = (j + 1) S locates
// the one bad proof j of a failed combination S.  Its per-proof final equations
// give its verdict (bulletproof.go:314-324, ipa.go:254-259), and every other proof
// is accepted -- the combination of the others is S - rho_j E_j = 0 with the
// batch check's own soundness.  -> 1 decided, 0 not a single fault (the group test
// decides), < 0 an API error.  The workspace's weights are index-weighted after it,
// which the group test accepts as its weights (any fresh random weights do).
static int rp_locate_single(fts_ctx* c, Lane& L, RpPass& P) {
  const int B = P.d.B;
  Workspace& w = L.ws;
  if (!w.r_loc.grow(4) || !w.r_save.grow(96)) return FTS_API_ENOMEM;
  L.tl.fallback();
  int32_t* loc = w.r_loc.as<int32_t>();
  HIP_OK(hipMemsetAsync(loc, 0xff, 4, L.s));
  launch_rlc_locate(P.d, P.r, c->d_tables.as<uint32_t>(), w.r_save.as<uint32_t>(), loc, L.s, &L.tl);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(&L.pin->flag, loc, 4, hipMemcpyDeviceToHost, L.s));
  HIP_OK(L.sync());
  const int i = L.pin->flag;
  if (i < 0 || i >= B) return 0;
  c->st_rp_perproof += 1;
  launch_rp_fallback(P.d, c->d_tables.as<uint32_t>(), loc, 1, L.s, &L.tl);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(&L.pin->flag, P.d.status + i, 4, hipMemcpyDeviceToHost, L.s));
  HIP_OK(L.sync());
  if (L.pin->flag == FTS_OK) return 0;  // not a fault after all: the group test decides
  launch_rlc_accept_except(B, i, P.d.status, P.d.ipa_flag, L.s);
  HIP_OK(hipGetLastError());
  c->st_rp_located++;
  std::fill(P.dense.begin(), P.dense.end(), 0);
  return 1;
}

// wait for an enqueued pass; on a failed combination, the single-fault locator,
// then (several bad proofs) the group-test fallback
static int rp_finish(fts_ctx* c, Lane& L, RpPass& P) {
  HIP_OK(L.sync());
  const double t_wait = now_ms();
  L.host_prep_ms = (float)(P.t_prep - P.t_start);
  L.host_enqueue_ms = (float)(P.t_enq - P.t_prep);
  L.host_wait_ms = (float)(t_wait - P.t_enq);
  const int32_t flag = L.pin->flag;
  c->st_rp_passes++;
  P.clean = flag != 0;
  if (flag) return FTS_API_OK;
  c->st_rp_failed++;
  if (P.r.G > 1) {  // per-caller-batch combination: only the failing batches go to the group test
    std::vector<uint8_t> only((size_t)P.r.G, 0);
    for (int q = 0; q < P.r.G; q++) only[q] = L.pin->gflag[q] ? 0 : 1;
    return rp_group_fallback(c, L, P.d, P.r, P.groups, P.dense, &only);
  }
  if (c->locate && P.d.B > 1 && std::none_of(P.dense.begin(), P.dense.end(), [](uint8_t x) { return x != 0; })) {
    // a batch of the pass still in its backoff skips the locator for the whole pass
    bool skip = false;
    for (fts_rp_batch* b : P.bats)
      if (b->locate_skip > 0) {
        b->locate_skip--;
        skip = true;
      }
    if (!skip) {
      const int rc = rp_locate_single(c, L, P);
      if (rc < 0) return rc;
      P.located = rc;
      if (rc == 1) {
        for (fts_rp_batch* b : P.bats) b->locate_backoff = 8;
        return FTS_API_OK;
      }
      // missed: the batches holding bad proofs back off once the verdicts are in (run_rp_groups)
    }
  }
  return rp_group_fallback(c, L, P.d, P.r, P.groups, P.dense);
}

template <class F>
static int rp_pipeline(fts_ctx* c, Lane& L, int B, uint8_t* d_raw, uint32_t* d_sc, int32_t* d_status, int32_t* d_ipa,
                       F&& between, const std::vector<int>& groups, void (*pre_rlc)(void*, hipStream_t) = nullptr,
                       void* pre_rlc_arg = nullptr) {
  RpPass P;
  if (int rc = rp_enqueue(c, L, B, d_raw, d_sc, d_status, d_ipa, between, groups, P, pre_rlc, pre_rlc_arg)) return rc;
  return rp_finish(c, L, P);
}

// Device passes over groups of staged batches, group j on lanes[j] (the
// dispatcher passes one group; several are enqueued back to back before any is
// waited for): a single batch runs in place; several are gathered (D2D) into the
// lane's contiguous input buffers, verified as one batch, and their verdicts
// scattered back.  rc[j] is the status of group j's requests.  (Round 4 measured
// staggered sub-passes of one coalesced group -- sub-pass j's fixed-base launch
// after sub-pass j-1's -- and dropped them: 20-batch bursts 3.77-3.89 vs 3.95-3.97
// M rp64/s as one pass)
// the pre_rlc hook of a pass with action calls: wait for their sigma equations, then
// exclude the range proofs of actions whose sigma proof failed (pass offsets `off`)
struct SigHook {
  Lane* L = nullptr;
  std::vector<const SigBatchDev*> sig;
  std::vector<int> off;  // first range proof of the call in the pass (-1: none)
  std::vector<hipEvent_t> ev;  // the call's sigma-done event (its slot's ev_sig[2])
};

static void run_rp_groups(fts_ctx* c, const std::vector<Lane*>& lanes, const std::vector<std::vector<RpReq*>>& sub,
                             std::vector<int>& rc) {
  const size_t m = sub.size();
  const int npts = rp_npts(c->k);
  std::vector<RpPass> P(m);
  std::vector<int32_t*> d_status(m, nullptr);
  std::vector<size_t> Bs(m, 0);
  rc.assign(m, FTS_API_OK);
  // per group: its requests with range proofs (the caller batches of the pass, in
  // pass order), their first proof, and the sigma-exclusion hook of its action calls
  std::vector<std::vector<RpReq*>> rpq(m);
  std::vector<std::vector<int>> first(m);
  std::vector<SigHook> hooks(m);
  std::vector<uint8_t> sig_only(m, 0);
  for (size_t j = 0; j < m; j++) {
    Lane& L = *lanes[j];
    const std::vector<RpReq*>& grp = sub[j];
    for (RpReq* q : grp)
      if (q->b->B > 0) rpq[j].push_back(q);
    auto enq = [&]() -> int {
      if (grp.size() == 1 && !grp[0]->act) {
        fts_rp_batch* b = grp[0]->b;
        HIP_OK(hipMemcpyAsync(b->status, b->status0, (size_t)b->B * 4, hipMemcpyDeviceToDevice, L.s));
        Bs[j] = (size_t)b->B;
        d_status[j] = b->status;
        first[j] = {0};
        return rp_enqueue(c, L, b->B, b->raw, b->sc, b->status, b->ipa_flag, [] {}, std::vector<int>{0, b->B}, P[j],
                          nullptr, nullptr);
      }
      size_t B = 0;
      for (RpReq* q : rpq[j]) B += (size_t)q->b->B;
      Workspace& w = L.ws;
      L.tl.begin(L.s);  // the gather on the pass's timeline
      P[j].tl_started = true;
      // the action calls' sigma decode (their slots' streams, since staging) wrote the
      // V slots of their range proofs: the gather waits for that part only; the sigma
      // equations are waited for by the exclusion hook, on the batch check's stream
      for (RpReq* q : grp)
        if (q->act) HIP_OK(hipStreamWaitEvent(L.s, q->act->ev_sig[1], 0));
      RpGather g{};
      if (B > 0) {
        const size_t Bal = std::max(B, std::min(c->coalesce_max, (size_t)1 << 20));  // sized once for the largest pass
        if (!w.rp_raw.grow(Bal * npts * 64) || !w.rp_sc.grow(Bal * RP_NSC * 32) || !w.rp_status.grow(Bal * 4) ||
            !w.rp_ipa.grow(Bal * 4))
          return FTS_API_ENOMEM;
        g.G = (int)rpq[j].size();
        size_t off = 0;
        for (int i = 0; i < g.G; i++) {
          const fts_rp_batch* b = rpq[j][i]->b;
          g.raw[i] = b->raw;
          g.sc[i] = b->sc;
          g.status0[i] = b->status0;
          g.ipa[i] = b->ipa_flag;
          g.off[i] = (int)off;
          first[j].push_back((int)off);
          off += (size_t)b->B;
        }
        g.off[g.G] = (int)off;
        launch_rp_gather(g, c->k, w.rp_raw.as<uint8_t>(), w.rp_sc.as<uint32_t>(), w.rp_status.as<int32_t>(),
                         w.rp_ipa.as<int32_t>(), L.s);
        L.tl.mark("k_rp_gather", L.s, 0);
      }
      Bs[j] = B;
      d_status[j] = w.rp_status.as<int32_t>();
      // the batch check's variable part drops the range proofs of actions whose sigma
      // proof failed (k_sig_exclude at the call's pass offset, on the check's stream, which
      // follows the main stream and so the sigma events)
      SigHook& h = hooks[j];
      h.L = &L;
      for (RpReq* q : grp) {
        if (!q->act || q->act->sd.A == 0) continue;
        int off = -1;
        for (size_t i = 0; i < rpq[j].size(); i++)
          if (rpq[j][i] == q) off = first[j][i];
        h.sig.push_back(&q->act->sd);
        h.off.push_back(off);
        h.ev.push_back(q->act->ev_sig[2]);
      }
      if (B == 0) {  // sigma proofs only: nothing left for the pass but the verdicts
        sig_only[j] = 1;
        for (hipEvent_t e : h.ev) HIP_OK(hipStreamWaitEvent(L.s, e, 0));
        return FTS_API_OK;
      }
      void (*pre)(void*, hipStream_t) = nullptr;
      if (!h.sig.empty()) {
        pre = [](void* arg, hipStream_t s) {
          SigHook* hk = static_cast<SigHook*>(arg);
          // the mask is read at launch time: rp_enqueue sizes (and may re-allocate) it
          for (size_t i = 0; i < hk->sig.size(); i++) {
            (void)hipStreamWaitEvent(s, hk->ev[i], 0);  // the call's sigma verdicts
            if (hk->off[i] >= 0) launch_sig_exclude(*hk->sig[i], hk->L->ws.rp_excl.as<int32_t>() + hk->off[i], s);
          }
        };
      }
      std::vector<int> groups = first[j];
      groups.push_back((int)B);
      return rp_enqueue(c, L, (int)B, w.rp_raw.as<uint8_t>(), w.rp_sc.as<uint32_t>(), w.rp_status.as<int32_t>(),
                        w.rp_ipa.as<int32_t>(), [] {}, groups, P[j], pre, pre ? &h : nullptr);
    };
    rc[j] = enq();
    // the verdicts' downloads behind the pass, before its flag is read: a clean pass
    // (no fallback) needs no second round trip (fin re-downloads after a fallback)
    if (rc[j] == FTS_API_OK && !sig_only[j]) {
      int32_t* pst = L.status_buf(std::max<size_t>(Bs[j], 1));
      if (!pst) {
        rc[j] = FTS_API_ENOMEM;
      } else {
        if (Bs[j] && hipMemcpyAsync(pst, d_status[j], Bs[j] * 4, hipMemcpyDeviceToHost, L.s) != hipSuccess)
          rc[j] = FTS_API_EDEVICE;
        for (RpReq* q : grp)
          if (q->act && q->act->sd.A &&
              hipMemcpyAsync(q->act->sig_res, q->act->sd.status, (size_t)q->act->sd.A * 4, hipMemcpyDeviceToHost,
                             L.s) != hipSuccess)
            rc[j] = FTS_API_EDEVICE;
      }
    }
    for (RpReq* q : rpq[j]) {
      P[j].dense.push_back(q->b->dense ? 1 : 0);
      P[j].bats.push_back(q->b);
    }
  }
  for (size_t j = 0; j < m; j++) {
    Lane& L = *lanes[j];
    if (rc[j] != FTS_API_OK) {
      (void)L.sync();  // drain whatever was enqueued before the failure
      continue;
    }
    auto fin = [&]() -> int {
      if (!sig_only[j]) {
        if (int r = rp_finish(c, L, P[j])) return r;
        for (size_t q = 0; q < rpq[j].size() && q < P[j].dense.size(); q++) rpq[j][q]->b->dense = P[j].dense[q] != 0;
      }
      int32_t* pst = L.status_buf(std::max<size_t>(Bs[j], 1));
      if (!pst) return FTS_API_ENOMEM;
      if (!P[j].clean) {  // a fallback (or a sigma-only pass) ran after the early downloads
        if (Bs[j]) HIP_OK(hipMemcpyAsync(pst, d_status[j], Bs[j] * 4, hipMemcpyDeviceToHost, L.s));
        for (RpReq* q : sub[j])
          if (q->act && q->act->sd.A)
            HIP_OK(hipMemcpyAsync(q->act->sig_res, q->act->sd.status, (size_t)q->act->sd.A * 4, hipMemcpyDeviceToHost,
                                  L.s));
        HIP_OK(L.sync());
      }
      for (size_t i = 0; i < rpq[j].size(); i++) {
        RpReq* q = rpq[j][i];
        const int32_t* v = pst + first[j][i];
        if (q->status) memcpy(q->status, v, (size_t)q->b->B * 4);
        if (P[j].located == 0 && std::any_of(v, v + q->b->B, [](int32_t x) { return x != 0; })) {
          q->b->locate_skip = q->b->locate_backoff;  // a batch of a multi-fault pass that holds bad proofs
          q->b->locate_backoff = std::min(2 * q->b->locate_backoff, 256);
        }
      }
      // host-side timings of the pass: the first action call's parse and staging
      for (RpReq* q : sub[j])
        if (q->act) {
          L.host_parse_ms = q->act->parse_ms;
          L.host_stage_ms = q->act->stage_ms;
          break;
        }
      // the sigma kernels of the pass's first action call (its slot's stream), beside
      const ActSlot* sa = nullptr;
      for (RpReq* q : sub[j])
        if (q->act && q->act->sd.A) {
          sa = q->act;
          break;
        }
      float sig_ms[2] = {0, 0};
      if (sa) {
        (void)hipEventElapsedTime(&sig_ms[0], sa->ev_sig[0], sa->ev_sig[1]);
        (void)hipEventElapsedTime(&sig_ms[1], sa->ev_sig[1], sa->ev_sig[2]);
      }
      for (RpReq* q : sub[j]) {
        collect_timings(c, L, q->b, sa ? sig_ms : nullptr);
        q->b->merged = (int)sub[j].size();
      }
      return FTS_API_OK;
    };
    rc[j] = fin();
  }
}

extern "C" {

// debug/parity hook: intermediates of proof i of the last range-proof run
//   ch_out: (8 + 2k) x 32 bytes canonical BE Fr  [x, x^2, y, y^-1, z, z^2, polEval, x0, x_j.., x_j^-1..]
//   com_out: 64 bytes com (BE) ; hp_out: n x 64 bytes H'_i (BE)
int fts_debug_rp_intermediates(fts_ctx* c, size_t i, uint8_t* ch_out, uint8_t* com_out, uint8_t* hp_out) {
  if (c && !c->shards.empty()) return fts_debug_rp_intermediates(c->shards[0], i, ch_out, com_out, hp_out);
  if (!c || c->device < 0) return FTS_API_EINVAL;
  int want;
  {
    std::lock_guard<std::mutex> g(c->tim_mu);
    want = c->last_lane;
  }
  LaneGuard lg(c, want);
  Workspace& ws = lg.L->ws;
  HIP_OK(hipSetDevice(c->device));
  const int n = c->n, k = c->k, nch = rp_nch(k);
  if (ch_out) {
    std::vector<uint32_t> ch(nch * 8);
    HIP_OK(hipMemcpy(ch.data(), ws.ch.as<uint32_t>() + i * nch * 8, nch * 32, hipMemcpyDeviceToHost));
    for (int q = 0; q < nch; q++) {
      Fr m;
      memcpy(m.v, &ch[q * 8], 32);
      fr_to_be(m, ch_out + 32 * q);
    }
  }
  if (com_out) HIP_OK(hipMemcpy(com_out, ws.hpbe.as<uint8_t>() + (i * (n + 1) + n) * 64, 64, hipMemcpyDeviceToHost));
  if (hp_out) HIP_OK(hipMemcpy(hp_out, ws.hpbe.as<uint8_t>() + i * (n + 1) * 64, n * 64, hipMemcpyDeviceToHost));
  return FTS_API_OK;
}

// debug: bucket-occupancy statistics of the last RLC MSM
// out[0] = max bucket count, out[1] = its bucket index, out[2] = NB, out[3] = #nonzero buckets
int fts_debug_msm_stats(fts_ctx* c, int64_t* out) {
  if (c && !c->shards.empty()) return fts_debug_msm_stats(c->shards[0], out);
  if (!c || c->device < 0 || !out) return FTS_API_EINVAL;
  int want;
  {
    std::lock_guard<std::mutex> g(c->tim_mu);
    want = c->last_lane;
  }
  LaneGuard lg(c, want);
  Workspace& ws = lg.L->ws;
  size_t nb = ws.m_counts.cap / 4;
  std::vector<uint32_t> cnt(nb);
  HIP_OK(hipMemcpy(cnt.data(), ws.m_counts.p, nb * 4, hipMemcpyDeviceToHost));
  size_t arg = 0, nz = 0;
  for (size_t i = 0; i < nb; i++) {
    if (cnt[i] > cnt[arg]) arg = i;
    nz += cnt[i] != 0;
  }
  out[0] = cnt[arg];
  out[1] = (int64_t)arg;
  out[2] = (int64_t)nb;
  out[3] = (int64_t)nz;
  return FTS_API_OK;
}

int fts_rp_batch_stage(fts_ctx* c, size_t n, const uint8_t* const* rp_der, const size_t* rp_len, const uint8_t* com64,
                       fts_rp_batch** out) {
  if (!c || !out || (n && (!rp_der || !rp_len || !com64))) return FTS_API_EINVAL;
  if (!c->shards.empty()) {  // one child batch per device, contiguous shards
    std::unique_ptr<fts_rp_batch> b(new fts_rp_batch());
    b->B = (int)n;
    b->device = c->device;
    b->bounds = plan(n, nullptr, (int)c->shards.size());
    b->parts.assign(c->shards.size(), nullptr);
    b->part_ctx = c->shards;
    int rc = run_shards(b->bounds, [&](int j, size_t lo, size_t hi) {
      return fts_rp_batch_stage(c->shards[j], hi - lo, rp_der + lo, rp_len + lo, com64 + 64 * lo, &b->parts[j]);
    });
    if (rc != FTS_API_OK) return rc;
    *out = b.release();
    return FTS_API_OK;
  }
  if (c->device < 0) return FTS_API_EDEVICE;
  HIP_OK(hipSetDevice(c->device));
  RpHost h;
  parse_rp_batch(c->k, n, rp_der, rp_len, com64, h);
  std::unique_ptr<fts_rp_batch> b(new fts_rp_batch());  // every early return releases it
  b->B = (int)n;
  b->device = c->device;
  size_t nb = std::max<size_t>(n, 1);
  if (!b->raw_mem.reserve(std::max<size_t>(h.raw.size(), 64)) ||
      !b->sc_mem.reserve(std::max<size_t>(h.sc.size() * 4, 32)) || !b->status0_mem.reserve(nb * 4) ||
      !b->status_mem.reserve(nb * 4) || !b->ipa_mem.reserve(nb * 4))
    return FTS_API_ENOMEM;
  b->raw = b->raw_mem.as<uint8_t>();
  b->sc = b->sc_mem.as<uint32_t>();
  b->status0 = b->status0_mem.as<int32_t>();
  b->status = b->status_mem.as<int32_t>();
  b->ipa_flag = b->ipa_mem.as<int32_t>();
  if (n) {
    HIP_OK(hipMemcpy(b->raw, h.raw.data(), h.raw.size(), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(b->sc, h.sc.data(), h.sc.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(b->status0, h.status.data(), n * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(b->ipa_flag, h.ipa.data(), n * 4, hipMemcpyHostToDevice));
  }
  *out = b.release();
  return FTS_API_OK;
}

int fts_rp_batch_verify(fts_ctx* c, fts_rp_batch* b, int32_t* status) {
  if (!c || !b) return FTS_API_EINVAL;
  if (!b->parts.empty()) {
    if (c->shards != b->part_ctx) return FTS_API_EINVAL;  // staged on another context
    int m = 0;
    int rc = run_shards(b->bounds, [&](int j, size_t lo, size_t hi) {
      return fts_rp_batch_verify(c->shards[j], b->parts[j], status ? status + lo : nullptr);
    });
    for (fts_rp_batch* q : b->parts)
      if (q) m = std::max(m, q->merged);
    b->merged = m;
    return rc;
  }
  if (c->device < 0) return FTS_API_EDEVICE;
  if (b->B == 0) return FTS_API_OK;
  HIP_OK(hipSetDevice(c->device));
  RpReq me(b, status);
  return rp_dispatch(c, me);
}

}  // extern "C"

// Work-sharing dispatcher: the request joins the pending queue; any waiting
// caller that finds a free lane takes the queue's head group (FIFO, up to
// coalesce_max proofs) and runs it as ONE device pass, so batches submitted
// while the lanes are busy are merged (a 4,096-proof batch alone fills only
// 64 waves in the per-proof chain kernels).  Verdicts stay per proof.  Staged
// range-proof batches and action calls share the queue and the passes.
int rp_dispatch(fts_ctx* c, RpReq& me) {
  fts_rp_batch* b = me.b;
  std::unique_lock<std::mutex> lk(c->mu);
  c->rp_pending.push_back(&me);
  c->pending_proofs += (size_t)b->B;
  // a lone arrival: nothing else arrived within the quiet gap before it
  const bool lone = me.arrived - c->last_arrival > std::chrono::microseconds(c->idle_quiet_us);
  c->last_arrival = me.arrived;
  c->arrivals++;
  // enough queued for a full pass: the head stops gathering
  if (c->pending_proofs >= c->gather_target && c->rp_pending.front() != &me) c->rp_pending.front()->cv.notify_one();
  if (c->hold_n > 0 && (int)c->rp_pending.size() >= c->hold_n) {  // test hook: release the held queue
    c->hold_n = 0;
    for (RpReq* q : c->rp_pending) q->cv.notify_one();
  }
  while (!me.done) {
    if (c->free_lanes.empty() || c->rp_pending.empty() || c->hold_n > 0) {
      me.cv.wait(lk);
      continue;
    }
    const bool device_busy = c->free_lanes.size() < c->lanes.size();
    const int wait_us = device_busy ? c->gather_us : c->idle_gather_us;
    if (wait_us > 0 && c->rp_pending.front() == &me && c->pending_proofs < c->gather_target) {
      auto deadline = me.arrived + std::chrono::microseconds(wait_us);
      if (!device_busy) {  // idle: only while the burst is still arriving
        deadline = std::min(deadline, c->last_arrival + std::chrono::microseconds(c->idle_quiet_us));
        if (lone && c->rp_pending.size() == 1) {
          // a lone caller: a short spin for company, then go (no wake-up latency)
          deadline = std::min(deadline, me.arrived + std::chrono::microseconds(c->idle_first_us));
          if (std::chrono::steady_clock::now() < deadline) {
            const uint64_t a0 = c->arrivals.load();
            lk.unlock();
            while (std::chrono::steady_clock::now() < deadline && c->arrivals.load() == a0) std::this_thread::yield();
            lk.lock();
            continue;
          }
        }
      }
      if (std::chrono::steady_clock::now() < deadline) {
        me.cv.wait_until(lk, deadline);
        continue;
      }
    }
    if (c->rp_pending.front() != &me && !me.done) {  // only the head leads a pass
      c->rp_pending.front()->cv.notify_one();
      me.cv.wait(lk);
      continue;
    }
    Lane* L = c->lanes[c->free_lanes.back()].get();
    c->free_lanes.pop_back();
    L->alone = c->free_lanes.size() + 1 == c->lanes.size();
    // an idle device's first pass stops at gather_target proofs (the rest of the
    // burst forms the next pass on another lane)
    const size_t cap = L->alone ? std::min(c->coalesce_max, std::max<size_t>(c->gather_target, 1)) : c->coalesce_max;
    std::vector<RpReq*> grp;
    size_t tot = 0;
    while (!c->rp_pending.empty()) {
      RpReq* q = c->rp_pending.front();
      if (!grp.empty() && (tot + (size_t)q->b->B > cap || (int)grp.size() == RP_GATHER_MAX)) break;
      grp.push_back(q);
      tot += (size_t)q->b->B;
      c->pending_proofs -= (size_t)q->b->B;
      c->rp_pending.pop_front();
    }
    std::vector<Lane*> lanes{L};
    std::vector<std::vector<RpReq*>> sub{grp};
    // the next head (if any) may lead a pass on another free lane
    if (!c->rp_pending.empty() && !c->free_lanes.empty()) c->rp_pending.front()->cv.notify_one();
    lk.unlock();
    std::vector<int> rcs;
    run_rp_groups(c, lanes, sub, rcs);
    c->st_passes++;
    c->st_reqs += (int64_t)grp.size();
    c->st_act_reqs += std::count_if(grp.begin(), grp.end(), [](const RpReq* q) { return q->act != nullptr; });
    for (int64_t mx = c->st_max_merged.load(); (int64_t)grp.size() > mx && !c->st_max_merged.compare_exchange_weak(mx, (int64_t)grp.size());) {
    }
    lk.lock();
    for (size_t j = 0; j < sub.size(); j++)
      for (RpReq* q : sub[j]) {
        q->rc = rcs[j];
        q->done = true;
        if (q != &me) q->cv.notify_one();
      }
    for (Lane* x : lanes) c->free_lanes.push_back(x->id);
    c->wake_lane_waiters();
  }
  return me.rc;
}

extern "C" {

int fts_rp_batch_timings(const fts_rp_batch* b, const char** names, float* ms, double* mads, int cap) {
  if (!b) return 0;
  if (!b->parts.empty()) return b->parts[0] ? fts_rp_batch_timings(b->parts[0], names, ms, mads, cap) : 0;
  return b->tim.copy_out(names, ms, mads, cap);
}

int fts_rp_batch_merged(const fts_rp_batch* b) { return b ? b->merged : 0; }

int fts_debug_hold(fts_ctx* c, int n) {
  if (!c) return FTS_API_EINVAL;
  for (fts_ctx* ch : c->shards) fts_debug_hold(ch, n);
  if (c->lanes.empty()) return FTS_API_OK;
  std::lock_guard<std::mutex> g(c->mu);
  c->hold_n = std::max(0, n);
  if (c->hold_n == 0 || (int)c->rp_pending.size() >= c->hold_n) {
    c->hold_n = 0;
    for (RpReq* q : c->rp_pending) q->cv.notify_one();
  }
  return FTS_API_OK;
}

int fts_debug_dispatch_stats(const fts_ctx* c, int64_t* out) {
  if (!c || !out) return FTS_API_EINVAL;
  if (!c->shards.empty()) return fts_debug_dispatch_stats(c->shards[0], out);
  out[0] = c->st_passes.load();
  out[1] = c->st_reqs.load();
  out[2] = c->st_max_merged.load();
  out[3] = c->st_act_reqs.load();
  return FTS_API_OK;
}

int fts_debug_pass_stats(const fts_ctx* c, int64_t out[4]) {
  if (!c || !out) return FTS_API_EINVAL;
  out[0] = c->st_rp_passes.load();
  out[1] = c->st_rp_failed.load();
  out[2] = c->st_rp_located.load();
  out[3] = c->st_rp_perproof.load();
  for (const fts_ctx* ch : c->shards) {
    int64_t o[4];
    if (int rc = fts_debug_pass_stats(ch, o)) return rc;
    for (int q = 0; q < 4; q++) out[q] += o[q];
  }
  return FTS_API_OK;
}

int fts_ctx_reserve(fts_ctx* c, size_t max_pass_proofs) {
  if (!c) return FTS_API_EINVAL;
  if (!c->shards.empty()) {
    std::vector<size_t> all(c->shards.size() + 1);
    for (size_t j = 0; j < all.size(); j++) all[j] = j;  // one "item" per device
    return run_shards(all, [&](int j, size_t, size_t) { return fts_ctx_reserve(c->shards[j], max_pass_proofs); });
  }
  if (c->device < 0) return FTS_API_EDEVICE;
  const size_t B = max_pass_proofs ? max_pass_proofs : c->coalesce_max;
  if (B == 0 || B > (1u << 20)) return FTS_API_ESIZE;
  HIP_OK(hipSetDevice(c->device));
  for (size_t i = 0; i < c->lanes.size(); i++) {
    LaneGuard lg(c, (int)i);
    if (int rc = lane_reserve(c, *lg.L, (int)B, true)) return rc;
    HIP_OK(lg.L->sync());
  }
  return FTS_API_OK;
}

}  // extern "C"

extern "C" {

void fts_rp_batch_free(fts_rp_batch* b) { delete b; }

// a staging slot sized for n proofs (idle one reused, else a new one); nullptr on
// allocation failure
static RpSlot* slot_acquire(fts_ctx* c, size_t n) {
  RpSlot* sl = nullptr;
  {
    std::lock_guard<std::mutex> g(c->slot_mu);
    if (!c->free_slots.empty()) {
      sl = c->free_slots.back();
      c->free_slots.pop_back();
    }
  }
  if (!sl) {
    std::unique_ptr<RpSlot> fresh(new RpSlot());
    if (!fresh->create(c->device)) return nullptr;
    sl = fresh.get();
    std::lock_guard<std::mutex> g(c->slot_mu);
    c->slots.push_back(std::move(fresh));
  }
  const size_t npts = (size_t)rp_npts(c->k);
  const size_t in_bytes = n * (npts * 64 + RP_NSC * 32 + 8), dev_bytes = in_bytes + n * 4;
  if (!sl->size(in_bytes, dev_bytes)) {
    std::lock_guard<std::mutex> g(c->slot_mu);
    c->free_slots.push_back(sl);
    return nullptr;
  }
  return sl;
}

int fts_rp_verify_batch(fts_ctx* c, size_t n, const uint8_t* const* rp_der, const size_t* rp_len, const uint8_t* com64,
                        int32_t* status) {
  if (!c || !status) return FTS_API_EINVAL;
  if (n == 0) return FTS_API_OK;
  if (!rp_der || !rp_len || !com64) return FTS_API_EINVAL;
  if (!c->shards.empty()) return multi_rp_verify(c, n, rp_der, rp_len, com64, status);
  auto not_run = [&](int rc) {
    for (size_t i = 0; i < n; i++) status[i] = FTS_E_NOT_RUN;
    return rc;
  };
  if (c->device < 0) return not_run(FTS_API_EDEVICE);
  if (n > (size_t)INT32_MAX) return not_run(FTS_API_ESIZE);
  if (hipSetDevice(c->device) != hipSuccess) return not_run(FTS_API_EDEVICE);
  // host DER -> pinned records (parallel), one async upload on the slot's stream,
  // then the staged batch joins the coalescing dispatcher like any other
  RpSlot* sl = slot_acquire(c, n);
  if (!sl) return not_run(FTS_API_ENOMEM);
  const size_t npts = (size_t)rp_npts(c->k);
  const size_t raw_b = n * npts * 64, sc_b = n * RP_NSC * 32, st_b = n * 4;
  uint8_t* p = sl->pin.as<uint8_t>();
  uint8_t* const dev = sl->dev.as<uint8_t>();
  parse_rp_into(c->k, n, rp_der, rp_len, com64, p, reinterpret_cast<uint32_t*>(p + raw_b),
                reinterpret_cast<int32_t*>(p + raw_b + sc_b), reinterpret_cast<int32_t*>(p + raw_b + sc_b + st_b));
  fts_rp_batch* b = sl->b.get();
  // the slot's batch object serves unrelated callers in turn: the adaptive
  // group-test state (FTS_GT_ADAPT) is per caller batch, so an honest call never
  // inherits the dense schedule of the previous caller's tampered one
  b->dense = false;
  b->locate_skip = 0, b->locate_backoff = 8;
  b->merged = 1;
  b->tim.n = 0;
  b->B = (int)n;
  b->raw = dev;
  b->sc = reinterpret_cast<uint32_t*>(dev + raw_b);
  b->status0 = reinterpret_cast<int32_t*>(dev + raw_b + sc_b);
  b->ipa_flag = reinterpret_cast<int32_t*>(dev + raw_b + sc_b + st_b);
  b->status = reinterpret_cast<int32_t*>(dev + raw_b + sc_b + 2 * st_b);
  int rc = FTS_API_OK;
  if (hipMemcpyAsync(dev, p, raw_b + sc_b + 2 * st_b, hipMemcpyHostToDevice, sl->s) != hipSuccess ||
      hipEventRecord(sl->done, sl->s) != hipSuccess || hipEventSynchronize(sl->done) != hipSuccess)
    rc = FTS_API_EDEVICE;
  if (rc == FTS_API_OK) rc = fts_rp_batch_verify(c, b, status);
  else not_run(rc);
  {
    std::lock_guard<std::mutex> g(c->slot_mu);
    c->free_slots.push_back(sl);
  }
  return rc;
}

}  // extern "C"
