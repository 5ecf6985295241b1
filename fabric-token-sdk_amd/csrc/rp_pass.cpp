// Range-proof (Bulletproof + IPA) batch verification for gfx950: the pass's launch
// sequence (host code only; the kernels are in rp_exact.hip, rp_x0.hip and rp_rlc.hip).
//
// One launch sequence verifies a whole batch of B proofs of bit length n
// (k = log2 n rounds).  Work is laid out per (proof, item) so a batch of a
// few thousand proofs fills the 256 CUs.  Streams of a lane: S main, S2 the
// x0 prefix (work path) / x*D (latency path), S3 the batch check's weights and
// MSM, S4 its x0-free fixed-base columns (fork/join through events).
// Work path (passes above FTS_COM_FIXED_MAX proofs):
//
//   S   k_rp_decode        (proof, point)   NewG1FromBytes checks + Montgomery form
//   S   k_rp_hash_small    (proof, msg)     x, y, x_j transcripts (SHA-256 over hex)  bulletproof.go:266-281, ipa.go:230
//   S   k_rp_chal_fr       proof            z, polEval, batch inversion of y, x_j       bulletproof.go:282-311, ipa.go:236-244
//   S   k_rp_powers        (chunk, proof)   y^-i, s_i, z^2 2^i y^-i                     ipa.go:343-356 (unrolled)
//   S   k_rp_fixed_exact   (proof, item)    H'_i = y^-i H_i, z K, -delta P (fixed base) bulletproof.go:483-489
//   S   k_rp_normalize     point (block)    batch affine normalisation of H'_i (one inversion per block)
//   S   k_rp_hsum_chunks   (proof, chunk)   S_c = sum_j 2^j H'_{16c+j} (Horner)
//   S   k_rp_hsum_join     proof            S = sum_c 2^(16c) S_c
//   S   k_rp_com_tab       2 lanes/proof    affine tables 1..8 D and 1..8 S with beta*x (one inversion each)
//   S   k_rp_com_var       proof            x*D + z^2*S (ONE joint GLV/Straus chain over the proof's table),
//                                           com = C + z K - delta P + x D + z^2 S       bulletproof.go:477-492
//   S2  k_rp_x0_build/hash proof            x0 prefix: H' records + shared template     ipa.go:200-213
//   S   k_rp_x0_build/hash proof            x0 suffix after com: x0 = HashToZr(...)     ipa.go:213
//   S3  k_rlc_prep + MSM                    weights, variable points of the batch equation (no x0)
//   S4  k_rlc_columns/fixed                 x0-free fixed-base columns of the batch equation
//   S   k_rlc_columns/fixed (Q), finalize   column Q (needs x0), verdict
//   k_rp_terms_fixed / k_rp_terms_var / k_rp_check: per-proof fallback
//
#include <algorithm>
#include <atomic>
#include "device/fixed_base.hpp"
#include "device/rp_kernels.hpp"
#include "device/rp_decls.hpp"
#include "device/wave_prio.hpp"

namespace fts {

// block size of the latency-bound per-proof kernels (few waves, long chains):
// 256-thread blocks put a block's 4 waves on the 4 SIMDs of one CU, and the
// dispatcher spreads blocks over CUs, so concurrent small kernels of the
// pass's streams rarely share a SIMD (64-thread blocks of two such kernels
// slowed each other by ~26 %, tools/experiments/colocate.cpp)
int g_lat_bs = 256;
// block size of the work path's per-proof latency kernels (k_rp_chal_fr, k_rlc_prep,
// k_rp_x0_hash; FTS_WORK_BS): they start beside another pass's fixed-base launch
// (64-thread blocks filling the register file), where a 256-thread block waits for
// four wave slots of one CU at once (k_rp_chal_fr 0.12 ms alone, 1.1 ms there;
// k_rlc_prep 0.18 -> 1.8 ms in a 20-batch burst, round 5)
std::atomic<int> g_work_bs{64};  // written by context creation while other lanes launch
// block size of the work path's S / com chain kernels
constexpr int g_chain_bs = 64;

namespace {
// what every step of one pass reads
struct Pass {
  const RpBatchDev& d;
  const RlcDev& r;
  const uint32_t *tables, *wtables;
  const uint8_t *x0_const, *x0_tmpl;
  hipStream_t s, s2, s3, s4;
  Timeline* tl;
  int wbits;
  int lbs;  // block size of the per-proof latency kernels: g_lat_bs (latency path) or g_work_bs (work path)
};

// decode, the x / y / x_j transcripts and the challenges on s; on the latency path x*D
// starts on s2 right after the x transcript
void head(const Pass& p) {
  const RpBatchDev& d = p.d;
  const int B = d.B, n = d.n, k = d.k;
  if (d.excl) (void)hipMemsetAsync(d.excl, 0, (size_t)B * 4, p.s);
  // 64-thread blocks for the elementwise head kernels: beside the previous pass's
  // fixed-base launch (64-thread blocks, the whole register file) a 256-thread block
  // waits for four wave slots of one CU to free at once (k_rp_decode 0.07 ms alone,
  // 1.15 ms there in a 20-batch burst, round 5)
  FTS_LAUNCH(k_rp_decode, B * rp_npts(k), 64, p.s, B, rp_npts(k), d.raw, d.pts, d.status);
  p.tl->mark("k_rp_decode", p.s, 0);
  FTS_LAUNCH(k_rp_hash_small, B * (2 + k), 64, p.s, B, n, k, d.raw, d.status, d.ch, d.small_msgs);
  p.tl->mark("k_rp_hash_small", p.s, 0);
  if (d.com_fixed) {
    // latency path: x*D on the side stream beside chal_fr and the fixed-base products
    p.tl->fork(p.s, p.s2);
    FTS_LAUNCH(k_rp_xd, 2 * B, g_lat_bs, p.s2, B, n, k, d.status, d.pts, d.small_msgs,
               d.scratch + (size_t)B * (k + 1) * 8, d.terms, com_fx_slots(n), n + 2);
    p.tl->mark("k_rp_xd", p.s2, (double)B * 2 * COST_VB128);
  }
  FTS_LAUNCH(k_rp_chal_fr, B, p.lbs, p.s, B, n, k, d.status, d.ch, d.scratch);
  p.tl->mark("k_rp_chal_fr", p.s, (double)B * (3 * k + 4 * (k + 1) + 12));
}

void powers(const Pass& p) {
  const RpBatchDev& d = p.d;
  const int B = d.B, n = d.n, k = d.k;
  FTS_LAUNCH(k_rp_powers, B * (n >> std::min(PW_LC, k)), 64, p.s, B, n, k, d.status, d.ch, d.ypow, d.svec, d.zvec);
  p.tl->mark("k_rp_powers", p.s, (double)B * (3.0 * n + 2.0 * k));
}

// the batch check's weights on stream `on`; column Q (check_verdict) waits for ev_coef
void weights_on(const Pass& p, hipStream_t on) {
  const RpBatchDev& d = p.d;
  const int B = d.B, k = d.k;
  FTS_LAUNCH(k_rlc_prep, B, p.lbs, on, B, d.n, k, d.status, d.excl, d.ipa_flag, d.sc, d.ch, p.r.key, p.r.msc, p.r.coef);
  p.tl->mark("k_rlc_prep", on, (double)B * (3 * k + 33));
  (void)hipEventRecord(d.ev_coef, on);
}

// batch check on s3 (after the caller's hook, e.g. the exclusion of range
// proofs whose action failed its sigma proof): the weights need only the
// challenges, so on the latency path (d.rlc_fork = 0) they start right after
// k_rp_chal_fr, before the exact phase's wide launches take the CUs; the
// work path forks after its widest launch (d.rlc_fork = 1) so the check's
// latency-bound chain does not share SIMDs with it.  The x0-free columns and
// their fixed-base products run on s4 (they need k_rp_powers' vectors): the
// MSM's bucket phase does not wait for them, only its window reduction.
void check_weights(const Pass& p) {
  p.tl->fork(p.s, p.s3);
  if (p.d.pre_rlc) p.d.pre_rlc(p.d.pre_rlc_arg, p.s3);
  weights_on(p, p.s3);
}

// d.rlc_fork == 3 (work path): the weights and the MSM's counting sort (memory /
// LDS work, no long chains) beside the fixed-base launch; its accumulation waits
// for that launch (after it, below), so the MSM chain starts sorted
// The weights run on s itself, ahead of the fixed-base launch (0.2 ms alone; on
// s3 beside that launch the 320 blocks starved for 6 ms), then the sort on s3.
// d.rlc_fork == 4: the whole sort on s itself (~0.6 ms alone, ahead of the
// fixed-base launch): beside the chain kernels the sort's small latency-bound
// launches starved (k_rs_hist 0.04 -> 2.2 ms in a 20-batch burst, round 5), and
// beside the fixed-base launch too (3: k_msm_split 6 ms)
void check_weights_and_early_sort(const Pass& p) {
  weights_on(p, p.s);
  if (p.d.rlc_fork == 4) {
    launch_msm_sort(p.r.plan, p.r.msc, p.s, p.tl);
  } else {
    p.tl->fork(p.s, p.s3);
    launch_msm_sort(p.r.plan, p.r.msc, p.s3, p.tl);
  }
}

// the x0-free fixed-base columns on s4 and the MSM on s3, which sums their products
// as extras.  presorted: the MSM's sort already ran (check_weights_and_early_sort);
// only its accumulation and reduction are left
void check_columns_and_msm(const Pass& p, bool presorted) {
  const RpBatchDev& d = p.d;
  const RlcDev& r = p.r;
  const int B = d.B, n = d.n, k = d.k, NC = rlc_ncols(n);
  const bool grouped = r.G > 1;
  p.tl->fork(p.s, p.s4);   // k_rp_powers' vectors
  p.tl->fork(p.s3, p.s4);  // the weights
  if (grouped) {
    // per caller batch: the x0-free column sums and products of every group (slot Q
    // left as the identity: zero words), the MSM's extras with stride NC
    (void)hipMemsetAsync(r.gfix, 0, (size_t)r.G * NC * 96, p.s4);
    hipLaunchKernelGGL(k_rlc_columns, dim3(NC - 1, r.G), dim3(256), 0, p.s4, B, n, k, r.gs, 0, r.sel, d.ch, r.coef,
                       d.ypow, d.svec, d.zvec, r.gcol);
    p.tl->mark("k_rlc_columns", p.s4, (double)B * 4 * n);
    FTS_LAUNCH(k_rlc_fixed, (size_t)r.G * (NC - 1) * FB_NW, RF_ITEMS * FB_NW, p.s4, n, r.G, 0, NC - 1, r.gcol, p.tables,
               r.gfix);
    p.tl->mark("k_rlc_fixed", p.s4, (double)r.G * (NC - 1) * (FB_NW * 3 + (FB_NW - 1) * COST_ADD));
  } else {
    hipLaunchKernelGGL(k_rlc_columns, dim3(NC - 1, 1), dim3(256), 0, p.s4, B, n, k, B, 0, (const int32_t*)nullptr, d.ch,
                       r.coef, d.ypow, d.svec, d.zvec, r.colsum);
    p.tl->mark("k_rlc_columns", p.s4, (double)B * 4 * n);
    FTS_LAUNCH(k_rlc_fixed, (size_t)(NC - 1) * FB_NW, RF_ITEMS * FB_NW, p.s4, n, 1, 0, NC - 1, r.colsum, p.tables,
               r.fixed);
    p.tl->mark("k_rlc_fixed", p.s4, (double)(NC - 1) * (FB_NW * 3 + (FB_NW - 1) * COST_ADD));
  }
  const uint32_t* extra = grouped ? r.gfix : r.fixed;
  const int nextra = grouped ? NC : NC - 1;
  if (presorted) launch_msm_reduce(r.plan, d.pts, extra, nextra, r.msm_scratch, p.s3, p.s4, p.tl);
  else launch_msm(r.plan, d.pts, r.msc, extra, nextra, r.msm_scratch, p.s3, p.s4, p.tl);
}

// the pass's widest launch on s: H'_i, z K, -delta P (work path), and the com terms
// Z_i as well (latency path)
void fixed_base_products(const Pass& p) {
  const RpBatchDev& d = p.d;
  const int B = d.B, n = d.n, k = d.k;
  // fixed-base products over the wide tables: 12 (20-bit) or 11 (22-bit) additions each
  const double cost_fbw = p.wbits == 22 ? 11.0 * COST_XMADD + COST_X2J : COST_FBW_FRESH;
  // FTS_FX_SERIAL: one pass's fixed-base launch at a time across the lanes (the
  // previous pass's launch has ended), so the next pass's launch overlaps this
  // pass's latency-bound chain instead of its own twin
  if (d.fx_wait) (void)hipStreamWaitEvent(p.s, d.fx_wait, 0);
  if (d.com_fixed) {
    if (p.wbits == 22)
      FTS_LAUNCH(k_rp_fixed_all<22>, (size_t)B * (2 * n + 2), 64, p.s, B, n, k, d.status, d.sc, d.ch, d.ypow, d.zvec,
                 p.wtables, d.hpj, d.terms);
    else
      FTS_LAUNCH(k_rp_fixed_all<FBW_W>, (size_t)B * (2 * n + 2), 64, p.s, B, n, k, d.status, d.sc, d.ch, d.ypow, d.zvec,
                 p.wtables, d.hpj, d.terms);
    p.tl->mark("k_rp_fixed_all", p.s, (double)B * (2.0 * n + 2.0) * cost_fbw);
  } else {
    if (p.wbits == 22)
      FTS_LAUNCH(k_rp_fixed_exact<22>, (size_t)B * (n + 2), 64, p.s, B, n, k, d.status, d.sc, d.ch, d.ypow, p.wtables,
                 d.hpj, d.terms);
    else
      FTS_LAUNCH(k_rp_fixed_exact<FBW_W>, (size_t)B * (n + 2), 64, p.s, B, n, k, d.status, d.sc, d.ch, d.ypow, p.wtables,
                 d.hpj, d.terms);
    p.tl->mark("k_rp_fixed_exact", p.s, (double)B * (n + 2) * cost_fbw);
  }
  if (d.ev_fx) (void)hipEventRecord(d.ev_fx, p.s);
}

// H'_i -> affine + BE bytes on stream `on`; with the x0 prefix split (FTS_X0_SPLIT bit 1),
// the normalisation also writes the H' hex records of the x0 messages (k_rp_x0_hdr the
// header and constant bytes around them)
void normalize_hprime(const Pass& p, hipStream_t on) {
  const RpBatchDev& d = p.d;
  const int B = d.B, n = d.n, nhp = B * n;
  if (d.x0_mid) FTS_LAUNCH(k_rp_x0_hdr, B, 256, on, B, n, d.status, p.x0_const, d.x0_msgs);
  launch_normalize(nhp, n, n + 1, 0, d.status, d.hpj, d.hpa, d.hp_be, on, d.x0_mid ? d.x0_msgs : nullptr);
  p.tl->mark("k_rp_normalize", on, (double)nhp * (7.0 + COST_INV / NORM_E));
}

// x0 prefix on the side stream: the H' records and the shared template
// (cb1 of the message's blocks) do not depend on com, so they are hashed
// beside the S / com chain; only the suffix waits for com
void x0_prefix(const Pass& p) {
  const RpBatchDev& d = p.d;
  FTS_LAUNCH(k_rp_x0_hash, d.B, p.lbs, p.s2, d.B, d.n, d.k, d.status, d.x0_msgs, p.x0_tmpl, 0u, x0_cb1(d.n), d.x0_mid,
             d.ch);
  p.tl->mark("k_rp_x0_prefix", p.s2, 0);
}

// com on the latency path: the normalisation on s, then the LDS tree over the fixed-base
// terms and x*D (s2); the x0 prefix is hashed on s2 beside com_tree
void exact_latency_path(const Pass& p) {
  const RpBatchDev& d = p.d;
  const int B = d.B, n = d.n, k = d.k;
  normalize_hprime(p, p.s);
  p.tl->fork(p.s2, p.s);  // x*D (k_rp_xd) before com_tree
  if (d.x0_mid) {         // after the fork above, so com_tree does not wait for the prefix
    p.tl->fork(p.s, p.s2);
    x0_prefix(p);
  }
  hipLaunchKernelGGL(k_rp_com_tree, dim3((B + CT_PROOFS - 1) / CT_PROOFS), dim3(CT_LANES * CT_PROOFS), 0, p.s, B, n,
                     k, d.status, d.pts, d.terms, d.hpj, d.hpa, d.hp_be);
  p.tl->mark("k_rp_com_sum", p.s, (double)B * ((com_fx_slots(n) + 1) * COST_ADD + COST_NORM1));
}

// com on the work path
void exact_work_path(const Pass& p) {
  const RpBatchDev& d = p.d;
  const int B = d.B, n = d.n, k = d.k;
  // H'_i -> affine + BE bytes (x0 transcript) on the side stream: the S / com
  // chain on s works on the Jacobian H' (k_rp_hsum_chunks) and does not wait
  // for it; com is normalised after com_var
  p.tl->fork(p.s, p.s2);
  normalize_hprime(p, p.s2);
  if (d.x0_mid) x0_prefix(p);
  const int nch = (n + HS_CHUNK - 1) / HS_CHUNK;
  FTS_LAUNCH(k_rp_hsum_chunks, B * nch, g_chain_bs, p.s, B, n, d.status, d.hpj, d.scratch);
  p.tl->mark("k_rp_hsum_chunks", p.s, (double)B * (n - nch) * (COST_DBL + COST_ADD));
  FTS_LAUNCH(k_rp_hsum_join, B, g_chain_bs, p.s, B, n, d.status, d.scratch);
  p.tl->mark("k_rp_hsum_join", p.s, (double)B * (nch - 1) * (HS_CHUNK * COST_DBL + COST_ADD));
  // scratch: [0, B*HS_SCRATCH) Horner chunks of S, then the B proofs' affine tables.
  // k_rp_com_tab: ceil(B / bs) blocks for D's rows, then as many for S's
  const size_t tab_blocks = ((size_t)B + g_chain_bs - 1) / g_chain_bs;
  FTS_LAUNCH(k_rp_com_tab, 2 * tab_blocks * g_chain_bs, g_chain_bs, p.s, B, n, k, d.status, d.pts, d.scratch,
             d.scratch + (size_t)B * HS_SCRATCH);
  p.tl->mark("k_rp_com_tab", p.s, (double)B * (COST_CTAB8_AFF + COST_CTAB8_JAC));
  FTS_LAUNCH(k_rp_com_var, B, g_chain_bs, p.s, B, n, k, d.status, d.pts, d.ch, d.scratch,
             d.scratch + (size_t)B * HS_SCRATCH, d.terms, d.hpj, d.hpa, d.hp_be);
  p.tl->mark("k_rp_com_var", p.s, (double)B * (COST_STRAUS4_CTAB + 3.0 * COST_ADD + COST_NORM1));
}

// x0 on s: the message (its tail only, with the prefix split) and its hash
void x0_tail(const Pass& p) {
  const RpBatchDev& d = p.d;
  const int B = d.B, n = d.n;
  const bool split = d.x0_mid != nullptr;
  // work path without the prefix split: the whole message needs the H' bytes of s2
  if (!d.com_fixed && !split) p.tl->fork(p.s2, p.s);
  hipLaunchKernelGGL(k_rp_x0_build, dim3(x0_build_grid(B)), dim3(64 * X0_PPB), x0_build_lds(n, split ? 1 : 2), p.s, B,
                     n, d.status, d.hp_be, p.x0_const, d.sc, d.x0_msgs, split ? 1 : 2);
  p.tl->mark(split ? "k_rp_x0_build_tail" : "k_rp_x0_build", p.s, 0);
  if (split) p.tl->fork(p.s2, p.s);  // the prefix's midstate
  FTS_LAUNCH(k_rp_x0_hash, B, p.lbs, p.s, B, n, d.k, d.status, d.x0_msgs, p.x0_tmpl, split ? x0_cb1(n) : 0u,
             0xffffffffu, d.x0_mid, d.ch);
  p.tl->mark("k_rp_x0_hash", p.s, 0);
}

// x0 tail: column Q (needs the weights of k_rlc_prep) and its product, then
// the verdict once the MSM is in
void check_verdict(const Pass& p) {
  const RpBatchDev& d = p.d;
  const RlcDev& r = p.r;
  const int B = d.B, n = d.n, k = d.k, NC = rlc_ncols(n);
  (void)hipStreamWaitEvent(p.s, d.ev_coef, 0);
  if (r.G > 1) {
    hipLaunchKernelGGL(k_rlc_columns, dim3(1, r.G), dim3(256), 0, p.s, B, n, k, r.gs, NC - 1, r.sel, d.ch, r.coef,
                       d.ypow, d.svec, d.zvec, r.gcol);
    FTS_LAUNCH(k_rlc_fixed, (size_t)r.G * FB_NW, RF_ITEMS * FB_NW, p.s, n, r.G, NC - 1, 1, r.gcol, p.tables, r.gqfix);
    p.tl->mark("k_rlc_q", p.s, (double)B + r.G * (FB_NW * 3 + (FB_NW - 1) * COST_ADD));
    (void)hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(r.flag), 1, 1, p.s);
    p.tl->fork(p.s3, p.s);
    FTS_LAUNCH(k_rlc_finalize_groups, (size_t)r.G * r.gs, 256, p.s, r.G * r.gs, r.gs, NC, r.sel, r.plan.out, r.gqfix,
               d.excl, d.status, d.ipa_flag, r.gflag, r.flag);
  } else {
    launch_rlc_q_column(d, r, p.tables, p.s, p.tl);
    p.tl->fork(p.s3, p.s);
    FTS_LAUNCH(k_rlc_finalize, B, 64, p.s, B, r.plan.out, r.fixed + (size_t)(NC - 1) * 24, d.excl, d.status, d.ipa_flag,
               r.flag);
  }
  p.tl->mark("k_rlc_finalize", p.s, 0);
}
}  // namespace

// Whole range-proof pipeline up to the batch verdict (flag): exact per-proof
// phase (everything that is hashed: challenges, H'_i, com, x0) and the
// random-linear-combination check of all final equations (one MSM).
// s = main stream (exact phase, then the x0-dependent tail), s2 = x*D beside
// the fixed-base products (latency path), s3 = the batch check's variable part
// (weights, x0-free columns, MSM), which needs only the challenges.
void launch_rp_batch(const RpBatchDev& d, const RlcDev& r, const uint32_t* tables, const uint32_t* wtables,
                     const uint8_t* x0_const, const uint8_t* x0_tmpl, hipStream_t s, hipStream_t s2, hipStream_t s3,
                     hipStream_t s4, Timeline* tl, int wbits) {
  if (!d.B) return;
  const Pass p{d, r, tables, wtables, x0_const, x0_tmpl, s, s2, s3, s4, tl, wbits,
               d.com_fixed ? g_lat_bs : g_work_bs.load(std::memory_order_relaxed)};
  // where the batch check leaves s (d.rlc_fork): 0 right after the challenges; 1 after the
  // fixed-base launch; 3 / 4 (work path only) weights and sort ahead of that launch, the
  // rest after it
  const bool early_sort = (d.rlc_fork == 3 || d.rlc_fork == 4) && !d.com_fixed && d.ev_fx && !d.pre_rlc;
  head(p);
  if (!d.rlc_fork) check_weights(p);
  powers(p);
  if (early_sort) check_weights_and_early_sort(p);
  if (!d.rlc_fork) check_columns_and_msm(p, false);
  fixed_base_products(p);
  if (early_sort) {
    (void)hipStreamWaitEvent(s3, d.ev_fx, 0);
    check_columns_and_msm(p, true);
  } else if (d.rlc_fork) {
    check_weights(p);
    check_columns_and_msm(p, false);
  }
  // exact per-proof phase on s
  if (d.com_fixed) exact_latency_path(p);
  else exact_work_path(p);
  x0_tail(p);
  check_verdict(p);
}

// staged batches -> one merged pass (raw points, scalars, host verdicts, IPA flags)
void launch_rp_gather(const RpGather& g, int k, uint8_t* raw, uint32_t* sc, int32_t* status, int32_t* ipa, hipStream_t s) {
  const int per = rp_npts(k) * 4 + RP_NSC * 2 + 1;
  FTS_LAUNCH(k_rp_gather, (size_t)g.off[g.G] * per, 64, s, g, rp_npts(k), raw, sc, status, ipa);
}

// FTS_WAVE_PRIO: every unit with prioritised kernels holds its own copy of the table
// (helpers.hpp); the first error wins
hipError_t set_wave_prio(const int* p) {
  for (auto upload : {upload_wave_prio_rp_exact, upload_wave_prio_rp_x0, upload_wave_prio_rp_rlc, upload_wave_prio_msm})
    if (const hipError_t e = upload(p); e != hipSuccess) return e;
  return hipSuccess;
}

}  // namespace fts
