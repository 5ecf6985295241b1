// Range-proof batch check (random linear combination of all final equations), its group
// test and the single-fault locator.  The pass itself launches the check's kernels from
// rp_pass.cpp; the launchers here run after a failed check.
#include "device/g1.hpp"
#include "device/fixed_base.hpp"
#include "device/glv.hpp"
#include "device/rp_kernels.hpp"
#include "device/rp_decls.hpp"
#include "device/transcript.hpp"
#include "device/helpers.hpp"
#include "device/msm.hpp"
#include "common/chacha20.hpp"
#include "../../include/fts_gpu.h"

namespace fts {

// ------------------------------------------------------------ RLC batch check
// Sum_p rho_p E1_p + rho'_p E2_p == O  (SURVEY Appendix B).  Fixed bases get
// batch-summed scalars (column reduction), variable points go to one MSM.
// com never enters as a point: E2's -rho' com is expanded through its
// definition (bulletproof.go:477-492)
//   -rho' com = -rho' C - rho' x D - rho' z K + rho' delta P - rho' sum_i z^2 2^i y^-i H_i
// so the variable points are T1, T2, V, C, D, L_j, R_j (all decoded from the
// proof) and the K, P, H_i terms join the fixed-base columns.  The check then
// depends only on the challenges (not on H'_i, com or x0, except column Q =
// rho'(ab - ip) x0 Q): the MSM runs beside the exact per-proof phase.

// full-width weight: 256 random bits reduced mod r (Montgomery form).  Full
// width keeps every MSM window's digits uniform (a 128-bit weight would put
// all proofs' top-digit entries into a few buckets of one window).
FTS_DEV Fr fr_from_u256(const uint32_t w[8]) {
  uint32_t be[8];
#pragma unroll
  for (int i = 0; i < 8; i++) be[i] = w[7 - i];
  return f_to_mont(digest_to_fr(be));
}

__global__ void __launch_bounds__(256) k_rlc_prep(int B, int n, int k, const int32_t* __restrict__ status,
                                                 const int32_t* __restrict__ excl,
                                                 const int32_t* __restrict__ ipa_flag, const uint32_t* __restrict__ sc,
                                                 const uint32_t* __restrict__ ch, const uint32_t* __restrict__ key,
                                                 uint32_t* __restrict__ msc, uint32_t* __restrict__ coef, int idxw) {
  wave_prio<PS_SORT>();
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int npts = rp_npts(k);
  uint32_t* M = msc + (size_t)b * npts * 8;
  uint32_t* K = coef + (size_t)b * RLC_NCOEF * 8;
  const bool e1 = status[b] == 0 && !(excl && excl[b]);
  const bool e2 = e1 && ipa_flag[b] == 0;
  Fr zero = f_zero<FrP>();
  for (int q = 0; q < npts; q++) store_f(M + q * 8, zero);
  for (int q = 0; q < RLC_NCOEF; q++) store_f(K + q * 8, zero);
  if (!e1) return;
  uint32_t kk[8], blk[16];
#pragma unroll
  for (int q = 0; q < 8; q++) kk[q] = key[q];
  chacha20_block(kk, (uint32_t)b, blk);
  Fr rho = fr_from_u256(blk), rho2 = fr_from_u256(blk + 8);
  if (idxw) {  // the single-fault locator's sum: both weights of proof b times b + 1
    const uint32_t w[8] = {(uint32_t)b + 1u, 0, 0, 0, 0, 0, 0, 0};
    const Fr wb = fr_from_canon(w);
    rho = fr_mul(rho, wb);
    rho2 = fr_mul(rho2, wb);
  }
  const uint32_t* C = ch + (size_t)b * rp_nch(k) * 8;
  const uint32_t* S = sc + (size_t)b * RP_NSC * 8;
  Fr x, x2, z2, pol;
  load_f(C + CH_X * 8, x);
  load_f(C + CH_X2 * 8, x2);
  load_f(C + CH_Z2 * 8, z2);
  load_f(C + CH_POL * 8, pol);
  Fr ip = fr_from_canon(S + RP_SC_IP * 8);
  auto put = [&](int slot, const Fr& v) { store_f(M + slot * 8, f_from_mont(f_neg(v))); };  // canonical, negated
  put(RP_PT_T1, fr_mul(rho, x));
  put(RP_PT_T2, fr_mul(rho, x2));
  put(RP_PT_V, fr_mul(rho, z2));
  store_f(K + 0 * 8, fr_mul(rho, f_sub(ip, pol)));
  store_f(K + 1 * 8, fr_mul(rho, fr_from_canon(S + RP_SC_TAU * 8)));
  if (!e2) return;
  Fr a = fr_from_canon(S + RP_SC_A * 8), bb = fr_from_canon(S + RP_SC_B * 8), z;
  load_f(C + CH_Z * 8, z);
  put(RP_PT_C, rho2);
  put(RP_PT_D, fr_mul(rho2, x));
  for (int j = 0; j < k; j++) {
    Fr xj, xji;
    load_f(C + (CH_XJ + j) * 8, xj);
    load_f(C + (CH_XJ + k + j) * 8, xji);
    put(RP_PT_L + j, fr_mul(rho2, fr_sqr(xj)));
    put(RP_PT_L + k + j, fr_mul(rho2, fr_sqr(xji)));
  }
  store_f(K + 2 * 8, fr_mul(rho2, f_sub(fr_mul(a, bb), ip)));
  store_f(K + 3 * 8, fr_mul(rho2, a));
  store_f(K + 4 * 8, fr_mul(rho2, bb));
  store_f(K + 5 * 8, rho2);
  store_f(K + 6 * 8, f_neg(fr_mul(rho2, z)));
  store_f(K + 7 * 8, fr_mul(rho2, fr_from_canon(S + RP_SC_DELTA * 8)));
}

// proof b's scalar in RLC column col (layout: rlc_ncols), Montgomery form.
// s_i, y^-i and z^2 2^i y^-i come precomputed, i-major, from k_rp_powers.
FTS_DEV Fr rlc_col_value(int col, int b, int B, int n, int k, const uint32_t* __restrict__ ch,
                         const uint32_t* __restrict__ coef, const uint32_t* __restrict__ ypow,
                         const uint32_t* __restrict__ svec, const uint32_t* __restrict__ zvec) {
  const uint32_t* K = coef + (size_t)b * RLC_NCOEF * 8;
  Fr v;
  if (col < 2) {
    load_f(K + col * 8, v);
  } else if (col < 2 + n) {  // rho' a s_i
    Fr ra;
    load_f(K + 3 * 8, ra);
    if (!f_is_zero(ra)) {
      Fr sv;
      load_f(svec + ((size_t)(col - 2) * B + b) * 8, sv);
      v = fr_mul(ra, sv);
    } else {
      v = ra;
    }
  } else if (col < 2 + 2 * n) {  // rho' b s_i^-1 y^-i - rho' z^2 2^i y^-i
    const int i = col - 2 - n;
    Fr r2;
    load_f(K + 5 * 8, r2);
    if (!f_is_zero(r2)) {
      Fr rb, sv, yp, zv;
      load_f(K + 4 * 8, rb);
      load_f(svec + ((size_t)(n - 1 - i) * B + b) * 8, sv);
      load_f(ypow + ((size_t)i * B + b) * 8, yp);
      load_f(zvec + ((size_t)i * B + b) * 8, zv);
      v = f_sub(fr_mul(fr_mul(rb, sv), yp), fr_mul(r2, zv));
    } else {
      v = r2;
    }
  } else if (col < 2 * n + 4) {  // -rho' z (K), rho' delta (P)
    load_f(K + (col - 2 * n + 4) * 8, v);
  } else {  // rho'(ab - ip) x0 (Q)
    load_f(K + 2 * 8, v);
    if (!f_is_zero(v)) {
      Fr x0;
      load_f(ch + ((size_t)b * rp_nch(k) + CH_X0) * 8, x0);
      v = fr_mul(v, x0);
    }
  }
  return v;
}

// one block per (column, group), columns col0 + blockIdx.x.  The batch check
// has one group of all B proofs; the group test has G groups of gs proof slots
// (sel[g gs + j], -1 = empty) -> colsum[g][col]
__global__ void __launch_bounds__(256) k_rlc_columns(int B, int n, int k, int gs, int col0,
                                                     const int32_t* __restrict__ sel, const uint32_t* __restrict__ ch,
                                                     const uint32_t* __restrict__ coef, const uint32_t* __restrict__ ypow,
                                                     const uint32_t* __restrict__ svec,
                                                     const uint32_t* __restrict__ zvec, uint32_t* __restrict__ colsum) {
  wave_prio<PS_COLS>();
  __shared__ uint32_t sh[256 * 8];
  const int col = col0 + blockIdx.x, grp = blockIdx.y, t = threadIdx.x, nt = blockDim.x;  // nt: 64 or 256
  Fr acc = f_zero<FrP>();
  for (int j = t; j < gs; j += nt) {
    const int b = sel ? sel[(size_t)grp * gs + j] : grp * gs + j;
    if (b < 0 || b >= B) continue;
    acc = f_add(acc, rlc_col_value(col, b, B, n, k, ch, coef, ypow, svec, zvec));
  }
  store_f(sh + t * 8, acc);
  __syncthreads();
  for (int half = nt / 2; half >= 1; half >>= 1) {
    if (t < half) {
      Fr o;
      load_f(sh + (t + half) * 8, o);
      acc = f_add(acc, o);
      store_f(sh + t * 8, acc);
    }
    __syncthreads();
  }
  if (t == 0) store_f(colsum + ((size_t)grp * rlc_ncols(n) + col) * 8, f_from_mont(acc));
}

// column Q over the whole pass, second stage: sum the RQ_PARTS partial sums that
// k_rlc_columns wrote per slice of proofs (rows 1..RQ_PARTS of colsum) into row 0.
// (One block over all B proofs took 0.76 ms at 81,920 on the x0-dependent tail.)
// (block x sums column col + x: the locator splits every column this way)
__global__ void __launch_bounds__(64) k_rlc_qsum(int ncols, int col0, uint32_t* __restrict__ colsum) {
  wave_prio<PS_FIN>();
  __shared__ uint32_t sh[RQ_PARTS * 8];
  const int t = threadIdx.x, col = col0 + blockIdx.x;
  Fr v;  // plain residues: the sum is the same in either representation
  load_f(colsum + ((size_t)(1 + t) * ncols + col) * 8, v);
  store_f(sh + t * 8, v);
  __syncthreads();
  for (int half = RQ_PARTS / 2; half >= 1; half >>= 1) {
    if (t < half) {
      Fr o;
      load_f(sh + (t + half) * 8, o);
      v = f_add(v, o);
      store_f(sh + t * 8, v);
    }
    __syncthreads();
  }
  if (t == 0) store_f(colsum + (size_t)col * 8, v);
}

FTS_DEV int rlc_col_base(int n, int col) {
  return col == 0 ? tb_G(n) : col == 1 ? tb_H(n) : col < 2 * n + 2 ? col - 2 : col == 2 * n + 2 ? tb_K(n)
         : col == 2 * n + 3 ? tb_P(n) : tb_Q(n);
}

// fixed-base product of each column sum, FB_NW lanes per (group, column):
// lane w looks up its window's entry, then an LDS tree of log2(FB_NW) full
// additions (latency: 4 additions instead of a chain of 16)
static_assert(FB_NW == 16, "one lane per 16-bit window");
__global__ void __launch_bounds__(RF_ITEMS * FB_NW) k_rlc_fixed(int n, int G, int col0, int ncl,
                                                               const uint32_t* __restrict__ colsum,
                                                               const uint32_t* __restrict__ tables,
                                                               uint32_t* __restrict__ out) {
  wave_prio<PS_COLS>();
  __shared__ uint32_t sh[RF_ITEMS * FB_NW * 24];
  const int w = threadIdx.x % FB_NW, it = blockIdx.x * RF_ITEMS + threadIdx.x / FB_NW;
  const bool live = it < G * ncl;
  const int NC = rlc_ncols(n), grp = live ? it / ncl : 0, col = col0 + (live ? it % ncl : 0);
  G1J acc = g1j_identity();
  if (live) {
    uint32_t s[8];
#pragma unroll
    for (int q = 0; q < 8; q++) s[q] = colsum[((size_t)grp * NC + col) * 8 + q];
    int carry = 0, d = 0;
    for (int q = 0; q <= w; q++) d = fb_next_digit(s, carry);
    if (d != 0)
      acc = g1j_from_affine(fb_entry(tables + (size_t)rlc_col_base(n, col) * FB_WORDS_PER_BASE, w, d));
  }
  uint32_t* S = sh + (size_t)(threadIdx.x - w) * 24;
  store_g1j(S + w * 24, acc);
  __syncthreads();
  for (int half = FB_NW / 2; half >= 1; half >>= 1) {
    if (live && w < half) add_inl(acc, load_g1j(S + (w + half) * 24));
    __syncthreads();
    if (live && w < half) store_g1j(S + w * 24, acc);
    __syncthreads();
  }
  if (live && w == 0) store_g1j(out + ((size_t)grp * NC + col) * 24, acc);
}

// Group test over many small groups (gs <= GT_SMALL_MAX proof slots): lane per
// (chunk of GT_CC columns, group), chunk-major so a wave's lanes read the same
// columns' tables: the group's column scalars (sum over its proof slots, as
// k_rlc_columns) and their fixed-base products, 16 mixed additions each from
// the 16-bit tables, accumulated in the lane -> gfix[grp][chunk] (Jacobian).
// (The per-column LDS-tree form above is for a few large groups: with 10^4
// groups of 8 it ran at ~20 % of the MAD peak.)
__global__ void __launch_bounds__(256) k_rlc_group_cols_small(int B, int n, int k, int G, int gs,
                                                              const int32_t* __restrict__ sel,
                                                              const uint32_t* __restrict__ ch,
                                                              const uint32_t* __restrict__ coef,
                                                              const uint32_t* __restrict__ ypow,
                                                              const uint32_t* __restrict__ svec,
                                                              const uint32_t* __restrict__ zvec,
                                                              const uint32_t* __restrict__ tables,
                                                              uint32_t* __restrict__ gfix) {
  const int NC = rlc_ncols(n), nch = gt_nchunks(n);
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (size_t)G * nch) return;
  const int chk = (int)(gid / G), grp = (int)(gid % G);
  G1J acc = g1j_identity();
  const int c1 = min(NC, (chk + 1) * GT_CC);
  for (int col = chk * GT_CC; col < c1; col++) {
    Fr v = f_zero<FrP>();
    for (int j = 0; j < gs; j++) {
      const int b = sel[(size_t)grp * gs + j];
      if (b < 0 || b >= B) continue;
      v = f_add(v, rlc_col_value(col, b, B, n, k, ch, coef, ypow, svec, zvec));
    }
    if (f_is_zero(v)) continue;
    const Fr cv = f_from_mont(v);
    Scalar sk;
#pragma unroll
    for (int q = 0; q < 8; q++) sk.v[q] = cv.v[q];
    fb_mul_acc(acc, tables + (size_t)rlc_col_base(n, col) * FB_WORDS_PER_BASE, sk);
  }
  store_g1j(gfix + ((size_t)grp * nch + chk) * 24, acc);
}

// batch verdict: flag = 1 if the combination is the identity; on success the
// deferred IPA structural verdicts become final (their E1 held)
// (msm_out + addend: the Q column's product, computed after x0)
__global__ void __launch_bounds__(64) k_rlc_finalize(int B, const uint32_t* __restrict__ msm_out,
                                                     const uint32_t* __restrict__ addend,
                                                     const int32_t* __restrict__ excl,
                                                     int32_t* __restrict__ status, const int32_t* __restrict__ ipa_flag,
                                                     int32_t* __restrict__ flag) {
  wave_prio<PS_FIN>();
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B && excl && excl[b] && status[b] == 0) status[b] = FTS_E_NOT_RUN;
  G1J e = load_g1j(msm_out);
  add_inl(e, load_g1j(addend));
  const bool pass = g1j_is_identity(e);
  if (b == 0) *flag = pass ? 1 : 0;
  if (b < B && pass && status[b] == 0 && ipa_flag[b] != 0) status[b] = ipa_flag[b];
}

// Single-fault locator (round 5).  When the batch combination S = sum_b rho_b E_b
// (E_b: proof b's final equations, rho_b its weights) is not the identity, the
// same combination with weights (b + 1) rho_b gives S' = sum_b (b + 1) rho_b E_b.
// If exactly one proof i is bad, S' = (i + 1) S; conversely S' = (j + 1) S means
// sum_b (b - j) rho_b E_b = 0, which for two or more bad proofs (or one bad proof
// other than j) holds only with probability ~1/r over the fresh random weights --
// the same soundness as the batch check itself.  Lane j tests S' == (j + 1) S.
__global__ void __launch_bounds__(64) k_rlc_total(const uint32_t* __restrict__ msm_out,
                                                  const uint32_t* __restrict__ addend, uint32_t* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  G1J e = load_g1j(msm_out);
  add_inl(e, load_g1j(addend));
  store_g1j(out, e);
}
__global__ void __launch_bounds__(64) k_rlc_locate(int B, const uint32_t* __restrict__ total,
                                                   const uint32_t* __restrict__ msm_out,
                                                   const uint32_t* __restrict__ addend, int32_t* __restrict__ loc) {
  wave_prio<PS_FIN>();
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= B) return;
  G1J t = load_g1j(msm_out);
  add_inl(t, load_g1j(addend));
  const G1J S = load_g1j(total);
  const uint32_t m = (uint32_t)j + 1u;
  G1J P = g1j_identity();
  for (int bit = 31 - __builtin_clz(m); bit >= 0; bit--) {
    P = g1j_dbl(P);
    if ((m >> bit) & 1u) P = g1j_add(P, S);
  }
  if (g1j_eq(P, t)) loc[0] = j;
}
// after the locator: every proof but `skip` whose deferred IPA structural verdict is
// pending takes it (the combination of the others closed, as in k_rlc_finalize)
__global__ void __launch_bounds__(256) k_rlc_accept_except(int B, int skip, int32_t* __restrict__ status,
                                                           const int32_t* __restrict__ ipa_flag) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B && b != skip && status[b] == 0 && ipa_flag[b] != 0) status[b] = ipa_flag[b];
}

// group test verdicts: lane per proof slot j of the selection (group j / gs);
// a group whose partial combination is the identity accepts its proofs (their
// deferred IPA structural verdicts become final, as in k_rlc_finalize), the
// proofs of the other groups are appended to `next` (the next round's list)
// the per-caller-batch combination (RlcDev::G > 1): slot j of group j / gs; group g
// closes when its MSM sum (x0-free columns included as extras) + column Q's product
// is the identity -> its proofs take their exact-phase verdicts, gflag[g] = 1; a
// failing group's proofs stay undecided (the group test runs over those batches only)
__global__ void __launch_bounds__(256) k_rlc_finalize_groups(int slots, int gs, int NC, const int32_t* __restrict__ sel,
                                                             const uint32_t* __restrict__ msm_out,
                                                             const uint32_t* __restrict__ qfix,
                                                             const int32_t* __restrict__ excl,
                                                             int32_t* __restrict__ status,
                                                             const int32_t* __restrict__ ipa_flag,
                                                             int32_t* __restrict__ gflag, int32_t* __restrict__ flag) {
  wave_prio<PS_FIN>();
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= slots) return;
  const int b = sel[j], g = j / gs;
  if (b < 0) return;
  if (excl && excl[b] && status[b] == 0) status[b] = FTS_E_NOT_RUN;
  G1J e = load_g1j(msm_out + (size_t)g * 24);
  add_inl(e, load_g1j(qfix + ((size_t)g * NC + NC - 1) * 24));
  const bool pass = g1j_is_identity(e);
  if (j % gs == 0) {  // a group's first slot is a real proof (padding trails)
    gflag[g] = pass ? 1 : 0;
    if (!pass) *flag = 0;
  }
  if (pass && status[b] == 0 && ipa_flag[b] != 0) status[b] = ipa_flag[b];
}

__global__ void __launch_bounds__(256) k_rlc_group_final(int slots, int gs, const int32_t* __restrict__ sel,
                                                         const uint32_t* __restrict__ msm_out,
                                                         int32_t* __restrict__ status,
                                                         const int32_t* __restrict__ ipa_flag,
                                                         int32_t* __restrict__ next, uint32_t* __restrict__ next_count) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= slots) return;
  const int b = sel ? sel[j] : j;
  if (b < 0 || status[b] != 0) return;
  Fp z;
  load_fp(msm_out + (size_t)(j / gs) * 24 + 16, z);
  if (f_is_zero(z)) {
    if (ipa_flag[b] != 0) status[b] = ipa_flag[b];
  } else {
    next[atomicAdd(next_count, 1u)] = b;
  }
}

// ------------------------------------------------------------ host launch
// column Q of the ungrouped combination (the only column that needs x0): RQ_PARTS partial
// sums over slices of proofs, their sum, and its fixed-base product -> r.fixed[NC - 1]
void launch_rlc_q_column(const RpBatchDev& d, const RlcDev& r, const uint32_t* tables, hipStream_t s, Timeline* tl) {
  const int B = d.B, n = d.n, k = d.k, NC = rlc_ncols(n);
  const int gsq = (B + RQ_PARTS - 1) / RQ_PARTS;  // proofs per partial sum
  hipLaunchKernelGGL(k_rlc_columns, dim3(1, RQ_PARTS), dim3(256), 0, s, B, n, k, gsq, NC - 1,
                     (const int32_t*)nullptr, d.ch, r.coef, d.ypow, d.svec, d.zvec, r.colsum + (size_t)NC * 8);
  hipLaunchKernelGGL(k_rlc_qsum, dim3(1), dim3(RQ_PARTS), 0, s, NC, NC - 1, r.colsum);
  FTS_LAUNCH(k_rlc_fixed, FB_NW, RF_ITEMS * FB_NW, s, n, 1, NC - 1, 1, r.colsum, tables, r.fixed);
  tl->mark("k_rlc_q", s, (double)B + FB_NW * 3 + (FB_NW - 1) * COST_ADD);
}

// the single-fault locator's device work on s, after a failed batch check of the
// (ungrouped) pass d: saves S, recomputes the combination with index weights into
// the same workspace (weights, columns, MSM, column Q) and writes to loc[0] the j
// with S' = (j + 1) S (loc[0] must be -1 before)
void launch_rlc_locate(const RpBatchDev& d, const RlcDev& r, const uint32_t* tables, uint32_t* save, int32_t* loc,
                       hipStream_t s, Timeline* tl) {
  const int B = d.B, n = d.n, k = d.k, NC = rlc_ncols(n);
  hipLaunchKernelGGL(k_rlc_total, dim3(1), dim3(64), 0, s, r.plan.out, r.fixed + (size_t)(NC - 1) * 24, save);
  FTS_LAUNCH(k_rlc_prep, B, 64, s, B, n, k, d.status, d.excl, d.ipa_flag, d.sc, d.ch, r.key, r.msc, r.coef, 1);
  tl->mark("k_rlc_prep", s, (double)B * (3 * k + 34));
  // alone on the GPU here: every column split over RQ_PARTS slices of proofs (NC x 64
  // blocks instead of NC), the partial rows then summed per column
  const int gsq = (B + RQ_PARTS - 1) / RQ_PARTS;
  hipLaunchKernelGGL(k_rlc_columns, dim3(NC - 1, RQ_PARTS), dim3(256), 0, s, B, n, k, gsq, 0,
                     (const int32_t*)nullptr, d.ch, r.coef, d.ypow, d.svec, d.zvec, r.colsum + (size_t)NC * 8);
  hipLaunchKernelGGL(k_rlc_qsum, dim3(NC - 1), dim3(RQ_PARTS), 0, s, NC, 0, r.colsum);
  tl->mark("k_rlc_columns", s, (double)B * 4 * n);
  FTS_LAUNCH(k_rlc_fixed, (size_t)(NC - 1) * FB_NW, RF_ITEMS * FB_NW, s, n, 1, 0, NC - 1, r.colsum, tables, r.fixed);
  tl->mark("k_rlc_fixed", s, (double)(NC - 1) * (FB_NW * 3 + (FB_NW - 1) * COST_ADD));
  launch_msm(r.plan, d.pts, r.msc, r.fixed, NC - 1, r.msm_scratch, s, s, tl);
  launch_rlc_q_column(d, r, tables, s, tl);
  FTS_LAUNCH(k_rlc_locate, B, 64, s, B, save, r.plan.out, r.fixed + (size_t)(NC - 1) * 24, loc);
  tl->mark("k_rlc_locate", s, (double)B * 28 * COST_ADD);
}
void launch_rlc_accept_except(int B, int skip, int32_t* status, const int32_t* ipa_flag, hipStream_t s) {
  FTS_LAUNCH(k_rlc_accept_except, B, 256, s, B, skip, status, ipa_flag);
}

// Group test of the batch check (after it failed): G groups of gs proof slots
// sel[g gs + j] (-1 = empty); every group's partial random linear combination
// (the batch check's weights) from per-group column sums + one grouped MSM
// (plan p: G groups of gs * npts points, indirection sel).  Groups that close
// accept their proofs; the proofs of the others are appended to next[] /
// next_count for the next round (smaller groups, or per-proof checks).
void launch_rlc_group_test(const RpBatchDev& d, const RlcDev& r, const uint32_t* tables, const MsmPlan& p,
                           const int32_t* sel, int G, int gs, uint32_t* gcol, uint32_t* gfix, int32_t* next,
                           uint32_t* next_count, hipStream_t s, Timeline* tl) {
  const int n = d.n, k = d.k;
  const int NC = rlc_ncols(n);
  if (gs <= GT_SMALL_MAX) {
    const int nch = gt_nchunks(n);
    FTS_LAUNCH(k_rlc_group_cols_small, (size_t)G * nch, 256, s, d.B, n, k, G, gs, sel, d.ch, r.coef, d.ypow, d.svec,
               d.zvec, tables, gfix);
    // per group: NC fixed-base products; a lane's first one is copied into its accumulator
    tl->mark("k_rlc_group_cols", s, (double)G * (gs * 3.0 * n + NC * COST_FB_FRESH + (NC - nch) * COST_ADD));
    launch_msm_small(p, d.pts, r.msc, gfix, nch, s, tl);
    FTS_LAUNCH(k_rlc_group_final, (size_t)G * gs, 256, s, G * gs, gs, sel, p.out, d.status, d.ipa_flag, next,
               next_count);
    tl->mark("k_rlc_group_final", s, 0);
    return;
  }
  hipLaunchKernelGGL(k_rlc_columns, dim3(NC, G), dim3(gs <= 64 ? 64 : 256), 0, s, d.B, n, k, gs, 0, sel, d.ch,
                     r.coef, d.ypow, d.svec, d.zvec, gcol);
  tl->mark("k_rlc_group_columns", s, (double)G * gs * 4 * n);
  FTS_LAUNCH(k_rlc_fixed, (size_t)NC * G * FB_NW, RF_ITEMS * FB_NW, s, n, G, 0, NC, gcol, tables, gfix);
  tl->mark("k_rlc_group_fixed", s, (double)G * NC * (FB_NW * 3 + (FB_NW - 1) * COST_ADD));
  launch_msm(p, d.pts, r.msc, gfix, NC, r.msm_scratch, s, s, tl);
  FTS_LAUNCH(k_rlc_group_final, (size_t)G * gs, 256, s, G * gs, gs, sel, p.out, d.status, d.ipa_flag, next,
             next_count);
  tl->mark("k_rlc_group_final", s, 0);
}

hipError_t upload_wave_prio_rp_rlc(const int* p) { return upload_wave_prio(p); }

}  // namespace fts
