// Range-proof per-proof final equations: the fallback when the batch combination fails.
#include <algorithm>
#include "device/g1.hpp"
#include "device/fixed_base.hpp"
#include "device/glv.hpp"
#include "device/rp_kernels.hpp"
#include "device/rp_decls.hpp"
#include "device/transcript.hpp"
#include "device/helpers.hpp"
#include "device/coop.hpp"
#include "../../include/fts_gpu.h"

namespace fts {

// ------------------------------------------------------------------ terms
// term slots per proof: [0,1] E1 fixed (G, H); [2,3,4] E1 var (T1, T2, V);
// [5 .. 5+2n] E2 fixed (G_i, H_i, Q); [6+2n .. 6+2n+2k-1] E2 var (L_j, R_j)
inline __host__ __device__ int rp_nterms(int n, int k) { return 6 + 2 * n + 2 * k; }

FTS_DEV Fr s_vec(const uint32_t* C, int k, int i) {
  // s_i = prod_j x_j^{+1 if bit (k-1-j) of i else -1}
  Fr s = f_one<FrP>();
  for (int j = 0; j < k; j++) {
    Fr f;
    int bit = (i >> (k - 1 - j)) & 1;
    load_f(C + (CH_XJ + (bit ? 0 : k) + j) * 8, f);
    s = fr_mul(s, f);
  }
  return s;
}

// sel != nullptr: lanes cover the B proofs sel[0 .. B) (the group test's failing
// proofs) instead of proofs 0 .. B
__global__ void __launch_bounds__(64) k_rp_terms_fixed(int B, int n, int k, const int32_t* __restrict__ sel,
                                                       const int32_t* __restrict__ status,
                                                       const int32_t* __restrict__ ipa_flag,
                                                       const uint32_t* __restrict__ sc, const uint32_t* __restrict__ ch,
                                                       const uint32_t* __restrict__ tables, uint32_t* __restrict__ terms) {
  const int nf = 3 + 2 * n;  // 2 (E1) + 2n + 1 (E2)
  int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= B * nf) return;
  int b = gid / nf, t = gid % nf;
  if (sel) b = sel[b];
  if (status[b] != 0) return;
  const uint32_t* C = ch + (size_t)b * rp_nch(k) * 8;
  const uint32_t* S = sc + (size_t)b * RP_NSC * 8;
  int slot, base;
  Fr s;
  if (t < 2) {
    slot = t;
    if (t == 0) {  // (ip - polEval) * G
      Fr pol;
      load_f(C + CH_POL * 8, pol);
      s = f_sub(fr_from_canon(S + RP_SC_IP * 8), pol);
      base = tb_G(n);
    } else {  // tau * H
      s = fr_from_canon(S + RP_SC_TAU * 8);
      base = tb_H(n);
    }
  } else {
    slot = 5 + (t - 2);
    if (ipa_flag[b] != 0) {
      store_g1j(terms + ((size_t)b * rp_nterms(n, k) + slot) * 24, g1j_identity());
      return;
    }
    int e = t - 2;
    if (e < n) {  // a * s_i * G_i
      s = fr_mul(fr_from_canon(S + RP_SC_A * 8), s_vec(C, k, e));
      base = e;
    } else if (e < 2 * n) {  // b * s_i^-1 * y^-i * H_i   (s_i^-1 = s_{n-1-i})
      int i = e - n;
      Fr yinv;
      load_f(C + CH_YINV * 8, yinv);
      s = fr_mul(fr_mul(fr_from_canon(S + RP_SC_B * 8), s_vec(C, k, n - 1 - i)), fr_pow_small(yinv, (uint32_t)i));
      base = n + i;
    } else {  // (a*b - ip) * x0 * Q
      Fr x0;
      load_f(C + CH_X0 * 8, x0);
      Fr ab = fr_mul(fr_from_canon(S + RP_SC_A * 8), fr_from_canon(S + RP_SC_B * 8));
      s = fr_mul(f_sub(ab, fr_from_canon(S + RP_SC_IP * 8)), x0);
      base = tb_Q(n);
    }
  }
  G1J r = nl_fb_mul(tables + (size_t)base * FB_WORDS_PER_BASE, fr_canon(s));
  store_g1j(terms + ((size_t)b * rp_nterms(n, k) + slot) * 24, r);
}

// the same terms with COOP_G lanes per product (device/coop.hpp): 12 products
// per wave, each doubling 3 product levels instead of 7 and each addition 5
// instead of 16, tables of 1..8 P and 1..8 phi(P) in LDS.  For a few
// thousand products on an otherwise idle GPU (the group test's last stage
// after a small failing group set) the chain latency, not the work, bounds the
// stage; the results are the same Jacobian triples as glv_mul's.
constexpr int TV_GPW = 64 / COOP_G;  // products per wave
constexpr size_t TV_COOP_MAX = 16384; // products up to which the cooperative form runs (~1,400 waves)
__global__ void __launch_bounds__(64) k_rp_terms_var_coop(int B, int n, int k, const int32_t* __restrict__ sel,
                                                          const int32_t* __restrict__ status,
                                                          const int32_t* __restrict__ ipa_flag,
                                                          const uint32_t* __restrict__ pts,
                                                          const uint32_t* __restrict__ ch,
                                                          uint32_t* __restrict__ terms) {
  __shared__ uint32_t T[TV_GPW][16][24];
  const int nv = 3 + 2 * k;
  const int lt = threadIdx.x, gi = lt / COOP_G, role = lt % COOP_G, base = gi * COOP_G;
  if (gi >= TV_GPW) return;  // lanes 60..63: no group
  const int item = blockIdx.x * TV_GPW + gi;
  if (item >= B * nv) return;  // whole groups leave together
  int b = item / nv;
  const int t = item % nv;
  if (sel) b = sel[b];
  if (status[b] != 0) return;
  const uint32_t* C = ch + (size_t)b * rp_nch(k) * 8;
  const uint32_t* Pt = pts + (size_t)b * rp_npts(k) * 16;
  int slot, pt;
  Fr s;
  if (t < 3) {
    slot = 2 + t;
    const int chi = t == 0 ? CH_X : (t == 1 ? CH_X2 : CH_Z2);
    load_f(C + chi * 8, s);
    pt = t == 0 ? RP_PT_T1 : (t == 1 ? RP_PT_T2 : RP_PT_V);
  } else {
    slot = 6 + 2 * n + (t - 3);
    if (ipa_flag[b] != 0) {
      if (role == 0) store_g1j(terms + ((size_t)b * rp_nterms(n, k) + slot) * 24, g1j_identity());
      return;
    }
    int j = t - 3;
    if (j < k) {
      load_f(C + (CH_XJ + j) * 8, s);
      pt = RP_PT_L + j;
    } else {
      j -= k;
      load_f(C + (CH_XJ + k + j) * 8, s);
      pt = RP_PT_L + k + j;
    }
    s = fr_sqr(s);
  }
  const G1A pa = load_g1a(Pt + pt * 16);
  G1J acc = g1j_identity();
  if (!g1a_is_identity(pa)) {
    const Scalar sk = fr_canon(f_neg(s));
    uint32_t k1[4], k2[4], s1, s2;
    glv_decompose(sk.v, k1, s1, k2, s2);
    G1J P = g1j_from_affine(pa), Q = P;
    Q.x = fp_mul(Q.x, glv_beta());
    if (s1) P.y = f_neg(P.y);
    if (s2) Q.y = f_neg(Q.y);
    uint32_t(*tb)[24] = T[gi];
    // 1..8 P, 1..8 Q (every lane of the group writes the same words)
    for (int h = 0; h < 2; h++) {
      const G1J t0 = h ? Q : P;
      G1J cur = t0;
      store_g1j(tb[8 * h], cur);
      cur = coop_dbl(t0, role, base);
      store_g1j(tb[8 * h + 1], cur);
      for (int e = 2; e < 8; e++) {
        coop_add(cur, t0, role, base);
        store_g1j(tb[8 * h + e], cur);
      }
    }
    const uint32_t ca = recode_carries(k1), cb = recode_carries(k2);
    for (int w = 31; w >= 0; w--) {
      const int da = window_digit(k1, ca, w), db = window_digit(k2, cb, w);
      if (w != 31)
        for (int r = 0; r < 4; r++) acc = coop_dbl(acc, role, base);
      if (da != 0) {
        G1J q = load_g1j(tb[(da < 0 ? -da : da) - 1]);
        if (da < 0) q.y = f_neg(q.y);
        coop_add(acc, q, role, base);
      }
      if (db != 0) {
        G1J q = load_g1j(tb[8 + (db < 0 ? -db : db) - 1]);
        if (db < 0) q.y = f_neg(q.y);
        coop_add(acc, q, role, base);
      }
    }
  }
  if (role == 0) store_g1j(terms + ((size_t)b * rp_nterms(n, k) + slot) * 24, acc);
}

__global__ void __launch_bounds__(64) k_rp_terms_var(int B, int n, int k, const int32_t* __restrict__ sel,
                                                     const int32_t* __restrict__ status,
                                                     const int32_t* __restrict__ ipa_flag,
                                                     const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ch,
                                                     uint32_t* __restrict__ terms, uint32_t* __restrict__ scratch) {
  const int nv = 3 + 2 * k;
  int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= B * nv) return;
  int b = gid / nv, t = gid % nv;
  if (sel) b = sel[b];
  if (status[b] != 0) return;
  const uint32_t* C = ch + (size_t)b * rp_nch(k) * 8;
  const uint32_t* Pt = pts + (size_t)b * rp_npts(k) * 16;
  int slot, pt;
  Fr s;
  if (t < 3) {
    slot = 2 + t;
    int chi = t == 0 ? CH_X : (t == 1 ? CH_X2 : CH_Z2);
    load_f(C + chi * 8, s);
    pt = t == 0 ? RP_PT_T1 : (t == 1 ? RP_PT_T2 : RP_PT_V);
  } else {
    slot = 6 + 2 * n + (t - 3);
    if (ipa_flag[b] != 0) {
      store_g1j(terms + ((size_t)b * rp_nterms(n, k) + slot) * 24, g1j_identity());
      return;
    }
    int j = t - 3;
    if (j < k) {  // x_j^2 * L_j
      load_f(C + (CH_XJ + j) * 8, s);
      s = fr_sqr(s);
      pt = RP_PT_L + j;
    } else {  // x_j^-2 * R_j
      j -= k;
      load_f(C + (CH_XJ + k + j) * 8, s);
      s = fr_sqr(s);
      pt = RP_PT_L + k + j;
    }
  }
  // all variable terms enter with a minus sign; GLV + joint Straus (124 doublings)
  G1J r = glv_mul(load_g1a(Pt + pt * 16), fr_canon(f_neg(s)), scratch, (size_t)B * nv, (size_t)gid);
  store_g1j(terms + ((size_t)b * rp_nterms(n, k) + slot) * 24, r);
}

// ------------------------------------------------------------------ check
// CK_LANES lanes per proof: E1 (5 terms) on lane 0; E2 (-com + the 1 + 2n + 2k
// other terms, 81 at n = 64) as CK_LANES partial sums + a 4-level LDS tree
// instead of one chain of ~80 additions.  Group addition is associative, so the
// verdict (identity or not) is the same.
constexpr int CK_LANES = 16, CK_PROOFS = 16;
__global__ void __launch_bounds__(CK_LANES * CK_PROOFS) k_rp_check(int B, int n, int k, const int32_t* __restrict__ sel,
                                                                   int32_t* __restrict__ status,
                                                                   const int32_t* __restrict__ ipa_flag,
                                                                   const uint32_t* __restrict__ terms,
                                                                   const uint32_t* __restrict__ hpa) {
  __shared__ uint32_t sh[CK_LANES * CK_PROOFS * 24];
  __shared__ int e1_ok[CK_PROOFS];
  const int l = threadIdx.x % CK_LANES, pl = threadIdx.x / CK_LANES;
  const int bi = blockIdx.x * CK_PROOFS + pl;
  int b = bi < B ? (sel ? sel[bi] : bi) : -1;
  const bool live = b >= 0 && status[b] == 0;
  const uint32_t* T = live ? terms + (size_t)b * rp_nterms(n, k) * 24 : terms;
  if (live && l == 0) {
    G1J e1 = load_g1j(T);
    for (int t = 1; t < 5; t++) e1 = nl_add_mem(e1, T + t * 24, 0);
    e1_ok[pl] = g1j_is_identity(e1);
  }
  G1J acc = g1j_identity();
  if (live) {
    if (l == 0) acc = g1j_from_affine(g1a_neg(load_g1a(hpa + ((size_t)b * (n + 1) + n) * 16)));
    for (int t = 5 + l; t < rp_nterms(n, k); t += CK_LANES) add_inl(acc, load_g1j(T + t * 24));
  }
  uint32_t* S = sh + (size_t)pl * CK_LANES * 24;
  store_g1j(S + l * 24, acc);
  __syncthreads();
  for (int half = CK_LANES / 2; half >= 1; half >>= 1) {
    if (live && l < half) add_inl(acc, load_g1j(S + (l + half) * 24));
    __syncthreads();
    if (live && l < half) store_g1j(S + l * 24, acc);
    __syncthreads();
  }
  if (!live || l != 0) return;
  if (!e1_ok[pl]) {
    status[b] = FTS_E_RP_INVALID;
  } else if (ipa_flag[b] != 0) {
    status[b] = ipa_flag[b];
  } else {
    status[b] = g1j_is_identity(acc) ? FTS_OK : FTS_E_IPA_INVALID;
  }
}

size_t rp_scratch_words(int B, int n, int k) {
  // per-proof fallback: 16-entry GLV lane tables of the 3 + 2k variable terms
  return std::max((size_t)B * (3 + 2 * k) * 16 * 24, (size_t)B * (HS_SCRATCH + 2 * ATAB_WORDS));
}
size_t rp_terms_words(int B, int n, int k) { return (size_t)B * rp_nterms(n, k) * 24; }

// ------------------------------------------------------------ host launch
// per-proof final equations of the nsel proofs sel[0 .. nsel) (all B if sel == nullptr)
void launch_rp_fallback(const RpBatchDev& d, const uint32_t* tables, const int32_t* sel, int nsel, hipStream_t s,
                        Timeline* tl) {
  const int B = sel ? nsel : d.B, n = d.n, k = d.k;
  FTS_LAUNCH(k_rp_terms_fixed, B * (3 + 2 * n), 64, s, B, n, k, sel, d.status, d.ipa_flag, d.sc, d.ch, tables, d.terms);
  tl->mark("k_rp_terms_fixed", s, (double)B * (3 + 2 * n) * COST_FB_FRESH);
  const size_t nvar = (size_t)B * (3 + 2 * k);
  if (nvar <= TV_COOP_MAX)  // latency-bound: lane-cooperative chains
    FTS_LAUNCH(k_rp_terms_var_coop, (nvar + TV_GPW - 1) / TV_GPW * 64, 64, s, B, n, k, sel, d.status, d.ipa_flag, d.pts,
               d.ch, d.terms);
  else
    FTS_LAUNCH(k_rp_terms_var, nvar, 64, s, B, n, k, sel, d.status, d.ipa_flag, d.pts, d.ch, d.terms, d.scratch);
  tl->mark("k_rp_terms_var", s, (double)B * (3 + 2 * k) * (4.0 * 7.0 + 12.0 * COST_ADD + 124 * COST_DBL + 60 * COST_ADD));
  if (B > 0)
    hipLaunchKernelGGL(k_rp_check, dim3((B + CK_PROOFS - 1) / CK_PROOFS), dim3(CK_LANES * CK_PROOFS), 0, s, B, n, k,
                       sel, d.status, d.ipa_flag, d.terms, d.hpa);
  tl->mark("k_rp_check", s, (double)B * rp_nterms(n, k) * COST_ADD);
}

}  // namespace fts
