// Idemix owner identities generated on the device: the prover of the association proof
// that k_idv_* (idv_kernels.hpp) verify.  Reference: KeyManager.Identity
// (token/services/identity/idemix/km.go:173-290) -> Csp.Sign(IdemixSignerOpts{4 hidden
// attributes, RhIndex 3, EidIndex 2, EidNymRhNym}) = IBM/idemix NewSignature, restated in
// oracle/idemix_identity.py sign.
//
// One wallet has one credential (A, B, E, S, attrs; user secret sk), so with 16-bit window
// tables of A and B beside the issuer's seven, every point of the proof is a sum of
// fixed-base products (no variable-base chain, no pairing):
//   Nym    = (HSk sk) + HRand rnym          A'   = A r1
//   ABar   = B r1 - A (r1 E)                B'   = B r1 - HRand r2
//   t1     = A (r1 rE) + HRand rR2          t3   = HSk rSk + HRand rRNym
//   t2     = HRand (rS' - r2 rR3) + B (r1 rR3) + HSk rSk + sum HAttrs[i] rAttrs[i]
//   EidNym = (HAttrs[2] a_eid) + HRand r_eid,  t4 = HAttrs[2] rAttrs[2] + HRand rr_eid
//   RhNym, t5: the same with HAttrs[3], a_rh, r_rh, rr_rh
// (the parenthesised points are constants of the credential, held affine).  Each is
// group-equal to the reference's expression, so its affine bytes are equal.
//
// Kernels, per curve (idemix_idgen_<cv>.hip):
//   k_idg_cred    one lane, at handle creation: B == g1 + HRand S + HSk sk + sum HAttrs[i]
//                 attrs[i] (Credential.Ver's B check) and the three constant points
//   k_idg_prep    lane per identity: the scalar prework in Fr (r3 = 1 / r1, r1 E, r1 rE,
//                 r1 rR3, rS' - r2 rR3, S' = S - r2 r3) -> the 19 product scalars
//   k_idg_points  lane per (output point, identity), identities fastest (a wave gathers
//                 from one table): the point's products summed in ONE accumulator, mixed
//                 additions only.  B r1, HSk rSk and HAttrs[2, 3] rAttrs[2, 3] serve two
//                 points each and are summed into both (23 table walks for the 19 distinct
//                 products): no Jacobian + Jacobian addition and 11, not 19, points of
//                 scratch per identity
//   k_idg_finish  lane per identity: the 11 transcript points to affine with one inversion
//                 (Montgomery's trick), the Fiat-Shamir transcript of k_idv_tvals (hashed by
//                 the same sink_digest and nonce_challenge), c, the 12 responses;
//                 six points and thirteen scalars (c and the responses) out, in wire byte order
// Not hardened against timing side channels (table indices and branches depend on secrets).
#pragma once
#include "idv_kernels.hpp"

namespace idv {

// affine Montgomery point (identity: zeros) -> X || Y as 16 big-endian words (the bytes of
// G1.Bytes() after the curve's prefix; AMCL writes infinity as 0 || 1)
template <class CV>
FTS_DEV void point_be_words(const typename CV::F& x, const typename CV::F& y, uint32_t pw[16]) {
  if constexpr (std::is_same<CV, BnCurve>::value) {
    g1_mont_to_be_words(x, y, pw);
  } else {
    const fbn::Fp ax = p256::from_mont(x);
    fbn::Fp ay = p256::from_mont(y);
    if (fbn::is_zero(ax) && fbn::is_zero(ay)) ay.v[0] = 1u;
#pragma unroll
    for (int k = 0; k < 8; k++) pw[k] = ax.v[7 - k], pw[8 + k] = ay.v[7 - k];
  }
}

// ---------------------------------------------------------------- the plan
// product p: its table (0..6 the issuer's HSk, HRand, HAttrs[0..3], g1; 7 A; 8 B)
__device__ constexpr int IDG_P_BASE[IDG_NPROD] = {B_HRAND, 7, 8, 7, B_HRAND, 7, B_HRAND, B_HRAND, 8, B_HSK,
                                                  B_HA + 0, B_HA + 1, B_HA + 2, B_HA + 3, B_HRAND, B_HRAND,
                                                  B_HRAND, B_HRAND, B_HRAND};
// output point q (transcript order t1 t2 t3 A' ABar B' Nym EidNym t4 RhNym t5): its products
// TERM_P[TERM_START[q] .. TERM_START[q + 1]) and its constant point (-1: none)
__device__ constexpr int IDG_TERM_START[IDG_NPT + 1] = {0, 2, 9, 11, 12, 14, 16, 17, 18, 20, 21, 23};
__device__ constexpr int IDG_TERM_P[23] = {5, 6, 7, 8, 9, 10, 11, 12, 13, 9, 14, 1, 2, 3, 2, 4, 0, 15, 12, 16, 17, 13, 18};
__device__ constexpr int IDG_Q_CONST[IDG_NPT] = {-1, -1, -1, -1, -1, -1, 0, 1, -1, 2, -1};
// output point q -> its place among the six written points (A' ABar B' Nym EidNym RhNym), -1: a t-value
__device__ constexpr int IDG_Q_OUT[IDG_NPT] = {-1, -1, -1, 0, 1, 2, 3, 4, -1, 5, -1};
// draws (host/identity_write.hpp D_*) and the credential's secrets (sk E S attrs[0..3])
constexpr int GD_RNYM = 0, GD_R1 = 1, GD_R2 = 2, GD_NONCE = 3, GD_RSK = 4, GD_RE = 5, GD_RR2 = 6, GD_RR3 = 7, GD_RSP = 8,
              GD_RRNYM = 9, GD_RA = 10, GD_REID = 14, GD_RRH = 15, GD_RREID = 16, GD_RRRH = 17;
constexpr int GS_SK = 0, GS_E = 1, GS_S = 2, GS_ATTR = 3;
constexpr int GSC_R3 = IDG_NPROD, GSC_SP = IDG_NPROD + 1;  // beside the product scalars
static_assert(IDG_NSC == IDG_NPROD + 2, "scalar slots");

// ----------------------------------------------------------------- kernels
// ab: A then B, affine Montgomery (16 words each); sec: sk E S attrs (IDG_SEC_WORDS);
// cpt <- HSk sk, HAttrs[2] attrs[2], HAttrs[3] attrs[3] affine Montgomery, then a mask of
// the ones at infinity (IDG_CPT_WORDS); ok[0] <- the B check
template <class CV>
__global__ void __launch_bounds__(64) k_idg_cred(const uint32_t* __restrict__ tables, const uint32_t* __restrict__ ab,
                                                 const uint32_t* __restrict__ sec, uint32_t* __restrict__ cpt,
                                                 int32_t* __restrict__ ok) {
  using B = typename CV::B;
  using F = typename CV::F;
  using PJ = typename CV::PJ;
  if (blockIdx.x || threadIdx.x) return;
  const uint32_t one[8] = {1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
  PJ acc = CV::inf();
  CV::fixed_mul_acc(acc, tables, B_G1, one);
  CV::fixed_mul_acc(acc, tables, B_HRAND, sec + 8 * GS_S);
  CV::fixed_mul_acc(acc, tables, B_HSK, sec + 8 * GS_SK);
#pragma unroll 1
  for (int a = 0; a < 4; a++) CV::fixed_mul_acc(acc, tables, B_HA + a, sec + 8 * (GS_ATTR + a));
  bool good = !CV::is_inf(acc);
  if (good) {
    const F z2 = B::mul(acc.z, acc.z), z3 = B::mul(z2, acc.z);
    good = B::eq(B::mul(B::ld(ab + 16), z2), acc.x) && B::eq(B::mul(B::ld(ab + 24), z3), acc.y);
  }
  ok[0] = good ? 1 : 0;
  uint32_t infm = 0;
#pragma unroll 1
  for (int j = 0; j < 3; j++) {
    PJ p = CV::inf();
    CV::fixed_mul_acc(p, tables, j == 0 ? B_HSK : B_HA + 1 + j, sec + 8 * (j == 0 ? GS_SK : GS_ATTR + 1 + j));
    F x = B::zero(), y = B::zero();
    if (CV::is_inf(p)) {
      infm |= 1u << j;
    } else {
      const F zi = B::inv(p.z), zi2 = B::mul(zi, zi);
      x = B::mul(p.x, zi2), y = B::mul(B::mul(p.y, zi2), zi);
    }
#pragma unroll
    for (int k = 0; k < 8; k++) cpt[16 * j + k] = x.v[k], cpt[16 * j + 8 + k] = y.v[k];
  }
  cpt[48] = infm;
}

// draws: [n][IDG_ND][8]; sc <- [IDG_NSC][n][8]
template <class CV>
__global__ void __launch_bounds__(256) k_idg_prep(int n, const uint32_t* __restrict__ draws,
                                                  const uint32_t* __restrict__ sec, uint32_t* __restrict__ sc,
                                                  const int32_t* __restrict__ status) {
  using Z = Zr<CV>;
  using T = typename Z::Z;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || status[i] != FTS_OK) return;
  const uint32_t* D = draws + (size_t)i * IDG_ND * 8;
  auto put = [&](int slot, const T& v) {
    uint32_t* o = sc + ((size_t)slot * n + i) * 8;
#pragma unroll
    for (int k = 0; k < 8; k++) o[k] = v.v[k];
  };
  const T r1 = Z::ld(D + 8 * GD_R1), r2 = Z::ld(D + 8 * GD_R2), rR3 = Z::ld(D + 8 * GD_RR3);
  const T r1m = Z::to_mont(r1), r3m = Z::inv_m(r1m), rR3m = Z::to_mont(rR3);
  put(0, Z::ld(D + 8 * GD_RNYM));
  put(1, r1);
  put(2, r1);
  put(3, Z::neg(Z::mul(r1m, Z::ld(sec + 8 * GS_E))));
  put(4, Z::neg(r2));
  put(5, Z::mul(r1m, Z::ld(D + 8 * GD_RE)));
  put(6, Z::ld(D + 8 * GD_RR2));
  put(7, Z::sub(Z::ld(D + 8 * GD_RSP), Z::mul(rR3m, r2)));
  put(8, Z::mul(rR3m, r1));
  put(9, Z::ld(D + 8 * GD_RSK));
#pragma unroll 1
  for (int a = 0; a < 4; a++) put(10 + a, Z::ld(D + 8 * (GD_RA + a)));
  put(14, Z::ld(D + 8 * GD_RRNYM));
  put(15, Z::ld(D + 8 * GD_REID));
  put(16, Z::ld(D + 8 * GD_RREID));
  put(17, Z::ld(D + 8 * GD_RRH));
  put(18, Z::ld(D + 8 * GD_RRRH));
  put(GSC_R3, Z::from_mont(r3m));
  put(GSC_SP, Z::sub(Z::ld(sec + 8 * GS_S), Z::mul(r3m, r2)));
}

// lane g = q * n + i; pts <- [IDG_NPT][24][n] Jacobian
template <class CV>
__global__ void __launch_bounds__(256) k_idg_points(int n, const uint32_t* __restrict__ sc,
                                                    const uint32_t* __restrict__ itab,
                                                    const uint32_t* __restrict__ ctab,
                                                    const uint32_t* __restrict__ cpt, uint32_t* __restrict__ pts,
                                                    const int32_t* __restrict__ status) {
  using B = typename CV::B;
  using PJ = typename CV::PJ;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (size_t)IDG_NPT * n) return;
  const int q = (int)(g / n), i = (int)(g % n);
  if (status[i] != FTS_OK) return;
  PJ acc = CV::inf();
#pragma unroll 1
  for (int t = IDG_TERM_START[q]; t < IDG_TERM_START[q + 1]; t++) {
    const int p = IDG_TERM_P[t], b = IDG_P_BASE[p];
    CV::fixed_mul_acc(acc, b < NB ? itab : ctab, b < NB ? b : b - NB, sc + ((size_t)p * n + i) * 8);
  }
  const int cq = IDG_Q_CONST[q];
  if (cq >= 0 && !((cpt[48] >> cq) & 1u)) CV::madd_to(acc, B::ld(cpt + 16 * cq), B::ld(cpt + 16 * cq + 8));
  const LaneWords P{pts + (size_t)q * 24 * n, (size_t)n, (size_t)i};
  put_f<CV>(P, 0, acc.x);
  put_f<CV>(P, 8, acc.y);
  put_f<CV>(P, 16, acc.z);
}

// pre: [IDG_NPT * 8][n] words; msg: [MSG_MAX][n] bytes; out <- [n][IDG_OUT_WORDS]: the six
// points (X || Y) then c sSk sE sR2 sR3 sS' sAttrs[0..3] sRNym sEid sRh, big-endian bytes
template <class CV>
__global__ void __launch_bounds__(256) k_idg_finish(int n, const uint32_t* __restrict__ draws,
                                                    const uint32_t* __restrict__ sec,
                                                    const uint32_t* __restrict__ sc, uint32_t* __restrict__ pts,
                                                    uint32_t* __restrict__ pre_w, uint8_t* __restrict__ msg,
                                                    const uint32_t* __restrict__ ipk_hash,  // 8 BE words
                                                    uint32_t* __restrict__ out, const int32_t* __restrict__ status) {
  using B = typename CV::B;
  using F = typename CV::F;
  using Z = Zr<CV>;
  using T = typename Z::Z;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || status[i] != FTS_OK) return;
  const LaneWords PRE{pre_w, (size_t)n, (size_t)i};
  // the 11 points -> affine with one inversion (identity -> (0, 0))
  {
    F pre = B::one();
#pragma unroll 1
    for (int q = 0; q < IDG_NPT; q++) {
      const LaneWords P{pts + (size_t)q * 24 * n, (size_t)n, (size_t)i};
      put_f<CV>(PRE, q * 8, pre);
      const F z = get_f<CV>(P, 16);
      if (!B::is_zero(z)) pre = B::mul(pre, z);
    }
    F inv = B::inv(pre);
#pragma unroll 1
    for (int q = IDG_NPT - 1; q >= 0; q--) {
      const LaneWords P{pts + (size_t)q * 24 * n, (size_t)n, (size_t)i};
      const F z = get_f<CV>(P, 16);
      F ax = B::zero(), ay = B::zero();
      if (!B::is_zero(z)) {
        const F zi = B::mul(inv, get_f<CV>(PRE, q * 8));
        inv = B::mul(inv, z);
        const F zi2 = B::mul(zi, zi);
        ax = B::mul(get_f<CV>(P, 0), zi2);
        ay = B::mul(B::mul(get_f<CV>(P, 8), zi2), zi);
      }
      put_f<CV>(P, 0, ax);
      put_f<CV>(P, 8, ay);
    }
  }
  uint32_t* O = out + (size_t)i * IDG_OUT_WORDS;
  // transcript: label || t1 t2 t3 A' ABar B' Nym EidNym t4 RhNym t5 || ipk.Hash || Disclosure
  ByteSink M{msg, (size_t)n, (size_t)i};
  for (int k = 0; k < LABEL_LEN; k++) M.put_byte((uint8_t)LABEL[k]);
#pragma unroll 1
  for (int q = 0; q < IDG_NPT; q++) {
    const LaneWords P{pts + (size_t)q * 24 * n, (size_t)n, (size_t)i};
    uint32_t pw[16];
    point_be_words<CV>(get_f<CV>(P, 0), get_f<CV>(P, 8), pw);
    if (CV::G1_BYTES == 65) M.put_byte(0x04);
#pragma unroll  // said, not left to the heuristic: rolled, the FP256BN kernel takes 98 registers for 86
    for (int k = 0; k < 16; k++) M.put_word(pw[k]);
    const int o = IDG_Q_OUT[q];
    if (o >= 0)
      for (int k = 0; k < 16; k++) O[16 * o + k] = __builtin_bswap32(pw[k]);
  }
  for (int k = 0; k < 8; k++) M.put_word(ipk_hash[k]);
  M.put_word(0u);  // Disclosure: four hidden attributes
  uint32_t c1[8], nonce[8];
  T c;
  sink_digest<CV>(M, c1);
  const uint32_t* D = draws + (size_t)i * IDG_ND * 8;
#pragma unroll
  for (int k = 0; k < 8; k++) nonce[k] = D[8 * GD_NONCE + 7 - k];  // a draw: LE limbs
  nonce_challenge<CV>(c1, nonce, c.v);
  const T cm = Z::to_mont(c);
  uint32_t* S = O + 16 * 6;
  auto put = [&](int slot, const T& v) {
#pragma unroll
    for (int k = 0; k < 8; k++) S[8 * slot + k] = __builtin_bswap32(v.v[7 - k]);
  };
  auto scl = [&](int slot) { return Z::ld(sc + ((size_t)slot * n + i) * 8); };
  put(0, c);
  put(1, Z::add(Z::ld(D + 8 * GD_RSK), Z::mul(cm, Z::ld(sec + 8 * GS_SK))));
  put(2, Z::sub(Z::ld(D + 8 * GD_RE), Z::mul(cm, Z::ld(sec + 8 * GS_E))));
  put(3, Z::add(Z::ld(D + 8 * GD_RR2), Z::mul(cm, Z::ld(D + 8 * GD_R2))));
  put(4, Z::sub(Z::ld(D + 8 * GD_RR3), Z::mul(cm, scl(GSC_R3))));
  put(5, Z::add(Z::ld(D + 8 * GD_RSP), Z::mul(cm, scl(GSC_SP))));
#pragma unroll 1
  for (int a = 0; a < 4; a++) put(6 + a, Z::add(Z::ld(D + 8 * (GD_RA + a)), Z::mul(cm, Z::ld(sec + 8 * (GS_ATTR + a)))));
  put(10, Z::add(Z::ld(D + 8 * GD_RRNYM), Z::mul(cm, Z::ld(D + 8 * GD_RNYM))));
  put(11, Z::add(Z::ld(D + 8 * GD_RREID), Z::mul(cm, Z::ld(D + 8 * GD_REID))));
  put(12, Z::add(Z::ld(D + 8 * GD_RRRH), Z::mul(cm, Z::ld(D + 8 * GD_RRH))));
}

// ------------------------------------------------- per-curve launch sequences
template <class CV>
void launch_idgen_cred(const uint32_t* tables, const uint32_t* ab, const uint32_t* sec, uint32_t* cpt, int32_t* ok,
                       hipStream_t s) {
  k_idg_cred<CV><<<1, 64, 0, s>>>(tables, ab, sec, cpt, ok);
}
template <class CV>
hipError_t launch_idgen(const GenChain& c) {
  const unsigned g256 = (unsigned)((c.n + 255) / 256), gpt = (unsigned)(((size_t)IDG_NPT * c.n + 255) / 256);
  k_idg_prep<CV><<<g256, 256, 0, c.s>>>(c.n, c.draws, c.sec, c.sc, c.st);
  k_idg_points<CV><<<gpt, 256, 0, c.s>>>(c.n, c.sc, c.itab, c.ctab, c.cpt, c.pts, c.st);
  const hipError_t e = hipEventRecord(c.ev_mid, c.s);
  k_idg_finish<CV><<<g256, 256, 0, c.s>>>(c.n, c.draws, c.sec, c.sc, c.pts, c.pre, c.msg, c.hash, c.out, c.st);
  return e;
}

}  // namespace idv
