// Idemix identity validity on the device (idemix half):
// the association proof every idemix owner identity carries, checked for EVERY
// transfer input by the reference with no cache:
//   validator/validator_transfer.go:46 GetOwnerVerifier(tok.Owner)
//   -> core/common/deserializer.go:63-64 DeserializeVerifier
//   -> services/identity/idemix/deserializer.go:83 Deserialize(raw, true)
//   -> services/identity/idemix/crypto/deserializer.go:36-86 (proto, nym import)
//   -> crypto/id.go:74-108 verifyProof -> IBM/idemix Signature.Ver
//      (ExpectEidNymRhNym, four hidden attributes, rhIndex 3, eidIndex 2, no message).
// Restated in oracle/idemix_identity.py (pairing pinned by the reference's
// credential fixtures; the proof's transcript layout is unpinned).
//
// One identity per lane, two kernels per curve:
//   k_idv_tvals    decode the 7 points (nym key, A', ABar, B', Nym, EidNym, RhNym)
//                  and the epoch key, the error precedence, then the five
//                  t-values (6 variable-base GLV products over affine lane
//                  tables + 11 fixed-base products from the issuer's tables),
//                  one batch normalisation, the Fiat-Shamir transcript in lane
//                  scratch ([byte][lane]: coalesced byte stores), SHA-256 and
//                  c == HashToZr(c' || Nonce)
//   k_idv_pairing  e(W, A') * e(g2, -ABar) == 1 (device/pairing.hpp: precomputed
//                  lines of W and g2, multi-Miller loop, final exponentiation)
// Curves: BN254 (gnark; G1 64-byte raw encodings, 16-bit signed fixed-base
// tables) and FP256BN (AMCL; 0x04 || X || Y, 16-bit unsigned tables), behind a
// traits struct each (idemix_curves.hpp).  Kernels, device tables and the launch_*<CV> templates only:
// idemix_identity_<cv>.hip, idemix_pairing_<cv>.hip and idemix_bp_<cv>.hip instantiate
// one curve's launch sequences each (a curve's two pairing kernels are minutes of device
// compilation each; the units build in parallel), and the host code (api_idemix.cpp)
// sees device/launch.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../../include/fts_gpu.h"
#include "../common/chacha20.hpp"
#include "idemix_curves.hpp"  // BnCurve, FbnCurve, Zr, LaneWords, ByteSink
#include "idemix_hash.hpp"    // sink_digest, nonce_challenge, padded_word
#include "pairing.hpp"
#include "launch.hpp"
#include "../host/idemix_parse.hpp"  // the record layout (NPT, P_*, R_*, F_*, ...)

namespace idv {

using namespace fts;

// ------------------------------------------------------------- constants
// targets: t1..t5 = 0..4
__device__ constexpr int VAR_PT[NVAR] = {P_AP, -1, P_BP, P_NYM, P_EID, P_RH};  // -1: D = ABar - B'
__device__ constexpr int VAR_T[NVAR] = {0, 0, 1, 2, 3, 4};
// Fixed-base products and the t-value(s) each is added to: sSk HSk, sA2 HAttrs[2] and
// sA3 HAttrs[3] appear in t2 and again in t3 / t4 / t5 with the same scalar (the
// reference's t3 = HSk^sSk HRand^sRNym ..., t4 = HAttrs[eid]^sEid ..., t5 =
// HAttrs[rh]^sRh ...; IBM/idemix signature.go Ver), so each is computed once and
// added twice (FIX_T2; round 6: 14 -> 11 table gathers of 16 rows per identity)
__device__ constexpr int FIX_B[NFIX] = {B_HRAND, B_HRAND, B_HSK, B_HA + 0, B_HA + 1, B_HA + 2, B_HA + 3,
                                         B_G1,    B_HRAND, B_HRAND, B_HRAND};
__device__ constexpr int FIX_T[NFIX] = {0, 1, 1, 1, 1, 1, 1, 1, 2, 3, 4};
__device__ constexpr int FIX_T2[NFIX] = {-1, -1, 2, -1, -1, 3, 4, -1, -1, -1, -1};
// transcript: label || t1 t2 t3 A' ABar B' Nym EidNym t4 RhNym t5 || ipk.Hash || Disclosure (4 zero bytes)
constexpr char LABEL[] = "signWithEidNymRhNym";
constexpr int LABEL_LEN = 19;

// affine lane table of 1..8 * P: XY rows [8][L][16] | Z, PRE [16][8][L] words (GTab)
constexpr int AT_WORDS = 8 * 16 + 8 * 8 + 8 * 8;
template <class CV>
FTS_DEV void put_f(const LaneWords& T, size_t w0, const typename CV::F& a) {
#pragma unroll
  for (int q = 0; q < 8; q++) T.at(w0 + q) = a.v[q];
}
template <class CV>
FTS_DEV typename CV::F get_f(const LaneWords& T, size_t w0) {
  typename CV::F a;
#pragma unroll
  for (int q = 0; q < 8; q++) a.v[q] = T.at(w0 + q);
  return a;
}

// Lane table of 1..8 * P for the GLV chains (round 6 layout): the affine entries as
// 64-byte rows, entry-major ([8][L][16] words: a window lookup reads ONE row per lane,
// four 16-byte loads, where the [word][lane] layout touched up to sixteen 128-byte
// lines per word and wave), then the build's z's and running products [16][8][L].
struct GTab {
  uint32_t* base;
  size_t L, lane;
  FTS_DEV uint32_t* row(int e) const { return base + ((size_t)e * L + lane) * 16; }
  FTS_DEV LaneWords zw() const { return LaneWords{base + (size_t)8 * 16 * L, L, lane}; }
};
template <class CV>
FTS_DEV void row_put(uint32_t* p, const typename CV::F& x, const typename CV::F& y) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
  q[1] = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
  q[2] = make_uint4(y.v[0], y.v[1], y.v[2], y.v[3]);
  q[3] = make_uint4(y.v[4], y.v[5], y.v[6], y.v[7]);
}
template <class CV>
FTS_DEV void row_get(const uint32_t* p, typename CV::F& x, typename CV::F& y) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1], c = q[2], d = q[3];
  x.v[0] = a.x, x.v[1] = a.y, x.v[2] = a.z, x.v[3] = a.w, x.v[4] = b.x, x.v[5] = b.y, x.v[6] = b.z, x.v[7] = b.w;
  y.v[0] = c.x, y.v[1] = c.y, y.v[2] = c.z, y.v[3] = c.w, y.v[4] = d.x, y.v[5] = d.y, y.v[6] = d.z, y.v[7] = d.w;
}

// 1..8 * P (P Jacobian, not the identity) into the lane table T, normalised to
// affine with one inversion (Montgomery's trick over the eight z's)
template <class CV>
FTS_DEV void glv_table(const typename CV::PJ& P, const GTab& T) {
  using B = typename CV::B;
  using F = typename CV::F;
  using PJ = typename CV::PJ;
  const LaneWords Z = T.zw();
  PJ cur = P;
  F pre = P.z;
  for (int e = 0; e < 8; e++) {
    if (e == 1) cur = CV::dbl(P);
    if (e > 1) CV::add_to(cur, P);
    row_put<CV>(T.row(e), cur.x, cur.y);
    put_f<CV>(Z, e * 8, cur.z);
    if (e) pre = B::mul(pre, cur.z);
    put_f<CV>(Z, 64 + e * 8, pre);
  }
  F inv = B::inv(pre);
  for (int e = 7; e >= 0; e--) {
    F zi = inv;
    if (e > 0) {
      zi = B::mul(inv, get_f<CV>(Z, 64 + (e - 1) * 8));
      inv = B::mul(inv, get_f<CV>(Z, e * 8));
    }
    const F zi2 = B::mul(zi, zi);
    F x, y;
    row_get<CV>(T.row(e), x, y);
    row_put<CV>(T.row(e), B::mul(x, zi2), B::mul(B::mul(y, zi2), zi));
  }
}

// (-1)^s1 k1 * P + (-1)^s2 k2 * phi(P) over the table of glv_table: NW signed 4-bit
// windows from the top (magnitudes below 2^(4 NW - 1)), 4 (NW - 1) doublings,
// <= 2 NW mixed additions
template <class CV, int NW>
FTS_DEV typename CV::PJ glv_chain(const GTab& T, const uint32_t k1[4], uint32_t s1, const uint32_t k2[4],
                                  uint32_t s2) {
  using B = typename CV::B;
  using F = typename CV::F;
  using PJ = typename CV::PJ;
  const uint32_t c1 = recode_carries(k1), c2 = recode_carries(k2);
  const F beta = CV::beta();
  PJ acc = CV::inf();
  for (int w = NW - 1; w >= 0; w--) {
    const int d1 = window_digit(k1, c1, w), d2 = window_digit(k2, c2, w);
    F x1, y1, x2, y2;
    if (d1) row_get<CV>(T.row((d1 < 0 ? -d1 : d1) - 1), x1, y1);
    if (d2) row_get<CV>(T.row((d2 < 0 ? -d2 : d2) - 1), x2, y2);
    if (w != NW - 1)
      for (int r = 0; r < 4; r++) acc = CV::dbl(acc);
    if (d1) {
      if ((d1 < 0) != (s1 != 0)) y1 = B::neg(y1);
      CV::madd_to(acc, x1, y1);
    }
    if (d2) {
      if ((d2 < 0) != (s2 != 0)) y2 = B::neg(y2);
      CV::madd_to(acc, B::mul(x2, beta), y2);
    }
  }
  return acc;
}

// k * P (k canonical mod r, P Jacobian) by GLV: k = k1 + k2 lambda; one table of
// 1..8 * P, normalised with one inversion; phi(mP) = (beta x, y) read from the
// same entries; 32 signed 4-bit windows, 124 doublings, <= 64 mixed additions
template <class CV>
FTS_DEV typename CV::PJ glv_mul(const typename CV::PJ& P, const uint32_t k[8], const GTab& T) {
  uint32_t nz = 0;
#pragma unroll
  for (int q = 0; q < 8; q++) nz |= k[q];
  if (CV::is_inf(P) || !nz) return CV::inf();
  glv_table<CV>(P, T);
  uint32_t k1[4], k2[4], s1, s2;
  CV::decompose(k, k1, s1, k2, s2);
  return glv_chain<CV, 32>(T, k1, s1, k2, s2);
}

// G2 point (affine Montgomery Fp2) on the twist y^2 = x^3 + b'
template <class B>
FTS_DEV bool g2_on_twist(const pair::F2<B>& x, const pair::F2<B>& y) {
  const pair::F2<B> rhs = pair::add(pair::mul(pair::sqr(x), x), pair::f2_ld<B>(B::K::TWB[0]));
  return pair::eq(pair::sqr(y), rhs);
}
// 128 raw bytes (four 32-byte big-endian coordinates in the curve's ECP2 order) ->
// affine Montgomery; false if a coordinate is >= p or the point is off the twist.
// BN254 (gnark raw): X.A1 X.A0 Y.A1 Y.A0; FP256BN (AMCL): xa xb ya yb
template <class CV>
FTS_DEV bool decode_g2(const uint8_t* raw, pair::F2<typename CV::B>& x, pair::F2<typename CV::B>& y);
template <>
FTS_DEV bool decode_g2<BnCurve>(const uint8_t* raw, pair::F2<pair::BnField>& x, pair::F2<pair::BnField>& y) {
  uint32_t pw[16], qw[16];
  load_be_words(raw, pw);
  load_be_words(raw + 64, qw);
  Fp c[4];
#pragma unroll
  for (int k = 0; k < 8; k++) c[0].v[k] = pw[7 - k], c[1].v[k] = pw[15 - k], c[2].v[k] = qw[7 - k], c[3].v[k] = qw[15 - k];
  bool ok = true, zero = true;
  for (int q = 0; q < 4; q++) ok = ok && limbs_lt_mod<FpP>(c[q].v), zero = zero && f_is_zero(c[q]);
  if (!ok) return false;
  if (zero) return true;  // the identity's raw encoding
  x.b = f_to_mont(c[0]), x.a = f_to_mont(c[1]), y.b = f_to_mont(c[2]), y.a = f_to_mont(c[3]);
  return g2_on_twist<pair::BnField>(x, y);
}
template <>
FTS_DEV bool decode_g2<FbnCurve>(const uint8_t* raw, pair::F2<pair::FbnField>& x, pair::F2<pair::FbnField>& y) {
  uint32_t pw[16], qw[16];
  load_be_words(raw, pw);
  load_be_words(raw + 64, qw);
  uint32_t c[4][8];
#pragma unroll
  for (int k = 0; k < 8; k++) c[0][k] = pw[7 - k], c[1][k] = pw[15 - k], c[2][k] = qw[7 - k], c[3][k] = qw[15 - k];
  uint32_t any = 0;
  for (int q = 0; q < 4; q++) {
    if (!p256::lt256(c[q], fbn::PM::M)) return false;
    for (int k = 0; k < 8; k++) any |= c[q][k];
  }
  if (!any) return true;  // all zero: the identity (as the oracle's decoding)
  x.a = p256::to_mont(fbn::load<fbn::PM>(c[0])), x.b = p256::to_mont(fbn::load<fbn::PM>(c[1]));
  y.a = p256::to_mont(fbn::load<fbn::PM>(c[2])), y.b = p256::to_mont(fbn::load<fbn::PM>(c[3]));
  return g2_on_twist<pair::FbnField>(x, y);
}

// ---------------------------------------------------- BN254 G2 subgroup check
// gnark-crypto's G2Affine.SetBytes (under mathlib's NewG2FromBytes) rejects twist
// points outside the order-r subgroup; the twist's cofactor is not 1, so decode_g2's
// on-twist check alone fails open.  [r - 1] Q == -Q  <=>  [r] Q == O, by
// double-and-add over Jacobian Fp2 coordinates with complete handling of the
// exceptional additions (points of small order hit them).
template <class B>
struct G2J {
  pair::F2<B> x, y, z;
};
template <class B>
FTS_DEV void g2j_dbl(G2J<B>& p) {  // dbl-2009-l (a = 0); the identity (z = 0) stays the identity
  using namespace pair;
  const F2<B> A = sqr(p.x), Bq = sqr(p.y), C = sqr(Bq);
  const F2<B> D = dbl(sub(sub(sqr(add(p.x, Bq)), A), C));
  const F2<B> E = add(dbl(A), A);
  const F2<B> X3 = sub(sqr(E), dbl(D));
  const F2<B> Y3 = sub(mul(E, sub(D, X3)), dbl(dbl(dbl(C))));
  p.z = dbl(mul(p.y, p.z));
  p.x = X3;
  p.y = Y3;
}
template <class B>
FTS_DEV void g2j_madd(G2J<B>& p, const pair::F2<B>& qx, const pair::F2<B>& qy) {  // madd-2007-bl, complete
  using namespace pair;
  if (is_zero(p.z)) {
    p.x = qx, p.y = qy, p.z = f2_one<B>();
    return;
  }
  const F2<B> Z1Z1 = sqr(p.z);
  const F2<B> U2 = mul(qx, Z1Z1), S2 = mul(mul(qy, p.z), Z1Z1);
  const F2<B> H = sub(U2, p.x), r = sub(S2, p.y);
  if (is_zero(H)) {
    if (is_zero(r)) g2j_dbl(p);  // p == q
    else p.z = f2_zero<B>();     // p == -q
    return;
  }
  const F2<B> HH = sqr(H), I = dbl(dbl(HH)), J = mul(H, I), rr = dbl(r), V = mul(p.x, I);
  const F2<B> X3 = sub(sub(sqr(rr), J), dbl(V));
  const F2<B> Y3 = sub(mul(rr, sub(V, X3)), dbl(mul(p.y, J)));
  p.z = sub(sub(sqr(add(p.z, H)), Z1Z1), HH);
  p.x = X3;
  p.y = Y3;
}
// (qx, qy) affine Montgomery on the twist, not the identity
FTS_DEV bool g2_in_subgroup_bn(const pair::F2<pair::BnField>& qx, const pair::F2<pair::BnField>& qy) {
  using namespace pair;
  using B = BnField;
  // r - 1 of BN254 (254 bits, little-endian words)
  constexpr uint32_t RM1[8] = {0xf0000000u, 0x43e1f593u, 0x79b97091u, 0x2833e848u,
                               0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
  G2J<B> acc{f2_zero<B>(), f2_one<B>(), f2_zero<B>()};
#pragma unroll 1
  for (int bit = 253; bit >= 0; bit--) {
    g2j_dbl(acc);
    if ((RM1[bit >> 5] >> (bit & 31)) & 1u) g2j_madd(acc, qx, qy);
  }
  if (is_zero(acc.z)) return false;
  const F2<B> z2 = sqr(acc.z), z3 = mul(z2, acc.z);
  return eq(acc.x, mul(qx, z2)) && eq(acc.y, neg(mul(qy, z3)));
}

// ----------------------------------------------------------------- kernels
// lines of W (lane 0) and g2 (lane 1); wraw: W as 128 raw bytes; ok[0] <- W valid
template <class CV>
__global__ void __launch_bounds__(64) k_idv_lines(const uint8_t* __restrict__ wraw, uint32_t* __restrict__ lines,
                                                  int32_t* __restrict__ ok) {
  using B = typename CV::B;
  using K = typename B::K;
  const int t = threadIdx.x;
  if (t > 1) return;
  pair::F2<B> qx, qy;
  if (t == 0) {
    if (!decode_g2<CV>(wraw, qx, qy) || (pair::is_zero(qx) && pair::is_zero(qy))) {
      ok[0] = 0;
      return;
    }
    if constexpr (std::is_same<CV, BnCurve>::value) {  // gnark SetBytes: subgroup check
      if (!g2_in_subgroup_bn(qx, qy)) {
        ok[0] = 0;
        return;
      }
    }
    ok[0] = 1;
  } else {
    qx = pair::f2_ld<B>(K::GEN2[0]);
    qy = pair::f2_ld<B>(K::GEN2[1]);
  }
  pair::precompute_lines<B>(qx, qy, lines + (size_t)t * pair::n_lines<K>() * pair::LINE_WORDS);
}

// Lane scratch ([word][lane], n lanes each): S = t1..t5 accumulators (5 x 24),
// DP = decoded points (NPT x 16), IDM = identity mask of the decoded points (1),
// VR = the NVAR variable-base then NFIX fixed-base products (NSC x 24), TV = the
// variable-base products' GLV lane tables
// (NVAR x AT_WORDS; TV[0] doubles as the normalisation's prefix products)
FTS_DEV size_t sc_s(size_t) { return 0; }
FTS_DEV size_t sc_dp(size_t n) { return (size_t)5 * 24 * n; }
FTS_DEV size_t sc_idm(size_t n) { return sc_dp(n) + (size_t)NPT * 16 * n; }
FTS_DEV size_t sc_vr(size_t n) { return sc_idm(n) + ((n + 3) & ~size_t(3)); }  // keeps sc_tv 16-byte aligned (GTab rows)
FTS_DEV size_t sc_tv(size_t n) { return sc_vr(n) + (size_t)NSC * 24 * n; }

// Three kernels per batch (round 4; one lane per identity for everything left
// 1,024 waves at one per SIMD, 30 % of the MAD peak):
//   k_idv_decode  identity per lane: status (pre-set by the host for identity-
//                 level errors), point decoding in the reference's order of
//                 checks, pin[i] <- (A', -ABar) for the pairing kernel
//   k_idv_var     lane per (product, identity): the six GLV products and the
//                 eleven fixed-base products of the t-values, 17x the lanes
//   k_idv_tvals   identity per lane: sum the products into t1..t5,
//                 normalisation, transcript, challenge;
//                 zk[i] <- 1 if c == c''
template <class CV>
__global__ void __launch_bounds__(256) k_idv_decode(int n, const uint32_t* __restrict__ rec,
                                                    const uint8_t* __restrict__ pts, const uint8_t* __restrict__ epk,
                                                    uint32_t* __restrict__ scratch, uint32_t* __restrict__ pin,
                                                    int32_t* __restrict__ zk, int32_t* __restrict__ status,
                                                    const int32_t* __restrict__ eidx, const int32_t* __restrict__ g2ok) {
  using B = typename CV::B;
  using F = typename CV::F;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  zk[i] = 0;
  if (status[i] != FTS_OK) return;
  const uint32_t* R = rec + (size_t)i * REC_STRIDE;
  const uint8_t* P = pts + (size_t)i * NPT * 64;
  const uint32_t flags = R[R_FLAGS];
  const LaneWords DP{scratch + sc_dp(n), (size_t)n, (size_t)i};
  uint32_t okm = 0, idm = 0;
#pragma unroll 1
  for (int q = 0; q < NPT; q++) {
    F px, py;
    bool id;
    if (CV::decode(P + q * 64, px, py, id)) okm |= 1u << q;
    if (id) idm |= 1u << q;
    put_f<CV>(DP, q * 16, px);
    put_f<CV>(DP, q * 16 + 8, py);
  }
  scratch[sc_idm(n) + i] = idm;
  // NymPublicKey import (crypto/deserializer.go:49-56) precedes the proof
  if (!(okm & (1u << P_NYMPK))) {
    status[i] = FTS_E_ID_BADNYM;
    return;
  }
  if (flags & F_EARLY_MALFORMED) {
    status[i] = FTS_E_ID_MALFORMED;
    return;
  }
  if (flags & F_NO_EID) {
    status[i] = FTS_E_ID_NO_EIDNYM;
    return;
  }
  if (flags & F_NO_RH) {
    status[i] = FTS_E_ID_NO_RHNYM;
    return;
  }
  bool all = okm == (1u << NPT) - 1;
  {
    pair::F2<B> ex, ey;
    all = all && decode_g2<CV>(epk + (size_t)i * 128, ex, ey);
    // BN254: the key's subgroup check, once per distinct key (k_idv_g2_check)
    if (g2ok) all = all && g2ok[eidx[i]] != 0;
  }
  if (!all || (flags & F_LATE_MALFORMED)) {
    status[i] = FTS_E_ID_MALFORMED;
    return;
  }
  if (flags & F_REVOCATION) {
    status[i] = FTS_E_ID_REVOCATION;
    return;
  }
  if (idm & (1u << P_AP)) {
    status[i] = FTS_E_ID_APRIME;
    return;
  }
  // pairing inputs: A' and -ABar
  uint32_t* pq = pin + (size_t)i * 32;
  const F ax = get_f<CV>(DP, P_AP * 16), ay = get_f<CV>(DP, P_AP * 16 + 8);
  const F bx = get_f<CV>(DP, P_ABAR * 16), by = get_f<CV>(DP, P_ABAR * 16 + 8);
  const F nby = (idm & (1u << P_ABAR)) ? by : B::neg(by);
#pragma unroll
  for (int q = 0; q < 8; q++) pq[q] = ax.v[q], pq[8 + q] = ay.v[q], pq[16 + q] = bx.v[q], pq[24 + q] = nby.v[q];
}

// lane g = v * n + i: identities fastest, so a wave runs one product kind
template <class CV>
__global__ void __launch_bounds__(256) k_idv_var(int n, const uint32_t* __restrict__ rec,
                                                 const uint32_t* __restrict__ tables,
                                                 uint32_t* __restrict__ scratch, const int32_t* __restrict__ status) {
  using B = typename CV::B;
  using PJ = typename CV::PJ;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (size_t)NSC * n) return;
  const int v = (int)(g / n), i = (int)(g % n);
  if (status[i] != FTS_OK) return;
  const uint32_t* R = rec + (size_t)i * REC_STRIDE;
  const LaneWords VR{scratch + sc_vr(n) + (size_t)v * 24 * n, (size_t)n, (size_t)i};
  if (v >= NVAR) {  // fixed-base product (issuer tables)
    PJ acc = CV::inf();
    CV::fixed_mul_acc(acc, tables, FIX_B[v - NVAR], R + R_SC + v * 8);
    put_f<CV>(VR, 0, acc.x);
    put_f<CV>(VR, 8, acc.y);
    put_f<CV>(VR, 16, acc.z);
    return;
  }
  const LaneWords DP{scratch + sc_dp(n), (size_t)n, (size_t)i};
  const uint32_t idm = scratch[sc_idm(n) + i];
  const int pq_ = VAR_PT[v] < 0 ? P_ABAR : VAR_PT[v];
  PJ base = (idm >> pq_) & 1u ? CV::inf() : CV::from_affine(get_f<CV>(DP, pq_ * 16), get_f<CV>(DP, pq_ * 16 + 8));
  if (VAR_PT[v] < 0 && !((idm >> P_BP) & 1u))  // D = ABar - B'
    CV::madd_to(base, get_f<CV>(DP, P_BP * 16), B::neg(get_f<CV>(DP, P_BP * 16 + 8)));
  const GTab T{scratch + sc_tv(n) + (size_t)v * AT_WORDS * n, (size_t)n, (size_t)i};
  const PJ r = glv_mul<CV>(base, R + R_SC + v * 8, T);
  put_f<CV>(VR, 0, r.x);
  put_f<CV>(VR, 8, r.y);
  put_f<CV>(VR, 16, r.z);
}

template <class CV>
__global__ void __launch_bounds__(256) k_idv_tvals(int n, const uint32_t* __restrict__ rec,
                                                   const uint32_t* __restrict__ tables,
                                                   const uint32_t* __restrict__ ipk_hash,  // 8 BE words
                                                   uint32_t* __restrict__ scratch, uint8_t* __restrict__ msg,
                                                   int32_t* __restrict__ zk, const int32_t* __restrict__ status) {
  using B = typename CV::B;
  using F = typename CV::F;
  using PJ = typename CV::PJ;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || status[i] != FTS_OK) return;
  const uint32_t* R = rec + (size_t)i * REC_STRIDE;
  const uint32_t flags = R[R_FLAGS];
  const LaneWords DP{scratch + sc_dp(n), (size_t)n, (size_t)i};
  const uint32_t idm = scratch[sc_idm(n) + i];
  // t-values: accumulators t1..t5 in lane scratch ([word][lane]), Jacobian
  const LaneWords S{scratch + sc_s(n), (size_t)n, (size_t)i};
  const LaneWords T{scratch + sc_tv(n), (size_t)n, (size_t)i};
  for (int t = 0; t < 5; t++) {
    const PJ z = CV::inf();
    put_f<CV>(S, t * 24, z.x);
    put_f<CV>(S, t * 24 + 8, z.y);
    put_f<CV>(S, t * 24 + 16, z.z);
  }
#pragma unroll 1
  for (int v = 0; v < NSC; v++) {
    const LaneWords VR{scratch + sc_vr(n) + (size_t)v * 24 * n, (size_t)n, (size_t)i};
    PJ r;
    r.x = get_f<CV>(VR, 0), r.y = get_f<CV>(VR, 8), r.z = get_f<CV>(VR, 16);
    const int t1 = v < NVAR ? VAR_T[v] : FIX_T[v - NVAR], t2 = v < NVAR ? -1 : FIX_T2[v - NVAR];
    for (int t : {t1, t2}) {
      if (t < 0) continue;
      PJ acc;
      acc.x = get_f<CV>(S, t * 24), acc.y = get_f<CV>(S, t * 24 + 8), acc.z = get_f<CV>(S, t * 24 + 16);
      CV::add_to(acc, r);
      put_f<CV>(S, t * 24, acc.x);
      put_f<CV>(S, t * 24 + 8, acc.y);
      put_f<CV>(S, t * 24 + 16, acc.z);
    }
  }
  // the five t-values -> affine with one inversion (Montgomery's trick; identity -> (0, 0))
  {
    F pre = B::one();
    for (int t = 0; t < 5; t++) {
      put_f<CV>(T, t * 8, pre);
      const F z = get_f<CV>(S, t * 24 + 16);
      if (!B::is_zero(z)) pre = B::mul(pre, z);
    }
    F inv = B::inv(pre);
    for (int t = 4; t >= 0; t--) {
      const F z = get_f<CV>(S, t * 24 + 16);
      F ax = B::zero(), ay = B::zero();
      if (!B::is_zero(z)) {
        const F zi = B::mul(inv, get_f<CV>(T, t * 8));
        inv = B::mul(inv, z);
        const F zi2 = B::mul(zi, zi);
        ax = B::mul(get_f<CV>(S, t * 24), zi2);
        ay = B::mul(B::mul(get_f<CV>(S, t * 24 + 8), zi2), zi);
      }
      put_f<CV>(S, t * 24, ax);
      put_f<CV>(S, t * 24 + 8, ay);
    }
  }
  // transcript
  ByteSink M{msg, (size_t)n, (size_t)i};
  for (int k = 0; k < LABEL_LEN; k++) M.put_byte((uint8_t)LABEL[k]);
  // t1 t2 t3 A' ABar B' Nym EidNym t4 RhNym t5: tags >= 0 are t-values, < 0 points (-1 - index)
  constexpr int ORDER[11] = {0, 1, 2, -1 - P_AP, -1 - P_ABAR, -1 - P_BP, -1 - P_NYM, -1 - P_EID, 3, -1 - P_RH, 4};
  for (int q = 0; q < 11; q++) {
    const int tag = ORDER[q];
    if (tag >= 0) {
      CV::encode(M, get_f<CV>(S, tag * 24), get_f<CV>(S, tag * 24 + 8));
    } else {
      const int pi = -1 - tag;
      F zx = get_f<CV>(DP, pi * 16), zy = get_f<CV>(DP, pi * 16 + 8);
      if ((idm >> pi) & 1u) zx = B::zero(), zy = B::zero();
      CV::encode(M, zx, zy);
    }
  }
  for (int k = 0; k < 8; k++) M.put_word(ipk_hash[k]);
  M.put_word(0u);  // Disclosure: four hidden attributes
  uint32_t c1[8], c2[8];
  sink_digest<CV>(M, c1);
  nonce_challenge<CV>(c1, R + R_NONCE, c2);
  uint32_t diff = (flags & F_C_BIG) ? 1u : 0u;
#pragma unroll
  for (int k = 0; k < 8; k++) diff |= c2[k] ^ R[R_C + k];
  zk[i] = diff ? 0 : 1;
}

// e(W, A') * e(g2, -ABar) == 1, then the verdict (pairing before the ZK proof, as Ver checks)
// waves per SIMD the pairing kernel is compiled for (A/B: -DFTS_IDV_OCC=2 caps it
// at 256 registers, with spills in the inlined Fp12 bodies)
#ifndef FTS_IDV_OCC
#define FTS_IDV_OCC 1
#endif
template <class CV>
__global__ void __launch_bounds__(64, FTS_IDV_OCC) k_idv_pairing(int n, const uint32_t* __restrict__ pin,
                                                    const uint32_t* __restrict__ lines, const int32_t* __restrict__ zk,
                                                    int32_t* __restrict__ status, const int32_t* __restrict__ list,
                                                    const int32_t* __restrict__ count) {
  using B = typename CV::B;
  using K = typename B::K;
  using F = typename B::F;
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (list) {  // the identities of the groups whose batch check failed (k_idv_bp_sel)
    if (i >= *count) return;
    i = list[i];
  }
  if (i >= n || status[i] != FTS_OK) return;
  const uint32_t* pq = pin + (size_t)i * 32;
  const uint32_t* const L[2] = {lines, lines + (size_t)pair::n_lines<K>() * pair::LINE_WORDS};
  const F xP[2] = {B::ld(pq), B::ld(pq + 16)};
  const F yP[2] = {B::ld(pq + 8), B::ld(pq + 24)};
  pair::F12<B> f;
  if (B::is_zero(xP[1]) && B::is_zero(yP[1])) {  // ABar = O: e(g2, O) = 1
    const uint32_t* const L1[1] = {L[0]};
    const F x1[1] = {xP[0]}, y1[1] = {yP[0]};
    f = pair::miller<B, 1>(L1, x1, y1);
  } else {
    f = pair::miller<B, 2>(L, xP, yP);
  }
  const bool one = pair::is_one(pair::final_exp_i(f));
  status[i] = !one ? FTS_E_ID_PAIRING : (zk[i] ? FTS_OK : FTS_E_ID_ZK);
}

// ---- batch pairing check (round 6)
// The equations e(W, A'_i) e(g2, -ABar_i) = 1 of a group of BP_G identities are
// checked as ONE: e(W, sum rho_i A'_i) e(g2, sum rho_i (-ABar_i)) = 1, with secret
// weights rho_i = a_i + b_i lambda (a_i, b_i: 64-bit ChaCha20 words under a key drawn
// with getrandom for every call; the GLV lattice {(x, y): x + y lambda = 0 mod r} has
// no nonzero vector shorter than ~2^126, so the 2^128 pairs are 2^128 distinct rho
// mod r).  Pairing values live in the order-r subgroup of GT (r prime), so a group
// holding an identity whose equation fails passes with probability <= 2^-128 (the
// small-exponents batch test of Bellare, Garay and Rabin).  A group that fails has
// its identities paired one by one (k_idv_pairing over the k_idv_bp_sel list), so
// every verdict is the per-identity one.  Work per identity: two 64-bit GLV chains
// (17 windows) instead of a 2-pairing Miller loop and a final exponentiation.
// BP_G identities per group = threads of a k_idv_bp_terms block; its scratch layout
// (bp_*_off) is with the other size functions in idemix_identity_bn.hip.

// block = group g, blockIdx.y = which point (0: A', 1: -ABar): rho_i * P_i summed
// over the group's identities still OK (the others contribute O), LDS tree
template <class CV>
__global__ void __launch_bounds__(BP_G) k_idv_bp_terms(int n, const uint32_t* __restrict__ pin,
                                                       const int32_t* __restrict__ status, Key8 key,
                                                       uint32_t* __restrict__ scratch, uint32_t* __restrict__ part) {
  using B = typename CV::B;
  using F = typename CV::F;
  using PJ = typename CV::PJ;
  __shared__ uint32_t sh[24 * BP_G];
  const int t = threadIdx.x, which = blockIdx.y;
  const int i = blockIdx.x * BP_G + t;
  PJ r = CV::inf();
  if (i < n && status[i] == FTS_OK) {
    const uint32_t* pq = pin + (size_t)i * 32 + which * 16;
    const F x = B::ld(pq), y = B::ld(pq + 8);
    if (!(B::is_zero(x) && B::is_zero(y))) {  // -ABar = O: e(g2, O) = 1, no term
      uint32_t blk[16];
      fts::chacha20_block(key.k, (uint32_t)i, blk);
      const uint32_t a[4] = {blk[0], blk[1], 0u, 0u}, b[4] = {blk[2], blk[3], 0u, 0u};
      const GTab T{scratch + (size_t)which * AT_WORDS * n, (size_t)n, (size_t)i};
      glv_table<CV>(CV::from_affine(x, y), T);
      r = glv_chain<CV, 17>(T, a, 0u, b, 0u);
    }
  }
  const LaneWords S{sh, (size_t)BP_G, (size_t)t};
  put_f<CV>(S, 0, r.x);
  put_f<CV>(S, 8, r.y);
  put_f<CV>(S, 16, r.z);
  for (int h = BP_G / 2; h > 0; h >>= 1) {
    __syncthreads();
    if (t < h) {
      const LaneWords O{sh, (size_t)BP_G, (size_t)(t + h)};
      PJ a, b;
      a.x = get_f<CV>(S, 0), a.y = get_f<CV>(S, 8), a.z = get_f<CV>(S, 16);
      b.x = get_f<CV>(O, 0), b.y = get_f<CV>(O, 8), b.z = get_f<CV>(O, 16);
      CV::add_to(a, b);
      put_f<CV>(S, 0, a.x);
      put_f<CV>(S, 8, a.y);
      put_f<CV>(S, 16, a.z);
    }
  }
  __syncthreads();  // lane 0's last sum, read by lanes 0..23
  if (t < 24) part[((size_t)blockIdx.x * 2 + which) * 24 + t] = sh[(size_t)t * BP_G];
}

// lane pair per group (lanes 2g, 2g + 1 of one wave): lane h takes sum h to affine
// and runs its single-pair Miller loop (h = 0: W with the A' sum, h = 1: g2 with the
// -ABar sum; a sum at O contributes 1), lane 1 hands its Fp12 value to lane 0 by
// shuffles, and lane 0 multiplies, exponentiates and writes gok[g] <- 1 if the
// product is 1 in GT.  The two Miller loops run side by side instead of one 2-pair
// loop on one lane (the group check is a call's latency, not its device work).
// Lane 0 also clears the list counter.
template <class B>
FTS_DEV void shfl_f(typename B::F& a, int src) {
#pragma unroll
  for (int q = 0; q < 8; q++) a.v[q] = (uint32_t)__shfl((int)a.v[q], src, 64);
}
template <class B>
FTS_DEV void shfl_f12(pair::F12<B>& f, int src) {
  shfl_f<B>(f.c0.c0.a, src), shfl_f<B>(f.c0.c0.b, src), shfl_f<B>(f.c0.c1.a, src), shfl_f<B>(f.c0.c1.b, src);
  shfl_f<B>(f.c0.c2.a, src), shfl_f<B>(f.c0.c2.b, src), shfl_f<B>(f.c1.c0.a, src), shfl_f<B>(f.c1.c0.b, src);
  shfl_f<B>(f.c1.c1.a, src), shfl_f<B>(f.c1.c1.b, src), shfl_f<B>(f.c1.c2.a, src), shfl_f<B>(f.c1.c2.b, src);
}
template <class CV>
__global__ void __launch_bounds__(64, FTS_IDV_OCC) k_idv_bp_pair(int ng, const uint32_t* __restrict__ part,
                                                    const uint32_t* __restrict__ lines, int32_t* __restrict__ gok,
                                                    int32_t* __restrict__ count) {
  using B = typename CV::B;
  using K = typename B::K;
  using F = typename B::F;
  static_assert(64 % 2 == 0, "a group's lane pair must sit in one wave");
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  const int g = gid >> 1, h = gid & 1;
  if (gid == 0) *count = 0;
  // no early return before the shuffle: both lanes of every pair reach it
  const bool live = g < ng;
  const uint32_t* S = part + (size_t)(live ? g : 0) * 48 + h * 24;
  const F z = B::ld(S + 16);
  const bool o = !live || B::is_zero(z);
  pair::F12<B> f = pair::f12_one<B>();
  if (!o) {
    const F zi = B::inv(z), zi2 = B::mul(zi, zi);
    const F x1[1] = {B::mul(B::ld(S), zi2)}, y1[1] = {B::mul(B::mul(B::ld(S + 8), zi2), zi)};
    const uint32_t* const L1[1] = {lines + (size_t)h * pair::n_lines<K>() * pair::LINE_WORDS};
    f = pair::miller<B, 1>(L1, x1, y1);
  }
  pair::F12<B> f1 = f;
  shfl_f12<B>(f1, (threadIdx.x & ~1) | 1);
  if (h == 0 && live) gok[g] = pair::is_one(pair::final_exp_i(pair::mul12_i(f, f1))) ? 1 : 0;
}

// identity per lane: verdict of the identities of passing groups; the others are
// appended to the list k_idv_pairing pairs one by one
template <class CV>  // (per-curve instance: one per translation unit)
__global__ void __launch_bounds__(256) k_idv_bp_sel(int n, const int32_t* __restrict__ gok,
                                                    const int32_t* __restrict__ zk, int32_t* __restrict__ status,
                                                    int32_t* __restrict__ list, int32_t* __restrict__ count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || status[i] != FTS_OK) return;
  if (gok[i / BP_G]) {
    status[i] = zk[i] ? FTS_OK : FTS_E_ID_ZK;
    return;
  }
  list[atomicAdd(count, 1)] = i;
}

// debug: e(Q, P) for Q = W (which 0) or g2 (1), P affine as the curve's host hands it over
// (CV::HOST_MONT: Montgomery, else canonical limbs < p, converted here) -> GT (12 Fp2
// coefficients w^0..w^5 as (c0.c0, c1.c0, c0.c1, c1.c1, c0.c2, c1.c2), Montgomery LE limbs)
template <class CV>
__global__ void __launch_bounds__(64) k_idv_pairing_debug(const uint32_t* __restrict__ lines, int which, const uint32_t* __restrict__ p16,
                                    uint32_t* __restrict__ out, int final_exp) {
  using B = typename CV::B;
  using K = typename B::K;
  using F = typename B::F;
  if (threadIdx.x) return;
  const uint32_t* const L[1] = {lines + (size_t)which * pair::n_lines<K>() * pair::LINE_WORDS};
  F xP[1] = {B::ld(p16)}, yP[1] = {B::ld(p16 + 8)};
  if constexpr (!CV::HOST_MONT) xP[0] = p256::to_mont(xP[0]), yP[0] = p256::to_mont(yP[0]);
  pair::F12<B> f = pair::miller<B, 1>(L, xP, yP);
  if (final_exp) f = pair::final_exp_i(f);
  const pair::F2<B> z[6] = {f.c0.c0, f.c1.c0, f.c0.c1, f.c1.c1, f.c0.c2, f.c1.c2};
  for (int k = 0; k < 6; k++) {
    pair::store_f2(out + k * 16, z[k]);
  }
}

// ------------------------------------------------- per-curve launch sequences
// Declared in device/launch.hpp (with Chain); each instantiated once per curve, in one
// of that curve's translation units.
// decode, the t-value products, the t-values and the transcript
template <class CV>
void launch_tvals(const Chain& c) {
  const unsigned g256 = (unsigned)((c.n + 255) / 256), gvar = (unsigned)(((size_t)NSC * c.n + 255) / 256);
  k_idv_decode<CV><<<g256, 256, 0, c.s>>>(c.n, c.rec, c.pts, c.epk, c.scr, c.pin, c.zk, c.st, c.eidx, c.g2ok);
  k_idv_var<CV><<<gvar, 256, 0, c.s>>>(c.n, c.rec, c.tables, c.scr, c.st);
  k_idv_tvals<CV><<<g256, 256, 0, c.s>>>(c.n, c.rec, c.tables, c.hash, c.scr, c.msg, c.zk, c.st);
}
// the batch pairing check up to the list of identities to pair one by one
template <class CV>
void launch_batch(const Chain& c) {
  const size_t n = (size_t)c.n, ng = (n + BP_G - 1) / BP_G;
  k_idv_bp_terms<CV><<<dim3((unsigned)ng, 2), BP_G, 0, c.s>>>(c.n, c.pin, c.st, c.key, c.scr, c.scr + bp_part_off(n));
  k_idv_bp_pair<CV><<<(unsigned)((2 * ng + 63) / 64), 64, 0, c.s>>>((int)ng, c.scr + bp_part_off(n), c.lines, c.gok,
                                                                  c.cnt);
  k_idv_bp_sel<CV><<<(unsigned)((n + 255) / 256), 256, 0, c.s>>>(c.n, c.gok, c.zk, c.st, c.list, c.cnt);
}
// one-by-one pairings: `lanes` identities of the list (list) or all n
template <class CV>
void launch_pairing(const Chain& c, unsigned lanes, bool list) {
  k_idv_pairing<CV><<<(lanes + 63) / 64, 64, 0, c.s>>>(c.n, c.pin, c.lines, c.zk, c.st, list ? c.list : nullptr,
                                                        list ? c.cnt : nullptr);
}
template <class CV>
void launch_lines(const uint8_t* w, uint32_t* lines, int32_t* ok, hipStream_t s) {
  k_idv_lines<CV><<<1, 64, 0, s>>>(w, lines, ok);
}
template <class CV>
void launch_pairing_debug(const uint32_t* lines, int which, const uint32_t* p16, uint32_t* out, int final_exp,
                          hipStream_t s) {
  k_idv_pairing_debug<CV><<<1, 64, 0, s>>>(lines, which, p16, out, final_exp);
}

}  // namespace idv
