// Idemix enrolment on the device: the user's NewCredRequest, the issuer's CredRequest.Check
// and NewCredential (IBM/idemix bccsp/schemes/dlog/crypto credrequest.go, credential.go;
// reached in the reference through idemixgen and its CA: token/services/identity/idemix/
// testdata/generate.go, integration/nwo/token/common/ca.go), restated in
// tests/cred_issue_ref.py.
//
//   request   Nym = HSk sk, t = HSk rSk,
//             c = HashToZr("credRequest" || t || HSk || Nym || IssuerNonce || ipk.Hash),
//             s = rSk + c sk
//   check     t = HSk s - Nym c, accept iff c == HashToZr(the same bytes)
//   issue     B = g1 + Nym + HRand S + sum HAttrs[i] attrs[i], A = B (isk + E)^-1
// UNPINNED (no vector in the reference): the label "credRequest" and the field order of the
// request transcript, restated from the published idemix code.  The credential equation is
// pinned: what this issues is accepted by Credential.Ver (k_cred_*, cred_kernels.hpp).
//
// Kernels, per curve (idemix_credissue_<cv>.hip):
//   k_ci_request  lane per item: HSk sk and HSk rSk (two fixed-base products), both to affine
//                 with one inversion, the transcript, c, s; Nym c s out in wire byte order
//   k_ci_decode   lane per request: Nym decoded, not the identity; FTS_E_CREDREQ_MALFORMED
//   k_ci_var      lane per (product, request), requests fastest (a wave runs one product kind
//                 and gathers from one table): c Nym by GLV over a lane table, s HSk, and for
//                 an issue HRand S and HAttrs[i] attrs[i] -- the two bodies of k_cred_var
//   k_ci_check    lane per request: t to affine, the 267- / 270-byte transcript and its five
//                 compressions, the verdict (FTS_E_CREDREQ_INVALID); for an issue B summed in
//                 one accumulator, (isk + E)^-1, B to affine (one base-field inversion shared
//                 with t by Montgomery's trick)
//   k_ci_sign     lane per request: A = inv B by GLV over the same lane table, A to affine,
//                 A and B written as X || Y
// Lane scratch ([word][lane], n lanes each): DP = Nym decoded (16), VR = the products
// (7 x 24), BA = B affine (16), IV = (isk + E)^-1 (8), TV = the lane table (AT_WORDS):
// 464 words = 1,856 B per lane, and 320 transcript bytes, in global memory (no kernel here
// asks for private scratch beyond what the two product bodies already take in k_cred_var).
// Not hardened against timing side channels (table indices and branches depend on secrets).
#pragma once
#include "idgen_kernels.hpp"  // point_be_words

namespace idv {

constexpr char CI_LABEL[] = "credRequest";
constexpr int CI_LABEL_LEN = 11;
// product v: 0 = c Nym (variable base), 1.. = fixed-base on the issuer's table CI_BASE[v]
// with the scalar at record word CI_SC[v]
__device__ constexpr int CI_BASE[CI_NPROD] = {-1, B_HSK, B_HRAND, B_HA + 0, B_HA + 1, B_HA + 2, B_HA + 3};
__device__ constexpr int CI_SC[CI_NPROD] = {CI_R_CMUL, CI_R_S,       CI_R_BIGS,     CI_R_ATTR,
                                            CI_R_ATTR + 8, CI_R_ATTR + 16, CI_R_ATTR + 24};
FTS_DEV size_t ci_dp(size_t) { return 0; }
FTS_DEV size_t ci_vr(size_t n) { return (size_t)16 * n; }
FTS_DEV size_t ci_ba(size_t n) { return ci_vr(n) + (size_t)CI_NPROD * 24 * n; }
FTS_DEV size_t ci_iv(size_t n) { return ci_ba(n) + (size_t)16 * n; }
FTS_DEV size_t ci_tv(size_t n) { return ci_iv(n) + (size_t)8 * n; }  // 208 n words: 16-byte aligned rows
constexpr size_t CI_SCRATCH_WORDS = 16 + CI_NPROD * 24 + 16 + 8 + AT_WORDS;

// "credRequest" || t || HSk || Nym || IssuerNonce || ipk.Hash -> HashToZr; hk: ipk.Hash (8
// big-endian words), then HSk as X || Y (16); nonce: 8 big-endian words
template <class CV>
FTS_DEV void ci_challenge(ByteSink& M, const typename CV::F& tx, const typename CV::F& ty, const typename CV::F& nx,
                          const typename CV::F& ny, const uint32_t* __restrict__ hk, const uint32_t* nonce,
                          uint32_t c[8]) {
  for (int k = 0; k < CI_LABEL_LEN; k++) M.put_byte((uint8_t)CI_LABEL[k]);
  CV::encode(M, tx, ty);
  if (CV::G1_BYTES == 65) M.put_byte(0x04);
  for (int k = 0; k < 16; k++) M.put_word(hk[8 + k]);
  CV::encode(M, nx, ny);
  for (int k = 0; k < 8; k++) M.put_word(nonce[k]);
  for (int k = 0; k < 8; k++) M.put_word(hk[k]);
  sink_digest<CV>(M, c);
}

// a, b (Jacobian) -> affine with one inversion; the identity -> (0, 0)
template <class CV>
FTS_DEV void ci_affine2(const typename CV::PJ& a, const typename CV::PJ& b, typename CV::F& ax, typename CV::F& ay,
                        typename CV::F& bx, typename CV::F& by) {
  using B = typename CV::B;
  using F = typename CV::F;
  const bool ia = CV::is_inf(a), ib = CV::is_inf(b);
  const F za = ia ? B::one() : a.z, zb = ib ? B::one() : b.z;
  const F inv = B::inv(B::mul(za, zb));
  const F zai = B::mul(inv, zb), zbi = B::mul(inv, za);
  const F za2 = B::mul(zai, zai), zb2 = B::mul(zbi, zbi);
  ax = ia ? B::zero() : B::mul(a.x, za2);
  ay = ia ? B::zero() : B::mul(B::mul(a.y, za2), zai);
  bx = ib ? B::zero() : B::mul(b.x, zb2);
  by = ib ? B::zero() : B::mul(B::mul(b.y, zb2), zbi);
}

// rec: [n][CIQ_REC_WORDS] sk rSk (canonical limbs) nonce (big-endian words); out <-
// [n][CI_OUT_WORDS]: Nym as X || Y, then c, s, big-endian bytes
template <class CV>
__global__ void __launch_bounds__(256) k_ci_request(int n, const uint32_t* __restrict__ rec,
                                                    const uint32_t* __restrict__ tables,
                                                    const uint32_t* __restrict__ hk, uint8_t* __restrict__ msg,
                                                    uint32_t* __restrict__ out, const int32_t* __restrict__ status) {
  using F = typename CV::F;
  using PJ = typename CV::PJ;
  using Z = Zr<CV>;
  using T = typename Z::Z;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || status[i] != FTS_OK) return;
  const uint32_t* R = rec + (size_t)i * CIQ_REC_WORDS;
  PJ nym = CV::inf(), t = CV::inf();
  CV::fixed_mul_acc(nym, tables, B_HSK, R);
  CV::fixed_mul_acc(t, tables, B_HSK, R + 8);
  F nx, ny, tx, ty;
  ci_affine2<CV>(nym, t, nx, ny, tx, ty);
  ByteSink M{msg, (size_t)n, (size_t)i};
  T c;
  ci_challenge<CV>(M, tx, ty, nx, ny, hk, R + 16, c.v);
  const T s = Z::add(Z::ld(R + 8), Z::mul(Z::to_mont(c), Z::ld(R)));
  uint32_t* O = out + (size_t)i * CI_OUT_WORDS;
  uint32_t pw[16];
  point_be_words<CV>(nx, ny, pw);
#pragma unroll
  for (int k = 0; k < 16; k++) O[k] = __builtin_bswap32(pw[k]);
#pragma unroll
  for (int k = 0; k < 8; k++) O[16 + k] = __builtin_bswap32(c.v[7 - k]), O[24 + k] = __builtin_bswap32(s.v[7 - k]);
}

// pts: [n][64] Nym as X || Y
template <class CV>
__global__ void __launch_bounds__(256) k_ci_decode(int n, const uint8_t* __restrict__ pts,
                                                   uint32_t* __restrict__ scratch, int32_t* __restrict__ status) {
  using F = typename CV::F;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || status[i] != FTS_OK) return;
  const LaneWords DP{scratch + ci_dp(n), (size_t)n, (size_t)i};
  F px, py;
  bool id;
  const bool good = CV::decode(pts + (size_t)i * 64, px, py, id) && !id;
  put_f<CV>(DP, 0, px);
  put_f<CV>(DP, 8, py);
  if (!good) status[i] = FTS_E_CREDREQ_MALFORMED;
}

// lane g = v * n + i, v < nprod (2: the check alone; CI_NPROD: an issue)
template <class CV>
__global__ void __launch_bounds__(256) k_ci_var(int n, int nprod, const uint32_t* __restrict__ rec,
                                                const uint32_t* __restrict__ tables, uint32_t* __restrict__ scratch,
                                                const int32_t* __restrict__ status) {
  using PJ = typename CV::PJ;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (size_t)nprod * n) return;
  const int v = (int)(g / n), i = (int)(g % n);
  if (status[i] != FTS_OK) return;
  const uint32_t* k = rec + (size_t)i * CI_REC_WORDS + CI_SC[v];
  const LaneWords VR{scratch + ci_vr(n) + (size_t)v * 24 * n, (size_t)n, (size_t)i};
  PJ r = CV::inf();
  if (v > 0) {
    CV::fixed_mul_acc(r, tables, CI_BASE[v], k);
  } else {
    const LaneWords DP{scratch + ci_dp(n), (size_t)n, (size_t)i};
    const GTab T{scratch + ci_tv(n), (size_t)n, (size_t)i};
    r = glv_mul<CV>(CV::from_affine(get_f<CV>(DP, 0), get_f<CV>(DP, 8)), k, T);
  }
  put_f<CV>(VR, 0, r.x);
  put_f<CV>(VR, 8, r.y);
  put_f<CV>(VR, 16, r.z);
}

// isk: the issuer's secret, canonical limbs (ISSUE only)
template <class CV, bool ISSUE>
__global__ void __launch_bounds__(256) k_ci_check(int n, const uint32_t* __restrict__ rec,
                                                  const uint32_t* __restrict__ isk, const uint32_t* __restrict__ hk,
                                                  uint32_t* __restrict__ scratch, uint8_t* __restrict__ msg,
                                                  int32_t* __restrict__ status) {
  using B = typename CV::B;
  using F = typename CV::F;
  using PJ = typename CV::PJ;
  using Z = Zr<CV>;
  using T = typename Z::Z;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || status[i] != FTS_OK) return;
  const uint32_t* R = rec + (size_t)i * CI_REC_WORDS;
  const LaneWords DP{scratch + ci_dp(n), (size_t)n, (size_t)i};
  auto product = [&](int v) {
    const LaneWords VR{scratch + ci_vr(n) + (size_t)v * 24 * n, (size_t)n, (size_t)i};
    PJ r;
    r.x = get_f<CV>(VR, 0), r.y = get_f<CV>(VR, 8), r.z = get_f<CV>(VR, 16);
    return r;
  };
  const F nx = get_f<CV>(DP, 0), ny = get_f<CV>(DP, 8);
  // t = HSk s - Nym c
  PJ t = product(0);
  t.y = B::neg(t.y);
  CV::add_to(t, product(1));
  // B = g1 + Nym + HRand S + sum HAttrs[i] attrs[i]; g1 = (1, 2) on both curves
  PJ b = CV::inf();
  if (ISSUE) {
    b = CV::from_affine(B::one(), B::add(B::one(), B::one()));
    CV::madd_to(b, nx, ny);
#pragma unroll 1
    for (int v = 2; v < CI_NPROD; v++) CV::add_to(b, product(v));
  }
  F tx, ty, bx, by;
  ci_affine2<CV>(t, b, tx, ty, bx, by);
  ByteSink M{msg, (size_t)n, (size_t)i};
  uint32_t c[8];
  ci_challenge<CV>(M, tx, ty, nx, ny, hk, R + CI_R_NONCE, c);
  // Zr.Equals on integers: a proof_c >= r (kept unreduced at CI_R_CCMP) never matches
  uint32_t diff = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) diff |= c[k] ^ R[CI_R_CCMP + k];
  if (diff) {
    status[i] = FTS_E_CREDREQ_INVALID;
    return;
  }
  if (ISSUE) {
    const LaneWords BA{scratch + ci_ba(n), (size_t)n, (size_t)i};
    put_f<CV>(BA, 0, bx);
    put_f<CV>(BA, 8, by);
    // (isk + E)^-1: the host redraws an E with isk + E = 0
    const T d = Z::add(Z::ld(isk), Z::ld(R + CI_R_E));
    const T inv = Z::from_mont(Z::inv_m(Z::to_mont(d)));
    const LaneWords IV{scratch + ci_iv(n), (size_t)n, (size_t)i};
#pragma unroll
    for (int k = 0; k < 8; k++) IV.at(k) = inv.v[k];
  }
}

// out <- [n][CI_OUT_WORDS]: A then B as X || Y, big-endian bytes
template <class CV>
__global__ void __launch_bounds__(256) k_ci_sign(int n, uint32_t* __restrict__ scratch, uint32_t* __restrict__ out,
                                                 const int32_t* __restrict__ status) {
  using B = typename CV::B;
  using F = typename CV::F;
  using PJ = typename CV::PJ;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || status[i] != FTS_OK) return;
  const LaneWords BA{scratch + ci_ba(n), (size_t)n, (size_t)i};
  const LaneWords IV{scratch + ci_iv(n), (size_t)n, (size_t)i};
  const GTab T{scratch + ci_tv(n), (size_t)n, (size_t)i};
  const F bx = get_f<CV>(BA, 0), by = get_f<CV>(BA, 8);
  uint32_t inv[8];
#pragma unroll
  for (int k = 0; k < 8; k++) inv[k] = IV.at(k);
  PJ a = CV::inf();
  if (!(B::is_zero(bx) && B::is_zero(by))) a = glv_mul<CV>(CV::from_affine(bx, by), inv, T);
  F ax = B::zero(), ay = B::zero();
  if (!CV::is_inf(a)) {
    const F zi = B::inv(a.z), zi2 = B::mul(zi, zi);
    ax = B::mul(a.x, zi2), ay = B::mul(B::mul(a.y, zi2), zi);
  }
  uint32_t* O = out + (size_t)i * CI_OUT_WORDS;
  uint32_t pw[16];
  point_be_words<CV>(ax, ay, pw);
#pragma unroll
  for (int k = 0; k < 16; k++) O[k] = __builtin_bswap32(pw[k]);
  point_be_words<CV>(bx, by, pw);
#pragma unroll
  for (int k = 0; k < 16; k++) O[16 + k] = __builtin_bswap32(pw[k]);
}

// BarG2 == isk BarG1 at issuer creation, one lane: bar = BarG1 then BarG2 as X || Y;
// ok[0] <- 1 iff both decode, neither is the identity and the equation holds
template <class CV>
__global__ void __launch_bounds__(64) k_ci_key(const uint8_t* __restrict__ bar, const uint32_t* __restrict__ isk,
                                               int32_t* __restrict__ ok) {
  using B = typename CV::B;
  using F = typename CV::F;
  using PJ = typename CV::PJ;
  if (blockIdx.x || threadIdx.x) return;
  F x1, y1, x2, y2;
  bool i1, i2;
  bool good = CV::decode(bar, x1, y1, i1) && !i1;
  good = CV::decode(bar + 64, x2, y2, i2) && !i2 && good;
  PJ acc = CV::inf();
  if (good) {
#pragma unroll 1
    for (int bit = 255; bit >= 0; bit--) {
      acc = CV::dbl(acc);
      if ((isk[bit >> 5] >> (bit & 31)) & 1u) CV::madd_to(acc, x1, y1);
    }
    good = !CV::is_inf(acc);
  }
  if (good) {
    const F z2 = B::mul(acc.z, acc.z), z3 = B::mul(z2, acc.z);
    good = B::eq(B::mul(x2, z2), acc.x) && B::eq(B::mul(y2, z3), acc.y);
  }
  ok[0] = good ? 1 : 0;
}

// ------------------------------------------------- per-curve launch sequences
template <class CV>
void launch_credreq_make(const CredReqChain& c) {
  k_ci_request<CV><<<(unsigned)((c.n + 255) / 256), 256, 0, c.s>>>(c.n, c.rec, c.tables, c.hk, c.msg, c.out, c.st);
}
template <class CV>
hipError_t launch_credissue(const CredReqChain& c, bool issue) {
  const int nprod = issue ? CI_NPROD : 2;
  const unsigned g256 = (unsigned)((c.n + 255) / 256), gvar = (unsigned)(((size_t)nprod * c.n + 255) / 256);
  k_ci_decode<CV><<<g256, 256, 0, c.s>>>(c.n, c.pts, c.scr, c.st);
  k_ci_var<CV><<<gvar, 256, 0, c.s>>>(c.n, nprod, c.rec, c.tables, c.scr, c.st);
  if (!issue) {
    k_ci_check<CV, false><<<g256, 256, 0, c.s>>>(c.n, c.rec, c.isk, c.hk, c.scr, c.msg, c.st);
    return hipSuccess;
  }
  k_ci_check<CV, true><<<g256, 256, 0, c.s>>>(c.n, c.rec, c.isk, c.hk, c.scr, c.msg, c.st);
  const hipError_t e = hipEventRecord(c.ev_mid, c.s);
  k_ci_sign<CV><<<g256, 256, 0, c.s>>>(c.n, c.scr, c.out, c.st);
  return e;
}
template <class CV>
void launch_credissue_key(const uint8_t* bar, const uint32_t* isk, int32_t* ok, hipStream_t s) {
  k_ci_key<CV><<<1, 64, 0, s>>>(bar, isk, ok);
}

}  // namespace idv
