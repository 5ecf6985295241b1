// Idemix issuer keys on the device: IssuerPublicKey.Check and NewIssuerKey (IBM/idemix
// bccsp/schemes/dlog/crypto issuerkey.go; reached in the reference when a key is imported and,
// for a new key, through idemixgen's CA key generation), restated in tests/issuer_key_ref.py.
//
//   check    t1 = g2 s - W c, t2 = BarG1 s - BarG2 c,
//            accept iff c == HashToZr(t1 || t2 || g2 || BarG1 || W || BarG2), as integers
//   keygen   HSk, HRand, HAttrs[0..3], BarG1 = their draws times g1, W = g2 isk,
//            BarG2 = BarG1 isk, t1 = g2 r, t2 = BarG1 r, c as above, s = r + c isk
// G1 points are hashed as G1.Bytes(); G2 points as their four 32-byte coordinates in the
// ECP2 proto's field order (BN254: X.A1 X.A0 Y.A1 Y.A0, gnark's raw bytes; FP256BN: xa xb ya
// yb).  PINNED: the reference's four issuer keys (tests/golden/idemix) verify under this
// reading on both curves and under no other coordinate order.
//
// The new arithmetic is g2_lincomb: a P + b Q on the twist E'(Fp2) over the Jacobian
// doubling and the complete mixed addition of idv_kernels.hpp (g2j_dbl, g2j_madd: a = 0, so
// the D-type and the M-type twist share them; b' enters only the on-twist check of
// decode_g2).  One rolled 256-step loop with one copy of the doubling and one of the complete
// addition, which the two points share and which holds a second doubling for its P == Q
// branch; no table.  The conversion to affine inverts in Fp, out of line on FP256BN
// (p256::inv) as everywhere else.
//
// Kernels, per curve (idemix_ipk_<cv>.hip), one lane per key, never launched in bulk:
//   k_ipk_decode   the key's G1 points (HSk, HRand, every HAttrs), BarG1, BarG2 and W decoded
//                  under the handles' rules (W on the twist and not the identity; BN254: in the
//                  subgroup); FTS_E_IPK_MALFORMED / FTS_E_IPK_UNDEFINED; W out, affine Montgomery
//   k_g2_lincomb   lane per product: a g2 + b Q (Q optional) -> four coordinates, proto order
//   k_ipk_t2       t2 = BarG1 s + BarG2 (-c) by one interleaved G1 chain, to affine
//   k_ipk_points   keygen, lane per (point, key): the nine multiples of g1 (HSk HRand HAttrs
//                  BarG1, BarG2 = g1 (d isk), t2 = g1 (d r)), each to affine
//   k_ipk_finish   the 576- / 579-byte transcript and its ten compressions; the check's verdict
//                  (FTS_E_IPK_PROOF) or the generator's c and s
// Every kernel has __launch_bounds__(64): the Fp2 working set of the G2 chain (accumulator 48
// words, two points 64, temporaries) wants the whole register file.  Registers and scratch
// per lane: DESIGN.md 5.6.4.
// Not hardened against timing side channels (branches depend on the secret scalars).
#pragma once
#include "idgen_kernels.hpp"  // point_be_words; idv_kernels.hpp: decode_g2, g2j_dbl, g2j_madd

namespace idv {

// a P + b Q on the twist; P, Q affine Montgomery and not the identity, a, b canonical limbs
// (Q is never touched where b = 0)
template <class B>
FTS_DEV G2J<B> g2_lincomb(const pair::F2<B>& px, const pair::F2<B>& py, const uint32_t a[8], const pair::F2<B>& qx,
                          const pair::F2<B>& qy, const uint32_t b[8]) {
  using namespace pair;
  G2J<B> acc{f2_zero<B>(), f2_one<B>(), f2_zero<B>()};
#pragma unroll 1
  for (int bit = 255; bit >= 0; bit--) {
    g2j_dbl(acc);
    const uint32_t sel = ((a[bit >> 5] >> (bit & 31)) & 1u) | (((b[bit >> 5] >> (bit & 31)) & 1u) << 1);
#pragma unroll 1
    for (int q = 0; q < 2; q++)
      if ((sel >> q) & 1u) g2j_madd(acc, q ? qx : px, q ? qy : py);
  }
  return acc;
}

// Jacobian twist point -> four coordinates, big-endian words in the ECP2 proto's order; the
// identity as the curves' libraries write it (gnark: zeros; AMCL: x = 0, y = 1)
template <class CV>
FTS_DEV void g2_be_words(const G2J<typename CV::B>& p, uint32_t pw[32]) {
  using namespace pair;
  using B = typename CV::B;
  using F = typename CV::F;
  constexpr bool bn = std::is_same<CV, BnCurve>::value;
  F c[4] = {B::zero(), B::zero(), B::zero(), B::zero()};
  const bool inf = is_zero(p.z);
  if (!inf) {
    const F2<B> zi = inv(p.z), zi2 = sqr(zi);
    const F2<B> x = mul(p.x, zi2), y = mul(mul(p.y, zi2), zi);
    if (bn) c[0] = x.b, c[1] = x.a, c[2] = y.b, c[3] = y.a;
    else c[0] = x.a, c[1] = x.b, c[2] = y.a, c[3] = y.b;
  }
  if constexpr (bn) {
    g1_mont_to_be_words(c[0], c[1], pw);
    g1_mont_to_be_words(c[2], c[3], pw + 16);
  } else {
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const F v = p256::from_mont(c[q]);
#pragma unroll
      for (int k = 0; k < 8; k++) pw[8 * q + k] = v.v[7 - k];
    }
    if (inf) pw[23] = 1u;
  }
}

// rec: [n][IPK_REC_WORDS]; g1: the keys' HSk, HRand, HAttrs as X || Y, key i's at
// rec[IPK_R_OFF] .. + rec[IPK_R_CNT]; bar: [n][128] BarG1 then BarG2; wraw: [n][128];
// wdec <- [n][32] W affine Montgomery (x.a x.b y.a y.b)
template <class CV>
__global__ void __launch_bounds__(64) k_ipk_decode(int n, const uint32_t* __restrict__ rec,
                                                   const uint8_t* __restrict__ g1, const uint8_t* __restrict__ bar,
                                                   const uint8_t* __restrict__ wraw, uint32_t* __restrict__ wdec,
                                                   int32_t* __restrict__ status) {
  using B = typename CV::B;
  using F = typename CV::F;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || status[i] != FTS_OK) return;
  const uint32_t* R = rec + (size_t)i * IPK_REC_WORDS;
  F x, y;
  bool id, good = true;
  const uint32_t off = R[IPK_R_OFF], cnt = R[IPK_R_CNT];
#pragma unroll 1
  for (uint32_t k = 0; k < cnt; k++) good = CV::decode(g1 + (size_t)(off + k) * 64, x, y, id) && !id && good;
  const uint8_t* bg = bar + (size_t)i * 128;
  // BarG1.IsInfinity(): gnark's identity is 64 zero bytes (CV::decode says so); AMCL holds it
  // as x = 0, y = 1, which is not on the curve
  bool bar_id = false;
  if (CV::G1_BYTES == 65) {
    uint32_t acc = 0;
    for (int k = 0; k < 64; k++) acc |= k == 63 ? (uint32_t)(bg[k] ^ 1u) : (uint32_t)bg[k];
    bar_id = acc == 0;
  }
  if (good && !bar_id) {
    good = CV::decode(bg, x, y, id);
    bar_id = good && id;
  }
  if (!good) {
    status[i] = FTS_E_IPK_MALFORMED;
    return;
  }
  if (bar_id) {
    status[i] = FTS_E_IPK_UNDEFINED;
    return;
  }
  good = CV::decode(bg + 64, x, y, id);
  pair::F2<B> wx = pair::f2_zero<B>(), wy = pair::f2_zero<B>();
  good = good && decode_g2<CV>(wraw + (size_t)i * 128, wx, wy) && !(pair::is_zero(wx) && pair::is_zero(wy));
  if constexpr (std::is_same<CV, BnCurve>::value) good = good && g2_in_subgroup_bn(wx, wy);
  if (!good) {
    status[i] = FTS_E_IPK_MALFORMED;
    return;
  }
  uint32_t* W = wdec + (size_t)i * 32;
  pair::store_f2(W, wx);
  pair::store_f2(W + 16, wy);
}

// lane g = v * n + i, v < nv: out[v][i] <- sc_i[a_off + v * a_step] g2 + sc_i[b_off] Q_i as 128
// bytes; sc: [n][sc_stride] canonical limbs; q (nullptr: no second term): [n][32] as k_ipk_decode
// writes them
template <class CV>
__global__ void __launch_bounds__(64) k_g2_lincomb(int n, int nv, const uint32_t* __restrict__ q,
                                                   const uint32_t* __restrict__ sc, int sc_stride, int a_off,
                                                   int a_step, int b_off, uint32_t* __restrict__ out,
                                                   const int32_t* __restrict__ status) {
  using B = typename CV::B;
  using K = typename B::K;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (size_t)nv * n) return;
  const int v = (int)(g / n), i = (int)(g % n);
  if (status[i] != FTS_OK) return;
  const uint32_t* S = sc + (size_t)i * sc_stride;
  uint32_t a[8], b[8];
#pragma unroll
  for (int k = 0; k < 8; k++) a[k] = S[a_off + v * a_step + k], b[k] = q ? S[b_off + k] : 0u;
  const pair::F2<B> px = pair::f2_ld<B>(K::GEN2[0]), py = pair::f2_ld<B>(K::GEN2[1]);
  pair::F2<B> qx = px, qy = py;
  if (q) qx = pair::load_f2<B>(q + (size_t)i * 32), qy = pair::load_f2<B>(q + (size_t)i * 32 + 16);
  const G2J<B> r = g2_lincomb<B>(px, py, a, qx, qy, b);
  uint32_t pw[32];
  g2_be_words<CV>(r, pw);
  uint32_t* O = out + g * 32;
#pragma unroll
  for (int k = 0; k < 32; k++) O[k] = __builtin_bswap32(pw[k]);
}

// t2out <- [n][16 words] BarG1 s + BarG2 (-c) as X || Y bytes (the identity as point_be_words
// writes it); s and -c mod r at rec words IPK_R_A, IPK_R_B
template <class CV>
__global__ void __launch_bounds__(64) k_ipk_t2(int n, const uint32_t* __restrict__ rec,
                                               const uint8_t* __restrict__ bar, uint32_t* __restrict__ t2out,
                                               const int32_t* __restrict__ status) {
  using B = typename CV::B;
  using F = typename CV::F;
  using PJ = typename CV::PJ;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || status[i] != FTS_OK) return;
  const uint32_t* R = rec + (size_t)i * IPK_REC_WORDS;
  F x1, y1, x2, y2;
  bool i1, i2;
  (void)CV::decode(bar + (size_t)i * 128, x1, y1, i1);  // decoded once already: k_ipk_decode
  (void)CV::decode(bar + (size_t)i * 128 + 64, x2, y2, i2);
  PJ acc = CV::inf();
#pragma unroll 1
  for (int bit = 255; bit >= 0; bit--) {
    acc = CV::dbl(acc);
    const uint32_t sel = ((R[IPK_R_A + (bit >> 5)] >> (bit & 31)) & 1u) |
                         (i2 ? 0u : ((R[IPK_R_B + (bit >> 5)] >> (bit & 31)) & 1u) << 1);
#pragma unroll 1
    for (int q = 0; q < 2; q++)
      if ((sel >> q) & 1u) CV::madd_to(acc, q ? x2 : x1, q ? y2 : y1);
  }
  F ax = B::zero(), ay = B::zero();
  if (!CV::is_inf(acc)) {
    const F zi = B::inv(acc.z), zi2 = B::mul(zi, zi);
    ax = B::mul(acc.x, zi2), ay = B::mul(B::mul(acc.y, zi2), zi);
  }
  uint32_t pw[16];
  point_be_words<CV>(ax, ay, pw);
  uint32_t* O = t2out + (size_t)i * 16;
#pragma unroll
  for (int k = 0; k < 16; k++) O[k] = __builtin_bswap32(pw[k]);
}

// keygen: lane g = v * n + i, v < IPK_NPT: pts[i][v] <- (the scalar of point v) g1 as X || Y
// bytes.  draws: [n][IPK_ND][8]; v < 7: draw 1 + v (HSk HRand HAttrs[0..3] BarG1); 7: BarG2 =
// g1 (dBar isk); 8: t2 = g1 (dBar r)
template <class CV>
__global__ void __launch_bounds__(64) k_ipk_points(int n, const uint32_t* __restrict__ draws,
                                                   uint32_t* __restrict__ pts) {
  using B = typename CV::B;
  using F = typename CV::F;
  using PJ = typename CV::PJ;
  using Z = Zr<CV>;
  using T = typename Z::Z;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (size_t)IPK_NPT * n) return;
  const int v = (int)(g / n), i = (int)(g % n);
  const uint32_t* D = draws + (size_t)i * IPK_ND * 8;
  T k = Z::ld(D + 8 * (v < 7 ? 1 + v : IPK_D_BAR));
  if (v >= 7) k = Z::mul(Z::to_mont(k), Z::ld(D + 8 * (v == 7 ? IPK_D_ISK : IPK_D_R)));
  const F gx = B::one(), gy = B::add(B::one(), B::one());  // g1 = (1, 2) on both curves
  PJ acc = CV::inf();
#pragma unroll 1
  for (int bit = 255; bit >= 0; bit--) {
    acc = CV::dbl(acc);
    if ((k.v[bit >> 5] >> (bit & 31)) & 1u) CV::madd_to(acc, gx, gy);
  }
  F ax = B::zero(), ay = B::zero();
  if (!CV::is_inf(acc)) {
    const F zi = B::inv(acc.z), zi2 = B::mul(zi, zi);
    ax = B::mul(acc.x, zi2), ay = B::mul(B::mul(acc.y, zi2), zi);
  }
  uint32_t pw[16];
  point_be_words<CV>(ax, ay, pw);
  uint32_t* O = pts + ((size_t)i * IPK_NPT + v) * 16;
#pragma unroll
  for (int k2 = 0; k2 < 16; k2++) O[k2] = __builtin_bswap32(pw[k2]);
}

// t1 || t2 || g2 || BarG1 || W || BarG2 -> HashToZr.  Every argument is the point's bytes as
// written on the wire (G1: X || Y after the curve's prefix)
template <class CV>
FTS_DEV void ipk_challenge(ByteSink& M, const uint8_t* t1, const uint8_t* t2, const uint8_t* g2, const uint8_t* bar1,
                           const uint8_t* w, const uint8_t* bar2, uint32_t c[8]) {
  const uint8_t* part[6] = {t1, t2, g2, bar1, w, bar2};
#pragma unroll 1
  for (int q = 0; q < 6; q++) {
    const int len = (q & 1) ? 64 : 128;
    if ((q & 1) && CV::G1_BYTES == 65) M.put_byte(0x04);
    for (int k = 0; k < len; k++) M.put_byte(part[q][k]);
  }
  sink_digest<CV>(M, c);
}

// GEN = false, the check: t1 [n][128], t2 [n][64], bar [n][128], w [n][128]; rec's IPK_R_CCMP is
// ProofC as sent (>= r: never equal); status <- FTS_E_IPK_PROOF.
// GEN = true: t1 is the second plane of k_g2_lincomb's output ([2][n][128]: W, t1), pts the
// nine points of k_ipk_points (bar = its points 6 and 7, t2 = point 8), rec the draws;
// out <- [n][16 words] c then s, big-endian bytes
template <class CV, bool GEN>
__global__ void __launch_bounds__(64) k_ipk_finish(int n, const uint32_t* __restrict__ rec,
                                                   const uint8_t* __restrict__ t1, const uint8_t* __restrict__ t2,
                                                   const uint8_t* __restrict__ bar, const uint8_t* __restrict__ w,
                                                   const uint8_t* __restrict__ g2, uint8_t* __restrict__ msg,
                                                   uint32_t* __restrict__ out, int32_t* __restrict__ status) {
  using Z = Zr<CV>;
  using T = typename Z::Z;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || status[i] != FTS_OK) return;
  ByteSink M{msg, (size_t)n, (size_t)i};
  T c;
  if (GEN) {
    const uint8_t* P = t2 + (size_t)i * IPK_NPT * 64;  // t2 = pts
    ipk_challenge<CV>(M, t1 + (size_t)i * 128, P + 8 * 64, g2, P + 6 * 64, w + (size_t)i * 128, P + 7 * 64, c.v);
    const uint32_t* D = rec + (size_t)i * IPK_ND * 8;
    const T s = Z::add(Z::ld(D + 8 * IPK_D_R), Z::mul(Z::to_mont(c), Z::ld(D + 8 * IPK_D_ISK)));
    uint32_t* O = out + (size_t)i * 16;
#pragma unroll
    for (int k = 0; k < 8; k++) O[k] = __builtin_bswap32(c.v[7 - k]), O[8 + k] = __builtin_bswap32(s.v[7 - k]);
  } else {
    const uint8_t* bg = bar + (size_t)i * 128;
    ipk_challenge<CV>(M, t1 + (size_t)i * 128, t2 + (size_t)i * 64, g2, bg, w + (size_t)i * 128, bg + 64, c.v);
    const uint32_t* R = rec + (size_t)i * IPK_REC_WORDS;
    uint32_t diff = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) diff |= c.v[k] ^ R[IPK_R_CCMP + k];
    if (diff) status[i] = FTS_E_IPK_PROOF;
  }
}

// ------------------------------------------------- per-curve launch sequences
template <class CV>
void launch_ipk_check(const IpkChain& c) {
  const unsigned g64 = (unsigned)((c.n + 63) / 64);
  k_ipk_decode<CV><<<g64, 64, 0, c.s>>>(c.n, c.rec, c.g1, c.bar, c.w, c.wdec, c.st);
  k_g2_lincomb<CV><<<g64, 64, 0, c.s>>>(c.n, 1, c.wdec, c.rec, IPK_REC_WORDS, IPK_R_A, 0, IPK_R_B, c.t1, c.st);
  k_ipk_t2<CV><<<g64, 64, 0, c.s>>>(c.n, c.rec, c.bar, c.t2, c.st);
  k_ipk_finish<CV, false><<<g64, 64, 0, c.s>>>(c.n, c.rec, reinterpret_cast<const uint8_t*>(c.t1),
                                               reinterpret_cast<const uint8_t*>(c.t2), c.bar, c.w, c.g2, c.msg, nullptr,
                                               c.st);
}
// c.rec: the draws; c.t1 <- [2][n][128] W then t1; c.t2 <- the nine points; c.out <- c, s
template <class CV>
void launch_ipk_keygen(const IpkChain& c) {
  const unsigned g64 = (unsigned)((c.n + 63) / 64);
  k_g2_lincomb<CV><<<(unsigned)((2 * (size_t)c.n + 63) / 64), 64, 0, c.s>>>(c.n, 2, nullptr, c.rec, IPK_ND * 8,
                                                                           8 * IPK_D_ISK, 8 * (IPK_D_R - IPK_D_ISK), 0,
                                                                           c.t1, c.st);
  k_ipk_points<CV><<<(unsigned)(((size_t)IPK_NPT * c.n + 63) / 64), 64, 0, c.s>>>(c.n, c.rec, c.t2);
  const uint8_t* wt = reinterpret_cast<const uint8_t*>(c.t1);
  k_ipk_finish<CV, true><<<g64, 64, 0, c.s>>>(c.n, c.rec, wt + (size_t)c.n * 128,
                                              reinterpret_cast<const uint8_t*>(c.t2), nullptr, wt, c.g2, c.msg, c.out,
                                              c.st);
}

}  // namespace idv
