// Idemix pseudonym signatures, verified and made on the device, one signature per
// lane, one template each over the curve traits (idemix_curves.hpp); idemix_kernels.hip
// instantiates k_nym_sign for both curves and k_nym_verify for FP256BN (BN254 verification
// keeps its earlier text there: as k_nym_verify<BnCurve> it measured 0.85 % slower).
//
// Verification (IBM/idemix NymSignature.Ver, reached from
// services/identity/idemix/crypto/id.go:145-161 NymSignatureVerifier.Verify):
//       t  = HSk^s_sk * HRand^s_rnym * Nym^-c
//       c' = HashToZr("sign" || t || Nym || ipk.Hash || msg)
//       ok = (c == HashToZr(c' || Nonce))
// Signing (IBM/idemix NewNymSignature): t = HSk^r_sk * HRand^r_r, the same two hashes,
// s_sk = r_sk + c sk and s_r = r_r + c rnym mod r; the nonces are drawn on the host.
//
// Both kernels are nym_challenge (decode Nym, the two fixed-base products from the
// issuer's 16-bit tables, verification's (r - c) Nym by GLV over the lane's table in
// global memory, t affine, the hashed stream, the second hash) and a few lines after it.
// What differs by curve is in NymOps<CV>: how the fixed-base products accumulate, the
// variable-base product, t's bytes and the stream's prefix.  The message (BN254) or
// the whole stream with t left zero (FP256BN, materialised by the host:
// host/idemix_parse.hpp pack_nym_item) is read from HBM as aligned words through
// padded_word (idemix_hash.hpp).
#pragma once
#include "idemix_curves.hpp"
#include "idemix_hash.hpp"
#include "fbn_glv.hpp"
#include "../host/idemix_parse.hpp"  // NREC, NSREC, NSOUT: the per-item records

namespace idv {

template <class CV>
struct NymOps;

// BN254: G1.Bytes() = X || Y, so the 164-byte prefix "sign" t Nym ipk.Hash is whole
// words and comes from registers; the staged buffer is the message alone
template <>
struct NymOps<BnCurve> {
  using RMod = FrP;
  static constexpr uint32_t PRE = 164, PRE_BLOCKS = 3;
  static FTS_DEV Scalar scalar(const uint32_t* p) {  // canonical plain limbs (LE)
    Scalar s;
#pragma unroll
    for (int k = 0; k < 8; k++) s.v[k] = p[k];
    return s;
  }
  // acc += k[0..8) HSk + k[8..16) HRand: 2 x 16 mixed additions
  static FTS_DEV void fixed2(G1J& acc, const uint32_t* tables, const uint32_t* k) {
    fb_mul_acc(acc, tables, scalar(k));
    fb_mul_acc(acc, tables + FB_WORDS_PER_BASE, scalar(k + 8));
  }
  static FTS_DEV G1J var_mul(const Fp& x, const Fp& y, const uint32_t e[8], uint32_t* __restrict__ vtab, size_t stride,
                             size_t li) {
    G1A p;
    p.x = x, p.y = y;
    return glv_mul(p, scalar(e), vtab, stride, li);
  }
  static FTS_DEV void t_words(const G1J& acc, uint32_t tw[16]) {
    const G1A t = g1j_to_affine(acc);  // identity -> (0, 0) -> 64 zero bytes (gnark RawBytes)
    g1_mont_to_be_words(t.x, t.y, tw);
  }
  static FTS_DEV void absorb_prefix(uint32_t st[8], uint32_t w[16], const uint32_t tw[16], const uint8_t* nym_raw,
                                    const uint32_t* __restrict__ ipk_hash, const uint32_t* __restrict__ m,
                                    uint32_t len, uint32_t nb) {
    uint32_t nw[16];
    load_be_words(nym_raw, nw);
    // block 0: "sign" t[0..14]
    w[0] = 0x7369676eu;
#pragma unroll
    for (int k = 1; k < 16; k++) w[k] = tw[k - 1];
    sha256_compress(st, w);
    // block 1: t[15] Nym[0..14]
    w[0] = tw[15];
#pragma unroll
    for (int k = 1; k < 16; k++) w[k] = nw[k - 1];
    sha256_compress(st, w);
    // block 2: Nym[15] ipk.Hash[0..7] then the message
    w[0] = nw[15];
#pragma unroll
    for (int k = 1; k < 9; k++) w[k] = ipk_hash[k - 1];
#pragma unroll
    for (int k = 9; k < 16; k++) w[k] = padded_word(m, PRE, len, nb, 32 + k);
    sha256_compress(st, w);
  }
};

// FP256BN: ECP.ToBytes = 0x04 || X || Y puts everything after "sign" off the word
// grid, so the host materialises the whole stream and the kernel lays t's words, one
// byte on, over the first two blocks
template <>
struct NymOps<FbnCurve> {
  using RMod = fbn::RM;
  static constexpr uint32_t PRE = 0, PRE_BLOCKS = 2;
  static FTS_DEV void fixed2(fbn::PJ& acc, const uint32_t* tables, const uint32_t* k) {
#pragma unroll 1
    for (int q = 0; q < 2; q++) FbnCurve::fixed_mul_acc(acc, tables, q, k + 8 * q);
  }
  static FTS_DEV fbn::PJ var_mul(const fbn::Fp& x, const fbn::Fp& y, const uint32_t e[8], uint32_t* __restrict__ vtab,
                                 size_t stride, size_t li) {
    return fbn::glv_mul_tab(x, y, e, vtab, stride, li);
  }
  static FTS_DEV void t_words(const fbn::PJ& X, uint32_t tw[16]) {
    fbn::Fp ax{}, ay{};
    ay.v[0] = 1u;  // t = O (zero nonces): AMCL ToBytes of infinity = 0x04 || 0 || 1
    if (!fbn::is_zero(X.z)) {
      const fbn::Fp zi = p256::inv(X.z), zi2 = fbn::sqr(zi);
      ax = p256::from_mont(fbn::mul(X.x, zi2)), ay = p256::from_mont(fbn::mul(X.y, fbn::mul(zi2, zi)));
    }
#pragma unroll
    for (int k = 0; k < 8; k++) tw[k] = ax.v[7 - k], tw[8 + k] = ay.v[7 - k];
  }
  static FTS_DEV void absorb_prefix(uint32_t st[8], uint32_t w[16], const uint32_t tw[16], const uint8_t*,
                                    const uint32_t* __restrict__, const uint32_t* __restrict__ m, uint32_t len,
                                    uint32_t nb) {
    // block 0: "sign" 0x04 t[0..58]
    w[0] = 0x7369676eu;
    w[1] = 0x04000000u | (tw[0] >> 8);
#pragma unroll
    for (int k = 2; k < 16; k++) w[k] = (tw[k - 2] << 24) | (tw[k - 1] >> 8);
    sha256_compress(st, w);
    // block 1: t[59..63] then the host's bytes (Nym, ipk.Hash, message)
    w[0] = (tw[14] << 24) | (tw[15] >> 8);
    w[1] = (tw[15] << 24) | (padded_word(m, PRE, len, nb, 17) & 0x00ffffffu);
#pragma unroll
    for (int k = 2; k < 16; k++) w[k] = padded_word(m, PRE, len, nb, 16 + k);
    sha256_compress(st, w);
  }
};

// c <- HashToZr(HashToZr("sign" || t || Nym || ipk.Hash || msg) || nonce) of item i with
// t = fk[0..8) HSk + fk[8..16) HRand (+ (r - sig_c) Nym: VERIFY); false: Nym is not a
// point of the curve.  nym_raw: the item's X || Y; mlen[i]: the staged bytes (BN254 the
// message, FP256BN the stream); vtab: the GLV lane table, [entry][word][stride]
template <class CV, bool VERIFY>
FTS_DEV bool nym_challenge(int i, const uint8_t* nym_raw, const uint32_t* fk, const uint32_t* sig_c,
                           const uint32_t* nonce, const uint32_t* __restrict__ msgw,
                           const uint64_t* __restrict__ moff, const uint32_t* __restrict__ mlen,
                           const uint32_t* __restrict__ tables, const uint32_t* __restrict__ ipk_hash,
                           uint32_t* __restrict__ vtab, size_t stride, size_t li, uint32_t c[8]) {
  using Ops = NymOps<CV>;
  // Nym: NewG1FromBytes (canonical coordinates, on the curve)
  typename CV::F nx, ny;
  bool ident;
  if (!CV::decode(nym_raw, nx, ny, ident)) return false;
  typename CV::PJ acc = CV::inf();
  Ops::fixed2(acc, tables, fk);
  if constexpr (VERIFY) {
    uint32_t e[8];  // r - c (c < r; c == 0 -> 0)
    uint32_t bw = 0, nz = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) nz |= sig_c[k];
#pragma unroll
    for (int k = 0; k < 8; k++) e[k] = nz ? subb(Ops::RMod::M[k], sig_c[k], bw, bw) : 0u;
    CV::add_to(acc, Ops::var_mul(nx, ny, e, vtab, stride, li));
  }
  uint32_t tw[16];
  Ops::t_words(acc, tw);
  const uint32_t* m = msgw + moff[i];
  const uint32_t len = mlen[i];
  const uint32_t nb = padded_blocks(Ops::PRE + len);  // >= 3
  uint32_t st[8], w[16];
  sha256_init(st);
  Ops::absorb_prefix(st, w, tw, nym_raw, ipk_hash, m, len, nb);
  for (uint32_t blk = Ops::PRE_BLOCKS; blk < nb; blk++) {
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = padded_word(m, Ops::PRE, len, nb, 16 * blk + k);
    sha256_compress(st, w);
  }
  uint32_t c1[8];
  CV::digest_mod_r(st, c1);
  nonce_challenge<CV>(c1, nonce, c);
  return true;
}

// rec: NREC words per item (c, s_sk, s_rnym as plain LE limbs, the nonce as big-endian
// words).  One launch per tile of `tile` items starting at `base`: the GLV lane tables
// are bounded device memory whatever n is
template <class CV>
__global__ __launch_bounds__(256) void k_nym_verify(int n, const uint32_t* __restrict__ rec,
                                                    const uint8_t* __restrict__ nym_raw,
                                                    const uint32_t* __restrict__ msgw,
                                                    const uint64_t* __restrict__ moff,  // word offsets
                                                    const uint32_t* __restrict__ mlen,
                                                    const uint32_t* __restrict__ tables,
                                                    const uint32_t* __restrict__ ipk_hash,  // 8 BE words
                                                    uint32_t* __restrict__ vtab, int32_t* __restrict__ status,
                                                    int base, int tile) {
  const int li = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = base + li;
  if (li >= tile || i >= n || status[i] != FTS_OK) return;
  const uint32_t* R = rec + (size_t)i * NREC;
  uint32_t c[8];
  if (!nym_challenge<CV, true>(i, nym_raw + (size_t)i * 64, R + 8, R, R + 24, msgw, moff, mlen, tables, ipk_hash,
                               vtab, (size_t)tile, (size_t)li, c)) {
    status[i] = FTS_E_NYM_BADKEY;
    return;
  }
  uint32_t diff = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) diff |= c[k] ^ R[k];
  status[i] = diff ? FTS_E_NYM_INVALID : FTS_OK;
}

// srec: NSREC words per item (sk, rnym, r_sk, r_r as canonical LE limbs, the nonce as
// big-endian words); out <- c, s_sk, s_r (canonical LE limbs).  Nym is decoded only to
// give a bad key the verifier's verdict.
template <class CV>
__global__ __launch_bounds__(256) void k_nym_sign(int n, const uint32_t* __restrict__ srec,
                                                  const uint8_t* __restrict__ nym_raw,
                                                  const uint32_t* __restrict__ msgw,
                                                  const uint64_t* __restrict__ moff,  // word offsets
                                                  const uint32_t* __restrict__ mlen,
                                                  const uint32_t* __restrict__ tables,
                                                  const uint32_t* __restrict__ ipk_hash,  // 8 BE words
                                                  int32_t* __restrict__ status, uint32_t* __restrict__ out) {
  using Z = Zr<CV>;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || status[i] != FTS_OK) return;
  const uint32_t* S = srec + (size_t)i * NSREC;
  typename Z::Z c;
  if (!nym_challenge<CV, false>(i, nym_raw + (size_t)i * 64, S + 16, nullptr, S + 32, msgw, moff, mlen, tables,
                                ipk_hash, nullptr, 0, 0, c.v)) {
    status[i] = FTS_E_NYM_BADKEY;
    return;
  }
  // s = r + c * secret mod r: a Montgomery-form factor times a plain one is plain
  const typename Z::Z cm = Z::to_mont(c);
  const typename Z::Z s_sk = Z::add(Z::mul(cm, Z::ld(S)), Z::ld(S + 16));
  const typename Z::Z s_r = Z::add(Z::mul(cm, Z::ld(S + 8)), Z::ld(S + 24));
  uint32_t* O = out + (size_t)i * NSOUT;
#pragma unroll
  for (int k = 0; k < 8; k++) O[k] = c.v[k], O[8 + k] = s_sk.v[k], O[16 + k] = s_r.v[k];
}

}  // namespace idv
