// Batched idemix pseudonym-signature verification over BN254 and FP256BN (SURVEY.md
// §8(f) row 4, the idemix half): the owner signatures of transfers whose
// input tokens are owned by idemix identities.
//
// Reference call chain:
//   validator/validator_transfer.go:29-62  TransferSignatureValidate, per input
//   services/identity/idemix/deserializer.go:82-105  owner verifier =
//       crypto.NymSignatureVerifier{IPK, NymPK}
//   services/identity/idemix/crypto/id.go:145-161  NymSignatureVerifier.Verify
//       -> bccsp Verify(NymPK, sigma, msg, IdemixNymSignerOpts{IssuerPK})
//   github.com/IBM/idemix (go.mod:6, not vendored) NymSignature.Ver:
//       t  = HSk^s_sk * HRand^s_rnym * Nym^-c
//       c' = HashToZr("sign" || t || Nym || ipk.Hash || msg)
//       ok = (c == HashToZr(c' || Nonce))
// (restated and pinned as far as the reference's fixtures allow in
// oracle/idemix.py).  The issuer key is the BN254 one that zkatdlog public
// parameters carry (IdemixIssuerPublicKeys, curve BN254 in zkatdlog_pp.json).
//
// Kernels (one signature per lane):
//   (build once per issuer key)  16-bit fixed-base tables of HSk and HRand
//       (rp_tables.hip launch_build_tables, 32 MiB each)
//   k_nym_verify  nym decode + on-curve check, t = s_sk HSk + s_rnym HRand
//       (2 x 16 mixed additions) + (r - c) Nym (GLV, glv.hpp), affine t,
//       SHA-256 over the 164-byte prefix and the message (streamed from HBM
//       as aligned words), HashToZr, the second 64-byte hash, c == c''.
//
// Signing (IBM/idemix NewNymSignature, reached from services/identity/idemix/crypto/id.go):
//   k_nym_sign / k_nym_sign_fbn  t = r_sk HSk + r_r HRand (2 x 16 mixed additions from
//       the same tables, no variable-base product), affine t, the verify kernels' hashed
//       stream (restated, so that their code is untouched), c, s_sk = r_sk + c sk and
//       s_r = r_r + c rnym mod r.  The nonces are drawn on the host.
// The host side (handle, parser, staging) is api_idemix.cpp over host/idemix_parse.hpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/fts_gpu.h"
#include "common/sha256.hpp"
#include "device/fixed_base.hpp"
#include "device/glv.hpp"
#include "device/helpers.hpp"
#include "device/transcript.hpp"
#include "device/fp256bn.hpp"
#include "device/launch.hpp"
#include "host/idemix_parse.hpp"  // NREC: the per-item record

using namespace fts;
using idv::NREC;
using idv::NSREC;
using idv::NSOUT;

namespace {

constexpr uint32_t PREFIX_WORDS = 41;  // "sign"(1) + t(16) + Nym(16) + ipk.Hash(8)

// message word j of the hashed stream (big-endian), with the SHA-256 0x80
// terminator and zero fill; m: the message's words (4-byte aligned, padded
// to a whole word in the staging buffer)
FTS_DEV uint32_t msg_word(const uint32_t* __restrict__ m, uint32_t len, uint32_t j) {
  const uint32_t b = 4 * j;
  if (b > len) return 0u;
  if (b == len) return 0x80000000u;
  const uint32_t raw = __builtin_bswap32(m[j]);
  if (b + 4 <= len) return raw;
  const uint32_t keep = len - b;  // 1..3 bytes
  const uint32_t mask = 0xffffffffu << (32 - 8 * keep);
  return (raw & mask) | (0x80000000u >> (8 * keep));
}

// word g >= PREFIX_WORDS of the padded stream of nb blocks (length in the last two)
FTS_DEV uint32_t stream_word(const uint32_t* __restrict__ m, uint32_t len, uint32_t nb, uint32_t g) {
  const uint64_t bits = (uint64_t)(164u + len) * 8u;
  if (g == 16 * nb - 2) return (uint32_t)(bits >> 32);
  if (g == 16 * nb - 1) return (uint32_t)bits;
  return msg_word(m, len, g - PREFIX_WORDS);
}

// canonical plain limbs (LE) -> Scalar
FTS_DEV Scalar load_scalar(const uint32_t* p) {
  Scalar s;
#pragma unroll
  for (int k = 0; k < 8; k++) s.v[k] = p[k];
  return s;
}

__global__ __launch_bounds__(256) void k_nym_verify(int n, const uint32_t* __restrict__ rec,
                                                    const uint8_t* __restrict__ nym_raw,
                                                    const uint32_t* __restrict__ msgw,
                                                    const uint64_t* __restrict__ moff,  // word offsets
                                                    const uint32_t* __restrict__ mlen,
                                                    const uint32_t* __restrict__ tables,
                                                    const uint32_t* __restrict__ ipk_hash,  // 8 BE words
                                                    uint32_t* __restrict__ vtab, int32_t* __restrict__ status,
                                                    int base, int tile) {
  // one launch per tile of `tile` items starting at `base`; the GLV lane table is
  // [entry][word][tile] (bounded device memory whatever n is)
  const int li = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = base + li;
  if (li >= tile || i >= n || status[i] != FTS_OK) return;
  const uint32_t* R = rec + (size_t)i * NREC;
  // Nym: NewG1FromBytes (64-byte raw, canonical coordinates, on the curve)
  G1A nym;
  if (!decode_point(nym_raw + (size_t)i * 64, nym)) {
    status[i] = FTS_E_NYM_BADKEY;
    return;
  }
  // t = s_sk HSk + s_rnym HRand + (r - c) Nym
  G1J acc = g1j_identity();
  fb_mul_acc(acc, tables, load_scalar(R + 8));
  fb_mul_acc(acc, tables + FB_WORDS_PER_BASE, load_scalar(R + 16));
  Scalar nc;  // r - c (c < r; c == 0 -> 0)
  {
    uint32_t bw = 0, nz = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) nz |= R[k];
#pragma unroll
    for (int k = 0; k < 8; k++) nc.v[k] = nz ? subb(FrP::M[k], R[k], bw, bw) : 0u;
  }
  const G1J cn = glv_mul(nym, nc, vtab, (size_t)tile, (size_t)li);
  add_inl(acc, cn);
  const G1A t = g1j_to_affine(acc);  // identity -> (0, 0) -> 64 zero bytes (gnark RawBytes)
  uint32_t tw[16], nw[16], hw[8];
  g1_mont_to_be_words(t.x, t.y, tw);
  load_be_words(nym_raw + (size_t)i * 64, nw);
#pragma unroll
  for (int k = 0; k < 8; k++) hw[k] = ipk_hash[k];
  const uint32_t* m = msgw + moff[i];
  const uint32_t len = mlen[i];
  const uint32_t nb = sha_blocks(164u + len);  // >= 3
  uint32_t st[8], w[16];
  sha256_init(st);
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
  for (int k = 1; k < 9; k++) w[k] = hw[k - 1];
#pragma unroll
  for (int k = 9; k < 16; k++) w[k] = stream_word(m, len, nb, 32 + k);
  sha256_compress(st, w);
  for (uint32_t blk = 3; blk < nb; blk++) {
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = stream_word(m, len, nb, 16 * blk + k);
    sha256_compress(st, w);
  }
  // c' = HashToZr(...) ; c'' = HashToZr(c' || Nonce)
  const Fr c1 = digest_to_fr(st);
#pragma unroll
  for (int k = 0; k < 8; k++) w[k] = c1.v[7 - k];
#pragma unroll
  for (int k = 0; k < 8; k++) w[8 + k] = R[24 + k];
  sha256_init(st);
  sha256_compress(st, w);
  w[0] = 0x80000000u;
#pragma unroll
  for (int k = 1; k < 15; k++) w[k] = 0u;
  w[15] = 512u;
  sha256_compress(st, w);
  const Fr c2 = digest_to_fr(st);
  uint32_t diff = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) diff |= c2.v[k] ^ R[k];
  status[i] = diff ? FTS_E_NYM_INVALID : FTS_OK;
}

// One BN254 nym signature per lane.  srec: sk, rnym, r_sk, r_r (canonical LE limbs)
// and the nonce (big-endian words); out <- c, s_sk, s_r (canonical LE limbs).
// Nym is decoded only to give a bad key the verifier's verdict.
__global__ __launch_bounds__(256) void k_nym_sign(int n, const uint32_t* __restrict__ srec,
                                                  const uint8_t* __restrict__ nym_raw,
                                                  const uint32_t* __restrict__ msgw,
                                                  const uint64_t* __restrict__ moff,  // word offsets
                                                  const uint32_t* __restrict__ mlen,
                                                  const uint32_t* __restrict__ tables,
                                                  const uint32_t* __restrict__ ipk_hash,  // 8 BE words
                                                  int32_t* __restrict__ status, uint32_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || status[i] != FTS_OK) return;
  const uint32_t* S = srec + (size_t)i * NSREC;
  G1A nym;
  if (!decode_point(nym_raw + (size_t)i * 64, nym)) {
    status[i] = FTS_E_NYM_BADKEY;
    return;
  }
  // t = r_sk HSk + r_r HRand
  G1J acc = g1j_identity();
  fb_mul_acc(acc, tables, load_scalar(S + 16));
  fb_mul_acc(acc, tables + FB_WORDS_PER_BASE, load_scalar(S + 24));
  const G1A t = g1j_to_affine(acc);  // identity (both nonces zero) -> 64 zero bytes
  uint32_t tw[16], nw[16], hw[8];
  g1_mont_to_be_words(t.x, t.y, tw);
  load_be_words(nym_raw + (size_t)i * 64, nw);
#pragma unroll
  for (int k = 0; k < 8; k++) hw[k] = ipk_hash[k];
  const uint32_t* m = msgw + moff[i];
  const uint32_t len = mlen[i];
  const uint32_t nb = sha_blocks(164u + len);  // >= 3
  uint32_t st[8], w[16];
  sha256_init(st);
  // "sign" t | t[15] Nym | Nym[15] ipk.Hash message (the stream of k_nym_verify)
  w[0] = 0x7369676eu;
#pragma unroll
  for (int k = 1; k < 16; k++) w[k] = tw[k - 1];
  sha256_compress(st, w);
  w[0] = tw[15];
#pragma unroll
  for (int k = 1; k < 16; k++) w[k] = nw[k - 1];
  sha256_compress(st, w);
  w[0] = nw[15];
#pragma unroll
  for (int k = 1; k < 9; k++) w[k] = hw[k - 1];
#pragma unroll
  for (int k = 9; k < 16; k++) w[k] = stream_word(m, len, nb, 32 + k);
  sha256_compress(st, w);
  for (uint32_t blk = 3; blk < nb; blk++) {
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = stream_word(m, len, nb, 16 * blk + k);
    sha256_compress(st, w);
  }
  // c = HashToZr(HashToZr(...) || nonce)
  const Fr c1 = digest_to_fr(st);
#pragma unroll
  for (int k = 0; k < 8; k++) w[k] = c1.v[7 - k];
#pragma unroll
  for (int k = 0; k < 8; k++) w[8 + k] = S[32 + k];
  sha256_init(st);
  sha256_compress(st, w);
  w[0] = 0x80000000u;
#pragma unroll
  for (int k = 1; k < 15; k++) w[k] = 0u;
  w[15] = 512u;
  sha256_compress(st, w);
  const Fr c = digest_to_fr(st);
  // s = r + c * secret: a Montgomery-form factor times a plain one is plain
  const Fr cm = f_to_mont(c);
  Fr sk, rn, rsk, rr;
#pragma unroll
  for (int k = 0; k < 8; k++) sk.v[k] = S[k], rn.v[k] = S[8 + k], rsk.v[k] = S[16 + k], rr.v[k] = S[24 + k];
  const Fr s_sk = f_add(f_mul(cm, sk), rsk), s_r = f_add(f_mul(cm, rn), rr);
  uint32_t* O = out + (size_t)i * NSOUT;
#pragma unroll
  for (int k = 0; k < 8; k++) O[k] = c.v[k], O[8 + k] = s_sk.v[k], O[16 + k] = s_r.v[k];
}

// ------------------------------------------------------------ FP256BN keys
// 16-bit unsigned fixed-base windows: entry (w, d) = d * 2^(16 w) * B, affine
// Montgomery (16 words), d = 0 unused; 64 MiB per base (as the ECDSA table)
constexpr int FBN_W = 16, FBN_NW = 16, FBN_ND = 1 << FBN_W;

// lane per (base, window, digit); bases: affine Montgomery (16 words each)
__global__ __launch_bounds__(256) void k_fbn_table(int nb, const uint32_t* __restrict__ bases,
                                                   uint32_t* __restrict__ table) {
  const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (size_t)nb * FBN_NW * FBN_ND) return;
  const int b = (int)(id / (FBN_NW * FBN_ND)), w = (int)((id / FBN_ND) % FBN_NW), d = (int)(id % FBN_ND);
  uint32_t* out = table + id * 16;
  if (d == 0) {
    for (int i = 0; i < 16; i++) out[i] = 0;
    return;
  }
  const fbn::Fp bx = fbn::load<fbn::PM>(bases + b * 16), by = fbn::load<fbn::PM>(bases + b * 16 + 8);
  fbn::PJ p = fbn::pj_inf();
  for (int k = FBN_W - 1; k >= 0; k--) {
    p = fbn::pj_dbl(p);
    if ((d >> k) & 1) p = fbn::pj_madd(p, bx, by);
  }
  for (int k = 0; k < FBN_W * w; k++) p = fbn::pj_dbl(p);
  const fbn::Fp zi = p256::inv(p.z), zi2 = fbn::sqr(zi);
  const fbn::Fp x = fbn::mul(p.x, zi2), y = fbn::mul(p.y, fbn::mul(zi2, zi));
  for (int i = 0; i < 8; i++) out[i] = x.v[i], out[8 + i] = y.v[i];
}

// big-endian word j of the materialised stream region (length ltot bytes), with
// the SHA-256 terminator / zero fill and the bit length in the last two words
FTS_DEV uint32_t region_word(const uint32_t* __restrict__ m, uint32_t ltot, uint32_t nb, uint32_t g) {
  const uint64_t bits = (uint64_t)ltot * 8u;
  if (g == 16 * nb - 2) return (uint32_t)(bits >> 32);
  if (g == 16 * nb - 1) return (uint32_t)bits;
  return msg_word(m, ltot, g);
}

// digest (state words) as a big-endian integer mod r_fbn, plain LE limbs
// (2^256 < 2 r: at most one subtraction)
FTS_DEV void digest_mod_rfbn(const uint32_t st[8], uint32_t out[8]) {
  uint32_t t[8], bw = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = st[7 - i];
#pragma unroll
  for (int i = 0; i < 8; i++) t[i] = subb(out[i], fbn::RM::M[i], bw, bw);
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = bw ? out[i] : t[i];
}

// FP256BN GLV chain helpers: the lane's 16-entry Jacobian table in global
// memory, [entry][word][stride] (as glv.hpp's vtab for BN254), and the signed
// 4-bit recoding of a 128-bit magnitude over 33 windows (window 32 = the carry)
__device__ inline void fbn_vtab_store(uint32_t* __restrict__ tab, size_t stride, size_t idx, int e, const fbn::PJ& p) {
#pragma unroll
  for (int k = 0; k < 8; k++) {
    tab[((size_t)(e * 24) + k) * stride + idx] = p.x.v[k];
    tab[((size_t)(e * 24) + 8 + k) * stride + idx] = p.y.v[k];
    tab[((size_t)(e * 24) + 16 + k) * stride + idx] = p.z.v[k];
  }
}
__device__ inline fbn::PJ fbn_vtab_load(const uint32_t* __restrict__ tab, size_t stride, size_t idx, int e) {
  fbn::PJ p;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    p.x.v[k] = tab[((size_t)(e * 24) + k) * stride + idx];
    p.y.v[k] = tab[((size_t)(e * 24) + 8 + k) * stride + idx];
    p.z.v[k] = tab[((size_t)(e * 24) + 16 + k) * stride + idx];
  }
  return p;
}
__device__ inline uint64_t fbn_recode(const uint32_t s[4]) {  // bit w = carry into window w
  uint64_t cm = 0;
  uint32_t c = 0;
#pragma unroll
  for (int w = 0; w < 33; w++) {
    cm |= (uint64_t)c << w;
    const uint32_t raw = w < 32 ? (s[w >> 3] >> (4 * (w & 7))) & 15u : 0u;
    c = raw + c > 8u;
  }
  return cm;
}
__device__ inline int fbn_digit(const uint32_t s[4], uint64_t cm, int w) {  // in [-8, 8]
  const int raw = w < 32 ? (int)((s[w >> 3] >> (4 * (w & 7))) & 15u) : 0;
  const int cin = (int)((cm >> w) & 1u);
  const int cout = w < 32 ? (int)((cm >> (w + 1)) & 1u) : 0;
  return raw + cin - 16 * cout;
}

// One FP256BN nym signature per lane.  The host materialises each item's hashed
// stream "sign" || 0x04 || t (64 zero bytes) || Nym (65) || ipk.Hash || msg in
// the region (word aligned); the kernel supplies t's words in registers.
// nymxy: X || Y (64 bytes, big-endian; the 0x04 prefix checked on the host).
__global__ __launch_bounds__(256) void k_nym_verify_fbn(int n, const uint32_t* __restrict__ rec,
                                                        const uint8_t* __restrict__ nymxy,
                                                        const uint32_t* __restrict__ region,
                                                        const uint64_t* __restrict__ roff,  // word offsets
                                                        const uint32_t* __restrict__ rlen,  // stream bytes
                                                        const uint32_t* __restrict__ tables,
                                                        uint32_t* __restrict__ vtab,
                                                        int32_t* __restrict__ status, int base, int tile) {
  const int li = blockIdx.x * blockDim.x + threadIdx.x;  // tiled as k_nym_verify
  const int i = base + li;
  if (li >= tile || i >= n || status[i] != FTS_OK) return;
  const uint32_t* R = rec + (size_t)i * NREC;
  uint32_t pw[16];
  load_be_words(nymxy + (size_t)i * 64, pw);
  uint32_t nx[8], ny[8];
#pragma unroll
  for (int k = 0; k < 8; k++) nx[k] = pw[7 - k], ny[k] = pw[15 - k];
  if (!p256::lt256(nx, fbn::PM::M) || !p256::lt256(ny, fbn::PM::M)) {
    status[i] = FTS_E_NYM_BADKEY;
    return;
  }
  const fbn::Fp Qx = p256::to_mont(fbn::load<fbn::PM>(nx)), Qy = p256::to_mont(fbn::load<fbn::PM>(ny));
  if (!fbn::on_curve(Qx, Qy)) {
    status[i] = FTS_E_NYM_BADKEY;
    return;
  }
  // s_sk HSk + s_rnym HRand: 2 x 16 mixed additions from the tables
  fbn::PJ acc = fbn::pj_inf();
#pragma unroll 1
  for (int q = 0; q < 2; q++) {
    const uint32_t* sc = R + 8 + 8 * q;
    const uint32_t* tb = tables + (size_t)q * FBN_NW * FBN_ND * 16;
    for (int w = 0; w < FBN_NW; w++) {
      const uint32_t d = (sc[w >> 1] >> (16 * (w & 1))) & 0xffffu;
      if (d) {
        const uint32_t* t = tb + ((size_t)w * FBN_ND + d) * 16;
        acc = fbn::pj_madd(acc, fbn::load<fbn::PM>(t), fbn::load<fbn::PM>(t + 8));
      }
    }
  }
  // (r - c) Nym by GLV: e = k1 + k2 lambda, one joint chain of k1 (+-Nym) +
  // k2 (+-phi(Nym)) over 33 signed 4-bit windows (|k_i| < 2^128), 128 doublings
  // instead of 252; tables 1..8 of both points in the lane's global slot
  uint32_t e[8];
  {
    uint32_t bw = 0, nz = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) nz |= R[k];
#pragma unroll
    for (int k = 0; k < 8; k++) e[k] = nz ? subb(fbn::RM::M[k], R[k], bw, bw) : 0u;
  }
  uint32_t k1[4], k2[4], s1, s2;
  fts::glv_decompose<fbn::GlvK>(e, k1, s1, k2, s2);
  const fbn::Fp nQy = fbn::sub(fbn::Fp{}, Qy);
  const fbn::Fp Px = Qx, Py = s1 ? nQy : Qy;
  const fbn::Fp Ex = fbn::mul(Qx, fbn::load<fbn::PM>(fbn::GlvK::BETA)), Ey = s2 ? nQy : Qy;
  const size_t stride = (size_t)tile;
  {
    fbn::PJ cp, ce;
    cp.x = Px, cp.y = Py, cp.z = fbn::load<fbn::PM>(fbn::PM::ONE);
    ce.x = Ex, ce.y = Ey, ce.z = cp.z;
    fbn_vtab_store(vtab, stride, (size_t)li, 0, cp);
    fbn_vtab_store(vtab, stride, (size_t)li, 8, ce);
    for (int k = 1; k < 8; k++) {
      cp = fbn::pj_madd(cp, Px, Py);
      ce = fbn::pj_madd(ce, Ex, Ey);
      fbn_vtab_store(vtab, stride, (size_t)li, k, cp);
      fbn_vtab_store(vtab, stride, (size_t)li, 8 + k, ce);
    }
  }
  const uint64_t ca = fbn_recode(k1), cb = fbn_recode(k2);
  fbn::PJ vb = fbn::pj_inf();
  for (int w = 32; w >= 0; w--) {
    const int da = fbn_digit(k1, ca, w), db = fbn_digit(k2, cb, w);
    fbn::PJ qa, qb;
    if (da) qa = fbn_vtab_load(vtab, stride, (size_t)li, (da < 0 ? -da : da) - 1);
    if (db) qb = fbn_vtab_load(vtab, stride, (size_t)li, 8 + (db < 0 ? -db : db) - 1);
    if (w != 32) vb = fbn::pj_dbl(fbn::pj_dbl(fbn::pj_dbl(fbn::pj_dbl(vb))));
    if (da) {
      if (da < 0) qa.y = fbn::sub(fbn::Fp{}, qa.y);
      vb = fbn::pj_add(vb, qa);
    }
    if (db) {
      if (db < 0) qb.y = fbn::sub(fbn::Fp{}, qb.y);
      vb = fbn::pj_add(vb, qb);
    }
  }
  const fbn::PJ X = fbn::pj_add(acc, vb);
  uint32_t tw[16];
  if (fbn::is_zero(X.z)) {
#pragma unroll
    for (int k = 0; k < 16; k++) tw[k] = 0u;  // t = O (zero nonces): AMCL ToBytes of infinity = 0x04 || 0 || 1
    tw[15] = 1u;
  } else {
    const fbn::Fp zi = p256::inv(X.z), zi2 = fbn::sqr(zi);
    const fbn::Fp ax = p256::from_mont(fbn::mul(X.x, zi2)), ay = p256::from_mont(fbn::mul(X.y, fbn::mul(zi2, zi)));
#pragma unroll
    for (int k = 0; k < 8; k++) tw[k] = ax.v[7 - k], tw[8 + k] = ay.v[7 - k];
  }
  const uint32_t* m = region + roff[i];
  const uint32_t ltot = rlen[i];
  const uint32_t nb = sha_blocks(ltot);  // >= 3
  uint32_t st[8], w[16];
  sha256_init(st);
  // block 0: "sign" 0x04 t[0..58]
  w[0] = 0x7369676eu;
  w[1] = 0x04000000u | (tw[0] >> 8);
#pragma unroll
  for (int k = 2; k < 16; k++) w[k] = (tw[k - 2] << 24) | (tw[k - 1] >> 8);
  sha256_compress(st, w);
  // block 1: t[59..63] then the host's bytes (Nym, ipk.Hash, message)
  w[0] = (tw[14] << 24) | (tw[15] >> 8);
  w[1] = (tw[15] << 24) | (region_word(m, ltot, nb, 17) & 0x00ffffffu);
#pragma unroll
  for (int k = 2; k < 16; k++) w[k] = region_word(m, ltot, nb, 16 + k);
  sha256_compress(st, w);
  for (uint32_t blk = 2; blk < nb; blk++) {
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = region_word(m, ltot, nb, 16 * blk + k);
    sha256_compress(st, w);
  }
  uint32_t c1[8], c2[8];
  digest_mod_rfbn(st, c1);
#pragma unroll
  for (int k = 0; k < 8; k++) w[k] = c1[7 - k];
#pragma unroll
  for (int k = 0; k < 8; k++) w[8 + k] = R[24 + k];
  sha256_init(st);
  sha256_compress(st, w);
  w[0] = 0x80000000u;
#pragma unroll
  for (int k = 1; k < 15; k++) w[k] = 0u;
  w[15] = 512u;
  sha256_compress(st, w);
  digest_mod_rfbn(st, c2);
  uint32_t diff = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) diff |= c2[k] ^ R[k];
  status[i] = diff ? FTS_E_NYM_INVALID : FTS_OK;
}

// One FP256BN nym signature per lane: srec and out as k_nym_sign, the region and nymxy
// as k_nym_verify_fbn.
__global__ __launch_bounds__(256) void k_nym_sign_fbn(int n, const uint32_t* __restrict__ srec,
                                                      const uint8_t* __restrict__ nymxy,
                                                      const uint32_t* __restrict__ region,
                                                      const uint64_t* __restrict__ roff,  // word offsets
                                                      const uint32_t* __restrict__ rlen,  // stream bytes
                                                      const uint32_t* __restrict__ tables,
                                                      int32_t* __restrict__ status, uint32_t* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || status[i] != FTS_OK) return;
  const uint32_t* S = srec + (size_t)i * NSREC;
  uint32_t pw[16];
  load_be_words(nymxy + (size_t)i * 64, pw);
  uint32_t nx[8], ny[8];
#pragma unroll
  for (int k = 0; k < 8; k++) nx[k] = pw[7 - k], ny[k] = pw[15 - k];
  if (!p256::lt256(nx, fbn::PM::M) || !p256::lt256(ny, fbn::PM::M) ||
      !fbn::on_curve(p256::to_mont(fbn::load<fbn::PM>(nx)), p256::to_mont(fbn::load<fbn::PM>(ny)))) {
    status[i] = FTS_E_NYM_BADKEY;
    return;
  }
  // t = r_sk HSk + r_r HRand: 2 x 16 mixed additions from the tables
  fbn::PJ acc = fbn::pj_inf();
#pragma unroll 1
  for (int q = 0; q < 2; q++) {
    const uint32_t* sc = S + 16 + 8 * q;
    const uint32_t* tb = tables + (size_t)q * FBN_NW * FBN_ND * 16;
    for (int w = 0; w < FBN_NW; w++) {
      const uint32_t d = (sc[w >> 1] >> (16 * (w & 1))) & 0xffffu;
      if (d) {
        const uint32_t* t = tb + ((size_t)w * FBN_ND + d) * 16;
        acc = fbn::pj_madd(acc, fbn::load<fbn::PM>(t), fbn::load<fbn::PM>(t + 8));
      }
    }
  }
  uint32_t tw[16];
  if (fbn::is_zero(acc.z)) {
#pragma unroll
    for (int k = 0; k < 16; k++) tw[k] = 0u;  // t = O (both nonces zero): AMCL ToBytes of infinity
    tw[15] = 1u;
  } else {
    const fbn::Fp zi = p256::inv(acc.z), zi2 = fbn::sqr(zi);
    const fbn::Fp ax = p256::from_mont(fbn::mul(acc.x, zi2)), ay = p256::from_mont(fbn::mul(acc.y, fbn::mul(zi2, zi)));
#pragma unroll
    for (int k = 0; k < 8; k++) tw[k] = ax.v[7 - k], tw[8 + k] = ay.v[7 - k];
  }
  const uint32_t* m = region + roff[i];
  const uint32_t ltot = rlen[i];
  const uint32_t nb = sha_blocks(ltot);  // >= 3
  uint32_t st[8], w[16];
  sha256_init(st);
  // "sign" 0x04 t[0..58] | t[59..63] then the host's bytes (the stream of k_nym_verify_fbn)
  w[0] = 0x7369676eu;
  w[1] = 0x04000000u | (tw[0] >> 8);
#pragma unroll
  for (int k = 2; k < 16; k++) w[k] = (tw[k - 2] << 24) | (tw[k - 1] >> 8);
  sha256_compress(st, w);
  w[0] = (tw[14] << 24) | (tw[15] >> 8);
  w[1] = (tw[15] << 24) | (region_word(m, ltot, nb, 17) & 0x00ffffffu);
#pragma unroll
  for (int k = 2; k < 16; k++) w[k] = region_word(m, ltot, nb, 16 + k);
  sha256_compress(st, w);
  for (uint32_t blk = 2; blk < nb; blk++) {
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = region_word(m, ltot, nb, 16 * blk + k);
    sha256_compress(st, w);
  }
  uint32_t c1[8];
  digest_mod_rfbn(st, c1);
#pragma unroll
  for (int k = 0; k < 8; k++) w[k] = c1[7 - k];
#pragma unroll
  for (int k = 0; k < 8; k++) w[8 + k] = S[32 + k];
  sha256_init(st);
  sha256_compress(st, w);
  w[0] = 0x80000000u;
#pragma unroll
  for (int k = 1; k < 15; k++) w[k] = 0u;
  w[15] = 512u;
  sha256_compress(st, w);
  using Fz = p256::F<fbn::RM>;
  Fz c;
  digest_mod_rfbn(st, c.v);
  // s = r + c * secret mod r: a Montgomery-form factor times a plain one is plain
  const Fz cm = p256::to_mont(c);
  const Fz s_sk = fbn::add(fbn::mul(cm, fbn::load<fbn::RM>(S)), fbn::load<fbn::RM>(S + 16));
  const Fz s_r = fbn::add(fbn::mul(cm, fbn::load<fbn::RM>(S + 8)), fbn::load<fbn::RM>(S + 24));
  uint32_t* O = out + (size_t)i * NSOUT;
#pragma unroll
  for (int k = 0; k < 8; k++) O[k] = c.v[k], O[8 + k] = s_sk.v[k], O[16 + k] = s_r.v[k];
}

// FP256BN issuer bases: plain big-endian ECP coordinates -> Montgomery, on-curve flags
__global__ void k_fbn_bases(int nb, const uint32_t* __restrict__ plain, uint32_t* __restrict__ mont,
                            int32_t* __restrict__ ok) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nb) return;
  uint32_t x[8], y[8];
  for (int k = 0; k < 8; k++) x[k] = plain[b * 16 + k], y[k] = plain[b * 16 + 8 + k];
  bool good = p256::lt256(x, fbn::PM::M) && p256::lt256(y, fbn::PM::M);
  const fbn::Fp mx = p256::to_mont(fbn::load<fbn::PM>(x)), my = p256::to_mont(fbn::load<fbn::PM>(y));
  good = good && fbn::on_curve(mx, my);
  for (int k = 0; k < 8; k++) mont[b * 16 + k] = mx.v[k], mont[b * 16 + 8 + k] = my.v[k];
  ok[b] = good ? 1 : 0;
}

}  // namespace

namespace fts {
// FP256BN fixed-base tables (FBN layout: FBN_NW windows x 2^16 unsigned digits,
// affine Montgomery) of nb bases given as plain LE-limb affine coordinates
// (16 words each, on the device); ok[b] <- base b canonical and on the curve.
// mont: nb * 16 words of scratch.  Used by the nym and identity-proof handles.
void fbn_build_tables(const uint32_t* plain, int nb, uint32_t* mont, int32_t* ok, uint32_t* tables, hipStream_t s) {
  k_fbn_bases<<<1, 64, 0, s>>>(nb, plain, mont, ok);
  const size_t ent = (size_t)nb * FBN_NW * FBN_ND;
  k_fbn_table<<<(unsigned)((ent + 255) / 256), 256, 0, s>>>(nb, mont, tables);
}
size_t fbn_words_per_base() { return (size_t)FBN_NW * FBN_ND * 16; }

void launch_nym_verify(bool bn, int n, const uint32_t* rec, const uint8_t* nym, const uint32_t* msgw,
                       const uint64_t* moff, const uint32_t* mlen, const uint32_t* tables, const uint32_t* ipk_hash,
                       uint32_t* vtab, int32_t* status, int base, int tile, hipStream_t s) {
  const unsigned grid = (unsigned)((tile + 255) / 256);
  if (bn) k_nym_verify<<<grid, 256, 0, s>>>(n, rec, nym, msgw, moff, mlen, tables, ipk_hash, vtab, status, base, tile);
  else k_nym_verify_fbn<<<grid, 256, 0, s>>>(n, rec, nym, msgw, moff, mlen, tables, vtab, status, base, tile);
}

void launch_nym_sign(bool bn, int n, const uint32_t* srec, const uint8_t* nym, const uint32_t* msgw,
                     const uint64_t* moff, const uint32_t* mlen, const uint32_t* tables, const uint32_t* ipk_hash,
                     int32_t* status, uint32_t* out, hipStream_t s) {
  const unsigned grid = (unsigned)((n + 255) / 256);
  if (bn) k_nym_sign<<<grid, 256, 0, s>>>(n, srec, nym, msgw, moff, mlen, tables, ipk_hash, status, out);
  else k_nym_sign_fbn<<<grid, 256, 0, s>>>(n, srec, nym, msgw, moff, mlen, tables, status, out);
}
}  // namespace fts
