// Batched idemix pseudonym signatures over BN254 and FP256BN (SURVEY.md §8(f) row 4,
// the idemix half): verifying the owner signatures of transfers whose input tokens
// are owned by idemix identities, and making them.
//
// Reference call chain:
//   validator/validator_transfer.go:29-62  TransferSignatureValidate, per input
//   services/identity/idemix/deserializer.go:82-105  owner verifier =
//       crypto.NymSignatureVerifier{IPK, NymPK}
//   services/identity/idemix/crypto/id.go:145-161  NymSignatureVerifier.Verify
//       -> bccsp Verify(NymPK, sigma, msg, IdemixNymSignerOpts{IssuerPK})
//   github.com/IBM/idemix (go.mod:6, not vendored) NymSignature.Ver / NewNymSignature
// (restated and pinned as far as the reference's fixtures allow in oracle/idemix.py).
//
// This unit instantiates k_nym_sign<CV> (device/nym_kernels.hpp) for BnCurve and FbnCurve
// and k_nym_verify<CV> for FbnCurve, holds the BN254 verifier as it was written before
// them (k_nym_verify below) and builds the FP256BN fixed-base tables.  The BN254 tables
// of HSk and HRand are rp_tables.hip's (launch_build_tables, 32 MiB each).
// The host side (handle, parser, staging) is api_idemix.cpp over host/idemix_parse.hpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device/nym_kernels.hpp"
#include "device/launch.hpp"

using namespace fts;
using idv::FBN_ND;
using idv::FBN_NW;
using idv::FBN_W;
using idv::NREC;

namespace {

// ------------------------------------------------------- BN254 verification
// k_nym_verify on BN254 keeps the text it had before the nym kernels became templates, its
// own stream words and second hash included: as k_nym_verify<BnCurve> (nym_challenge over
// NymOps<BnCurve> and idemix_hash.hpp), and again written out in this statement order over
// those helpers, it measured 0.023 ms per 65,536 signatures (0.85 %) slower than this text
// in every round, with the same registers.  What it computes is
// nym_challenge<BnCurve, true>; a transcript fix is made there and here.
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

// ------------------------------------------------------------ FP256BN keys
// 16-bit unsigned fixed-base windows: entry (w, d) = d * 2^(16 w) * B, affine
// Montgomery (16 words), d = 0 unused; 64 MiB per base (as the ECDSA table)

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

// msgw: the messages (bn) or the materialised streams (FP256BN, which does not read ipk_hash)
void launch_nym_verify(bool bn, int n, const uint32_t* rec, const uint8_t* nym, const uint32_t* msgw,
                       const uint64_t* moff, const uint32_t* mlen, const uint32_t* tables, const uint32_t* ipk_hash,
                       uint32_t* vtab, int32_t* status, int base, int tile, hipStream_t s) {
  const unsigned grid = (unsigned)((tile + 255) / 256);
  auto* k = bn ? k_nym_verify : idv::k_nym_verify<idv::FbnCurve>;
  k<<<grid, 256, 0, s>>>(n, rec, nym, msgw, moff, mlen, tables, ipk_hash, vtab, status, base, tile);
}

void launch_nym_sign(bool bn, int n, const uint32_t* srec, const uint8_t* nym, const uint32_t* msgw,
                     const uint64_t* moff, const uint32_t* mlen, const uint32_t* tables, const uint32_t* ipk_hash,
                     int32_t* status, uint32_t* out, hipStream_t s) {
  const unsigned grid = (unsigned)((n + 255) / 256);
  auto* k = bn ? idv::k_nym_sign<idv::BnCurve> : idv::k_nym_sign<idv::FbnCurve>;
  k<<<grid, 256, 0, s>>>(n, srec, nym, msgw, moff, mlen, tables, ipk_hash, status, out);
}

}  // namespace fts
