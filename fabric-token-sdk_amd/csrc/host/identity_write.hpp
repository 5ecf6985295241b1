// Host side of identity generation (fts_idemix_identity_generate_batch): the draws of one
// identity, the parsers of the credential and its revocation information, and the writer of
// SerializedIdemixIdentity{1 nym_public_key, 4 proof} with the Signature proto laid out as
// oracle/idemix_identity.py encode_signature writes it.  Host only: no HIP call, no handle,
// no global state; lib/idgen_check runs it under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "pb.hpp"
#include "prover.hpp"  // Rng
#include "u256.hpp"

namespace fts {
namespace idgen {

// ------------------------------------------------------------------ draws
// The 18 scalars of one identity, in the order they are drawn from the item's stream
// (RngSource(seed).at(i)): rnym first, then the order of the oracle's sign.
constexpr int ND = 18;
constexpr int D_RNYM = 0, D_R1 = 1, D_R2 = 2, D_NONCE = 3, D_RSK = 4, D_RE = 5, D_RR2 = 6, D_RR3 = 7, D_RSP = 8,
              D_RRNYM = 9, D_RA = 10, D_REID = 14, D_RRH = 15, D_RREID = 16, D_RRRH = 17;

// uniform below the curve's r by rejection (canonical LE limbs): four words of the stream,
// the top two bits masked off for the 254-bit r of BN254 (the values Rng::fr() yields)
inline void draw_below_r(host::Rng& rng, bool bn, uint32_t out[8]) {
  const uint32_t* r = bn ? u256::kRbn : u256::kRfbn;
  do {
    for (int k = 0; k < 4; k++) {
      uint64_t v = rng.next();
      if (bn && k == 3) v &= 0x3fffffffffffffffULL;
      out[2 * k] = (uint32_t)v, out[2 * k + 1] = (uint32_t)(v >> 32);
    }
  } while (u256::ge(out, r));
}
inline bool is_zero8(const uint32_t a[8]) {
  uint32_t o = 0;
  for (int k = 0; k < 8; k++) o |= a[k];
  return o == 0;
}
// r1 = 0 is redrawn (its inverse is needed)
inline void identity_draws(bool bn, host::Rng rng, uint32_t out[ND][8]) {
  for (int k = 0; k < ND; k++) do draw_below_r(rng, bn, out[k]);
    while (k == D_R1 && is_zero8(out[k]));
}

// canonical LE limbs <-> 32 big-endian bytes
inline void limbs_to_be32(const uint32_t a[8], uint8_t out[32]) {
  for (int k = 0; k < 8; k++)
    for (int b = 0; b < 4; b++) out[4 * k + b] = (uint8_t)(a[7 - k] >> (24 - 8 * b));
}

// ------------------------------------------------- credential and revocation info
// Credential{1 a, 2 b (ECP), 3 e, 4 s, 5 attrs (repeated)}: A and B as X || Y, the scalars
// as canonical limbs.  false: malformed, not exactly four attributes, or a scalar >= r.
struct CredFields {
  uint8_t a[64], b[64];
  uint32_t e[8], s[8], attrs[4][8];
};
inline bool parse_credential(const uint8_t* cred, size_t len, bool bn, CredFields& c) {
  const uint32_t* r = bn ? u256::kRbn : u256::kRfbn;
  Pb pb{cred, len};
  Pb::Field d;
  Span pa, pbb, e, s, at[4];
  size_t na = 0;
  while (pb.o < pb.n) {
    if (!pb.next(d)) return false;
    if (d.f >= 1 && d.f <= 5 && d.wt != 2) return false;
    const Span v{d.v, d.vl, true};
    if (d.f == 1) pa = v;
    if (d.f == 2) pbb = v;
    if (d.f == 3) e = v;
    if (d.f == 4) s = v;
    if (d.f == 5) {
      if (na < 4) at[na] = v;
      na++;
    }
  }
  if (na != 4 || !ecp_xy(pa, c.a, true) || !ecp_xy(pbb, c.b, true)) return false;
  auto zr = [&](const Span& f, uint32_t out[8]) { return u256::be_limbs(f.p, f.n, out) && !u256::ge(out, r); };
  if (!zr(e, c.e) || !zr(s, c.s)) return false;
  for (int k = 0; k < 4; k++)
    if (!zr(at[k], c.attrs[k])) return false;
  return true;
}

// the G2 generators as the curves' ECP2 protos carry them (BN254: gnark's raw order,
// imaginary parts first; FP256BN: AMCL's, real parts first): what ALG_NO_REVOCATION
// writes as epoch_pk
constexpr uint8_t kG2Bn[128] = {
    0x19, 0x8e, 0x93, 0x93, 0x92, 0x0d, 0x48, 0x3a, 0x72, 0x60, 0xbf, 0xb7, 0x31, 0xfb, 0x5d, 0x25, 0xf1, 0xaa, 0x49,
    0x33, 0x35, 0xa9, 0xe7, 0x12, 0x97, 0xe4, 0x85, 0xb7, 0xae, 0xf3, 0x12, 0xc2, 0x18, 0x00, 0xde, 0xef, 0x12, 0x1f,
    0x1e, 0x76, 0x42, 0x6a, 0x00, 0x66, 0x5e, 0x5c, 0x44, 0x79, 0x67, 0x43, 0x22, 0xd4, 0xf7, 0x5e, 0xda, 0xdd, 0x46,
    0xde, 0xbd, 0x5c, 0xd9, 0x92, 0xf6, 0xed, 0x09, 0x06, 0x89, 0xd0, 0x58, 0x5f, 0xf0, 0x75, 0xec, 0x9e, 0x99, 0xad,
    0x69, 0x0c, 0x33, 0x95, 0xbc, 0x4b, 0x31, 0x33, 0x70, 0xb3, 0x8e, 0xf3, 0x55, 0xac, 0xda, 0xdc, 0xd1, 0x22, 0x97,
    0x5b, 0x12, 0xc8, 0x5e, 0xa5, 0xdb, 0x8c, 0x6d, 0xeb, 0x4a, 0xab, 0x71, 0x80, 0x8d, 0xcb, 0x40, 0x8f, 0xe3, 0xd1,
    0xe7, 0x69, 0x0c, 0x43, 0xd3, 0x7b, 0x4c, 0xe6, 0xcc, 0x01, 0x66, 0xfa, 0x7d, 0xaa};
constexpr uint8_t kG2Fbn[128] = {
    0xfe, 0x0c, 0x33, 0x50, 0xb4, 0xc9, 0x6c, 0x20, 0x28, 0x56, 0x0f, 0x57, 0x7c, 0x28, 0x91, 0x3a, 0xce, 0x1c, 0x53,
    0x9a, 0x12, 0xbf, 0x84, 0x3c, 0xd2, 0x26, 0x16, 0xb6, 0x89, 0xc0, 0x9e, 0xfb, 0x4e, 0xa6, 0x60, 0x57, 0x73, 0x8a,
    0xc0, 0x54, 0xdb, 0x5a, 0xe1, 0xc6, 0x37, 0xd8, 0x13, 0xb9, 0x24, 0xdd, 0x78, 0xe2, 0x87, 0xd0, 0x35, 0x89, 0xd2,
    0x69, 0xed, 0x34, 0xa3, 0x7e, 0x6a, 0x2b, 0x70, 0x20, 0x46, 0xe7, 0xc5, 0x42, 0xa3, 0xb3, 0x76, 0x77, 0x0d, 0x75,
    0x12, 0x4e, 0x3e, 0x51, 0xef, 0xcb, 0x24, 0x75, 0x8d, 0x61, 0x58, 0x48, 0xe9, 0x09, 0xb4, 0x81, 0xbe, 0xdc, 0x27,
    0xff, 0x05, 0x54, 0xe3, 0xbc, 0xd3, 0x88, 0xc2, 0x90, 0x42, 0xee, 0xa6, 0x49, 0x29, 0x7e, 0xb2, 0x9f, 0x8b, 0x4c,
    0xbe, 0x80, 0x82, 0x1a, 0x98, 0xb3, 0xe0, 0x12, 0x81, 0x11, 0x4a, 0xad, 0x04, 0x9b};

// CredentialRevocationInformation{1 epoch, 2 epoch_pk (ECP2), 3 epoch_pk_sig, 4 revocation_alg,
// 5 revocation_data}; nullptr: epoch 0 and the generator.  false: malformed, no epoch key, or
// a revocation algorithm other than ALG_NO_REVOCATION (0).
struct CriFields {
  uint64_t epoch = 0;
  uint8_t epoch_pk[128];
};
inline bool parse_cri(const uint8_t* cri, size_t len, bool bn, CriFields& c) {
  c.epoch = 0;
  memcpy(c.epoch_pk, bn ? kG2Bn : kG2Fbn, 128);
  if (!cri) return true;
  Pb pb{cri, len};
  Pb::Field d;
  Span pk;
  uint64_t alg = 0;
  while (pb.o < pb.n) {
    if (!pb.next(d)) return false;
    if ((d.f == 1 || d.f == 4) && d.wt != 0) return false;
    if ((d.f == 2 || d.f == 3 || d.f == 5) && d.wt != 2) return false;
    if (d.f == 1) c.epoch = d.iv;
    if (d.f == 4) alg = d.iv;
    if (d.f == 2) pk = Span{d.v, d.vl, true};
  }
  if (alg != 0) return false;
  if ((int64_t)c.epoch < 0) return false;  // an int64 on the wire
  return ecp2_raw(pk, c.epoch_pk);
}

// --------------------------------------------------------------- the writer
inline size_t varint_len(uint64_t v) {
  size_t n = 1;
  while (v >>= 7) n++;
  return n;
}
// one identity's values, every one in the byte order of the wire
struct IdentityParts {
  const uint8_t* pts;     // A', ABar, B', Nym, EidNym, RhNym: X || Y, 64 bytes each
  const uint8_t* sc;      // c sSk sE sR2 sR3 sS' sAttrs[0..3] sRNym sEid sRh: 32 bytes each
  const uint8_t* nonce;   // 32 bytes
  const uint8_t* epoch_pk;  // 128 bytes
  uint64_t epoch;
};
constexpr int NPTS = 6, NSC = 13;
constexpr int W_AP = 0, W_ABAR = 1, W_BP = 2, W_NYM = 3, W_EID = 4, W_RH = 5;
constexpr int W_C = 0, W_SSK = 1, W_SE = 2, W_SR2 = 3, W_SR3 = 4, W_SSP = 5, W_SA = 6, W_SRNYM = 10, W_SEID = 11,
              W_SRH = 12;
static_assert(W_SRH + 1 == NSC, "scalar slots");

inline size_t proof_len(uint64_t epoch) {
  // 1..3, 12: ECP (70 each); 4..9, 10 x 4, 11, 13: Zr (34 each); 14: ECP2 (139); 17 (3); 18, 19 (107 each)
  return 4 * 70 + 12 * 34 + 139 + 3 + 2 * 107 + (epoch ? 2 + varint_len(epoch) : 0);
}
inline size_t identity_len(bool bn, uint64_t epoch) {
  const size_t pl = proof_len(epoch), nl = bn ? 64 : 65;
  return 2 + nl + 1 + varint_len(pl) + pl;
}

struct Wr {
  uint8_t* p;
  void byte(uint8_t b) { *p++ = b; }
  void varint(uint64_t v) {
    while (v > 0x7f) byte((uint8_t)(v | 0x80)), v >>= 7;
    byte((uint8_t)v);
  }
  void key(uint32_t f, uint32_t wt) { varint(((uint64_t)f << 3) | wt); }
  void bytes(const uint8_t* s, size_t n) {
    memcpy(p, s, n);
    p += n;
  }
  void zr(uint32_t f, const uint8_t* s) { key(f, 2), byte(32), bytes(s, 32); }
  void ecp_body(const uint8_t* xy) { zr(1, xy), zr(2, xy + 32); }
  void ecp(uint32_t f, const uint8_t* xy) { key(f, 2), byte(68), ecp_body(xy); }
  void nym(uint32_t f, const uint8_t* xy, const uint8_t* s) { key(f, 2), byte(104), ecp(1, xy), zr(2, s); }
};

// writes exactly identity_len(bn, v.epoch) bytes at out
inline void write_identity(bool bn, const IdentityParts& v, uint8_t* out) {
  Wr w{out};
  const uint8_t* P = v.pts;
  const uint8_t* S = v.sc;
  // nym_public_key = G1.Bytes(): X || Y (BN254), 0x04 || X || Y (FP256BN)
  w.key(1, 2);
  w.byte(bn ? 64 : 65);
  if (!bn) w.byte(0x04);
  w.bytes(P + 64 * W_NYM, 64);
  w.key(4, 2);
  w.varint(proof_len(v.epoch));
  w.ecp(1, P + 64 * W_AP), w.ecp(2, P + 64 * W_ABAR), w.ecp(3, P + 64 * W_BP);
  for (int k = 0; k < 6; k++) w.zr(4 + k, S + 32 * (W_C + k));  // c sSk sE sR2 sR3 sS'
  for (int k = 0; k < 4; k++) w.zr(10, S + 32 * (W_SA + k));
  w.zr(11, v.nonce);
  w.ecp(12, P + 64 * W_NYM);
  w.zr(13, S + 32 * W_SRNYM);
  w.key(14, 2), w.varint(136);
  for (int k = 0; k < 4; k++) w.zr(1 + k, v.epoch_pk + 32 * k);
  if (v.epoch) w.key(16, 0), w.varint(v.epoch);
  w.key(17, 2), w.byte(0);
  w.nym(18, P + 64 * W_EID, S + 32 * W_SEID);
  w.nym(19, P + 64 * W_RH, S + 32 * W_SRH);
}

}  // namespace idgen
}  // namespace fts
