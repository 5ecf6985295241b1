// Host side of the issuer-key calls (fts_idemix_ipk_check_batch, fts_idemix_issuer_keygen_batch):
// the reading of an untrusted IssuerPublicKey{1 attribute_names, 2 h_sk, 3 h_rand, 4 h_attrs,
// 5 w, 6 bar_g1, 7 bar_g2, 8 proof_c, 9 proof_s, 10 hash} as IssuerPublicKey.Check takes it, its
// hash, the draws of one new key and the writer of its proto.  Host only: no HIP call, no
// handle, no global state; lib/ipk_check runs it under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../../include/fts_gpu.h"
#include "../common/sha256.hpp"
#include "identity_write.hpp"  // draw_below_r, is_zero8, limbs_to_be32, Wr, kG2Bn, kG2Fbn
#include "pb.hpp"
#include "u256.hpp"

namespace fts {
namespace ipkw {

// the four attribute names the handles require; field 1 of a generated key
constexpr const char* kNames[4] = {"OU", "Role", "EnrollmentID", "RevocationHandle"};
// names 4 + 6 + 14 + 18; eight ECP fields of 70; W 3 + 136; ProofC, ProofS and hash 34 each
constexpr size_t IPK_LEN = 42 + 8 * 70 + 139 + 3 * 34;
static_assert(IPK_LEN == FTS_IDEMIX_IPK_LEN, "wire length");

// ----------------------------------------------------------------- the check's reading
// What the device needs of one key.  A field with another wire type is ignored and the last
// occurrence of a singular field wins, as in idv::parse_ipk; HAttrs are counted here and
// fetched by hattr().
struct CheckFields {
  uint8_t h_sk[64], h_rand[64], bar[128], w[128];
  uint32_t c_cmp[8], s[8], neg_c[8];  // ProofC as sent, ProofS mod r, -ProofC mod r
  size_t n_names, n_attrs;
};
// -> FTS_OK (to the device), FTS_E_IPK_MALFORMED or FTS_E_IPK_UNDEFINED, in this order: a NULL or
// empty input or a proto that does not parse (malformed); a missing HSk, HRand, W, BarG1, BarG2,
// ProofC or ProofS, or fewer HAttrs than attribute names (undefined); a ProofC or ProofS not of
// 32 bytes, a coordinate not of 32 bytes (malformed)
inline int32_t parse_for_check(const uint8_t* ipk, size_t len, bool bn, CheckFields& k) {
  const uint32_t* rmod = bn ? u256::kRbn : u256::kRfbn;
  memset(&k, 0, sizeof k);
  if (!ipk || !len) return FTS_E_IPK_MALFORMED;
  Pb pb{ipk, len};
  Pb::Field d;
  Span f[10];
  while (pb.o < pb.n) {
    if (!pb.next(d)) return FTS_E_IPK_MALFORMED;
    if (d.wt != 2) continue;
    if (d.f == 1) k.n_names++;
    if (d.f == 4) k.n_attrs++;
    if (d.f >= 2 && d.f <= 9 && d.f != 4) f[d.f] = Span{d.v, d.vl, true};
  }
  for (int q : {2, 3, 5, 6, 7, 8, 9})
    if (!f[q].set) return FTS_E_IPK_UNDEFINED;
  if (k.n_attrs < k.n_names) return FTS_E_IPK_UNDEFINED;
  if (f[8].n != 32 || f[9].n != 32) return FTS_E_IPK_MALFORMED;
  if (!ecp_xy(f[2], k.h_sk, true) || !ecp_xy(f[3], k.h_rand, true) || !ecp2_raw(f[5], k.w) ||
      !ecp_xy(f[6], k.bar, false) || !ecp_xy(f[7], k.bar + 64, false)) {
    memset(k.h_sk, 0, 64), memset(k.h_rand, 0, 64), memset(k.bar, 0, 128), memset(k.w, 0, 128);
    return FTS_E_IPK_MALFORMED;
  }
  u256::be_limbs(f[8].p, 32, k.c_cmp);
  u256::mod_m(f[9].p, 32, rmod, k.s);
  uint32_t c[8];
  u256::mod_m(f[8].p, 32, rmod, c);
  if (!idgen::is_zero8(c)) {
    memcpy(k.neg_c, rmod, 32);
    u256::sub(k.neg_c, c);
  }
  return FTS_OK;
}
// every HAttrs of a key that parsed as X || Y, 64 bytes each, in one pass: out holds cap of
// them (cap = the key's n_attrs).  false: one is not an ECP of two 32-byte coordinates.
inline bool hattrs(const uint8_t* ipk, size_t len, uint8_t* out, size_t cap) {
  Pb pb{ipk, len};
  Pb::Field d;
  size_t seen = 0;
  while (pb.o < pb.n) {
    if (!pb.next(d)) return false;
    if (d.wt != 2 || d.f != 4) continue;
    if (seen >= cap || !ecp_xy(Span{d.v, d.vl, true}, out + 64 * seen, true)) return false;
    seen++;
  }
  return seen == cap;
}

// HashToZr of the key's bytes without its hash: every field but number 10, in the order of the
// wire (a key marshalled by Go carries its fields in number order, so this is the encoding
// SetHash hashes).  false: the proto does not parse.
inline bool hash_without_field10(const uint8_t* ipk, size_t len, bool bn, uint8_t out[32]) {
  memset(out, 0, 32);
  if (!ipk) return false;
  Pb pb{ipk, len};
  Pb::Field d;
  Sha256 h;
  h.init();
  while (pb.o < pb.n) {
    const size_t at = pb.o;
    if (!pb.next(d)) return false;
    if (d.f != 10) h.update(ipk + at, pb.o - at);
  }
  uint8_t dg[32];
  h.final(dg);
  uint32_t z[8];
  u256::mod_m(dg, 32, bn ? u256::kRbn : u256::kRfbn, z);
  idgen::limbs_to_be32(z, out);
  return true;
}

// ------------------------------------------------------------------ draws
// one new key, in the order they are drawn from the item's stream: isk, HSk, HRand,
// HAttrs[0..3], BarG1, r; each uniform in [1, r) by rejection (a zero is drawn again)
constexpr int ND = 9;
inline void keygen_draws(bool bn, host::Rng& rng, uint32_t out[][8], int nd = ND) {
  for (int k = 0; k < nd; k++) do idgen::draw_below_r(rng, bn, out[k]);
    while (idgen::is_zero8(out[k]));
}

// --------------------------------------------------------------- the writer
// exactly IPK_LEN bytes at out: fields 1..9 in number order, then field 10 = HashToZr of those
// bytes.  pts: HSk, HRand, HAttrs[0..3], BarG1, BarG2 as X || Y; w: four coordinates in the
// proto's order; c, s: 32 bytes each
inline void write_ipk(bool bn, const uint8_t pts[8 * 64], const uint8_t w[128], const uint8_t c[32],
                      const uint8_t s[32], uint8_t* out) {
  idgen::Wr wr{out};
  for (const char* nm : kNames) {
    const size_t l = strlen(nm);
    wr.key(1, 2), wr.byte((uint8_t)l), wr.bytes(reinterpret_cast<const uint8_t*>(nm), l);
  }
  wr.ecp(2, pts), wr.ecp(3, pts + 64);
  for (int a = 0; a < 4; a++) wr.ecp(4, pts + 64 * (2 + a));
  wr.key(5, 2), wr.varint(136);
  for (int q = 0; q < 4; q++) wr.zr(1 + q, w + 32 * q);
  wr.ecp(6, pts + 64 * 6), wr.ecp(7, pts + 64 * 7);
  wr.zr(8, c), wr.zr(9, s);
  uint8_t dg[32], hz[32];
  sha256(out, (size_t)(wr.p - out), dg);
  uint32_t z[8];
  u256::mod_m(dg, 32, bn ? u256::kRbn : u256::kRfbn, z);
  idgen::limbs_to_be32(z, hz);
  wr.zr(10, hz);
}

}  // namespace ipkw
}  // namespace fts
