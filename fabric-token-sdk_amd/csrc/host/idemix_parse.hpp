// The idemix verifiers' parsers of untrusted bytes (nym signatures, serialized
// identities with their association proof, issuer public keys) and the record
// layouts they share with the kernels.  Host only: no HIP include, no handle, no
// global state, no device; lib/idemix_parse_check runs them under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../../include/fts_gpu.h"
#include "pb.hpp"
#include "u256.hpp"

namespace idv {

using fts::Pb;
using fts::Span;

// ------------------------------------------------------- nym signature record
// per-item record (words): c[8] s_sk[8] s_rnym[8] (plain LE limbs, c < r,
// s mod r), nonce[8] (big-endian words, as hashed)
constexpr int NREC = 32;
// nym signing: per-item secrets sk[8] rnym[8] r_sk[8] r_r[8] (canonical LE limbs) nonce[8]
// (big-endian words), and the device's answer c[8] s_sk[8] s_r[8] (canonical LE limbs)
constexpr int NSREC = 40, NSOUT = 24;

// ------------------------------------------------------------ identity record
// bases of the issuer tables: HSk, HRand, HAttrs[0..3], g1
constexpr int NB = 7, B_HSK = 0, B_HRAND = 1, B_HA = 2, B_G1 = 6;
constexpr int NPT = 7;   // raw points per item: nymPK, A', ABar, B', Nym, EidNym, RhNym
constexpr int P_NYMPK = 0, P_AP = 1, P_ABAR = 2, P_BP = 3, P_NYM = 4, P_EID = 5, P_RH = 6;
constexpr int NVAR = 6;  // variable-base products: A' sE, D (-c), B' sR3, Nym (-c), EidNym (-c), RhNym (-c)
constexpr int NFIX = 11;  // distinct fixed-base products (three serve two t-values each)
constexpr int NSC = NVAR + NFIX;
// record words: flags, c (raw LE limbs, compared), nonce (BE words, hashed), scalars
constexpr int R_FLAGS = 0, R_C = 1, R_NONCE = 9, R_SC = 17;
constexpr int REC_WORDS = R_SC + NSC * 8;  // 153
constexpr int REC_STRIDE = 156;            // 16-byte aligned records
static_assert(REC_STRIDE >= REC_WORDS && REC_STRIDE % 4 == 0, "record stride");
// flags (host parse), in the reference's order of checks
constexpr uint32_t F_EARLY_MALFORMED = 1u, F_NO_EID = 2u, F_NO_RH = 4u, F_LATE_MALFORMED = 8u, F_REVOCATION = 16u,
                   F_C_BIG = 32u;

// NymSignature (idemix.proto): 1 proof_c, 2 proof_s_sk, 3 proof_s_r_nym, 4 nonce
// -> record + host verdict (FTS_OK: goes to the device)
inline int32_t parse_nym_sig(const uint8_t* sig, size_t len, bool bn, uint32_t* rec) {
  using namespace fts::u256;
  memset(rec, 0, NREC * 4);
  if (!sig || len == 0) return FTS_E_NYM_MALFORMED;  // "invalid signature, it must not be empty"
  Pb pb{sig, len};
  Pb::Field d;
  Span f[5];
  while (pb.o < pb.n) {
    if (!pb.next(d)) return FTS_E_NYM_MALFORMED;
    if (d.f >= 1 && d.f <= 4) {
      if (d.wt != 2) return FTS_E_NYM_MALFORMED;
      f[d.f] = Span{d.v, d.vl, true};  // proto3: the last occurrence wins
    }
  }
  uint32_t c[8], nonce[8];
  if (bn) {
    // Nonce.Bytes() of a value wider than 32 bytes panics in mathlib BigToBytes
    if (!be_limbs(f[4].p, f[4].n, nonce)) return FTS_E_NYM_MALFORMED;
    mod_m(f[2].p, f[2].n, kRbn, rec + 8);
    mod_m(f[3].p, f[3].n, kRbn, rec + 16);
    for (int k = 0; k < 8; k++) rec[24 + k] = nonce[7 - k];  // big-endian words
    // Zr.Equals compares integers: an unreduced challenge can never match
    if (!be_limbs(f[1].p, f[1].n, c) || ge(c, kRbn)) return FTS_E_NYM_INVALID;
  } else {
    // FP256BN_AMCL Zr from bytes: AMCL FromBytes reads exactly the first 32 bytes
    // (a shorter field makes the Go code index out of range -> FTS_E_NYM_MALFORMED)
    for (int q = 1; q <= 4; q++)
      if (f[q].n < 32) return FTS_E_NYM_MALFORMED;
    be_limbs(f[1].p, 32, c);
    be_limbs(f[4].p, 32, nonce);
    for (int q = 2; q <= 3; q++) {  // s mod r (2^256 < 2 r: one subtraction)
      uint32_t* s = rec + 8 * (q - 1);
      be_limbs(f[q].p, 32, s);
      if (ge(s, kRfbn)) sub(s, kRfbn);
    }
    for (int k = 0; k < 8; k++) rec[24 + k] = nonce[7 - k];
    if (ge(c, kRfbn)) return FTS_E_NYM_INVALID;  // Zr.Equals: an unreduced c never matches
  }
  memcpy(rec, c, 32);
  return FTS_OK;
}

// Staging of one nym item for k_nym_verify / k_nym_sign.  The kernels read the hashed
// stream's tail from HBM as aligned words: BN254 the message alone (the 164-byte prefix
// is whole words, from registers), FP256BN the whole stream
// "sign" || 0x04 || t (64 zero bytes: the device's) || Nym (65) || ipk.Hash || msg.
constexpr size_t NYM_PRE_FBN = 166;
// words of an item's region: its bytes in whole words, zero-filled, and one spare word
inline size_t nym_stream_words(bool bn, size_t msg_len) { return ((bn ? 0 : NYM_PRE_FBN) + msg_len + 3) / 4 + 1; }
// nym_slot (64 bytes) <- X || Y, mw (nym_stream_words words) <- the region, *len <- its
// bytes; false (slot and Nym zeroed): a key of the wrong length or form.  NymPublicKey
// import (crypto/deserializer.go:49-56): BN254 G1.Bytes() raw X || Y (64 B), FP256BN
// ECP.ToBytes 0x04 || X || Y (65 B); the point checks run on the device.
inline bool pack_nym_item(bool bn, const uint8_t* nym, size_t nym_len, const uint8_t ipk_hash[32], const uint8_t* msg,
                          size_t msg_len, uint8_t* nym_slot, uint8_t* mw, uint32_t* len) {
  const size_t pre = bn ? 0 : NYM_PRE_FBN;
  const bool key_ok = nym && (bn ? nym_len == 64 : nym_len == 65 && nym[0] == 0x04);
  if (key_ok) memcpy(nym_slot, nym + (bn ? 0 : 1), 64);
  else memset(nym_slot, 0, 64);
  *len = (uint32_t)(pre + msg_len);
  if (!bn) {
    memcpy(mw, "sign", 4);
    mw[4] = 0x04;
    memset(mw + 5, 0, 64);
    if (key_ok) memcpy(mw + 69, nym, 65);
    else memset(mw + 69, 0, 65);
    memcpy(mw + 134, ipk_hash, 32);
  }
  if (msg_len) memcpy(mw + pre, msg, msg_len);
  memset(mw + pre + msg_len, 0, nym_stream_words(bn, msg_len) * 4 - pre - msg_len);
  return key_ok;
}

// SerializedIdemixIdentity + its Signature proto -> record, raw points, epoch key;
// returns the identity-level status (FTS_OK: to the device)
inline int32_t parse_identity(const uint8_t* id, size_t len, bool bn, uint32_t* rec, uint8_t* pts, uint8_t* epk) {
  using namespace fts::u256;
  const uint32_t* rmod = bn ? kRbn : kRfbn;
  memset(rec, 0, REC_STRIDE * 4);
  memset(pts, 0, NPT * 64);
  memset(epk, 0, 128);
  if (!id || !len) return FTS_E_ID_MALFORMED;  // "empty identity"
  Pb::Field d;
  Span nym, proof;
  {
    Pb pb{id, len};
    while (pb.o < pb.n) {
      if (!pb.next(d)) return FTS_E_ID_MALFORMED;
      if (d.f >= 1 && d.f <= 4 && d.wt != 2) return FTS_E_ID_MALFORMED;
      if (d.f == 1) nym = Span{d.v, d.vl, true};
      if (d.f == 4) proof = Span{d.v, d.vl, true};
    }
  }
  if (nym.n == 0) return FTS_E_ID_MALFORMED;  // "pseudonym's public key is empty"
  // KeyImport: G1.Bytes() form; its point checks run on the device
  if (bn ? nym.n != 64 : (nym.n != 65 || nym.p[0] != 0x04)) return FTS_E_ID_BADNYM;
  memcpy(pts + P_NYMPK * 64, nym.p + (bn ? 0 : 1), 64);
  uint32_t& flags = rec[R_FLAGS];
  // Signature proto (IBM/idemix idemix.proto, restated): 1 a_prime 2 a_bar 3 b_prime (ECP),
  // 4 c 5 s_sk 6 s_e 7 s_r2 8 s_r3 9 s_s_prime, 10 s_attrs (repeated), 11 nonce, 12 nym (ECP),
  // 13 s_r_nym, 14 revocation_epoch_pk (ECP2), 15 revocation_pk_sig, 16 epoch, 17 non_revocation_proof,
  // 18 eid_nym {1 nym, 2 s_eid}, 19 rh_nym {1 nym, 2 s_rh}
  Span f[20];
  std::vector<Span> attrs;
  attrs.reserve(4);
  if (proof.n == 0) {
    flags |= F_EARLY_MALFORMED;  // an empty signature is rejected before Unmarshal
  } else {
    Pb pb{proof.p, proof.n};
    while (pb.o < pb.n) {
      if (!pb.next(d) || (d.f >= 1 && d.f <= 19 && d.f != 16 && d.wt != 2) || (d.f == 16 && d.wt != 0)) {
        flags |= F_EARLY_MALFORMED;
        break;
      }
      if (d.f == 10) attrs.push_back(Span{d.v, d.vl, true});
      else if (d.f >= 1 && d.f <= 19) f[d.f] = Span{d.v, d.vl, true};
    }
  }
  // Zr fields: BN254 big-endian integers of any length; FP256BN AMCL FromBytes reads
  // exactly 32 bytes (a shorter field panics in the reference)
  auto zr = [&](const Span& s, uint32_t out[8]) -> bool {
    if (bn) {
      mod_m(s.p, s.n, rmod, out);
      return true;
    }
    if (s.n < 32) return false;
    be_limbs(s.p, 32, out);
    if (ge(out, rmod)) sub(out, rmod);
    return true;
  };
  uint32_t sc[24][8];
  memset(sc, 0, sizeof sc);
  Span eid_nym, rh_nym, s_eid, s_rh;
  uint32_t rev_alg = 0;
  if (!(flags & F_EARLY_MALFORMED)) {
    // sub-messages: 17 NonRevocationProof{1 revocation_alg}, 18 / 19 {1 nym, 2 s}
    auto nym_msg = [&](const Span& s, Span& a, Span& b) -> bool {
      if (!s.set) return true;
      Pb pb{s.p, s.n};
      while (pb.o < pb.n) {
        if (!pb.next(d)) return false;
        if ((d.f == 1 || d.f == 2) && d.wt != 2) return false;
        if (d.f == 1) a = Span{d.v, d.vl, true};
        if (d.f == 2) b = Span{d.v, d.vl, true};
      }
      return true;
    };
    bool good = nym_msg(f[18], eid_nym, s_eid) && nym_msg(f[19], rh_nym, s_rh);
    if (f[17].set) {
      Pb pb{f[17].p, f[17].n};
      while (good && pb.o < pb.n) {
        if (!pb.next(d)) good = false;
        else if (d.f == 1 && d.wt != 0) good = false;
        else if (d.f == 1) rev_alg = (uint32_t)d.iv;
        else if (d.f == 2 && d.wt != 2) good = false;
      }
    }
    // the scalars: c(4) sSk(5) sE(6) sR2(7) sR3(8) sS'(9) nonce(11) sRNym(13) sAttrs sEid sRh
    const int fld[8] = {4, 5, 6, 7, 8, 9, 11, 13};
    for (int q = 0; q < 8 && good; q++) good = zr(f[fld[q]], sc[q]);
    for (size_t a = 0; a < attrs.size() && good; a++) {
      uint32_t tmp[8];
      good = zr(attrs[a], a < 4 ? sc[8 + a] : tmp);
    }
    if (good && f[18].set) good = zr(s_eid, sc[12]);
    if (good && f[19].set) good = zr(s_rh, sc[13]);
    if (!good) {
      flags |= F_EARLY_MALFORMED;
    } else {
      // nonce: Zr.Bytes() of a value wider than 32 bytes panics (mathlib BigToBytes)
      uint32_t nonce[8];
      if (bn) {
        if (!be_limbs(f[11].p, f[11].n, nonce)) flags |= F_EARLY_MALFORMED;
      } else {
        be_limbs(f[11].p, 32, nonce);
      }
      for (int k = 0; k < 8; k++) rec[R_NONCE + k] = nonce[7 - k];
      // c: compared as an integer with the recomputed (reduced) challenge
      uint32_t craw[8];
      if (!be_limbs(f[4].p, bn ? f[4].n : 32, craw) || ge(craw, rmod)) flags |= F_C_BIG;
      memcpy(rec + R_C, craw, 32);
    }
  }
  if (!(flags & F_EARLY_MALFORMED)) {
    if (!f[18].set) flags |= F_NO_EID;
    else if (!f[19].set) flags |= F_NO_RH;
  }
  if (!(flags & (F_EARLY_MALFORMED | F_NO_EID | F_NO_RH))) {
    bool good = ecp_xy(f[1], pts + P_AP * 64, true) && ecp_xy(f[2], pts + P_ABAR * 64, true) &&
                ecp_xy(f[3], pts + P_BP * 64, true) && ecp_xy(f[12], pts + P_NYM * 64, true) &&
                ecp_xy(eid_nym, pts + P_EID * 64, true) && ecp_xy(rh_nym, pts + P_RH * 64, true) &&
                attrs.size() == 4 && ecp2_raw(f[14], epk);
    if (!good) flags |= F_LATE_MALFORMED;
    if (rev_alg != 0) flags |= F_REVOCATION;
    // scalars: var [sE, -c, sR3, -c, -c, -c]; fixed as FIX_B / FIX_T
    uint32_t cm[8], nc[8];
    memcpy(cm, sc[0], 32);
    memset(nc, 0, 32);
    uint32_t z = 0;
    for (int k = 0; k < 8; k++) z |= cm[k];
    if (z) {
      memcpy(nc, rmod, 32);
      sub(nc, cm);
    }
    const uint32_t* var[NVAR] = {sc[2], nc, sc[4], nc, nc, nc};
    // fixed: sR2, sS', sSk (t2, t3), sA0, sA1, sA2 (t2, t4), sA3 (t2, t5), c, sRNym, sEid, sRh
    const uint32_t* fix[NFIX] = {sc[3], sc[5], sc[1], sc[8], sc[9], sc[10], sc[11], cm, sc[7], sc[12], sc[13]};
    for (int v = 0; v < NVAR; v++) memcpy(rec + R_SC + v * 8, var[v], 32);
    for (int q = 0; q < NFIX; q++) memcpy(rec + R_SC + (NVAR + q) * 8, fix[q], 32);
  }
  return FTS_OK;
}

// ------------------------------------------------------- audit info matching
// AuditInfo.Match (idemix/crypto/audit.go:40-84) reads an identity far more loosely
// than Signature.Ver: proto.Unmarshal of SerializedIdemixIdentity and of its whole
// Signature (embedded messages included), then only EidNym.Nym and RhNym.Nym.  No
// scalar is parsed, no other point decoded, the nym public key never read -- so none
// of parse_identity's scalar or point rules apply here.
namespace audit_wire {
// every field of an embedded message on the wire, the known ones with their wire type:
// `bytes_lo..bytes_hi` length-delimited, `varint_f` (0: none) a varint
inline bool msg_ok(const Span& s, uint32_t bytes_lo, uint32_t bytes_hi, uint32_t varint_f) {
  Pb pb{s.p, s.n};
  Pb::Field d;
  while (pb.o < pb.n) {
    if (!pb.next(d)) return false;
    if (d.f >= bytes_lo && d.f <= bytes_hi && d.wt != 2) return false;
    if (varint_f && d.f == varint_f && d.wt != 0) return false;
  }
  return true;
}
// a merged ECP{1 x, 2 y}: proto3 merges the occurrences of an embedded message, the
// last x and the last y win
struct Ecp {
  Span x, y;
  bool set = false;  // the message field was seen (a non-nil *ECP)
  bool merge(const Span& s) {
    set = true;
    Pb pb{s.p, s.n};
    Pb::Field d;
    while (pb.o < pb.n) {
      if (!pb.next(d)) return false;
      if ((d.f == 1 || d.f == 2) && d.wt != 2) return false;
      if (d.f == 1) x = Span{d.v, d.vl, true};
      if (d.f == 2) y = Span{d.v, d.vl, true};
    }
    return true;
  }
  // G1FromProto's length rule (its canonical / on-curve rules run on the device)
  bool raw(uint8_t out[64]) const {
    if (x.n != 32 || y.n != 32) return false;
    memcpy(out, x.p, 32);
    memcpy(out + 32, y.p, 32);
    return true;
  }
};
// EidNym / RhNym {1 nym (ECP), 2 proof_s}: one occurrence merged into `nym`
inline bool nym_merge(const Span& s, Ecp& nym) {
  Pb pb{s.p, s.n};
  Pb::Field d;
  while (pb.o < pb.n) {
    if (!pb.next(d)) return false;
    if ((d.f == 1 || d.f == 2) && d.wt != 2) return false;
    if (d.f == 1 && !nym.merge(Span{d.v, d.vl, true})) return false;
  }
  return true;
}
}  // namespace audit_wire

// SerializedIdemixIdentity -> the status known before the device and the raw EidNym /
// RhNym points (64 bytes each, zeroed unless the call returns FTS_OK and, for rh_pt,
// rh_pre is FTS_OK too).  Returns FTS_OK, FTS_E_AUDIT_MALFORMED, FTS_E_AUDIT_NO_EIDNYM
// or FTS_E_AUDIT_EID_POINT (a coordinate that is not 32 bytes); these end the match.
// rh_pre <- FTS_OK, FTS_E_AUDIT_NO_RHNYM or FTS_E_AUDIT_RH_POINT: the RH half's verdict
// as far as the host knows it, which counts only after the EID half has passed on the
// device (all EID checks precede all RH checks).  No allocation.
inline int32_t parse_audit_identity(const uint8_t* id, size_t len, bool bn, uint8_t eid_pt[64], uint8_t rh_pt[64],
                                    int32_t& rh_pre) {
  using namespace audit_wire;
  (void)bn;  // the wire rules are the same on both curves; the point rules differ on the device
  memset(eid_pt, 0, 64);
  memset(rh_pt, 0, 64);
  rh_pre = FTS_OK;
  if (!id) return FTS_E_AUDIT_MALFORMED;
  Pb::Field d;
  Span proof;
  {
    Pb pb{id, len};
    while (pb.o < pb.n) {
      if (!pb.next(d)) return FTS_E_AUDIT_MALFORMED;
      if (d.f >= 1 && d.f <= 4 && d.wt != 2) return FTS_E_AUDIT_MALFORMED;
      if (d.f == 4) proof = Span{d.v, d.vl, true};
    }
  }
  if (proof.n == 0) return FTS_E_AUDIT_MALFORMED;  // "invalid signature, it must not be empty"
  // Signature (field numbers as in parse_identity): 1 2 3 12 ECP, 14 ECP2 {1..4},
  // 17 NonRevocationProof {1 revocation_alg (varint), 2 non_revocation_proof}, 18 19 the
  // nyms, 16 epoch (varint), every other field up to 19 bytes
  Ecp eid, rh;
  Pb pb{proof.p, proof.n};
  while (pb.o < pb.n) {
    if (!pb.next(d) || (d.f >= 1 && d.f <= 19 && d.f != 16 && d.wt != 2) || (d.f == 16 && d.wt != 0))
      return FTS_E_AUDIT_MALFORMED;
    const Span s{d.v, d.vl, true};
    bool ok = true;
    switch (d.f) {
      case 1: case 2: case 3: case 12: ok = msg_ok(s, 1, 2, 0); break;
      case 14: ok = msg_ok(s, 1, 4, 0); break;
      case 17: ok = msg_ok(s, 2, 2, 1); break;
      case 18: ok = nym_merge(s, eid); break;
      case 19: ok = nym_merge(s, rh); break;
      default: break;
    }
    if (!ok) return FTS_E_AUDIT_MALFORMED;
  }
  if (!eid.set) return FTS_E_AUDIT_NO_EIDNYM;  // sig.EidNym == nil || sig.EidNym.Nym == nil
  if (!eid.raw(eid_pt)) return FTS_E_AUDIT_EID_POINT;
  if (!rh.set) rh_pre = FTS_E_AUDIT_NO_RHNYM;
  else if (!rh.raw(rh_pt)) rh_pre = FTS_E_AUDIT_RH_POINT;
  return FTS_OK;
}

// IssuerPublicKey: 2 h_sk, 3 h_rand, 4 h_attrs (repeated ECP), 5 w (ECP2), 6 bar_g1, 7 bar_g2
// (ECP; an issuer handle checks its secret against them), 10 hash;
// a field with another wire type is ignored.  false: proto.Unmarshal fails.  Each
// creator applies its own acceptance rule to the spans.
struct IpkFields {
  Span h_sk, h_rand, h_attrs[4], w, bar_g1, bar_g2, hash;
  size_t n_attrs = 0;  // occurrences of field 4 (the first four are kept)
};
inline bool parse_ipk(const uint8_t* ipk, size_t len, IpkFields& k) {
  Pb pb{ipk, len};
  Pb::Field d;
  while (pb.o < pb.n) {
    if (!pb.next(d)) return false;
    if (d.wt != 2) continue;
    const Span s{d.v, d.vl, true};
    if (d.f == 2) k.h_sk = s;
    if (d.f == 3) k.h_rand = s;
    if (d.f == 4 && k.n_attrs++ < 4) k.h_attrs[k.n_attrs - 1] = s;
    if (d.f == 5) k.w = s;
    if (d.f == 6) k.bar_g1 = s;
    if (d.f == 7) k.bar_g2 = s;
    if (d.f == 10) k.hash = s;
  }
  return true;
}
// ipk.Hash as hashed: copy(proofData[index:], ipk.Hash) into a FieldBytes window
inline void ipk_hash32(const IpkFields& k, uint8_t h[32]) {
  memset(h, 0, 32);
  if (k.hash.set) memcpy(h, k.hash.p, k.hash.n < 32 ? k.hash.n : 32);
}

}  // namespace idv
