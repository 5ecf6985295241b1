// Host side of idemix enrolment (fts_idemix_cred_request_batch, _request_verify_batch,
// fts_idemix_cred_issue_batch): the draws of one item, the parser of the untrusted
// CredRequest{1 nym (ECP), 2 issuer_nonce, 3 proof_c, 4 proof_s} and the writers of that
// proto and of Credential{1 a, 2 b (ECP), 3 e, 4 s, 5 attrs x 4}.  Host only: no HIP call, no
// handle, no global state; lib/credissue_check runs it under the sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../../include/fts_gpu.h"
#include "identity_write.hpp"  // draw_below_r, limbs_to_be32, Wr
#include "pb.hpp"
#include "u256.hpp"

namespace fts {
namespace credis {

// nym 2 + 68, three 32-byte fields 34 each; a, b 70 each, six scalars 34 each
constexpr size_t REQ_LEN = 70 + 3 * 34, CRED_LEN = 2 * 70 + 6 * 34;
static_assert(REQ_LEN == FTS_IDEMIX_CRED_REQUEST_LEN && CRED_LEN == FTS_IDEMIX_CREDENTIAL_LEN, "wire lengths");

// ------------------------------------------------------------------ draws
// (uniform below r by rejection from the item's stream RngSource(seed).at(i), as the other
// signers draw)
// the request: rSk
inline void request_draw(bool bn, host::Rng rng, uint32_t rsk[8]) { idgen::draw_below_r(rng, bn, rsk); }
// the credential: E, then S.  avoid (nullptr: nothing) = r - isk: an E with E + isk = 0 mod r
// has no inverse and is drawn again
inline void issue_draws(bool bn, host::Rng rng, const uint32_t* avoid, uint32_t e[8], uint32_t s[8]) {
  do idgen::draw_below_r(rng, bn, e);
  while (avoid && memcmp(e, avoid, 32) == 0);
  idgen::draw_below_r(rng, bn, s);
}

// ----------------------------------------------------------- the request parser
// -> FTS_OK (to the device: Nym as X || Y, proof_c as sent, proof_c and proof_s mod r, the
// nonce as big-endian words) or FTS_E_CREDREQ_MALFORMED: a NULL or empty input, a proto that
// does not parse, a field of 1..4 with another wire type, a missing field, a scalar or a
// nonce not of 32 bytes, a Nym coordinate not of 32 bytes.  proto3: the last occurrence of a
// field wins; unknown fields and groups are skipped.
struct ReqFields {
  uint8_t nym[64];
  uint32_t c_cmp[8], c_mul[8], s[8], nonce_be[8];
};
inline int32_t parse_request(const uint8_t* req, size_t len, bool bn, ReqFields& r) {
  const uint32_t* rmod = bn ? u256::kRbn : u256::kRfbn;
  memset(&r, 0, sizeof r);
  if (!req || !len) return FTS_E_CREDREQ_MALFORMED;
  Pb pb{req, len};
  Pb::Field d;
  Span f[5];
  while (pb.o < pb.n) {
    if (!pb.next(d)) return FTS_E_CREDREQ_MALFORMED;
    if (d.f >= 1 && d.f <= 4) {
      if (d.wt != 2) return FTS_E_CREDREQ_MALFORMED;
      f[d.f] = Span{d.v, d.vl, true};
    }
  }
  for (int q = 2; q <= 4; q++)
    if (!f[q].set || f[q].n != 32) return FTS_E_CREDREQ_MALFORMED;
  if (!ecp_xy(f[1], r.nym, true)) {
    memset(r.nym, 0, 64);
    return FTS_E_CREDREQ_MALFORMED;
  }
  uint32_t nonce[8];
  u256::be_limbs(f[2].p, 32, nonce);
  for (int k = 0; k < 8; k++) r.nonce_be[k] = nonce[7 - k];
  u256::be_limbs(f[3].p, 32, r.c_cmp);
  u256::mod_m(f[3].p, 32, rmod, r.c_mul);
  u256::mod_m(f[4].p, 32, rmod, r.s);
  return FTS_OK;
}

// --------------------------------------------------------------- the writers
// exactly REQ_LEN bytes at out; every input in the byte order of the wire
inline void write_request(const uint8_t nym_xy[64], const uint8_t nonce[32], const uint8_t c[32], const uint8_t s[32],
                          uint8_t* out) {
  idgen::Wr w{out};
  w.ecp(1, nym_xy);
  w.zr(2, nonce), w.zr(3, c), w.zr(4, s);
}
// exactly CRED_LEN bytes at out
inline void write_credential(const uint8_t a_xy[64], const uint8_t b_xy[64], const uint8_t e[32], const uint8_t s[32],
                             const uint8_t attrs4x32[128], uint8_t* out) {
  idgen::Wr w{out};
  w.ecp(1, a_xy), w.ecp(2, b_xy);
  w.zr(3, e), w.zr(4, s);
  for (int k = 0; k < 4; k++) w.zr(5, attrs4x32 + 32 * k);
}

}  // namespace credis
}  // namespace fts
