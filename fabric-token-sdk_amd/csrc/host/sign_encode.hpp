// Encoders of the signing entry points (host only): the DER form of an ECDSA
// signature as utils.MarshalECDSASignature writes it (validator/ecdsa/ecdsa.go:49-63
// returns it from Signer.Sign), and the idemix NymSignature proto.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace fts {
namespace host {

constexpr size_t ECDSA_SIG_MAX = 72;  // 30 46 (02 21 00 r) (02 21 00 s)
constexpr size_t NYM_SIG_LEN = 136;   // four fields of key, length 32, 32 bytes

// minimal DER INTEGER (tag, length, two's complement) of a 32-byte big-endian
// magnitude -> bytes written (3..35)
inline size_t der_uint256(const uint8_t v[32], uint8_t* out) {
  size_t st = 0;
  while (st < 31 && v[st] == 0) st++;
  const size_t pad = (v[st] & 0x80) ? 1 : 0, len = 32 - st + pad;
  out[0] = 0x02;
  out[1] = (uint8_t)len;
  if (pad) out[2] = 0x00;
  memcpy(out + 2 + pad, v + st, 32 - st);
  return 2 + len;
}

// SEQUENCE { INTEGER r, INTEGER s } -> bytes written (8..72)
inline uint32_t ecdsa_sig_der(const uint8_t r32[32], const uint8_t s32[32], uint8_t out[ECDSA_SIG_MAX]) {
  uint8_t body[70];
  size_t n = der_uint256(r32, body);
  n += der_uint256(s32, body + n);
  out[0] = 0x30;
  out[1] = (uint8_t)n;  // <= 70: the short length form
  memcpy(out + 2, body, n);
  return (uint32_t)(2 + n);
}

// NymSignature{1 proof_c, 2 proof_s_sk, 3 proof_s_r_nym, 4 nonce}, each Zr.Bytes()
// (32 bytes big-endian)
inline void nym_sig_proto(const uint8_t c[32], const uint8_t s_sk[32], const uint8_t s_r[32], const uint8_t nonce[32],
                          uint8_t out[NYM_SIG_LEN]) {
  const uint8_t* const f[4] = {c, s_sk, s_r, nonce};
  for (int k = 0; k < 4; k++) {
    out[34 * k] = (uint8_t)(((k + 1) << 3) | 2);
    out[34 * k + 1] = 32;
    memcpy(out + 34 * k + 2, f[k], 32);
  }
}

}  // namespace host
}  // namespace fts
