// Writers of the prover side's wire formats (no HIP, no library state): what a
// generated action hands to fts_request_verify_batch or to a Fabric endorser.
//
//   TransferAction / IssueAction   Action.Serialize (crypto/transfer/action.go:290-323,
//                                  crypto/issue/action.go:192-229) over NewTransfer
//                                  (:127-153) / NewAction (:62-77): proto.Marshal writes
//                                  the fields in number order and omits proto3 empty
//                                  scalars; a non-nil sub-message is written even when
//                                  empty; neither constructor fills the metadata map
//   G1 / Zr                        nogh.G1{raw = 1} / nogh.Zr{raw = 1} over mathlib's JSON
//                                  {"curve":1,"element":"<base64 of Bytes()>"}
//                                  (protos-go/utils/proto.go:22-31)
//   token.Metadata                 Metadata.Serialize (crypto/token/token.go:161-180):
//                                  asn1 TypedToken{2, TokenMetadata{type = 1, value = 2,
//                                  blinding_factor = 3, issuer = 4}}
//
// Every message length is a function of the field lengths alone, so a caller sizes
// (and bounds-checks) its buffers with the *_len functions before any byte is written;
// each write_* returns the end of what it wrote, which is begin + the matching *_len.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../../include/fts_gpu.h"

namespace fts {
namespace host {
namespace aw {

// ---- protobuf wire primitives
inline size_t varint_len(uint64_t v) {
  size_t n = 1;
  while (v >= 0x80) v >>= 7, n++;
  return n;
}
inline uint8_t* put_varint(uint8_t* p, uint64_t v) {
  while (v >= 0x80) *p++ = (uint8_t)(v | 0x80), v >>= 7;
  *p++ = (uint8_t)v;
  return p;
}
// a length-delimited field of a field number below 16: key byte, length, body
inline size_t ld_len(size_t body) { return 1 + varint_len(body) + body; }
inline uint8_t* put_ld_head(uint8_t* p, int field, size_t body) {
  *p++ = (uint8_t)((field << 3) | 2);
  return put_varint(p, body);
}
inline uint8_t* put_ld(uint8_t* p, int field, const uint8_t* b, size_t n) {
  p = put_ld_head(p, field, n);
  if (n) memcpy(p, b, n);
  return p + n;
}
// proto3 bytes / string scalar: an empty value is not written
inline size_t opt_len(size_t n) { return n ? ld_len(n) : 0; }
inline uint8_t* put_opt(uint8_t* p, int field, const uint8_t* b, size_t n) { return n ? put_ld(p, field, b, n) : p; }

// ---- mathlib JSON (G1.MarshalJSON / Zr.MarshalJSON): {"curve":1,"element":"<base64>"}
inline size_t b64_len(size_t n) { return (n + 2) / 3 * 4; }
inline uint8_t* put_b64(uint8_t* p, const uint8_t* b, size_t n) {
  static const char* A = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
  size_t i = 0;
  for (; i + 3 <= n; i += 3) {
    const uint32_t w = ((uint32_t)b[i] << 16) | ((uint32_t)b[i + 1] << 8) | b[i + 2];
    *p++ = A[w >> 18], *p++ = A[(w >> 12) & 63], *p++ = A[(w >> 6) & 63], *p++ = A[w & 63];
  }
  if (n - i == 1) {
    const uint32_t w = (uint32_t)b[i] << 16;
    *p++ = A[w >> 18], *p++ = A[(w >> 12) & 63], *p++ = '=', *p++ = '=';
  } else if (n - i == 2) {
    const uint32_t w = ((uint32_t)b[i] << 16) | ((uint32_t)b[i + 1] << 8);
    *p++ = A[w >> 18], *p++ = A[(w >> 12) & 63], *p++ = A[(w >> 6) & 63], *p++ = '=';
  }
  return p;
}
constexpr size_t JSON_HEAD = 22, JSON_TAIL = 2;  // {"curve":1,"element":"  and  "}
inline size_t json_len(size_t n) { return JSON_HEAD + b64_len(n) + JSON_TAIL; }
inline uint8_t* put_json(uint8_t* p, const uint8_t* b, size_t n) {
  memcpy(p, "{\"curve\":1,\"element\":\"", JSON_HEAD);
  p = put_b64(p + JSON_HEAD, b, n);
  memcpy(p, "\"}", JSON_TAIL);
  return p + JSON_TAIL;
}
// the body of a nogh.G1 (64-byte point) / nogh.Zr (32-byte scalar) message: raw = 1
inline size_t elem_len(size_t n) { return ld_len(json_len(n)); }
inline uint8_t* put_elem(uint8_t* p, const uint8_t* b, size_t n) {
  p = put_ld_head(p, 1, json_len(n));
  return put_json(p, b, n);
}

// ---- nogh.Token{owner = 1, data = 2 G1}
inline size_t token_len(size_t owner_len) { return opt_len(owner_len) + ld_len(elem_len(64)); }
inline uint8_t* put_token(uint8_t* p, const uint8_t* owner, size_t owner_len, const uint8_t* com64) {
  p = put_opt(p, 1, owner, owner_len);
  p = put_ld_head(p, 2, elem_len(64));
  return put_elem(p, com64, 64);
}
// {Transfer,Issue}ActionOutput{token = 1} as repeated field `field` of the action
inline size_t output_len(size_t owner_len) { return ld_len(ld_len(token_len(owner_len))); }
inline uint8_t* put_output(uint8_t* p, int field, const fts_gen_output& o, const uint8_t* com64) {
  const size_t tl = token_len(o.owner_len);
  p = put_ld_head(p, field, ld_len(tl));
  p = put_ld_head(p, 1, tl);
  return put_token(p, o.owner, o.owner_len, com64);
}
// TransferActionInput{token_id = 1 TokenID{tx_id = 1, index = 2}, input = 2 Token}: both
// sub-messages are non-nil, so an empty token id is written as an empty message
inline size_t token_id_len(const fts_gen_input& in) {
  return opt_len(in.tx_id_len) + (in.index ? 1 + varint_len(in.index) : 0);
}
inline size_t input_len(const fts_gen_input& in) {
  return ld_len(ld_len(token_id_len(in)) + ld_len(token_len(in.owner_len)));
}
inline uint8_t* put_input(uint8_t* p, const fts_gen_input& in) {
  const size_t il = token_id_len(in), tl = token_len(in.owner_len);
  p = put_ld_head(p, 1, ld_len(il) + ld_len(tl));
  p = put_ld_head(p, 1, il);
  p = put_opt(p, 1, in.tx_id, in.tx_id_len);
  if (in.index) {
    *p++ = 2 << 3;
    p = put_varint(p, in.index);
  }
  p = put_ld_head(p, 2, tl);
  return put_token(p, in.owner, in.owner_len, in.com64);
}
// Proof{proof = 1} as field `field` (always non-nil)
inline size_t proof_len(size_t n) { return ld_len(opt_len(n)); }
inline uint8_t* put_proof(uint8_t* p, int field, const uint8_t* proof, size_t n) {
  p = put_ld_head(p, field, opt_len(n));
  return put_opt(p, 1, proof, n);
}

// ---- TransferAction{inputs = 1, outputs = 2, proof = 3}; coms: n_out x 64 B
inline size_t transfer_action_len(const fts_gen_action& a, size_t proof_bytes) {
  size_t n = proof_len(proof_bytes);
  for (size_t i = 0; i < a.n_in; i++) n += input_len(a.inputs[i]);
  for (size_t j = 0; j < a.n_out; j++) n += output_len(a.outputs[j].owner_len);
  return n;
}
inline uint8_t* write_transfer_action(uint8_t* p, const fts_gen_action& a, const uint8_t* coms, const uint8_t* proof,
                                      size_t proof_bytes) {
  for (size_t i = 0; i < a.n_in; i++) p = put_input(p, a.inputs[i]);
  for (size_t j = 0; j < a.n_out; j++) p = put_output(p, 2, a.outputs[j], coms + 64 * j);
  return put_proof(p, 3, proof, proof_bytes);
}
// ---- IssueAction{issuer = 1 Identity{raw = 1}, outputs = 3, proof = 4}: NewAction sets no inputs
inline size_t issue_action_len(const fts_gen_action& a, size_t proof_bytes) {
  size_t n = ld_len(opt_len(a.issuer_len)) + proof_len(proof_bytes);
  for (size_t j = 0; j < a.n_out; j++) n += output_len(a.outputs[j].owner_len);
  return n;
}
inline uint8_t* write_issue_action(uint8_t* p, const fts_gen_action& a, const uint8_t* coms, const uint8_t* proof,
                                   size_t proof_bytes) {
  p = put_ld_head(p, 1, opt_len(a.issuer_len));
  p = put_opt(p, 1, a.issuer, a.issuer_len);
  for (size_t j = 0; j < a.n_out; j++) p = put_output(p, 3, a.outputs[j], coms + 64 * j);
  return put_proof(p, 4, proof, proof_bytes);
}

// ---- token.Metadata: DER SEQUENCE{INTEGER 2, OCTET STRING TokenMetadata}
inline size_t der_len_len(size_t n) {
  size_t nb = 0;
  for (size_t v = n; v; v >>= 8) nb++;
  return n < 0x80 ? 1 : 1 + nb;
}
inline uint8_t* put_der_len(uint8_t* p, size_t n) {
  if (n < 0x80) {
    *p++ = (uint8_t)n;
    return p;
  }
  int nb = 0;
  for (size_t v = n; v; v >>= 8) nb++;
  *p++ = (uint8_t)(0x80 | nb);
  for (int i = nb - 1; i >= 0; i--) *p++ = (uint8_t)(n >> (8 * i));
  return p;
}
inline size_t metadata_body_len(size_t type_len, size_t issuer_len) {
  return opt_len(type_len) + 2 * ld_len(elem_len(32)) + ld_len(opt_len(issuer_len));
}
inline size_t metadata_len(size_t type_len, size_t issuer_len) {
  const size_t body = metadata_body_len(type_len, issuer_len), inner = 3 + 1 + der_len_len(body) + body;
  return 1 + der_len_len(inner) + inner;
}
// value: Zr.Bytes() of the uint64; bf32: Zr.Bytes() of the blinding factor
inline uint8_t* write_metadata(uint8_t* p, const uint8_t* type, size_t type_len, uint64_t value, const uint8_t* bf32,
                               const uint8_t* issuer, size_t issuer_len) {
  const size_t body = metadata_body_len(type_len, issuer_len), inner = 3 + 1 + der_len_len(body) + body;
  *p++ = 0x30;
  p = put_der_len(p, inner);
  *p++ = 0x02, *p++ = 0x01, *p++ = 0x02;  // TypedToken.Type = 2 (the zkatdlog token type)
  *p++ = 0x04;
  p = put_der_len(p, body);
  p = put_opt(p, 1, type, type_len);
  uint8_t v32[32] = {0};
  for (int i = 0; i < 8; i++) v32[31 - i] = (uint8_t)(value >> (8 * i));
  p = put_ld_head(p, 2, elem_len(32));
  p = put_elem(p, v32, 32);
  p = put_ld_head(p, 3, elem_len(32));
  p = put_elem(p, bf32, 32);
  p = put_ld_head(p, 4, opt_len(issuer_len));
  return put_opt(p, 1, issuer, issuer_len);
}

}  // namespace aw
}  // namespace host
}  // namespace fts
