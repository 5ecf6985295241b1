// Stand-alone check of enrolment's host side (host/credreq_write.hpp): the CredRequest parser
// on honest and mutated requests, the CredRequest and Credential writers round-tripped, the
// draws.  Built with the host address and undefined-behaviour sanitizers (any report is
// fatal).  No device, no library, no input.  Every buffer handed to the code under test is a
// heap block of exactly its size, so a read or a write past its end is a report.
// Prints "credissue_check: ok" and exits 0 iff every expectation held.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../host/credreq_write.hpp"

using namespace fts;
typedef std::vector<uint8_t> Bytes;

static int g_bad = 0;
#define EXPECT(c)                                                        \
  do {                                                                   \
    if (!(c)) {                                                          \
      fprintf(stderr, "credissue_check: line %d: %s\n", __LINE__, #c);   \
      g_bad++;                                                           \
    }                                                                    \
  } while (0)

// the parser on an exact-size heap copy
static int32_t parse(const Bytes& v, bool bn, credis::ReqFields& f) {
  std::unique_ptr<uint8_t[]> p(new uint8_t[v.size() ? v.size() : 1]);
  if (!v.empty()) memcpy(p.get(), v.data(), v.size());
  return credis::parse_request(v.empty() ? nullptr : p.get(), v.size(), bn, f);
}
static void put_varint(Bytes& o, uint64_t v) {
  while (v > 0x7f) o.push_back((uint8_t)(v | 0x80)), v >>= 7;
  o.push_back((uint8_t)v);
}
static void put_field(Bytes& o, uint32_t f, const Bytes& v) {
  put_varint(o, ((uint64_t)f << 3) | 2);
  put_varint(o, v.size());
  o.insert(o.end(), v.begin(), v.end());
}
static Bytes cat(std::initializer_list<Bytes> parts) {
  Bytes o;
  for (const Bytes& p : parts) o.insert(o.end(), p.begin(), p.end());
  return o;
}
static Bytes fill(size_t n, uint8_t first) {
  Bytes o(n);
  for (size_t i = 0; i < n; i++) o[i] = (uint8_t)(first + 3 * i);
  return o;
}
static Bytes field(uint32_t f, const Bytes& v) {
  Bytes o;
  put_field(o, f, v);
  return o;
}
static void be32(const uint32_t a[8], uint8_t out[32]) { idgen::limbs_to_be32(a, out); }

int main() {
  for (int curve = 0; curve < 2; curve++) {
    const bool bn = curve == 1;
    const uint32_t* r = bn ? u256::kRbn : u256::kRfbn;
    // ---- an honest request through the writer, read back by the parser
    const Bytes x = fill(32, 1), y = fill(32, 7), nonce = fill(32, 0x80), s = fill(32, 0x11);
    Bytes c = fill(32, 0x21);
    c[0] = 0x05;  // below both r
    Bytes nym = cat({x, y});
    std::unique_ptr<uint8_t[]> out(new uint8_t[credis::REQ_LEN]);
    credis::write_request(nym.data(), nonce.data(), c.data(), s.data(), out.get());
    const Bytes honest(out.get(), out.get() + credis::REQ_LEN);
    const Bytes ecp = cat({field(1, x), field(2, y)});
    EXPECT(honest == cat({field(1, ecp), field(2, nonce), field(3, c), field(4, s)}));
    credis::ReqFields f;
    EXPECT(parse(honest, bn, f) == FTS_OK);
    uint8_t b[32];
    EXPECT(memcmp(f.nym, nym.data(), 64) == 0);
    be32(f.c_cmp, b);
    EXPECT(memcmp(b, c.data(), 32) == 0);
    be32(f.c_mul, b);
    EXPECT(memcmp(b, c.data(), 32) == 0);
    {  // s = 0x11.. is below r on FP256BN and reduced on BN254
      uint32_t want[8];
      u256::mod_m(s.data(), 32, r, want);
      EXPECT(memcmp(want, f.s, 32) == 0 && !u256::ge(f.s, r));
    }
    for (int k = 0; k < 8; k++)
      EXPECT(f.nonce_be[k] == (((uint32_t)nonce[4 * k] << 24) | ((uint32_t)nonce[4 * k + 1] << 16) |
                               ((uint32_t)nonce[4 * k + 2] << 8) | nonce[4 * k + 3]));
    // ---- proof_c >= r is kept as sent for the comparison and reduced for the product
    {
      Bytes big(32, 0xff);
      EXPECT(parse(cat({field(1, ecp), field(2, nonce), field(3, big), field(4, big)}), bn, f) == FTS_OK);
      EXPECT(u256::ge(f.c_cmp, r) && !u256::ge(f.c_mul, r) && !u256::ge(f.s, r));
    }
    // ---- every strict prefix: malformed, never a read past the end
    for (size_t n = 0; n < honest.size(); n++) {
      const Bytes pre(honest.begin(), honest.begin() + n);
      EXPECT(parse(pre, bn, f) == FTS_E_CREDREQ_MALFORMED);
    }
    // ---- single-byte corruptions: any verdict, no report
    for (size_t k = 0; k < honest.size(); k++)
      for (int v : {0x00, 0x7f, 0x80, 0xff}) {
        Bytes m = honest;
        m[k] = (uint8_t)v;
        (void)parse(m, bn, f);
      }
    // ---- missing fields, fields of another length, another wire type
    for (uint32_t drop = 1; drop <= 4; drop++) {
      Bytes m;
      const Bytes body[5] = {Bytes(), ecp, nonce, c, s};
      for (uint32_t q = 1; q <= 4; q++)
        if (q != drop) put_field(m, q, body[q]);
      EXPECT(parse(m, bn, f) == FTS_E_CREDREQ_MALFORMED);
    }
    for (size_t len : {(size_t)0, (size_t)31, (size_t)33, (size_t)64, (size_t)300})
      for (uint32_t q = 2; q <= 4; q++) {
        const Bytes body[5] = {Bytes(), ecp, q == 2 ? fill(len, 9) : nonce, q == 3 ? fill(len, 9) : c,
                               q == 4 ? fill(len, 9) : s};
        EXPECT(parse(cat({field(1, body[1]), field(2, body[2]), field(3, body[3]), field(4, body[4])}), bn, f) ==
               FTS_E_CREDREQ_MALFORMED);
      }
    for (size_t len : {(size_t)0, (size_t)31, (size_t)33}) {
      const Bytes e2 = cat({field(1, fill(len, 2)), field(2, y)});
      EXPECT(parse(cat({field(1, e2), field(2, nonce), field(3, c), field(4, s)}), bn, f) == FTS_E_CREDREQ_MALFORMED);
    }
    {
      Bytes m = honest;  // proof_c as a varint field
      Bytes v;
      put_varint(v, (3u << 3) | 0), put_varint(v, 5);
      m.insert(m.end(), v.begin(), v.end());
      EXPECT(parse(m, bn, f) == FTS_E_CREDREQ_MALFORMED);
    }
    // ---- varint overflow in a key and in a length; field 0; wire types 6, 7; a stray end group
    {
      Bytes over(10, 0xff);
      over.push_back(0x01);
      EXPECT(parse(cat({honest, over}), bn, f) == FTS_E_CREDREQ_MALFORMED);
      Bytes len_over = {0x2a};  // field 5, bytes
      len_over.insert(len_over.end(), 9, 0xff);
      len_over.push_back(0x7f);
      EXPECT(parse(cat({honest, len_over}), bn, f) == FTS_E_CREDREQ_MALFORMED);
      EXPECT(parse(cat({honest, Bytes{0x02, 0x00}}), bn, f) == FTS_E_CREDREQ_MALFORMED);
      EXPECT(parse(cat({honest, Bytes{0x2e}}), bn, f) == FTS_E_CREDREQ_MALFORMED);
      EXPECT(parse(cat({honest, Bytes{0x2f}}), bn, f) == FTS_E_CREDREQ_MALFORMED);
      EXPECT(parse(cat({honest, Bytes{0x2c}}), bn, f) == FTS_E_CREDREQ_MALFORMED);
      EXPECT(parse(cat({honest, Bytes{0x2a, 0x05, 0x01}}), bn, f) == FTS_E_CREDREQ_MALFORMED);  // length past the end
    }
    // ---- repeated fields (the last wins), unknown fields of every wire type, a group
    {
      const Bytes c2 = fill(32, 0x02);
      EXPECT(parse(cat({field(3, c2), honest}), bn, f) == FTS_OK);
      be32(f.c_cmp, b);
      EXPECT(memcmp(b, c.data(), 32) == 0);
      EXPECT(parse(cat({honest, field(3, c2)}), bn, f) == FTS_OK);
      be32(f.c_cmp, b);
      EXPECT(memcmp(b, c2.data(), 32) == 0);
      const Bytes unknown = cat({Bytes{0x28, 0x96, 0x01}, Bytes{0x31, 1, 2, 3, 4, 5, 6, 7, 8}, Bytes{0x3d, 1, 2, 3, 4},
                                 field(9, fill(5, 1)), Bytes{0x53, 0x08, 0x01, 0x54}});  // group 10 { 1: 1 }
      EXPECT(parse(cat({unknown, honest, unknown}), bn, f) == FTS_OK);
      EXPECT(memcmp(f.nym, nym.data(), 64) == 0);
      EXPECT(parse(cat({honest, Bytes{0x53, 0x08, 0x01}}), bn, f) == FTS_E_CREDREQ_MALFORMED);        // group never closed
      EXPECT(parse(cat({honest, Bytes{0x53, 0x08, 0x01, 0x5c}}), bn, f) == FTS_E_CREDREQ_MALFORMED);  // closed by field 11
      // a group in place of a known field: the field stays missing
      EXPECT(parse(cat({field(1, ecp), field(2, nonce), Bytes{0x1b, 0x1c}, field(4, s)}), bn, f) ==
             FTS_E_CREDREQ_MALFORMED);
    }
    EXPECT(credis::parse_request(nullptr, 0, bn, f) == FTS_E_CREDREQ_MALFORMED);
    EXPECT(credis::parse_request(nullptr, 5, bn, f) == FTS_E_CREDREQ_MALFORMED);
    // ---- the credential writer: exact size, the layout of the Credential proto
    {
      const Bytes a = cat({fill(32, 3), fill(32, 4)}), bb = cat({fill(32, 5), fill(32, 6)}), e = fill(32, 0x31),
                  ss = fill(32, 0x41), at = fill(128, 0x51);
      std::unique_ptr<uint8_t[]> co(new uint8_t[credis::CRED_LEN]);
      credis::write_credential(a.data(), bb.data(), e.data(), ss.data(), at.data(), co.get());
      Bytes want = cat({field(1, cat({field(1, Bytes(a.begin(), a.begin() + 32)), field(2, Bytes(a.begin() + 32, a.end()))})),
                        field(2, cat({field(1, Bytes(bb.begin(), bb.begin() + 32)), field(2, Bytes(bb.begin() + 32, bb.end()))})),
                        field(3, e), field(4, ss)});
      for (int k = 0; k < 4; k++) put_field(want, 5, Bytes(at.begin() + 32 * k, at.begin() + 32 * k + 32));
      EXPECT(want.size() == credis::CRED_LEN && memcmp(want.data(), co.get(), credis::CRED_LEN) == 0);
      // and it is what the credential parser of the wallet's side reads (values below r)
      Bytes small = want;
      idgen::CredFields cf;
      std::unique_ptr<uint8_t[]> pc(new uint8_t[small.size()]);
      memcpy(pc.get(), small.data(), small.size());
      const bool parsed = idgen::parse_credential(pc.get(), small.size(), bn, cf);
      EXPECT(parsed == !bn);  // 0x31.. >= r on BN254 (r < 2^254), below r on FP256BN
      if (parsed) EXPECT(memcmp(cf.a, a.data(), 64) == 0 && memcmp(cf.b, bb.data(), 64) == 0);
    }
    // ---- draws: deterministic per (seed, i), distinct, below r; the avoided E is drawn again
    for (uint64_t seed : {0ull, 1ull, 77ull, (1ull << 63) + 5}) {
      uint32_t e[8], sd[8], e2[8], s2[8], rs[8];
      credis::issue_draws(bn, host::Rng(seed), nullptr, e, sd);
      credis::issue_draws(bn, host::Rng(seed), nullptr, e2, s2);
      EXPECT(memcmp(e, e2, 32) == 0 && memcmp(sd, s2, 32) == 0 && memcmp(e, sd, 32) != 0);
      EXPECT(!u256::ge(e, r) && !u256::ge(sd, r));
      credis::issue_draws(bn, host::Rng(seed + 1), nullptr, e2, s2);
      EXPECT(memcmp(e, e2, 32) != 0 && memcmp(sd, s2, 32) != 0);
      credis::request_draw(bn, host::Rng(seed), rs);
      EXPECT(memcmp(rs, e, 32) == 0);  // the first value of the item's stream, in either call
      // avoiding the first E: the stream's second value becomes E, its third S
      credis::issue_draws(bn, host::Rng(seed), e, e2, s2);
      EXPECT(memcmp(e2, sd, 32) == 0 && memcmp(s2, sd, 32) != 0 && !u256::ge(s2, r));
    }
  }
  if (g_bad) {
    fprintf(stderr, "credissue_check: %d expectations failed\n", g_bad);
    return 1;
  }
  printf("credissue_check: ok\n");
  return 0;
}
