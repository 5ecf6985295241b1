// Stand-alone check of the issuer-key calls' host side (host/ipk_write.hpp): the check's
// reading of an IssuerPublicKey on honest keys and their mutations (truncations at every length,
// length-field overflows, repeated and missing fields, 31- and 33-byte coordinates), the hash
// over the key without field 10, the draws and the writer of a new key.  Built with the host
// address and undefined-behaviour sanitizers (any report is fatal).  No device, no library.
// Every buffer handed to the code under test is a heap block of exactly its size, so a read or
// a write past its end is a report.
//   ipk_check (bn254|fp256bn):<IssuerPublicKey file> ...
// Prints "ipk_check: ok" and exits 0 iff every expectation held.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../host/ipk_write.hpp"

using namespace fts;
typedef std::vector<uint8_t> Bytes;

static int g_bad = 0;
#define EXPECT(c)                                                  \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "ipk_check: line %d: %s\n", __LINE__, #c);   \
      g_bad++;                                                     \
    }                                                              \
  } while (0)

// an exact-size heap copy (one byte for an empty input, never read)
struct Exact {
  std::unique_ptr<uint8_t[]> p;
  size_t n;
  explicit Exact(const Bytes& v) : p(new uint8_t[v.size() ? v.size() : 1]), n(v.size()) {
    if (n) memcpy(p.get(), v.data(), n);
  }
};
static int32_t parse(const Bytes& v, bool bn, ipkw::CheckFields& f) {
  const Exact e(v);
  return ipkw::parse_for_check(v.empty() ? nullptr : e.p.get(), e.n, bn, f);
}
static bool hash(const Bytes& v, bool bn, uint8_t out[32]) {
  const Exact e(v);
  return ipkw::hash_without_field10(e.p.get(), e.n, bn, out);
}
static bool attrs(const Bytes& v, size_t cap, Bytes& out) {
  const Exact e(v);
  std::unique_ptr<uint8_t[]> o(new uint8_t[cap ? cap * 64 : 1]);
  const bool ok = ipkw::hattrs(e.p.get(), e.n, o.get(), cap);
  out.assign(o.get(), o.get() + cap * 64);
  return ok;
}
static void put_varint(Bytes& o, uint64_t v) {
  while (v > 0x7f) o.push_back((uint8_t)(v | 0x80)), v >>= 7;
  o.push_back((uint8_t)v);
}
static Bytes field(uint32_t f, const Bytes& v) {
  Bytes o;
  put_varint(o, ((uint64_t)f << 3) | 2);
  put_varint(o, v.size());
  o.insert(o.end(), v.begin(), v.end());
  return o;
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
// the top-level fields of a well-formed proto: (number, the field's bytes with key and length)
static std::vector<std::pair<uint32_t, Bytes>> split(const Bytes& v) {
  std::vector<std::pair<uint32_t, Bytes>> out;
  Pb pb{v.data(), v.size()};
  Pb::Field d;
  while (pb.o < pb.n) {
    const size_t at = pb.o;
    if (!pb.next(d)) break;
    out.emplace_back(d.f, Bytes(v.begin() + at, v.begin() + pb.o));
  }
  return out;
}
static Bytes join(const std::vector<std::pair<uint32_t, Bytes>>& fs) {
  Bytes o;
  for (const auto& f : fs) o.insert(o.end(), f.second.begin(), f.second.end());
  return o;
}
// the value of a length-delimited field written by field()
static Bytes value_of(const Bytes& fld) {
  Pb pb{fld.data(), fld.size()};
  Pb::Field d;
  if (!pb.next(d)) return Bytes();
  return Bytes(d.v, d.v + d.vl);
}

static void check_key(const Bytes& honest, bool bn) {
  const uint32_t* r = bn ? u256::kRbn : u256::kRfbn;
  ipkw::CheckFields f;
  uint8_t h[32], b[32];
  const auto fs = split(honest);
  EXPECT(join(fs) == honest);
  // ---- the honest key: accepted, its stored hash is the hash of the rest
  EXPECT(parse(honest, bn, f) == FTS_OK);
  EXPECT(f.n_attrs == f.n_names && f.n_names > 0);
  EXPECT(!u256::ge(f.s, r) && !u256::ge(f.neg_c, r) && !u256::ge(f.c_cmp, r));
  {  // c + (-c) = 0 mod r
    uint32_t sum[8];
    uint64_t cy = 0;
    for (int k = 0; k < 8; k++) {
      const uint64_t v = (uint64_t)f.c_cmp[k] + f.neg_c[k] + cy;
      sum[k] = (uint32_t)v, cy = v >> 32;
    }
    EXPECT(cy == 0 && memcmp(sum, r, 32) == 0);
  }
  Bytes stored, at;
  size_t hash_at = 0, off = 0;
  for (const auto& x : fs) {
    if (x.first == 10) stored = value_of(x.second), hash_at = off;
    off += x.second.size();
  }
  EXPECT(stored.size() == 32 && hash_at + 34 == honest.size());
  EXPECT(hash(honest, bn, h) && stored.size() == 32 && memcmp(h, stored.data(), 32) == 0);
  EXPECT(attrs(honest, f.n_attrs, at));
  EXPECT(!attrs(honest, f.n_attrs - 1, at) && !attrs(honest, f.n_attrs + 1, at));
  const size_t n_attrs = f.n_attrs;
  // ---- every strict prefix: never accepted before ProofS is whole, never a read past the end
  for (size_t n = 0; n < honest.size(); n++) {
    const Bytes pre(honest.begin(), honest.begin() + n);
    const int32_t st = parse(pre, bn, f);
    EXPECT(st == (n == hash_at ? FTS_OK : st));
    if (n < hash_at) EXPECT(st == FTS_E_IPK_MALFORMED || st == FTS_E_IPK_UNDEFINED);
    if (n == 0) EXPECT(st == FTS_E_IPK_MALFORMED);
    (void)hash(pre, bn, h);
    (void)attrs(pre, n_attrs, at);
  }
  // ---- single-byte corruptions: any verdict, no report
  for (size_t k = 0; k < honest.size(); k++)
    for (int v : {0x00, 0x7f, 0x80, 0xff}) {
      Bytes m = honest;
      m[k] = (uint8_t)v;
      if (parse(m, bn, f) == FTS_OK) (void)attrs(m, f.n_attrs, at);
      (void)hash(m, bn, h);
    }
  // ---- length-field and key overflows, field 0, wire types 6 and 7, a stray end group
  {
    Bytes over(10, 0xff);
    over.push_back(0x01);
    EXPECT(parse(cat({honest, over}), bn, f) == FTS_E_IPK_MALFORMED);
    Bytes len_over = {0x5a};  // field 11, bytes
    len_over.insert(len_over.end(), 9, 0xff);
    len_over.push_back(0x7f);
    EXPECT(parse(cat({honest, len_over}), bn, f) == FTS_E_IPK_MALFORMED);
    EXPECT(!hash(cat({honest, len_over}), bn, h));
    EXPECT(parse(cat({honest, Bytes{0x5a, 0x05, 0x01}}), bn, f) == FTS_E_IPK_MALFORMED);  // length past the end
    EXPECT(parse(cat({honest, Bytes{0x02, 0x00}}), bn, f) == FTS_E_IPK_MALFORMED);
    EXPECT(parse(cat({honest, Bytes{0x5e}}), bn, f) == FTS_E_IPK_MALFORMED);
    EXPECT(parse(cat({honest, Bytes{0x5f}}), bn, f) == FTS_E_IPK_MALFORMED);
    EXPECT(parse(cat({honest, Bytes{0x5c}}), bn, f) == FTS_E_IPK_MALFORMED);
    // an overflowing length inside W: the ECP2 does not parse
    auto g = fs;
    for (auto& x : g)
      if (x.first == 5) x.second = field(5, cat({Bytes{0x0a, 0xff, 0xff, 0xff, 0xff, 0x0f}, fill(8, 1)}));
    EXPECT(parse(join(g), bn, f) == FTS_E_IPK_MALFORMED);
  }
  // ---- repeated fields: the last ProofC wins, a further HAttrs counts, unknown fields are skipped
  {
    const Bytes c2 = fill(32, 0x02);
    EXPECT(parse(cat({honest, field(8, c2)}), bn, f) == FTS_OK);
    idgen::limbs_to_be32(f.c_cmp, b);
    EXPECT(memcmp(b, c2.data(), 32) == 0);
    EXPECT(parse(cat({field(8, c2), honest}), bn, f) == FTS_OK);
    idgen::limbs_to_be32(f.c_cmp, b);
    EXPECT(memcmp(b, c2.data(), 32) != 0);
    const Bytes ecp = cat({field(1, fill(32, 5)), field(2, fill(32, 9))});
    const Bytes more = cat({honest, field(4, ecp)});
    EXPECT(parse(more, bn, f) == FTS_OK && f.n_attrs == n_attrs + 1);
    EXPECT(attrs(more, n_attrs + 1, at) && memcmp(at.data() + 64 * n_attrs, fill(32, 5).data(), 32) == 0);
    const Bytes unknown = cat({Bytes{0x58, 0x96, 0x01}, Bytes{0x61, 1, 2, 3, 4, 5, 6, 7, 8}, Bytes{0x6d, 1, 2, 3, 4},
                               field(14, fill(5, 1)), Bytes{0x7b, 0x08, 0x01, 0x7c}});  // group 15 { 1: 1 }
    EXPECT(parse(cat({unknown, honest, unknown}), bn, f) == FTS_OK && f.n_attrs == n_attrs);
    EXPECT(parse(cat({honest, Bytes{0x7b, 0x08, 0x01}}), bn, f) == FTS_E_IPK_MALFORMED);  // group never closed
    // ProofS as a varint field: ignored, so the earlier one stands
    EXPECT(parse(cat({honest, Bytes{0x48, 0x05}}), bn, f) == FTS_OK);
  }
  // ---- missing fields
  for (uint32_t drop : {2u, 3u, 5u, 6u, 7u, 8u, 9u}) {
    auto g = fs;
    for (size_t k = 0; k < g.size(); k++)
      if (g[k].first == drop) g.erase(g.begin() + k--);
    EXPECT(parse(join(g), bn, f) == FTS_E_IPK_UNDEFINED);
  }
  {
    auto g = fs;  // one HAttrs fewer than names
    for (size_t k = 0; k < g.size(); k++)
      if (g[k].first == 4) {
        g.erase(g.begin() + k);
        break;
      }
    EXPECT(parse(join(g), bn, f) == FTS_E_IPK_UNDEFINED);
    g = fs;  // no names at all: nothing is required of HAttrs
    for (size_t k = 0; k < g.size(); k++)
      if (g[k].first == 1 || g[k].first == 4) g.erase(g.begin() + k--);
    EXPECT(parse(join(g), bn, f) == FTS_OK && f.n_attrs == 0 && f.n_names == 0);
    EXPECT(attrs(join(g), 0, at));
  }
  // ---- 31- and 33-byte coordinates and proof values
  for (size_t len : {(size_t)0, (size_t)31, (size_t)33}) {
    const Bytes ecp = cat({field(1, fill(len, 2)), field(2, fill(32, 3))});
    const Bytes ecp2 = cat({field(1, fill(32, 2)), field(2, fill(32, 3)), field(3, fill(len, 4)), field(4, fill(32, 5))});
    for (uint32_t q : {2u, 3u, 5u, 6u, 7u, 8u, 9u}) {
      auto g = fs;
      for (auto& x : g)
        if (x.first == q) x.second = field(q, q == 5 ? ecp2 : q >= 8 ? fill(len, 7) : ecp);
      EXPECT(parse(join(g), bn, f) == FTS_E_IPK_MALFORMED);
    }
    auto g = fs;  // an HAttrs: found when the points are collected
    for (auto& x : g)
      if (x.first == 4) {
        x.second = field(4, ecp);
        break;
      }
    EXPECT(parse(join(g), bn, f) == FTS_OK && !attrs(join(g), f.n_attrs, at));
  }
  // ---- ProofC and ProofS at and above r: kept as sent for the comparison, reduced for the products
  {
    const Bytes big(32, 0xff);
    auto g = fs;
    for (auto& x : g)
      if (x.first == 8 || x.first == 9) x.second = field(x.first, big);
    EXPECT(parse(join(g), bn, f) == FTS_OK);
    EXPECT(u256::ge(f.c_cmp, r) && !u256::ge(f.s, r) && !u256::ge(f.neg_c, r));
  }
  EXPECT(ipkw::parse_for_check(nullptr, 0, bn, f) == FTS_E_IPK_MALFORMED);
  EXPECT(ipkw::parse_for_check(nullptr, 5, bn, f) == FTS_E_IPK_MALFORMED);
}

static void check_writer(bool bn) {
  const uint32_t* r = bn ? u256::kRbn : u256::kRfbn;
  const Bytes pts = fill(8 * 64, 0x11), w = fill(128, 0x21), s = fill(32, 0x41);
  Bytes c = fill(32, 0x31);
  c[0] = 0x05;  // below both r
  std::unique_ptr<uint8_t[]> out(new uint8_t[ipkw::IPK_LEN]);
  ipkw::write_ipk(bn, pts.data(), w.data(), c.data(), s.data(), out.get());
  const Bytes key(out.get(), out.get() + ipkw::IPK_LEN);
  auto ecp = [&](int k) {
    return cat({field(1, Bytes(pts.begin() + 64 * k, pts.begin() + 64 * k + 32)),
                field(2, Bytes(pts.begin() + 64 * k + 32, pts.begin() + 64 * k + 64))});
  };
  Bytes want;
  for (const char* nm : ipkw::kNames) {
    const std::string sn(nm);
    const Bytes fb = field(1, Bytes(sn.begin(), sn.end()));
    want.insert(want.end(), fb.begin(), fb.end());
  }
  Bytes ecp2;
  for (int q = 0; q < 4; q++) {
    const Bytes fb = field(1 + q, Bytes(w.begin() + 32 * q, w.begin() + 32 * q + 32));
    ecp2.insert(ecp2.end(), fb.begin(), fb.end());
  }
  want = cat({want, field(2, ecp(0)), field(3, ecp(1)), field(4, ecp(2)), field(4, ecp(3)), field(4, ecp(4)),
              field(4, ecp(5)), field(5, ecp2), field(6, ecp(6)), field(7, ecp(7)), field(8, c), field(9, s)});
  EXPECT(want.size() + 34 == ipkw::IPK_LEN);
  EXPECT(key.size() >= want.size() && memcmp(key.data(), want.data(), want.size()) == 0);
  // field 10 is the hash of the rest, and the check's reading takes the key back
  uint8_t h[32], b[32];
  EXPECT(hash(key, bn, h));
  EXPECT(key[want.size()] == 0x52 && key[want.size() + 1] == 32 && memcmp(key.data() + want.size() + 2, h, 32) == 0);
  EXPECT(hash(want, bn, b) && memcmp(h, b, 32) == 0);
  ipkw::CheckFields f;
  EXPECT(parse(key, bn, f) == FTS_OK && f.n_names == 4 && f.n_attrs == 4);
  EXPECT(memcmp(f.h_sk, pts.data(), 64) == 0 && memcmp(f.h_rand, pts.data() + 64, 64) == 0);
  EXPECT(memcmp(f.bar, pts.data() + 6 * 64, 128) == 0 && memcmp(f.w, w.data(), 128) == 0);
  idgen::limbs_to_be32(f.c_cmp, b);
  EXPECT(memcmp(b, c.data(), 32) == 0);
  Bytes at;
  EXPECT(attrs(key, 4, at) && memcmp(at.data(), pts.data() + 2 * 64, 4 * 64) == 0);
  // ---- draws: in [1, r), deterministic per (seed, i), distinct between neighbours
  for (uint64_t seed : {0ull, 1ull, 77ull, (1ull << 63) + 5}) {
    uint32_t d1[ipkw::ND][8], d2[ipkw::ND][8], d3[ipkw::ND][8];
    host::Rng r1(seed), r2(seed), r3(seed + 1);
    ipkw::keygen_draws(bn, r1, d1);
    ipkw::keygen_draws(bn, r2, d2);
    ipkw::keygen_draws(bn, r3, d3);
    EXPECT(memcmp(d1, d2, sizeof d1) == 0);
    for (int k = 0; k < ipkw::ND; k++) {
      EXPECT(!u256::ge(d1[k], r) && !idgen::is_zero8(d1[k]) && memcmp(d1[k], d3[k], 32) != 0);
      for (int j = 0; j < k; j++) EXPECT(memcmp(d1[k], d1[j], 32) != 0);
    }
  }
}

int main(int argc, char** argv) {
  int keys = 0;
  for (int a = 1; a < argc; a++) {
    const std::string arg(argv[a]);
    const size_t colon = arg.find(':');
    const std::string tag = arg.substr(0, colon == std::string::npos ? 0 : colon);
    if (tag != "bn254" && tag != "fp256bn") {
      fprintf(stderr, "ipk_check: argument %d is not (bn254|fp256bn):<file>\n", a);
      return 2;
    }
    std::ifstream in(arg.substr(colon + 1), std::ios::binary);
    const Bytes raw((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    if (!in || raw.empty()) {
      fprintf(stderr, "ipk_check: cannot read %s\n", arg.c_str() + colon + 1);
      return 2;
    }
    check_key(raw, tag == "bn254");
    keys++;
  }
  for (int curve = 0; curve < 2; curve++) {
    check_writer(curve == 1);
    // a written key goes through the same mutations as the fixtures
    const Bytes pts = fill(8 * 64, 0x11), w = fill(128, 0x21), c = fill(32, 0x05), s = fill(32, 0x41);
    std::unique_ptr<uint8_t[]> out(new uint8_t[ipkw::IPK_LEN]);
    ipkw::write_ipk(curve == 1, pts.data(), w.data(), c.data(), s.data(), out.get());
    check_key(Bytes(out.get(), out.get() + ipkw::IPK_LEN), curve == 1);
  }
  if (g_bad) {
    fprintf(stderr, "ipk_check: %d expectations failed\n", g_bad);
    return 1;
  }
  printf("ipk_check: ok (%d fixture keys)\n", keys);
  return 0;
}
