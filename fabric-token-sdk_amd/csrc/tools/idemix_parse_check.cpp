// Stand-alone check of host/idemix_parse.hpp (over host/pb.hpp and host/u256.hpp),
// the idemix verifiers' parsers of untrusted bytes, built with the host address and
// undefined-behaviour sanitizers (any report is fatal).  No device, no library.
// Every input lives in a heap block of exactly its length and every output (record,
// points, epoch key) in a block of exactly its size, so a read or write past either
// is a report.  Each input is parsed as it is, as every strict prefix, with every
// byte flipped two ways (^0x01, ^0x80; every 16th byte for the `tile` identities)
// and in the null / zero-length forms.
//   idemix_parse_check <file of lines: kind curve hex [honest|tile]>
//     kind: id | nym | ipk | audit; curve: bn254 | fp256bn; honest, tile: an honest golden case
//     (audit: an identity read by parse_audit_identity, the audit-info matcher's parser)
//   first checks the nym items' staging (check_pack) and prints "pack <cases> cases";
//   prints "audit <input index> <pre> <rh_pre>" for every audit input as given, then a
//   SHA-256 over every output of the run; exit status 0 iff every check holds
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../common/sha256.hpp"
#include "../host/idemix_parse.hpp"

using namespace idv;
using fts::Sha256;

static std::atomic<int> g_failed{0};
#define CHECK(x)                                                                                \
  do {                                                                                          \
    if (!(x)) {                                                                                 \
      if (g_failed++ < 20) fprintf(stderr, "idemix_parse_check: %s (line %d)\n", #x, __LINE__); \
    }                                                                                           \
  } while (0)

enum Kind { ID, NYM, IPK, AUDIT };
struct Input {
  Kind kind;
  bool bn, honest, tile;
  std::string bytes;
};
struct Result {
  uint8_t digest[32];
  size_t calls = 0;
  int32_t pre = 0, rh_pre = 0;  // audit: the statuses of the input as given
};

static void put32(Sha256& h, uint32_t v) {
  const uint8_t b[4] = {(uint8_t)v, (uint8_t)(v >> 8), (uint8_t)(v >> 16), (uint8_t)(v >> 24)};
  h.update(b, 4);
}

// ---- one call of each parser over exactly-sized blocks, its outputs hashed
// (p == nullptr: the null form)
static std::unique_ptr<uint8_t[]> exact(const uint8_t* p, size_t len) {
  std::unique_ptr<uint8_t[]> b(new uint8_t[len]);
  if (len) memcpy(b.get(), p, len);
  return b;
}
static int32_t run_id(const uint8_t* p, size_t len, bool null, bool bn, uint32_t& flags, Sha256& h) {
  const auto in = exact(p, null ? 0 : len);
  std::unique_ptr<uint32_t[]> rec(new uint32_t[REC_STRIDE]);
  std::unique_ptr<uint8_t[]> pts(new uint8_t[NPT * 64]), epk(new uint8_t[128]);
  const int32_t st = parse_identity(null ? nullptr : in.get(), len, bn, rec.get(), pts.get(), epk.get());
  flags = rec[R_FLAGS];
  put32(h, (uint32_t)st);
  h.update(reinterpret_cast<const uint8_t*>(rec.get()), REC_STRIDE * 4);
  h.update(pts.get(), NPT * 64);
  h.update(epk.get(), 128);
  CHECK(st == FTS_OK || st == FTS_E_ID_MALFORMED || st == FTS_E_ID_BADNYM);
  return st;
}
static int32_t run_nym(const uint8_t* p, size_t len, bool null, bool bn, Sha256& h) {
  const auto in = exact(p, null ? 0 : len);
  std::unique_ptr<uint32_t[]> rec(new uint32_t[NREC]);
  const int32_t st = parse_nym_sig(null ? nullptr : in.get(), len, bn, rec.get());
  put32(h, (uint32_t)st);
  h.update(reinterpret_cast<const uint8_t*>(rec.get()), NREC * 4);
  CHECK(st == FTS_OK || st == FTS_E_NYM_MALFORMED || st == FTS_E_NYM_INVALID);
  return st;
}
static int32_t run_audit(const uint8_t* p, size_t len, bool null, bool bn, int32_t& rh_pre, Sha256& h) {
  const auto in = exact(p, null ? 0 : len);
  std::unique_ptr<uint8_t[]> eid(new uint8_t[64]), rh(new uint8_t[64]);
  const int32_t st = parse_audit_identity(null ? nullptr : in.get(), len, bn, eid.get(), rh.get(), rh_pre);
  put32(h, (uint32_t)st);
  put32(h, (uint32_t)rh_pre);
  h.update(eid.get(), 64);
  h.update(rh.get(), 64);
  CHECK(st == FTS_OK || st == FTS_E_AUDIT_MALFORMED || st == FTS_E_AUDIT_NO_EIDNYM || st == FTS_E_AUDIT_EID_POINT);
  CHECK(rh_pre == FTS_OK || (st == FTS_OK && (rh_pre == FTS_E_AUDIT_NO_RHNYM || rh_pre == FTS_E_AUDIT_RH_POINT)));
  // a point is handed over only with a clean status for its half
  const uint8_t zero[64] = {0};
  if (st != FTS_OK) CHECK(memcmp(eid.get(), zero, 64) == 0);
  if (st != FTS_OK || rh_pre != FTS_OK) CHECK(memcmp(rh.get(), zero, 64) == 0);
  return st;
}
// the issuer key's walk and every blob either creator extracts (accept bit, then the bytes)
static void run_ipk(const uint8_t* p, size_t len, Sha256& h) {
  const auto in = exact(p, len);
  IpkFields f;
  const bool ok = parse_ipk(in.get(), len, f);
  put32(h, ok ? (uint32_t)f.n_attrs + 1u : 0u);
  if (!ok) return;
  std::unique_ptr<uint8_t[]> out(new uint8_t[64]), out2(new uint8_t[128]), h32(new uint8_t[32]);
  const Span* pt[6] = {&f.h_sk, &f.h_rand, &f.h_attrs[0], &f.h_attrs[1], &f.h_attrs[2], &f.h_attrs[3]};
  for (int q = 0; q < 6; q++)
    for (int strict = 0; strict < 2; strict++) {
      memset(out.get(), 0, 64);
      put32(h, fts::ecp_xy(*pt[q], out.get(), strict != 0) ? 1u : 0u);
      h.update(out.get(), 64);
    }
  memset(out2.get(), 0, 128);
  put32(h, fts::ecp2_raw(f.w, out2.get()) ? 1u : 0u);
  h.update(out2.get(), 128);
  ipk_hash32(f, h32.get());
  h.update(h32.get(), 32);
}

// ---- which prefixes of an identity may parse: from its field list, the cut must fall
// on a boundary of the outer message; `nym` / `proof`: fields 1 / 4 lie before the cut
struct Cut {
  bool boundary = false, nym = false, proof = false;
};
static std::vector<Cut> identity_cuts(const std::string& id) {
  std::vector<Cut> cuts(id.size() + 1);
  Pb pb{reinterpret_cast<const uint8_t*>(id.data()), id.size()};
  Pb::Field d;
  Cut c;
  while (pb.o < pb.n && pb.next(d)) {
    c.boundary = true;
    c.nym = c.nym || d.f == 1;
    c.proof = c.proof || d.f == 4;
    cuts[pb.o] = c;
  }
  return cuts;
}

static Result run_input(const Input& in) {
  Result r;
  Sha256 h;
  h.init();
  const uint8_t* p = reinterpret_cast<const uint8_t*>(in.bytes.data());
  const size_t len = in.bytes.size();
  const uint32_t bad = F_EARLY_MALFORMED | F_LATE_MALFORMED | F_NO_EID | F_NO_RH;
  const std::vector<Cut> cuts = in.kind == ID || in.kind == AUDIT ? identity_cuts(in.bytes) : std::vector<Cut>();
  // k: prefix k; -1: the input itself; -2: a corrupted copy or a null / zero-length form
  auto one = [&](const uint8_t* q, size_t l, bool null, long k) {
    r.calls++;
    if (in.kind == ID) {
      uint32_t flags = 0;
      const int32_t st = run_id(q, l, null, in.bn, flags, h);
      if (k >= 0) {  // a strict prefix: never a clean record unless the field list allows it
        const Cut& c = cuts[(size_t)k];
        if (st == FTS_OK && !(flags & bad)) CHECK(c.boundary && c.nym && c.proof);
        if (st == FTS_E_ID_BADNYM) CHECK(c.boundary && c.nym);
      } else if (k == -1 && in.honest) {
        CHECK(st == FTS_OK && flags == 0);
      } else if (null || l == 0) {
        CHECK(st == FTS_E_ID_MALFORMED);
      }
    } else if (in.kind == AUDIT) {
      int32_t rh_pre = 0;
      const int32_t st = run_audit(q, l, null, in.bn, rh_pre, h);
      if (k >= 0) {  // a strict prefix parses only at a field boundary past the proof (the nym key is not read)
        if (st != FTS_E_AUDIT_MALFORMED) CHECK(cuts[(size_t)k].boundary && cuts[(size_t)k].proof);
      } else if (k == -1) {
        r.pre = st, r.rh_pre = rh_pre;
        if (in.honest) CHECK(st == FTS_OK && rh_pre == FTS_OK);
      } else if (null || l == 0) {
        CHECK(st == FTS_E_AUDIT_MALFORMED);
      }
    } else if (in.kind == NYM) {
      const int32_t st = run_nym(q, l, null, in.bn, h);
      if (k == -1 && in.honest) CHECK(st == FTS_OK);
      if (null || l == 0) CHECK(st == FTS_E_NYM_MALFORMED);
    } else if (!null) {  // the creators reject a null key before parsing
      run_ipk(q, l, h);
    }
  };
  one(p, len, false, -1);
  one(p, 0, false, -2);
  one(nullptr, 0, true, -2);
  one(nullptr, len, true, -2);
  for (size_t k = 0; k < len; k++) one(p, k, false, (long)k);
  std::string m = in.bytes;
  for (size_t k = 0; k < len; k += in.tile ? 16 : 1)
    for (uint8_t x : {(uint8_t)0x01, (uint8_t)0x80}) {
      m[k] = (char)(in.bytes[k] ^ x);
      one(reinterpret_cast<const uint8_t*>(m.data()), len, false, -2);
      m[k] = in.bytes[k];
    }
  h.final(r.digest);
  return r;
}

// ---- the nym items' staging (pack_nym_item, nym_stream_words) into exactly-sized blocks,
// against the layout written out here: both curves, message lengths 0..5 (every fill to
// the word boundary), a null message of length 0, a nym of the wrong length and an
// FP256BN nym without its 0x04.  Returns the number of cases.
static int check_pack() {
  int cases = 0;
  uint8_t hash[32], key[65], text[5];
  for (int k = 0; k < 32; k++) hash[k] = (uint8_t)(0xa0 + k);
  for (int k = 0; k < 65; k++) key[k] = (uint8_t)(k + 1);
  for (int k = 0; k < 5; k++) text[k] = (uint8_t)(0xf1 + k);
  for (bool bn : {true, false}) {
    const size_t klen = bn ? 64 : 65;
    key[0] = bn ? 0x01 : 0x04;
    for (int form = 0; form < 4; form++) {  // 0 good, 1 short, 2 null, 3 FP256BN without the 0x04
      if (form == 3 && bn) continue;
      for (size_t ml = 0; ml <= 5; ml++)
        for (bool null_msg : {false, true}) {
          if (null_msg && ml) continue;
          const bool good = form == 0;
          const auto nym = exact(key, form == 1 ? klen - 1 : klen);
          if (form == 3) nym[0] = 0x02;
          const auto msg = exact(text, ml);
          const size_t pre = bn ? 0 : 166, words = (pre + ml + 3) / 4 + 1;
          CHECK(nym_stream_words(bn, ml) == words);
          std::unique_ptr<uint8_t[]> slot(new uint8_t[64]), mw(new uint8_t[words * 4]);
          memset(slot.get(), 0xee, 64);
          memset(mw.get(), 0xee, words * 4);
          uint32_t len = 0;
          const bool ok = pack_nym_item(bn, form == 2 ? nullptr : nym.get(), form == 1 ? klen - 1 : klen, hash,
                                        null_msg ? nullptr : msg.get(), ml, slot.get(), mw.get(), &len);
          std::vector<uint8_t> want_slot(64, 0), want;
          if (good) want_slot.assign(key + (bn ? 0 : 1), key + klen);
          if (!bn) {
            want = {'s', 'i', 'g', 'n', 0x04};
            want.resize(69, 0);
            if (good) want.insert(want.end(), key, key + 65);
            want.resize(134, 0);
            want.insert(want.end(), hash, hash + 32);
          }
          want.insert(want.end(), text, text + ml);
          want.resize(words * 4, 0);
          CHECK(ok == good && len == pre + ml);
          CHECK(memcmp(slot.get(), want_slot.data(), 64) == 0);
          CHECK(memcmp(mw.get(), want.data(), words * 4) == 0);
          cases++;
        }
    }
  }
  return cases;
}

// the inputs' digests in input order -> the run's digest
static std::string run_all(const std::vector<Input>& in, size_t threads, size_t& calls, std::vector<Result>& res) {
  res.assign(in.size(), Result());
  std::vector<std::thread> th;
  for (size_t t = 0; t < threads; t++)
    th.emplace_back([&, t] {
      for (size_t i = t; i < in.size(); i += threads) res[i] = run_input(in[i]);
    });
  for (auto& x : th) x.join();
  Sha256 h;
  h.init();
  calls = 0;
  for (const Result& r : res) h.update(r.digest, 32), calls += r.calls;
  uint8_t d[32];
  h.final(d);
  char hex[65];
  for (int i = 0; i < 32; i++) snprintf(hex + 2 * i, 3, "%02x", d[i]);
  return hex;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: idemix_parse_check <inputs>\n");
    return 2;
  }
  std::ifstream f(argv[1]);
  std::vector<Input> in;
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream ss(line);
    std::string kind, curve, hex, mark;
    if (!(ss >> kind >> curve)) continue;
    ss >> hex >> mark;
    if (hex == "-") hex.clear();
    Input x;
    x.kind = kind == "id" ? ID : kind == "nym" ? NYM : kind == "audit" ? AUDIT : IPK;
    x.bn = curve == "bn254";
    x.tile = mark == "tile";
    x.honest = x.tile || mark == "honest";
    const bool known = (kind == "id" || kind == "nym" || kind == "ipk" || kind == "audit") && (x.bn || curve == "fp256bn") &&
                       hex.size() % 2 == 0 && (mark.empty() || x.honest);
    CHECK(known);
    if (!known) continue;
    for (size_t k = 0; k < hex.size(); k += 2) x.bytes.push_back((char)strtoul(hex.substr(k, 2).c_str(), nullptr, 16));
    in.push_back(x);
  }
  CHECK(!in.empty());
  printf("idemix_parse_check: pack %d cases\n", check_pack());
  size_t calls = 0, calls4 = 0;
  std::vector<Result> res, res4;
  const std::string serial = run_all(in, 1, calls, res), threaded = run_all(in, 4, calls4, res4);
  CHECK(serial == threaded && calls == calls4);
  for (size_t i = 0; i < in.size(); i++)
    if (in[i].kind == AUDIT) printf("audit %zu %d %d\n", i, res[i].pre, res[i].rh_pre);
  printf("idemix_parse_check: %zu inputs, %zu parser calls, sha256 %s\n", in.size(), calls, serial.c_str());
  if (g_failed) {
    fprintf(stderr, "idemix_parse_check: %d checks failed\n", g_failed.load());
    return 1;
  }
  printf("idemix_parse_check: ok\n");
  return 0;
}
