// Stand-alone driver of identity generation's host side (host/identity_write.hpp): the
// draws, the credential / revocation-information parsers and the identity writer, built with
// the host address and undefined-behaviour sanitizers (any report is fatal).  No device, no
// library.  One command per line of standard input, one line per result; curve = 1 (BN254)
// or 0 (FP256BN_AMCL):
//   draws <curve> <seed> <i>                        the 18 scalars, 32 B big-endian each
//   len   <curve> <epoch>                           the identity's length
//   write <curve> <epoch> <pts> <sc> <nonce> <epk|->  the identity (pts 6 x 64 B, sc 13 x 32 B)
//   cred  <curve> <credential proto>                "ok" + E S attrs, or "bad"
//   cri   <curve> <cri proto|->                     "ok" + epoch + epoch_pk, or "bad"
// Every input and output buffer is a heap block of exactly its size.  Exit status 0 iff every
// line was understood.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../host/identity_write.hpp"

using namespace fts;

static bool unhex(const std::string& s, std::vector<uint8_t>& out) {
  out.clear();
  if (s == "-") return true;
  if (s.size() % 2) return false;
  auto nib = [](char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; };
  for (size_t i = 0; i < s.size(); i += 2) {
    const int h = nib(s[i]), l = nib(s[i + 1]);
    if (h < 0 || l < 0) return false;
    out.push_back((uint8_t)(16 * h + l));
  }
  return true;
}
static void put_hex(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; i++) printf("%02x", p[i]);
}
// an exact-size heap copy (a read past the end is a sanitizer report)
static std::unique_ptr<uint8_t[]> exact(const std::vector<uint8_t>& v) {
  std::unique_ptr<uint8_t[]> p(new uint8_t[v.size() ? v.size() : 1]);
  if (!v.empty()) memcpy(p.get(), v.data(), v.size());
  return p;
}

int main() {
  std::string line;
  int bad = 0;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    std::string cmd;
    int curve = -1;
    if (!(is >> cmd)) continue;
    if (!(is >> curve) || (curve != 0 && curve != 1)) {
      bad++;
      continue;
    }
    const bool bn = curve == 1;
    std::vector<std::string> a;
    for (std::string tok; is >> tok;) a.push_back(tok);
    if (cmd == "draws" && a.size() == 2) {
      const uint64_t seed = strtoull(a[0].c_str(), nullptr, 10), i = strtoull(a[1].c_str(), nullptr, 10);
      std::unique_ptr<uint32_t[][8]> d(new uint32_t[idgen::ND][8]);
      idgen::identity_draws(bn, host::Rng(seed + i), d.get());
      std::unique_ptr<uint8_t[]> o(new uint8_t[32]);
      for (int k = 0; k < idgen::ND; k++) {
        idgen::limbs_to_be32(d[k], o.get());
        put_hex(o.get(), 32);
      }
      printf("\n");
    } else if (cmd == "len" && a.size() == 1) {
      printf("%zu\n", idgen::identity_len(bn, strtoull(a[0].c_str(), nullptr, 10)));
    } else if (cmd == "write" && a.size() == 5) {
      const uint64_t epoch = strtoull(a[0].c_str(), nullptr, 10);
      std::vector<uint8_t> pts, sc, nonce, epk;
      if (!unhex(a[1], pts) || !unhex(a[2], sc) || !unhex(a[3], nonce) || !unhex(a[4], epk) ||
          pts.size() != 64 * idgen::NPTS || sc.size() != 32 * idgen::NSC || nonce.size() != 32 ||
          (a[4] != "-" && epk.size() != 128)) {
        bad++;
        continue;
      }
      const auto p = exact(pts), s = exact(sc), nn = exact(nonce), e = exact(epk);
      const idgen::IdentityParts v{p.get(), s.get(), nn.get(), a[4] == "-" ? (bn ? idgen::kG2Bn : idgen::kG2Fbn) : e.get(),
                                   epoch};
      const size_t n = idgen::identity_len(bn, epoch);
      std::unique_ptr<uint8_t[]> out(new uint8_t[n]);
      idgen::write_identity(bn, v, out.get());
      put_hex(out.get(), n);
      printf("\n");
    } else if (cmd == "cred" && a.size() == 1) {
      std::vector<uint8_t> raw;
      if (!unhex(a[0], raw)) {
        bad++;
        continue;
      }
      const auto p = exact(raw);
      std::unique_ptr<idgen::CredFields> c(new idgen::CredFields);
      if (!idgen::parse_credential(p.get(), raw.size(), bn, *c)) {
        printf("bad\n");
        continue;
      }
      printf("ok ");
      put_hex(c->a, 64), put_hex(c->b, 64);
      uint8_t o[32];
      const uint32_t* sc[6] = {c->e, c->s, c->attrs[0], c->attrs[1], c->attrs[2], c->attrs[3]};
      for (int k = 0; k < 6; k++) idgen::limbs_to_be32(sc[k], o), put_hex(o, 32);
      printf("\n");
    } else if (cmd == "cri" && a.size() == 1) {
      std::vector<uint8_t> raw;
      if (!unhex(a[0], raw)) {
        bad++;
        continue;
      }
      const auto p = exact(raw);
      std::unique_ptr<idgen::CriFields> c(new idgen::CriFields);
      if (!idgen::parse_cri(a[0] == "-" ? nullptr : p.get(), raw.size(), bn, *c)) {
        printf("bad\n");
        continue;
      }
      printf("ok %llu ", (unsigned long long)c->epoch);
      put_hex(c->epoch_pk, 128);
      printf("\n");
    } else {
      bad++;
    }
  }
  if (bad) fprintf(stderr, "idgen_check: %d lines not understood\n", bad);
  return bad ? 1 : 0;
}
