// Stand-alone driver of the signing code that runs on the host: the RFC 6979
// HMAC-DRBG (common/hmac_drbg.hpp, the code k_ecdsa_sign runs per lane) and the two
// encoders (host/sign_encode.hpp), built with the host address and
// undefined-behaviour sanitizers (any report is fatal).  No device, no library.
// One command per line of standard input, one line of hex per result:
//   k   <x> <h1> [extra]      the nonce for private scalar x and digest h1 (32 B each)
//   k3  <x> <h1> [extra]      three successive candidates (the retry step between them)
//   km  <x> <message hex|->   the nonce for SHA-256(message)
//   der <r> <s>               the DER signature
//   nym <c> <s_sk> <s_r> <nonce>   the NymSignature proto
//   pad <prefix hex|-> <tail hex|->   SHA-256 of prefix || tail with the padded stream assembled
//                             by padded_word / padded_blocks (common/sha_padding.hpp, the nym and
//                             audit kernels' code); exit status 2 if the streaming hash differs
//   blocks <len, 4 B>         padded_blocks(len), 4 B
// Every output buffer is a heap block of exactly its size.  Exit status 0 iff every
// line was understood.
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "../common/hmac_drbg.hpp"
#include "../common/sha_padding.hpp"
#include "../host/sign_encode.hpp"

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
static void words(const uint8_t b[32], uint32_t w[8]) {
  for (int i = 0; i < 8; i++)
    w[i] = ((uint32_t)b[4 * i] << 24) | ((uint32_t)b[4 * i + 1] << 16) | ((uint32_t)b[4 * i + 2] << 8) | b[4 * i + 3];
}
static void put_words(const uint32_t w[8]) {
  for (int i = 0; i < 8; i++) printf("%08x", w[i]);
}

int main() {
  std::string line;
  int bad = 0;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    std::string cmd, tok;
    if (!(is >> cmd)) continue;
    std::vector<std::vector<uint8_t>> a;
    bool ok = true;
    while (is >> tok) {
      a.emplace_back();
      ok = ok && unhex(tok, a.back());
    }
    auto all32 = [&](size_t lo, size_t hi) {
      for (size_t i = lo; i < hi && i < a.size(); i++)
        if (a[i].size() != 32) return false;
      return true;
    };
    if (ok && (cmd == "k" || cmd == "k3" || cmd == "km") && a.size() >= 2) {
      const bool msg = cmd == "km";
      if (!all32(0, 1) || (msg ? a.size() != 2 : (a.size() > 3 || !all32(1, 3)))) {
        bad++;
        continue;
      }
      uint8_t dg[32];
      if (msg) sha256(a[1].data(), a[1].size(), dg);
      else memcpy(dg, a[1].data(), 32);
      uint32_t x[8], h1[8], ex[8];
      words(a[0].data(), x);
      words(dg, h1);
      Rfc6979 g;
      if (a.size() == 3) {
        words(a[2].data(), ex);
        g.init<true>(x, h1, ex);
      } else {
        g.init<false>(x, h1, nullptr);
      }
      std::unique_ptr<uint32_t[]> k(new uint32_t[8]);
      for (int r = 0; r < (cmd == "k3" ? 3 : 1); r++) {
        g.next(k.get());
        if (r) printf(" ");
        put_words(k.get());
      }
      printf("\n");
    } else if (ok && cmd == "der" && a.size() == 2 && all32(0, 2)) {
      // the length first, into a scratch block of the documented maximum; then again
      // into a block of exactly that length
      std::unique_ptr<uint8_t[]> big(new uint8_t[host::ECDSA_SIG_MAX]);
      const uint32_t n = host::ecdsa_sig_der(a[0].data(), a[1].data(), big.get());
      std::unique_ptr<uint8_t[]> exact(new uint8_t[n]);
      const uint32_t n2 = host::ecdsa_sig_der(a[0].data(), a[1].data(), exact.get());
      if (n2 != n || memcmp(big.get(), exact.get(), n) != 0) return 2;
      put_hex(exact.get(), n);
      printf("\n");
    } else if (ok && cmd == "nym" && a.size() == 4 && all32(0, 4)) {
      std::unique_ptr<uint8_t[]> out(new uint8_t[host::NYM_SIG_LEN]);
      host::nym_sig_proto(a[0].data(), a[1].data(), a[2].data(), a[3].data(), out.get());
      put_hex(out.get(), host::NYM_SIG_LEN);
      printf("\n");
    } else if (ok && cmd == "pad" && a.size() == 2 && a[0].size() % 4 == 0) {
      // the stream as the kernels assemble it: the prefix's words from the caller, the
      // rest through padded_word over a block of exactly the staged size
      const uint32_t pre = (uint32_t)a[0].size(), len = (uint32_t)a[1].size(), nb = padded_blocks(pre + len);
      const size_t mw = (len + 3) / 4 + 1;
      std::unique_ptr<uint32_t[]> m(new uint32_t[mw]);
      memset(m.get(), 0, mw * 4);
      if (len) memcpy(m.get(), a[1].data(), len);
      uint32_t st[8], w[16];
      sha256_init(st);
      for (uint32_t blk = 0; blk < nb; blk++) {
        for (uint32_t k = 0; k < 16; k++) {
          const uint32_t g = 16 * blk + k;
          if (g < pre / 4) {
            const uint8_t* p = a[0].data() + 4 * g;
            w[k] = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
          } else {
            w[k] = padded_word(m.get(), pre, len, nb, g);
          }
        }
        sha256_compress(st, w);
      }
      // against the byte-streaming hash of the same bytes
      std::vector<uint8_t> all(a[0]);
      all.insert(all.end(), a[1].begin(), a[1].end());
      uint8_t dg[32];
      uint32_t want[8];
      sha256(all.data(), all.size(), dg);
      words(dg, want);
      if (memcmp(st, want, 32) != 0) return 2;
      put_words(st);
      printf("\n");
    } else if (ok && cmd == "blocks" && a.size() == 1 && a[0].size() == 4) {
      const uint32_t len = ((uint32_t)a[0][0] << 24) | ((uint32_t)a[0][1] << 16) | ((uint32_t)a[0][2] << 8) | a[0][3];
      printf("%08x\n", padded_blocks(len));
    } else {
      bad++;
    }
  }
  if (bad) fprintf(stderr, "sign_check: %d lines not understood\n", bad);
  return bad ? 1 : 0;
}
