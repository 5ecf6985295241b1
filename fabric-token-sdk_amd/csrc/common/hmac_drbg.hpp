// RFC 6979 nonce derivation for ECDSA P-256: HMAC-DRBG (SP 800-90A) over SHA-256,
// shared by the device (k_ecdsa_sign, one signature per lane) and the host
// (lib/sign_check, which checks it against the RFC's vectors on the CPU).
//
// Every value is 8 big-endian words (word 0 = the most significant 32 bits).
// qlen = hlen = 256, so bits2int is the identity and one HMAC output is one
// candidate.  The HMAC messages have fixed lengths:
//   V                                   32 bytes   (1 inner block)
//   V || 0x00                           33 bytes   (1 inner block, the retry step)
//   V || byte || x || h1                97 bytes   (2 inner blocks)
//   V || byte || x || h1 || extra      129 bytes   (3 inner blocks, section 3.6)
// so each is built as whole 16-word blocks with static indices (registers on the
// device, no scratch); the byte after V shifts the tail by 8 bits.
#pragma once
#include "sha256.hpp"

namespace fts {

// P-256 group order n, big-endian words
struct P256Order {
  static constexpr uint32_t N[8] = {0xffffffffu, 0x00000000u, 0xffffffffu, 0xffffffffu,
                                    0xbce6faadu, 0xa7179e84u, 0xf3b9cac2u, 0xfc632551u};
};

// a < b, both 8 big-endian words
FTS_HD bool be_lt(const uint32_t a[8], const uint32_t b[8]) {
  bool lt = false, decided = false;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    lt = decided ? lt : a[i] < b[i];
    decided = decided || a[i] != b[i];
  }
  return lt;
}

// bits2octets for hlen = qlen: h mod n (h < 2^256 < 2n: one subtraction)
FTS_HD void bits2octets_p256(const uint32_t h[8], uint32_t out[8]) {
  const bool sub = !be_lt(h, P256Order::N);
  uint32_t bw = 0;
#pragma unroll
  for (int i = 7; i >= 0; i--) {
    const uint64_t d = (uint64_t)h[i] - (sub ? P256Order::N[i] : 0u) - bw;
    out[i] = (uint32_t)d;
    bw = (uint32_t)(d >> 63);
  }
}

// HMAC-SHA-256 under a 32-byte key: the states after the ipad / opad blocks
struct HmacKey {
  uint32_t in[8], out[8];
};

FTS_HD void hmac_key(const uint32_t K[8], HmacKey& hk) {
  uint32_t w[16];
#pragma unroll 1
  for (int side = 0; side < 2; side++) {
    const uint32_t pad = side ? 0x5c5c5c5cu : 0x36363636u;
    uint32_t st[8];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = (i < 8 ? K[i] : 0u) ^ pad;
    sha256_init(st);
    sha256_compress(st, w);
#pragma unroll
    for (int i = 0; i < 8; i++) {  // no pointer into hk: it stays in registers on the device
      if (side) hk.out[i] = st[i];
      else hk.in[i] = st[i];
    }
  }
}

// outer hash over the 32-byte inner digest `st` (consumed) -> mac
FTS_HD void hmac_outer(const HmacKey& hk, const uint32_t st[8], uint32_t mac[8]) {
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = st[i], mac[i] = hk.out[i];
  w[8] = 0x80000000u;
#pragma unroll
  for (int i = 9; i < 15; i++) w[i] = 0u;
  w[15] = (64u + 32u) * 8u;
  sha256_compress(mac, w);
}

// HMAC_K(V || byte || tail[0..NT-1]) for NT tail words; NT < 0: HMAC_K(V) alone
template <int NT>
FTS_HD void hmac_v(const HmacKey& hk, const uint32_t V[8], uint32_t byte, const uint32_t* tail, uint32_t mac[8]) {
  constexpr int LEN = NT < 0 ? 32 : 33 + 4 * NT;  // message bytes
  constexpr int NB = (LEN + 9 + 63) / 64;         // inner blocks behind the ipad block
  uint32_t s[16 * NB];
#pragma unroll
  for (int i = 0; i < 16 * NB; i++) s[i] = 0u;
#pragma unroll
  for (int i = 0; i < 8; i++) s[i] = V[i];
  if (NT < 0) {
    s[8] = 0x80000000u;
  } else {
    uint32_t carry = byte << 24;
#pragma unroll
    for (int j = 0; j < (NT < 0 ? 0 : NT); j++) {
      s[8 + j] = carry | (tail[j] >> 8);
      carry = tail[j] << 24;
    }
    s[8 + (NT < 0 ? 0 : NT)] = carry | 0x00800000u;
  }
  s[16 * NB - 1] = (64u + (uint32_t)LEN) * 8u;
  uint32_t st[8];
#pragma unroll
  for (int i = 0; i < 8; i++) st[i] = hk.in[i];
#pragma unroll
  for (int b = 0; b < NB; b++) sha256_compress(st, s + 16 * b);
  hmac_outer(hk, st, mac);
}

// The generator of RFC 6979 section 3.2 for one (private key, digest) pair.
// init<EXTRA>(x, h1, extra): steps b-g (x: the private scalar, h1: SHA-256 of the
// message, not reduced; extra: 8 words of additional data, section 3.6).
// next(k): step h -- the next candidate in [1, n-1]; a second call continues the
// RFC's loop as after a rejected candidate (r = 0 or s = 0 in the caller).
struct Rfc6979 {
  uint32_t K[8], V[8];
  bool drawn;

  template <bool EXTRA>
  FTS_HD void init(const uint32_t x[8], const uint32_t h1[8], const uint32_t* extra) {
    constexpr int NT = EXTRA ? 24 : 16;
    uint32_t tail[NT];
    bits2octets_p256(h1, tail + 8);
#pragma unroll
    for (int i = 0; i < 8; i++) tail[i] = x[i], V[i] = 0x01010101u, K[i] = 0u;
    if (EXTRA) {
#pragma unroll
      for (int i = 0; i < 8; i++) tail[(EXTRA ? 16 : 0) + i] = extra[i];
    }
#pragma unroll 1
    for (uint32_t byte = 0; byte < 2; byte++) {
      HmacKey hk;
      hmac_key(K, hk);
      hmac_v<NT>(hk, V, byte, tail, K);
      hmac_key(K, hk);
      hmac_v<-1>(hk, V, 0u, nullptr, V);
    }
    drawn = false;
  }

  FTS_HD void next(uint32_t k[8]) {
    uint32_t zero[8];
#pragma unroll
    for (int i = 0; i < 8; i++) zero[i] = 0u;
    for (;;) {
      HmacKey hk;
      hmac_key(K, hk);
      if (drawn) {
        hmac_v<0>(hk, V, 0u, nullptr, K);
        hmac_key(K, hk);
        hmac_v<-1>(hk, V, 0u, nullptr, V);
      }
      drawn = true;
      hmac_v<-1>(hk, V, 0u, nullptr, V);
#pragma unroll
      for (int i = 0; i < 8; i++) k[i] = V[i];
      if (be_lt(zero, k) && be_lt(k, P256Order::N)) return;
    }
  }
};

}  // namespace fts
