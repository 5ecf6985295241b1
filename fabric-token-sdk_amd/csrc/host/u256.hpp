// 256-bit arithmetic on untrusted big-endian byte strings (the idemix host
// parsers' Zr fields): LE 32-bit limbs, the modulus a parameter.  No HIP include.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace fts {
namespace u256 {

// group orders of BN254 (gnark) and FP256BN (AMCL), LE limbs
constexpr uint32_t kRbn[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u,
                              0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
constexpr uint32_t kRfbn[8] = {0xd10b500du, 0xf62d536cu, 0x1299921au, 0x0cdc65fbu,
                               0xee71a49eu, 0x46e5f25eu, 0xfffcf0cdu, 0xffffffffu};

// field prime of FP256BN
constexpr uint32_t kPfbn[8] = {0xaed33013u, 0xd3292ddbu, 0x12980a82u, 0x0cdc65fbu,
                               0xee71a49fu, 0x46e5f25eu, 0xfffcf0cdu, 0xffffffffu};

inline bool ge(const uint32_t a[8], const uint32_t m[8]) {
  for (int k = 7; k >= 0; k--)
    if (a[k] != m[k]) return a[k] > m[k];
  return true;
}
inline void sub(uint32_t a[8], const uint32_t m[8]) {
  uint64_t bw = 0;
  for (int k = 0; k < 8; k++) {
    const uint64_t d = (uint64_t)a[k] - m[k] - bw;
    a[k] = (uint32_t)d;
    bw = (d >> 63) & 1;
  }
}
// big-endian bytes -> LE limbs if the value fits 256 bits
inline bool be_limbs(const uint8_t* b, size_t len, uint32_t out[8]) {
  size_t st = 0;
  while (st < len && b[st] == 0) st++;
  memset(out, 0, 32);
  if (len - st > 32) return false;
  for (size_t k = st; k < len; k++) {
    const size_t bit = (len - 1 - k) * 8;
    out[bit / 32] |= (uint32_t)b[k] << (bit % 32);
  }
  return true;
}
// (x * 256 + byte) mod m for x < m < 2^256
inline void mulacc_byte(uint32_t x[8], uint8_t byte, const uint32_t m[8]) {
  uint32_t t[9];
  uint64_t c = byte;
  for (int k = 0; k < 8; k++) {
    const uint64_t v = ((uint64_t)x[k] << 8) + c;
    t[k] = (uint32_t)v;
    c = v >> 32;
  }
  t[8] = (uint32_t)c;
  // x < m gives t = 256 x + byte < 256 m: at most 256 subtractions, the guard is never reached
  for (int guard = 0; guard < 300; guard++) {
    if (t[8] == 0 && !ge(t, m)) break;
    uint64_t bw = 0;
    for (int k = 0; k < 9; k++) {
      const uint64_t d = (uint64_t)t[k] - (k < 8 ? m[k] : 0u) - bw;
      t[k] = (uint32_t)d;
      bw = (d >> 63) & 1;
    }
  }
  memcpy(x, t, 32);
}
// G1.Mul semantics for an unreduced big-endian scalar of any length: value mod m
inline void mod_m(const uint8_t* b, size_t len, const uint32_t m[8], uint32_t out[8]) {
  if (be_limbs(b, len, out)) {
    while (ge(out, m)) sub(out, m);
    return;
  }
  memset(out, 0, 32);
  for (size_t k = 0; k < len; k++) mulacc_byte(out, b[k], m);
}

}  // namespace u256
}  // namespace fts
