// The SHA-256 padding of a byte string held as words, for kernels that read a message from
// HBM as aligned words and build the blocks in registers (the idemix nym and audit kernels,
// device/idemix_hash.hpp).  Host and device: lib/sign_check compares the stream assembled
// through these two functions with the byte-streaming Sha256.
#pragma once
#include "sha256.hpp"

namespace fts {

// SHA-256 blocks of a string of len bytes: (len + 1 + 8) rounded up to 64, without
// the 32-bit overflow of that sum (the API takes lengths up to 0xffffff00 + a prefix)
FTS_HD uint32_t padded_blocks(uint32_t len) { return len / 64u + 1u + ((len % 64u) >= 56u ? 1u : 0u); }

// Big-endian word g of the padded stream of nb = padded_blocks(pre + len) blocks over
// pre + len bytes, for g >= pre / 4.  The stream's last len bytes are m (4-byte
// aligned, zero-filled to a whole word, one spare word: host staging); its first pre
// bytes (a multiple of 4) are the caller's, from registers.
FTS_HD uint32_t padded_word(const uint32_t* __restrict__ m, uint32_t pre, uint32_t len, uint32_t nb, uint32_t g) {
  const uint64_t bits = ((uint64_t)pre + len) * 8u;
  if (g == 16u * nb - 2u) return (uint32_t)(bits >> 32);
  if (g == 16u * nb - 1u) return (uint32_t)bits;
  const uint32_t j = g - pre / 4u, b = 4u * j;  // g <= 16 nb - 3: 4 j < 64 nb <= 2^32
  if (b > len) return 0u;
  if (b == len) return 0x80000000u;  // the terminator
  const uint32_t raw = __builtin_bswap32(m[j]);
  const uint32_t keep = len - b;
  if (keep >= 4u) return raw;
  // 1..3 bytes, then the terminator
  return (raw & (0xffffffffu << (32 - 8 * keep))) | (0x80000000u >> (8 * keep));
}

}  // namespace fts
