// The hashing every idemix kernel shares (mathlib HashToZr = SHA-256 read big-endian
// mod r), written once for both curves: the SHA-256 padding of a byte string held as
// words (common/sha_padding.hpp: padded_blocks, padded_word), the Fiat-Shamir transcript
// of a ByteSink, and the second hash c = HashToZr(Zr.Bytes(c') || Zr.Bytes(nonce)).  CV is
// a curve traits struct (idemix_curves.hpp).
#pragma once
#include "../common/sha_padding.hpp"
#include "field.hpp"  // FTS_DEV

namespace fts {

// out <- HashToZr(Zr.Bytes(c1) || nonce): c1 canonical LE limbs, the nonce as its eight
// big-endian words; two compressions (the second block is padding alone)
template <class CV>
FTS_DEV void nonce_challenge(const uint32_t c1[8], const uint32_t* nonce, uint32_t out[8]) {
  uint32_t st[8], w[16];
#pragma unroll
  for (int k = 0; k < 8; k++) w[k] = c1[7 - k];
#pragma unroll
  for (int k = 0; k < 8; k++) w[8 + k] = nonce[k];
  sha256_init(st);
  sha256_compress(st, w);
  w[0] = 0x80000000u;
#pragma unroll
  for (int k = 1; k < 15; k++) w[k] = 0u;
  w[15] = 512u;
  sha256_compress(st, w);
  CV::digest_mod_r(st, out);
}

// out <- HashToZr(the sink's bytes): the padding goes into the sink's lane scratch
// (room for padded_blocks(off) blocks), then the blocks are read back as words
template <class CV, class Sink>
FTS_DEV void sink_digest(Sink& M, uint32_t out[8]) {
  const uint32_t len = M.off, nb = padded_blocks(len);
  M.put_byte(0x80);
  while (M.off < nb * 64 - 8) M.put_byte(0);
  M.put_word(0u);
  M.put_word(len * 8u);
  uint32_t st[8], w[16];
  sha256_init(st);
  for (uint32_t b = 0; b < nb; b++) {
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = M.word(16 * b + k);
    sha256_compress(st, w);
  }
  CV::digest_mod_r(st, out);
}

}  // namespace fts
