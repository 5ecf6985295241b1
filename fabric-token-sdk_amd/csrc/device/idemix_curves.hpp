// The two curves idemix keys use here, behind one traits struct each, for every
// idemix kernel (nym signatures, identity proof, audit match, identity generation,
// credential verification): BN254 (gnark; G1 64-byte raw encodings, 16-bit signed
// fixed-base tables) and FP256BN (AMCL; 0x04 || X || Y, 16-bit unsigned tables).
// With them the base-field adaptors the pairing tower is written over, the scalar
// field Zr<CV> and the lane scratch views.  No tower code: the nym unit includes this
// header without pairing.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fixed_base.hpp"
#include "glv.hpp"
#include "helpers.hpp"
#include "transcript.hpp"
#include "fp256bn.hpp"
#include "pairing_consts.hpp"

// ------------------------------------------------------- base-field adaptors
// (BnField: fts::Fp with the grouped-MAC product; FbnField: the full-width
// Montgomery code of p256.hpp on FP256BN's p)
namespace pair {

struct BnField {
  using F = fts::Fp;
  using K = pairc::Bn254;
  static FTS_DEV F add(const F& a, const F& b) { return fts::f_add(a, b); }
  static FTS_DEV F sub(const F& a, const F& b) { return fts::f_sub(a, b); }
  static FTS_DEV F neg(const F& a) { return fts::f_neg(a); }
  // (the two-accumulator product f_mul_fips2 made k_idv_pairing slower, 21.9 ->
  // 26.7 ms per 65,536 identities: its extra column adds cost more than the
  // shorter MAD chain saves, even at one wave per SIMD)
  static FTS_DEV F mul(const F& a, const F& b) { return fts::fp_mul(a, b); }
  static FTS_DEV F zero() { return fts::f_zero<fts::FpP>(); }
  static FTS_DEV F one() { return fts::f_one<fts::FpP>(); }
  static FTS_DEV bool is_zero(const F& a) { return fts::f_is_zero(a); }
  static FTS_DEV bool eq(const F& a, const F& b) { return fts::f_eq(a, b); }
  static FTS_DEV F inv(const F& a) { return fts::nl_fp_inv(a); }
  static FTS_DEV F ld(const uint32_t* w) {
    F r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = w[i];
    return r;
  }
};

struct FbnField {
  using F = fbn::Fp;
  using K = pairc::Fp256bn;
  static FTS_DEV F add(const F& a, const F& b) { return p256::add(a, b); }
  static FTS_DEV F sub(const F& a, const F& b) { return p256::sub(a, b); }
  static FTS_DEV F zero() {
    F r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = 0;
    return r;
  }
  static FTS_DEV F neg(const F& a) { return p256::sub(zero(), a); }
  static FTS_DEV F mul(const F& a, const F& b) { return p256::mul(a, b); }
  static FTS_DEV F one() { return p256::load<fbn::PM>(fbn::PM::ONE); }
  static FTS_DEV bool is_zero(const F& a) { return p256::is_zero(a); }
  static FTS_DEV bool eq(const F& a, const F& b) { return p256::eq(a, b); }
  static FTS_DEV F inv(const F& a) { return p256::inv(a); }
  static FTS_DEV F ld(const uint32_t* w) { return p256::load<fbn::PM>(w); }
};

}  // namespace pair

namespace idv {

using namespace fts;

// ----------------------------------------------------------- curve traits
// BN254 (gnark-crypto through mathlib): G1.Bytes() = 64-byte raw X || Y, 64 zero
// bytes = identity; fixed-base tables of fixed_base.hpp (signed 16-bit windows)
struct BnCurve {
  using B = pair::BnField;
  using F = Fp;
  using PJ = G1J;
  static constexpr int G1_BYTES = 64;
  static constexpr bool HOST_MONT = true;  // the host hands points over in Montgomery form (host/bn254_host.hpp)
  static FTS_DEV PJ inf() { return g1j_identity(); }
  static FTS_DEV bool is_inf(const PJ& p) { return f_is_zero(p.z); }
  static FTS_DEV PJ dbl(const PJ& p) { return g1j_dbl(p); }
  static FTS_DEV void add_to(PJ& acc, const PJ& q) { add_inl(acc, q); }
  static FTS_DEV void madd_to(PJ& acc, const F& x, const F& y) {
    G1A q;
    q.x = x, q.y = y;
    madd_inl(acc, q);
  }
  static FTS_DEV PJ from_affine(const F& x, const F& y) {
    PJ r;
    r.x = x, r.y = y, r.z = f_one<FpP>();
    return r;
  }
  // raw BE X || Y -> affine Montgomery; NewG1FromBytes rules (canonical, on the curve; zeros = identity)
  static FTS_DEV bool decode(const uint8_t* raw, F& x, F& y, bool& ident) {
    G1A a;
    const bool ok = decode_point(raw, a);
    ident = ok && g1a_is_identity(a);
    x = a.x, y = a.y;
    return ok;
  }
  // affine Montgomery (identity: zeros) -> G1.Bytes()
  template <class Sink>
  static FTS_DEV void encode(Sink& s, const F& x, const F& y) {
    uint32_t pw[16];
    g1_mont_to_be_words(x, y, pw);
    for (int k = 0; k < 16; k++) s.put_word(pw[k]);
  }
  static FTS_DEV void fixed_mul_acc(PJ& acc, const uint32_t* tables, int base, const uint32_t* k) {
    Scalar s;
#pragma unroll
    for (int q = 0; q < 8; q++) s.v[q] = k[q];
    fb_mul_acc_jac(acc, tables + (size_t)base * FB_WORDS_PER_BASE, s);  // Jacobian: k_idv_var's registers
  }
  static FTS_DEV void decompose(const uint32_t k[8], uint32_t k1[4], uint32_t& s1, uint32_t k2[4], uint32_t& s2) {
    glv_decompose<Glv>(k, k1, s1, k2, s2);
  }
  static FTS_DEV F beta() { return glv_beta(); }
  // HashToZr of a digest -> canonical LE limbs
  static FTS_DEV void digest_mod_r(const uint32_t st[8], uint32_t out[8]) {
    const Fr r = digest_to_fr(st);
#pragma unroll
    for (int q = 0; q < 8; q++) out[q] = r.v[q];
  }
};

// FP256BN (AMCL through mathlib): G1.Bytes() = 0x04 || X || Y; decoded points
// must be canonical and on the curve (no identity encoding); fixed-base tables
// built by idemix_kernels.hip (k_fbn_table), FBN_NW unsigned 16-bit windows of 2^16 entries
constexpr int FBN_W = 16, FBN_NW = 16, FBN_ND = 1 << FBN_W;
struct FbnCurve {
  using B = pair::FbnField;
  using F = fbn::Fp;
  using PJ = fbn::PJ;
  static constexpr int G1_BYTES = 65;
  static constexpr bool HOST_MONT = false;  // the host hands over plain LE limbs (no Montgomery code for this p there)
  static FTS_DEV PJ inf() { return fbn::pj_inf(); }
  static FTS_DEV bool is_inf(const PJ& p) { return fbn::is_zero(p.z); }
  static FTS_DEV PJ dbl(const PJ& p) { return fbn::pj_dbl(p); }
  static FTS_DEV void add_to(PJ& acc, const PJ& q) { acc = fbn::pj_add(acc, q); }
  static FTS_DEV void madd_to(PJ& acc, const F& x, const F& y) { acc = fbn::pj_madd(acc, x, y); }
  static FTS_DEV PJ from_affine(const F& x, const F& y) {
    PJ r;
    r.x = x, r.y = y, r.z = fbn::load<fbn::PM>(fbn::PM::ONE);
    return r;
  }
  static FTS_DEV bool decode(const uint8_t* raw, F& x, F& y, bool& ident) {
    uint32_t pw[16];
    load_be_words(raw, pw);
    uint32_t nx[8], ny[8];
#pragma unroll
    for (int k = 0; k < 8; k++) nx[k] = pw[7 - k], ny[k] = pw[15 - k];
    ident = false;
    if (!p256::lt256(nx, fbn::PM::M) || !p256::lt256(ny, fbn::PM::M)) return false;
    x = p256::to_mont(fbn::load<fbn::PM>(nx));
    y = p256::to_mont(fbn::load<fbn::PM>(ny));
    return fbn::on_curve(x, y);
  }
  template <class Sink>
  // AMCL ECP.ToBytes(b, false): the point at infinity (held here as (0, 0)) is
  // AMCL's projective (0, 1, 0), which Affine() leaves as is -> 0x04 || 0 || 1
  static FTS_DEV void encode(Sink& s, const F& x, const F& y) {
    s.put_byte(0x04);
    const F ax = p256::from_mont(x);
    F ay = p256::from_mont(y);
    if (fbn::is_zero(ax) && fbn::is_zero(ay)) ay.v[0] = 1u;
    for (int k = 7; k >= 0; k--) s.put_word(ax.v[k]);
    for (int k = 7; k >= 0; k--) s.put_word(ay.v[k]);
  }
  static FTS_DEV void fixed_mul_acc(PJ& acc, const uint32_t* tables, int base, const uint32_t* k) {
    const uint32_t* tb = tables + (size_t)base * FBN_NW * FBN_ND * 16;
    for (int w = 0; w < FBN_NW; w++) {
      const uint32_t d = (k[w >> 1] >> (16 * (w & 1))) & 0xffffu;
      if (d) {
        const uint32_t* t = tb + ((size_t)w * FBN_ND + d) * 16;
        acc = fbn::pj_madd(acc, fbn::load<fbn::PM>(t), fbn::load<fbn::PM>(t + 8));
      }
    }
  }
  static FTS_DEV void decompose(const uint32_t k[8], uint32_t k1[4], uint32_t& s1, uint32_t k2[4], uint32_t& s2) {
    glv_decompose<fbn::GlvK>(k, k1, s1, k2, s2);
  }
  static FTS_DEV F beta() { return fbn::load<fbn::PM>(fbn::GlvK::BETA); }
  // (2^256 < 2 r: at most one subtraction)
  static FTS_DEV void digest_mod_r(const uint32_t st[8], uint32_t out[8]) {
    uint32_t t[8], bw = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = st[7 - i];
#pragma unroll
    for (int i = 0; i < 8; i++) t[i] = subb(out[i], fbn::RM::M[i], bw, bw);
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = bw ? out[i] : t[i];
  }
};

// ------------------------------------------------------------- Fr per curve
// Values are canonical LE limbs; `m` marks a Montgomery-form factor: mul(m, plain) is plain.
template <class CV>
struct Zr;
template <>
struct Zr<BnCurve> {
  using Z = Fr;
  static FTS_DEV Z ld(const uint32_t* p) {
    Z r;
#pragma unroll
    for (int k = 0; k < 8; k++) r.v[k] = p[k];
    return r;
  }
  static FTS_DEV Z add(const Z& a, const Z& b) { return f_add(a, b); }
  static FTS_DEV Z sub(const Z& a, const Z& b) { return f_sub(a, b); }
  static FTS_DEV Z neg(const Z& a) { return f_neg(a); }
  static FTS_DEV Z mul(const Z& a, const Z& b) { return f_mul(a, b); }
  static FTS_DEV Z to_mont(const Z& a) { return f_to_mont(a); }
  static FTS_DEV Z from_mont(const Z& a) { return f_from_mont(a); }
  static FTS_DEV Z inv_m(const Z& am) { return f_inv(am); }  // Montgomery in and out
};
template <>
struct Zr<FbnCurve> {
  using Z = p256::F<fbn::RM>;
  static FTS_DEV Z ld(const uint32_t* p) { return p256::load<fbn::RM>(p); }
  static FTS_DEV Z add(const Z& a, const Z& b) { return p256::add(a, b); }
  static FTS_DEV Z sub(const Z& a, const Z& b) { return p256::sub(a, b); }
  static FTS_DEV Z neg(const Z& a) {
    Z z;
#pragma unroll
    for (int k = 0; k < 8; k++) z.v[k] = 0u;
    return p256::sub(z, a);
  }
  static FTS_DEV Z mul(const Z& a, const Z& b) { return p256::mul(a, b); }
  static FTS_DEV Z to_mont(const Z& a) { return p256::to_mont(a); }
  static FTS_DEV Z from_mont(const Z& a) { return p256::from_mont(a); }
  // a^(r - 2), Montgomery in and out (r's top bit is set; r - 2 borrows nothing past limb 0)
  static FTS_DEV Z inv_m(const Z& am) {
    Z r = am;
#pragma unroll 1
    for (int bit = 254; bit >= 0; bit--) {
      r = p256::mul(r, r);
      const uint32_t e = bit < 32 ? fbn::RM::M[0] - 2u : fbn::RM::M[bit >> 5];
      if ((e >> (bit & 31)) & 1u) r = p256::mul(r, am);
    }
    return r;
  }
};

// ------------------------------------------------------------ lane scratch
// [unit][lane] layouts: neighbouring lanes touch neighbouring addresses
struct LaneWords {
  uint32_t* base;
  size_t L, lane;
  FTS_DEV uint32_t& at(size_t w) const { return base[w * L + lane]; }
};
// transcript bytes, [byte][lane]
struct ByteSink {
  uint8_t* base;
  size_t L, lane;
  uint32_t off = 0;
  FTS_DEV void put_byte(uint32_t b) { base[(size_t)(off++) * L + lane] = (uint8_t)b; }
  FTS_DEV void put_word(uint32_t w) {  // big-endian
    put_byte(w >> 24), put_byte(w >> 16), put_byte(w >> 8), put_byte(w);
  }
  FTS_DEV uint32_t word(uint32_t j) const {
    const uint8_t* p = base + (size_t)(4 * j) * L + lane;
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[L] << 16) | ((uint32_t)p[2 * L] << 8) | p[3 * L];
  }
};

}  // namespace idv
