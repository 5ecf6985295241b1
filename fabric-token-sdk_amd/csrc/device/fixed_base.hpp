// Fixed-base scalar multiplication over device-resident window tables.
//
// Every public generator the verifier multiplies (H_i, G_i, ped0..2, P, Q,
// K = sum H_i - sum G_i) gets a table
//     T[w][d-1] = d * 2^(FB_W * w) * B,   d = 1 .. 2^(FB_W-1),  w < FB_NW
// of affine Montgomery points (16 words).  A canonical scalar k < r < 2^254
// is recoded into FB_NW signed FB_W-bit digits, so k*B costs FB_NW mixed
// additions and no doublings.  With FB_W = 16 that is 16 additions per
// product (32 with byte windows) for 32 MiB of table per base: the
// 134 bases of a 64-bit context take 4.3 GiB of HBM, which the 288 GB part
// affords; every lookup is one 64-byte gather.
//
// The multiplication loop is fully inlined (no out-of-line calls: the call
// ABI would spill the accumulator to scratch on every addition) and
// prefetches the next table entry while the current addition runs.
//
// A product is a sum of table entries with no doubling, so its accumulator is
// extended Jacobian (G1X, g1.hpp: 10 products per mixed addition instead of 11);
// every entry point still returns or updates a G1J (g1x_to_jac, 2 products).
#pragma once
#include "g1.hpp"

namespace fts {

constexpr int FB_W = 16;                                   // window bits
constexpr int FB_NW = (255 + FB_W - 1) / FB_W;             // windows (covers 255 bits)
constexpr int FB_E = 1 << (FB_W - 1);                      // entries per window
constexpr size_t FB_WORDS_PER_BASE = (size_t)FB_NW * FB_E * 16;
// two-level construction of a window: d - 1 = hi * FB_S + lo
constexpr int FB_S = 1 << ((FB_W) / 2);                    // small multiples per window
constexpr int FB_L = FB_E / FB_S;                          // large multiples per window

// The same layout for any window width W.  The per-proof bases of the
// range-proof pipeline (H_i, K, P: the n + 2 fixed-base products of every
// proof) use FBW_W = 20-bit windows: 13 mixed additions per product instead
// of 16, for 436 MiB per base (28.8 GiB at n = 64 -- the 288 GB part holds it).
template <int W>
struct FbCfg {
  static constexpr int NW = (255 + W - 1) / W;
  static constexpr int E = 1 << (W - 1);
  static constexpr size_t WORDS_PER_BASE = (size_t)NW * E * 16;
  static constexpr int S = 1 << (W / 2);
  static constexpr int L = E / S;
};
constexpr int FBW_W = 20;
using FbWide = FbCfg<FBW_W>;

// next signed digit of k (LSB first): consumes FB_W bits of s (shifted in
// place: constant register indices, no scratch), carry in/out via `carry`
FTS_DEV int fb_next_digit(uint32_t s[8], int& carry) {
  int d = (int)(s[0] & (uint32_t)(2 * FB_E - 1)) + carry;
#pragma unroll
  for (int i = 0; i < 7; i++) s[i] = (s[i] >> FB_W) | (s[i + 1] << (32 - FB_W));
  s[7] >>= FB_W;
  carry = d > FB_E;
  return carry ? d - 2 * FB_E : d;
}

// p += q (q affine, not the identity): madd-2007-bl, inlined
FTS_DEV void madd_inl(G1J& p, const G1A& q) {
  if (f_is_zero(p.z)) {
    p.x = q.x;
    p.y = q.y;
    p.z = f_one<FpP>();
    return;
  }
  Fp z1z1 = fp_sqr(p.z);
  Fp u2 = fp_mul(q.x, z1z1);
  Fp s2 = fp_mul(fp_mul(q.y, p.z), z1z1);
  Fp h = f_sub(u2, p.x);
  Fp rr = f_sub(s2, p.y);
  if (f_is_zero(h)) {  // P == +-Q: exceptional, out of line
    p = f_is_zero(rr) ? g1j_dbl(p) : g1j_identity();
    return;
  }
  Fp hh = fp_sqr(h);
  Fp i = f_dbl(f_dbl(hh));
  Fp j = fp_mul(h, i);
  rr = f_dbl(rr);
  Fp v = fp_mul(p.x, i);
  Fp x3 = f_sub(f_sub(fp_sqr(rr), j), f_dbl(v));
  Fp y3 = f_sub(fp_mul(rr, f_sub(v, x3)), f_dbl(fp_mul(p.y, j)));
  p.z = f_sub(f_sub(fp_sqr(f_add(p.z, h)), z1z1), hh);
  p.x = x3;
  p.y = y3;
}

// p += q (both Jacobian): add-2007-bl, inlined (exceptional cases inline too,
// so the caller's loop never makes an out-of-line call)
FTS_DEV void add_inl(G1J& p, const G1J& q) {
  if (f_is_zero(q.z)) return;
  if (f_is_zero(p.z)) {
    p = q;
    return;
  }
  Fp z1z1 = fp_sqr(p.z);
  Fp z2z2 = fp_sqr(q.z);
  Fp u1 = fp_mul(p.x, z2z2);
  Fp u2 = fp_mul(q.x, z1z1);
  Fp s1 = fp_mul(fp_mul(p.y, q.z), z2z2);
  Fp s2 = fp_mul(fp_mul(q.y, p.z), z1z1);
  Fp h = f_sub(u2, u1);
  Fp rr = f_sub(s2, s1);
  if (f_is_zero(h)) {
    p = f_is_zero(rr) ? g1j_dbl(p) : g1j_identity();
    return;
  }
  Fp i = fp_sqr(f_dbl(h));
  Fp j = fp_mul(h, i);
  rr = f_dbl(rr);
  Fp v = fp_mul(u1, i);
  Fp x3 = f_sub(f_sub(fp_sqr(rr), j), f_dbl(v));
  Fp y3 = f_sub(fp_mul(rr, f_sub(v, x3)), f_dbl(fp_mul(s1, j)));
  p.z = fp_mul(f_sub(f_sub(fp_sqr(f_add(p.z, q.z)), z1z1), z2z2), h);
  p.x = x3;
  p.y = y3;
}

// p += q (q affine, not the identity) in XYZZ: madd-2008-s, inlined.  The
// exceptional cases are those of madd_inl and stay off the straight-line path
FTS_DEV void xmadd_inl(G1X& p, const G1A& q) {
  if (f_is_zero(p.zz)) {
    p.x = q.x;
    p.y = q.y;
    p.zz = f_one<FpP>();
    p.zzz = f_one<FpP>();
    return;
  }
  Fp u2 = fp_mul(q.x, p.zz);
  Fp s2 = fp_mul(q.y, p.zzz);
  Fp h = f_sub(u2, p.x);
  Fp rr = f_sub(s2, p.y);
  if (f_is_zero(h)) {  // P == +-Q: exceptional, out of line
    p = f_is_zero(rr) ? g1x_dbl(p) : g1x_identity();
    return;
  }
  Fp hh = fp_sqr(h);
  Fp hhh = fp_mul(h, hh);
  Fp v = fp_mul(p.x, hh);
  Fp x3 = f_sub(f_sub(fp_sqr(rr), hhh), f_dbl(v));
  Fp y3 = f_sub(fp_mul(rr, f_sub(v, x3)), fp_mul(p.y, hhh));
  p.zz = fp_mul(p.zz, hh);
  p.zzz = fp_mul(p.zzz, hhh);
  p.x = x3;
  p.y = y3;
}

// p += q, both XYZZ: add-2008-s, inlined
FTS_DEV void xadd_inl(G1X& p, const G1X& q) {
  if (f_is_zero(q.zz)) return;
  if (f_is_zero(p.zz)) {
    p = q;
    return;
  }
  Fp u1 = fp_mul(p.x, q.zz);
  Fp u2 = fp_mul(q.x, p.zz);
  Fp s1 = fp_mul(p.y, q.zzz);
  Fp s2 = fp_mul(q.y, p.zzz);
  Fp h = f_sub(u2, u1);
  Fp rr = f_sub(s2, s1);
  if (f_is_zero(h)) {
    p = f_is_zero(rr) ? g1x_dbl(p) : g1x_identity();
    return;
  }
  Fp hh = fp_sqr(h);
  Fp hhh = fp_mul(h, hh);
  Fp v = fp_mul(u1, hh);
  Fp x3 = f_sub(f_sub(fp_sqr(rr), hhh), f_dbl(v));
  Fp y3 = f_sub(fp_mul(rr, f_sub(v, x3)), fp_mul(s1, hhh));
  p.zz = fp_mul(fp_mul(p.zz, q.zz), hh);
  p.zzz = fp_mul(fp_mul(p.zzz, q.zzz), hhh);
  p.x = x3;
  p.y = y3;
}

FTS_DEV G1A fb_entry(const uint32_t* __restrict__ table, int w, int d) {
  const int ad = d < 0 ? -d : d;
  G1A q = load_g1a(table + ((size_t)w * FB_E + (ad - 1)) * 16);
  if (d < 0) q.y = f_neg(q.y);
  return q;
}

// ka * A + kb * B over two 16-bit-window tables in ONE accumulator: a
// fixed-base product is a sum of table entries (no doublings), so the joint sum
// takes the two products' additions with no final full addition; the next
// window's entries are loaded during the current window's additions
FTS_DEV G1J fb_mul2(const uint32_t* __restrict__ ta, const Scalar& ka, const uint32_t* __restrict__ tb,
                    const Scalar& kb) {
  uint32_t sa[8], sb[8];
#pragma unroll
  for (int i = 0; i < 8; i++) sa[i] = ka.v[i], sb[i] = kb.v[i];
  G1X acc = g1x_identity();
  int ca = 0, cb = 0;
  int da = fb_next_digit(sa, ca), db = fb_next_digit(sb, cb);
  G1A qa, qb;
  if (da != 0) qa = fb_entry(ta, 0, da);
  if (db != 0) qb = fb_entry(tb, 0, db);
  for (int w = 0; w < FB_NW; w++) {
    int dan = 0, dbn = 0;
    G1A na, nb;
    if (w + 1 < FB_NW) {
      dan = fb_next_digit(sa, ca);
      dbn = fb_next_digit(sb, cb);
      if (dan != 0) na = fb_entry(ta, w + 1, dan);
      if (dbn != 0) nb = fb_entry(tb, w + 1, dbn);
    }
    if (da != 0) xmadd_inl(acc, qa);
    if (db != 0) xmadd_inl(acc, qb);
    da = dan, db = dbn, qa = na, qb = nb;
  }
  return g1x_to_jac(acc);
}

// digits and entries of a width-W table (FbCfg<W> layout)
template <int W>
FTS_DEV int fb_next_digit_w(uint32_t s[8], int& carry) {
  constexpr int E = FbCfg<W>::E;
  int d = (int)(s[0] & (uint32_t)(2 * E - 1)) + carry;
#pragma unroll
  for (int i = 0; i < 7; i++) s[i] = (s[i] >> W) | (s[i + 1] << (32 - W));
  s[7] >>= W;
  carry = d > E;
  return carry ? d - 2 * E : d;
}
template <int W>
FTS_DEV G1A fb_entry_w(const uint32_t* __restrict__ table, int w, int d) {
  const int ad = d < 0 ? -d : d;
  G1A q = load_g1a(table + ((size_t)w * FbCfg<W>::E + (ad - 1)) * 16);
  if (d < 0) q.y = f_neg(q.y);
  return q;
}
// the sum of the table entries of k's non-zero digits over a width-W table, in
// XYZZ (xmadd_inl: 10 products per entry after the first, which is a copy)
template <int W>
FTS_DEV G1X fb_sum_w(const uint32_t* __restrict__ table, const Scalar& k) {
  constexpr int NW = FbCfg<W>::NW;
  uint32_t s[8];
#pragma unroll
  for (int i = 0; i < 8; i++) s[i] = k.v[i];
  G1X acc = g1x_identity();
  int carry = 0, w = 0, d = 0;
  // first nonzero digit
  for (; w < NW; w++) {
    d = fb_next_digit_w<W>(s, carry);
    if (d != 0) break;
  }
  if (w == NW) return acc;
  G1A cur = fb_entry_w<W>(table, w, d);
  for (;;) {
    int wn = w + 1, dn = 0;
    for (; wn < NW; wn++) {
      dn = fb_next_digit_w<W>(s, carry);
      if (dn != 0) break;
    }
    G1A nxt;
    if (wn < NW) nxt = fb_entry_w<W>(table, wn, dn);  // in flight during the addition
    xmadd_inl(acc, cur);
    if (wn >= NW) break;
    cur = nxt;
    w = wn;
  }
  return acc;
}
// k * B over a width-W table: the XYZZ sum handed on as a Jacobian point (2 products)
template <int W>
FTS_DEV G1J fb_mul_w(const uint32_t* __restrict__ table, const Scalar& k) {
  return g1x_to_jac(fb_sum_w<W>(table, k));
}

// acc += k * B over a width-W table (FbCfg<W> layout): the product is summed in
// an XYZZ accumulator of its own and joins acc by one full addition
template <int W>
FTS_DEV void fb_mul_acc_w(G1J& acc, const uint32_t* __restrict__ table, const Scalar& k) {
  const G1X s = fb_sum_w<W>(table, k);
  if (f_is_zero(s.zz)) return;
  add_inl(acc, g1x_to_jac(s));
}
// acc += k * B over a 16-bit window table
FTS_DEV void fb_mul_acc(G1J& acc, const uint32_t* __restrict__ table, const Scalar& k) {
  fb_mul_acc_w<FB_W>(acc, table, k);
}

// acc += k * B over a 16-bit window table with every entry added straight into
// the Jacobian accumulator (madd_inl, 11 products per window): for a kernel whose
// register budget has no room for the XYZZ sum beside its accumulator
// (idv_kernels.hpp k_idv_var: 155 -> 179 VGPRs, 3 -> 2 waves per SIMD with it)
FTS_DEV void fb_mul_acc_jac(G1J& acc, const uint32_t* __restrict__ table, const Scalar& k) {
  uint32_t s[8];
#pragma unroll
  for (int i = 0; i < 8; i++) s[i] = k.v[i];
  int carry = 0, w = 0, d = 0;
  for (; w < FB_NW; w++) {
    d = fb_next_digit(s, carry);
    if (d != 0) break;
  }
  if (w == FB_NW) return;
  G1A cur = fb_entry(table, w, d);
  for (;;) {
    int wn = w + 1, dn = 0;
    for (; wn < FB_NW; wn++) {
      dn = fb_next_digit(s, carry);
      if (dn != 0) break;
    }
    G1A nxt;
    if (wn < FB_NW) nxt = fb_entry(table, wn, dn);  // in flight during the addition
    madd_inl(acc, cur);
    if (wn >= FB_NW) break;
    cur = nxt;
    w = wn;
  }
}

// k * B for a canonical scalar k (8 LE limbs), 16-bit window table
FTS_DEV G1J fb_mul(const uint32_t* __restrict__ table, const Scalar& k) { return fb_mul_w<FB_W>(table, k); }

// out-of-line copy for cold call sites (keeps their kernels small)
__device__ __noinline__ G1J nl_fb_mul(const uint32_t* __restrict__ table, Scalar k) { return fb_mul(table, k); }

}  // namespace fts
