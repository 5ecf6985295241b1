// Range-proof batch verification, the exact per-proof phase up to com: everything that
// is hashed (decode, challenges, H'_i, com on the work path and on the latency path).
// Launched by rp_pass.cpp (the table of kernels per stream is there).
#include "device/g1.hpp"
#include "device/fixed_base.hpp"
#include "device/glv.hpp"
#include "device/rp_kernels.hpp"
#include "device/rp_decls.hpp"
#include "device/transcript.hpp"
#include "device/helpers.hpp"
#include "../../include/fts_gpu.h"

namespace fts {

// ------------------------------------------------------------------ gather
// thread per (proof, 16-byte chunk) of the merged pass: raw points
// (npts x 64 B), canonical scalars (RP_NSC x 32 B), host verdicts, IPA flags
__global__ void __launch_bounds__(256) k_rp_gather(RpGather g, int npts, uint8_t* __restrict__ raw,
                                                   uint32_t* __restrict__ sc, int32_t* __restrict__ status,
                                                   int32_t* __restrict__ ipa) {
  wave_prio<PS_HEAD>();
  const int per = npts * 4 + RP_NSC * 2 + 1;  // uint4 chunks of raw, sc, + 1 lane for the two flags
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int B = g.off[g.G];
  if (gid >= (size_t)B * per) return;
  const int p = (int)(gid / per), c = (int)(gid % per);
  int q = 0;
  while (q + 1 < g.G && g.off[q + 1] <= p) q++;
  const int i = p - g.off[q];
  if (c < npts * 4) {
    reinterpret_cast<uint4*>(raw)[(size_t)p * npts * 4 + c] = reinterpret_cast<const uint4*>(g.raw[q])[(size_t)i * npts * 4 + c];
  } else if (c < npts * 4 + RP_NSC * 2) {
    const int cc = c - npts * 4;
    reinterpret_cast<uint4*>(sc)[(size_t)p * RP_NSC * 2 + cc] = reinterpret_cast<const uint4*>(g.sc[q])[(size_t)i * RP_NSC * 2 + cc];
  } else {
    status[p] = g.status0[q][i];
    ipa[p] = g.ipa[q][i];
  }
}

// ------------------------------------------------------------------ decode
// NewG1FromBytes (asn1.go:148 -> gnark SetBytes): 64 bytes, flag bits 00,
// canonical coordinates, on the curve; 64 zero bytes = identity.
__global__ void __launch_bounds__(256) k_rp_decode(int B, int npts, const uint8_t* __restrict__ raw,
                                                   uint32_t* __restrict__ pts, int32_t* __restrict__ status) {
  wave_prio<PS_HEAD>();
  int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= B * npts) return;
  G1A a;
  if (!decode_point(raw + (size_t)gid * 64, a)) status[gid / npts] = FTS_E_MALFORMED;
  store_g1a(pts + (size_t)gid * 16, a);
}

// -------------------------------------------------------------- challenges
// (k_rp_hash_small, the x / y / x_j transcripts, is in rp_x0.hip)
// thread per proof: z = Hz(Zb(y)), Montgomery forms, polEval, and one batch
// inversion (Montgomery trick) for y and the k round challenges
__global__ void __launch_bounds__(256) k_rp_chal_fr(int B, int n, int k, const int32_t* __restrict__ status,
                                                   uint32_t* __restrict__ ch, uint32_t* __restrict__ tmp) {
  wave_prio<PS_HEAD>();
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B || status[b] != 0) return;
  uint32_t* C = ch + (size_t)b * rp_nch(k) * 8;
  uint32_t* T = tmp + (size_t)b * (k + 1) * 8;  // prefix products
  Fr yc, xc;
  load_f(C + CH_Y * 8, yc);
  load_f(C + CH_X * 8, xc);
  uint32_t w[16], st[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = yc.v[7 - i];
  w[8] = 0x80000000u;
#pragma unroll
  for (int i = 9; i < 15; i++) w[i] = 0;
  w[15] = 256;
  sha256_init(st);
  sha256_compress(st, w);
  Fr z = f_to_mont(digest_to_fr(st));
  Fr y = f_to_mont(yc), x = f_to_mont(xc);
  Fr x2 = fr_sqr(x), z2 = fr_sqr(z), z3 = fr_mul(z2, z);
  // sum_{i<n} y^i by doubling (n = 2^k): S_2m = S_m (1 + y^m), y^2m = (y^m)^2
  // (same field element as the reference's loop, bulletproof.go:287-305)
  Fr ipy = f_one<FrP>(), ym = y;
  for (int m = 1; m < n; m <<= 1) {
    ipy = fr_mul(ipy, f_add(f_one<FrP>(), ym));
    ym = fr_sqr(ym);
  }
  // sum_{i<n} 2^i = 2^n - 1 (< r for n <= 64)
  Fr ip2 = f_zero<FrP>();
  ip2.v[0] = n >= 32 ? 0xffffffffu : (1u << n) - 1u;
  ip2.v[1] = n >= 64 ? 0xffffffffu : (n > 32 ? (1u << (n - 32)) - 1u : 0u);
  ip2 = f_to_mont(ip2);
  Fr pol = f_sub(fr_mul(f_sub(z, z2), ipy), fr_mul(z3, ip2));  // bulletproof.go:307-311
  store_f(C + CH_X * 8, x);
  store_f(C + CH_X2 * 8, x2);
  store_f(C + CH_Y * 8, y);
  store_f(C + CH_Z * 8, z);
  store_f(C + CH_Z2 * 8, z2);
  store_f(C + CH_POL * 8, pol);
  // batch inversion of v_0 = y, v_{1+j} = x_j (zeros invert to zero, as Fermat does)
  Fr acc = f_one<FrP>();
  for (int q = 0; q <= k; q++) {
    Fr v;
    if (q == 0) v = y;
    else {
      load_f(C + (CH_XJ + q - 1) * 8, v);
      v = f_to_mont(v);
      store_f(C + (CH_XJ + q - 1) * 8, v);
    }
    store_f(T + q * 8, acc);
    if (!f_is_zero(v)) acc = fr_mul(acc, v);
  }
  Fr inv = nl_fr_inv(acc);
  for (int q = k; q >= 0; q--) {
    Fr v, pre;
    if (q == 0) v = y;
    else load_f(C + (CH_XJ + q - 1) * 8, v);
    load_f(T + q * 8, pre);
    Fr vi = f_zero<FrP>();
    if (!f_is_zero(v)) {
      vi = fr_mul(inv, pre);
      inv = fr_mul(inv, v);
    }
    store_f(C + (q == 0 ? CH_YINV : CH_XJ + k + q - 1) * 8, vi);
  }
}

// lane per (chunk c of PW_CH indices, proof b), chunk-major: for i in the chunk
//   ypow[i][b] = y^-i                                 (bulletproof.go:483-485)
//   svec[i][b] = s_i = prod_j x_j^(+1 if bit k-1-j of i else -1)
// (the generator folding of ipa.go:343-356 unrolled: G_fin = sum s_i G_i,
// H'_fin = sum s_i^-1 H'_i = sum s_{n-1-i} H'_i).  The chunk's high index
// bits give a common prefix product; the low bits expand as a binary tree.
// (latency path, zvec != nullptr: also zvec[i][b] = z^2 2^i y^-i, the scalars of
// the com terms Z_i of k_rp_fixed_all)
__global__ void __launch_bounds__(64) k_rp_powers(int B, int n, int k, const int32_t* __restrict__ status,
                                                  const uint32_t* __restrict__ ch, uint32_t* __restrict__ ypow,
                                                  uint32_t* __restrict__ svec, uint32_t* __restrict__ zvec) {
  wave_prio<PS_HEAD>();
  const int lc = min(PW_LC, k), cs = 1 << lc, nch = n >> lc;
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= B * nch) return;
  const int c = gid / B, b = gid % B;
  if (status[b] != 0) return;
  const uint32_t* C = ch + (size_t)b * rp_nch(k) * 8;
  const int i0 = c * cs;
  Fr yinv;
  load_f(C + CH_YINV * 8, yinv);
  Fr yp = fr_pow_small(yinv, (uint32_t)i0);
  Fr zv;  // z^2 2^i
  if (zvec) {
    load_f(C + CH_Z2 * 8, zv);
    for (int i = 0; i < i0; i++) zv = f_add(zv, zv);
  }
  for (int q = 0; q < cs; q++) {
    if (q) yp = fr_mul(yp, yinv);
    store_f(ypow + ((size_t)(i0 + q) * B + b) * 8, yp);
    if (zvec) {
      store_f(zvec + ((size_t)(i0 + q) * B + b) * 8, fr_mul(zv, yp));
      zv = f_add(zv, zv);
    }
  }
  // prefix over the high bits: j = 0 .. k-1-lc  (bit k-1-j of i0)
  Fr pre = f_one<FrP>();
  for (int j = 0; j < k - lc; j++) {
    Fr f;
    load_f(C + (CH_XJ + (((i0 >> (k - 1 - j)) & 1) ? 0 : k) + j) * 8, f);
    pre = j ? fr_mul(pre, f) : f;
  }
  if (lc == PW_LC) {
    Fr v[PW_CH];
    v[0] = pre;
#pragma unroll
    for (int l = 0; l < PW_LC; l++) {  // low bits, MSB first: index 2t + bit
      const int j = k - PW_LC + l;
      Fr xj, xji;
      load_f(C + (CH_XJ + j) * 8, xj);
      load_f(C + (CH_XJ + k + j) * 8, xji);
#pragma unroll
      for (int t = (1 << l) - 1; t >= 0; t--) {
        const Fr base = v[t];
        v[2 * t + 1] = fr_mul(base, xj);
        v[2 * t] = fr_mul(base, xji);
      }
    }
#pragma unroll
    for (int q = 0; q < PW_CH; q++) store_f(svec + ((size_t)(i0 + q) * B + b) * 8, v[q]);
  } else {  // n < 8: one chunk, direct products
    for (int q = 0; q < cs; q++) {
      Fr sv = f_one<FrP>();
      for (int j = 0; j < k; j++) {
        Fr f;
        load_f(C + (CH_XJ + (((q >> (k - 1 - j)) & 1) ? 0 : k) + j) * 8, f);
        sv = fr_mul(sv, f);
      }
      store_f(svec + ((size_t)q * B + b) * 8, sv);
    }
  }
}

// ------------------------------------------------------------ H' and com
// com = x*D + C - z sum G_i + sum (z y^i + z^2 2^i) H'_i - delta*P   (bulletproof.go:477-492)
//     = x*D + C + z*K - delta*P + z^2 * S,   K = sum H_i - sum G_i,  S = sum_i 2^i H'_i
// (z y^i H'_i = z H_i folds into z K; the same group element, and only its
// affine form is observable).  S is a Horner sum over the exact H'_i, so
// the n fixed-base products of the com terms become one variable-base product.

// Jacobian -> affine (Montgomery, 16 words) and BE bytes of ONE point by its own
// inversion (identity -> (0, 0)): com at the end of its chain (round 5: instead of
// a k_rp_normalize launch of one point per proof on the critical path)
FTS_DEV void store_affine_one(const G1J& p, uint32_t* aff, uint8_t* be) {
  G1A r;
  if (f_is_zero(p.z)) {
    r.x = f_zero<FpP>();
    r.y = f_zero<FpP>();
  } else {
    const Fp zi = nl_fp_inv(p.z), zi2 = fp_sqr(zi);
    r.x = fp_mul(p.x, zi2);
    r.y = fp_mul(fp_mul(p.y, zi2), zi);
  }
  store_g1a(aff, r);
  store_point_be(be, r);
}

// lane per (proof, item): items 0..n-1: H'_i = y^-i H_i (-> hpj[b][i]);
// n: z K; n+1: -delta P (-> terms[b][0..1])
// wtables: the 20-bit tables of [H_0 .. H_{n-1}, K, P] (FbWide layout)
template <int W>
__global__ void __launch_bounds__(64, 4) k_rp_fixed_exact(int B, int n, int k, const int32_t* __restrict__ status,
                                                          const uint32_t* __restrict__ sc, const uint32_t* __restrict__ ch,
                                                          const uint32_t* __restrict__ ypow,
                                                          const uint32_t* __restrict__ wtables, uint32_t* __restrict__ hpj,
                                                          uint32_t* __restrict__ terms) {
  wave_prio<PS_FIXED>();
  const int ni = n + 2;
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (size_t)B * ni) return;
  // proof index fastest: a wave's 64 lanes gather from the same base's table (and
  // read ypow[t][b] coalesced): 6.9 -> 6.2 ms per 81,920-proof launch and 4.77 ->
  // 1.79 GB fetched against one proof's items side by side (round 2)
  const int b = (int)(gid % B), t = (int)(gid / B);
  if (status[b] != 0) return;
  const uint32_t* C = ch + (size_t)b * rp_nch(k) * 8;
  uint32_t* out;
  const uint32_t* tab;
  Scalar sk;
  if (t < n) {
    Fr yp;
    load_f(ypow + ((size_t)t * B + b) * 8, yp);
    tab = wtables + (size_t)t * FbCfg<W>::WORDS_PER_BASE;
    sk = fr_canon(yp);
    out = hpj + ((size_t)b * (n + 1) + t) * 24;
  } else if (t == n) {
    Fr z;
    load_f(C + CH_Z * 8, z);
    tab = wtables + (size_t)n * FbCfg<W>::WORDS_PER_BASE;
    sk = fr_canon(z);
    out = terms + ((size_t)b * COM_NTERMS + 0) * 24;
  } else {
    Fr d;
    load_f(sc + ((size_t)b * RP_NSC + RP_SC_DELTA) * 8, d);  // canonical
    Fr nd = f_neg(d);
#pragma unroll
    for (int q = 0; q < 8; q++) sk.v[q] = nd.v[q];
    tab = wtables + (size_t)(n + 1) * FbCfg<W>::WORDS_PER_BASE;
    out = terms + ((size_t)b * COM_NTERMS + 1) * 24;
  }
  G1J r = fb_mul_w<W>(tab, sk);
  store_g1j(out, r);
}

// lane per (proof, chunk c): S_c = sum_{j < 16} 2^j H'_{16c+j} (Horner over the
// Jacobian H' of k_rp_fixed_exact: full additions, so the chain does not wait for
// the H' normalisation, which runs beside it on the x0 stream)
__global__ void __launch_bounds__(256) k_rp_hsum_chunks(int B, int n, const int32_t* __restrict__ status,
                                                       const uint32_t* __restrict__ hpj, uint32_t* __restrict__ chunks) {
  wave_prio<PS_HSUM>();
  const int nc = (n + HS_CHUNK - 1) / HS_CHUNK;
  int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= B * nc) return;
  const int b = gid / nc, c = gid % nc;
  if (status[b] != 0) return;
  const int lo = c * HS_CHUNK, hi = min(n, lo + HS_CHUNK);
  const uint32_t* H = hpj + (size_t)b * (n + 1) * 24;  // Jacobian H'
  G1J acc = load_g1j(H + (hi - 1) * 24);
  for (int i = hi - 2; i >= lo; i--) {
    acc = g1j_dbl(acc);
    add_inl(acc, load_g1j(H + i * 24));
  }
  store_g1j(chunks + (size_t)gid * 24, acc);
}

// lane per proof: S = sum_c 2^(16c) S_c (Horner over k_rp_hsum_chunks' chunk sums,
// 3 x (16 doublings + 1 addition) at n = 64) -> slot 0 of the proof's chunks.
// Once per proof: the two lanes of k_rp_com_var used to join S each, 17 % of
// their chain
__global__ void __launch_bounds__(256) k_rp_hsum_join(int B, int n, const int32_t* __restrict__ status,
                                                     uint32_t* __restrict__ chunks) {
  wave_prio<PS_HSUM>();
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B || status[b] != 0) return;
  const int nc = (n + HS_CHUNK - 1) / HS_CHUNK;
  uint32_t* Sc = chunks + (size_t)b * nc * 24;
  G1J S = load_g1j(Sc + (nc - 1) * 24);
  for (int c = nc - 2; c >= 0; c--) {
    for (int q = 0; q < HS_CHUNK; q++) S = g1j_dbl(S);
    add_inl(S, load_g1j(Sc + c * 24));
  }
  store_g1j(Sc, S);
}

// The affine tables of the com chain (glv.hpp CTab), one per proof: 1..8 D in rows
// 0..7, 1..8 S (S from k_rp_hsum_join) in rows 8..15, each normalised with one
// inversion.  The first half of the grid's blocks builds D's rows (D is affine: a
// mixed doubling and mixed additions), the second half S's (full additions), so every
// wave runs one instruction stream; the chain reads the rows after the launch
// boundary (no fence, no barrier).  Launched with 2 * ceil(B / blockDim.x) blocks
__global__ void __launch_bounds__(256) k_rp_com_tab(int B, int n, int k, const int32_t* __restrict__ status,
                                                   const uint32_t* __restrict__ pts,
                                                   const uint32_t* __restrict__ chunks, uint32_t* __restrict__ atab) {
  wave_prio<PS_COMVAR>();
  const int nb = gridDim.x >> 1;
  const bool h = (int)blockIdx.x >= nb;
  const int b = ((int)blockIdx.x - (h ? nb : 0)) * blockDim.x + threadIdx.x;
  if (b >= B || status[b] != 0) return;
  const CTab T{atab, (size_t)B, (size_t)b};
  if (!h) {
    const G1A Da = load_g1a(pts + ((size_t)b * rp_npts(k) + RP_PT_D) * 16);
    ctab_build8<true>(T, 0, g1j_from_affine(Da), g1a_is_identity(Da));
  } else {
    const int nc = (n + HS_CHUNK - 1) / HS_CHUNK;
    const G1J S = load_g1j(chunks + (size_t)b * nc * 24);
    ctab_build8<false>(T, 8, S, f_is_zero(S.z));
  }
}

// com = C + z K - delta P + x D + z^2 S (bulletproof.go:477-492), one lane per
// proof: with x = x1 + x2 lambda and z^2 = w1 + w2 lambda (GLV), x D + z^2 S =
// x1 D + x2 phi(D) + w1 S + w2 phi(S) is ONE joint Straus chain over the proof's
// table (glv.hpp straus4_ctab; k_rp_com_tab built it), 124 doublings where a lane
// per phi half doubled 2 x 124 times; then the fixed-base terms z K, -delta P
// (k_rp_fixed_exact -> terms[b][0..1]) and C, and com's own normalisation
#ifndef FTS_COMVAR_OCC
#define FTS_COMVAR_OCC 3  // waves per SIMD the register budget allows (A/B builds: -DFTS_COMVAR_OCC=4)
#endif
__global__ void __launch_bounds__(256, FTS_COMVAR_OCC) k_rp_com_var(int B, int n, int k, const int32_t* __restrict__ status,
                                                   const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ch,
                                                   const uint32_t* __restrict__ chunks, uint32_t* __restrict__ atab,
                                                   const uint32_t* __restrict__ terms, uint32_t* __restrict__ hpj,
                                                   uint32_t* __restrict__ hpa, uint8_t* __restrict__ hp_be) {
  wave_prio<PS_COMVAR>();
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B || status[b] != 0) return;
  const uint32_t* C = ch + (size_t)b * rp_nch(k) * 8;
  Fr x, z2;
  load_f(C + CH_X * 8, x);
  load_f(C + CH_Z2 * 8, z2);
  uint32_t xa[4], xb[4], xs0, xs1, wa[4], wb[4], ws0, ws1;
  glv_decompose(fr_canon(x).v, xa, xs0, xb, xs1);
  glv_decompose(fr_canon(z2).v, wa, ws0, wb, ws1);
  const int nc = (n + HS_CHUNK - 1) / HS_CHUNK;
  // the identity flags as k_rp_com_tab saw them: S's z (k_rp_hsum_join), D's coordinates
  Fp sz;
  load_fp(chunks + (size_t)b * nc * 24 + 16, sz);
  const bool idS = f_is_zero(sz);
  const bool idD = g1a_is_identity(load_g1a(pts + ((size_t)b * rp_npts(k) + RP_PT_D) * 16));
  const CTab T{atab, (size_t)B, (size_t)b};
  G1J r = straus4_ctab(T, xa, xs0 != 0, xb, xs1 != 0, wa, ws0 != 0, wb, ws1 != 0, idD, idS);
  // + z K - delta P + C: three full additions through ONE add_inl body (a second
  // madd_inl copy for the affine C would cost more code than its 5 products save)
#pragma unroll 1
  for (int h = 0; h < 3; h++) {
    G1J t;
    if (h < 2) t = load_g1j(terms + ((size_t)b * COM_NTERMS + h) * 24);
    else t = g1j_from_affine(load_g1a(pts + ((size_t)b * rp_npts(k) + RP_PT_C) * 16));
    add_inl(r, t);
  }
  const size_t q = (size_t)b * (n + 1) + n;
  store_g1j(hpj + q * 24, r);
  store_affine_one(r, hpa + q * 16, hp_be + q * 64);  // com for the x0 suffix (no normalize_com launch)
}

// ----------------------------------------- com, latency path (small passes)
// The same group element as the work path below/above, computed without a
// per-proof doubling chain on the critical path (bulletproof.go:477-492):
//   com = C + x*D + z*K - delta*P + sum_i (z^2 2^i y^-i) H_i
// (z^2 2^i H'_i = z^2 2^i y^-i H_i): the n z^2-terms become fixed-base products
// on the 20-bit tables of H_i, computed by the same lanes as the H'_i
// (k_rp_fixed_all: two products per lane, same table), summed by an LDS tree
// (k_rp_com_tree); x*D runs beside them on the side stream (k_rp_xd, one GLV
// half per lane, started right after the x transcript).  ~3.8 k more products
// per rp64 than the work path, but every product runs at the fixed-base
// kernels' occupancy: used for passes of up to FTS_COM_FIXED_MAX proofs, where
// the work path's per-proof chains leave most SIMDs idle.

// lane per (item, proof), proof index fastest (a wave's 64 lanes gather from
// the same table), one fixed-base product per lane: items i < n: H'_i = y^-i H_i
// -> hpj[b][i]; items n + i: Z_i = (z^2 2^i y^-i) H_i -> terms[b][i]; item 2n:
// z K -> terms[b][n]; item 2n + 1: -delta P -> terms[b][n + 1]
template <int W>
__global__ void __launch_bounds__(64, 4) k_rp_fixed_all(int B, int n, int k, const int32_t* __restrict__ status,
                                                        const uint32_t* __restrict__ sc, const uint32_t* __restrict__ ch,
                                                        const uint32_t* __restrict__ ypow,
                                                        const uint32_t* __restrict__ zvec,
                                                        const uint32_t* __restrict__ wtables, uint32_t* __restrict__ hpj,
                                                        uint32_t* __restrict__ terms) {
  wave_prio<PS_FIXED>();
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (size_t)(2 * n + 2) * B) return;
  const int t = (int)(gid / B), b = (int)(gid % B);
  if (status[b] != 0) return;
  const uint32_t* C = ch + (size_t)b * rp_nch(k) * 8;
  const int base = t < n ? t : t - n;  // H_i (i < n), K (n), P (n + 1)
  Scalar sk;
  if (t < 2 * n) {
    Fr v;
    load_f((t < n ? ypow : zvec) + ((size_t)base * B + b) * 8, v);
    sk = fr_canon(v);
  } else if (t == 2 * n) {
    Fr z;
    load_f(C + CH_Z * 8, z);
    sk = fr_canon(z);
  } else {
    Fr d;
    load_f(sc + ((size_t)b * RP_NSC + RP_SC_DELTA) * 8, d);  // canonical
    const Fr nd = f_neg(d);
#pragma unroll
    for (int q = 0; q < 8; q++) sk.v[q] = nd.v[q];
  }
  const G1J r = fb_mul_w<W>(wtables + (size_t)base * FbCfg<W>::WORDS_PER_BASE, sk);
  uint32_t* out = t < n ? hpj + ((size_t)b * (n + 1) + t) * 24 : terms + ((size_t)b * com_fx_slots(n) + base) * 24;
  store_g1j(out, r);
}

// x*D (bulletproof.go:478), one GLV half per lane: x = x1 + x2 lambda, lane h
// computes x_h phi^h(D) -> terms[b][n + 2 + h]; lane tables 1..8 * P in vtab.
// x is read from the digest k_rp_hash_small left at the head of its slot
// (canonical), so this runs concurrently with k_rp_chal_fr.
__global__ void __launch_bounds__(256) k_rp_xd(int B, int n, int k, const int32_t* __restrict__ status,
                                              const uint32_t* __restrict__ pts, const uint8_t* __restrict__ small_msgs,
                                              uint32_t* __restrict__ vtab, uint32_t* __restrict__ terms, int tstride,
                                              int toff) {
  wave_prio<PS_COMVAR>();
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= 2 * B) return;
  const int h = gid / B, b = gid % B;
  if (status[b] != 0) return;
  Fr x;
  load_f(reinterpret_cast<const uint32_t*>(small_msgs + (size_t)b * (2 + k) * SMALL_SLOT), x);
  uint32_t xk[2][4], xs[2];
  glv_decompose(x.v, xk[0], xs[0], xk[1], xs[1]);
  G1J D = g1j_from_affine(load_g1a(pts + ((size_t)b * rp_npts(k) + RP_PT_D) * 16));
  if (h) D.x = fp_mul(D.x, glv_beta());
  if (xs[h]) D.y = f_neg(D.y);
  const G1J r = vb128j(D, xk[h], vtab, (size_t)2 * B, (size_t)gid);
  store_g1j(terms + ((size_t)b * tstride + toff + h) * 24, r);
}

// com = C + sum of the n + 4 terms: CT_LANES lanes per proof (CT_PROOFS proofs
// per block), lane l sums slots l, l + CT_LANES, ... (5 full additions at
// n = 64), then a log2(CT_LANES)-level LDS tree -> hpj[b][n]
__global__ void __launch_bounds__(CT_LANES * CT_PROOFS) k_rp_com_tree(int B, int n, int k,
                                                                      const int32_t* __restrict__ status,
                                                                      const uint32_t* __restrict__ pts,
                                                                      const uint32_t* __restrict__ terms,
                                                                      uint32_t* __restrict__ hpj,
                                                                      uint32_t* __restrict__ hpa,
                                                                      uint8_t* __restrict__ hp_be) {
  wave_prio<PS_COMVAR>();
  __shared__ uint32_t sh[CT_LANES * CT_PROOFS * 24];
  const int l = threadIdx.x % CT_LANES, pl = threadIdx.x / CT_LANES;
  const int b = blockIdx.x * CT_PROOFS + pl;
  const bool live = b < B && status[b] == 0;
  const int ns = com_fx_slots(n);
  G1J acc = g1j_identity();
  if (live) {
    const uint32_t* T = terms + (size_t)b * ns * 24;
    if (l == 0) acc = g1j_from_affine(load_g1a(pts + ((size_t)b * rp_npts(k) + RP_PT_C) * 16));
    for (int q = l; q < ns; q += CT_LANES) add_inl(acc, load_g1j(T + q * 24));
  }
  uint32_t* S = sh + (size_t)pl * CT_LANES * 24;
  store_g1j(S + l * 24, acc);
  __syncthreads();
  for (int half = CT_LANES / 2; half >= 1; half >>= 1) {
    if (live && l < half) add_inl(acc, load_g1j(S + (l + half) * 24));
    __syncthreads();
    if (live && l < half) store_g1j(S + l * 24, acc);
    __syncthreads();
  }
  if (live && l == 0) {
    const size_t q = (size_t)b * (n + 1) + n;
    store_g1j(hpj + q * 24, acc);
    store_affine_one(acc, hpa + q * 16, hp_be + q * 64);
  }
}

// the wide-table instances rp_pass.cpp launches (device/rp_decls.hpp)
template __global__ void k_rp_fixed_exact<FBW_W>(int, int, int, const int32_t*, const uint32_t*, const uint32_t*,
                                                 const uint32_t*, const uint32_t*, uint32_t*, uint32_t*);
template __global__ void k_rp_fixed_exact<22>(int, int, int, const int32_t*, const uint32_t*, const uint32_t*,
                                              const uint32_t*, const uint32_t*, uint32_t*, uint32_t*);
template __global__ void k_rp_fixed_all<FBW_W>(int, int, int, const int32_t*, const uint32_t*, const uint32_t*,
                                               const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*, uint32_t*);
template __global__ void k_rp_fixed_all<22>(int, int, int, const int32_t*, const uint32_t*, const uint32_t*,
                                            const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*, uint32_t*);

hipError_t upload_wave_prio_rp_exact(const int* p) { return upload_wave_prio(p); }

}  // namespace fts
