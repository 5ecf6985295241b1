// FP256BN variable-base product by GLV for the nym kernels: e * Q with
// e = k1 + k2 lambda, one joint chain of k1 (+-Q) + k2 (+-phi(Q)) over 33 signed
// 4-bit windows (|k_i| < 2^128), 128 doublings instead of 252.  The lane's 16-entry
// Jacobian table (1..8 of both points) lives in global memory, [entry][word][stride]
// (as glv.hpp's vtab for BN254): 16 x 24 words per lane.
#pragma once
#include "fp256bn.hpp"
#include "glv.hpp"  // glv_decompose

namespace fbn {

__device__ inline void vtab_store(uint32_t* __restrict__ tab, size_t stride, size_t idx, int e, const PJ& p) {
#pragma unroll
  for (int k = 0; k < 8; k++) {
    tab[((size_t)(e * 24) + k) * stride + idx] = p.x.v[k];
    tab[((size_t)(e * 24) + 8 + k) * stride + idx] = p.y.v[k];
    tab[((size_t)(e * 24) + 16 + k) * stride + idx] = p.z.v[k];
  }
}
__device__ inline PJ vtab_load(const uint32_t* __restrict__ tab, size_t stride, size_t idx, int e) {
  PJ p;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    p.x.v[k] = tab[((size_t)(e * 24) + k) * stride + idx];
    p.y.v[k] = tab[((size_t)(e * 24) + 8 + k) * stride + idx];
    p.z.v[k] = tab[((size_t)(e * 24) + 16 + k) * stride + idx];
  }
  return p;
}
// signed 4-bit recoding of a 128-bit magnitude over 33 windows (window 32 = the carry)
__device__ inline uint64_t recode(const uint32_t s[4]) {  // bit w = carry into window w
  uint64_t cm = 0;
  uint32_t c = 0;
#pragma unroll
  for (int w = 0; w < 33; w++) {
    cm |= (uint64_t)c << w;
    const uint32_t raw = w < 32 ? (s[w >> 3] >> (4 * (w & 7))) & 15u : 0u;
    c = raw + c > 8u;
  }
  return cm;
}
__device__ inline int digit(const uint32_t s[4], uint64_t cm, int w) {  // in [-8, 8]
  const int raw = w < 32 ? (int)((s[w >> 3] >> (4 * (w & 7))) & 15u) : 0;
  const int cin = (int)((cm >> w) & 1u);
  const int cout = w < 32 ? (int)((cm >> (w + 1)) & 1u) : 0;
  return raw + cin - 16 * cout;
}

// e * Q: Q = (Qx, Qy) affine Montgomery on the curve, e canonical LE limbs below r;
// vtab + idx with `stride` lanes per word: the lane's table
FTS_DEV PJ glv_mul_tab(const Fp& Qx, const Fp& Qy, const uint32_t e[8], uint32_t* __restrict__ vtab, size_t stride,
                       size_t idx) {
  uint32_t k1[4], k2[4], s1, s2;
  fts::glv_decompose<GlvK>(e, k1, s1, k2, s2);
  const Fp nQy = sub(Fp{}, Qy);
  const Fp Px = Qx, Py = s1 ? nQy : Qy;
  const Fp Ex = mul(Qx, load<PM>(GlvK::BETA)), Ey = s2 ? nQy : Qy;
  {
    PJ cp, ce;
    cp.x = Px, cp.y = Py, cp.z = load<PM>(PM::ONE);
    ce.x = Ex, ce.y = Ey, ce.z = cp.z;
    vtab_store(vtab, stride, idx, 0, cp);
    vtab_store(vtab, stride, idx, 8, ce);
    for (int k = 1; k < 8; k++) {
      cp = pj_madd(cp, Px, Py);
      ce = pj_madd(ce, Ex, Ey);
      vtab_store(vtab, stride, idx, k, cp);
      vtab_store(vtab, stride, idx, 8 + k, ce);
    }
  }
  const uint64_t ca = recode(k1), cb = recode(k2);
  PJ vb = pj_inf();
  for (int w = 32; w >= 0; w--) {
    const int da = digit(k1, ca, w), db = digit(k2, cb, w);
    PJ qa, qb;
    if (da) qa = vtab_load(vtab, stride, idx, (da < 0 ? -da : da) - 1);
    if (db) qb = vtab_load(vtab, stride, idx, 8 + (db < 0 ? -db : db) - 1);
    if (w != 32) vb = pj_dbl(pj_dbl(pj_dbl(pj_dbl(vb))));
    if (da) {
      if (da < 0) qa.y = sub(Fp{}, qa.y);
      vb = pj_add(vb, qa);
    }
    if (db) {
      if (db < 0) qb.y = sub(Fp{}, qb.y);
      vb = pj_add(vb, qb);
    }
  }
  return vb;
}

}  // namespace fbn
