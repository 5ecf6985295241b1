// Idemix credentials verified on the device: the check KeyManager construction makes of a
// signer config (token/services/identity/idemix/km.go:117-133 -> IBM/idemix Credential.Ver,
// restated in oracle/idemix_identity.py credential_b / credential_pairing_ok), up to the
// inputs of the pairing stage that k_idv_pairing and k_idv_bp_* (idv_kernels.hpp) run for
// the identities' proofs.
//
// Credential.Ver checks B = g1 + HRand S + HSk sk + sum HAttrs[i] attrs[i], then
// e(W + g2 E, A) = e(g2, B).  By bilinearity the second is
//   e(W, A) e(g2, E A - B) = 1,
// the shape of the identity verifier's e(W, A') e(g2, -ABar) = 1: the fixed G2 arguments
// whose lines the handle holds, two G1 points per item.  G1 has cofactor 1 on both curves,
// so every point that decodes has order r and the pairing values lie in the order-r
// subgroup of GT, which is what the small-exponents group check (k_idv_bp_*) needs.
//
// Kernels, per curve (idemix_cred_<cv>.hip):
//   k_cred_decode  lane per credential: A and B decoded (status pre-set by the host for
//                  what it decides: NULL inputs, the proto, the scalars' range), neither the
//                  identity; FTS_E_CRED_MALFORMED
//   k_cred_var     lane per (product, credential), credentials fastest (a wave runs one
//                  product kind): E A by GLV over a lane table, then HRand S, HSk sk and
//                  HAttrs[i] attrs[i] from the issuer's tables -- the two bodies of k_idv_var
//   k_cred_join    lane per credential: g1 + the six fixed-base products against B
//                  (projective, no inversion; FTS_E_CRED_B), T = E A - B to affine with one
//                  inversion, pin[i] <- (A, T) as k_idv_decode writes (A', -ABar), zk[i] <- 1
// Lane scratch ([word][lane], n lanes each): DP = A and B decoded (2 x 16), VR = the seven
// products (7 x 24), TV = the lane table of E A (AT_WORDS): 456 words = 1,824 B per lane, in
// global memory (no kernel here asks for private scratch beyond what the two product bodies
// already take in k_idv_var).
// Not hardened against timing side channels (table indices and branches depend on sk).
#pragma once
#include "idv_kernels.hpp"

namespace idv {

// product v: 0 = E A (variable base), 1.. = fixed-base on the issuer's table CRV_BASE[v];
// its scalar is record word 8 v (E S sk attrs[0..3])
__device__ constexpr int CRV_BASE[CRV_NPROD] = {-1, B_HRAND, B_HSK, B_HA + 0, B_HA + 1, B_HA + 2, B_HA + 3};
FTS_DEV size_t crv_dp(size_t) { return 0; }
FTS_DEV size_t crv_vr(size_t n) { return (size_t)2 * 16 * n; }
FTS_DEV size_t crv_tv(size_t n) { return crv_vr(n) + (size_t)CRV_NPROD * 24 * n; }  // 200 n words: 16-byte aligned rows
constexpr size_t CRV_SCRATCH_WORDS = 2 * 16 + CRV_NPROD * 24 + AT_WORDS;

template <class CV>
__global__ void __launch_bounds__(256) k_cred_decode(int n, const uint8_t* __restrict__ pts,
                                                     uint32_t* __restrict__ scratch, int32_t* __restrict__ zk,
                                                     int32_t* __restrict__ status) {
  using F = typename CV::F;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  zk[i] = 0;
  if (status[i] != FTS_OK) return;
  const uint8_t* P = pts + (size_t)i * CRV_PTS_BYTES;
  const LaneWords DP{scratch + crv_dp(n), (size_t)n, (size_t)i};
  bool good = true;
#pragma unroll 1
  for (int q = 0; q < 2; q++) {
    F px, py;
    bool id;
    good = CV::decode(P + q * 64, px, py, id) && !id && good;
    put_f<CV>(DP, q * 16, px);
    put_f<CV>(DP, q * 16 + 8, py);
  }
  if (!good) status[i] = FTS_E_CRED_MALFORMED;
}

// lane g = v * n + i
template <class CV>
__global__ void __launch_bounds__(256) k_cred_var(int n, const uint32_t* __restrict__ rec,
                                                  const uint32_t* __restrict__ tables,
                                                  uint32_t* __restrict__ scratch, const int32_t* __restrict__ status) {
  using PJ = typename CV::PJ;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (size_t)CRV_NPROD * n) return;
  const int v = (int)(g / n), i = (int)(g % n);
  if (status[i] != FTS_OK) return;
  const uint32_t* k = rec + (size_t)i * CRV_REC_WORDS + v * 8;
  const LaneWords VR{scratch + crv_vr(n) + (size_t)v * 24 * n, (size_t)n, (size_t)i};
  PJ r = CV::inf();
  if (v > 0) {
    CV::fixed_mul_acc(r, tables, CRV_BASE[v], k);
  } else {
    const LaneWords DP{scratch + crv_dp(n), (size_t)n, (size_t)i};
    const GTab T{scratch + crv_tv(n), (size_t)n, (size_t)i};
    r = glv_mul<CV>(CV::from_affine(get_f<CV>(DP, 0), get_f<CV>(DP, 8)), k, T);
  }
  put_f<CV>(VR, 0, r.x);
  put_f<CV>(VR, 8, r.y);
  put_f<CV>(VR, 16, r.z);
}

template <class CV>
__global__ void __launch_bounds__(256) k_cred_join(int n, uint32_t* __restrict__ scratch, uint32_t* __restrict__ pin,
                                                   int32_t* __restrict__ zk, int32_t* __restrict__ status) {
  using B = typename CV::B;
  using F = typename CV::F;
  using PJ = typename CV::PJ;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || status[i] != FTS_OK) return;
  const LaneWords DP{scratch + crv_dp(n), (size_t)n, (size_t)i};
  auto product = [&](int v) {
    const LaneWords VR{scratch + crv_vr(n) + (size_t)v * 24 * n, (size_t)n, (size_t)i};
    PJ r;
    r.x = get_f<CV>(VR, 0), r.y = get_f<CV>(VR, 8), r.z = get_f<CV>(VR, 16);
    return r;
  };
  // g1 = (1, 2) on both curves
  PJ acc = CV::from_affine(B::one(), B::add(B::one(), B::one()));
#pragma unroll 1
  for (int v = 1; v < CRV_NPROD; v++) CV::add_to(acc, product(v));
  const F bx = get_f<CV>(DP, 16), by = get_f<CV>(DP, 24);
  bool good = !CV::is_inf(acc);  // B is not the identity (k_cred_decode)
  if (good) {
    const F z2 = B::mul(acc.z, acc.z), z3 = B::mul(z2, acc.z);
    good = B::eq(B::mul(bx, z2), acc.x) && B::eq(B::mul(by, z3), acc.y);
  }
  if (!good) {
    status[i] = FTS_E_CRED_B;
    return;
  }
  // T = E A - B; O is written as zeros (k_idv_pairing: e(g2, O) = 1, k_idv_bp_terms: no term)
  PJ t = product(0);
  CV::madd_to(t, bx, B::neg(by));
  F tx = B::zero(), ty = B::zero();
  if (!CV::is_inf(t)) {
    const F zi = B::inv(t.z), zi2 = B::mul(zi, zi);
    tx = B::mul(t.x, zi2), ty = B::mul(B::mul(t.y, zi2), zi);
  }
  const F ax = get_f<CV>(DP, 0), ay = get_f<CV>(DP, 8);
  uint32_t* pq = pin + (size_t)i * 32;
#pragma unroll
  for (int q = 0; q < 8; q++) pq[q] = ax.v[q], pq[8 + q] = ay.v[q], pq[16 + q] = tx.v[q], pq[24 + q] = ty.v[q];
  zk[i] = 1;
}

// ------------------------------------------------- per-curve launch sequence
template <class CV>
void launch_cred_prep(const CredChain& c) {
  const unsigned g256 = (unsigned)((c.n + 255) / 256), gvar = (unsigned)(((size_t)CRV_NPROD * c.n + 255) / 256);
  k_cred_decode<CV><<<g256, 256, 0, c.s>>>(c.n, c.pts, c.scr, c.zk, c.st);
  k_cred_var<CV><<<gvar, 256, 0, c.s>>>(c.n, c.rec, c.tables, c.scr, c.st);
  k_cred_join<CV><<<g256, 256, 0, c.s>>>(c.n, c.scr, c.pin, c.zk, c.st);
}

}  // namespace idv
