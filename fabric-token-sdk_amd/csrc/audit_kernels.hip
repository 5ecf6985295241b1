// Token opening checks: the auditor's and the wallet's
// re-commitment of a token from its opening,
//
//   tokenComm = HashToZr(type) * ped0 + value * ped1 + bf * ped2
//   accept iff tokenComm == token.Data
//
// (crypto/audit/auditor.go:226-238 InspectOutput, crypto/token/token.go:69-83
// Token.ToClear, both through commit() token.go:208-217 / auditor.go:412-418).
//
// One lane per token: three fixed-base products over the context's 16-bit
// window tables of ped0/ped1/ped2 (tb_ped0 / tb_G / tb_H), accumulated into
// ONE Jacobian accumulator (no intermediate point additions), then compared
// with the affine commitment in projective form (X == x Z^2, Y == y Z^3): no
// inversion, no normalisation.  48 mixed additions per token at most.
//
// Record layout (host-staged, SoA): raw[n][64] = token.Data as X||Y
// big-endian (NewG1FromBytes input), sc[n][24] = canonical Fr limbs of
// (HashToZr(type), value mod r, bf mod r) -- G1.Mul(s) multiplies by s mod r.
//
// k_token_commit (below) publishes the same sum instead of comparing it: the
// batched commit() of the prover side (fts_token_commit_batch_gpu, action generation).
#include "device/g1.hpp"
#include "device/fixed_base.hpp"
#include "device/helpers.hpp"
#include "device/rp_kernels.hpp"
#include "device/launch.hpp"
#include "../../include/fts_gpu.h"

namespace fts {

__global__ void __launch_bounds__(64) k_open_check(int n, const uint8_t* __restrict__ raw,
                                                   const uint32_t* __restrict__ sc, const uint32_t* __restrict__ t_ped0,
                                                   const uint32_t* __restrict__ t_ped1,
                                                   const uint32_t* __restrict__ t_ped2, int32_t* __restrict__ status) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || status[i] != FTS_OK) return;
  G1A com;
  if (!decode_point(raw + (size_t)i * 64, com)) {  // NewG1FromBytes of token.Data
    status[i] = FTS_E_MALFORMED;
    return;
  }
  const uint32_t* S = sc + (size_t)i * 24;
  Scalar k0, k1, k2;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    k0.v[j] = S[j];
    k1.v[j] = S[8 + j];
    k2.v[j] = S[16 + j];
  }
  G1J acc = g1j_identity();  // c.NewG1() then com.Add(g_i.Mul(v_i)) for i = 0..2
  fb_mul_acc(acc, t_ped0, k0);
  fb_mul_acc(acc, t_ped1, k1);
  fb_mul_acc(acc, t_ped2, k2);
  bool eq;
  if (g1a_is_identity(com)) {
    eq = g1j_is_identity(acc);
  } else if (g1j_is_identity(acc)) {
    eq = false;
  } else {
    const Fp z2 = fp_sqr(acc.z);
    eq = f_eq(acc.x, fp_mul(com.x, z2)) && f_eq(acc.y, fp_mul(com.y, fp_mul(z2, acc.z)));
  }
  status[i] = eq ? FTS_OK : FTS_E_OPEN_MISMATCH;
}

void launch_open_check(int n, const uint8_t* raw, const uint32_t* sc, const uint32_t* tables, int nb,
                       int32_t* status, hipStream_t s) {
  if (n <= 0) return;
  const uint32_t* t0 = tables + (size_t)tb_ped0(nb) * FB_WORDS_PER_BASE;
  const uint32_t* t1 = tables + (size_t)tb_G(nb) * FB_WORDS_PER_BASE;
  const uint32_t* t2 = tables + (size_t)tb_H(nb) * FB_WORDS_PER_BASE;
  hipLaunchKernelGGL(k_open_check, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, n, raw, sc, t0, t1, t2, status);
}

// Token commitments (token.go:208-217 as token.GetTokensWithWitness :109-133 calls it):
// the same three products from the same staging, sc[n][24], but the result is
// published, so it is the exact affine point: out[n][64] = G1.Bytes().
//
// A lane commits E tokens, token (wave * E + j) * 64 + lane for j < E: at each j the
// lanes of a wave hold 64 consecutive tokens (coalesced scalars, one table at a time),
// and the lane normalises its E sums with ONE inversion (the prefix-product pattern of
// k_rp_normalize).  The Jacobian sums wait in `out` (x, y: the 64 bytes the token's
// encoding will replace) and zs[n][8]; pre[n][8] holds the exclusive prefix products.
//
// A sum that ends at the identity (z == 0; HashToZr(type), value and bf would have to
// solve a discrete-log relation of ped0/ped1/ped2, so no test reaches it) is left out
// of the lane's product -- it must not zero its neighbours' shared inverse -- and comes
// out as 64 zero bytes, the G1.Bytes() of the identity.
template <int E>
__global__ void __launch_bounds__(64) k_token_commit(int n, const uint32_t* __restrict__ sc,
                                                     const uint32_t* __restrict__ t_ped0,
                                                     const uint32_t* __restrict__ t_ped1,
                                                     const uint32_t* __restrict__ t_ped2, uint32_t* __restrict__ zs,
                                                     uint32_t* __restrict__ pre, uint8_t* __restrict__ out) {
  const size_t gid = (size_t)blockIdx.x * 64 + threadIdx.x;
  const size_t g0 = (gid >> 6) * (size_t)E * 64 + (gid & 63);
  Fp run = f_one<FpP>();
  for (int j = 0; j < E; j++) {
    const size_t g = g0 + (size_t)j * 64;
    if (g >= (size_t)n) break;
    const uint32_t* S = sc + g * 24;
    Scalar k0, k1, k2;
#pragma unroll
    for (int q = 0; q < 8; q++) {
      k0.v[q] = S[q];
      k1.v[q] = S[8 + q];
      k2.v[q] = S[16 + q];
    }
    G1J acc = g1j_identity();
    fb_mul_acc(acc, t_ped0, k0);
    fb_mul_acc(acc, t_ped1, k1);
    fb_mul_acc(acc, t_ped2, k2);
    uint32_t* xy = reinterpret_cast<uint32_t*>(out + g * 64);
    store_fp(xy, acc.x);
    store_fp(xy + 8, acc.y);
    store_fp(zs + g * 8, acc.z);
    store_fp(pre + g * 8, run);
    if (!f_is_zero(acc.z)) run = fp_mul(run, acc.z);
  }
  if (g0 >= (size_t)n) return;
  Fp inv = nl_fp_inv(run);
  for (int j = E - 1; j >= 0; j--) {
    const size_t g = g0 + (size_t)j * 64;
    if (g >= (size_t)n) continue;
    uint32_t* xy = reinterpret_cast<uint32_t*>(out + g * 64);
    G1J p;
    load_fp(xy, p.x);
    load_fp(xy + 8, p.y);
    load_fp(zs + g * 8, p.z);
    G1A r;
    if (f_is_zero(p.z)) {
      r.x = f_zero<FpP>();
      r.y = f_zero<FpP>();
    } else {
      Fp pr;
      load_fp(pre + g * 8, pr);
      const Fp zi = fp_mul(inv, pr);
      inv = fp_mul(inv, p.z);
      const Fp zi2 = fp_sqr(zi);
      r.x = fp_mul(p.x, zi2);
      r.y = fp_mul(fp_mul(p.y, zi2), zi);
    }
    store_point_be(out + g * 64, r);
  }
}

void launch_token_commit(int n, int per_lane, const uint32_t* sc, const uint32_t* tables, int nb, uint32_t* zs,
                         uint32_t* pre, uint8_t* out, hipStream_t s) {
  if (n <= 0) return;
  const uint32_t* t0 = tables + (size_t)tb_ped0(nb) * FB_WORDS_PER_BASE;
  const uint32_t* t1 = tables + (size_t)tb_G(nb) * FB_WORDS_PER_BASE;
  const uint32_t* t2 = tables + (size_t)tb_H(nb) * FB_WORDS_PER_BASE;
  if (per_lane != 1 && per_lane != 2 && per_lane != 4 && per_lane != 8 && per_lane != 16) per_lane = TOKEN_COMMIT_PER_LANE;
  const unsigned waves = (unsigned)(((size_t)n + (size_t)per_lane * 64 - 1) / ((size_t)per_lane * 64));
#define FTS_COMMIT_CASE(E) \
  case E: hipLaunchKernelGGL(k_token_commit<E>, dim3(waves), dim3(64), 0, s, n, sc, t0, t1, t2, zs, pre, out); break
  switch (per_lane) {
    FTS_COMMIT_CASE(1);
    FTS_COMMIT_CASE(2);
    FTS_COMMIT_CASE(4);
    FTS_COMMIT_CASE(8);
    FTS_COMMIT_CASE(16);
  }
#undef FTS_COMMIT_CASE
}

}  // namespace fts
