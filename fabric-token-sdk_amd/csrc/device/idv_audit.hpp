// Idemix audit info against owner identities: the auditor's
// AuditInfo.Match (services/identity/idemix/crypto/audit.go:40-84), reached through
// InspectIdentity for every output, input and issuer of an audited request
// (crypto/audit/auditor.go:225-282).  Match makes two Csp.Verify calls, with
// EidNymAuditOpts and RhNymAuditOpts (IBM/idemix AuditNymEid / AuditNymRh, restated
// in tests/idemix_audit_ref.py; unpinned like the identity proof's transcript):
//
//   EidNym' = HAttrs[2] * HashToZr(eid) + HRand * r_eid,  accept iff EidNym' == sig.EidNym.Nym
//   RhNym'  = HAttrs[3] * HashToZr(rh)  + HRand * r_rh,   accept iff RhNym'  == sig.RhNym.Nym
//
// One lane per (identity, half), half-major: lanes [0, n) are the EID halves, lanes
// [n, 2n) the RH halves, so a wave gathers from one pair of tables (but the wave that
// straddles n).  A lane hashes its attribute string (SHA-256, any number of blocks),
// reduces the digest and its rand mod r, decodes its point, accumulates the two
// fixed-base products of the issuer's tables (fts_idemix_idv: HRand, HAttrs[2..3])
// into ONE accumulator and compares projectively (X == x Z^2, Y == y Z^3, as
// k_open_check): no inversion, no early exit on a mismatch, 32 mixed additions at
// most.  Each half writes its own verdict word; the host folds them in the
// reference's order (pre ? pre : eid ? eid : rh).
#pragma once
#include "idv_kernels.hpp"

namespace idv {

// pts, rnd: [2][n] raw points (X || Y) and rands (32 B big-endian); attrw + aoff[g]:
// lane g's string, alen[g] bytes; pre[n]: the host's verdicts that end a match;
// rh_pre[n]: the RH half's verdict as far as the host knows it (no nym, a coordinate
// of the wrong length); half_st[2][n] <- FTS_OK or the half's FTS_E_AUDIT_*
template <class CV>
__global__ void __launch_bounds__(64) k_idv_audit(int n, const uint8_t* __restrict__ pts,
                                                  const uint32_t* __restrict__ rnd,
                                                  const uint32_t* __restrict__ attrw,
                                                  const uint64_t* __restrict__ aoff,
                                                  const uint32_t* __restrict__ alen, const int32_t* __restrict__ pre,
                                                  const int32_t* __restrict__ rh_pre,
                                                  const uint32_t* __restrict__ tables,
                                                  int32_t* __restrict__ half_st) {
  using B = typename CV::B;
  using F = typename CV::F;
  using PJ = typename CV::PJ;
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= 2 * (size_t)n) return;
  const int half = g >= (size_t)n ? 1 : 0;
  const size_t i = g - (size_t)half * n;
  half_st[g] = FTS_OK;
  if (pre[i] != FTS_OK) return;
  if (half && rh_pre[i] != FTS_OK) {
    half_st[g] = rh_pre[i];
    return;
  }
  // G1FromProto of the nym
  F px, py;
  bool ident;
  if (!CV::decode(pts + g * 64, px, py, ident)) {
    half_st[g] = half ? FTS_E_AUDIT_RH_POINT : FTS_E_AUDIT_EID_POINT;
    return;
  }
  // HashToZr(attribute)
  const uint32_t* m = attrw + aoff[g];
  const uint32_t len = alen[g], nb = padded_blocks(len);
  uint32_t st[8], w[16];
  sha256_init(st);
  for (uint32_t blk = 0; blk < nb; blk++) {
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = padded_word(m, 0u, len, nb, 16u * blk + k);
    sha256_compress(st, w);
  }
  uint32_t h[8], r[8];
  CV::digest_mod_r(st, h);
  // rand mod r: 32 big-endian bytes, the digest's form
#pragma unroll
  for (int k = 0; k < 8; k++) st[k] = __builtin_bswap32(rnd[g * 8 + k]);
  CV::digest_mod_r(st, r);
  PJ acc = CV::inf();
  CV::fixed_mul_acc(acc, tables, B_HA + 2 + half, h);
  CV::fixed_mul_acc(acc, tables, B_HRAND, r);
  bool eq;
  if (ident) {
    eq = CV::is_inf(acc);
  } else if (CV::is_inf(acc)) {
    eq = false;
  } else {
    const F z2 = B::mul(acc.z, acc.z);
    eq = B::eq(acc.x, B::mul(px, z2)) && B::eq(acc.y, B::mul(py, B::mul(z2, acc.z)));
  }
  if (!eq) half_st[g] = half ? FTS_E_AUDIT_RH_MISMATCH : FTS_E_AUDIT_EID_MISMATCH;
}

}  // namespace idv
