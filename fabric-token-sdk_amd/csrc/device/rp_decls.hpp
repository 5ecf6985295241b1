// The range-proof pass's kernels that one unit defines and rp_pass.cpp launches, and the
// constants a kernel shares with its launcher.  Included by every rp_*.hip unit and by
// rp_pass.cpp (launch.hpp's rule): a changed parameter declares a different overload, so
// the launch fails to link instead of surfacing at run time.  The <W> templates are
// instantiated explicitly by their defining unit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fixed_base.hpp"
#include "rp_kernels.hpp"

namespace fts {

// ---- launch constants
constexpr int NORM_BS = 256;
// points per lane of k_rp_normalize (one inversion per lane, round 5): 16 for
// normalisations of >= NORM_BIG points, 4 below (more lanes for small batches)
constexpr int NORM_E = 16;  // nominal, for the cost model
constexpr size_t NORM_BIG = (size_t)1 << 16;
// k_rp_powers: indices per lane (the chunk's low bits expand as a binary tree)
constexpr int PW_LC = 3, PW_CH = 1 << PW_LC;
// com terms per proof, work path: slots 0 z*K, 1 -delta*P (k_rp_fixed_exact ->
// k_rp_com_var)
constexpr int COM_NTERMS = 2;
// Horner chunks of S = sum_i 2^i H'_i: 16 H' per chunk (4 chunks at n = 64),
// joined once per proof by k_rp_hsum_join (slot 0 of the proof's chunks)
constexpr int HS_CHUNK = 16;
constexpr int HS_SCRATCH = 4 * 24;  // scratch words per proof for the chunks (n <= 64)
// com terms per proof, latency path: terms layout [B][n + 4][24]: Z_0..Z_{n-1}, z K, -delta P, x*D halves
inline __host__ __device__ int com_fx_slots(int n) { return n + 4; }
// k_rp_com_tree: lanes per proof, proofs per block
constexpr int CT_LANES = 16, CT_PROOFS = 16;
// k_rp_x0_build: proofs (waves) per block
constexpr int X0_PPB = 4;
// LDS bytes per proof of a part: part 1 assembles only the blocks after the template
inline uint32_t x0_part_lds_base(int n, int part) { return part == 1 ? 64u * x0_cb0(n) : 0u; }
inline size_t x0_build_lds(int n, int part = 2) {
  return (size_t)X0_PPB * (x0_var_bytes(n) - x0_part_lds_base(n, part));
}
inline unsigned x0_build_grid(int B) { return (unsigned)((B + X0_PPB - 1) / X0_PPB); }
// column Q over the whole pass: partial sums per slice of proofs (k_rlc_columns), summed by k_rlc_qsum
constexpr int RQ_PARTS = 64;
// k_rlc_fixed: (group, column) items per block, FB_NW lanes each
constexpr int RF_ITEMS = 16;

// ---- rp_exact.hip
__global__ void k_rp_gather(RpGather g, int npts, uint8_t* raw, uint32_t* sc, int32_t* status, int32_t* ipa);
__global__ void k_rp_decode(int B, int npts, const uint8_t* raw, uint32_t* pts, int32_t* status);
__global__ void k_rp_chal_fr(int B, int n, int k, const int32_t* status, uint32_t* ch, uint32_t* tmp);
__global__ void k_rp_powers(int B, int n, int k, const int32_t* status, const uint32_t* ch, uint32_t* ypow,
                            uint32_t* svec, uint32_t* zvec);
template <int W>
__global__ void k_rp_fixed_exact(int B, int n, int k, const int32_t* status, const uint32_t* sc, const uint32_t* ch,
                                 const uint32_t* ypow, const uint32_t* wtables, uint32_t* hpj, uint32_t* terms);
__global__ void k_rp_hsum_chunks(int B, int n, const int32_t* status, const uint32_t* hpj, uint32_t* chunks);
__global__ void k_rp_hsum_join(int B, int n, const int32_t* status, uint32_t* chunks);
__global__ void k_rp_com_tab(int B, int n, int k, const int32_t* status, const uint32_t* pts, const uint32_t* chunks,
                             uint32_t* atab);
__global__ void k_rp_com_var(int B, int n, int k, const int32_t* status, const uint32_t* pts, const uint32_t* ch,
                             const uint32_t* chunks, uint32_t* atab, const uint32_t* terms, uint32_t* hpj,
                             uint32_t* hpa, uint8_t* hp_be);
template <int W>
__global__ void k_rp_fixed_all(int B, int n, int k, const int32_t* status, const uint32_t* sc, const uint32_t* ch,
                               const uint32_t* ypow, const uint32_t* zvec, const uint32_t* wtables, uint32_t* hpj,
                               uint32_t* terms);
__global__ void k_rp_xd(int B, int n, int k, const int32_t* status, const uint32_t* pts, const uint8_t* small_msgs,
                        uint32_t* vtab, uint32_t* terms, int tstride, int toff);
__global__ void k_rp_com_tree(int B, int n, int k, const int32_t* status, const uint32_t* pts, const uint32_t* terms,
                              uint32_t* hpj, uint32_t* hpa, uint8_t* hp_be);

// ---- rp_x0.hip
__global__ void k_rp_hash_small(int B, int n, int k, const uint8_t* raw, const int32_t* status, uint32_t* ch,
                                uint8_t* small_msgs);
__global__ void k_rp_x0_hdr(int B, int n, const int32_t* status, const uint8_t* x0_const, uint8_t* msgs);
__global__ void k_rp_x0_build(int B, int n, const int32_t* status, const uint8_t* hp_be, const uint8_t* x0_const,
                              const uint32_t* sc, uint8_t* msgs, int part);
__global__ void k_rp_x0_hash(int B, int n, int k, const int32_t* status, const uint8_t* msgs, const uint8_t* tmpl,
                             uint32_t b0, uint32_t b1, uint32_t* mid, uint32_t* ch);

// ---- rp_rlc.hip
__global__ void k_rlc_prep(int B, int n, int k, const int32_t* status, const int32_t* excl, const int32_t* ipa_flag,
                           const uint32_t* sc, const uint32_t* ch, const uint32_t* key, uint32_t* msc, uint32_t* coef,
                           int idxw = 0);
__global__ void k_rlc_columns(int B, int n, int k, int gs, int col0, const int32_t* sel, const uint32_t* ch,
                              const uint32_t* coef, const uint32_t* ypow, const uint32_t* svec, const uint32_t* zvec,
                              uint32_t* colsum);
__global__ void k_rlc_fixed(int n, int G, int col0, int ncl, const uint32_t* colsum, const uint32_t* tables,
                            uint32_t* out);
__global__ void k_rlc_finalize(int B, const uint32_t* msm_out, const uint32_t* addend, const int32_t* excl,
                               int32_t* status, const int32_t* ipa_flag, int32_t* flag);
__global__ void k_rlc_finalize_groups(int slots, int gs, int NC, const int32_t* sel, const uint32_t* msm_out,
                                      const uint32_t* qfix, const int32_t* excl, int32_t* status,
                                      const int32_t* ipa_flag, int32_t* gflag, int32_t* flag);

extern template __global__ void k_rp_fixed_exact<FBW_W>(int, int, int, const int32_t*, const uint32_t*, const uint32_t*,
                                                     const uint32_t*, const uint32_t*, uint32_t*, uint32_t*);
extern template __global__ void k_rp_fixed_exact<22>(int, int, int, const int32_t*, const uint32_t*, const uint32_t*,
                                                     const uint32_t*, const uint32_t*, uint32_t*, uint32_t*);
extern template __global__ void k_rp_fixed_all<FBW_W>(int, int, int, const int32_t*, const uint32_t*, const uint32_t*,
                                                   const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*,
                                                   uint32_t*);
extern template __global__ void k_rp_fixed_all<22>(int, int, int, const int32_t*, const uint32_t*, const uint32_t*,
                                                   const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*,
                                                   uint32_t*);

}  // namespace fts
