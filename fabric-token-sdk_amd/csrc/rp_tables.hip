// Range-proof context creation and staging, off the pass: the fixed-base tables of a
// context (device/fixed_base.hpp layout) and the config-C3 staging of MSM points.
#include "device/g1.hpp"
#include "device/fixed_base.hpp"
#include "device/transcript.hpp"
#include "device/launch.hpp"

namespace fts {

// ---------------------------------------------------------- context tables
// Built once per context (device/fixed_base.hpp layout), for nb bases:
//   kt_window_bases  lane per (base, window)   B_w = 2^(W w) B            (Jacobian)
//   kt_small_large   lane per (base, window)   small[lo] = (lo+1) B_w, large[hi] = hi S B_w
//   kt_entries       lane per entry            T[w][d-1] = large[hi] + small[lo], d-1 = hi S + lo
// for window width W (FbCfg<W>: 16-bit for every base, 20-bit for H_i, K, P)
//   k_rp_normalize   block per 256 entries     affine (one inversion per block)
template <int W>
__global__ void __launch_bounds__(64) kt_window_bases(const uint32_t* __restrict__ bases, int nb,
                                                      uint32_t* __restrict__ bw) {
  using C = FbCfg<W>;
  int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= nb * C::NW) return;
  int b = gid / C::NW, w = gid % C::NW;
  G1J p = g1j_from_affine(load_g1a(bases + b * 16));
  for (int i = 0; i < W * w; i++) p = nl_dbl(p);
  store_g1j(bw + (size_t)gid * 24, p);
}

template <int W>
__global__ void __launch_bounds__(64) kt_small_large(int nb, const uint32_t* __restrict__ bw,
                                                     uint32_t* __restrict__ small, uint32_t* __restrict__ large) {
  using C = FbCfg<W>;
  int gid = blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= nb * C::NW) return;
  const uint32_t* Bw = bw + (size_t)gid * 24;
  uint32_t* S = small + (size_t)gid * C::S * 24;
  uint32_t* L = large + (size_t)gid * C::L * 24;
  G1J acc = load_g1j(Bw);
  store_g1j(S, acc);
  for (int lo = 1; lo < C::S; lo++) {
    acc = nl_add_mem(acc, Bw, 0);
    store_g1j(S + lo * 24, acc);
  }
  // acc = S * B_w
  store_g1j(L, g1j_identity());
  G1J big = g1j_identity();
  for (int hi = 1; hi < C::L; hi++) {
    big = nl_add_mem(big, S + (C::S - 1) * 24, 0);
    store_g1j(L + hi * 24, big);
  }
}

template <int W>
__global__ void __launch_bounds__(64) kt_entries(int nb, const uint32_t* __restrict__ small,
                                                 const uint32_t* __restrict__ large, uint32_t* __restrict__ jac) {
  using C = FbCfg<W>;
  size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (gid >= (size_t)nb * C::NW * C::E) return;
  const size_t bw = gid / C::E;
  const int e = (int)(gid % C::E);  // d - 1
  const int hi = e / C::S, lo = e % C::S;
  G1J p = load_g1j(small + (bw * C::S + lo) * 24);
  if (hi) p = nl_add_mem(p, large + (bw * C::L + hi) * 24, 0);
  store_g1j(jac + gid * 24, p);
}

size_t fb_words_per_base() { return FB_WORDS_PER_BASE; }
// the per-proof bases' wide tables: 20-bit windows (13 per scalar, 436 MiB per base)
// or 22-bit (12, 1.5 GiB per base) where the device has the memory (api_ctx.cpp)
size_t fbw_words_per_base(int wbits) { return wbits == 22 ? FbCfg<22>::WORDS_PER_BASE : FbWide::WORDS_PER_BASE; }
template <int W>
static size_t build_scratch_bytes(int nb) {
  using C = FbCfg<W>;
  const size_t nbw = (size_t)nb * C::NW;
  return nbw * 24 * 4 + nbw * (C::S + C::L) * 24 * 4 + nbw * C::E * 24 * 4;
}
size_t table_build_scratch_bytes(int nb) { return build_scratch_bytes<FB_W>(nb); }
size_t wide_build_scratch_bytes(int nb, int wbits) {
  return wbits == 22 ? build_scratch_bytes<22>(nb) : build_scratch_bytes<FBW_W>(nb);
}
// tables: nb * WORDS_PER_BASE words; scratch: build_scratch_bytes<W>(nb)
template <int W>
static void build_tables(const uint32_t* bases, int nb, uint32_t* tables, uint32_t* scratch, hipStream_t s) {
  using C = FbCfg<W>;
  const size_t nbw = (size_t)nb * C::NW;
  uint32_t* bw = scratch;
  uint32_t* small = bw + nbw * 24;
  uint32_t* large = small + nbw * C::S * 24;
  uint32_t* jac = large + nbw * C::L * 24;
  FTS_LAUNCH(kt_window_bases<W>, nbw, 64, s, bases, nb, bw);
  FTS_LAUNCH(kt_small_large<W>, nbw, 64, s, nb, bw, small, large);
  FTS_LAUNCH(kt_entries<W>, nbw * C::E, 64, s, nb, small, large, jac);
  launch_normalize_all((int)(nbw * C::E), jac, tables, s);
}
void launch_build_tables(const uint32_t* bases, int nb, uint32_t* tables, uint32_t* scratch, hipStream_t s) {
  build_tables<FB_W>(bases, nb, tables, scratch, s);
}
void launch_build_wide_tables(const uint32_t* bases, int nb, uint32_t* tables, uint32_t* scratch, hipStream_t s,
                              int wbits) {
  if (wbits == 22) build_tables<22>(bases, nb, tables, scratch, s);
  else build_tables<FBW_W>(bases, nb, tables, scratch, s);
}

// Config C3 staging (fts_msm_stage_multiples): N distinct points P_i = k_i * B
// from a fixed-base table (16-bit windows), k_i = 32-byte BE integers mod r,
// as Jacobian into jac (normalised by the caller), and the MSM scalars s_i
// (BE, reduced mod r as G1.Mul does) as canonical limbs
__global__ void __launch_bounds__(256) k_msm_gen_points(int N, const uint8_t* __restrict__ raw_k,
                                                       const uint8_t* __restrict__ raw_s,
                                                       const uint32_t* __restrict__ table, uint32_t* __restrict__ jac,
                                                       uint32_t* __restrict__ sc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  auto be_fr = [](const uint8_t* p) {
    uint32_t w[8];
    const uint4* s4 = reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const uint4 u = s4[q];
      w[4 * q + 0] = __builtin_bswap32(u.x);
      w[4 * q + 1] = __builtin_bswap32(u.y);
      w[4 * q + 2] = __builtin_bswap32(u.z);
      w[4 * q + 3] = __builtin_bswap32(u.w);
    }
    return digest_to_fr(w);  // canonical limbs mod r
  };
  const Fr k = be_fr(raw_k + (size_t)i * 32), sv = be_fr(raw_s + (size_t)i * 32);
  Scalar ks;
#pragma unroll
  for (int q = 0; q < 8; q++) ks.v[q] = k.v[q], sc[(size_t)i * 8 + q] = sv.v[q];
  store_g1j(jac + (size_t)i * 24, fb_mul(table, ks));
}
void launch_msm_gen_points(int N, const uint8_t* raw_k, const uint8_t* raw_s, const uint32_t* table, uint32_t* jac,
                           uint32_t* pts, uint32_t* sc, hipStream_t s) {
  FTS_LAUNCH(k_msm_gen_points, N, 256, s, N, raw_k, raw_s, table, jac, sc);
  launch_normalize_all(N, jac, pts, s);
}

}  // namespace fts
