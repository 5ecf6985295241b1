// BN254 instances of the identity-proof kernels (device/idv_kernels.hpp) but the pairing
// ones (idemix_pairing_bn.hip, idemix_bp_bn.hip): the t-values and the line tables, the
// BN254-only epoch-key check and the size functions the host code needs.
#include "device/idv_kernels.hpp"

namespace idv {

template void launch_tvals<BnCurve>(const Chain&);
template void launch_lines<BnCurve>(const uint8_t*, uint32_t*, int32_t*, hipStream_t);

// U distinct epoch keys (128 raw bytes each, BN254): ok[u] <- the key decodes (on the
// twist, canonical) and lies in the subgroup (the identity does)
// lane j checks distinct key idx[j] (the keys the context has not checked before)
__global__ void __launch_bounds__(64) k_idv_g2_check(int M, const int32_t* __restrict__ idx,
                                                     const uint8_t* __restrict__ keys, int32_t* __restrict__ ok) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= M) return;
  const int u = idx[j];
  pair::F2<pair::BnField> x, y;
  const uint8_t* kr = keys + (size_t)u * 128;
  bool good = decode_g2<BnCurve>(kr, x, y);
  bool zero = true;
  for (int q = 0; q < 128; q++) zero = zero && kr[q] == 0;
  if (good && !zero) good = g2_in_subgroup_bn(x, y);
  ok[u] = good ? 1 : 0;
}
void launch_g2_check(int M, const int32_t* idx, const uint8_t* keys, int32_t* ok, hipStream_t s) {
  k_idv_g2_check<<<(unsigned)((M + 63) / 64), 64, 0, s>>>(M, idx, keys, ok);
}

size_t line_words(bool bn) {
  return (size_t)(bn ? pair::n_lines<pairc::Bn254>() : pair::n_lines<pairc::Fp256bn>()) * pair::LINE_WORDS;
}
size_t idv_scratch_words(size_t n) { return (5 * 24 + NPT * 16 + 1 + NSC * 24 + NVAR * AT_WORDS) * n + 3; }
size_t bp_part_off(size_t n) { return (size_t)2 * AT_WORDS * n; }
size_t bp_gok_off(size_t n, size_t ng) { return bp_part_off(n) + ng * 48; }
size_t bp_cnt_off(size_t n, size_t ng) { return bp_gok_off(n, ng) + ng; }
size_t bp_list_off(size_t n, size_t ng) { return bp_cnt_off(n, ng) + 64; }
size_t bp_scratch_words(size_t n) {
  const size_t ng = (n + BP_G - 1) / BP_G;
  return bp_list_off(n, ng) + n;
}

}  // namespace idv
