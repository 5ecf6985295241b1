// BN254 instance of the one-by-one pairing check (device/idv_kernels.hpp k_idv_pairing) and
// the BN254-only debug pairing.  A unit of its own: the kernel inlines a Miller loop and a
// final exponentiation, minutes of device compilation, as does k_idv_bp_pair (idemix_bp_bn.hip).
#include "device/idv_kernels.hpp"

namespace idv {

template void launch_pairing<BnCurve>(const Chain&, unsigned, bool);

void launch_pairing_debug(const uint32_t* lines, int which, const uint32_t* p16, uint32_t* out, int final_exp,
                          hipStream_t s) {
  k_idv_pairing_debug<BnCurve><<<1, 64, 0, s>>>(lines, which, p16, out, final_exp);
}

}  // namespace idv
