// BN254 instance of the one-by-one pairing check (device/idv_kernels.hpp k_idv_pairing) and
// of the debug pairing.  A unit of its own: the kernel inlines a Miller loop and a
// final exponentiation, minutes of device compilation, as does k_idv_bp_pair (idemix_bp_bn.hip).
#include "device/idv_kernels.hpp"

namespace idv {

template void launch_pairing<BnCurve>(const Chain&, unsigned, bool);
template void launch_pairing_debug<BnCurve>(const uint32_t*, int, const uint32_t*, uint32_t*, int, hipStream_t);

}  // namespace idv
