// FP256BN instances of the identity-proof kernels (device/idv_kernels.hpp) but the pairing
// ones (idemix_pairing_fbn.hip, idemix_bp_fbn.hip): the t-values and the line tables.
#include "device/idv_kernels.hpp"

namespace idv {

template void launch_tvals<FbnCurve>(const Chain&);
template void launch_lines<FbnCurve>(const uint8_t*, uint32_t*, int32_t*, hipStream_t);

}  // namespace idv
