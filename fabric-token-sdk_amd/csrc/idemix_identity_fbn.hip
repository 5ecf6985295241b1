// FP256BN instances of the identity-proof kernels (device/idv_kernels.hpp).
#include "device/idv_kernels.hpp"

namespace idv {

template void launch_tvals<FbnCurve>(const Chain&);
template void launch_batch<FbnCurve>(const Chain&);
template void launch_pairing<FbnCurve>(const Chain&, unsigned, bool);
template void launch_lines<FbnCurve>(const uint8_t*, uint32_t*, int32_t*, hipStream_t);

}  // namespace idv
