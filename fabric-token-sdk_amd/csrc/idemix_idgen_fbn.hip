// FP256BN instances of the identity-generation kernels (device/idgen_kernels.hpp).
#include "device/idgen_kernels.hpp"

namespace idv {

template void launch_idgen_cred<FbnCurve>(const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*, int32_t*,
                                          hipStream_t);
template hipError_t launch_idgen<FbnCurve>(const GenChain&);

}  // namespace idv
