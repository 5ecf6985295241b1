// FP256BN instance of the one-by-one pairing check (device/idv_kernels.hpp k_idv_pairing) and
// of the debug pairing.
#include "device/idv_kernels.hpp"

namespace idv {

template void launch_pairing<FbnCurve>(const Chain&, unsigned, bool);
template void launch_pairing_debug<FbnCurve>(const uint32_t*, int, const uint32_t*, uint32_t*, int, hipStream_t);

}  // namespace idv
