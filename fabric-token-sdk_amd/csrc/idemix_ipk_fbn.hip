// FP256BN instances of the issuer-key kernels (device/ipk_kernels.hpp).
#include "device/ipk_kernels.hpp"

namespace idv {

template void launch_ipk_check<FbnCurve>(const IpkChain&);
template void launch_ipk_keygen<FbnCurve>(const IpkChain&);

}  // namespace idv
