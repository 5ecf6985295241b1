// BN254 instances of the issuer-key kernels (device/ipk_kernels.hpp).
#include "device/ipk_kernels.hpp"

namespace idv {

template void launch_ipk_check<BnCurve>(const IpkChain&);
template void launch_ipk_keygen<BnCurve>(const IpkChain&);

}  // namespace idv
