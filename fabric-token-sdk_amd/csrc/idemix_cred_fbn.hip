// FP256BN instances of the credential-verification kernels (device/cred_kernels.hpp).
#include "device/cred_kernels.hpp"

namespace idv {

template void launch_cred_prep<FbnCurve>(const CredChain&);

}  // namespace idv
