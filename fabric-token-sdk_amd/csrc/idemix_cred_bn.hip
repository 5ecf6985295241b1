// BN254 instances of the credential-verification kernels (device/cred_kernels.hpp) and the
// size function the host code needs.
#include "device/cred_kernels.hpp"

namespace idv {

template void launch_cred_prep<BnCurve>(const CredChain&);

size_t cred_scratch_words(size_t n) { return CRV_SCRATCH_WORDS * n; }

}  // namespace idv
