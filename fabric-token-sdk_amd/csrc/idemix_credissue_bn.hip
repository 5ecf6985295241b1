// BN254 instances of the credential-request and credential-issuance kernels
// (device/credissue_kernels.hpp) and the size function the host code needs.
#include "device/credissue_kernels.hpp"

namespace idv {

template void launch_credreq_make<BnCurve>(const CredReqChain&);
template hipError_t launch_credissue<BnCurve>(const CredReqChain&, bool);
template void launch_credissue_key<BnCurve>(const uint8_t*, const uint32_t*, int32_t*, hipStream_t);

size_t credissue_scratch_words(size_t n) { return CI_SCRATCH_WORDS * n; }

}  // namespace idv
