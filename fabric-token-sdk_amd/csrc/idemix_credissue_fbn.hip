// FP256BN instances of the credential-request and credential-issuance kernels
// (device/credissue_kernels.hpp).
#include "device/credissue_kernels.hpp"

namespace idv {

template void launch_credreq_make<FbnCurve>(const CredReqChain&);
template hipError_t launch_credissue<FbnCurve>(const CredReqChain&, bool);
template void launch_credissue_key<FbnCurve>(const uint8_t*, const uint32_t*, int32_t*, hipStream_t);

}  // namespace idv
