// FP256BN instance of the batch pairing check (device/idv_kernels.hpp k_idv_bp_terms / _pair / _sel).
#include "device/idv_kernels.hpp"

namespace idv {

template void launch_batch<FbnCurve>(const Chain&);

}  // namespace idv
