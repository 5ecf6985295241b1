// BN254 instance of the batch pairing check (device/idv_kernels.hpp k_idv_bp_terms / _pair / _sel).
#include "device/idv_kernels.hpp"

namespace idv {

template void launch_batch<BnCurve>(const Chain&);

}  // namespace idv
