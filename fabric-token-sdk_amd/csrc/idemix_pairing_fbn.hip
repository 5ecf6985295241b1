// FP256BN instance of the one-by-one pairing check (device/idv_kernels.hpp k_idv_pairing).
#include "device/idv_kernels.hpp"

namespace idv {

template void launch_pairing<FbnCurve>(const Chain&, unsigned, bool);

}  // namespace idv
