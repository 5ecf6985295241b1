// Both curves' instances of the audit-match kernel (device/idv_audit.hpp).  A unit
// of its own: the curves' pairing units each take minutes to compile, this one
// instantiates k_idv_audit alone.
#include "device/idv_audit.hpp"

namespace idv {

void launch_idv_audit(bool bn, int n, const uint8_t* pts, const uint32_t* rnd, const uint32_t* attrw,
                      const uint64_t* aoff, const uint32_t* alen, const int32_t* pre, const int32_t* rh_pre,
                      const uint32_t* tables, int32_t* half_st, hipStream_t s) {
  if (n <= 0) return;
  const unsigned grid = (unsigned)((2 * (size_t)n + 63) / 64);
  if (bn) k_idv_audit<BnCurve><<<grid, 64, 0, s>>>(n, pts, rnd, attrw, aoff, alen, pre, rh_pre, tables, half_st);
  else k_idv_audit<FbnCurve><<<grid, 64, 0, s>>>(n, pts, rnd, attrw, aoff, alen, pre, rh_pre, tables, half_st);
}

}  // namespace idv
