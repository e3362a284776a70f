// qpd_k_generic_dm.hip -- the blind-detection metric instantiation of the float
// FastSC kernel (generic_decode_kernel<..., DM = true>, qpd_generic.hip:
// qpd_dmetric), as a unit of its own (build.py UNITS): the plain instantiations
// of qpd_k_generic.hip compile to what they were.
#include "qpd_generic.hip"

namespace qpd {

const void *dmetric_kernel() {
    return reinterpret_cast<const void *>(&generic_decode_kernel<K_FASTSC_LUT, DOM_FLOAT, kMaxL, true>);
}

}  // namespace qpd
