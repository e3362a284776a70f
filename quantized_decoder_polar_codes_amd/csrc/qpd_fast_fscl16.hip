// qpd_fast_fscl16.hip -- the FastSCL-LUT instantiations of lut_fast_kernel
// (qpd_fast.hip) for list sizes 9..16 (W16: lane groups of 16, keep_all16 /
// select_survivors16 at the leaf forks, the REP nodes' 2L -> L step and every R1
// layer; R1 nodes of up to 15 layers), with two or one pointer words per path.
// A unit of its own: it compiles beside the others and leaves their objects as
// they are.  See qpd_k_fast.hip for the units.
#ifndef QPD_VEC_CHAIN  // as the other FastSCL-LUT units (qpd_fast_fscl.hip)
#define QPD_VEC_CHAIN 1
#endif
#include "qpd_fast.hip"

namespace qpd {

const void *QPD_UNIT_FN(fast_kernel_fscl_w16)(int sets, bool pw1) {
#define QPD_FW(S, P) reinterpret_cast<const void *>(&lut_fast_kernel<K_FASTSCL_LUT, S, false, false, false, P, true, QPD_ST>)
    if (sets == 2) return pw1 ? QPD_FW(2, true) : QPD_FW(2, false);
    if (sets == 1) return pw1 ? QPD_FW(1, true) : QPD_FW(1, false);
    return nullptr;
#undef QPD_FW
}

}  // namespace qpd
