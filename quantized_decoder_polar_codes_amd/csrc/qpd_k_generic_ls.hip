// qpd_k_generic_ls.hip -- the list-output instantiations of the generic engine's list
// kinds (generic_decode_kernel<..., LS = true>, qpd_generic.hip: qpd_decode_list), as a
// unit of their own (build.py UNITS): the plain instantiations of qpd_k_generic.hip
// compile to what they were.
#include "qpd_generic.hip"
#include "qpd.h"

namespace qpd {

// wide: the instantiation for 9 <= L <= 16 (lane groups of 16 or 32).
const void *generic_list_kernel(int fam, int dom, bool wide) {
#define QPD_GL(K, D) (wide ? reinterpret_cast<const void *>(&generic_decode_kernel<K, D, kMaxLWide, false, true>) \
                           : reinterpret_cast<const void *>(&generic_decode_kernel<K, D, kMaxL, false, true>))
    const bool scl = fam == QPD_SCL_LUT;
    if (!scl && fam != QPD_FASTSCL_LUT) return nullptr;
    switch (dom) {
        case DOM_LUT: return scl ? QPD_GL(K_SCL_LUT, DOM_LUT) : QPD_GL(K_FASTSCL_LUT, DOM_LUT);
        case DOM_FLOAT: return scl ? QPD_GL(K_SCL_LUT, DOM_FLOAT) : QPD_GL(K_FASTSCL_LUT, DOM_FLOAT);
        case DOM_UNIFORM: return scl ? QPD_GL(K_SCL_LUT, DOM_UNIFORM) : nullptr;
        case DOM_LLOYD: return scl ? QPD_GL(K_SCL_LUT, DOM_LLOYD) : nullptr;
        default: return nullptr;
    }
#undef QPD_GL
}

}  // namespace qpd
