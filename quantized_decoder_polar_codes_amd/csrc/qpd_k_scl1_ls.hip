// qpd_k_scl1_ls.hip -- the list-output instantiations (lut_fast_kernel<..., ST = QPD_TAIL_LIST>,
// qpd_fast.hip: qpd_decode_list) of qpd_k_scl1.hip's kernels (SCL-LUT, one pointer word per path),
// as a unit of their own: the plain and status instantiations compile to what they were.
#define QPD_LIST_UNIT 1
#include "qpd_k_scl1.hip"
