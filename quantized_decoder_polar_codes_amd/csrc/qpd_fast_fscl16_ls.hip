// qpd_fast_fscl16_ls.hip -- the list-output instantiations (lut_fast_kernel<..., ST = QPD_TAIL_LIST>,
// qpd_fast.hip: qpd_decode_list) of qpd_fast_fscl16.hip's kernels (FastSCL-LUT, list sizes 9..16),
// as a unit of their own: the plain and status instantiations compile to what they were.
#define QPD_LIST_UNIT 1
#include "qpd_fast_fscl16.hip"
