// qpd_fast_fscl16_st.hip -- the decode-status instantiations (lut_fast_kernel<..., ST = true>,
// qpd_fast.hip: qpd_decode_status) of qpd_fast_fscl16.hip's kernels (FastSCL-LUT, list sizes 9..16),
// as a unit of their own: the plain instantiations compile to what they were.
#define QPD_STATUS_UNIT 1
#include "qpd_fast_fscl16.hip"
