// qpd_fast_fscl1_st.hip -- the decode-status instantiations (lut_fast_kernel<..., ST = true>,
// qpd_fast.hip: qpd_decode_status) of qpd_fast_fscl1.hip's kernels (FastSCL-LUT, one pointer word per path),
// as a unit of their own: the plain instantiations compile to what they were.
#define QPD_STATUS_UNIT 1
#include "qpd_fast_fscl1.hip"
