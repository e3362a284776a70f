// qpd_tx_kernels.hpp -- what the C-ABI's unit (qpd_capi.hip) and the transmit
// kernels' unit (qpd_tx.hip) agree on: the kernels' pointer block, the output
// modes, and the kernels' addresses for hipLaunchKernel.
#pragma once
#include <stdint.h>

namespace qpd {

// What tx_frames_kernel writes per frame: int32 symbols, uint8 symbols, the
// float64 LLRs, or the reconstruction values of the LLRs' symbols (qpd_tx_out,
// the last with rec).
enum TxOut { TX_SYM_I32 = 0, TX_SYM_U8 = 1, TX_LLR = 2, TX_LLR_REC = 3 };

struct TxIo {
    const uint8_t *msg;  // [B][A]; tx_frames_kernel with no_signal: not read, may be null
    uint8_t *info;       // tx_encode_kernel: [B][K] or null
    uint8_t *cw;         // tx_encode_kernel: [B][N] or null
    void *frames;        // tx_frames_kernel: [B][N] of the output mode's type
    int32_t *err;        // the decoder's error word (ERR_MSG_BIT)
    uint32_t mask;       // CRC mask as a register word (qpd_tx::check_common)
    int32_t no_signal;   // tx_frames_kernel: y = sigma * noise
};

const void *tx_encode_kernel_fn();         // tx_encode_kernel(McChannel, int64_t B, TxIo)
const void *tx_frames_kernel_fn(int out);  // tx_frames_kernel<out>(McChannel, int64_t frame0, int64_t B, TxIo)

}  // namespace qpd
