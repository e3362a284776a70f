// qpd_dmetric.hpp -- the argument rules of qpd_dmetric / qpd_dmetric_host (qpd.h)
// and the host engine's metric run.  Host code without HIP, as qpd_status.hpp:
// the CPU tests build it beside the host engine (tests/native/dmetric_harness.cpp).
#pragma once
#include <cstdint>
#include <string>

#include "qpd.h"
#include "qpd_host.hpp"

namespace qpd_dm {

// The reference's class name of a decoder kind (enum qpd_kind), for messages.
inline const char *kind_name(int kind) {
    static const char *const names[] = {"SCDecoder", "SCLUTDecoder", "SCLLUTDecoder", "FastSCLUTDecoder",
                                        "FastSCLLUTDecoder", "CASCLLUTDecoder", "CAFastSCLLUTDecoder", "SCLDecoder",
                                        "CASCLDecoder", "FastSCDecoder", "FastSCLDecoder", "SCUniformQuantizedDecoder",
                                        "SCLUniformQuantizedDecoder", "SCLloydQuantizedDecoder",
                                        "SCLLloydQuantizedDecoder"};
    return kind >= 0 && kind < (int)(sizeof(names) / sizeof(names[0])) ? names[kind] : "unknown kind";
}

// kind: the decoder's public kind (qpd_config.kind).  The metric is the float
// FastSC traversal's (DMetric.cpp:24-177 is FastSCDecoder.cpp:21-151 plus one
// accumulator), so only that decoder computes it; metric is the required output.
// Returns QPD_OK or the refusal with its message in err.
inline int check(int kind, const void *metric, std::string &err) {
    if (kind != QPD_FASTSC_FLOAT) {
        err = std::string("the blind-detection metric needs a FastSCDecoder (QPD_FASTSC_FLOAT): this decoder is a ") +
              kind_name(kind) + " (kind " + std::to_string(kind) + ")";
        return QPD_E_INVALID;
    }
    if (!metric) {
        err = "metric is NULL";
        return QPD_E_INVALID;
    }
    return QPD_OK;
}

// B frames on the host engine: their metrics and, where h_out is given, their
// bits (host pointers).  Returns the frames' error flags ORed (qpd::ErrFlag).
template <class Eng>
int host_run(Eng *eng, const double *h_llr, int64_t B, int N, int out_bits, double *h_metric, uint8_t *h_out) {
    int32_t flag = 0;
    eng->want_dmetric = true;
    for (int64_t b = 0; b < B; ++b) {
        const int f = eng->decode(h_llr + b * N, h_out ? h_out + b * out_bits : nullptr);
        flag |= f;
        if (!f) h_metric[b] = eng->last_dmetric;
    }
    eng->want_dmetric = false;
    return flag;
}

}  // namespace qpd_dm
