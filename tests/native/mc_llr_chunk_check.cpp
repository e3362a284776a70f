// mc_llr_chunk_check.cpp -- prints qpd_mc_decode_f64's frames per chunk
// (csrc/qpd_chunk.hpp: mc_llr_chunk_frames) for each code length given on the
// command line, one per line (tests/test_mc_llr.py).
#include <cstdio>
#include <cstdlib>

#include "qpd_chunk.hpp"

int main(int argc, char **argv) {
    for (int i = 1; i < argc; ++i) std::printf("%lld\n", (long long)qpd::mc_llr_chunk_frames(std::atoi(argv[i])));
    return 0;
}
