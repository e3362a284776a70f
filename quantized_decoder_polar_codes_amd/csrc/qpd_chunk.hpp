// qpd_chunk.hpp -- the per-decoder buffer of one chunk of frames: grown on
// demand, halved on an allocation failure, the smaller size kept from then on
// (fewer frames per launch, same results).  Host code without HIP: the policy
// is checked on the CPU with a scripted allocator (tests/test_capi_host.py);
// the library's allocator is hipMalloc / hipFree (qpd_decoder.hpp: DeviceChunk).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace qpd {

struct ChunkBuf {
    void *p = nullptr;
    int64_t cap = 0;         // frames p holds
    bool fell_back = false;  // an allocation failed: cap is the chunk from then on (never cleared)

    // Room for `want` >= 1 frames of bytes_per_frame each.  Returns the frames
    // per chunk (<= want), or 0 with p == nullptr when no size down to one
    // frame could be allocated.  alloc(bytes) returns the block or nullptr,
    // release(block) frees it.
    template <class Alloc, class Release>
    int64_t reserve(int64_t want, size_t bytes_per_frame, Alloc &&alloc, Release &&release) {
        // after a fallback the smaller buffer is the chunk: no device-wide free
        // and failing allocations on every later call
        if (fell_back) want = std::min(want, cap);
        if (cap >= want) return want;
        if (p) release(p);
        p = nullptr;
        cap = 0;
        for (int64_t got = want; got >= 1; got /= 2) {
            if ((p = alloc((size_t)got * bytes_per_frame))) {
                fell_back = fell_back || got < want;
                cap = got;
                return got;
            }
        }
        return 0;
    }
};

// qpd_mc_decode_f64's frames per chunk (qpd.h): 2^28 bytes (256 MB) of float64
// LLRs, at least one frame.
inline int64_t mc_llr_chunk_frames(int N) { return std::max<int64_t>(1, ((int64_t)1 << 28) / (8 * (int64_t)N)); }

}  // namespace qpd
