// Test program (CPU, stand-alone): the chunk buffer's policy (csrc/qpd_chunk.hpp)
// against a scripted allocator -- one that fails while the request exceeds a
// limit and records every call.  Each case asserts the exact sequence of
// allocator calls, the value reserve returns and the buffer's three fields.
// The blocks are real heap blocks, so under -fsanitize=address a double
// release or a use of a released block stops the program.  Prints "ok" and
// returns 0, or the first failed case and 1.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "qpd_chunk.hpp"

namespace {

struct Script {
    size_t limit;                 // an allocation of more bytes fails
    std::vector<std::string> log; // "a<bytes>+" / "a<bytes>-" (allocation, obtained / failed), "r" (release)
    int live = 0;                 // blocks handed out and not released
    void *alloc(size_t bytes) {
        const bool ok = bytes <= limit;
        log.push_back("a" + std::to_string(bytes) + (ok ? "+" : "-"));
        if (!ok) return nullptr;
        ++live;
        return std::malloc(bytes);
    }
    void release(void *p) {
        log.push_back("r");
        --live;
        std::free(p);
    }
};

int failures = 0;

std::string join(const std::vector<std::string> &v) {
    std::string s;
    for (const auto &x : v) s += (s.empty() ? "" : " ") + x;
    return s;
}

// One reserve call on (buf, script), then: what it returned, the calls it made, the buffer's state.
void step(const char *name, qpd::ChunkBuf &b, Script &s, int64_t want, size_t bpf, int64_t ret, const std::string &calls,
          int64_t cap, bool fell_back) {
    s.log.clear();
    const int64_t got = b.reserve(
        want, bpf, [&](size_t bytes) { return s.alloc(bytes); }, [&](void *p) { s.release(p); });
    const bool ok = got == ret && join(s.log) == calls && b.cap == cap && b.fell_back == fell_back && (b.p != nullptr) == (cap > 0) &&
                    s.live == (cap > 0 ? 1 : 0);
    if (ok) {
        if (b.p) static_cast<char *>(b.p)[(size_t)cap * bpf - 1] = 1;  // the block holds cap frames
        return;
    }
    ++failures;
    std::printf("FAIL %s: reserve(%lld, %zu) = %lld (want %lld), calls [%s] (want [%s]), cap %lld (want %lld), "
                "fell_back %d (want %d), p %s, live %d\n",
                name, (long long)want, bpf, (long long)got, (long long)ret, join(s.log).c_str(), calls.c_str(), (long long)b.cap,
                (long long)cap, (int)b.fell_back, (int)fell_back, b.p ? "set" : "null", s.live);
}

void finish(qpd::ChunkBuf &b, Script &s) {  // what the owner's destructor does
    if (b.p) s.release(b.p);
    b.p = nullptr;
    if (s.live != 0) {
        ++failures;
        std::printf("FAIL: %d blocks live at the end\n", s.live);
    }
}

}  // namespace

int main() {
    {  // the first request fits; a request within capacity makes no allocator call; a grow releases
       // the old block exactly once before allocating
        qpd::ChunkBuf b;
        Script s{1 << 20, {}};
        step("first fits", b, s, 100, 8, 100, "a800+", 100, false);
        step("within capacity", b, s, 100, 8, 100, "", 100, false);
        step("smaller", b, s, 7, 8, 7, "", 100, false);
        step("grow", b, s, 101, 8, 101, "r a808+", 101, false);
        finish(b, s);
    }
    {  // a failure at `want` succeeds at want / 2^k and sets the flag; from then on a larger request
       // is clamped and makes no allocator call, and the flag stays
        qpd::ChunkBuf b;
        Script s{300, {}};
        step("halves", b, s, 100, 10, 25, "a1000- a500- a250+", 25, true);
        step("clamped", b, s, 100, 10, 25, "", 25, true);
        step("clamped, larger", b, s, 1000000, 10, 25, "", 25, true);
        step("below the kept size", b, s, 3, 10, 3, "", 25, true);
        s.limit = 1 << 20;  // memory came back: the smaller size is kept all the same
        step("stays clamped", b, s, 100, 10, 25, "", 25, true);
        finish(b, s);
    }
    {  // odd sizes halve by integer division: 7, 3, 1
        qpd::ChunkBuf b;
        Script s{16, {}};
        step("odd halves", b, s, 7, 16, 1, "a112- a48- a16+", 1, true);
        finish(b, s);
    }
    {  // a grow that falls back: the old block is released once, before the first attempt
        qpd::ChunkBuf b;
        Script s{64, {}};
        step("fits", b, s, 8, 8, 8, "a64+", 8, false);
        step("grow falls back", b, s, 32, 8, 8, "r a256- a128- a64+", 8, true);
        finish(b, s);
    }
    {  // every size down to 1 fails: failure, a null pointer, zero capacity, no release of anything,
       // no flag (nothing smaller was kept); a later call tries again
        qpd::ChunkBuf b;
        Script s{0, {}};
        step("all fail", b, s, 5, 4, 0, "a20- a8- a4-", 0, false);
        step("all fail again", b, s, 2, 4, 0, "a8- a4-", 0, false);
        s.limit = 8;
        step("then fits", b, s, 2, 4, 2, "a8+", 2, false);
        finish(b, s);
    }
    {  // a grow whose every attempt fails: the old block is released once, never again
        qpd::ChunkBuf b;
        Script s{8, {}};
        step("fits", b, s, 2, 4, 2, "a8+", 2, false);
        s.limit = 0;
        step("grow, all fail", b, s, 4, 4, 0, "r a16- a8- a4-", 0, false);
        step("still failing", b, s, 1, 4, 0, "a4-", 0, false);
        finish(b, s);
    }
    {  // want = 1
        qpd::ChunkBuf b;
        Script s{4, {}};
        step("one frame", b, s, 1, 4, 1, "a4+", 1, false);
        step("one frame again", b, s, 1, 4, 1, "", 1, false);
        finish(b, s);
        qpd::ChunkBuf c;
        Script t{3, {}};
        step("one frame fails", c, t, 1, 4, 0, "a4-", 0, false);
        finish(c, t);
    }
    if (!failures) std::printf("ok\n");
    return failures ? 1 : 0;
}
