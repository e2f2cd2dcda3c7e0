// owners_check.hip — the owner types of csrc/engine_internal.h (DevBuf, PinBuf) on their own, meant for the host side's
// -fsanitize=address,undefined.  Only EMPTY owners: nothing is allocated, so no device is needed and none is touched.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -g -O1 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         tools/owners_check.hip -o owners_check
//   ./owners_check
//
// Move construction, move assignment (onto another object and onto itself), destruction, a growing std::vector of each (the
// stream's slabs are one), reserve(0) and release() on an empty owner; the process-wide byte counts stay at zero throughout.
// What an owner does with memory it really holds is the GPU tests' (tests/test_gpu_engine_life.py).  Exit status 0: all held.
#include "../yacrd_amd/csrc/engine_internal.h"

#include <cstdio>
#include <type_traits>
#include <utility>
#include <vector>

std::string &yke::err_slot() // (engine.hip's, for yke::fail)
{
    static thread_local std::string s;
    return s;
}

namespace {

int g_bad = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        if (!(c)) std::fprintf(stderr, "line %d: %s\n", __LINE__, #c), g_bad++; \
    } while (0)

bool counts_zero() { return yke::live_bytes()[0].load() == 0 && yke::live_bytes()[1].load() == 0; }

template <class Buf>
void check_empty_owner()
{
    static_assert(!std::is_copy_constructible<Buf>::value && !std::is_copy_assignable<Buf>::value, "an owner is never copied");
    static_assert(std::is_nothrow_move_constructible<Buf>::value && std::is_nothrow_move_assignable<Buf>::value, "std::vector moves it");
    Buf a;
    CHECK(a.p == nullptr && a.cap == 0);
    CHECK(a.reserve(0) == hipSuccess); // (bytes <= cap: nothing is asked of the runtime)
    a.release();
    Buf b(std::move(a));
    CHECK(a.p == nullptr && a.cap == 0 && b.p == nullptr && b.cap == 0);
    Buf c;
    c = std::move(b);
    Buf *self = &c;
    c = std::move(*self);
    CHECK(c.p == nullptr && c.cap == 0 && c.template as<char>() == nullptr);
    struct Slab { // (stream.hip's)
        Buf buf;
        uint64_t cap = 0, used = 0;
    };
    std::vector<Slab> slabs;
    std::vector<Buf> bufs;
    for (int i = 0; i < 1000; i++) { // (both reallocate many times on the way)
        slabs.emplace_back();
        slabs.back().cap = (uint64_t)i;
        bufs.emplace_back();
        CHECK(counts_zero());
    }
    for (int i = 0; i < 1000; i++) CHECK(slabs[i].cap == (uint64_t)i && slabs[i].buf.p == nullptr && bufs[i].cap == 0);
    slabs.erase(slabs.begin(), slabs.begin() + 500);
    slabs.pop_back();
    CHECK(slabs.size() == 499 && slabs[0].cap == 500);
    CHECK(counts_zero());
}

} // namespace

int main()
{
    check_empty_owner<yke::DevBuf>();
    check_empty_owner<yke::PinBuf>();
    {
        yke::Events ev; // (empty ones go without a call into the runtime as well)
        yke::Streams st;
        CHECK(ev.add(0) && st.add(0) && ev.v.empty() && st.v.empty());
    }
    CHECK(counts_zero());
    std::printf(g_bad ? "owners_check: %d checks failed\n" : "owners_check: ok\n", g_bad);
    return g_bad ? 1 : 0;
}
