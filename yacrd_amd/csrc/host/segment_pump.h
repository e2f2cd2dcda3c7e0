// segment_pump.h — a text of `total` bytes leaves its source in segments through the two halves of one buffer: the copy of
// segment i + 1 is started before segment i is handed to the sink, so the source's link and the sink work side by side.
// Plain C++, no device call: gpu_report_write.hip, gpu_inflate.hip and — for every editor, through way_out.h — gpu_out.h plug a
// DMA into `Link` (gpu_text.h: HomeLink), tools/segment_pump_check.cc a memcpy (the stand-alone program that runs this
// arithmetic under -fsanitize=address,undefined).  `Sink` is where every text path's bytes end up (gpu_deflate.hip's writer
// puts into one without the pump).
//
//   Link::start(i, dst, at, len)   begin copying text[at, at + len) to dst; false: the link failed
//   Link::wait(i)                  the copy of segment i has landed; false: the link failed
//   Link::drain()                  nothing is in flight any more (called on every way out)
#pragma once

#include <cerrno>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <unistd.h>

namespace yseg {

// where bytes go, one behind the other: a file descriptor at its running position (a fresh file), memory the caller
// sized (cap == 0), or memory from malloc that grows when it is full (cap != 0, or no memory yet: the size is not known in
// advance)
struct Sink {
    int fd = -1;
    char *mem = nullptr;
    uint64_t at = 0;  // bytes put so far
    uint64_t cap = 0; // of a growing `mem`
    bool put(const char *p, size_t k)
    {
        if (fd < 0 && (cap || !mem) && at + k > cap) {
            const uint64_t roomy = cap + cap / 2 + 4096, want = at + k > roomy ? at + k : roomy;
            char *q = (char *)std::realloc(mem, (size_t)want);
            if (!q) return false;
            mem = q, cap = want;
        }
        if (fd < 0) {
            if (k) std::memcpy(mem + at, p, k);
        }
        else
            for (size_t done = 0; done < k;) {
                const ssize_t w = ::write(fd, p + done, k - done);
                if (w < 0 && errno == EINTR) continue;
                if (w <= 0) return false;
                done += (size_t)w;
            }
        at += k;
        return true;
    }
};

enum { kPumped = 0, kLinkFailed = 1, kSinkFailed = 2 };

// segment i is text[i * seg, min((i + 1) * seg, total)) and passes through half i & 1; `halves` holds 2 * seg bytes, seg >= 1.
// The sink takes the segments behind whatever it holds already.  `around(f)` runs f, one put: the caller times it there (the
// writer's busy time).
template <class Link, class Around>
int pump(uint64_t total, uint64_t seg, char *halves, Link &link, Sink &sink, Around around)
{
    if (!total) return kPumped;
    if (seg > total) seg = total;
    char *half[2] = {halves, halves + seg};
    const uint64_t n_seg = (total + seg - 1) / seg;
    auto len_of = [&](uint64_t i) { return (size_t)(total - i * seg < seg ? total - i * seg : seg); };
    bool ok = link.start(0, half[0], 0, len_of(0)), written = true;
    for (uint64_t i = 0; i < n_seg && ok && written; i++) {
        ok = link.wait(i);
        if (ok && i + 1 < n_seg) ok = link.start(i + 1, half[(i + 1) & 1], (i + 1) * seg, len_of(i + 1));
        if (!ok) break;
        around([&] { written = sink.put(half[i & 1], len_of(i)); });
    }
    link.drain(); // (a copy may still be flying into a half)
    return !ok ? kLinkFailed : !written ? kSinkFailed : kPumped;
}

} // namespace yseg
