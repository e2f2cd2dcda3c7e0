// inflate_stream_host.cc — the plain-gzip decoder's text (../inflate_stream.h, ../gzip_walk.h) compiled for the host: one
// thread plays every wavefront and every team of the five steps, one after the other.  What the tests without a GPU pin to
// zlib, what yacrd_engine_gunzip_stream_mem's counters are compared with, and what a sanitizer build runs (tools/
// inflate_stream_check.cc); nobody's fast path (that is codec.cc's, on zlib).
#include <cstdlib>
#include <string>

#include "../../../include/yacrd_host.h"
#include "../gzip_walk.h"
#include "../inflate_stream.h"
#include "host_common.h"

extern "C" {

int yacrd_gzip_stream_decode_host(const char *data, uint64_t n, uint32_t chunk, char **out, uint64_t *out_bytes, uint64_t counters[6])
{
    if ((!data && n) || !out || !out_bytes) return yh::fail("bad argument");
    *out = nullptr, *out_bytes = 0;
    const unsigned char *d = reinterpret_cast<const unsigned char *>(data ? data : "");
    ygw::GzipFrame f;
    if (!ygw::walk(d, n, &f)) return yh::fail("not a gzip member");
    yis::StreamCounts c;
    unsigned char *text = nullptr;
    const int st = yis::str_decode_host(d + f.payload_off, f.payload_bytes, f.crc, f.isize, chunk ? chunk : yis::kDefaultChunk, &text, c);
    if (st < 0) return yh::fail("host allocation failed");
    if (st) return yh::fail(std::string("gzip stream not taken: ") + yis::str_status_name((uint32_t)st));
    *out = reinterpret_cast<char *>(text), *out_bytes = c.out_bytes;
    if (counters)
        counters[0] = c.n_chunks, counters[1] = c.n_spans, counters[2] = c.n_false_starts, counters[3] = c.rounds, counters[4] = c.n_blocks,
        counters[5] = c.out_bytes;
    return 0;
}

} // extern "C"
