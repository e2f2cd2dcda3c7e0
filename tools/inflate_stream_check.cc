// inflate_stream_check.cc — the plain-gzip decoder's text (yacrd_amd/csrc/inflate_stream.h) and the header walk
// (gzip_walk.h) built for the host in a program of their own, so that they can run under a sanitizer:
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o inflate_stream_check tools/inflate_stream_check.cc
//   ./inflate_stream_check cases.bin
//
// cases.bin (tests/gunzip_stream_cases.py: write_check_file): u64 count, then per record u64 stream bytes, u32 chunk, u8
// has_text, u64 text bytes, the stream, the text.  has_text 1: the stream must decode to the text; 0: it must be refused
// (not a gzip member, or a payload not taken); 2 (a mutated stream zlib still takes): refused, or exactly the text.  Every
// stream is copied into an allocation of exactly its size; the decoder allocates exactly the text's symbols and bytes
// (str_decode_host), so a read beyond the input, a store beyond the text or a marker that leads outside the scratch is the
// sanitizer's to see.  Exit status 0: every record came out as expected.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../yacrd_amd/csrc/gzip_walk.h"
#include "../yacrd_amd/csrc/inflate_stream.h"

static bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
        return 2;
    }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    uint64_t count = 0;
    if (!read_exact(f, &count, 8)) return 2;
    uint64_t bad = 0, taken = 0, refused = 0;
    for (uint64_t k = 0; k < count; k++) {
        uint64_t n = 0, n_text = 0;
        uint32_t chunk = 0;
        unsigned char has_text = 0;
        if (!read_exact(f, &n, 8) || !read_exact(f, &chunk, 4) || !read_exact(f, &has_text, 1) || !read_exact(f, &n_text, 8)) return 2;
        unsigned char *blob = (unsigned char *)std::malloc(n ? (size_t)n : 1); // exactly n bytes are the stream's
        std::vector<unsigned char> text((size_t)n_text);
        if (!blob || !read_exact(f, blob, (size_t)n) || !read_exact(f, text.data(), (size_t)n_text)) return 2;
        ygw::GzipFrame fr;
        int status = -2; // (not a gzip member)
        unsigned char *got = nullptr;
        yis::StreamCounts c;
        if (ygw::walk(blob, n, &fr)) status = yis::str_decode_host(blob + fr.payload_off, fr.payload_bytes, fr.crc, fr.isize, chunk, &got, c);
        if (status == -1) return 2; // (no memory)
        const bool ok = status == 0;
        const bool same = ok && c.out_bytes == text.size() && (text.empty() || std::memcmp(got, text.data(), text.size()) == 0);
        const bool as_expected = has_text == 1 ? same : has_text == 2 ? same || !ok : !ok;
        if (!as_expected) {
            bad++;
            std::fprintf(stderr, "record %llu: %s, expected %s (status %d: %s)\n", (unsigned long long)k, ok ? "taken" : "refused",
                         has_text == 1 ? "its text" : has_text == 2 ? "its text or a refusal" : "a refusal", status,
                         status > 0 ? yis::str_status_name((uint32_t)status) : status == -2 ? "not a gzip member" : "ok");
        }
        (ok ? taken : refused)++;
        std::free(blob);
        std::free(got);
    }
    std::fclose(f);
    std::printf("%llu records: %llu taken, %llu refused, %llu not as expected\n", (unsigned long long)count, (unsigned long long)taken,
                (unsigned long long)refused, (unsigned long long)bad);
    return bad ? 1 : 0;
}
