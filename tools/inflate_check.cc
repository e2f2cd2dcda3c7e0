// inflate_check.cc — the inflate decoder's text (yacrd_amd/csrc/inflate_block.h) and the member walk (bgzf_walk.h) built
// for the host in a program of their own, so that they can run under a sanitizer:
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o inflate_check tools/inflate_check.cc
//   ./inflate_check cases.bin
//
// cases.bin (tests/inflate_cases.py: write_check_file): u64 count, then per record u64 stream bytes, u8 has_text, u64 text
// bytes, the stream, the text.  has_text 1: the stream must decode to the text; 0: it must be refused (not BGZF, or a
// member not taken); 2 (a mutated stream zlib still takes): refused, or exactly the text.  Every stream is copied into an
// allocation of exactly its size and every text is decoded into one, so a read beyond the input or a store beyond the text
// is the sanitizer's to see.  Exit status 0: every record came out as expected.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../yacrd_amd/csrc/bgzf_walk.h"
#include "../yacrd_amd/csrc/inflate_block.h"

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
    std::unique_ptr<yif::InfShared> sh(new yif::InfShared());
    uint64_t bad = 0, taken = 0, refused = 0;
    for (uint64_t k = 0; k < count; k++) {
        uint64_t n = 0, n_text = 0;
        unsigned char has_text = 0;
        if (!read_exact(f, &n, 8) || !read_exact(f, &has_text, 1) || !read_exact(f, &n_text, 8)) return 2;
        unsigned char *blob = (unsigned char *)std::malloc(n ? (size_t)n : 1); // exactly n bytes are the stream's
        std::vector<unsigned char> text((size_t)n_text);
        if (!blob || !read_exact(f, blob, (size_t)n) || !read_exact(f, text.data(), (size_t)n_text)) return 2;
        std::vector<yif::InfMember> members;
        uint64_t total = 0;
        bool ok = ybw::walk(blob, n, members, &total);
        // exactly `total` bytes are the text's: a store beyond a member's ISIZE is the sanitizer's to see
        unsigned char *got = (unsigned char *)std::malloc(ok && total ? (size_t)total : 1);
        const size_t n_got = ok ? (size_t)total : 0;
        if (!got) return 2;
        unsigned status = 0;
        for (size_t m = 0; ok && m < members.size(); m++) {
            const yif::InfMember &mm = members[m];
            const unsigned char *t = blob + mm.in_off + mm.csize;
            const uint32_t crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
            status = yif::inf_decode_member(*sh, blob + mm.in_off, mm.csize, mm.isize, crc, got + mm.out_off);
            if (status != yif::kInfOk) ok = false;
        }
        const bool same = ok && n_got == text.size() && (n_got == 0 || std::memcmp(got, text.data(), n_got) == 0);
        const bool as_expected = has_text == 1 ? same : has_text == 2 ? same || !ok : !ok;
        if (!as_expected) {
            bad++;
            std::fprintf(stderr, "record %llu: %s, expected %s (status %u: %s)\n", (unsigned long long)k, ok ? "taken" : "refused",
                         has_text == 1 ? "its text" : has_text == 2 ? "its text or a refusal" : "a refusal", status, yif::inf_status_name(status));
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
