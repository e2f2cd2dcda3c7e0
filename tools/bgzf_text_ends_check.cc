// bgzf_text_ends_check.cc — what the device overlap editor asks of a BGZF text before its first launch
// (yacrd_amd/csrc/host/inflate_sample.cc: bgzf_text_ends) over the member walk (bgzf_walk.h), built for the host in a program
// of its own, so that it can run under a sanitizer:
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o bgzf_text_ends_check tools/bgzf_text_ends_check.cc
//   ./bgzf_text_ends_check cases.bin
//
// cases.bin (tests/inflate_cases.py: write_check_file): u64 count, then per record u64 stream bytes, u8 has_text, u64 text
// bytes, the stream, the text.  has_text 1: the helper must answer, for a tab and for a space as the delimiter, what the
// plain rule (below: gpu_edit.hip's first_line_fields, restated) answers on the text; 0: it must refuse the stream (not
// BGZF, a sampled member not taken, a first line that outgrows the sample).  bgzf_last_byte — the last byte alone, what a BGZF
// FASTQ / FASTA in windows asks — runs over the same records: the text's last byte where has_text is 1; elsewhere an answer or a
// status that agree, under the sanitizers.  Every stream and every member table lies in an
// allocation of exactly its size.  Exit status 0: every record came out as expected.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../yacrd_amd/csrc/bgzf_walk.h"
#include "../yacrd_amd/csrc/host/inflate_sample.cc"

static bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

// the field count of the first non-empty line (0: none), whether the last byte is a newline (true for no bytes)
static void plain_rule(const std::vector<unsigned char> &t, unsigned char delim, uint32_t &n_fields, bool &ends_nl)
{
    n_fields = 0, ends_nl = t.empty() || t.back() == '\n';
    bool in_line = false;
    uint32_t nf = 0;
    for (unsigned char c : t) {
        if (c == '\n') {
            if (in_line) break;
            continue;
        }
        if (!in_line) in_line = true, nf = 1;
        if (c == delim) nf++;
    }
    if (in_line) n_fields = nf;
}

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
    uint64_t count = 0, bad = 0, answered = 0, refused = 0;
    if (!read_exact(f, &count, 8)) return 2;
    for (uint64_t k = 0; k < count; k++) {
        uint64_t n = 0, n_text = 0;
        unsigned char has_text = 0;
        if (!read_exact(f, &n, 8) || !read_exact(f, &has_text, 1) || !read_exact(f, &n_text, 8)) return 2;
        unsigned char *blob = (unsigned char *)std::malloc(n ? (size_t)n : 1); // exactly n bytes are the stream's
        std::vector<unsigned char> text((size_t)n_text);
        if (!blob || !read_exact(f, blob, (size_t)n) || !read_exact(f, text.data(), (size_t)n_text)) return 2;
        std::vector<yif::InfMember> walked;
        uint64_t total = 0;
        bool ok = ybw::walk(blob, n, walked, &total);
        const bool is_bgzf = ok;
        const size_t M = walked.size();
        yif::InfMember *mem = (yif::InfMember *)std::malloc(M ? M * sizeof(yif::InfMember) : 1); // exactly M members
        if (!mem) return 2;
        if (M) std::memcpy(mem, walked.data(), M * sizeof(yif::InfMember));
        const char *why = nullptr;
        for (int d = 0; d < 2 && ok && !why; d++) {
            const unsigned char delim = d ? ' ' : '\t';
            uint32_t nf = 77, status = 0, want_nf = 0;
            bool nl = false, want_nl = true;
            const int rc = yke::bgzf_text_ends(blob, n, mem, M, (uint64_t)1 << 20, delim, &nf, &nl, &status);
            if (rc) {
                ok = false;
                break;
            }
            if (has_text != 1) continue;
            plain_rule(text, delim, want_nf, want_nl);
            if (total != text.size()) why = "the walk's text size is not the text's";
            else if (nf != want_nf) why = "another field count than the plain rule's";
            else if (nl != want_nl) why = "another last byte than the plain rule's";
        }
        if (!why && ok && has_text == 1) { // bgzf_last_byte: the second answer alone, from the last member that holds text
            bool nl = false;
            uint32_t status = 77;
            if (yke::bgzf_last_byte(blob, n, mem, M, &nl, &status) != 0 || status != yif::kInfOk) why = "bgzf_last_byte refused a text that is answered";
            else if (nl != (text.empty() || text.back() == '\n')) why = "bgzf_last_byte: another last byte than the text's";
        }
        if (is_bgzf && has_text != 1) { // a stream to refuse: whatever its last member holds, an answer or a status, nothing else
            bool nl = false;
            uint32_t status = 77;
            const int rc = yke::bgzf_last_byte(blob, n, mem, M, &nl, &status);
            if (rc != 0 && rc != 1) why = "bgzf_last_byte: neither an answer nor a status";
            else if ((rc == 1) != (status != yif::kInfOk)) why = "bgzf_last_byte: code and status disagree";
        }
        if (!why && ok != (has_text == 1)) why = ok ? "answered, expected a refusal" : "refused, expected an answer";
        if (why) {
            bad++;
            std::fprintf(stderr, "record %llu (%llu members, %llu bytes of text): %s\n", (unsigned long long)k, (unsigned long long)M,
                         (unsigned long long)total, why);
        }
        (ok ? answered : refused)++;
        std::free(blob), std::free(mem);
    }
    std::fclose(f);
    std::printf("%llu records: %llu answered, %llu refused, %llu not as expected\n", (unsigned long long)count, (unsigned long long)answered,
                (unsigned long long)refused, (unsigned long long)bad);
    return bad ? 1 : 0;
}
