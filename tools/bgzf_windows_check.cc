// bgzf_windows_check.cc — where the windows of a BGZF text end (yacrd_amd/csrc/bgzf_windows.h) over the member walk
// (bgzf_walk.h), built for the host in a program of its own, so that it can run under a sanitizer:
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o bgzf_windows_check tools/bgzf_windows_check.cc
//   ./bgzf_windows_check cases.bin
//
// cases.bin (tests/test_bgzf_windows.py: write_cuts_file): u64 count, then per record u64 stream bytes, u64 W, u64 the number
// of windows expected, the stream.  Every stream and every member table lies in an allocation of exactly its size.  Checked
// per record: the cuts partition [0, M), the stream and the text; both caps hold for every window; no window could have
// taken its successor's first member; with neither cap binding there is one cut; the count is the expected one.  A W under
// 65 536 must be refused.  Exit status 0: every record held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../yacrd_amd/csrc/bgzf_walk.h"
#include "../yacrd_amd/csrc/bgzf_windows.h"

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
    uint64_t count = 0, bad = 0, n_cuts = 0;
    if (!read_exact(f, &count, 8)) return 2;
    for (uint64_t k = 0; k < count; k++) {
        uint64_t n = 0, W = 0, want = 0;
        if (!read_exact(f, &n, 8) || !read_exact(f, &W, 8) || !read_exact(f, &want, 8)) return 2;
        unsigned char *blob = (unsigned char *)std::malloc(n ? (size_t)n : 1);
        if (!blob || !read_exact(f, blob, (size_t)n)) return 2;
        std::vector<yif::InfMember> walked;
        uint64_t total = 0;
        if (!ybw::walk(blob, n, walked, &total)) {
            std::fprintf(stderr, "record %llu: not BGZF\n", (unsigned long long)k);
            return 2;
        }
        const size_t M = walked.size();
        yif::InfMember *mem = (yif::InfMember *)std::malloc(M ? M * sizeof(yif::InfMember) : 1); // exactly M members
        if (!mem) return 2;
        if (M) std::memcpy(mem, walked.data(), M * sizeof(yif::InfMember));
        const char *why = nullptr;
        std::vector<ybw::WindowCut> cuts;
        const bool made = ybw::window_cuts(mem, M, W, cuts);
        if (W < ybw::kMinWindow) {
            if (made || !cuts.empty()) why = "a window under 65 536 bytes was not refused";
        } else if (!made) why = "refused";
        else {
            uint64_t m = 0, c = 0, t = 0;
            for (size_t j = 0; j < cuts.size() && !why; j++) {
                const ybw::WindowCut &w = cuts[j];
                if (w.m0 != m || w.c0 != c || w.t0 != t) why = "the cuts do not follow one another";
                else if (w.m1 <= w.m0 || w.m1 > M) why = "a window without a member, or beyond the table";
                else if (w.c1 != mem[w.m1 - 1].in_off + mem[w.m1 - 1].csize + 8u) why = "c1 is not the end of the last member's trailer";
                else if (w.t1 != mem[w.m1 - 1].out_off + mem[w.m1 - 1].isize) why = "t1 is not the end of the last member's text";
                else if (w.c1 - w.c0 > W || w.t1 - w.t0 > W) why = "a cap does not hold";
                else if (w.m1 < M) {
                    const yif::InfMember &x = mem[w.m1];
                    if (x.out_off + x.isize - w.t0 <= W && x.in_off + x.csize + 8u - w.c0 <= W) why = "a window could have taken the next member";
                }
                m = w.m1, c = w.c1, t = w.t1;
            }
            if (!why && (m != M || c != n || t != total)) why = "the cuts do not cover the table, the stream and the text";
            if (!why && M && n <= W && total <= W && cuts.size() != 1) why = "more than one cut with neither cap binding";
            if (!why && !M && !cuts.empty()) why = "a cut of no members";
            if (!why && cuts.size() != want) why = "not the expected number of windows";
            n_cuts += cuts.size();
        }
        if (why) {
            bad++;
            std::fprintf(stderr, "record %llu (%llu members, %llu bytes of text, W %llu): %s\n", (unsigned long long)k, (unsigned long long)M,
                         (unsigned long long)total, (unsigned long long)W, why);
        }
        std::free(blob), std::free(mem);
    }
    std::fclose(f);
    std::printf("%llu records, %llu cuts, %llu not as expected\n", (unsigned long long)count, (unsigned long long)n_cuts, (unsigned long long)bad);
    return bad ? 1 : 0;
}
