// bgzf_plan_check.cc — the planner of the segment-wise device inflate (yacrd_amd/csrc/bgzf_plan.h) over the member walk
// (bgzf_walk.h), built for the host in a program of its own, so that it can run under a sanitizer:
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o bgzf_plan_check tools/bgzf_plan_check.cc
//   ./bgzf_plan_check schedules.bin
//
// schedules.bin (tests/test_bgzf_plan.py: write_plan_file): u64 count, then per record u64 stream bytes, u64 chunk, u64
// seg_chunks, u64 landings, the stream, the landings (u64 each, never falling, the last one the stream's size).  Every stream
// and every member table lies in an allocation of exactly its size.  Checked per record: every member is launched exactly
// once and only when its trailer has landed; the text segments tile [0, n) in order, on chunk boundaries; avail never
// exceeds the inflated text and reaches a chunk beyond the segment or the text's end; exactly one step ends the text, and it
// is the last.  Exit status 0: every record held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../yacrd_amd/csrc/bgzf_plan.h"
#include "../yacrd_amd/csrc/bgzf_walk.h"

static bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s schedules.bin\n", argv[0]);
        return 2;
    }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) {
        std::perror(argv[1]);
        return 2;
    }
    uint64_t count = 0, bad = 0, steps = 0;
    if (!read_exact(f, &count, 8)) return 2;
    for (uint64_t k = 0; k < count; k++) {
        uint64_t n = 0, chunk = 0, seg = 0, n_landed = 0;
        if (!read_exact(f, &n, 8) || !read_exact(f, &chunk, 8) || !read_exact(f, &seg, 8) || !read_exact(f, &n_landed, 8)) return 2;
        unsigned char *blob = (unsigned char *)std::malloc(n ? (size_t)n : 1);
        uint64_t *landed = (uint64_t *)std::malloc(n_landed ? (size_t)n_landed * 8 : 1);
        if (!blob || !landed || !read_exact(f, blob, (size_t)n) || !read_exact(f, landed, (size_t)n_landed * 8)) return 2;
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
        uint64_t next_m = 0, next_t = 0, ends = 0;
        ybw::SegmentPlan plan(mem, M, total, chunk, seg);
        ybw::PlanStep s;
        for (uint64_t j = 0; j < n_landed && !why; j++)
            while (!why && plan.next(landed[j], s)) {
                steps++;
                if (ends) why = "a step behind the last";
                if (s.m0 != next_m || s.m1 < s.m0 || s.m1 > M) why = "member ranges are not consecutive";
                for (uint64_t m = s.m0; !why && m < s.m1; m++)
                    if (mem[m].in_off + mem[m].csize + 8u > landed[j]) why = "a member launched before its trailer landed";
                if (!why && s.m1 < M && mem[s.m1].in_off + mem[s.m1].csize + 8u <= landed[j]) why = "a complete member left behind";
                if (!why) next_m = s.m1;
                const uint64_t inflated = next_m < M ? mem[next_m].out_off : total;
                if (!why && s.inflated != inflated) why = "inflated is not the first unlaunched member's place";
                if (!why && s.t1 > s.t0) {
                    if (s.t0 != next_t || s.t0 % chunk || s.t1 % chunk || s.t1 - s.t0 > seg * chunk) why = "text segments do not tile on chunk boundaries";
                    else if (s.avail > inflated || s.avail > total) why = "avail exceeds the inflated text";
                    else if (s.avail != total && s.avail < s.t1 + chunk) why = "avail neither a chunk beyond the segment nor the text's end";
                    else if (s.t1 < total && s.t1 - s.t0 != seg * chunk) why = "a short segment that is not the last";
                    next_t = s.t1;
                }
                if (s.last) ends++;
            }
        if (!why && next_m != M) why = "members never launched";
        if (!why && next_t < total) why = "text never handed on";
        if (!why && ends != 1) why = "not exactly one step ends the text";
        if (!why && !plan.done()) why = "the plan is not done";
        if (why) {
            bad++;
            std::fprintf(stderr, "record %llu (%llu members, %llu bytes of text, chunk %llu x %llu): %s\n", (unsigned long long)k, (unsigned long long)M,
                         (unsigned long long)total, (unsigned long long)chunk, (unsigned long long)seg, why);
        }
        std::free(blob), std::free(landed), std::free(mem);
    }
    std::fclose(f);
    std::printf("%llu records, %llu steps, %llu not as expected\n", (unsigned long long)count, (unsigned long long)steps, (unsigned long long)bad);
    return bad ? 1 : 0;
}
