// inflate_host.cc — the device decoder's text (../inflate_block.h) compiled for the host: one thread plays the 64 lanes of
// a wavefront, member after member.  What the tests without a GPU pin to zlib and what a sanitizer build runs (tools/
// inflate_check.cc); nobody's fast path (that is codec.cc's, on zlib).
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../../include/yacrd_host.h"
#include "../bgzf_plan.h"
#include "../bgzf_walk.h"
#include "../bgzf_windows.h"
#include "../edit_route.h"
#include "../inflate_block.h"
#include "host_common.h"

namespace yke { // inflate_sample.cc (also part of the engine library, which declares it in engine_internal.h)
int bgzf_text_ends(const unsigned char *comp, uint64_t comp_bytes, const yif::InfMember *members, uint64_t n_members, uint64_t max_text,
                   unsigned char delim, uint32_t *n_fields, bool *ends_nl, uint32_t *status);
}

extern "C" {

int yacrd_bgzf_decode_host(const char *data, uint64_t n, char **out, uint64_t *out_bytes)
{
    if ((!data && n) || !out || !out_bytes) return yh::fail("bad argument");
    *out = nullptr, *out_bytes = 0;
    const unsigned char *d = reinterpret_cast<const unsigned char *>(data);
    std::vector<yif::InfMember> members;
    uint64_t total = 0;
    if (!ybw::walk(d, n, members, &total)) return yh::fail("not BGZF");
    std::unique_ptr<yif::InfShared> sh(new (std::nothrow) yif::InfShared());
    char *res = (char *)std::malloc((size_t)total + 1);
    if (!sh || !res) {
        std::free(res);
        return yh::fail("host allocation failed");
    }
    for (size_t k = 0; k < members.size(); k++) {
        const yif::InfMember &m = members[k];
        const unsigned char *t = d + m.in_off + m.csize; // the trailer: inside the member (the walk)
        const uint32_t crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
        const uint32_t st = yif::inf_decode_member(*sh, d + m.in_off, m.csize, m.isize, crc, reinterpret_cast<unsigned char *>(res) + m.out_off);
        if (st != yif::kInfOk) {
            std::free(res);
            return yh::fail("BGZF member " + std::to_string(k) + " not taken: " + yif::inf_status_name(st));
        }
    }
    *out = res, *out_bytes = total;
    return 0;
}

int yacrd_bgzf_plan_segments(const char *data, uint64_t n, const uint64_t *landed, uint64_t n_landed, uint64_t chunk, uint64_t seg_chunks,
                             uint64_t **members_out, uint64_t *n_members, uint64_t **steps_out, uint64_t *n_steps)
{
    if ((!data && n) || (!landed && n_landed) || !members_out || !n_members || !steps_out || !n_steps) return yh::fail("bad argument");
    *members_out = *steps_out = nullptr, *n_members = *n_steps = 0;
    for (uint64_t k = 1; k < n_landed; k++)
        if (landed[k] < landed[k - 1]) return yh::fail("the landed bytes fall");
    std::vector<yif::InfMember> members;
    uint64_t total = 0;
    if (!ybw::walk(reinterpret_cast<const unsigned char *>(data), n, members, &total)) return yh::fail("not BGZF");
    std::vector<uint64_t> steps;
    try {
        ybw::SegmentPlan plan(members.data(), members.size(), total, chunk ? chunk : ybw::kPlanChunk, seg_chunks ? seg_chunks : ybw::kPlanSeg);
        ybw::PlanStep s;
        for (uint64_t k = 0; k < n_landed; k++)
            while (plan.next(landed[k], s)) steps.insert(steps.end(), {k, s.m0, s.m1, s.inflated, s.t0, s.t1, s.avail, s.last ? 1u : 0u});
    } catch (...) {
        return yh::fail("host allocation failed");
    }
    uint64_t *mo = (uint64_t *)std::malloc((members.size() * 4 + 1) * sizeof(uint64_t));
    uint64_t *so = (uint64_t *)std::malloc((steps.size() + 1) * sizeof(uint64_t));
    if (!mo || !so) {
        std::free(mo), std::free(so);
        return yh::fail("host allocation failed");
    }
    for (size_t k = 0; k < members.size(); k++)
        mo[4 * k] = members[k].in_off, mo[4 * k + 1] = members[k].csize, mo[4 * k + 2] = members[k].isize, mo[4 * k + 3] = members[k].out_off;
    if (!steps.empty()) std::memcpy(so, steps.data(), steps.size() * sizeof(uint64_t));
    *members_out = mo, *n_members = members.size(), *steps_out = so, *n_steps = steps.size() / 8;
    return 0;
}

int yacrd_bgzf_window_cuts(const char *data, uint64_t n, uint64_t window_bytes, uint64_t **cuts_out, uint64_t *n_cuts)
{
    if ((!data && n) || !cuts_out || !n_cuts) return yh::fail("bad argument");
    *cuts_out = nullptr, *n_cuts = 0;
    std::vector<yif::InfMember> members;
    uint64_t total = 0;
    if (!ybw::walk(reinterpret_cast<const unsigned char *>(data ? data : ""), n, members, &total)) return yh::fail("not BGZF");
    if (window_bytes < ybw::kMinWindow) return yh::fail("a BGZF window is at least 65 536 bytes");
    std::vector<ybw::WindowCut> cuts;
    if (!ybw::window_cuts(members.data(), members.size(), window_bytes, cuts)) return yh::fail("host allocation failed");
    uint64_t *co = (uint64_t *)std::malloc((cuts.size() * 6 + 1) * sizeof(uint64_t));
    if (!co) return yh::fail("host allocation failed");
    for (size_t k = 0; k < cuts.size(); k++) {
        const ybw::WindowCut &w = cuts[k];
        uint64_t *o = co + 6 * k;
        o[0] = w.m0, o[1] = w.m1, o[2] = w.c0, o[3] = w.c1, o[4] = w.t0, o[5] = w.t1;
    }
    *cuts_out = co, *n_cuts = cuts.size();
    return 0;
}

int yacrd_edit_window_route(uint64_t n, uint64_t window_switch, int whole_fits, int ring_fits, uint64_t *window_bytes, uint64_t *chunk_bytes)
{
    const uint64_t W = yer::window_of(window_switch);
    if (window_bytes) *window_bytes = W;
    if (chunk_bytes) *chunk_bytes = yer::chunk_of(W);
    return (int)yer::route(n, window_switch, whole_fits != 0, ring_fits != 0);
}

int yacrd_bgzf_text_ends(const char *data, uint64_t n, int delim, uint32_t *n_fields, int *ends_nl)
{
    if ((!data && n) || !n_fields || !ends_nl || delim < 0 || delim > 255) return yh::fail("bad argument");
    *n_fields = 0, *ends_nl = 1;
    const unsigned char *d = reinterpret_cast<const unsigned char *>(data ? data : "");
    std::vector<yif::InfMember> members;
    uint64_t total = 0;
    if (!ybw::walk(d, n, members, &total)) return yh::fail("not BGZF");
    bool nl = true;
    uint32_t status = 0;
    const int rc = yke::bgzf_text_ends(d, n, members.data(), members.size(), (uint64_t)1 << 20, (unsigned char)delim, n_fields, &nl, &status);
    if (rc == 1) return yh::fail(std::string("a BGZF member the device decoder does not take (") + yif::inf_status_name(status) + ")");
    if (rc == 2) return yh::fail("the first non-empty line is not complete within the first MiB of the text");
    if (rc) return yh::fail("host allocation failed");
    *ends_nl = nl ? 1 : 0;
    return 0;
}

} // extern "C"
