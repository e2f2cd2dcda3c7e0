// bgzf_plan.h — what to inflate and what to hand on while a BGZF stream is still landing in HBM: plain C++, no HIP.  Shared by
// the engine library (gpu_inflate.hip: move_bgzf_text), libyacrd_host (host/inflate_host.cc: yacrd_bgzf_plan_segments, for the
// tests without a GPU) and tools/bgzf_plan_check.cc (the same under a sanitizer).
//
// In: the walked member table (bgzf_walk.h) and, call after call, the number of COMPRESSED bytes that have landed — a
// sequence that never falls, move_text's `avail` over the compressed stream.  Out, step by step:
//   [m0, m1)     the members that have become complete (in_off + csize + 8 <= landed: payload and trailer) and have not been
//                launched yet: one launch of the decoder.  Every member is in exactly one step's range.
//   inflated     the text that is whole once that launch has run: the out_off of the first member not yet launched, or
//                all of it
//   [t0, t1)     the segment of TEXT to hand to the consumer behind that launch, under move_text's contract: t0 and t1 are
//                multiples of `chunk`, a segment is `seg_chunks` chunks (the last one what is left, and its t1 may lie beyond
//                the text), `avail` reaches one chunk beyond t1 or is the whole text, and never exceeds `inflated`.  t0 == t1: no
//                segment in this step.  The segments tile the text once, in order.
//   last         the step that ends the text.  A text of no bytes (no members, or EOF members only) ends in one step with
//                an empty segment.
// next() gives one step per call and false when nothing more can be done before more bytes land.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "inflate_block.h" // yif::InfMember

namespace ybw {

constexpr uint64_t kPlanChunk = (uint64_t)4 << 20; // move_text's: what one copy moves,
constexpr uint64_t kPlanSeg = 32;                  // and the chunks of a segment

struct PlanStep {
    uint64_t m0, m1, inflated, t0, t1, avail;
    bool last;
};

class SegmentPlan {
public:
    SegmentPlan(const yif::InfMember *members, uint64_t n_members, uint64_t text_bytes, uint64_t chunk = kPlanChunk, uint64_t seg_chunks = kPlanSeg)
        : mem_(members), n_mem_(n_members), n_(text_bytes), chunk_(chunk ? chunk : 1), seg_(seg_chunks ? seg_chunks : 1)
    {
        n_chunks_ = n_ / chunk_ + (n_ % chunk_ ? 1u : 0u);
    }
    bool done() const { return done_; }
    bool next(uint64_t landed, PlanStep &s)
    {
        if (done_) return false;
        s.m0 = next_m_;
        while (next_m_ < n_mem_ && mem_[next_m_].in_off <= landed && landed - mem_[next_m_].in_off >= (uint64_t)mem_[next_m_].csize + 8u) next_m_++;
        s.m1 = next_m_;
        s.inflated = next_m_ < n_mem_ ? std::min(mem_[next_m_].out_off, n_) : n_;
        s.t0 = s.t1 = next_c_ * chunk_, s.avail = std::min(n_, s.t0), s.last = false;
        const uint64_t c1 = std::min(next_c_ + seg_, n_chunks_), need = std::min(c1 + 1, n_chunks_);
        const uint64_t want = std::min(n_, need * chunk_); // (no overflow: need * chunk < n + chunk)
        if (next_c_ < n_chunks_ && s.inflated >= want) {
            s.t1 = c1 * chunk_, s.avail = want;
            next_c_ = c1;
        }
        // the text ends with its last segment; the members behind it (EOF members) end the run
        if (next_c_ == n_chunks_ && next_m_ == n_mem_) s.last = done_ = true;
        return s.m1 > s.m0 || s.t1 > s.t0 || s.last;
    }

private:
    const yif::InfMember *mem_;
    uint64_t n_mem_, n_, chunk_, seg_, n_chunks_ = 0, next_m_ = 0, next_c_ = 0;
    bool done_ = false;
};

} // namespace ybw
