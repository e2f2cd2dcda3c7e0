// bgzf_windows.h — where the windows of a BGZF text end: plain C++, no HIP and no zlib.  Shared by the engine library
// (gpu_seq_edit.hip: a BGZF FASTQ / FASTA edited window by window), libyacrd_host (host/inflate_host.cc:
// yacrd_bgzf_window_cuts, for the tests without a GPU) and tools/bgzf_windows_check.cc (the same under a sanitizer).
//
// A member inflates as a unit, so a window of a BGZF run ends where a member ends, not at a multiple of W.  In: the walked
// member table (bgzf_walk.h) and W.  Out: the cuts, one per window —
//   [m0, m1)   the window's members
//   [c0, c1)   the bytes of the COMPRESSED STREAM that hold those members' whole frames: c0 is the end of member m0 - 1's
//              trailer (0 for the first window), c1 = in_off[m1 - 1] + csize[m1 - 1] + 8.  The walk takes no gaps between
//              frames, so the windows' ranges tile the stream.
//   [t0, t1)   the window's text
// The rule is greedy: a window takes members while t1 - t0 <= W AND c1 - c0 <= W, and always at least one.  A frame is at
// most 65 536 bytes and an ISIZE at most 65 536, so with W >= kMinWindow both caps hold for every window.  Members of
// ISIZE 0 (EOF members, anywhere) are taken like any other: a window may hold no text at all.  The last window is the one
// with m1 == M; a table of no members has no window.
#pragma once
#include <stdint.h>

#include <vector>

#include "inflate_block.h" // yif::InfMember

namespace ybw {

constexpr uint64_t kMinWindow = 65536; // the largest frame, the largest ISIZE: under it a single member may exceed a cap

struct WindowCut {
    uint64_t m0, m1, c0, c1, t0, t1;
};

// false: W is under kMinWindow, or no memory.  `cuts` is cleared first.
inline bool window_cuts(const yif::InfMember *members, uint64_t n_members, uint64_t W, std::vector<WindowCut> &cuts)
{
    cuts.clear();
    if (W < kMinWindow) return false;
    try {
        uint64_t m = 0, c = 0, t = 0;
        while (m < n_members) {
            WindowCut w{m, m, c, c, t, t};
            while (w.m1 < n_members) {
                const yif::InfMember &x = members[w.m1];
                const uint64_t c1 = x.in_off + (uint64_t)x.csize + 8u, t1 = x.out_off + (uint64_t)x.isize;
                if (w.m1 > w.m0 && (t1 - w.t0 > W || c1 - w.c0 > W)) break;
                w.m1++, w.c1 = c1, w.t1 = t1;
            }
            cuts.push_back(w);
            m = w.m1, c = w.c1, t = w.t1;
        }
    } catch (...) {
        cuts.clear();
        return false;
    }
    return true;
}

} // namespace ybw
