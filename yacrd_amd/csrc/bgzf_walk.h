// bgzf_walk.h — the member walk of a BGZF stream (SAM spec 4.1): plain C++, no zlib.  Shared by the engine library
// (gpu_inflate.hip: the member table the kernel works from) and libyacrd_host (host/inflate_host.cc).
//
// A member is taken when it begins `1f 8b 08 04` (deflate, FEXTRA and no other flag: FNAME, FCOMMENT, FHCRC or plain gzip
// make the stream somebody else's), its extra field is a run of well-formed subfields among which exactly one is `BC` with
// two bytes (anywhere: XLEN may exceed 6), BSIZE + 1 covers the header and the trailer and lies inside the input, and the
// trailer's ISIZE is at most 65 536.  The members must tile the input: bytes behind the last one make it not BGZF.  EOF
// members (ISIZE 0) may appear anywhere.  An exclusive sum of the ISIZEs gives every member's place in the text.
#pragma once
#include <stdint.h>

#include <vector>

#include "inflate_block.h" // yif::InfMember, kMaxOut

namespace ybw {

// false: not BGZF (or no memory for the table).  An empty input is an empty table.
inline bool walk(const unsigned char *d, uint64_t n, std::vector<yif::InfMember> &members, uint64_t *text_bytes)
{
    members.clear();
    uint64_t at = 0, total = 0;
    try {
        while (at < n) {
            const uint64_t room = n - at;
            if (room < 12u) return false;
            const unsigned char *h = d + at;
            if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || h[3] != 4) return false;
            const uint64_t xlen = (uint64_t)h[10] | ((uint64_t)h[11] << 8), end = 12u + xlen;
            if (end > room) return false;
            int64_t bsize = -1;
            uint64_t q = 12;
            while (q + 4u <= end) {
                const uint64_t slen = (uint64_t)h[q + 2] | ((uint64_t)h[q + 3] << 8);
                if (slen > end - (q + 4u)) return false;
                if (h[q] == 'B' && h[q + 1] == 'C') {
                    if (slen != 2u || bsize >= 0) return false;
                    bsize = (int64_t)h[q + 4] | ((int64_t)h[q + 5] << 8);
                }
                q += 4u + slen;
            }
            if (q != end || bsize < 0) return false;
            const uint64_t size = (uint64_t)bsize + 1u;
            if (size < end + 8u || size > room) return false;
            const uint64_t isize = (uint64_t)h[size - 4] | ((uint64_t)h[size - 3] << 8) | ((uint64_t)h[size - 2] << 16) | ((uint64_t)h[size - 1] << 24);
            if (isize > yif::kMaxOut) return false;
            yif::InfMember m;
            m.in_off = at + end, m.out_off = total, m.csize = (uint32_t)(size - end - 8u), m.isize = (uint32_t)isize;
            members.push_back(m);
            total += isize, at += size;
        }
    } catch (...) {
        return false;
    }
    *text_bytes = total;
    return true;
}

} // namespace ybw
