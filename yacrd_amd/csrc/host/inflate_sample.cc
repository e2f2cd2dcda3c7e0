// inflate_sample.cc — the first members of a BGZF stream decoded on the host, for the device parser's record-room estimate
// (gpu_paf.hip: the line density of the text's head, which no longer lies in host memory).  The device decoder's text
// (../inflate_block.h) in its host build, so this unit is compiled by the host compiler and linked into the engine library.
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "../inflate_block.h"

namespace yke {

// Members from the first on, as long as their text stays within max_text bytes: *text bytes decoded, *lines newlines among
// them.  false: nothing to go by (a member the decoder does not take — the device will say so —, or no memory).
bool bgzf_head_lines(const unsigned char *comp, uint64_t comp_bytes, const yif::InfMember *members, uint64_t n_members, uint64_t max_text,
                     uint64_t *text, uint64_t *lines)
{
    *text = *lines = 0;
    std::unique_ptr<yif::InfShared> sh(new (std::nothrow) yif::InfShared());
    std::unique_ptr<unsigned char[]> out(new (std::nothrow) unsigned char[yif::kMaxOut]);
    if (!sh || !out) return false;
    for (uint64_t k = 0; k < n_members; k++) {
        const yif::InfMember &m = members[k];
        if (*text + m.isize > max_text) break;
        if (m.isize > yif::kMaxOut || m.in_off > comp_bytes || comp_bytes - m.in_off < (uint64_t)m.csize + 8u) return false;
        const unsigned char *t = comp + m.in_off + m.csize;
        const uint32_t crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
        if (yif::inf_decode_member(*sh, comp + m.in_off, m.csize, m.isize, crc, out.get()) != yif::kInfOk) return false;
        for (const unsigned char *q = out.get(), *end = q + m.isize; (q = (const unsigned char *)std::memchr(q, '\n', (size_t)(end - q))) != nullptr; q++) ++*lines;
        *text += m.isize;
    }
    return *text != 0;
}

} // namespace yke
