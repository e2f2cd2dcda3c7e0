// inflate_sample.cc — the first members of a BGZF stream decoded on the host, for the device parser's record-room estimate
// (gpu_paf.hip: the line density of the text's head, which no longer lies in host memory) and for what the device overlap
// editor's plan asks of a text (gpu_edit.hip: the first line's field count, the last byte).  The device decoder's text
// (../inflate_block.h) in its host build, so this unit is compiled by the host compiler and linked into the engine library;
// libyacrd_host takes it too (yacrd_bgzf_text_ends: the tests without a GPU) and tools/bgzf_text_ends_check.cc includes it.
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "../inflate_block.h"

// Two libraries hold a copy of this unit each, and one process may load both: the two functions stay inside the library that
// was linked with them (hidden), so a caller never gets the other library's copy should the two ever differ.
#define YK_LOCAL __attribute__((visibility("hidden")))

namespace yke {

// Members from the first on, as long as their text stays within max_text bytes: *text bytes decoded, *lines newlines among
// them.  false: nothing to go by (a member the decoder does not take — the device will say so —, or no memory).
YK_LOCAL bool bgzf_head_lines(const unsigned char *comp, uint64_t comp_bytes, const yif::InfMember *members, uint64_t n_members, uint64_t max_text,
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

// What the overlap editor's plan (gpu_edit.hip) asks of a text before its first launch, for a text that is not in host memory:
// *n_fields, the field count under `delim` of the first non-empty line (0: there is none), and *ends_nl, whether the text's
// last byte is a newline (true for a text of no bytes) — first_line_fields' answers on the inflated text.  Decoded for that:
// members from the first on until that line is complete, as long as their text stays within max_text bytes, and the last
// member that holds text, for its last byte.  Returns 0; 1: a member the decoder does not take (*status says which cause: the
// device would refuse it too); 2: the first non-empty line is not complete inside the sample and the text goes on; 3: no memory.
YK_LOCAL int bgzf_text_ends(const unsigned char *comp, uint64_t comp_bytes, const yif::InfMember *members, uint64_t n_members, uint64_t max_text,
                   unsigned char delim, uint32_t *n_fields, bool *ends_nl, uint32_t *status)
{
    *n_fields = 0, *ends_nl = true, *status = yif::kInfOk;
    std::unique_ptr<yif::InfShared> sh(new (std::nothrow) yif::InfShared());
    std::unique_ptr<unsigned char[]> out(new (std::nothrow) unsigned char[yif::kMaxOut]);
    if (!sh || !out) return 3;
    auto decode = [&](const yif::InfMember &m) -> uint32_t {
        if (m.isize > yif::kMaxOut || m.in_off > comp_bytes || comp_bytes - m.in_off < (uint64_t)m.csize + 8u) return yif::kInfTable;
        const unsigned char *t = comp + m.in_off + m.csize;
        const uint32_t crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
        return yif::inf_decode_member(*sh, comp + m.in_off, m.csize, m.isize, crc, out.get());
    };
    uint64_t last = n_members; // the last member that holds text
    for (uint64_t k = n_members; k-- > 0;)
        if (members[k].isize) {
            last = k;
            break;
        }
    if (last == n_members) return 0; // a text of no bytes
    bool in_line = false, complete = false;
    uint32_t nf = 0;
    uint64_t text = 0, k = 0;
    for (; k <= last && !complete; k++) {
        const yif::InfMember &m = members[k];
        if (text + m.isize > max_text) break;
        if ((*status = decode(m)) != yif::kInfOk) return 1;
        for (uint32_t i = 0; i < m.isize && !complete; i++) {
            const unsigned char c = out[i];
            if (c == '\n') {
                complete = in_line;
                continue;
            }
            if (!in_line) in_line = true, nf = 1;
            if (c == delim) nf++;
        }
        text += m.isize;
    }
    if (!complete && k <= last) return 2; // the text goes on behind the sample
    if (in_line) *n_fields = nf;
    if ((*status = decode(members[last])) != yif::kInfOk) return 1;
    *ends_nl = out[members[last].isize - 1] == '\n';
    return 0;
}

// bgzf_text_ends' second answer alone, for a caller that asks nothing of the first line (gpu_seq_edit.hip: a BGZF FASTQ /
// FASTA in windows, before its first launch): *ends_nl, whether the text's last byte is a newline (true for a text of no
// bytes), from the last member that holds text.  Returns 0; 1: the decoder does not take that member (*status says which
// cause); 3: no memory.
YK_LOCAL int bgzf_last_byte(const unsigned char *comp, uint64_t comp_bytes, const yif::InfMember *members, uint64_t n_members, bool *ends_nl,
                            uint32_t *status)
{
    *ends_nl = true, *status = yif::kInfOk;
    uint64_t last = n_members;
    while (last > 0 && !members[last - 1].isize) last--;
    if (!last) return 0; // a text of no bytes
    const yif::InfMember &m = members[last - 1];
    if (m.isize > yif::kMaxOut || m.in_off > comp_bytes || comp_bytes - m.in_off < (uint64_t)m.csize + 8u) {
        *status = yif::kInfTable;
        return 1;
    }
    std::unique_ptr<yif::InfShared> sh(new (std::nothrow) yif::InfShared());
    std::unique_ptr<unsigned char[]> out(new (std::nothrow) unsigned char[yif::kMaxOut]);
    if (!sh || !out) return 3;
    const unsigned char *t = comp + m.in_off + m.csize;
    const uint32_t crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
    if ((*status = yif::inf_decode_member(*sh, comp + m.in_off, m.csize, m.isize, crc, out.get())) != yif::kInfOk) return 1;
    *ends_nl = out[m.isize - 1] == '\n';
    return 0;
}

} // namespace yke
