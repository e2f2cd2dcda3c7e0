// gzip_walk.h — the framing of ONE plain gzip member (RFC 1952): where its deflate payload lies and what its trailer says.
// Plain C++, no zlib; shared by the engine library (gpu_gunzip_stream.hip), libyacrd_host (host/inflate_stream_host.cc) and
// tools/inflate_stream_check.cc.  The other framing, BGZF's many small members, is bgzf_walk.h's.
//
//   header   1f 8b 08 FLG, the reserved FLG bits (5-7) zero; MTIME, XFL and OS are skipped; FEXTRA (a u16 length and that
//            many bytes), FNAME and FCOMMENT (to their zero byte) and FHCRC (two bytes, not checked) are skipped where set
//   payload  everything from the header's end to 8 bytes in front of the input's end
//   trailer  CRC-32 and ISIZE (the text's size mod 2^32), little endian, the input's last 8 bytes
// One member only: the walk does not look for a second one.  Whoever decodes the payload asks that its final block ends in
// the payload's last byte, so concatenated members, trailing bytes and a BGZF stream come out of the decoder as "bytes left
// over" (or as whatever else the bytes behind the first member's final block spell), never as a text.
#pragma once
#include <stdint.h>

namespace ygw {

struct GzipFrame {
    uint64_t payload_off = 0, payload_bytes = 0;
    uint32_t crc = 0, isize = 0;
};

// false: not a gzip member this walk takes (a header cut short, reserved bits, an input shorter than header + 8)
inline bool walk(const unsigned char *p, uint64_t n, GzipFrame *f)
{
    if (n < 10 + 8 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8) return false;
    const unsigned flg = p[3];
    if (flg & 0xE0u) return false;
    uint64_t at = 10;
    if (flg & 4u) { // FEXTRA
        if (n - at < 2) return false;
        const uint64_t xlen = (uint64_t)p[at] | ((uint64_t)p[at + 1] << 8);
        at += 2;
        if (n - at < xlen) return false;
        at += xlen;
    }
    for (unsigned bit = 8u; bit <= 16u; bit <<= 1) // FNAME, FCOMMENT: to the zero byte
        if (flg & bit) {
            while (at < n && p[at]) at++;
            if (at >= n) return false;
            at++;
        }
    if (flg & 2u) { // FHCRC
        if (n - at < 2) return false;
        at += 2;
    }
    if (n - at < 8) return false;
    f->payload_off = at, f->payload_bytes = n - 8 - at;
    const unsigned char *t = p + (n - 8);
    f->crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
    f->isize = (uint32_t)t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
    return true;
}

} // namespace ygw
