// inflate_block.h — one BGZF member's deflate payload -> its text (at most 65 536 bytes): a full RFC 1951 decoder (stored,
// fixed and dynamic blocks, any number of them; lengths to 258, distances to 32 768, copies that overlap their source), the
// member's CRC-32 and ISIZE checked against what was produced.  The other half of deflate_block.h, written the same way.
//
// The text is written for a TEAM OF 64 LANES that all walk the bit stream together: what they compute from the stream is
// the same in every lane (YI_UNI says so to the compiler), one lane stores what a single symbol produces (YI_ONE), and
// inside YI_LANES(lane) ... YI_END every lane runs the body with its own number: table fills, stored bytes, match copies
// and the CRC.  hipcc compiles the team as one wavefront (gpu_inflate.hip: one 64-thread workgroup per member, the tables of
// InfShared in LDS, the output where it belongs in HBM; LDS and memory serve one wavefront's accesses to an address in
// program order, the fences of inf_wave_sync keep the compiler to it);
// any other compiler as one thread with a loop over `lane` (libyacrd_host: yacrd_bgzf_decode_host, what the tests without
// a GPU pin to zlib and what a sanitizer build runs).  Nothing may depend on the order in which the lanes of a section
// run: a match's sources all lie in front of the match (period `dist`), the CRC is XORed together.
//
// THE RULES (they hold in both builds):
//   - every read of the payload goes through inf_load4 / the stored copy and is bounded by the payload's end (csize);
//   - every store into out[] is bounded by the member's ISIZE (<= kMaxOut), checked in front of the store, and is one byte;
//   - every distance is bounded by the bytes this member has produced so far (no dictionary);
//   - every loop consumes at least one input bit or produces at least one output byte, and the bits consumed are compared
//     with 8 * csize in every turn (the reader hands out zeros behind the end, never bytes that are not the payload's);
//   - a member that is not taken yields a status (InfStatus), never an access out of range.
// Stricter than zlib, never more lenient: every Huffman code must be complete; the one incomplete code accepted is a
// distance code with a single symbol of length 1, which zlib writes.  A distance code without any symbol is refused.
#pragma once
#include <stdint.h>

#include "deflate_block.h" // YD_FN, the CRC polynomial and CRC(A ++ B), the length / distance bases

#if defined(__HIPCC__)
#define YI_LANES(lane)                                                                                                 \
    {                                                                                                                  \
        yif::inf_wave_sync();                                                                                          \
        const uint32_t lane = threadIdx.x & 63u;
#define YI_END                                                                                                         \
    }                                                                                                                  \
    yif::inf_wave_sync();
#define YI_ONE if ((threadIdx.x & 63u) == 0u)
#define YI_SYNC yif::inf_wave_sync();
#define YI_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define YI_LANES(lane) for (uint32_t lane = 0; lane < 64u; lane++) {
#define YI_END }
#define YI_ONE
#define YI_SYNC
#define YI_UNI(x) ((uint32_t)(x))
#endif

namespace yif {

using ydf::u16;
using ydf::u32;
using ydf::u64;
using ydf::u8;

enum InfStatus : u32 {
    kInfOk = 0,
    kInfEarly,      // the payload ends before the last block does
    kInfLeftOver,   // bytes of the payload left behind the last block
    kInfBlockType,  // BTYPE 3
    kInfStoredLen,  // LEN / NLEN do not match
    kInfOverSub,    // over-subscribed code lengths
    kInfIncomplete, // incomplete code lengths (or no end-of-block code)
    kInfRepeat,     // repeat code 16 with nothing in front, or a repeat beyond the lengths
    kInfCounts,     // HLIT beyond 286 / HDIST beyond 30
    kInfSymbol,     // length symbol 286-287, distance symbol 30-31, or bits no code begins with
    kInfDistance,   // a distance beyond the produced bytes
    kInfOutput,     // output beyond ISIZE or short of it
    kInfCrc,        // CRC-32 mismatch
    kInfTable,      // the member table does not fit its buffers (gpu_inflate.hip)
    kInfStatuses
};
inline const char *inf_status_name(u32 s) // (host code: the messages)
{
    const char *const names[kInfStatuses] = {"ok", "payload ends early", "payload has bytes left over", "block type 3", "LEN / NLEN mismatch",
                                             "over-subscribed code lengths", "incomplete code lengths", "bad repeat of a code length",
                                             "HLIT / HDIST beyond 286 / 30", "invalid symbol", "distance beyond the produced bytes",
                                             "output beyond ISIZE or short of it", "CRC mismatch", "member table out of range"};
    return s < kInfStatuses ? names[s] : "?";
}

// one member of a BGZF stream, as the walk (bgzf_walk.h) finds it
struct InfMember {
    u64 in_off;  // where its deflate payload begins in the stream
    u64 out_off; // where its text begins in the inflated text
    u32 csize;   // bytes of payload; the trailer (CRC-32, ISIZE) lies behind them
    u32 isize;   // the trailer's ISIZE, <= kMaxOut
};

constexpr u32 kMaxOut = 65536;
constexpr u32 kLitFast = 10, kDistFast = 8, kClFast = 7; // bits the one-look tables resolve
constexpr u32 kLitSyms = 288, kDistSyms = 32, kClSyms = 19;
constexpr u32 kNoSym = 0xFFFFu;
constexpr u32 kCrcSpan = 1024; // bytes a lane sums
static_assert(64u * kCrcSpan >= kMaxOut, "the lanes' spans cover a member");
static_assert((1u << kDistFast) >= (1u << kClFast), "the code-length code borrows the distance table");

struct InfShared {
    u16 lfast[1u << kLitFast]; // symbol << 4 | code length, by the next bits; 0: a longer code (or none)
    u16 dfast[1u << kDistFast]; // (the code-length code's while a dynamic header is read)
    u16 lsym[kLitSyms], dsym[kDistSyms]; // symbols by (length, symbol): the longer codes' walk
    u16 lcount[16], dcount[16];          // symbols per code length
    u16 next[16], offs[16];              // the build's: next code / next place in *sym per length
    u8 lens[kLitSyms + kDistSyms];
    u32 crc_tab[256];
    u32 crc;
};

YD_FN void inf_wave_sync()
{
#if defined(__HIPCC__)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#endif
}

// bytes [off, off + 4) of the payload p[0, n), little endian; zeros where the payload has ended
YD_FN u32 inf_load4(const u8 *p, u32 n, u32 off)
{
    u32 v = 0;
    if (off < n && n - off >= 4u) __builtin_memcpy(&v, p + off, 4);
    else
        for (u32 k = 0; k < 4u; k++)
            if (off < n && k < n - off) v |= (u32)p[off + k] << (8u * k);
    return v;
}

// ---- the bit reader: least significant bit first ----------------------------------------------------------------------
struct InfBits {
    const u8 *p;
    u32 n;    // the payload
    u64 acc;  // the next `cnt` bits
    u32 cnt;
    u32 next; // the payload byte the next fetch begins with; bits consumed = 8 * next - cnt
#if defined(__HIPCC__)
    u32 win, ahead, chunk; // lane i holds payload bytes [256 chunk + 4 i, + 4) in `win`, the chunk behind it in `ahead`
#endif
};
YD_FN void inf_bits_init(InfBits &b, const u8 *p, u32 n)
{
    b.p = p, b.n = n, b.acc = 0, b.cnt = 0, b.next = 0;
#if defined(__HIPCC__)
    b.win = b.ahead = 0, b.chunk = 0xFFFFFFF0u;
#endif
}
// the payload's dword at byte `off` (a multiple of 4)
YD_FN u32 inf_word(InfBits &b, u32 off)
{
#if defined(__HIPCC__)
    // a chunk of 256 bytes lies in the wavefront's registers, the next one is on its way: the walk waits for memory once
    // per chunk at the most
    const u32 c = off >> 8;
    if (c != b.chunk) {
        const u32 lane = threadIdx.x & 63u;
        b.win = c == b.chunk + 1u ? b.ahead : inf_load4(b.p, b.n, c * 256u + 4u * lane);
        b.ahead = inf_load4(b.p, b.n, (c + 1u) * 256u + 4u * lane);
        b.chunk = c;
    }
    return (u32)__builtin_amdgcn_readlane((int)b.win, (int)YI_UNI((off >> 2) & 63u));
#else
    return inf_load4(b.p, b.n, off);
#endif
}
// at least 33 bits in acc (zeros behind the payload's end: inf_over tells)
YD_FN void inf_refill(InfBits &b)
{
    while (b.cnt <= 32u) {
        const u32 skip = b.next & 3u;
        const u32 w = inf_word(b, b.next - skip) >> (8u * skip);
        b.acc |= (u64)w << b.cnt;
        b.cnt += 32u - 8u * skip;
        b.next = YI_UNI(b.next + 4u - skip);
    }
}
YD_FN void inf_drop(InfBits &b, u32 k) { b.acc >>= k, b.cnt -= k; } // k <= cnt
YD_FN u32 inf_take(InfBits &b, u32 k)                               // k <= 16, k <= cnt
{
    const u32 v = YI_UNI((u32)b.acc & ((1u << k) - 1u));
    inf_drop(b, k);
    return v;
}
YD_FN u32 inf_used_bits(const InfBits &b) { return 8u * b.next - b.cnt; }
YD_FN bool inf_over(const InfBits &b) { return inf_used_bits(b) > 8u * b.n; } // bits were taken that the payload does not have

// ---- a code: lens[0, n) -> the one-look table of `fb` bits, the counts per length, the symbols by (length, symbol) ---------
// kInfOk, kInfOverSub or kInfIncomplete (`dist`: a single code of length 1 passes).
YD_FN u32 inf_build(InfShared &sh, const u8 *lens, u32 n, u32 fb, u16 *fast, u16 *count, u16 *sym, bool dist)
{
    YI_LANES(lane)
    for (u32 i = lane; i < (1u << fb); i += 64u) fast[i] = 0;
    if (lane < 16u) count[lane] = 0;
    YI_END
    YI_ONE
    {
        for (u32 s = 0; s < n; s++) count[lens[s]]++;
    }
    YI_SYNC
    u32 used = 0;
    int left = 1;
    for (u32 l = 1; l <= 15u; l++) {
        const u32 c = YI_UNI(count[l]);
        used += c;
        left = 2 * left - (int)c;
        if (left < 0) return kInfOverSub;
    }
    if (left > 0 && !(dist && used == 1u && YI_UNI(count[1]) == 1u)) return kInfIncomplete;
    YI_ONE
    {
        u32 code = 0, off = 0;
        for (u32 l = 1; l <= 15u; l++) {
            sh.next[l] = (u16)code, sh.offs[l] = (u16)off; // (code < 2^l: the lengths are not over-subscribed)
            code = (code + count[l]) << 1, off += count[l];
        }
    }
    YI_SYNC
    for (u32 s = 0; s < n; s++) {
        const u32 l = YI_UNI(lens[s]);
        if (l == 0) continue;
        const u32 c = YI_UNI(sh.next[l]), o = YI_UNI(sh.offs[l]);
        YI_ONE
        {
            sh.next[l] = (u16)(c + 1u), sh.offs[l] = (u16)(o + 1u);
            sym[o] = (u16)s; // (o < used <= n)
        }
        YI_SYNC
        if (l <= fb) {
            u32 r = 0; // the code as it arrives: first bit lowest
            for (u32 i = 0; i < l; i++) r |= ((c >> i) & 1u) << (l - 1u - i);
            YI_LANES(lane)
            for (u32 i = r + (lane << l); i < (1u << fb); i += 64u << l) fast[i] = (u16)((s << 4) | l);
            YI_END
        }
    }
    return kInfOk;
}

// the symbol the next bits spell, taken off the reader; kNoSym: no code begins with them.  Wants 15 bits in acc.
YD_FN u32 inf_symbol(InfBits &b, const u16 *fast, u32 fb, const u16 *count, const u16 *sym)
{
    const u32 e = YI_UNI(fast[(u32)b.acc & ((1u << fb) - 1u)]);
    if (e) {
        inf_drop(b, e & 15u);
        return e >> 4;
    }
    // the canonical walk, a bit at a time: codes of a length are consecutive, `first` is the first of them
    u32 code = 0, first = 0, index = 0;
    u64 a = b.acc;
    for (u32 l = 1; l <= 15u; l++) {
        code |= (u32)a & 1u;
        a >>= 1;
        const u32 c = YI_UNI(count[l]);
        if (code < first + c) { // (code >= first: whatever is below went out at a shorter length)
            inf_drop(b, l);
            return YI_UNI(sym[index + (code - first)]);
        }
        index += c, first = (first + c) << 1, code <<= 1;
    }
    return kNoSym;
}

// ---- one member: p[0, csize) -> out[0, isize); the status.  Every lane of the team calls it (hipcc) / one caller
// (elsewhere); every lane returns the same status.  `out` is the member's place in the text itself (hipcc: global memory):
// every store is a single byte, so members that begin and end inside a dword never write each other's bytes, and a match
// reads back what this wavefront has stored (one wavefront's accesses to an address are served in order; inf_wave_sync
// keeps the compiler to it).  After a status other than kInfOk out[0, isize) holds whatever was decoded until then.
YD_FN u32 inf_decode_member(InfShared &sh, const u8 *p, u32 csize, u32 isize, u32 crc_want, u8 *out)
{
    if (isize > kMaxOut) return kInfOutput;
    YI_LANES(lane)
    for (u32 t = lane; t < 256u; t += 64u) {
        u32 c = t;
        for (int k = 0; k < 8; k++) c = c & 1u ? (c >> 1) ^ ydf::kCrcPoly : c >> 1;
        sh.crc_tab[t] = c;
    }
    if (lane == 0) sh.crc = 0;
    YI_END
    InfBits b;
    inf_bits_init(b, p, csize);
    u32 pos = 0, last = 0;
    do { // a block: at least 3 bits
        inf_refill(b);
        last = inf_take(b, 1);
        const u32 type = inf_take(b, 2);
        if (inf_over(b)) return kInfEarly;
        if (type == 3u) return kInfBlockType;
        if (type == 0u) {
            inf_drop(b, b.cnt & 7u); // to the byte's end (8 * next is whole bytes)
            inf_refill(b);
            const u32 len = inf_take(b, 16), nlen = inf_take(b, 16);
            if (inf_over(b)) return kInfEarly;
            if ((len ^ nlen) != 0xFFFFu) return kInfStoredLen;
            const u32 at = inf_used_bits(b) >> 3; // (<= csize)
            if (len > csize - at) return kInfEarly;
            if (len > isize - pos) return kInfOutput;
            YI_LANES(lane)
            for (u32 i = lane; i < len; i += 64u) out[pos + i] = p[at + i];
            YI_END
            pos += len;
            b.acc = 0, b.cnt = 0, b.next = at + len;
            continue;
        }
        u32 hlit = kLitSyms, hdist = kDistSyms;
        if (type == 1u) {
            YI_LANES(lane)
            for (u32 s = lane; s < kLitSyms + kDistSyms; s += 64u) sh.lens[s] = (u8)(s < 144u ? 8 : s < 256u ? 9 : s < 280u ? 7 : s < 288u ? 8 : 5);
            YI_END
        } else {
            hlit = inf_take(b, 5) + 257u, hdist = inf_take(b, 5) + 1u;
            const u32 hclen = inf_take(b, 4) + 4u;
            if (inf_over(b)) return kInfEarly;
            if (hlit > 286u || hdist > 30u) return kInfCounts;
            YI_LANES(lane)
            if (lane < kClSyms) sh.lens[lane] = 0;
            YI_END
            for (u32 i = 0; i < hclen; i++) {
                inf_refill(b);
                const u32 v = inf_take(b, 3);
                YI_ONE sh.lens[ydf::df_cl_order(i)] = (u8)v;
            }
            YI_SYNC
            if (inf_over(b)) return kInfEarly;
            if (const u32 st = inf_build(sh, sh.lens, kClSyms, kClFast, sh.dfast, sh.dcount, sh.dsym, false)) return st;
            const u32 total = hlit + hdist;
            u32 prev = 0;
            for (u32 i = 0; i < total;) { // a code length symbol: at least 1 bit, at least one length
                inf_refill(b);
                const u32 s = inf_symbol(b, sh.dfast, kClFast, sh.dcount, sh.dsym);
                if (s >= kClSyms) return kInfSymbol;
                u32 rep = 1, val = s;
                if (s == 16u) {
                    if (i == 0) return kInfRepeat;
                    rep = 3u + inf_take(b, 2), val = prev;
                } else if (s == 17u) rep = 3u + inf_take(b, 3), val = 0;
                else if (s == 18u) rep = 11u + inf_take(b, 7), val = 0;
                if (inf_over(b)) return kInfEarly;
                if (rep > total - i) return kInfRepeat;
                YI_ONE
                {
                    for (u32 k = 0; k < rep; k++) sh.lens[i + k] = (u8)val; // (i + rep <= total <= 316)
                }
                i += rep, prev = val;
            }
            YI_SYNC
            if (YI_UNI(sh.lens[256]) == 0) return kInfIncomplete; // no end-of-block code
        }
        if (const u32 st = inf_build(sh, sh.lens, hlit, kLitFast, sh.lfast, sh.lcount, sh.lsym, false)) return st;
        if (const u32 st = inf_build(sh, sh.lens + hlit, hdist, kDistFast, sh.dfast, sh.dcount, sh.dsym, true)) return st;
        for (;;) { // a symbol: at least 1 bit
            inf_refill(b);
            u32 s = inf_symbol(b, sh.lfast, kLitFast, sh.lcount, sh.lsym);
            if (s == kNoSym) return kInfSymbol;
            if (inf_over(b)) return kInfEarly;
            if (s < 256u) {
                if (pos >= isize) return kInfOutput;
                YI_ONE out[pos] = (u8)s;
                pos++;
                continue;
            }
            if (s == 256u) break;
            s -= 257u;
            if (s >= 29u) return kInfSymbol;
            const u32 len = ydf::df_len_base(s) + inf_take(b, ydf::df_len_extra(s)); // (5 extra bits at the most)
            inf_refill(b);
            const u32 ds = inf_symbol(b, sh.dfast, kDistFast, sh.dcount, sh.dsym);
            if (ds >= 30u) return kInfSymbol; // (kNoSym too)
            const u32 dist = ydf::df_dist_base(ds) + inf_take(b, ydf::df_dist_extra(ds)); // (13 extra bits at the most)
            if (inf_over(b)) return kInfEarly;
            if (dist > pos) return kInfDistance;
            if (len > isize - pos) return kInfOutput;
            const u32 from = pos - dist;
            // byte i of the match is byte i mod dist of the `dist` bytes in front of it: every source lies below pos
            YI_LANES(lane)
            for (u32 i = lane; i < len; i += 64u) out[pos + i] = out[from + (dist < len ? i % dist : i)];
            YI_END
            pos += len;
        }
    } while (!last);
    const u32 used = (inf_used_bits(b) + 7u) >> 3;
    if (used != csize) return used < csize ? kInfLeftOver : kInfEarly;
    if (pos != isize) return kInfOutput;
    YI_LANES(lane)
    {
        const u32 lo = lane * kCrcSpan < isize ? lane * kCrcSpan : isize, hi = (lane + 1u) * kCrcSpan < isize ? (lane + 1u) * kCrcSpan : isize;
        if (hi > lo) {
            u32 c = 0xFFFFFFFFu;
            for (u32 i = lo; i < hi; i++) c = sh.crc_tab[(c ^ out[i]) & 255u] ^ (c >> 8);
            c ^= 0xFFFFFFFFu;
            const u32 part = ydf::df_mulmod(ydf::df_xpow8(isize - hi), c);
#if defined(__HIPCC__)
            atomicXor(&sh.crc, part);
#else
            sh.crc ^= part;
#endif
        }
    }
    YI_END
    if (YI_UNI(sh.crc) != crc_want) return kInfCrc;
    return kInfOk;
}

} // namespace yif
