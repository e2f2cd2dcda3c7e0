// inflate_stream.h — ONE long deflate stream (a plain gzip member's payload, gzip_walk.h) -> its text, decoded in parallel
// from guessed block starts.  The companion of inflate_block.h, whose bit reader, code tables, status codes and RULES it
// keeps: every read of the payload is bounded by the payload's end, every store by the size the step before has proven,
// every loop eats a bit or makes a byte, and what is not taken yields a status, never an access out of range.  One text for
// both builds: hipcc compiles the per-span walks as one wavefront (gpu_gunzip_stream.hip), any other compiler as one
// thread (libyacrd_host: yacrd_gzip_stream_decode_host; tools/inflate_stream_check.cc under the sanitizers).
//
// The payload is cut into CHUNKS of C compressed bytes.  Five steps, each its own launch or launches; nobody waits for
// anybody inside a launch (no spin, no look-back, no ticket): order comes from launch boundaries and, for the repair, from
// the host.
//
//   FIND     per chunk k >= 1, the first bit position in it at which a DYNAMIC, NON-FINAL block header is acceptable
//            (str_header_ok: the acceptance rule, in registers, one candidate per lane).  Stored, fixed and final blocks are
//            not looked for: a chunk without a find belongs to the span in front of it.  False accepts are allowed.
//   SIZE     a SPAN begins at bit 0 or at a find.  Its walk (str_walk_span<false>) decodes symbols and stores nothing: it
//            counts bytes and blocks and stops at the first block end at or beyond the next find (its stop bit), or behind
//            the final block.  The host then walks the CHAIN from span 0 (str_chain): a span is TRUE when the true span in
//            front of it ended exactly on its start; finds the chain stepped over are dropped, whatever their own walk said;
//            where a true span ends on no find, that end is a PROVEN block start and becomes a span of its own, sized in
//            the next round (at most kMaxRounds of them).  A status in a true span is the stream's.  Behind this step the
//            text's size, every true span's place in it and the chain are known, before a byte is stored.  A wrong guess
//            costs a round, never a byte: only what follows from bit 0 block by block is ever used.
//   SYMBOLS  every true span is walked again (str_walk_span<true>) into one u16 per text byte at its place: a literal is its
//            value; a byte whose source lies in front of the span's first byte is the MARKER 256 + j, "text byte
//            span_start - 1 - j" (j <= 32 767: distances end at 32 768).  Matches copy u16s, markers included.  The walk
//            must end where SIZE said and make the bytes SIZE counted, or it is a status.
//   WINDOWS  spans in order, one team: each span's last min(32 768, length) symbols are resolved through the 32 768
//            in front of the span, which are literals by then (induction over the spans; a span shorter than 32 768 is
//            resolved whole and so carries the window through).  The one serial chain of the design.
//   BYTES    position-parallel: a literal goes out as its byte, a marker takes the resolved symbol it names (its span by
//            binary search).  Each thread sums the CRC-32 of its 16 bytes; parts are joined by CRC(A ++ B) =
//            CRC(A) x^(8|B|) + CRC(B) (deflate_block.h: df_mulmod; str_xpow8: the power for 64-bit lengths).
//
// BOUNDS.  The payload: at most kMaxPayload bytes.  A span reads at most kSpanMaxComp bytes of payload and makes at most
// kSpanMaxOut bytes: a span beyond either is kStrSpanLong, never wrapped.  The bounds are bounds on WORK, far inside what
// the bit reader's 32-bit counts would hold: a span is one wavefront's walk at a few MB of text a second, twice over, so
// 64 MiB of text is already tens of seconds of one launch, and what is longer is the host reader's.  A stream of stored or
// fixed blocks alone is one span: one walk's work, slow and correct up to these bounds.
#pragma once
#include <stdint.h>

#include "inflate_block.h"

#if defined(__HIPCC__)
#define YS_EACH(x, lo, hi) for (uint64_t x = (lo) + threadIdx.x; x < (hi); x += blockDim.x)
#define YS_BARRIER __syncthreads();
#else
#define YS_EACH(x, lo, hi) for (uint64_t x = (lo); x < (hi); x++)
#define YS_BARRIER
#endif

namespace yis {

using yif::u16;
using yif::u32;
using yif::u64;
using yif::u8;

constexpr u32 kMinChunk = 1024, kDefaultChunk = 32768;
constexpr u64 kMaxPayload = (u64)1 << 40;
constexpr u32 kSpanMaxComp = 1u << 25, kSpanMaxOut = 1u << 26; // 32 MiB of payload, 64 MiB of text
constexpr u32 kMaxRounds = 64; // repair rounds: beyond them "too many wrong block starts"
constexpr u32 kWindow = 32768;
constexpr u64 kNoBit = ~(u64)0;
constexpr u32 kTileThreads = 256, kThreadBytes = 16, kTile = kTileThreads * kThreadBytes; // the BYTES step

enum : u32 { // statuses of the stream, beside yif::InfStatus
    kStrSpanLong = 32, // a span beyond kSpanMaxComp / kSpanMaxOut
    kStrRounds,        // too many wrong block starts
    kStrPayload,       // a payload beyond kMaxPayload
    kStrChain,         // SYMBOLS did not end where SIZE did / a marker names no literal: never, by the chain rule
};
inline const char *str_status_name(u32 s)
{
    return s == kStrSpanLong ? "a span beyond the decoder's bounds" : s == kStrRounds ? "too many wrong block starts" :
           s == kStrPayload ? "a payload beyond the decoder's bounds" : s == kStrChain ? "the steps disagree" : yif::inf_status_name(s);
}

struct Span {
    u64 start_bit, stop_bit; // where its walk begins; it stops at the first block end at or beyond stop_bit
    u64 end_bit;             // SIZE: where it stopped
    u64 out_off;             // the chain: its place in the text
    u32 out_bytes, n_blocks, status, saw_final; // SIZE
};

// ---- FIND ------------------------------------------------------------------------------------------------------------
// the next 57 bits and more at `bit` of p[0, n), zeros behind the end
YD_FN u64 str_peek(const u8 *p, u64 n, u64 bit)
{
    const u64 off = bit >> 3;
    u64 v = 0;
    if (off < n && n - off >= 8u) __builtin_memcpy(&v, p + off, 8);
    else
        for (u32 k = 0; k < 8u; k++)
            if (off < n && k < n - off) v |= (u64)p[off + k] << (8u * k);
    return v >> (bit & 7u);
}

// THE ACCEPTANCE RULE: a dynamic, non-final block header begins at `bit` exactly when inf_decode_member's header code
// would pass it: BFINAL 0, BTYPE 2, HLIT <= 286, HDIST <= 30; the code-length code complete (Kraft sum 1); the HLIT + HDIST
// lengths decode with no repeat in front of the first length and none beyond the last, inside the payload; the
// literal / length code complete with symbol 256 present; the distance code complete, or one symbol of length 1.  (Over-
// subscribed and incomplete are both "Kraft sum not 1": inf_build's `left` is the sum's complement.)  Nothing of the
// block's symbols is read.  One lane's work, in registers: the code-length code lives in two u64s and is decoded by the
// canonical walk.
YD_FN bool str_header_ok(const u8 *p, u64 n, u64 bit)
{
    const u64 end = 8u * n;
    if (bit >= end || end - bit < 17u) return false;
    u64 v = str_peek(p, n, bit);
    if ((v & 7u) != 4u) return false;
    const u32 hlit = (u32)((v >> 3) & 31u) + 257u, hdist = (u32)((v >> 8) & 31u) + 1u, hclen = (u32)((v >> 13) & 15u) + 4u;
    if (hlit > 286u || hdist > 30u) return false;
    bit += 17u;
    if (end - bit < 3u * hclen) return false;
    v = str_peek(p, n, bit); // (57 bits: 19 lengths)
    u64 cl = 0, cnts = 0;    // length of symbol s at bits [3 s, 3 s + 3); symbols of length l at bits [8 l, 8 l + 8)
    u32 kraft = 0;           // in 1 / 128
    for (u32 i = 0; i < hclen; i++) {
        const u32 l = (u32)(v >> (3u * i)) & 7u;
        cl |= (u64)l << (3u * ydf::df_cl_order(i));
        if (l) kraft += 128u >> l, cnts += (u64)1 << (8u * l);
    }
    if (kraft != 128u) return false;
    bit += 3u * hclen;
    const u32 total = hlit + hdist;
    u32 lit_k = 0, dist_k = 0, n_dist = 0, dist_one = 0, has_eob = 0, prev = 0; // Kraft sums in 1 / 32 768
    for (u32 i = 0; i < total;) {                                               // a code length symbol: at least 1 bit
        if (bit >= end) return false;
        v = str_peek(p, n, bit);
        u32 code = 0, first = 0, l = 1, rank = 0;
        for (; l <= 7u; l++) {
            code |= (u32)(v >> (l - 1u)) & 1u;
            const u32 c = (u32)(cnts >> (8u * l)) & 255u;
            if (code < first + c) {
                rank = code - first;
                break;
            }
            first = (first + c) << 1, code <<= 1;
        }
        if (l > 7u) return false; // (a complete code: never)
        u32 s = 0;
        for (;; s++) { // the rank-th symbol of length l (there is one: c > rank)
            if (s >= yif::kClSyms) return false;
            if (((u32)(cl >> (3u * s)) & 7u) == l) {
                if (rank == 0) break;
                rank--;
            }
        }
        v >>= l, bit += l;
        u32 rep = 1, val = s;
        if (s == 16u) {
            if (i == 0) return false;
            rep = 3u + ((u32)v & 3u), val = prev, bit += 2u;
        } else if (s == 17u) rep = 3u + ((u32)v & 7u), val = 0, bit += 3u;
        else if (s == 18u) rep = 11u + ((u32)v & 127u), val = 0, bit += 7u;
        if (bit > end || rep > total - i) return false;
        if (val)
            for (u32 k = i; k < i + rep; k++) {
                if (k < hlit) lit_k += 32768u >> val, has_eob |= k == 256u;
                else dist_k += 32768u >> val, n_dist++, dist_one += val == 1u;
            }
        i += rep, prev = val;
    }
    if (lit_k != 32768u || !has_eob) return false;
    return dist_k == 32768u || (n_dist == 1u && dist_one == 1u);
}

// the first acceptable bit in [lo, hi) (hi <= 8 n), or kNoBit: 64 candidates a step, the lowest lane that accepts.
// Every lane of the wavefront calls it (hipcc) and gets the same answer.
YD_FN u64 str_find(const u8 *p, u64 n, u64 lo, u64 hi)
{
    for (u64 b0 = lo; b0 < hi; b0 += 64u) {
#if defined(__HIPCC__)
        const u64 cand = b0 + (threadIdx.x & 63u);
        const u64 mask = __ballot(cand < hi && str_header_ok(p, n, cand));
        if (mask) return b0 + (u64)__builtin_ctzll(mask);
#else
        for (u64 cand = b0; cand < hi && cand < b0 + 64u; cand++)
            if (str_header_ok(p, n, cand)) return cand;
#endif
    }
    return kNoBit;
}

// ---- SIZE and SYMBOLS: one span's walk ---------------------------------------------------------------------------------
// Walks the blocks from sp.start_bit to the first block end at or beyond sp.stop_bit or behind the final block.  kStore
// false (SIZE): nothing is stored; end_bit, out_bytes, n_blocks, saw_final and the status are left in `sp`.  Distances are
// checked against the absolute bytes produced where those are known (the span at bit 0); elsewhere SYMBOLS checks them.
// kStore true (SYMBOLS): sym[0, sp.out_bytes) is the span's place in the scratch, sp.out_off its first byte's place in the
// text; returns the status, kStrChain where the walk does not end as SIZE said.  Every lane of the team calls it; every
// lane returns the same.
template <bool kStore>
YD_FN u32 str_walk_span(yif::InfShared &sh, const u8 *pay, u64 pay_bytes, Span &sp, u16 *sym)
{
    using namespace yif;
    const u64 base = sp.start_bit >> 3;
    if (base > pay_bytes) return kInfEarly;
    const u8 *p = pay + base;
    const bool clamped = pay_bytes - base > kSpanMaxComp;
    const u32 csize = clamped ? kSpanMaxComp : (u32)(pay_bytes - base);
    const u32 early = clamped ? (u32)kStrSpanLong : (u32)kInfEarly; // the slice ends: the payload's end, or the bound
    const u32 cap = kStore ? sp.out_bytes : kSpanMaxOut, full = kStore ? (u32)kInfOutput : (u32)kStrSpanLong;
    // bytes in front of the span's first one that a distance may reach
    const u64 front = kStore ? sp.out_off : sp.start_bit == 0 ? 0 : (u64)kWindow;
    InfBits b;
    inf_bits_init(b, p, csize);
    inf_refill(b);
    inf_drop(b, (u32)(sp.start_bit & 7u));
    u32 pos = 0, last = 0, blocks = 0;
    for (;;) { // a block: at least 3 bits
        inf_refill(b);
        last = inf_take(b, 1);
        const u32 type = inf_take(b, 2);
        if (inf_over(b)) return early;
        if (type == 3u) return kInfBlockType;
        if (type == 0u) {
            inf_drop(b, b.cnt & 7u);
            inf_refill(b);
            const u32 len = inf_take(b, 16), nlen = inf_take(b, 16);
            if (inf_over(b)) return early;
            if ((len ^ nlen) != 0xFFFFu) return kInfStoredLen;
            const u32 at = inf_used_bits(b) >> 3; // (<= csize)
            if (len > csize - at) return early;
            if (len > cap - pos) return full;
            if (kStore) {
                YI_LANES(lane)
                for (u32 i = lane; i < len; i += 64u) sym[pos + i] = p[at + i];
                YI_END
            }
            pos += len;
            b.acc = 0, b.cnt = 0, b.next = at + len;
        } else {
            u32 hlit = kLitSyms, hdist = kDistSyms;
            if (type == 1u) {
                YI_LANES(lane)
                for (u32 s = lane; s < kLitSyms + kDistSyms; s += 64u) sh.lens[s] = (u8)(s < 144u ? 8 : s < 256u ? 9 : s < 280u ? 7 : s < 288u ? 8 : 5);
                YI_END
            } else {
                hlit = inf_take(b, 5) + 257u, hdist = inf_take(b, 5) + 1u;
                const u32 hclen = inf_take(b, 4) + 4u;
                if (inf_over(b)) return early;
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
                if (inf_over(b)) return early;
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
                    if (inf_over(b)) return early;
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
                if (inf_over(b)) return early;
                if (s < 256u) {
                    if (pos >= cap) return full;
                    if (kStore) {
                        YI_ONE sym[pos] = (u16)s;
                    }
                    pos++;
                    continue;
                }
                if (s == 256u) break;
                s -= 257u;
                if (s >= 29u) return kInfSymbol;
                const u32 len = ydf::df_len_base(s) + inf_take(b, ydf::df_len_extra(s));
                inf_refill(b);
                const u32 ds = inf_symbol(b, sh.dfast, kDistFast, sh.dcount, sh.dsym);
                if (ds >= 30u) return kInfSymbol; // (kNoSym too)
                const u32 dist = ydf::df_dist_base(ds) + inf_take(b, ydf::df_dist_extra(ds));
                if (inf_over(b)) return early;
                if (dist > front + pos) return kInfDistance;
                if (len > cap - pos) return full;
                if (kStore) {
                    // element i of the match is element i mod dist of the `dist` in front of it; what lies in front of the
                    // span's first byte is a marker (dist - pos - k - 1 <= 32 767)
                    YI_LANES(lane)
                    for (u32 i = lane; i < len; i += 64u) {
                        const u32 k = pos + (dist < len ? i % dist : i);
                        sym[pos + i] = k >= dist ? sym[k - dist] : (u16)(256u + (dist - k - 1u));
                    }
                    YI_END
                }
                pos += len;
            }
        }
        blocks++;
        const u64 at_bit = 8u * base + inf_used_bits(b);
        if (last || at_bit >= sp.stop_bit) {
            if (kStore) return at_bit == sp.end_bit && pos == sp.out_bytes && last == sp.saw_final ? (u32)kInfOk : (u32)kStrChain;
            sp.end_bit = at_bit, sp.out_bytes = pos, sp.n_blocks = blocks, sp.saw_final = last;
            return kInfOk;
        }
    }
}

// ---- WINDOWS: one team, spans in order ---------------------------------------------------------------------------------
// true spans sp[0, n_spans) in text order, their symbols in sym[0, total).  Every thread of the team calls it.  *status
// takes kStrChain where a marker names a place that does not exist or is no literal (the chain rule says: never).
YD_FN void str_windows(const Span *sp, u32 n_spans, u16 *sym, u64 total, u32 *status)
{
    for (u32 s = 1; s < n_spans; s++) {
        const u64 S = sp[s].out_off, len = sp[s].out_bytes;
        if (S > total || len > total - S) { // (the host made the table from SIZE: never)
            *status = kStrChain;
            return;
        }
        const u64 from = S + len - (len < kWindow ? len : (u64)kWindow);
        YS_EACH(x, from, S + len)
        {
            const u32 v = sym[x];
            if (v >= 256u) {
                const u64 j = v - 256u;
                const u32 w = j < S ? sym[S - 1u - j] : 256u;
                if (w >= 256u) *status = kStrChain;
                else sym[x] = (u16)w;
            }
        }
        YS_BARRIER
    }
}

// ---- BYTES ---------------------------------------------------------------------------------------------------------------
YD_FN u32 str_xpow8(u64 n_bytes) // x^(8 n) mod P for lengths beyond 32 bits (df_xpow8's loop, wider)
{
    u32 p = 1u << 31, sq = 1u << 23;
    while (n_bytes) {
        if (n_bytes & 1u) p = ydf::df_mulmod(sq, p);
        sq = ydf::df_mulmod(sq, sq);
        n_bytes >>= 1;
    }
    return p;
}

// the true span that holds text byte x: the last one that begins at or in front of it (empty spans share their start with
// the span behind them)
YD_FN u32 str_span_of(const Span *sp, u32 n_spans, u64 x)
{
    u32 lo = 0, hi = n_spans; // sp[lo].out_off <= x (out_off of span 0 is 0)
    while (hi - lo > 1u) {
        const u32 mid = lo + (hi - lo) / 2u;
        if (sp[mid].out_off <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// text bytes [x0, x0 + kThreadBytes) cut at `total`: out[] takes them, the return value is their CRC-32 (0 for none).
// x0 is a multiple of 16 and `out` is 16-byte aligned: a thread that owns all 16 bytes stores them as one.
YD_FN u32 str_bytes_thread(const Span *sp, u32 n_spans, const u16 *sym, u64 total, u64 x0, const u32 *crc_tab, u8 *out, u32 *status)
{
    if (x0 >= total) return 0;
    const u32 n = total - x0 < kThreadBytes ? (u32)(total - x0) : kThreadBytes;
    u32 w[kThreadBytes / 4] = {0, 0, 0, 0};
    u32 c = 0xFFFFFFFFu;
    for (u32 i = 0; i < n; i++) {
        u32 v = sym[x0 + i];
        if (v >= 256u) {
            const u64 S = sp[str_span_of(sp, n_spans, x0 + i)].out_off, j = v - 256u;
            v = j < S ? sym[S - 1u - j] : 256u;
            if (v >= 256u) *status = kStrChain, v = 0;
        }
        w[i >> 2] |= v << (8u * (i & 3u));
        c = crc_tab[(c ^ v) & 255u] ^ (c >> 8);
    }
    if (n == kThreadBytes) __builtin_memcpy(__builtin_assume_aligned(out + x0, 16), w, kThreadBytes);
    else
        for (u32 i = 0; i < n; i++) out[x0 + i] = (u8)(w[i >> 2] >> (8u * (i & 3u)));
    return c ^ 0xFFFFFFFFu;
}

YD_FN u32 str_crc_entry(u32 t)
{
    u32 c = t;
    for (int k = 0; k < 8; k++) c = c & 1u ? (c >> 1) ^ ydf::kCrcPoly : c >> 1;
    return c;
}

} // namespace yis

// ---- the host's part: the chain, and (not under hipcc) the whole decoder as one thread runs it ---------------------------
#include <cstddef>
#include <cstdlib>
#include <memory>
#include <new>
#include <vector>

namespace yis {

struct StreamCounts {
    u64 n_chunks = 0, n_spans = 0, n_false_starts = 0, rounds = 0, n_blocks = 0, out_bytes = 0;
};

inline u64 str_chunks(u64 pay_bytes, u32 chunk) { return pay_bytes ? (pay_bytes + chunk - 1) / chunk : 1; }

// THE CHAIN.  finds[k]: FIND's answer for chunk k + 1 (kNoBit: none); size(spans, n) walks n spans (SIZE) and fills them in,
// false: it could not (a device call failed).  true_spans: the true spans in order, their out_off set.  Returns a status;
// -1: size() failed.
template <class SizeFn>
int str_chain(const std::vector<u64> &finds, u64 pay_bytes, u32 isize, SizeFn &&size, std::vector<Span> &true_spans, StreamCounts &n)
{
    std::vector<Span> cand;
    cand.push_back(Span{0, kNoBit, 0, 0, 0, 0, 0, 0});
    for (u64 f : finds)
        if (f != kNoBit && f > cand.back().start_bit) cand.push_back(Span{f, kNoBit, 0, 0, 0, 0, 0, 0});
    for (size_t k = 0; k + 1 < cand.size(); k++) cand[k].stop_bit = cand[k + 1].start_bit;
    for (Span &c : cand) c.status = yif::kInfEarly; // (what a walk that did not run leaves)
    if (!size(cand.data(), cand.size())) return -1;
    n.rounds = 1;
    true_spans.clear();
    u64 total = 0;
    for (size_t cur = 0;;) {
        Span &c = cand[cur];
        if (c.status != yif::kInfOk) return (int)c.status;
        c.out_off = total, total += c.out_bytes, n.n_blocks += c.n_blocks;
        true_spans.push_back(c);
        if (c.saw_final) {
            const u64 used = (c.end_bit + 7u) >> 3;
            if (used != pay_bytes) return used < pay_bytes ? (int)yif::kInfLeftOver : (int)yif::kInfEarly;
            break;
        }
        size_t j = cur + 1;
        while (j < cand.size() && cand[j].start_bit < c.end_bit) j++, n.n_false_starts++; // stepped over: not block starts
        if (j < cand.size() && cand[j].start_bit == c.end_bit) {
            cur = j;
            continue;
        }
        // a proven block start without a span: one more round
        if (n.rounds > kMaxRounds) return (int)kStrRounds;
        Span fresh{c.end_bit, j < cand.size() ? cand[j].start_bit : kNoBit, 0, 0, 0, 0, yif::kInfEarly, 0};
        if (!size(&fresh, 1)) return -1;
        n.rounds++;
        cand.insert(cand.begin() + (std::ptrdiff_t)j, fresh);
        cur = j;
    }
    n.n_spans = true_spans.size(), n.out_bytes = total;
    if ((u32)total != isize) return (int)yif::kInfOutput;
    return (int)yif::kInfOk;
}

#if !defined(__HIPCC__)
// The whole decoder, one thread: pay[0, pay_bytes) -> text (exactly the text's bytes, allocated here with malloc; the
// caller frees).  Returns the status; *text is nullptr unless it is kInfOk.  -1: no memory.
inline int str_decode_host(const u8 *pay, u64 pay_bytes, u32 crc_want, u32 isize, u32 chunk, u8 **text, StreamCounts &n)
{
    *text = nullptr;
    if (chunk < kMinChunk) chunk = kMinChunk;
    if (pay_bytes > kMaxPayload) return (int)kStrPayload;
    std::unique_ptr<yif::InfShared> sh(new (std::nothrow) yif::InfShared());
    if (!sh) return -1;
    n.n_chunks = str_chunks(pay_bytes, chunk);
    std::vector<u64> finds;
    for (u64 k = 1; k < n.n_chunks; k++) {
        const u64 lo = 8u * k * chunk, hi = 8u * ((k + 1) * chunk < pay_bytes ? (k + 1) * chunk : pay_bytes);
        finds.push_back(str_find(pay, pay_bytes, lo, hi));
    }
    std::vector<Span> spans;
    const int st = str_chain(finds, pay_bytes, isize, [&](Span *s, size_t m) {
        for (size_t k = 0; k < m; k++) s[k].status = str_walk_span<false>(*sh, pay, pay_bytes, s[k], nullptr);
        return true;
    }, spans, n);
    if (st != (int)yif::kInfOk) return st;
    const u64 total = n.out_bytes;
    // exactly `total` symbols and `total` bytes (16-byte aligned for the whole-thread stores): what a sanitizer watches
    u16 *sym = (u16 *)std::malloc(total ? (size_t)total * sizeof(u16) : 1);
    u8 *out = nullptr;
    if (posix_memalign((void **)&out, 16, total ? (size_t)total : 1)) out = nullptr;
    auto give_up = [&](int code) {
        std::free(sym), std::free(out);
        return code;
    };
    if (!sym || !out) return give_up(-1);
    for (Span &s : spans)
        if (const u32 w = str_walk_span<true>(*sh, pay, pay_bytes, s, sym + s.out_off)) return give_up((int)w);
    u32 status = 0;
    str_windows(spans.data(), (u32)spans.size(), sym, total, &status);
    u32 pw[kTileThreads]; // x^(8 * 16 t): what a thread's part is shifted by inside a full tile
    for (u32 t = 0; t < kTileThreads; t++) pw[t] = str_xpow8((u64)kThreadBytes * t);
    for (u32 t = 0; t < 256u; t++) sh->crc_tab[t] = str_crc_entry(t);
    u32 crc = 0;
    for (u64 t0 = 0; t0 < total; t0 += kTile) {
        const u64 t1 = total - t0 < kTile ? total : t0 + kTile;
        u32 tile_crc = 0;
        for (u32 tid = 0; tid < kTileThreads; tid++) {
            const u64 x0 = t0 + (u64)tid * kThreadBytes;
            const u32 c = str_bytes_thread(spans.data(), (u32)spans.size(), sym, total, x0, sh->crc_tab, out, &status);
            if (x0 >= t1) continue;
            const u64 my_end = t1 - x0 < kThreadBytes ? t1 : x0 + kThreadBytes;
            tile_crc ^= ydf::df_mulmod(t1 - t0 == kTile ? pw[kTileThreads - 1u - tid] : str_xpow8(t1 - my_end), c);
        }
        crc ^= ydf::df_mulmod(str_xpow8(total - t1), tile_crc);
    }
    if (status) return give_up((int)status);
    if (crc != crc_want) return give_up((int)yif::kInfCrc);
    std::free(sym);
    *text = out;
    return (int)yif::kInfOk;
}
#endif

} // namespace yis
