// deflate_block.h — one block of text (at most 65 280 bytes) -> one BGZF member: LZ77 matches and a dynamic Huffman code
// built for the block (RFC 1951 BTYPE 2), or a stored block when that does not shrink it; the 18-byte BGZF header
// (SAM spec 4.1), CRC-32 and ISIZE.
//
// The text is written as PHASES of a 256-thread team: inside YD_PHASE(tid) ... YD_END every thread runs the body with
// its own tid, between two phases the team waits for all of them.  hipcc compiles a phase as the body plus a workgroup
// barrier (gpu_deflate.hip: one workgroup per block, DfShared in LDS); any other compiler as a loop over tid
// (libyacrd_host: yacrd_bgzf_encode_host, what the tests without a GPU check and what the GPU's bytes are compared
// with).  So nothing here may depend on the order in which the threads of a phase run: the hash table takes the
// MAXIMUM of the positions that meet in a slot, histograms add, the CRC is XORed together.  The output is a pure function
// of the block's bytes.
//
//   stage    the block -> DfShared::txt (zeros behind it); the slot is zeroed; small tables
//   crc      a thread takes 255 bytes; CRC(A ++ B) = CRC(A) * x^(8 |B|) + CRC(B) in GF(2)[x] / P joins them
//   cost     byte histogram -> what a literal costs, in 1/8 bit (integer log2: no float leaves the same bytes everywhere)
//   match    1024 positions at a time: every position looks its 4 bytes up in the hash table (u16 positions, filled
//            by the sub-chunks in front of it only) and at the byte in front of it (a run), measures the match and proposes
//            the better one when the literals it replaces cost more than a length / distance pair; then the positions enter the table; thread 0 walks the proposals
//            left to right (greedy) and writes the parse: m8[p] = 0 a literal, else length - 2 with the distance - 1
//            in m8[p + 1], m8[p + 2] (a match covers at least 4 positions)
//   count    symbol histograms (a thread takes the tokens that START in its 255 positions)
//   codes    thread 0: code lengths (Huffman by two queues over the sorted leaves; when the tree is deeper than the
//            limit the weights are halved and it is built again), canonical codes, the code-length code, header bits
//   size     bits per thread, their exclusive sums, dynamic or stored
//   emit     every thread ORs its bits into its dwords of the slot: whole dwords by plain stores, the two it shares with
//            its neighbours by atomic OR into the zeroed slot
#pragma once
#include <stdint.h>

#include "bgzf_sizes.h" // kBlock, kSlot, kEofBytes

#if defined(__HIPCC__)
#define YD_FN __device__ __forceinline__
#define YD_PHASE(tid)                                                                                                  \
    {                                                                                                                  \
        const uint32_t tid = threadIdx.x;
#define YD_END                                                                                                         \
    }                                                                                                                  \
    __syncthreads();
#else
#define YD_FN inline
#define YD_PHASE(tid) for (uint32_t tid = 0; tid < 256u; tid++) {
#define YD_END }
#endif

namespace ydf {

typedef uint8_t u8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef uint64_t u64;

constexpr u32 kT = 256;        // threads of the team
constexpr u32 kRange = kBlock / kT; // positions whose tokens a thread counts and emits
constexpr u32 kSub = 1024;     // positions per matching step
constexpr u32 kHashBits = 12;
constexpr u32 kMinMatch = 4, kMaxMatch = 257, kMaxDist = 32768;
constexpr u32 kLit = 286, kDist = 30, kCl = 19;
constexpr u32 kHdr = 18, kTrailer = 8;
static_assert(kRange * kT == kBlock, "ranges tile the block");
static_assert(kBlock + 5 + kHdr + kTrailer <= kSlot, "a stored block fits a member");

struct DfShared {
    alignas(16) u8 txt[kSlot + 16];
    alignas(16) u8 m8[kBlock + 16];
    u16 hash[1u << kHashBits]; // position + 1 of the last earlier occurrence; 0 = none
    u32 cand[kSub];            // length << 16 | distance; 0 = none
    u16 first[kT + 1];         // the first token start at or behind the range's begin
    u32 lfreq[kLit + 2], dfreq[kDist + 2], clfreq[kCl + 1];
    u16 lcode[kLit], dcode[kDist], clcode[kCl];
    u8 llen[kLit + 2], dlen[kDist + 2], cllen[kCl + 1];
    u8 len_sym[256];  // match length - 3 -> length symbol - 257
    u8 dist_sym[512]; // zlib's d_code: distance - 1 below 256, else 256 + ((distance - 1) >> 7)
    u8 lit_cost[256]; // 1/8 bit
    u32 crc_tab[256];
    u32 bits[kT + 1];
    u32 bfreq[256];
    // thread 0's between phases
    u32 pos, nr, crc, hdr_bits, total_bits, stored, hlit, hdist, hclen, member;
    // the code builder's (thread 0)
    u16 h_idx[kLit];
    u32 h_w[2 * kLit];
    u16 h_parent[2 * kLit];
    u8 h_depth[2 * kLit];
    u32 h_f[kLit];
};

YD_FN u32 df_len_base(u32 s)
{
    const u32 eb = s < 8 ? 0 : (s - 4) >> 2;
    return s == 28 ? 258 : s < 8 ? 3 + s : 3 + ((4 + (s & 3)) << eb);
}
YD_FN u32 df_len_extra(u32 s) { return s < 8 || s == 28 ? 0 : (s - 4) >> 2; }
YD_FN u32 df_dist_base(u32 s)
{
    const u32 eb = s < 4 ? 0 : (s - 2) >> 1;
    return s < 4 ? 1 + s : 1 + ((2 + (s & 1)) << eb);
}
YD_FN u32 df_dist_extra(u32 s) { return s < 4 ? 0 : (s - 2) >> 1; }

YD_FN u32 df_ilog2(u32 v) // floor(log2(v)), v >= 1
{
    u32 e = 0;
    while (v >>= 1) e++;
    return e;
}
// 8 * log2(v), v >= 1: the exponent and the three bits behind the leading one
YD_FN u32 df_log2x8(u32 v)
{
    const u32 e = df_ilog2(v);
    const u32 frac = e >= 3 ? (v >> (e - 3)) & 7u : (v << (3 - e)) & 7u;
    return 8 * e + frac;
}

// ---- CRC-32 (reflected, 0xEDB88320) and its algebra ------------------------------------------------------------------
constexpr u32 kCrcPoly = 0xEDB88320u;
YD_FN u32 df_mulmod(u32 a, u32 b) // a * b mod P, reflected: bit 31 is x^0
{
    u32 m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = b & 1 ? (b >> 1) ^ kCrcPoly : b >> 1;
        if (m == 0) break;
    }
    return p;
}
YD_FN u32 df_xpow8(u32 n_bytes) // x^(8 n) mod P
{
    u32 p = 1u << 31, sq = 1u << 23; // x^0; x^8
    while (n_bytes) {
        if (n_bytes & 1) p = df_mulmod(sq, p);
        sq = df_mulmod(sq, sq);
        n_bytes >>= 1;
    }
    return p;
}

// ---- code lengths: freq[n] -> len[n], at most `limit` bits; fewer than two used symbols get company (zlib does the
// same: a decoder wants a complete code).  One thread's work; `sh` lends the arrays.
YD_FN void df_code_lengths(DfShared &sh, const u32 *freq, u32 n, u32 limit, u8 *len)
{
    u32 used = 0;
    for (u32 s = 0; s < n; s++) {
        sh.h_f[s] = freq[s];
        used += freq[s] != 0;
        len[s] = 0;
    }
    for (u32 s = 0; s < n && used < 2; s++)
        if (sh.h_f[s] == 0) sh.h_f[s] = 1, used++;
    const u32 m = used;
    for (;;) {
        // leaves sorted by (weight, symbol)
        u32 k = 0;
        for (u32 s = 0; s < n; s++) {
            if (sh.h_f[s] == 0) continue;
            u32 i = k++;
            while (i > 0 && sh.h_f[sh.h_idx[i - 1]] > sh.h_f[s]) sh.h_idx[i] = sh.h_idx[i - 1], i--;
            sh.h_idx[i] = (u16)s;
        }
        for (u32 i = 0; i < m; i++) sh.h_w[i] = sh.h_f[sh.h_idx[i]];
        // two queues: leaves [0, m), inner nodes [m, 2m - 1) in the order they are made (their weights never fall)
        u32 a = 0, b = m, made = m;
        while (made < 2 * m - 1) {
            u32 pick[2];
            for (int q = 0; q < 2; q++) {
                if (a < m && (b >= made || sh.h_w[a] <= sh.h_w[b])) pick[q] = a++;
                else pick[q] = b++;
            }
            sh.h_w[made] = sh.h_w[pick[0]] + sh.h_w[pick[1]];
            sh.h_parent[pick[0]] = sh.h_parent[pick[1]] = (u16)made;
            made++;
        }
        sh.h_depth[2 * m - 2] = 0;
        u32 deepest = 0;
        for (u32 i = 2 * m - 2; i-- > 0;) {
            const u32 d = (u32)sh.h_depth[sh.h_parent[i]] + 1;
            sh.h_depth[i] = (u8)(d > 255 ? 255 : d);
            if (i < m && d > deepest) deepest = d;
        }
        if (deepest <= limit) break;
        for (u32 s = 0; s < n; s++)
            if (sh.h_f[s]) sh.h_f[s] = (sh.h_f[s] + 1) >> 1;
    }
    for (u32 i = 0; i < m; i++) len[sh.h_idx[i]] = sh.h_depth[i];
}
// canonical codes (RFC 1951 3.2.2), bit-reversed: they leave least significant bit first
YD_FN void df_codes(const u8 *len, u32 n, u16 *code)
{
    u32 count[16] = {0}, next[16];
    for (u32 s = 0; s < n; s++) count[len[s]]++;
    count[0] = 0;
    u32 c = 0;
    next[0] = 0;
    for (u32 b = 1; b < 16; b++) c = (c + count[b - 1]) << 1, next[b] = c;
    for (u32 s = 0; s < n; s++) {
        const u32 l = len[s];
        u32 v = 0;
        if (l) {
            const u32 x = next[l]++;
            for (u32 i = 0; i < l; i++) v |= ((x >> i) & 1u) << (l - 1 - i);
        }
        code[s] = (u16)v;
    }
}

// ---- the bit writer of one thread: bits [start, ...) of the slot -------------------------------------------------------
YD_FN void df_or32(u32 *p, u32 v)
{
#if defined(__HIPCC__)
    if (v) atomicOr(p, v);
#else
    *p |= v;
#endif
}
struct DfBits {
    u32 *w;
    u64 acc;
    u32 n, at;
    bool shared; // the dword at `at` may hold a neighbour's bits
    YD_FN void init(u32 *words, u32 bitpos) { w = words, acc = 0, n = bitpos & 31u, at = bitpos >> 5, shared = true; }
    YD_FN void put(u32 v, u32 nbits) // nbits <= 32, v < 2^nbits
    {
        acc |= (u64)v << n;
        n += nbits;
        if (n >= 32) {
            if (shared) df_or32(w + at, (u32)acc);
            else w[at] = (u32)acc;
            shared = false, acc >>= 32, n -= 32, at++;
        }
    }
    YD_FN u32 bitpos() const { return at * 32u + n; }
    YD_FN void finish()
    {
        if (n) df_or32(w + at, (u32)acc);
    }
};

YD_FN u32 df_cl_order(u32 i) // the order in which the code-length code's lengths are sent
{
    const u8 order[kCl] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return order[i];
}

// byte j of the member when the block is stored
YD_FN u32 df_stored_byte(const DfShared &sh, u32 n, u32 j, u32 crc)
{
    const u32 member = kHdr + 5 + n + kTrailer;
    if (j < kHdr) {
        const u32 bsize = member - 1;
        switch (j) {
        case 0: return 0x1f;
        case 1: return 0x8b;
        case 2: return 8;
        case 3: return 4;
        case 9: return 0xff;
        case 10: return 6;
        case 12: return 'B';
        case 13: return 'C';
        case 14: return 2;
        case 16: return bsize & 255u;
        case 17: return bsize >> 8;
        default: return 0;
        }
    }
    j -= kHdr;
    if (j == 0) return 1; // BFINAL, BTYPE 0
    if (j == 1) return n & 255u;
    if (j == 2) return n >> 8;
    if (j == 3) return (~n) & 255u;
    if (j == 4) return ((~n) >> 8) & 255u;
    j -= 5;
    if (j < n) return sh.txt[j];
    j -= n;
    if (j < 4) return (crc >> (8 * j)) & 255u;
    j -= 4;
    return j < 4 ? (n >> (8 * j)) & 255u : 0u;
}

// src[0, n) -> slot[0, member size): one member.  1 <= n <= kBlock; src and slot 16-byte aligned, slot kSlot bytes,
// src readable up to the next multiple of 16.  Every thread of the team calls it (hipcc) / one caller (elsewhere).
// *member_out, *stored_out: written by one thread.
YD_FN void df_encode_block(DfShared &sh, const u8 *src, u32 n, u8 *slot, u32 *member_out, u32 *stored_out)
{
    u32 *slot_w = reinterpret_cast<u32 *>(slot);
    // ---- stage
    YD_PHASE(tid)
    for (u32 i = tid * 16u; i < kSlot + 16u; i += kT * 16u) {
#if defined(__HIPCC__)
        uint4 v = make_uint4(0, 0, 0, 0);
        if (i + 16u <= n) v = *reinterpret_cast<const uint4 *>(src + i);
        else
            for (u32 k = 0; k < 16u; k++) {
                const u32 c = i + k < n ? src[i + k] : 0u;
                (&v.x)[k >> 2] |= c << (8 * (k & 3));
            }
        *reinterpret_cast<uint4 *>(sh.txt + i) = v;
        if (i < kSlot) *reinterpret_cast<uint4 *>(slot + i) = make_uint4(0, 0, 0, 0);
#else
        for (u32 k = 0; k < 16u; k++) {
            sh.txt[i + k] = i + k < n ? src[i + k] : 0;
            if (i < kSlot) slot[i + k] = 0;
        }
#endif
    }
    for (u32 i = tid; i < (1u << kHashBits); i += kT) sh.hash[i] = 0;
    for (u32 i = tid; i < kLit + 2; i += kT) sh.lfreq[i] = 0;
    if (tid < kDist + 2) sh.dfreq[tid] = 0;
    if (tid < kCl + 1) sh.clfreq[tid] = 0;
    sh.bfreq[tid] = 0;
    {
        u32 c = tid;
        for (int k = 0; k < 8; k++) c = c & 1 ? (c >> 1) ^ kCrcPoly : c >> 1;
        sh.crc_tab[tid] = c;
    }
    {
        u32 s = 0; // length tid + 3
        while (s < 28 && df_len_base(s + 1) <= tid + 3) s++;
        sh.len_sym[tid] = (u8)s;
        for (u32 h = 0; h < 2; h++) {
            const u32 d = h ? ((tid << 7) + 1) : tid + 1; // the smallest distance of the slot
            u32 t = 0;
            while (t < 29 && df_dist_base(t + 1) <= d) t++;
            sh.dist_sym[h * 256 + tid] = (u8)t;
        }
    }
    if (tid == 0) sh.pos = 0, sh.nr = 0, sh.crc = 0;
    YD_END
    // ---- crc of the thread's range, carried to the block's end; byte histogram
    YD_PHASE(tid)
    const u32 lo = tid * kRange < n ? tid * kRange : n, hi = (tid + 1) * kRange < n ? (tid + 1) * kRange : n;
    if (hi > lo) {
        u32 c = 0xFFFFFFFFu;
        for (u32 i = lo; i < hi; i++) c = sh.crc_tab[(c ^ sh.txt[i]) & 255u] ^ (c >> 8);
        c ^= 0xFFFFFFFFu;
        const u32 part = df_mulmod(df_xpow8(n - hi), c);
#if defined(__HIPCC__)
        atomicXor(&sh.crc, part);
        for (u32 i = lo; i < hi; i++) atomicAdd(&sh.bfreq[sh.txt[i]], 1u);
#else
        sh.crc ^= part;
        for (u32 i = lo; i < hi; i++) sh.bfreq[sh.txt[i]]++;
#endif
    }
    YD_END
    YD_PHASE(tid)
    {
        const u32 f = sh.bfreq[tid];
        u32 c = f ? df_log2x8(n) - df_log2x8(f) : 15 * 8;
        c = c < 8 ? 8 : c > 15 * 8 ? 15 * 8 : c;
        sh.lit_cost[tid] = (u8)c;
    }
    YD_END
    // ---- matches and the parse
    for (u32 base = 0; base < n; base += kSub) {
        YD_PHASE(tid)
        for (u32 j = 0; j < kSub / kT; j++) {
            const u32 q = j * kT + tid, p = base + q;
            u32 prop = 0;
            if (p + kMinMatch <= n) {
                const u32 x = (u32)sh.txt[p] | ((u32)sh.txt[p + 1] << 8) | ((u32)sh.txt[p + 2] << 16) | ((u32)sh.txt[p + 3] << 24);
                const u32 h = (x * 2654435761u) >> (32 - kHashBits);
                const u32 c = sh.hash[h];
                const u32 cap = n - p < kMaxMatch ? n - p : kMaxMatch;
                u32 best = 0;
                // two places to copy from: the last earlier occurrence the table knows, and the byte in front (a run: the one
                // repeat the table cannot know, since a sub-chunk does not see itself)
                for (u32 which = 0; which < 2; which++) {
                    u32 from;
                    if (which == 0) {
                        if (!c || p - (c - 1) > kMaxDist) continue;
                        from = c - 1;
                    } else {
                        if (p == 0 || sh.txt[p - 1] != sh.txt[p]) continue;
                        from = p - 1;
                    }
                    const u32 dist = p - from;
                    u32 l = 0, cost = 0;
                    while (l < cap && sh.txt[from + l] == sh.txt[p + l]) cost += sh.lit_cost[sh.txt[p + l]], l++;
                    if (l < kMinMatch) continue;
                    const u32 dextra = dist <= 4 ? 0 : df_ilog2(dist - 1) - 1;
                    const u32 pay = 8 * (13 + dextra + df_len_extra(sh.len_sym[l - 3])) + 8;
                    if (cost >= pay && cost - pay + 1 > best) best = cost - pay + 1, prop = (l << 16) | dist;
                }
            }
            sh.cand[q] = prop;
        }
        YD_END
        YD_PHASE(tid)
        for (u32 j = 0; j < kSub / kT; j++) {
            const u32 p = base + j * kT + tid;
            if (p + kMinMatch <= n) {
                const u32 x = (u32)sh.txt[p] | ((u32)sh.txt[p + 1] << 8) | ((u32)sh.txt[p + 2] << 16) | ((u32)sh.txt[p + 3] << 24);
                const u32 h = (x * 2654435761u) >> (32 - kHashBits);
#if defined(__HIPCC__)
                // the larger position stays: a CAS loop on the dword that holds the u16
                u32 *wp = reinterpret_cast<u32 *>(sh.hash) + (h >> 1);
                const u32 sft = (h & 1u) * 16u;
                u32 old = *wp;
                for (;;) {
                    if (((old >> sft) & 0xFFFFu) >= p + 1) break;
                    const u32 want = (old & ~(0xFFFFu << sft)) | ((p + 1) << sft);
                    const u32 seen = atomicCAS(wp, old, want);
                    if (seen == old) break;
                    old = seen;
                }
#else
                if (sh.hash[h] < p + 1) sh.hash[h] = (u16)(p + 1);
#endif
            }
        }
        if (tid == 0) { // the greedy walk over this sub-chunk's proposals
            const u32 end = base + kSub < n ? base + kSub : n;
            u32 pos = sh.pos, nr = sh.nr;
            while (pos < end) {
                while (nr < kT && nr * kRange <= pos) sh.first[nr++] = (u16)pos;
                const u32 c = sh.cand[pos - base];
                if (c) {
                    const u32 l = c >> 16, d1 = (c & 0xFFFFu) - 1;
                    sh.m8[pos] = (u8)(l - 2), sh.m8[pos + 1] = (u8)(d1 & 255u), sh.m8[pos + 2] = (u8)(d1 >> 8);
                    pos += l;
                } else {
                    sh.m8[pos] = 0;
                    pos++;
                }
            }
            sh.pos = pos, sh.nr = nr;
        }
        YD_END
    }
    YD_PHASE(tid)
    if (tid == 0)
        for (u32 nr = sh.nr; nr <= kT; nr++) sh.first[nr] = (u16)n; // (n <= 65280 fits)
    YD_END
    // ---- count
    YD_PHASE(tid)
    {
        const u32 hi = (tid + 1) * kRange < n ? (tid + 1) * kRange : n;
        for (u32 pos = sh.first[tid]; pos < hi;) {
            const u32 k = sh.m8[pos];
            u32 ls, ds = kDist + 1;
            if (k == 0) ls = sh.txt[pos], pos++;
            else {
                const u32 d1 = (u32)sh.m8[pos + 1] | ((u32)sh.m8[pos + 2] << 8);
                ls = 257u + sh.len_sym[k - 1], ds = sh.dist_sym[d1 < 256 ? d1 : 256 + (d1 >> 7)];
                pos += k + 2;
            }
#if defined(__HIPCC__)
            atomicAdd(&sh.lfreq[ls], 1u);
            if (ds < kDist) atomicAdd(&sh.dfreq[ds], 1u);
#else
            sh.lfreq[ls]++;
            if (ds < kDist) sh.dfreq[ds]++;
#endif
        }
    }
    YD_END
    // ---- codes and the header's size
    YD_PHASE(tid)
    if (tid == 0) {
        sh.lfreq[256] = 1;
        df_code_lengths(sh, sh.lfreq, kLit, 15, sh.llen);
        df_code_lengths(sh, sh.dfreq, kDist, 15, sh.dlen);
        df_codes(sh.llen, kLit, sh.lcode);
        df_codes(sh.dlen, kDist, sh.dcode);
        u32 hlit = kLit, hdist = kDist;
        while (hlit > 257 && sh.llen[hlit - 1] == 0) hlit--;
        while (hdist > 1 && sh.dlen[hdist - 1] == 0) hdist--;
        for (u32 i = 0; i < hlit; i++) sh.clfreq[sh.llen[i]]++;
        for (u32 i = 0; i < hdist; i++) sh.clfreq[sh.dlen[i]]++;
        df_code_lengths(sh, sh.clfreq, kCl, 7, sh.cllen);
        df_codes(sh.cllen, kCl, sh.clcode);
        u32 hclen = kCl;
        while (hclen > 4 && sh.cllen[df_cl_order(hclen - 1)] == 0) hclen--;
        u32 hb = 3 + 5 + 5 + 4 + 3 * hclen;
        for (u32 i = 0; i < hlit; i++) hb += sh.cllen[sh.llen[i]];
        for (u32 i = 0; i < hdist; i++) hb += sh.cllen[sh.dlen[i]];
        sh.hlit = hlit, sh.hdist = hdist, sh.hclen = hclen, sh.hdr_bits = hb;
    }
    YD_END
    // ---- size: the bits of every thread's tokens
    YD_PHASE(tid)
    {
        const u32 hi = (tid + 1) * kRange < n ? (tid + 1) * kRange : n;
        u32 b = 0;
        for (u32 pos = sh.first[tid]; pos < hi;) {
            const u32 k = sh.m8[pos];
            if (k == 0) b += sh.llen[sh.txt[pos]], pos++;
            else {
                const u32 d1 = (u32)sh.m8[pos + 1] | ((u32)sh.m8[pos + 2] << 8);
                const u32 ls = sh.len_sym[k - 1], ds = sh.dist_sym[d1 < 256 ? d1 : 256 + (d1 >> 7)];
                b += (u32)sh.llen[257u + ls] + df_len_extra(ls) + (u32)sh.dlen[ds] + df_dist_extra(ds);
                pos += k + 2;
            }
        }
        if (tid == kT - 1) b += sh.llen[256];
        sh.bits[tid] = b;
    }
    YD_END
    YD_PHASE(tid)
    if (tid == 0) {
        u32 run = sh.hdr_bits;
        for (u32 t = 0; t < kT; t++) {
            const u32 b = sh.bits[t];
            sh.bits[t] = run;
            run += b;
        }
        sh.total_bits = run;
        const u32 dyn = kHdr + (run + 7) / 8 + kTrailer, sto = kHdr + 5 + n + kTrailer;
        sh.stored = dyn >= sto;
        sh.member = sh.stored ? sto : dyn;
        *member_out = sh.member;
        *stored_out = sh.stored;
    }
    YD_END
    // ---- emit
    YD_PHASE(tid)
    if (sh.stored) {
        const u32 words = (sh.member + 3) / 4;
        for (u32 w = tid; w < words; w += kT) {
            u32 v = 0;
            for (u32 k = 0; k < 4; k++) v |= df_stored_byte(sh, n, 4 * w + k, sh.crc) << (8 * k);
            slot_w[w] = v;
        }
    } else {
        DfBits bw;
        if (tid == 0) {
            bw.init(slot_w, 0);
            const u32 bsize = sh.member - 1;
            const u8 hdr[kHdr] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, (u8)(bsize & 255u), (u8)(bsize >> 8)};
            for (u32 i = 0; i < kHdr; i++) bw.put(hdr[i], 8);
            bw.put(1, 1), bw.put(2, 2);
            bw.put(sh.hlit - 257, 5), bw.put(sh.hdist - 1, 5), bw.put(sh.hclen - 4, 4);
            for (u32 i = 0; i < sh.hclen; i++) bw.put(sh.cllen[df_cl_order(i)], 3);
            for (u32 i = 0; i < sh.hlit; i++) bw.put(sh.clcode[sh.llen[i]], sh.cllen[sh.llen[i]]);
            for (u32 i = 0; i < sh.hdist; i++) bw.put(sh.clcode[sh.dlen[i]], sh.cllen[sh.dlen[i]]);
        } else
            bw.init(slot_w, kHdr * 8 + sh.bits[tid]);
        const u32 hi = (tid + 1) * kRange < n ? (tid + 1) * kRange : n;
        for (u32 pos = sh.first[tid]; pos < hi;) {
            const u32 k = sh.m8[pos];
            if (k == 0) {
                const u32 c = sh.txt[pos];
                bw.put(sh.lcode[c], sh.llen[c]);
                pos++;
            } else {
                const u32 d1 = (u32)sh.m8[pos + 1] | ((u32)sh.m8[pos + 2] << 8);
                const u32 ls = sh.len_sym[k - 1], ds = sh.dist_sym[d1 < 256 ? d1 : 256 + (d1 >> 7)];
                bw.put(sh.lcode[257u + ls], sh.llen[257u + ls]);
                if (df_len_extra(ls)) bw.put(k + 2 - df_len_base(ls), df_len_extra(ls));
                bw.put(sh.dcode[ds], sh.dlen[ds]);
                if (df_dist_extra(ds)) bw.put(d1 + 1 - df_dist_base(ds), df_dist_extra(ds));
                pos += k + 2;
            }
        }
        if (tid == kT - 1) {
            bw.put(sh.lcode[256], sh.llen[256]);
            const u32 pad = (8u - (bw.bitpos() & 7u)) & 7u;
            if (pad) bw.put(0, pad);
            bw.put(sh.crc, 32);
            bw.put(n, 32);
        }
        bw.finish();
    }
    YD_END
}

// the empty member bgzip ends a file with
YD_FN u32 df_eof_byte(u32 j)
{
    const u8 eof[kEofBytes] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    return eof[j];
}

} // namespace ydf
