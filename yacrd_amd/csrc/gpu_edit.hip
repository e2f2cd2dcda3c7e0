// gpu_edit.hip — filter / extract on an OVERLAP file with the decision and the compaction on the GPU
// (include/yacrd_engine.h: yacrd_engine_edit_overlaps).
//
// Reference: Filter::run_paf / run_m4 (src/editor/filter.rs:140-228) and Extract::run_paf / run_m4
// (src/editor/extract.rs:144-232): a csv reader (not flexible) over the file, the ids of columns 0 and 5 (PAF, tabs)
// or 0 and 1 (M4 / MHAP, spaces) looked up in the bad-part table — an id it does not hold is NotBad,
// src/stack.rs:164-169 — and the record written back when both reads are good (filter) or when one is not (extract).
// The host loop (host/editors.cc: edit_overlaps) does that on one thread with two hash lookups per line; here the host
// only MOVES the text (gpu_text.h: the parser's mover) and the kept bytes.  On the device:
//   table    the reads' names uploaded once; an open-addressing table keyed by the name bytes (gp_hash), a slot names
//            a read, an id is compared against the uploaded bytes; value = the read's type
//   mark     32 KiB of text staged in LDS per workgroup; a thread takes the lines that START in its 128 bytes: fields
//            counted, both ids looked up, the verdict written as one bit at the line's first byte.  Bytes are then
//            counted where they LIE: a byte is kept when the line start at or in front of it is kept; the tile writes
//            its kept bytes behind its first line start, the bytes in front of it (the tail of a line that began in an
//            earlier tile) and the verdict of its last line start — which passes through tiles without one
//   carry    a tile's incoming verdict = that of the nearest earlier tile with a line start; kept bytes per tile
//   scan     stream.hip's device-wide exclusive scan over the tiles of the segment
//   pack     the tile staged again, the same keep mask rebuilt from the verdict bits, kept bytes packed in LDS and
//            stored with 16-byte stores at the tile's offset of the output buffer
// Every line ends in exactly one '\n' (a last line without one gets it: the text is one byte longer on the device);
// empty lines are lines that are never kept.  The kept bytes of a segment go home (pinned buffers, one writer thread,
// in order) while later segments are still being moved and marked.  What the path does not take — a '"' or a CR
// anywhere, a line whose field count differs from the first line's, a line more than one 4 MiB chunk longer than its
// segment — comes back as YACRD_EFALLBACK with nothing written: the caller runs the host loop.
//
// gzip out (yacrd_engine_edit_overlaps_gzip_mem / _file): the kept bytes are deflated where they lie.  The pack pass writes
// them contiguously, in file order, so when a segment's pack has finished every whole block of 65 280 bytes behind the last
// encoded one is complete: the writer thread, which learns the segment's kept count anyway, sends those blocks through
// gpu_deflate.hip's device-resident step on a stream of its own (a block's start is a multiple of 16 x 4080: the encoder's
// 16-byte loads stay aligned), the ragged tail waits for the next segment and the last batch carries the EOF member.  What
// crosses the link and reaches the file are members; one batch is fetched and written while the next is encoded and while
// later segments are moved, marked and packed.  Blocks are counted from the start of the kept stream, so the bytes are
// those of yacrd_engine_gzip_mem on the kept bytes whatever the segments, the threads or the timing.
//
// BGZF in (yacrd_engine_edit_overlaps_bgzf_mem / _file): the text comes from a TextProducer (gpu_text.h), as the
// parser's does — a BGZF stream in host memory goes up compressed, its members are inflated into the editor's text buffer as
// they land (gpu_inflate.hip: move_bgzf_text) and every whole segment of text is handed to launch_segment behind the launches
// that decoded it.  What plan() must know before the first launch comes from the stream's first and last members, decoded on
// the host (host/inflate_sample.cc).  The decoder's status word is read in verdict() before anything else and wins: the
// kernels may have run over any bytes by then (their reads are bounded whatever the text holds), and the sink may hold kept
// bytes of earlier segments — the file beside out_path goes, the buffer is freed.
// Resident (yacrd_engine_edit_overlaps_resident_mem / _file): the mirror of the engine's last one-engine overlap ingest, with
// the plan's facts recorded beside it (engine_internal.h: mirror); nothing goes up.
// In windows (EditRun::windows_loop; the route: edit_route.h): a plain text of more than one window that finds no
// room whole — or with yacrd_debug_edit_window set — goes through two text slots and two output slots whose size does not
// depend on it.  A window is to that run what a segment is to the whole-text run: one round of the same kernels, over
// positions that count from the window's first byte, with the first chunk of the next window behind it as look-ahead.  The
// byte in front of a window, the verdict that runs into it, the kept bytes so far and (gzip out) the ragged tail behind the
// last whole block are handed from window to window on the device.  The resident forms and an edit from the parser's mirror
// take the same route: their text lies whole in HBM already, so window k is the mirror's bytes from k W on, no text
// slot is held and nothing is moved; only the output ring and one window's tables are allocated.  BGZF in: the windows are the
// cuts of bgzf_windows.h that hold text — a window ends where a member ends, anywhere inside a tile —, each inflated into its
// text slot from byte 0 out of ONE compressed slot (gpu_inflate.hip: inflate_device_run_window); EditRun::bgzf_windows_loop.
#include "engine_internal.h"
#include "gpu_text.h"
#include "edit_table.h"
#include "edit_route.h"
#include "bgzf_windows.h"
#include "gpu_out.h"
#include "host/beside_file.h"

#include <condition_variable>
#include <cstdio>
#include <cstdlib>

using namespace yke;

namespace yk {

constexpr int kEdOver = 1024; // bytes staged beyond the tile: most lines that start in it end there
constexpr u32 kEdNeedHost = 1u, kEdInternal = 4u;

struct EdArgs {
    const unsigned char *text;
    u64 n;     // bytes of text
    u64 nl;    // n, or n + 1 when the last line has no newline: position n then reads as one
    u64 avail; // bytes [0, avail) of the mirror have landed (== n for the last segment)
    EdTable tab;
    uint4 *kbits;    // a bit per byte (a uint4 per 128 bytes): a KEPT line starts here
    uint4 *tile;     // per tile: kept bytes behind its first line start, bytes in front of it, flags (1: has a start, 2: its last start is kept)
    u32 *tile_kept;  // per tile: kept bytes
    u32 *tile_cin;   // per tile: the line that runs into it is kept
    const u64 *tile_off; // the segment's exclusive scan of tile_kept (entry t + seg: every segment has one more entry than tiles)
    const u64 *seg_base; // kept bytes in front of the segment
    unsigned char *out;
    unsigned long long *ctl; // [0] lines (non-empty), [1] kept lines, [2] status
    u32 tile0;       // the launch's first tile
    u32 seg;
    u32 delim, ib, n_fields, keep_good; // keep_good: filter (keep when both reads are good); else extract
    // A run in windows (EditRun::windows_loop): `text` is a window's first byte in its slot and every position, n,
    // nl, avail and the tiles count from there; the byte in front of it lies in the slot's front pad.
    u64 pos0; // the text position of text[0] (0: nothing precedes it, it begins a line)
    u64 wend; // the window's bytes: a line that ends behind them reaches into the next window (~0: the text is whole)
    unsigned long long *win; // the words handed from window to window (kEdWin*, by parity), nullptr for a whole text
    u32 wpar;                // the window's parity: it reads words [.. + wpar], writes [.. + (wpar ^ 1)]
};
// the words of EdArgs::win, two of each: window k reads the one of parity k & 1 and writes the other for window k + 1
constexpr u32 kEdWinVerdict = 0; // the verdict of the last line start so far: it runs into the window
constexpr u32 kEdWinKept = 2;    // kept bytes in front of the window
constexpr u32 kEdWinBase = 4;    // where the window's kept bytes begin in its output slot (gzip out: behind the tail; else 0)
constexpr u32 kEdWinTailAt = 6;  // gzip out: where the tail the window takes over lies in the slot of the window before
constexpr u32 kEdWinWords = 8;

// The tile [tile0, tile0 + want) -> LDS, 16 bytes per thread and step (the mirror is padded by 64 zero bytes and the last
// step is clipped to whole 16-byte pieces inside it; an inner segment's `avail` is a chunk boundary); the newline mask of
// the tile's kGpTile bytes -> nlm (a u16 per 16 bytes); returns whether a '"' or a CR lies in the tile.
__device__ __forceinline__ u32 ed_stage(const EdArgs &a, u64 tile0, u32 window, unsigned char *win, unsigned short *nlm)
{
    const u64 lim = a.avail == a.n ? ((a.n + 63) & ~(u64)15) : a.avail;
    const u32 want = (u32)min((u64)window, lim - tile0);
    u32 special = 0;
    for (u32 i = threadIdx.x * 16u; i < (u32)window; i += (u32)kGpT * 16u) {
        uint4 v = make_uint4(0, 0, 0, 0);
        if (i < want) v = *reinterpret_cast<const uint4 *>(a.text + tile0 + i);
        *reinterpret_cast<uint4 *>(win + i) = v;
        if (i < (u32)kGpTile) {
            u32 nlb = gp_eq16(v, '\n');
            const u64 at = tile0 + i;
            if (a.nl > a.n && a.n >= at && a.n < at + 16u) nlb |= 1u << (u32)(a.n - at); // (the newline the last line lacks)
            nlm[i >> 4] = (unsigned short)nlb;
            special |= gp_eq16(v, '"') | gp_eq16(v, '\r');
        }
    }
    return special;
}

struct EdMasks {
    u64 nl[2], s[2], v[2]; // of the thread's 128 bytes: newlines, line starts, bytes in front of the text's end
};
// (after ed_stage and a barrier)
__device__ __forceinline__ EdMasks ed_starts(const EdArgs &a, u64 tile0, const unsigned char *win, const unsigned short *nlm)
{
    EdMasks m;
    const uint4 q = *reinterpret_cast<const uint4 *>(nlm + threadIdx.x * 8u);
    m.nl[0] = (u64)q.x | ((u64)q.y << 32);
    m.nl[1] = (u64)q.z | ((u64)q.w << 32);
    const u64 lo = tile0 + (u64)threadIdx.x * 128u;
    const u64 left = lo < a.nl ? a.nl - lo : 0;
    m.v[0] = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
    m.v[1] = left >= 128 ? ~0ull : left > 64 ? ((1ull << (left - 64)) - 1ull) : 0ull;
    u64 prev = 1; // position 0 starts a line; any other does when a newline precedes it (a window's byte 0: the front pad's last)
    if (a.pos0 + lo != 0) prev = (threadIdx.x ? (u32)win[threadIdx.x * 128u - 1u] : (u32)(a.text - 1)[lo]) == '\n' ? 1ull : 0ull;
    m.s[0] = ((m.nl[0] << 1) | prev) & m.v[0];
    m.s[1] = ((m.nl[1] << 1) | (m.nl[0] >> 63)) & m.v[1];
    return m;
}

// bit i of the result: the nearest bit of `s` at or below i is in `k` (cin when there is none); k is a subset of s
__device__ __forceinline__ u64 ed_smear(u64 s, u64 k, u64 cin)
{
    const u64 p = ~s;
    const u64 r = ((k << 1) | cin) + p; // a carry runs from behind every kept start (or from cin) up to the next start
    return k | (p & ~r);
}
__device__ __forceinline__ u64 ed_top(u64 s, u64 k) { return (k >> (63 - __clzll((long long)s))) & 1ull; } // s != 0

// The keep mask of the thread's 128 bytes from line starts s and kept starts k; cin: the verdict that runs into the tile.
// flags: bit 0 the tile has a line start, bit 1 its last one is kept (all threads get them).  sw: 4 u32 of LDS; ends with a barrier.
__device__ __forceinline__ void ed_keep(const u64 s[2], const u64 k[2], u32 cin_tile, u32 *sw, u64 keep[2], u32 &flags)
{
    const bool has = (s[0] | s[1]) != 0;
    const u64 lastv = has ? (s[1] ? ed_top(s[1], k[1]) : ed_top(s[0], k[0])) : 0ull;
    const u64 hm = __ballot(has), vm = __ballot(lastv != 0);
    const u32 lane = lane_id(), wv = threadIdx.x >> 6;
    if (lane == 0) sw[wv] = hm ? (1u | ((u32)ed_top(hm, vm) << 1)) : 0u;
    __syncthreads();
    u32 cin = cin_tile, fl = 0;
#pragma unroll
    for (u32 w = 0; w < (u32)kGpT / 64u; w++) {
        const u32 x = sw[w];
        if (x & 1u) {
            if (w < wv) cin = x >> 1;
            fl = x;
        }
    }
    __syncthreads();
    const u64 lower = hm & ((1ull << lane) - 1ull);
    u64 c0 = lower ? ed_top(lower, vm) : (u64)cin;
    keep[0] = ed_smear(s[0], k[0], c0);
    const u64 c1 = s[0] ? ed_top(s[0], k[0]) : c0;
    keep[1] = ed_smear(s[1], k[1], c1);
    flags = fl;
}

// ---- mark: the verdict of every line that starts in the tile, and the tile's kept bytes ------------------------
__global__ __launch_bounds__(kGpT) void ed_mark_kernel(EdArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned char win[kGpTile + kEdOver];
    __shared__ __attribute__((aligned(16))) unsigned short nlm[kGpTile / 16];
    __shared__ u32 sw[4], s_first, s_inner;
    const u32 gt = a.tile0 + blockIdx.x;
    const u64 tile0 = (u64)gt * (u64)kGpTile;
    if (threadIdx.x == 0) s_first = 0xFFFFFFFFu, s_inner = 0;
    u32 status = ed_stage(a, tile0, kGpTile + kEdOver, win, nlm) ? kEdNeedHost : 0u;
    __syncthreads();
    const EdMasks m = ed_starts(a, tile0, win, nlm);
    GpText t;
    t.lds = win, t.glob = a.text, t.t0 = tile0;
    t.t1 = min(a.avail, tile0 + (u64)(kGpTile + kEdOver));
    const u64 lo = tile0 + (u64)threadIdx.x * 128u;
    u64 k[2] = {0, 0};
    u32 lines = 0, kept = 0;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        u64 todo = m.s[h] & ~m.nl[h]; // (an empty line is a start that is never kept)
        while (todo) {
            const u32 bit = (u32)__builtin_ctzll(todo);
            todo &= todo - 1;
            const u64 p = lo + (u64)h * 64u + bit;
            if (p >= a.n) break; // (the newline the last line lacks is no line)
            // fields: the first one's end, field ib's begin and end, how many
            u32 nf = 1;
            u64 i = p, end_a = 0, beg_b = 0, end_b = 0;
            for (;; i++) {
                if (i >= a.avail) {
                    if (a.avail < a.n) status |= kEdNeedHost; // (the line reaches into text still on its way)
                    break;
                }
                const u32 c = t[i];
                if (c == '\n') break;
                if (c == a.delim) {
                    if (nf == 1) end_a = i;
                    if (nf == a.ib) beg_b = i + 1;
                    if (nf == a.ib + 1) end_b = i;
                    nf++;
                }
            }
            if (nf == a.ib + 1) end_b = i;
            if (i >= a.wend) atomicMax(a.ctl + 3, (unsigned long long)(min(i + 1, a.n) - a.wend)); // (its bytes in the next window)
            if (nf != a.n_fields || nf <= a.ib) { // (csv, not flexible: the host loop words the error)
                status |= kEdNeedHost;
                continue;
            }
            const u32 ta = ed_lookup(a.tab, t, p, (u32)(end_a - p));
            const u32 tb = ed_lookup(a.tab, t, beg_b, (u32)(end_b - beg_b));
            const bool both_good = ta == 0u && tb == 0u;
            const bool keep = a.keep_good ? both_good : !both_good;
            lines++;
            if (keep) kept++, k[h] |= 1ull << bit;
        }
    }
    a.kbits[(u64)gt * (u64)kGpT + threadIdx.x] = make_uint4((u32)k[0], (u32)(k[0] >> 32), (u32)k[1], (u32)(k[1] >> 32));
    u64 keep[2];
    u32 flags;
    ed_keep(m.s, k, 0u, sw, keep, flags);
    u32 inner = (u32)__popcll(keep[0] & m.v[0]) + (u32)__popcll(keep[1] & m.v[1]);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        inner += (u32)__shfl_xor((int)inner, d, 64);
        lines += (u32)__shfl_xor((int)lines, d, 64);
        kept += (u32)__shfl_xor((int)kept, d, 64);
    }
    status = wave_or(status);
    if (m.s[0] | m.s[1]) atomicMin(&s_first, threadIdx.x * 128u + (m.s[0] ? (u32)__builtin_ctzll(m.s[0]) : 64u + (u32)__builtin_ctzll(m.s[1])));
    if (lane_id() == 0) {
        atomicAdd(&s_inner, inner);
        if (lines) atomicAdd(a.ctl, (unsigned long long)lines);
        if (kept) atomicAdd(a.ctl + 1, (unsigned long long)kept);
        if (status) atomicOr(a.ctl + 2, (unsigned long long)status);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const u32 valid = (u32)min((u64)kGpTile, a.nl - tile0);
        a.tile[gt] = make_uint4(s_inner, min(s_first, valid), flags, 0u);
    }
}

// ---- carry: the verdict that runs into every tile of the segment; its kept bytes ----------------------------------
__global__ __launch_bounds__(256) void ed_carry_kernel(EdArgs a, u32 t_end)
{
    const u32 t = a.tile0 + blockIdx.x * 256u + threadIdx.x;
    if (t >= t_end) return;
    u32 cin = a.win ? (u32)a.win[kEdWinVerdict + a.wpar] : 0u; // (a window: what the windows before it hand over)
    for (u32 q = t; q-- > 0u;) { // (one step, unless a line is longer than a tile)
        const u32 f = a.tile[q].z;
        if (f & 1u) {
            cin = (f >> 1) & 1u;
            break;
        }
    }
    const uint4 rec = a.tile[t];
    a.tile_kept[t] = rec.x + (cin ? rec.y : 0u);
    a.tile_cin[t] = cin;
    // the window's last tile hands on the verdict of the last line start so far: its own, or — a window without one — what came in
    if (a.win && t + 1u == t_end) a.win[kEdWinVerdict + (a.wpar ^ 1u)] = (rec.z & 1u) ? (rec.z >> 1) & 1u : cin;
}
// a window's other words for the next one: kept bytes so far; gzip out (block != 0): the ragged tail behind the slot's last
// whole block — it is encoded with the next window's bytes, at the front of that window's slot
__global__ void ed_window_base_kernel(unsigned long long *win, u32 par, const u64 *kept_in_window, u32 block, u32 last)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const u64 kept = *kept_in_window, filled = win[kEdWinBase + par] + kept;
    const u64 tail = block && !last ? filled % block : 0;
    win[kEdWinKept + (par ^ 1u)] = win[kEdWinKept + par] + kept;
    win[kEdWinBase + (par ^ 1u)] = tail;
    win[kEdWinTailAt + (par ^ 1u)] = filled - tail;
}
// gzip out: the tail the window of parity `par` takes over, from the slot of the window before (a multiple of the block, so
// of 16) to offset 0 of its own; its length is on the device alone
__global__ __launch_bounds__(256) void ed_tail_kernel(unsigned char *dst, const unsigned char *src, const unsigned long long *win, u32 par)
{
    const u64 len = win[kEdWinBase + par];
    src += win[kEdWinTailAt + par];
    for (u64 i = ((u64)blockIdx.x * 256u + threadIdx.x) * 16u; i < len; i += (u64)gridDim.x * 256u * 16u) {
        if (i + 16u <= len) *reinterpret_cast<uint4 *>(dst + i) = *reinterpret_cast<const uint4 *>(src + i);
        else
            for (u64 b = i; b < len; b++) dst[b] = src[b];
    }
}
__global__ void ed_base_kernel(u64 *seg_base, u32 seg, const u64 *seg_total)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) seg_base[seg + 1] = seg_base[seg] + *seg_total;
}

// ---- pack: the tile's kept bytes, packed, to its place in the output ------------------------------------------------
__global__ __launch_bounds__(kGpT) void ed_pack_kernel(EdArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned char win[kGpTile];
    __shared__ __attribute__((aligned(16))) unsigned char outb[kGpTile + 16];
    __shared__ __attribute__((aligned(16))) unsigned short nlm[kGpTile / 16]; // newline masks, then keep masks
    __shared__ __attribute__((aligned(16))) unsigned short poff[kGpTile / 16]; // where every 16-byte piece's kept bytes go
    __shared__ u32 sw[4];
    const u32 gt = a.tile0 + blockIdx.x;
    const u64 tile0 = (u64)gt * (u64)kGpTile;
    const u32 want_total = a.tile_kept[gt];
    if (want_total == 0u) return; // (uniform)
    (void)ed_stage(a, tile0, kGpTile, win, nlm);
    __syncthreads();
    const EdMasks m = ed_starts(a, tile0, win, nlm);
    if (a.nl > a.n && a.n >= tile0 && a.n < tile0 + (u64)kGpTile && threadIdx.x == 0) win[a.n - tile0] = '\n';
    const uint4 kb = a.kbits[(u64)gt * (u64)kGpT + threadIdx.x];
    const u64 k[2] = {(u64)kb.x | ((u64)kb.y << 32), (u64)kb.z | ((u64)kb.w << 32)};
    u64 keep[2];
    u32 flags;
    ed_keep(m.s, k, a.tile_cin[gt], sw, keep, flags); // (its barriers: every thread has read its nlm entries)
    keep[0] &= m.v[0], keep[1] &= m.v[1];
    u32 total = 0;
    const u32 mine = (u32)__popcll(keep[0]) + (u32)__popcll(keep[1]);
    u32 at = block_excl_add<kGpT>(mine, sw, total);
    const u64 dst0 = a.seg_base[a.seg] + a.tile_off[(u64)gt + a.seg];
    const u32 shift = (u32)(dst0 & 15u); // the packed bytes lie in outb as they will in memory: 16-byte pieces match
    {
        u32 pk[4], mk[4];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const u32 m16 = (u32)(keep[j >> 2] >> (16 * (j & 3))) & 0xFFFFu;
            const u32 o = at + shift;
            at += (u32)__popc(m16);
            if (j & 1) pk[j >> 1] |= o << 16, mk[j >> 1] |= m16 << 16;
            else pk[j >> 1] = o, mk[j >> 1] = m16;
        }
        *reinterpret_cast<uint4 *>(poff + threadIdx.x * 8u) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
        *reinterpret_cast<uint4 *>(nlm + threadIdx.x * 8u) = make_uint4(mk[0], mk[1], mk[2], mk[3]);
    }
    __syncthreads();
    if (total != want_total) { // (the two passes disagree: nothing is stored)
        if (threadIdx.x == 0) atomicOr(a.ctl + 2, (unsigned long long)kEdInternal);
        return;
    }
    for (u32 piece = threadIdx.x; piece < (u32)kGpTile / 16u; piece += (u32)kGpT) {
        u32 m16 = nlm[piece];
        if (m16 == 0u) continue;
        u32 o = poff[piece];
        const uint4 v = *reinterpret_cast<const uint4 *>(win + piece * 16u);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
        if (m16 == 0xFFFFu && (o & 3u) == 0u) {
#pragma unroll
            for (int q = 0; q < 4; q++) *reinterpret_cast<u32 *>(outb + o + 4 * q) = w[q];
        } else {
#pragma unroll
            for (int b = 0; b < 16; b++)
                if ((m16 >> b) & 1u) outb[o++] = (unsigned char)(w[b >> 2] >> (8 * (b & 3)));
        }
    }
    __syncthreads();
    // outb[shift, shift + total) -> out[dst0, dst0 + total): whole 16-byte pieces wide, the two ragged ends by bytes
    unsigned char *base = a.out + (dst0 - shift);
    const u32 end = shift + total;
    for (u32 q = threadIdx.x * 16u; q < end; q += (u32)kGpT * 16u) {
        if (q >= shift && q + 16u <= end) *reinterpret_cast<uint4 *>(base + q) = *reinterpret_cast<const uint4 *>(outb + q);
        else
            for (u32 b = max(q, shift); b < min(q + 16u, end); b++) base[b] = outb[b];
    }
}

} // namespace yk

namespace {

constexpr u64 kSegBytes = (u64)(kTextChunk * kTextSeg); // the mover's segment: what one round of mark, carry, scan and pack covers
static_assert(yer::kTile == (u64)yk::kGpTile && yer::kChunkMax == (u64)kTextChunk && yer::kWindowDefault == kSegBytes && yer::kGzBlock == (u64)ydf::kBlock,
              "edit_route.h restates the tile, the chunk, the segment and the encoder's block");

struct EditScratch { // the editor's buffers; they stay with the engine (grow-only), go with yacrd_engine_trim / destroy
    static constexpr yacrd_engine::Slot kScratchSlot = yacrd_engine::kEdit;
    DevBuf text, out, kbits, tile, tile_kept, tile_cin, tile_off, ctl, part;
    DevBuf wtext[2], wout[2]; // a run in windows (EditRun::windows_loop): its two text slots, its two output slots
    EdTableOwner table; // the reads' names and types, the id table over them
    PinBuf pin; // two output pieces + the per-segment control words
};

using yseg::Sink; // where the kept bytes go: a file descriptor or memory, sized or growing (host/segment_pump.h)

struct EditJob {
    int op = 0;
    bool m4 = false;
    int n_threads = 0;
    const yacrd_type_table *types = nullptr;
    bool use_mirror = false; // edit from the parser's mirror (the same file: checked by the caller)
    bool resident = false;   // ... with nothing but the mirror: what the plan asks of the text was recorded with it
    bool gzip = false;       // the sink takes BGZF members of the kept bytes instead of the kept bytes
    yacrd_gzip_stats *gzip_stats = nullptr;
};

// One edit on its way through the device: built once per call (run_edit), its phases in the order they run.
struct EditRun {
    yacrd_engine *e;
    const EditJob &job;
    TextProducer &tp; // plain text, or a BGZF stream inflated in HBM as it lands (gpu_text.h)
    const u64 n;      // bytes of text
    Sink &sink;
    yacrd_edit_stats *stats;
    EditScratch &S;
    // plan(): sizes
    u64 R = 0, name_bytes = 0; // reads of the type table, their names' bytes
    u64 nl = 0, n_tiles = 0;   // n, or n + 1 when the last line lacks its newline; tiles of that
    size_t n_segs = 0;
    u64 cap = 1024;            // slots of the id table
    u64 gz_blocks = 0;         // gzip out: a batch is at most a segment's kept bytes and the tail carried into it
    u32 n_fields = 0;
    double t_start = 0, t_table = 0;
    u64 W = 0;  // 0: the whole text at once; else the run goes window by window, this many bytes each (windows_loop)
    u64 wt = 0; // ... tiles of a window
    bool win_fresh[2] = {false, false}; // a text slot that is a new allocation fills faster by copy kernel, once
    // BGZF in, in windows: the cuts of the member table, those of them that hold text (the edit's windows), the
    // decoder's one compressed slot
    std::vector<ybw::WindowCut> cuts;
    std::vector<size_t> wcut;
    InflateWindow iw;
    std::atomic<u64> win_released{0};   // the writer has let go of the output of every window below this one
    // reserve(), upload_table()
    bool blit = false; // a fresh mirror fills faster by copy kernel (gpu_paf.hip)
    yk::EdArgs ga{};
    u64 *seg_base = nullptr;
    volatile u64 *h_seg = nullptr; // pinned, per segment: lines, kept, status, kept bytes so far
    volatile u32 *h_inflate = nullptr; // pinned: the decoder's status word (a BGZF text), fetched behind the last segment
    int rc_open = YACRD_OK;            // the code of an inflate that could not be set up
    // run(): the segments' kernels on the engine's stream, the writer thread behind their events
    Events ev0, ev1;           // around a segment's kernels (timing)
    std::atomic<int> bad{0};   // 1 a HIP call failed, 2 the output could not be written, 3 the text is not for this path
    OutDevice od;              // the way out of HBM (gpu_out.h; the order and the release rule: host/way_out.h)
    Out out{od, sink};
    std::atomic<size_t> dispatched{0};
    std::atomic<bool> no_more{false};
    int moved = 0; // move_text's verdict
    double out_busy_ms = 0;
    float kernel_ms = 0;

    // sizes, and whether this device's free memory takes the edit
    int plan()
    {
        const yacrd_type_table &tt = *job.types;
        R = tt.n_reads;
        if (R >= 0x7FFFFFFFull) return fail(YACRD_EFALLBACK, "more reads than the device table holds");
        if (R && (!tt.name_off || !tt.names || !tt.read_type)) return fail(YACRD_EINVAL, "the type table is incomplete");
        name_bytes = R ? tt.name_off[R] : 0;
        const char delim = job.m4 ? ' ' : '\t';
        const u32 ib = job.m4 ? 1u : 5u;
        bool ends_nl = true;
        // what the host needs of the text before the first launch: recorded with the mirror, sampled from the stream's first
        // and last members (no text on the host), or read from the text
        if (job.resident) n_fields = e->mirror.n_fields, ends_nl = e->mirror.ends_nl;
        else if (tp.bgzf) {
            if (const int rcs = tp.bgzf->text_ends(delim, n_fields, ends_nl)) return rcs;
        } else if (!first_line_fields(tp.src, n, delim, n_fields, ends_nl)) return fail(YACRD_EINVAL, "read error in the overlap file");
        if (n_fields && n_fields <= ib) return fail(YACRD_EFALLBACK, "the first line has too few fields: the host loop words the error");
        nl = n + (ends_nl ? 0 : 1);
        n_tiles = (nl + yk::kGpTile - 1) / yk::kGpTile;
        if (n_tiles >= 0x7FFFFFFFull) return fail(YACRD_EFALLBACK, "file too large for the device editor");
        n_segs = (size_t)((n + kSegBytes - 1) / kSegBytes);
        while (cap < 2 * R) cap <<= 1;
        gz_blocks = job.gzip ? (std::min<u64>(nl, kSegBytes) + ydf::kBlock - 1) / ydf::kBlock + 1 : 0;
        ga.delim = (u32)(unsigned char)delim, ga.ib = ib, ga.n_fields = n_fields, ga.keep_good = job.op == 1 ? 1u : 0u;
        t_start = now_ms();
        // HBM: the text (unless the parser's mirror serves), as many bytes again for what is kept, a bit per byte, the table
        // The route (edit_route.h): a plain text of more than one window runs in windows where the whole-text need
        // finds no room, where the switch names a window, or — kEdWindowsWhenFits — always.  The resident forms and an edit from
        // the parser's mirror take the same route with the text left out of both needs: it lies in HBM already.
        // BGZF in: the window is at least bgzf_windows.h's smallest (a member inflates as a unit), the windows are the cuts
        // that hold text, and the ring counts the decoder's compressed slot and the largest slice of the member table.
        u64 sw = e->edit_window;
        if (tp.bgzf && sw != 0 && sw != UINT64_MAX && yer::window_of(sw) < ybw::kMinWindow) sw = ybw::kMinWindow;
        const u64 Wn = yer::window_of(sw), w_tiles = Wn / yk::kGpTile + 2;
        u64 max_slice = 0;
        if (tp.bgzf && n > Wn && sw != UINT64_MAX) {
            if (!ybw::window_cuts(tp.bgzf->members.data(), tp.bgzf->members.size(), Wn, cuts)) return fail(YACRD_ENOMEM, "host allocation failed");
            try {
                for (size_t i = 0; i < cuts.size(); i++) {
                    max_slice = std::max<u64>(max_slice, cuts[i].m1 - cuts[i].m0);
                    if (cuts[i].t1 > cuts[i].t0) wcut.push_back(i);
                }
            } catch (...) {
                return fail(YACRD_ENOMEM, "host allocation failed");
            }
        }
        const u64 w_gz_blocks = job.gzip ? (yer::out_slot_bytes(Wn, true) + ydf::kBlock - 1) / ydf::kBlock : 0;
        bool whole_fits = true, ring_fits = true;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const double table_need = (double)name_bytes * 1.125 + (double)cap * 4.0 + (double)R * 10.0 + (double)((size_t)64 << 20);
            // (a BGZF stream: its compressed bytes and the member table lie in HBM beside the text; the inflate scratch counts as held)
            const double have = (double)free_b + (double)S.text.cap + (double)S.out.cap + (double)S.kbits.cap + (double)S.table.names.cap +
                                (double)S.table.slots.cap + (tp.bgzf ? (double)inflate_device_held(e) : 0.0);
            const double need = (job.use_mirror ? 0.0 : (double)n) + (tp.bgzf ? tp.bgzf->device_bytes() : 0.0) + (double)nl * 1.125 + (double)nl / 8.0 * 1.125 +
                                table_need + (double)n_tiles * 40.0 +
                                (double)gz_blocks * (double)ydf::kSlot * 3.0 * 1.125; // (the members' slots and two batches of members)
            whole_fits = need <= have;
            // the ring: two text and two output slots, one window's tables (the whole text's buffers go before it is taken);
            // from the mirror: the two output slots alone (text slots an earlier run left go as well)
            const double ring_have = have + (double)S.wtext[0].cap + (double)S.wtext[1].cap + (double)S.wout[0].cap + (double)S.wout[1].cap +
                                     (tp.bgzf ? (double)inflate_window_held(e) : 0.0);
            const double ring_need = (job.use_mirror ? 0.0 : 2.0 * (double)yer::text_slot_bytes(Wn)) + 2.0 * (double)yer::out_slot_bytes(Wn, job.gzip) +
                                     (tp.bgzf ? ((double)Wn + 64.0 + (double)(max_slice + 64) * sizeof(yif::InfMember)) * 1.125 : 0.0) +
                                     (double)w_tiles * ((double)yk::kGpT * 16.0 + 40.0) * 1.125 + table_need +
                                     (double)w_gz_blocks * (double)ydf::kSlot * 3.0 * 1.125;
            ring_fits = ring_need <= ring_have;
        }
        const yer::Route route = yer::route(n, sw, whole_fits, ring_fits, tp.bgzf ? yer::kEdBgzfWindowsWhenFits : yer::kEdWindowsWhenFits);
        if (route == yer::kFallback) return fail(YACRD_EFALLBACK, "the file is too large to be edited in this device's free memory: the host loop streams it");
        if (route == yer::kWindows) {
            W = Wn, wt = Wn / yk::kGpTile;
            // (a window is what a segment is to the whole-text run: one round of the kernels)
            n_segs = tp.bgzf ? wcut.size() : (size_t)((n + W - 1) / W);
            gz_blocks = w_gz_blocks;
        }
        return YACRD_OK;
    }

    // every buffer of the edit, the encoder's included: nothing is allocated once the first segment is handed over
    int reserve()
    {
        const void *mirror_before = S.text.p;
        if (W) {
            // the ring is what a run in windows holds: the whole-text run's two buffers go first; the slots are exactly their
            // size (no slack: the ring's bytes are a function of W alone)
            S.text.release(), S.out.release();
            if (tp.bgzf) {
                inflate_device_release_whole(e); // (and the whole stream's buffer and member table in the inflate scratch)
                if (const int rcw = inflate_window_open(e, W, &iw)) return rcw;
            }
            for (int i = 0; i < 2; i++) {
                const void *before = S.wtext[i].p;
                if (job.use_mirror) S.wtext[i].release(); // (the windows are the mirror's own bytes: no text slot is held)
                else HIP_TRY(S.wtext[i].reserve_exact((size_t)yer::text_slot_bytes(W)));
                win_fresh[i] = !job.use_mirror && S.wtext[i].p != before;
                HIP_TRY(S.wout[i].reserve_exact((size_t)yer::out_slot_bytes(W, job.gzip)));
            }
        } else {
            if (!job.use_mirror) HIP_TRY(S.text.reserve((size_t)n + 64));
            blit = !job.use_mirror && S.text.p != mirror_before;
            if (!job.use_mirror) HIP_TRY(hipMemsetAsync(S.text.as<char>() + n, 0, 64, e->stream));
            HIP_TRY(S.out.reserve((size_t)nl + 64));
        }
        const u64 tiles = W ? wt + 1 : n_tiles; // (a window: its tiles and the one the newline the last line lacks may open)
        HIP_TRY(S.kbits.reserve((size_t)(tiles + 1) * yk::kGpT * sizeof(uint4)));
        HIP_TRY(S.tile.reserve((size_t)(tiles + 1) * sizeof(uint4)));
        HIP_TRY(S.tile_kept.reserve((size_t)(tiles + 1) * sizeof(u32)));
        HIP_TRY(S.tile_cin.reserve((size_t)(tiles + 1) * sizeof(u32)));
        HIP_TRY(S.tile_off.reserve((size_t)(tiles + (W ? 0 : n_segs) + 2) * sizeof(u64)));
        const size_t ctl_words = 8 + (W ? (size_t)yk::kEdWinWords : n_segs + 2);
        HIP_TRY(S.ctl.reserve(ctl_words * sizeof(u64)));
        HIP_TRY(hipMemsetAsync(S.ctl.p, 0, ctl_words * sizeof(u64), e->stream));
        HIP_TRY(S.pin.reserve(2 * kOutPiece + (n_segs + 2) * 4 * sizeof(u64) + (job.gzip ? 4 * sizeof(u64) : 0) + sizeof(u64)));
        h_seg = reinterpret_cast<volatile u64 *>(S.pin.as<char>() + 2 * kOutPiece);
        volatile u64 *h_gz = h_seg + (n_segs + 2) * 4; // gzip out: the encoder's two pairs of words
        h_inflate = reinterpret_cast<volatile u32 *>(h_gz + (job.gzip ? 4 : 0));
        *h_inflate = 0;
        // (no wait for the engine's stream behind the open: upload_table() waits for it, in front of the first segment)
        if (job.gzip)
            if (const int rcg = od.open(e, gz_blocks, false)) return rcg;
        od.stop = &bad;
        out.bind(S.pin.as<char>(), h_gz);
        return YACRD_OK;
    }

    // the reads' names and types -> HBM, the id table over them; the kernels' arguments
    int upload_table()
    {
        const yacrd_type_table &tt = *job.types;
        yk::EdTable tab{};
        if (const int rc = S.table.upload(e, tt.names, tt.name_off, tt.read_type, R, name_bytes, cap, &tab)) return rc;
        HIP_TRY(hipStreamSynchronize(e->stream));
        t_table = now_ms();
        ga.text = job.use_mirror ? e->mirror.p : S.text.as<unsigned char>();
        ga.n = n, ga.nl = nl;
        ga.tab = tab;
        ga.kbits = S.kbits.as<uint4>(), ga.tile = S.tile.as<uint4>(), ga.tile_kept = S.tile_kept.as<u32>(), ga.tile_cin = S.tile_cin.as<u32>();
        ga.tile_off = S.tile_off.as<u64>();
        ga.ctl = S.ctl.as<unsigned long long>();
        seg_base = S.ctl.as<u64>() + 8;
        ga.seg_base = seg_base;
        ga.out = S.out.as<unsigned char>();
        ga.pos0 = 0, ga.wend = ~0ull, ga.win = nullptr, ga.wpar = 0; // (a run in windows sets them window by window)
        return YACRD_OK;
    }

    // a segment has landed (or lies in the mirror): mark, carry, scan, pack on the engine's stream, its counts to the host
    void launch_segment(u64 seg_begin, u64 seg_end, u64 avail)
    {
        const size_t s = (size_t)(seg_begin / kSegBytes);
        const u32 t0 = (u32)(seg_begin / yk::kGpTile), t1 = seg_end >= n ? (u32)n_tiles : (u32)(seg_end / yk::kGpTile);
        ga.avail = avail, ga.tile0 = t0, ga.seg = (u32)s;
        bool ok = hipEventRecord(ev0[s], e->stream) == hipSuccess;
        if (t1 > t0) {
            hipLaunchKernelGGL(yk::ed_mark_kernel, dim3(t1 - t0), dim3(yk::kGpT), 0, e->stream, ga);
            hipLaunchKernelGGL(yk::ed_carry_kernel, dim3((t1 - t0 + 255) / 256), dim3(256), 0, e->stream, ga, t1);
        }
        u64 *seg_off = S.tile_off.as<u64>() + t0 + s;
        ok = ok && scan_u32_to_u64(e, S.tile_kept.as<u32>() + t0, (u64)(t1 - t0), seg_off, S.part) == YACRD_OK;
        hipLaunchKernelGGL(yk::ed_base_kernel, dim3(1), dim3(64), 0, e->stream, seg_base, (u32)s, seg_off + (t1 - t0));
        if (t1 > t0) hipLaunchKernelGGL(yk::ed_pack_kernel, dim3(t1 - t0), dim3(yk::kGpT), 0, e->stream, ga);
        ok = ok && hipMemcpyAsync((void *)(h_seg + 4 * s), S.ctl.p, 3 * sizeof(u64), hipMemcpyDeviceToHost, e->stream) == hipSuccess;
        ok = ok && hipMemcpyAsync((void *)(h_seg + 4 * s + 3), seg_base + s + 1, sizeof(u64), hipMemcpyDeviceToHost, e->stream) == hipSuccess;
        ok = ok && hipEventRecord(ev1[s], e->stream) == hipSuccess;
        if (!ok) bad = 1;
        dispatched.store(s + 1, std::memory_order_release);
    }

    // ---- a run in windows ------------------------------------------------------------------------------------
    u64 win_tail = 0; // gzip out, the writer's: the kept bytes behind the last encoded block (what the device holds in kEdWinBase)
    unsigned char *wslot(u64 k) const // window k's byte 0: behind its slot's front pad, or where it lies in the mirror
    {
        return job.use_mirror ? const_cast<unsigned char *>(e->mirror.p) + k * W /* (read only) */ : S.wtext[k & 1].as<unsigned char>() + 16;
    }
    // window k's first text position and its bytes (BGZF in: those of the k-th cut that holds text, at most W)
    u64 wbase(u64 k) const { return tp.bgzf ? cuts[wcut[k]].t0 : k * W; }
    u64 wlen(u64 k) const { return tp.bgzf ? cuts[wcut[k]].t1 - cuts[wcut[k]].t0 : std::min<u64>(W, n - k * W); }

    // Window k lies in its slot with `ahead` bytes of window k + 1 behind it: the same mark, carry, scan and pack as a segment
    // of the whole-text run, over positions that count from the window's byte 0.  What it takes from the windows before it
    // and leaves for the next lies on the device (EdArgs::win); its counts go to the host behind the pack, as a segment's do.
    // From the mirror the window lies where the ingest left it: W is a multiple of the tile, so its byte 0 is as aligned as the
    // mirror's, the byte in front of it and the look-ahead are the mirror's own, and the 64 zero bytes behind the text's end
    // are the ones the ingest put there (gpu_paf.hip: ingest_text).
    void launch_window(u64 k, u64 ahead)
    {
        const bool last = k + 1 == n_segs;
        const u32 par = (u32)(k & 1);
        // BGZF in: a window that is not the last ends where a member ends, anywhere inside a tile.  Its `nl` is its own bytes L:
        // ed_starts' mask of positions below nl then keeps every position >= L from being a line start, from being counted
        // and from being packed, the last tile's `valid` is min(tile, L - tile0) and its flags — so the verdict handed on —
        // come from the window's last line start.  The line walk reads up to avail = L + ahead as before.  (nl > n, the
        // newline the text's last line lacks, only ever concerns the last window.)
        const u64 base = wbase(k), L = wlen(k);
        const u64 n_loc = n - base, nl_loc = tp.bgzf && !last ? L : nl - base;
        const u32 t1 = last || tp.bgzf ? (u32)((nl_loc + yk::kGpTile - 1) / yk::kGpTile) : (u32)wt; // (at most wt + 1: reserve())
        unsigned long long *win = S.ctl.as<unsigned long long>() + 8;
        ga.text = wslot(k), ga.n = n_loc, ga.nl = nl_loc;
        ga.avail = last ? n_loc : L + ahead; // (== n_loc where the look-ahead holds the text's end: position n_loc then ends a line)
        ga.tile0 = 0, ga.seg = 0, ga.pos0 = base, ga.wend = last ? ~0ull : L, ga.win = win, ga.wpar = par;
        ga.seg_base = reinterpret_cast<const u64 *>(win + yk::kEdWinBase + par);
        ga.out = S.wout[par].as<unsigned char>();
        bool ok = hipEventRecord(ev0[k], e->stream) == hipSuccess;
        // (the 64 zero bytes ed_stage's last 16-byte steps read behind the text's end: inside the slot, n_loc <= W + C here)
        // (BGZF in: avail is no multiple of 16, so those steps read up to 15 bytes behind it wherever it lies: L + ahead <= W + C)
        if ((ga.avail == n_loc || tp.bgzf) && !job.use_mirror) ok = ok && hipMemsetAsync(wslot(k) + ga.avail, 0, 64, e->stream) == hipSuccess;
        if (job.gzip && k)
            hipLaunchKernelGGL(yk::ed_tail_kernel, dim3(16), dim3(256), 0, e->stream, ga.out, S.wout[par ^ 1].as<unsigned char>(), win, par);
        hipLaunchKernelGGL(yk::ed_mark_kernel, dim3(t1), dim3(yk::kGpT), 0, e->stream, ga);
        hipLaunchKernelGGL(yk::ed_carry_kernel, dim3((t1 + 255) / 256), dim3(256), 0, e->stream, ga, t1);
        u64 *off = S.tile_off.as<u64>();
        ok = ok && scan_u32_to_u64(e, S.tile_kept.as<u32>(), (u64)t1, off, S.part) == YACRD_OK;
        hipLaunchKernelGGL(yk::ed_window_base_kernel, dim3(1), dim3(64), 0, e->stream, win, par, off + t1, job.gzip ? (u32)ydf::kBlock : 0u, last ? 1u : 0u);
        hipLaunchKernelGGL(yk::ed_pack_kernel, dim3(t1), dim3(yk::kGpT), 0, e->stream, ga);
        ok = ok && hipMemcpyAsync((void *)(h_seg + 4 * k), S.ctl.p, 3 * sizeof(u64), hipMemcpyDeviceToHost, e->stream) == hipSuccess;
        ok = ok && hipMemcpyAsync((void *)(h_seg + 4 * k + 3), win + yk::kEdWinKept + (par ^ 1u), sizeof(u64), hipMemcpyDeviceToHost, e->stream) == hipSuccess;
        ok = ok && hipEventRecord(ev1[k], e->stream) == hipSuccess;
        if (!ok) bad = 1;
        dispatched.store((size_t)k + 1, std::memory_order_release);
    }

    // The windows, on the launching thread; move_text's code.  Window k's text lands in slot k & 1 in two moves: its first
    // chunk C = min(4 MiB, W) while window k - 1 waits for it as its look-ahead, the rest afterwards, beside window k - 1's
    // kernels.  Then window k + 1's first chunk lands in the other slot, is copied on the device behind window k's W bytes
    // — with window k's last byte to the other slot's front pad —, and window k's kernels follow those copies on the
    // engine's stream.  A line that starts in window k is marked in window k and may end up to C bytes into window k + 1;
    // one that reaches farther sets kEdNeedHost, as in the whole-text run a line that reaches beyond the chunk behind its
    // segment does.  Who may write which slot when:
    //   text slot k & 1       Read by window k's kernels (mark, pack); window k - 2's were the last before them.  Its bytes
    //     [0, C) are written by window k's first move, which begins after this thread has waited for window k - 2's
    //     event (ev1: behind its pack); its bytes [C, W) by the second move, later still.  The look-ahead [W, W + C) and
    //     the front pad are written by copies on the engine's stream, behind window k - 2's kernels and in front of
    //     window k's.  Both moves end (move_text waits for its copy streams) before the copies that read them are enqueued.
    //   text slot (k + 1) & 1  While window k's kernels run it takes window k + 1's rest: they read of it only what the
    //     device copies took before them — nothing.
    //   output slot k & 1     Written by window k's tail copy and pack, behind the wait below for win_released > k - 2 (when
    //     the writer lets a slot go: host/way_out.h), and window k - 1's tail copy, the only other reader, ran on the
    //     engine's stream in front of window k's launches.  The writer reads it behind ev1[k].
    //   the per-window tables, the words of EdArgs::win   One stream, in order; a word read by window k + 1 is written by
    //     window k and overwritten by window k + 2 at the earliest.  The pinned words are per window.
    // From the mirror there is no text slot and no move: the text is read-only for the whole run and lay complete
    // before it began (the ingest that left it has returned), so of the above only the output slots and the per-window tables
    // remain, argued as they are there.
    int windows_loop()
    {
        const u64 K = n_segs, C = yer::chunk_of(W);
        auto nap = [] {
            struct timespec ts = {0, 20000};
            nanosleep(&ts, nullptr);
        };
        if (job.use_mirror) {
            for (u64 k = 0; k < K && !bad.load(); k++) {
                while (k >= 2 && win_released.load(std::memory_order_acquire) < k - 1 && !bad.load()) nap(); // (the output slot)
                if (bad.load()) break;
                launch_window(k, k + 1 == K ? 0 : std::min(C, wlen(k + 1)));
            }
            (void)hipStreamSynchronize(e->stream);
            return 0;
        }
        Streams lanes; // the mover's copy streams, made once for all the moves
        auto land = [&](u64 k, u64 from, u64 upto) -> int { // bytes [from, upto) of window k -> its slot
            if (upto <= from) return 0;
            return move_text(e, tp.src, k * W + from, upto - from, reinterpret_cast<char *>(wslot(k)) + from, win_fresh[k & 1], job.n_threads,
                             [](u64, u64, u64) {}, (size_t)C, &lanes);
        };
        int rc = land(0, 0, std::min(C, wlen(0)));
        for (u64 k = 0; k < K && !rc && !bad.load(); k++) {
            const bool last = k + 1 == K;
            rc = land(k, C, wlen(k));
            win_fresh[k & 1] = false;
            u64 ahead = 0;
            if (!rc && !last) {
                if (k >= 1 && hipEventSynchronize(ev1[k - 1]) != hipSuccess) bad = 1; // (the other text slot: window k - 1's pack has read it)
                if (bad.load()) break;
                ahead = std::min(C, wlen(k + 1));
                rc = land(k + 1, 0, ahead);
                if (rc) break;
                if (hipMemcpyAsync(wslot(k) + W, wslot(k + 1), (size_t)ahead, hipMemcpyDeviceToDevice, e->stream) != hipSuccess ||
                    hipMemcpyAsync(wslot(k + 1) - 1, wslot(k) + W - 1, 1, hipMemcpyDeviceToDevice, e->stream) != hipSuccess)
                    bad = 1;
            }
            while (k >= 2 && win_released.load(std::memory_order_acquire) < k - 1 && !bad.load()) nap(); // (the output slot)
            if (rc || bad.load()) break;
            launch_window(k, ahead);
        }
        (void)hipStreamSynchronize(e->stream); // (the copy streams go with `lanes`; nothing of theirs is pending: move_text waits)
        return rc;
    }

    // BGZF in, in windows, on the launching thread; move_text's code.  The cuts of the member table are taken in
    // order; cut i's bytes [c0, c1) of the stream land in the ONE compressed slot, its slice of the member table goes up and its
    // members are inflated on the engine's stream.  A cut that holds text is the edit's window k: it is inflated into text slot
    // k & 1 from byte 0 (tile-aligned), not moved.  A cut without text (a trailing EOF member in a cut of its own, more than W
    // bytes of empty members) is inflated and checked like any other, stores nothing, launches no edit kernel and is
    // invisible to the look-ahead and to the words of EdArgs::win.  Window k's look-ahead is the first ahead = min(C, L(k + 1))
    // bytes of window k + 1, copied on the device behind window k's L(k) bytes, and window k's last byte goes to the other
    // slot's front pad: 7n's two copies with L(k) in place of W.  Everything the device does here is enqueued on the engine's
    // stream, in this order per window k: [inflate of the cuts up to window k + 1's] [the two copies] [window k's kernels].
    // Who may write which buffer when:
    //   compressed slot   Written by this thread's move (move_text waits for its copy streams) for cut i only after it has
    //     waited for the event behind the inflate of cut i - 1, the slot's only reader.  That inflate stands in the stream in
    //     front of window k - 1's kernels, so the landing of window k + 1's cut runs beside them.
    //   member slice      (grow-only, in the inflate scratch) reserved and filled inside inflate_device_run_window, behind the
    //     same wait: the inflate of cut i - 1, its last reader, has ended, so a reserve that grows it frees nothing a kernel
    //     reads; the refill is ordered on the engine's stream.
    //   text slot (k + 1) & 1   Written by the inflate of window k + 1, enqueued behind window k - 1's kernels (mark, pack:
    //     its last readers) on the same stream, so behind ev1[k - 1]; its front pad by the one-byte copy behind that inflate.
    //     Read by the look-ahead copy and by window k + 1's kernels, both enqueued later.
    //   text slot k & 1   Its bytes [L(k), L(k) + ahead + 64) are written by the look-ahead copy and launch_window's memset,
    //     behind the inflate of window k (which stored [0, L(k)) only) and in front of window k's kernels.
    //   status word       One for the run, zeroed by inflate_window_open on the engine's stream; only ever raised.  It comes
    //     home behind the last launch and verdict() reads it before anything the text says is believed: output of earlier
    //     windows may have left by then, which is what bad = 3's path is for (the file beside out_path goes, the buffer is freed).
    //   output slots (host/way_out.h), the per-window tables, the words of EdArgs::win   As in windows_loop.
    int bgzf_windows_loop()
    {
        const u64 K = n_segs, C = yer::chunk_of(W);
        BgzfIn &in = *tp.bgzf;
        Streams lanes;
        TextSource comp_src;
        comp_src.mem = in.comp;
        bool comp_fresh = iw.fresh;
        size_t next_cut = 0; // the first cut not yet inflated
        auto inflate_cut = [&](size_t i, unsigned char *dst) -> int {
            const ybw::WindowCut &c = cuts[i];
            if (i && hipEventSynchronize(in.move.ev[2 * i - 1]) != hipSuccess) return 1; // (the compressed slot, the member slice)
            const double t0 = now_ms();
            const int moved_c = move_text(e, comp_src, c.c0, c.c1 - c.c0, reinterpret_cast<char *>(iw.comp), comp_fresh, job.n_threads, [](u64, u64, u64) {},
                                          (size_t)C, &lanes);
            comp_fresh = false;
            in.move.h2d_ms += (float)(now_ms() - t0);
            if (moved_c) return moved_c;
            if (!in.move.ev.add(2) || hipEventRecord(in.move.ev[2 * i], e->stream) != hipSuccess) return 1;
            if (const int rcw = inflate_device_run_window(e, iw, e->stream, in.members.data() + c.m0, c.m1 - c.m0, c.c0, c.c1, c.t0, c.t1, dst)) {
                rc_open = rcw;
                return 1;
            }
            if (hipEventRecord(in.move.ev[2 * i + 1], e->stream) != hipSuccess) return 1;
            in.move.n_ev = 2 * i + 2, in.move.n_launches++;
            return 0;
        };
        auto inflate_upto = [&](u64 k) -> int { // every cut not yet inflated up to window k's own; that one into window k's slot
            for (; next_cut <= wcut[k]; next_cut++)
                if (const int r = inflate_cut(next_cut, wslot(k))) return r;
            return 0;
        };
        auto nap = [] {
            struct timespec ts = {0, 20000};
            nanosleep(&ts, nullptr);
        };
        int rc = inflate_upto(0);
        for (u64 k = 0; k < K && !rc && !bad.load(); k++) {
            u64 ahead = 0;
            if (k + 1 < K) {
                rc = inflate_upto(k + 1);
                if (rc) break;
                ahead = std::min(C, wlen(k + 1));
                if (hipMemcpyAsync(wslot(k) + wlen(k), wslot(k + 1), (size_t)ahead, hipMemcpyDeviceToDevice, e->stream) != hipSuccess ||
                    hipMemcpyAsync(wslot(k + 1) - 1, wslot(k) + wlen(k) - 1, 1, hipMemcpyDeviceToDevice, e->stream) != hipSuccess)
                    bad = 1;
            } else // (the cuts behind the last window: no text, their members inflated and checked all the same)
                for (; next_cut < cuts.size() && !rc; next_cut++) rc = inflate_cut(next_cut, wslot(k + 1));
            while (k >= 2 && win_released.load(std::memory_order_acquire) < k - 1 && !bad.load()) nap(); // (the output slot)
            if (rc || bad.load()) break;
            launch_window(k, ahead);
        }
        *h_inflate = 0;
        if (hipMemcpyAsync(const_cast<u32 *>(h_inflate), iw.status, sizeof(u32), hipMemcpyDeviceToHost, e->stream) != hipSuccess && !rc) rc = 1;
        (void)hipStreamSynchronize(e->stream);
        return rc;
    }

    // what the way out says (host/way_out.h) as this run's code; a stop is another thread's code, which stays
    void took(yout::Result r)
    {
        if (r == yout::kSinkFailed) bad = 2;
        else if ((r == yout::kDeviceFailed || r == yout::kBoundBroken) && !bad.load()) bad = 1;
    }

    // the writer thread: segment by segment, in order, what the pack has finished goes home (or to the encoder)
    void writer()
    {
        if (hipSetDevice(e->device) != hipSuccess) bad = 1;
        u64 from = 0;
        size_t seen = 0; // segments taken
        for (size_t s = 0; s < n_segs && !bad.load(); s++) {
            while (dispatched.load(std::memory_order_acquire) <= s && !no_more.load() && !bad.load()) {
                struct timespec ts = {0, 50000};
                nanosleep(&ts, nullptr);
            }
            if (dispatched.load(std::memory_order_acquire) <= s || bad.load()) break;
            if (hipEventSynchronize(ev1[s]) != hipSuccess) {
                bad = 1;
                break;
            }
            if (h_seg[4 * s + 2] != 0) { // (a quote, a CR, a line of another shape: nothing more is written)
                bad = 3;
                break;
            }
            const u64 upto = h_seg[4 * s + 3];
            if (upto < from || upto > nl) {
                bad = 1;
                break;
            }
            const double t0 = now_ms();
            const bool last = s + 1 == n_segs;
            if (W) {
                // a window's kept bytes lie in its own slot, from 0 (gzip out: behind the tail of the window before, which
                // ed_tail_kernel has put there).  The slot is let go when nothing reads it any more: plain, when its bytes
                // are home; gzip out, one window later, when every batch but this window's has been fetched — so that a batch
                // is encoded while the one before it comes home, as in the whole-text run
                if (!job.gzip) {
                    took(out.home(S.wout[s & 1].as<char>(), upto - from));
                    win_released.store((u64)s + 1, std::memory_order_release);
                } else {
                    const u64 filled = win_tail + (upto - from), whole = last ? filled : filled / ydf::kBlock * ydf::kBlock;
                    took(out.text(S.wout[s & 1].as<unsigned char>(), whole, last, yout::kNoTag));
                    win_tail = filled - whole;
                    win_released.store((u64)s, std::memory_order_release);
                }
            } else if (!job.gzip) took(out.home(S.out.as<char>() + from, upto - from));
            else {
                // every whole block that now lies complete behind the last encoded one (the last segment: the tail too, and
                // the EOF member) goes to the encoder; the batch before it comes home while this one is encoded
                const u64 whole = last ? upto : upto / ydf::kBlock * ydf::kBlock;
                if (whole > out.text_bytes || last) took(out.text(S.out.as<unsigned char>() + out.text_bytes, whole - out.text_bytes, last, yout::kNoTag));
            }
            from = upto, seen = s + 1;
            out_busy_ms += now_ms() - t0;
        }
        if (job.gzip && !bad.load() && seen == n_segs) {
            const double t0 = now_ms();
            if (n_segs == 0) took(out.text(S.out.as<unsigned char>(), 0, true, yout::kNoTag)); // (an empty text: the EOF member alone)
            took(out.drain());
            out_busy_ms += now_ms() - t0;
        }
    }

    // streams and events, then the text through the device: this thread moves it (or walks the mirror) and launches the
    // segments, the writer thread takes them from their events.  false: a stream or an event could not be created
    bool run()
    {
        if (!od.make(job.gzip) || !ev0.add(n_segs) || !ev1.add(n_segs)) return false;
        std::thread wt([this] { writer(); });
        if (W) moved = tp.bgzf ? bgzf_windows_loop() : windows_loop();
        else if (job.use_mirror) {
            for (size_t s = 0; s < n_segs && !bad.load(); s++) launch_segment((u64)s * kSegBytes, (u64)(s + 1) * kSegBytes, n);
        } else {
            // (a BGZF stream: the segments are the inflated text's, each behind the launches that decoded it; the decoder's
            // status word follows the last of them home, for verdict() to read before anything else)
            moved = tp.move(e, 0, n, S.text.as<char>(), blit, job.n_threads,
                            [&](u64 seg_begin, u64 seg_end, u64 avail) { launch_segment(seg_begin, seg_end, avail); }, &rc_open);
            if (!moved && tp.fetch_inflate_status(e, const_cast<u32 *>(h_inflate)) != YACRD_OK) moved = 1;
        }
        no_more = true;
        const double t_text_done = now_ms();
        wt.join();
        (void)hipStreamSynchronize(e->stream);
        od.quiet();
        if (stats) stats->text_ms = job.use_mirror ? 0.0f : (float)(t_text_done - t_table);
        if (!bad.load() && !moved) {
            for (size_t s = 0; s < n_segs; s++) {
                float ms = 0;
                if (hipEventElapsedTime(&ms, ev0[s], ev1[s]) == hipSuccess) kernel_ms += ms;
            }
        }
        return true;
    }

    // what the mover, the writer and the segments' status words say -> the return code and the stats
    int verdict(bool ran)
    {
        (void)hipGetLastError();
        if (!ran) return fail(YACRD_ENODEV, "overlap editor: a HIP stream or event could not be created");
        // the inflate's status word first: a text decoded from a member that was not taken may hold anything, and whatever the
        // kernels and the writer made of it (a refusal, a count, bytes already in the sink) says nothing
        if (h_inflate && *h_inflate) return inflate_not_taken(*h_inflate);
        if (rc_open) return rc_open;
        if (moved == 2) return fail(YACRD_EINVAL, "read error in the overlap file");
        if (moved == 3) return fail(YACRD_ENOMEM, "overlap text to HBM: no pinned memory");
        if (moved || bad.load() == 1) return fail(YACRD_ENODEV, "overlap editor: a HIP call failed");
        if (bad.load() == 2) return fail(YACRD_EINVAL, "Error during writing of the output file");
        u64 h_lines = 0, h_kept = 0, h_status = 0, h_bytes = 0;
        if (n_segs) {
            h_lines = h_seg[4 * (n_segs - 1)], h_kept = h_seg[4 * (n_segs - 1) + 1], h_status = h_seg[4 * (n_segs - 1) + 2];
            h_bytes = h_seg[4 * (n_segs - 1) + 3];
        }
        if (bad.load() == 3 || (h_status & yk::kEdNeedHost))
            return fail(YACRD_EFALLBACK, "the text holds a '\"', a CR, a line whose field count differs from the first line's or one that is "
                                         "megabytes long: the host loop decides");
        if (h_status) return fail(YACRD_EINTERNAL, "overlap editor: the mark and the pack pass disagree");
        if ((job.gzip ? out.text_bytes : sink.at) != h_bytes) return fail(YACRD_EINTERNAL, "overlap editor: fewer bytes written than kept");
        if (job.gzip && out.got != out.sent) return fail(YACRD_EINTERNAL, "overlap editor: a batch of members was not fetched");
        fill_gzip_stats(job.gzip_stats, out.text_bytes, sink.at, out.members, out.stored, od.kernel_ms(), out_busy_ms, out.put_ms);
        if (W) { // how the edit ran (yacrd_debug_edit_windows); the farthest reach lies in the control words behind the last pack
            u64 reach = 0;
            HIP_TRY(hipMemcpy(&reach, S.ctl.as<u64>() + 3, sizeof reach, hipMemcpyDeviceToHost));
            e->edit_windows[0] = n_segs, e->edit_windows[1] = reach;
            // (from the mirror: no text ring; BGZF in: the decoder's compressed slot and member slice count with the text ring)
            e->edit_windows[2] = S.wtext[0].cap + S.wtext[1].cap + (tp.bgzf ? inflate_window_held(e) : 0);
            e->edit_windows[3] = S.wout[0].cap + S.wout[1].cap;
        }
        if (stats) {
            stats->text_bytes = n;
            stats->kept_bytes = h_bytes;
            stats->n_lines = h_lines;
            stats->n_kept = h_kept;
            stats->table_ms = (float)(t_table - t_start);
            stats->kernel_ms = kernel_ms;
            stats->out_ms = (float)out_busy_ms;
            stats->mirror_reused = job.use_mirror ? 1u : 0u;
        }
        return YACRD_OK;
    }
};

int run_edit(yacrd_engine *e, const EditJob &job, TextProducer &tp, u64 n, Sink &sink, yacrd_edit_stats *stats)
{
    DeviceGuard guard(e->device);
    EditScratch *S = scratch_of<EditScratch>(e);
    if (!S) return fail(YACRD_ENOMEM, "host allocation failed");
    for (u64 &w : e->edit_windows) w = 0;
    EditRun r{e, job, tp, n, sink, stats, *S};
    if (const int rc = r.plan()) return rc;
    if (const int rc = r.reserve()) return rc;
    if (const int rc = r.upload_table()) return rc;
    return r.verdict(r.run());
}

int edit_args(yacrd_engine *e, int op, const yacrd_type_table *types, yacrd_edit_stats *stats);

// ---- what every form shares: where the output goes --------------------------------------------------------------------------
// memory: the kept bytes are at most the text and its added newline; members start at a quarter of the text (PAF text shrinks
// to about that) and grow
int edit_to_mem(yacrd_engine *e, const EditJob &job, TextProducer &tp, u64 n, char **out, uint64_t *out_bytes, yacrd_edit_stats *es)
{
    Sink sink;
    if (job.gzip) sink.cap = (size_t)(n / 4 + 4096);
    sink.mem = (char *)std::malloc(job.gzip ? (size_t)sink.cap : (size_t)n + 2);
    if (!sink.mem) return fail(YACRD_ENOMEM, "host allocation failed");
    const int rc = run_edit(e, job, tp, n, sink, es);
    if (rc != YACRD_OK) { // (kept bytes or members of earlier segments may lie in the buffer: it goes)
        std::free(sink.mem);
        return rc;
    }
    *out = sink.mem, *out_bytes = sink.at;
    return YACRD_OK;
}
// a file: written beside its place and moved there when every byte (gzip out: the EOF member) is in it — a text that turns out
// not to be for this path (a later segment may say so, with earlier ones already written) leaves nothing behind
int edit_to_file(yacrd_engine *e, const EditJob &job, TextProducer &tp, u64 n, const char *out_path, yacrd_edit_stats *es)
{
    struct stat ost;
    if (lstat(out_path, &ost) == 0 && !S_ISREG(ost.st_mode)) return fail(YACRD_EFALLBACK, "the output is not a regular file: the host loop writes it");
    yseg::BesideFile file;
    if (!file.open(out_path)) return fail(YACRD_EFALLBACK, std::string("cannot create a file beside ") + out_path + ": the host loop words the error");
    Sink sink;
    sink.fd = file.fd;
    int rc = run_edit(e, job, tp, n, sink, es);
    if (rc == YACRD_OK && !file.commit()) rc = fail(YACRD_EINVAL, "Error during writing of the output file");
    return rc;
}

// One call of the _bgzf_ forms (out_path, or out and out_bytes): the walk on the host, everything else on the device
int edit_bgzf(yacrd_engine *e, int op, const char *bgzf, uint64_t n_bytes, int format, const yacrd_type_table *types, int gzip_out, const char *out_path,
              char **out, uint64_t *out_bytes, yacrd_edit_stats *es, yacrd_gzip_stats *gs, yacrd_gunzip_stats *us)
{
    if (gs) std::memset(gs, 0, sizeof(*gs));
    if (us) std::memset(us, 0, sizeof(*us));
    if (out) *out = nullptr;
    if (out_bytes) *out_bytes = 0;
    if (const int rca = edit_args(e, op, types, es)) return rca;
    if ((!bgzf && n_bytes) || (!out_path && (!out || !out_bytes))) return fail(YACRD_EINVAL, "null argument");
    if (gzip_out != 0 && gzip_out != 1) return fail(YACRD_EINVAL, "gzip_out: 0 = the kept bytes, 1 = a BGZF stream of them");
    EditJob job;
    job.op = op, job.types = types, job.gzip = gzip_out == 1, job.gzip_stats = gzip_out == 1 ? gs : nullptr;
    if (const int rcf = overlap_format(nullptr, format, job.m4)) return rcf;
    BgzfIn in;
    if (const int rcw = in.walk(bgzf, n_bytes)) return rcw;
    TextProducer tp;
    tp.bgzf = &in;
    int rc = out_path ? edit_to_file(e, job, tp, in.text_bytes, out_path, es) : edit_to_mem(e, job, tp, in.text_bytes, out, out_bytes, es);
    {
        DeviceGuard guard(e->device);
        (void)hipStreamSynchronize(e->stream); // (whatever failed: nothing of this call is in flight when its events go)
        (void)hipGetLastError();
        if (rc == YACRD_OK) in.stats(us);
    }
    if (rc != YACRD_OK) {
        if (es) std::memset(es, 0, sizeof(*es));
        if (gs) std::memset(gs, 0, sizeof(*gs));
    }
    return rc;
}

// One call of the _resident_ forms: the text the engine's last successful overlap ingest left in HBM, nothing goes up
int edit_resident(yacrd_engine *e, int op, const yacrd_type_table *types, int gzip_out, const char *out_path, char **out, uint64_t *out_bytes,
                  yacrd_edit_stats *es, yacrd_gzip_stats *gs)
{
    if (gs) std::memset(gs, 0, sizeof(*gs));
    if (out) *out = nullptr;
    if (out_bytes) *out_bytes = 0;
    if (const int rca = edit_args(e, op, types, es)) return rca;
    if (!out_path && (!out || !out_bytes)) return fail(YACRD_EINVAL, "null argument");
    if (gzip_out != 0 && gzip_out != 1) return fail(YACRD_EINVAL, "gzip_out: 0 = the kept bytes, 1 = a BGZF stream of them");
    if (!e->mirror.valid || !e->mirror.p)
        return fail(YACRD_EINVAL, "no overlap text is resident: the engine's last ingest was no one-engine overlap ingest that succeeded");
    if (!e->mirror.facts) // (the ingest could not say what the plan asks: a first line beyond the BGZF sample, a read error)
        return fail(YACRD_EFALLBACK, "the resident text's first line could not be sampled at ingest time: the host loop words the error");
    EditJob job;
    job.op = op, job.types = types, job.gzip = gzip_out == 1, job.gzip_stats = gzip_out == 1 ? gs : nullptr;
    job.m4 = e->mirror.m4, job.use_mirror = job.resident = true;
    TextProducer tp; // (never asked: the mirror is walked)
    int rc = out_path ? edit_to_file(e, job, tp, e->mirror.n, out_path, es) : edit_to_mem(e, job, tp, e->mirror.n, out, out_bytes, es);
    if (rc != YACRD_OK) {
        if (es) std::memset(es, 0, sizeof(*es));
        if (gs) std::memset(gs, 0, sizeof(*gs));
    }
    return rc;
}

int edit_args(yacrd_engine *e, int op, const yacrd_type_table *types, yacrd_edit_stats *stats)
{
    if (!e || !types) return fail(YACRD_EINVAL, "null argument");
    if (op != 1 && op != 2) return fail(YACRD_EINVAL, "op: 1 = filter, 2 = extract");
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (e->pending.active || e->host_pending) return fail(YACRD_EINVAL, "the engine has a submitted batch pending");
    return YACRD_OK;
}

} // namespace

extern "C" {

int yacrd_engine_edit_overlaps(yacrd_engine *e, int op, const char *in_path, const char *out_path, int format, int n_threads,
                               const yacrd_type_table *types, yacrd_edit_stats *stats)
{
    if (const int rca = edit_args(e, op, types, stats)) return rca;
    if (!in_path || !out_path) return fail(YACRD_EINVAL, "null argument");
    EditJob job;
    job.op = op, job.n_threads = n_threads, job.types = types;
    if (const int rcf = overlap_format(in_path, format, job.m4)) return rcf;
    const int fd = ::open(in_path, O_RDONLY);
    if (fd < 0) return fail(YACRD_EFALLBACK, std::string("cannot open ") + in_path + ": the host loop words the error");
    FdGuard fdg{fd};
    struct stat st, ost;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) return fail(YACRD_EFALLBACK, "not a regular file: the host loop reads it");
    if (is_compressed_magic(fd)) return fail(YACRD_EFALLBACK, "a compressed file: the host loop inflates it and deflates what it keeps");
    // the output: written beside its place and moved there when every byte is in it (edit_to_file) — a text that turns out not
    // to be for this path (the last segment may say so) leaves nothing behind.  Anything but a new or a regular file is the host
    // loop's, and so is a regular one that is the input
    if (lstat(out_path, &ost) == 0 && S_ISREG(ost.st_mode) && ost.st_dev == st.st_dev && ost.st_ino == st.st_ino)
        return fail(YACRD_EFALLBACK, "input and output are one file: the host loop's case");
    // (a mirror that did not come from a file has no identity: it never matches one)
    job.use_mirror = e->mirror.valid && e->mirror.from_file && e->mirror.p && e->mirror.n == (u64)st.st_size && e->mirror.dev == (u64)st.st_dev &&
                     e->mirror.ino == (u64)st.st_ino && e->mirror.mtime_s == (int64_t)st.st_mtim.tv_sec &&
                     e->mirror.mtime_ns == (int64_t)st.st_mtim.tv_nsec;
    TextProducer tp;
    tp.src.fd = fd;
    return edit_to_file(e, job, tp, (u64)st.st_size, out_path, stats);
}

int yacrd_engine_edit_overlaps_mem(yacrd_engine *e, int op, const char *text, uint64_t n, int format, const yacrd_type_table *types,
                                   char **out, uint64_t *out_bytes, yacrd_edit_stats *stats)
{
    if (const int rca = edit_args(e, op, types, stats)) return rca;
    if ((!text && n) || !out || !out_bytes) return fail(YACRD_EINVAL, "null argument");
    *out = nullptr, *out_bytes = 0;
    EditJob job;
    job.op = op, job.types = types;
    if (const int rcf = overlap_format(nullptr, format, job.m4)) return rcf;
    TextProducer tp;
    tp.src.mem = text ? text : "";
    return edit_to_mem(e, job, tp, n, out, out_bytes, stats);
}

int yacrd_engine_edit_overlaps_gzip_mem(yacrd_engine *e, int op, const char *text, uint64_t n, int format, const yacrd_type_table *types,
                                        char **out, uint64_t *out_bytes, yacrd_edit_stats *es, yacrd_gzip_stats *gs)
{
    if (gs) std::memset(gs, 0, sizeof(*gs));
    if (const int rca = edit_args(e, op, types, es)) return rca;
    if ((!text && n) || !out || !out_bytes) return fail(YACRD_EINVAL, "null argument");
    *out = nullptr, *out_bytes = 0;
    EditJob job;
    job.op = op, job.types = types, job.gzip = true, job.gzip_stats = gs;
    if (const int rcf = overlap_format(nullptr, format, job.m4)) return rcf;
    TextProducer tp;
    tp.src.mem = text ? text : "";
    const int rc = edit_to_mem(e, job, tp, n, out, out_bytes, es);
    if (rc != YACRD_OK && gs) std::memset(gs, 0, sizeof(*gs));
    return rc;
}

int yacrd_engine_edit_overlaps_gzip_file(yacrd_engine *e, int op, const char *text, uint64_t n, int format, const yacrd_type_table *types,
                                         const char *out_path, yacrd_edit_stats *es, yacrd_gzip_stats *gs)
{
    if (gs) std::memset(gs, 0, sizeof(*gs));
    if (const int rca = edit_args(e, op, types, es)) return rca;
    if ((!text && n) || !out_path) return fail(YACRD_EINVAL, "null argument");
    EditJob job;
    job.op = op, job.types = types, job.gzip = true, job.gzip_stats = gs;
    if (const int rcf = overlap_format(nullptr, format, job.m4)) return rcf;
    TextProducer tp;
    tp.src.mem = text ? text : "";
    const int rc = edit_to_file(e, job, tp, n, out_path, es);
    if (rc != YACRD_OK && gs) std::memset(gs, 0, sizeof(*gs));
    return rc;
}

int yacrd_engine_edit_overlaps_bgzf_mem(yacrd_engine *e, int op, const char *bgzf, uint64_t n_bytes, int format, const yacrd_type_table *types,
                                        int gzip_out, char **out, uint64_t *out_bytes, yacrd_edit_stats *es, yacrd_gzip_stats *gs, yacrd_gunzip_stats *us)
{
    if (!out || !out_bytes) return fail(YACRD_EINVAL, "null argument");
    return edit_bgzf(e, op, bgzf, n_bytes, format, types, gzip_out, nullptr, out, out_bytes, es, gs, us);
}

int yacrd_engine_edit_overlaps_bgzf_file(yacrd_engine *e, int op, const char *bgzf, uint64_t n_bytes, int format, const yacrd_type_table *types,
                                         int gzip_out, const char *out_path, yacrd_edit_stats *es, yacrd_gzip_stats *gs, yacrd_gunzip_stats *us)
{
    if (!out_path) return fail(YACRD_EINVAL, "null argument");
    return edit_bgzf(e, op, bgzf, n_bytes, format, types, gzip_out, out_path, nullptr, nullptr, es, gs, us);
}

int yacrd_engine_edit_overlaps_resident_mem(yacrd_engine *e, int op, const yacrd_type_table *types, int gzip_out, char **out, uint64_t *out_bytes,
                                            yacrd_edit_stats *es, yacrd_gzip_stats *gs)
{
    if (!out || !out_bytes) return fail(YACRD_EINVAL, "null argument");
    return edit_resident(e, op, types, gzip_out, nullptr, out, out_bytes, es, gs);
}

int yacrd_engine_edit_overlaps_resident_file(yacrd_engine *e, int op, const yacrd_type_table *types, int gzip_out, const char *out_path,
                                             yacrd_edit_stats *es, yacrd_gzip_stats *gs)
{
    if (!out_path) return fail(YACRD_EINVAL, "null argument");
    return edit_resident(e, op, types, gzip_out, out_path, nullptr, nullptr, es, gs);
}

void yacrd_edit_text_free(char *p) { std::free(p); }

int yacrd_debug_edit_window(yacrd_engine *e, uint64_t window_bytes)
{
    if (!e) return fail(YACRD_EINVAL, "null argument");
    e->edit_window = window_bytes;
    return YACRD_OK;
}
void yacrd_debug_edit_windows(const yacrd_engine *e, uint64_t out[4])
{
    for (int i = 0; i < 4; i++) out[i] = e ? e->edit_windows[i] : 0;
}

} // extern "C"
