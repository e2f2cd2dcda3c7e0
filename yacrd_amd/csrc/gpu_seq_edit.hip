// gpu_seq_edit.hip — scrubb / split / filter / extract on a FASTQ or FASTA file with the decision, the sizing and the gather on the GPU
// (include/yacrd_engine.h: yacrd_engine_edit_fastq, yacrd_engine_edit_fasta).  One pipeline with a format plugged in: the
// mover, the line index, the id table, the op's rule (seq_verdict), the plan and copy kernels (seq_plan_kernel<Format, EMIT>,
// seq_copy_kernel<Format>), the way home and the deflate step know no format.  A format is a struct — Fastq, Fasta — with its
// kernel arguments (SeqArgs and what is its own), its piece descriptor, record<EMIT>() (where a record's lines lie, its
// canonical form, name, key, description and byte arithmetic), at() (byte k of a piece) and a per-thread cursor; on the host,
// its front in SeqRun::size_output (what numbers the records) and its message.  The stages are told for FASTQ here; what
// FASTA does otherwise stands in front of its kernels below.
//
// Reference: Scrubbing::run (src/editor/scrubbing.rs:156-236), Split::run (src/editor/split.rs), Filter::run and Extract::run on
// sequence files: a record's key — the first whitespace token of its name — is looked up in the bad-part table (an id it does not
// hold is NotBad with no region, src/stack.rs:164-169); filter copies a NotBad record, extract any other; scrubb and split drop
// NotCovered reads, copy a read with no region (scrubb) or a NotBad one (split) and cut every other at its regions: one read
// becomes several records `@{name}_{p0}_{p1}[ {desc}]` with that slice of the sequence and of the quality.  The host loop
// (host/editors.cc: edit_sequences, FASTQ branch; cut_positions) defines the bytes; here the host only MOVES the text
// (gpu_text.h: the parser's mover) and the output.  On the device:
//   table    the reads' names, lengths, types and region CSR uploaded once; the id table of edit_table.h over the names
//   lines    per segment as it lands: the newlines of every 32 KiB tile, and whether a CR lies in it
//   scan     the tiles' line counts (stream.hip's device-wide scan): the index of every tile's first newline
//   index    every tile writes the offsets of its newlines to line_end[]: record r is lines 4r .. 4r + 3 — nothing is guessed,
//            a quality line that begins with '@' is just line 4r + 3
//   plan     a thread per record: the canonical form checked, the key found and looked up, the op's rule applied, the
//            record's output pieces and bytes counted
//   scans    of the pieces and of the bytes
//   pieces   a thread per record writes its piece descriptors at their scanned places
//   copy     a workgroup per 4 KiB tile of the OUTPUT: a thread finds the piece that covers its first byte by binary search and
//            walks on from there; every 4-byte word of the tile is composed in LDS — header bytes formatted, text bytes fetched
//            with aligned 4-byte loads (neighbouring lanes read neighbouring words) — and the tile is stored with 16-byte stores;
//            the bytes stored are counted, a total that differs from the scan's is YACRD_EINTERNAL
// In the whole-text run index, plan, pieces and copy wait for the last segment of text, and the text and the whole output lie in
// HBM.  A FASTQ or FASTA of more than one window whose text comes from a file or from host memory may instead run WINDOW BY
// WINDOW (SeqRun::run_windows): the same kernels on bytes [lo, hi) of a text slot, a carry kernel between windows, two
// text slots and two output slots, a writer thread on the way out; always where the whole text finds no room.
// What the path does not take — a CR, a line count that is no multiple of four, a header without '@' or without a name, a
// "@name \n", a '+' line that is not bare, sequence and quality of different lengths, a cut position beyond the read, a region
// with begin > end — comes back as YACRD_EFALLBACK with nothing written: the caller runs the host loop.
//
// gzip out (yacrd_engine_edit_fastq_gzip_mem / _file): the finished output buffer goes through gpu_deflate.hip's
// device-resident step, batch by batch (a batch begins on a multiple of 65 280 bytes: the encoder's 16-byte loads stay
// aligned); one batch comes home while the next is encoded.  Blocks are counted from byte 0 of the output, so the stream is
// yacrd_engine_gzip_mem's for the same bytes.
//
// BGZF in (yacrd_engine_edit_fastq_bgzf_mem / _file): the compressed file crosses the link through the same mover into the
// inflate scratch's buffer, gpu_inflate.hip's device-resident step inflates its members into the text buffer, and the run goes
// on from `lines` as above.  The text's last byte, which the other forms read from the host's copy, comes back from the device
// behind the inflate, with the decoder's status word.
#include "engine_internal.h"
#include "gpu_text.h"
#include "edit_table.h"
#include "bgzf_walk.h"
#include "bgzf_windows.h"
#include "gpu_out.h"
#include "host/beside_file.h"

#include <cstdio>
#include <cstdlib>
#include <deque>
#include <initializer_list>
#include <mutex>
#include <type_traits>

using namespace yke;

namespace yk {

constexpr u32 kSqNeedHost = 1u;
constexpr u32 kSqCarryLong = 2u;      // status: what a window leaves for the next one is longer than a window (sq_carry_kernel)
constexpr int kSqOutTile = kGpT * 16; // bytes of output per workgroup of the copy pass
constexpr u32 kSqCopy = 1u;           // SqPiece::flags: the record as it stands in the text
constexpr u32 kSqRaw = 2u;            // ... bytes [rec, rec + len) of SqArgs::raw, not of the text: the output tail of the window before
constexpr u64 kSqMaxRecord = 0xFF000000ull; // bytes of a record, of a piece: offsets inside them are u32

struct SqPiece { // one record of the output
    u64 out;     // where its first byte goes
    u64 rec;     // the input record's '@'
    u32 len;     // its bytes
    u32 flags;
    u32 name_len, desc_len;
    u32 seq_rel, qual_rel; // the record's sequence / quality line, from `rec`
    u32 p0, p1;
};
static_assert(sizeof(SqPiece) == 48, "host code sizes the piece buffer by this");

struct SeqArgs { // what the kernels of both formats read; SqArgs and FaArgs (below) add what is theirs
    const unsigned char *text;
    EdTable tab;
    const u32 *lengths;  // [n_reads]
    const u64 *bad_off;  // [n_reads + 1]
    const u32 *bad_reg;  // [2 * regions]
    u64 *line_end;       // [n_lines]: where every newline lies
    u64 n_lines, n_rec;
    u32 *rec_pieces, *rec_bytes;        // per record: output records, output bytes
    const u64 *piece_off, *byte_off;    // their exclusive scans
    u64 n_pieces, total;                // output records, output bytes
    unsigned char *out;
    unsigned long long *ctl; // [0] status, [1] bytes the copy pass stored
    u32 op;
    u64 lo;    // the text's first byte: 0, or where a window's carry begins in its slot (what lies below is stale)
    // a window of a gzip run (run_windows): piece 0 is `out0` bytes at `raw`, the records' pieces and bytes lie behind it
    const unsigned char *raw;
    u64 out0;   // bytes of the output slot in front of the first record's
    u32 piece0; // pieces in front of the first record's (0 or 1)
};

struct SqArgs : SeqArgs {
    u64 n;     // bytes of text
    u64 avail; // bytes [0, avail) have landed (== n for the last segment)
    u32 *tile_nl;        // per text tile: its newlines
    const u64 *tile_l0;  // their exclusive scan
    u32 tile0;           // the launch's first text tile
    SqPiece *pieces;
};
static_assert(std::is_trivially_copyable<SqArgs>::value, "a kernel argument by value");

// a thread's status bits -> ctl[0]: ORed over the wavefront, one atomic from lane 0
__device__ __forceinline__ void seq_status(unsigned long long *ctl, u32 status)
{
    status = wave_or(status);
    if (status && lane_id() == 0) atomicOr(ctl, (unsigned long long)status);
}

// the tile's newline masks (a u16 per 16 bytes) -> nlm; returns the thread's newline count and ORs a CR into `cr`.  The
// mirror is padded by 64 zero bytes and the last step is clipped to whole 16-byte pieces inside it; an inner segment's
// `avail` is a chunk boundary.  A byte below a.lo gives no bit: a piece wholly below it is not loaded, the one it cuts is masked.
__device__ __forceinline__ u32 sq_stage(const SqArgs &a, u64 tile0, unsigned short *nlm, u32 &cr)
{
    const u64 lim = a.avail == a.n ? ((a.n + 63) & ~(u64)15) : a.avail;
    u32 cnt = 0;
    for (u32 i = threadIdx.x * 16u; i < (u32)kGpTile; i += (u32)kGpT * 16u) {
        u32 nlb = 0;
        const u64 at = tile0 + i;
        if (at < lim && at + 16u > a.lo) {
            const uint4 v = *reinterpret_cast<const uint4 *>(a.text + at);
            const u32 keep = at < a.lo ? ~0u << (u32)(a.lo - at) : ~0u;
            nlb = gp_eq16(v, '\n') & keep;
            cr |= gp_eq16(v, '\r') & keep;
        }
        if (nlm) nlm[i >> 4] = (unsigned short)nlb;
        cnt += (u32)__popc(nlb);
    }
    return cnt;
}

// ---- lines: the newlines of every tile of a segment, a CR anywhere -----------------------------------------------------------
__global__ __launch_bounds__(kGpT) void sq_lines_kernel(SqArgs a)
{
    __shared__ u32 sw[kGpT / 64];
    const u32 gt = a.tile0 + blockIdx.x;
    u32 cr = 0;
    const u32 cnt = sq_stage(a, (u64)gt * (u64)kGpTile, nullptr, cr);
    seq_status(a.ctl, cr ? kSqNeedHost : 0u);
    const u32 tot = block_add<kGpT>(cnt, sw);
    if (threadIdx.x == 0) a.tile_nl[gt] = tot;
}

// ---- index: where every newline lies, in line order ----------------------------------------------------------------------------
__global__ __launch_bounds__(kGpT) void sq_index_kernel(SqArgs a)
{
    __shared__ __attribute__((aligned(16))) unsigned short nlm[kGpTile / 16];
    __shared__ u32 sw[kGpT / 64];
    const u32 gt = a.tile0 + blockIdx.x;
    const u64 tile0 = (u64)gt * (u64)kGpTile;
    u32 cr = 0;
    (void)sq_stage(a, tile0, nlm, cr);
    __syncthreads();
    const uint4 q = *reinterpret_cast<const uint4 *>(nlm + threadIdx.x * 8u);
    u64 m[2] = {(u64)q.x | ((u64)q.y << 32), (u64)q.z | ((u64)q.w << 32)};
    u32 tot = 0;
    const u32 at = block_excl_add<kGpT>((u32)__popcll(m[0]) + (u32)__popcll(m[1]), sw, tot);
    u64 g = a.tile_l0[gt] + at;
    const u64 lo = tile0 + (u64)threadIdx.x * 128u;
#pragma unroll
    for (int h = 0; h < 2; h++)
        while (m[h]) {
            const u32 bit = (u32)__builtin_ctzll(m[h]);
            m[h] &= m[h] - 1;
            if (g < a.n_lines) a.line_end[g] = lo + (u64)h * 64u + bit; // (the two passes count alike: always)
            g++;
        }
}

__device__ __forceinline__ u32 sq_digits(u32 v)
{
    u32 d = 1;
    while (v >= 10u) v /= 10u, d++;
    return d;
}
// digit k (from the left) of v, which has nd digits
__device__ __forceinline__ u32 sq_digit_at(u32 v, u32 nd, u32 k)
{
    for (u32 i = nd - 1u - k; i; i--) v /= 10u;
    return '0' + v % 10u;
}

// The cut pieces of a read, in order (host/editors.cc: cut_positions and the loop behind it): scrubb takes every region, a
// leading (0, 0) pair is skipped and `len` closes the list unless it is its last element already — then the odd element is
// ignored —; split takes the regions that touch neither end.  f(p0, p1) returns false to stop.
template <class F>
__device__ __forceinline__ void sq_cuts(u32 op, const u32 *reg, u32 n, u32 len, F &&f)
{
    u32 p0 = 0;
    if (op == 0u) {
        for (u32 i = 0; i < n; i++) {
            const u32 b = reg[2 * i], e = reg[2 * i + 1];
            if (!(i == 0 && b == 0u) && !f(p0, b)) return;
            p0 = e;
        }
        if (p0 != len) (void)f(p0, len);
    } else {
        for (u32 i = 0; i < n; i++) {
            const u32 b = reg[2 * i], e = reg[2 * i + 1];
            if (b == 0u || e == len) continue;
            if (!f(p0, b)) return;
            p0 = e;
        }
        (void)f(p0, len);
    }
}

// ---- what becomes of a record: the one place that knows the op's rule -----------------------------------------------------------
enum : u32 { kSeqDrop = 0, kSeqCopy = 1, kSeqCut = 2 };
struct SeqVerdict {
    u32 what;           // kSeqDrop, kSeqCopy: the record as it stands; kSeqCut: at the read's regions
    u32 type, n_reg, len; // the read's type, regions and length: zeros for an id the table does not hold
    const u32 *reg;
};
// the read named text[key, key + key_len): filter copies a NotBad record, extract any other; scrubb and split drop NotCovered
// reads, copy a read with no region (scrubb) or a NotBad one (split) and cut every other
__device__ __forceinline__ SeqVerdict seq_verdict(const SeqArgs &a, u64 key, u32 key_len)
{
    SeqVerdict v{};
    const u32 read = ed_find(a.tab, GpBytes{a.text}, key, key_len);
    if (read != kEdNoRead) {
        v.type = a.tab.type[read];
        const u64 o = a.bad_off[read];
        v.n_reg = (u32)(a.bad_off[read + 1] - o);
        v.reg = a.bad_reg + 2 * o;
        v.len = a.lengths[read];
    }
    if (a.op == 1u) v.what = v.type == 0u ? kSeqCopy : kSeqDrop;
    else if (a.op == 2u) v.what = v.type != 0u ? kSeqCopy : kSeqDrop;
    else if (v.type == 2u) v.what = kSeqDrop;
    else v.what = (a.op == 0u ? v.n_reg == 0u : v.type == 0u) ? kSeqCopy : kSeqCut;
    return v;
}

// Record r, of seq_len bases, cut: piece(p0, p1, k, at) answers the bytes of output record k, which begins `at` bytes into
// what the record becomes, and (EMIT) writes its descriptor.  EMIT false: the pieces and their bytes counted.
template <bool EMIT, class P>
__device__ __forceinline__ u32 seq_cut(const SeqArgs &a, u64 r, const SeqVerdict &v, u32 seq_len, P &&piece)
{
    u32 status = 0, pieces = 0;
    u64 bytes = 0;
    sq_cuts(a.op, v.reg, v.n_reg, v.len, [&](u32 p0, u32 p1) {
        if (p0 > seq_len || p1 > seq_len || p0 > p1) { // (the host prints the reference's [ERROR] line, or fails: its case)
            status = kSqNeedHost;
            return false;
        }
        const u64 plen = piece(p0, p1, pieces, bytes);
        pieces++, bytes += plen;
        return true;
    });
    if (bytes >= kSqMaxRecord) status = kSqNeedHost;
    if (!EMIT && !status) a.rec_pieces[r] = pieces, a.rec_bytes[r] = (u32)bytes;
    return status;
}

// ---- plan / pieces: a thread per record.  Format::record<EMIT>(a, r): the record's lines found, its canonical form checked,
// its verdict, its pieces; EMIT false: the pieces and bytes counted; true: the piece descriptors written.  Returns the status bits.
template <class Format, bool EMIT>
__global__ __launch_bounds__(256) void seq_plan_kernel(typename Format::Args a)
{
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    seq_status(a.ctl, r < a.n_rec ? Format::template record<EMIT>(a, r) : 0u);
}

// four bytes of one run of text: the aligned words that hold them (the word behind begins inside the run when it is read)
__device__ __forceinline__ u32 sq_load4(const unsigned char *src)
{
    const uintptr_t ad = reinterpret_cast<uintptr_t>(src);
    const u32 *al = reinterpret_cast<const u32 *>(ad & ~(uintptr_t)3);
    const u32 sh = (u32)(ad & 3u) * 8u;
    u32 word = al[0];
    if (sh) word = (word >> sh) | (al[1] << (32u - sh));
    return word;
}

// ---- carry: what a window leaves behind its last whole record -> the front of the next window's slot ---------------------------
// Window k's text is bytes [lo, hi) of its slot; its n_rec whole records end at line_end[4 n_rec - 1] (FASTQ; FASTA: in front
// of the window's last header line, fa_carry_kernel).  The bytes behind them,
// [cb, hi), are moved to end at offset W of the next slot — in front of the new bytes, which land at W whatever the carry's
// length turns out to be.  Every thread reads cb itself; thread 0 reports the length and sets kSqCarryLong when the carry
// area (W bytes) does not hold it: nothing is moved then.  The destination's end is 16-byte aligned, so the move is whole
// aligned 16-byte stores and bytes in the first, cut piece; a piece is loaded with one 16-byte load when source and
// destination are aligned alike, else as four words put together from aligned 4-byte loads (sq_load4: at most 7 bytes
// behind hi are read, inside the slot's 64 bytes of padding).  The two slots are different buffers: nothing overlaps.
struct SqCarry {
    const u64 *line_end;
    u64 n_rec, lo, hi, W;
    const unsigned char *src; // this window's slot
    unsigned char *dst;       // the next window's
    unsigned long long *ctl;  // [0] status, [2] the carry's bytes
};
// the move, from the carry's first byte on: the format's kernel says where that is
__device__ __forceinline__ void sq_carry_from(const SqCarry &c, const u64 cb)
{
    const u64 len = c.hi - cb;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        c.ctl[2] = len;
        if (len > c.W) atomicOr(c.ctl, (unsigned long long)kSqCarryLong);
    }
    if (len > c.W) return;
    const u64 d0 = c.W - len;
    const unsigned char *from = c.src + cb - d0; // (byte o of the destination is from[o], d0 <= o < W)
    const bool alike = ((cb ^ d0) & 15u) == 0;
    for (u64 q = (d0 >> 4) + (u64)blockIdx.x * 256u + threadIdx.x; q < (c.W >> 4); q += (u64)gridDim.x * 256u) {
        const u64 o = q << 4;
        if (o < d0) { // the piece the carry's first byte cuts
            for (u64 b = d0; b < o + 16u; b++) c.dst[b] = from[b];
            continue;
        }
        uint4 v;
        if (alike) v = *reinterpret_cast<const uint4 *>(from + o);
        else v = make_uint4(sq_load4(from + o), sq_load4(from + o + 4), sq_load4(from + o + 8), sq_load4(from + o + 12));
        *reinterpret_cast<uint4 *>(c.dst + o) = v;
    }
}
__global__ __launch_bounds__(256) void sq_carry_kernel(SqCarry c) { sq_carry_from(c, c.n_rec ? c.line_end[4 * c.n_rec - 1] + 1 : c.lo); }

// the composed tile -> the output, 16 bytes per thread; the bytes the workgroup composed -> ctl[1], one add per workgroup
__device__ __forceinline__ void sq_store_tile(unsigned char *out, u64 total, unsigned long long *ctl, const u32 *tile, u32 *sw, u64 tile0, u32 stored)
{
    __syncthreads();
    const u64 o = tile0 + (u64)threadIdx.x * 16u;
    if (o < total) *reinterpret_cast<uint4 *>(out + o) = *reinterpret_cast<const uint4 *>(tile + threadIdx.x * 4u);
    const u32 tot = block_add<kGpT>(stored, sw);
    if (threadIdx.x == 0) atomicAdd(ctl + 1, (unsigned long long)tot);
}

// ---- copy: a tile of the output, composed in LDS, stored 16 bytes wide -----------------------------------------------------------
// Thread t composes words t, t + 256, t + 512 and t + 768 of the tile, so that a wavefront's loads from a run of text are
// consecutive words; it then stores bytes [16 t, 16 t + 16).  The output buffer is padded to whole 16-byte pieces (the
// bytes behind the total are zeros).  Format::at(a, p, k, cursor, src, rem, lit): byte k of piece p is a byte of the text (src,
// with `rem` bytes of the same run behind it) or a formatted one (lit, src null); a word takes the aligned path when its four
// bytes lie in one run.  The cursor is the thread's own between calls and is reset when the piece advances.
template <class Format>
__global__ __launch_bounds__(kGpT) void seq_copy_kernel(typename Format::Args a)
{
    __shared__ __attribute__((aligned(16))) u32 tile[kSqOutTile / 4];
    __shared__ u32 sw[kGpT / 64];
    const u64 tile0 = (u64)blockIdx.x * (u64)kSqOutTile;
    u32 stored = 0;
    u64 pi = 0;
    typename Format::Piece p{};
    typename Format::Cursor cur{};
    bool have = false;
#pragma unroll 1
    for (u32 w = 0; w < 4u; w++) {
        const u64 j = tile0 + ((u64)w * (u32)kGpT + threadIdx.x) * 4u;
        u32 word = 0;
        if (j < a.total) {
            if (!have) { // the last piece that begins at or in front of j (piece 0 begins at 0)
                u64 lo = 0, hi = a.n_pieces;
                while (hi - lo > 1) {
                    const u64 mid = lo + (hi - lo) / 2;
                    if (a.pieces[mid].out <= j) lo = mid;
                    else hi = mid;
                }
                pi = lo, p = a.pieces[lo], have = true;
            }
            const u32 nb = (u32)min((u64)4, a.total - j);
            for (u32 b = 0; b < nb;) {
                const u64 jj = j + b;
                while (jj >= p.out + p.len && pi + 1 < a.n_pieces) p = a.pieces[++pi], cur.reset(); // (jj < total: there is such a piece)
                const unsigned char *src;
                u32 rem, lit;
                Format::at(a, p, (u32)(jj - p.out), cur, src, rem, lit);
                if (src && b == 0 && rem >= 4u) { // four bytes of one run: the aligned words that hold them
                    word = sq_load4(src);
                    b = 4, stored += 4;
                } else {
                    word |= (src ? (u32)*src : lit) << (8u * b);
                    b++, stored++;
                }
            }
        }
        tile[w * (u32)kGpT + threadIdx.x] = word;
    }
    sq_store_tile(a.out, a.total, a.ctl, tile, sw, tile0, stored);
}

// ==== FASTQ: record r is lines 4r .. 4r + 3 ======================================================================================
struct Fastq {
    using Args = SqArgs;
    using Piece = SqPiece;
    struct Cursor { // (a piece's bytes are found from the piece alone)
        __device__ __forceinline__ void reset() {}
    };

    template <bool EMIT>
    static __device__ __forceinline__ u32 record(const SqArgs &a, u64 r)
    {
        const unsigned char *t = a.text;
        const u64 s = r ? a.line_end[4 * r - 1] + 1 : a.lo;
        const u64 e0 = a.line_end[4 * r], e1 = a.line_end[4 * r + 1], e2 = a.line_end[4 * r + 2], e3 = a.line_end[4 * r + 3];
        if (!EMIT) a.rec_pieces[r] = 0u, a.rec_bytes[r] = 0u;
        const u64 rec_len = e3 + 1 - s;
        if (rec_len >= kSqMaxRecord) return kSqNeedHost;
        if (t[s] != '@' || e0 == s + 1) return kSqNeedHost;
        u64 sp = e0, key_end = e0; // the first blank; the first whitespace of any kind in front of it
        for (u64 i = s + 1; i < e0; i++) {
            const u32 c = t[i];
            if (c == ' ') {
                sp = i;
                break;
            }
            if ((c == '\t' || c == '\x0c') && key_end == e0) key_end = i;
        }
        if (key_end > sp) key_end = sp;
        if (sp == s + 1 || sp + 1 == e0) return kSqNeedHost; // (no name; "@name \n": the writer drops the blank)
        if (e2 != e1 + 2 || t[e1 + 1] != '+') return kSqNeedHost;
        const u64 seq_len64 = e1 - e0 - 1;
        if (seq_len64 != e3 - e2 - 1) return kSqNeedHost;
        const u32 name_len = (u32)(sp - s - 1), desc_len = sp < e0 ? (u32)(e0 - sp - 1) : 0u;

        const SeqVerdict v = seq_verdict(a, s + 1, (u32)(key_end - s - 1));
        if (v.what == kSeqDrop) return 0u;
        if (v.what == kSeqCopy) {
            if (!EMIT) a.rec_pieces[r] = 1u, a.rec_bytes[r] = (u32)rec_len;
            else {
                SqPiece p{};
                p.out = a.out0 + a.byte_off[r], p.rec = s, p.len = (u32)rec_len, p.flags = kSqCopy;
                a.pieces[a.piece0 + a.piece_off[r]] = p;
            }
            return 0u;
        }
        const u32 head = 1u + name_len + (desc_len ? 1u + desc_len : 0u) + 1u;
        return seq_cut<EMIT>(a, r, v, (u32)seq_len64, [&](u32 p0, u32 p1, u32 k, u64 at) {
            const u64 plen = (u64)head + 2u + sq_digits(p0) + sq_digits(p1) + 2ull * (p1 - p0) + 4u;
            if (EMIT) {
                SqPiece p{};
                p.out = a.out0 + a.byte_off[r] + at, p.rec = s, p.len = (u32)plen, p.flags = 0u;
                p.name_len = name_len, p.desc_len = desc_len;
                p.seq_rel = (u32)(e0 + 1 - s), p.qual_rel = (u32)(e2 + 1 - s);
                p.p0 = p0, p.p1 = p1;
                a.pieces[a.piece0 + a.piece_off[r] + k] = p;
            }
            return plen;
        });
    }

    static SqPiece raw_piece(u64 at, u32 len) // (host) `len` bytes at `at` of SeqArgs::raw, first in the output
    {
        SqPiece p{};
        p.rec = at, p.len = len, p.flags = kSqRaw;
        return p;
    }

    static __device__ __forceinline__ void at(const SqArgs &a, const SqPiece &p, u32 k, Cursor &, const unsigned char *&src, u32 &rem, u32 &lit)
    {
        const unsigned char *rec = (p.flags & kSqRaw ? a.raw : a.text) + p.rec;
        if (p.flags & (kSqCopy | kSqRaw)) {
            src = rec + k, rem = p.len - k;
            return;
        }
        src = nullptr, rem = 1, lit = '\n';
        if (k == 0) {
            lit = '@';
            return;
        }
        k -= 1;
        if (k < p.name_len) {
            src = rec + 1 + k, rem = p.name_len - k;
            return;
        }
        k -= p.name_len;
        const u32 d0 = sq_digits(p.p0), d1 = sq_digits(p.p1);
        if (k < 2u + d0 + d1) {
            lit = k == 0 || k == d0 + 1u ? '_' : k <= d0 ? sq_digit_at(p.p0, d0, k - 1u) : sq_digit_at(p.p1, d1, k - d0 - 2u);
            return;
        }
        k -= 2u + d0 + d1;
        if (p.desc_len) {
            if (k == 0) {
                lit = ' ';
                return;
            }
            k -= 1;
            if (k < p.desc_len) {
                src = rec + 1 + p.name_len + 1 + k, rem = p.desc_len - k;
                return;
            }
            k -= p.desc_len;
        }
        if (k == 0) return; // the header's newline
        k -= 1;
        const u32 L = p.p1 - p.p0;
        if (k < L) {
            src = rec + p.seq_rel + p.p0 + k, rem = L - k;
            return;
        }
        k -= L;
        if (k < 3u) {
            lit = k == 1u ? '+' : '\n';
            return;
        }
        k -= 3u;
        if (k < L) src = rec + p.qual_rel + p.p0 + k, rem = L - k; // (else: the record's last newline)
    }
};

// ==== FASTA (yacrd_engine_edit_fasta) ===========================================================================================
// A record is a '>' line and every line up to the next one; its sequence is those lines without their newlines, and every
// record that goes out — copied or cut — is written again, 80 bases a line (host/editors.cc: next_fasta, write_fasta).  Behind
// the line index of the FASTQ path:
//   mark     a thread per line: head[g] (the line begins with '>'), bases[g] (0 for a header, else the line's length)
//   scans    head -> the record ordinal of every line; bases -> base_before[g], the bases of the whole text in front of line g
//   heads    rec_line[r] = the line of header r; a line with bases and no header in front of it is the host loop's error
//   widths   a thread per line: rec_width[r] = the one width of record r's lines, 0 when a line does not fit
//   plan     a thread per record: name, separator, description; the name looked up; the op's rule; pieces and bytes counted
//   pieces   the same walk writes the descriptors
//   copy     a workgroup per 4 KiB of the output: byte k of a body is row k / 81, column k % 81 — column 80 and the last byte
//            are newlines, every other byte is base p0 + 80 row + column of the record: the last line of the record whose
//            base_before is not beyond that base holds it.  A thread keeps the line it last read from, tries the one behind
//            it and searches what is left of the record otherwise (a walk forward from the tile's first search measured
//            slower: 3.22 against 2.93 ms); a record whose lines all have one width is addressed without the tables (fa_widths_kernel)
// In a window (run_windows) "the text" is the bytes of a slot from a.lo on and every table is the window's own: lines,
// ordinals and bases count from a.lo.  A window that is not the last has H header lines among its whole lines and completes
// n_rec = max(H - 1, 0) records: nothing in it says that the byte behind it is a '>', so its last record waits for the next
// window (fa_carry_kernel), and the kernels leave the lines of that record alone.  One thing can say so: a partial last line
// that begins with '>' (fa_mark_kernel reports it).  Then all H records are whole and only that line waits — without this a
// record of exactly a window's bytes with a '>' behind it would make a carry of more than a window, and "a record of at most
// a window is always taken" would not hold.
constexpr u32 kFaWidth = 80; // noodles::fasta::Writer's line

struct FaPiece { // one record of the output
    u64 out;     // where its first byte goes
    u64 hdr;     // the input record's '>'; kSqRaw: where the bytes lie in FaArgs::raw
    u64 base0;   // the ordinal, in the text (a window: from its first byte), of the record's first base
    u64 line0, line1; // the record's lines behind its header
    u32 len;     // its bytes
    u32 flags;   // kSqCopy: the whole record with its description; kSqRaw: bytes [hdr, hdr + len) of `raw`; else the piece [p0, p1) named name_p0_p1
    u32 name_len, desc_len;
    u32 p0, p1;
    u32 width;   // every line of the record but the last holds this many bases, the last 1 to `width`; 0: its lines differ
    u32 pad;
};
static_assert(sizeof(FaPiece) == 72, "host code sizes the piece buffer by this");

struct FaArgs : SeqArgs {
    u32 *head, *bases;      // [n_lines]
    const u64 *line_rec;    // [n_lines + 1]: headers in front of line g
    const u64 *base_before; // [n_lines + 1]
    u64 *rec_line;          // [n_rec + 1]: the line of header r; n_lines closes the list, or the line of header n_rec (n_head > n_rec)
    u32 *rec_width;         // [n_rec]: the one width of the record's lines, or 0 (fa_widths_kernel)
    FaPiece *pieces;
    u64 n_head;             // header lines: n_rec, or n_rec + 1 in a window whose last record waits
    u64 hi;                 // a window that is not the last: its end in the slot (mark: is there a partial line behind the last newline); else 0
};
static_assert(std::is_trivially_copyable<FaArgs>::value, "a kernel argument by value");

__global__ __launch_bounds__(256) void fa_mark_kernel(FaArgs a)
{
    const u64 g = (u64)blockIdx.x * 256u + threadIdx.x;
    u32 status = 0;
    if (g < a.n_lines) {
        const u64 s = g ? a.line_end[g - 1] + 1 : a.lo, len = a.line_end[g] - s;
        const bool head = len && a.text[s] == '>';
        if (len >= kSqMaxRecord) status = kSqNeedHost;
        a.head[g] = head ? 1u : 0u;
        a.bases[g] = head || status ? 0u : (u32)len;
        // a window: the partial line behind its last newline begins with '>' -> ctl[3] (zeroed with the window's words)
        if (g + 1 == a.n_lines && a.line_end[g] + 1 < a.hi && a.text[a.line_end[g] + 1] == '>') a.ctl[3] = 1ull;
    }
    seq_status(a.ctl, status);
}

__global__ __launch_bounds__(256) void fa_heads_kernel(FaArgs a)
{
    const u64 g = (u64)blockIdx.x * 256u + threadIdx.x;
    u32 status = 0;
    if (g < a.n_lines) {
        if (a.head[g]) {
            // header n_rec (a window that is not the last): the record that waits; its line closes the list, it has no width
            const u64 r = a.line_rec[g];
            if (r <= a.n_rec) a.rec_line[r] = g;
            if (r < a.n_rec) a.rec_width[r] = g + 1 < a.n_lines && !a.head[g + 1] ? a.bases[g + 1] : 0u; // (its first line's; fa_widths_kernel)
        } else if (a.bases[g] && a.line_rec[g] == 0) status = kSqNeedHost; // bases in front of the first header (a window behind
                                                                           // one with a header begins with a header: never there)
        if (g == 0 && a.n_head == a.n_rec) a.rec_line[a.n_rec] = a.n_lines; // (else header n_rec's thread writes this element)
    }
    seq_status(a.ctl, status);
}

// ---- carry, FASTA: from the window's last header line on; all of the window when it has none -------------------------------------
// Runs behind fa_heads_kernel (rec_line[n_rec] is that header's line — or, where the partial last line is a header's and
// every record is whole, n_lines: the carry is that line) and, like sq_carry_kernel, in front of nothing that overwrites
// the slot.  A partial last line lies inside the carry whatever it holds.
struct FaCarry : SqCarry {
    const u64 *rec_line;
    u64 n_head;
};
__global__ __launch_bounds__(256) void fa_carry_kernel(FaCarry c)
{
    const u64 l = c.n_head ? c.rec_line[c.n_rec] : 0; // (l >= 1 lines lie in front of it, or it is the window's first)
    sq_carry_from(c, l ? c.line_end[l - 1] + 1 : c.lo);
}

// The one width of a record's lines, or 0: every line but the last holds as many bases as the first, the last 1 to as many,
// none is blank.  A record that has it needs no search: base b lies at byte b / w * (w + 1) + b % w of its sequence lines.
// A thread per line, which clears its record's width when the line does not fit: a record of millions of lines costs what
// its lines cost anywhere else.  Measured on 400 MB of reads wrapped at 80, scrubb / filter: the closed form took the
// kernels from 2.93 / 2.13 ms to 2.1 / 1.6 ms.
__global__ __launch_bounds__(256) void fa_widths_kernel(FaArgs a)
{
    const u64 g = (u64)blockIdx.x * 256u + threadIdx.x;
    if (g >= a.n_lines || a.head[g] || a.line_rec[g] == 0) return;
    const u64 r = a.line_rec[g] - 1;
    if (r >= a.n_rec) return; // (a line of the record that waits for the next window: rec_line[r + 1], rec_width[r] are not there)
    const u64 l0 = a.rec_line[r], l1 = a.rec_line[r + 1];
    const u32 w = a.bases[l0 + 1], n = a.bases[g]; // (l0 + 1 <= g: the record has this line)
    if (w == 0u || (g + 1 < l1 ? n != w : n == 0u || n > w)) a.rec_width[r] = 0u;
}

__device__ __forceinline__ u32 fa_rows(u32 n) { return (n + kFaWidth - 1u) / kFaWidth; }

struct FaLine { // the input line a thread last took a base from: bases [b0, b1) of the text, its first byte at `start`
    u64 g, b0, b1, start;
    bool have;
    __device__ __forceinline__ void reset() { have = false; }
};

// the line of piece p that holds base B of the text (p.base0 <= B < base_before[p.line1]): the last one whose base_before is
// not beyond B — blank lines share their base_before with the line behind them and are never the last.  The line behind the
// one in hand is tried first, then a search over what is left of the record.
__device__ __forceinline__ void fa_seek(const FaArgs &a, const FaPiece &p, u64 B, FaLine &ln)
{
    if (ln.have && B >= ln.b0 && B < ln.b1) return;
    u64 lo = p.line0;
    if (ln.have && B >= ln.b1) {
        lo = ln.g + 1; // (base_before[lo] == ln.b1 <= B; lo < line1, for B lies in the record)
        const u64 nb = a.base_before[lo + 1];
        if (B < nb) {
            ln.g = lo, ln.b0 = ln.b1, ln.b1 = nb, ln.start = a.line_end[lo - 1] + 1;
            return;
        }
    }
    u64 hi = p.line1;
    while (hi - lo > 1) {
        const u64 mid = lo + (hi - lo) / 2;
        if (a.base_before[mid] <= B) lo = mid;
        else hi = mid;
    }
    ln.g = lo, ln.b0 = a.base_before[lo], ln.b1 = a.base_before[lo + 1], ln.start = a.line_end[lo - 1] + 1, ln.have = true;
}

struct Fasta {
    using Args = FaArgs;
    using Piece = FaPiece;
    using Cursor = FaLine;

    template <bool EMIT>
    static __device__ __forceinline__ u32 record(const FaArgs &a, u64 r)
    {
        const unsigned char *t = a.text;
        const u64 l0 = a.rec_line[r], l1 = a.rec_line[r + 1];
        const u64 s = l0 ? a.line_end[l0 - 1] + 1 : a.lo, e0 = a.line_end[l0];
        if (!EMIT) a.rec_pieces[r] = 0u, a.rec_bytes[r] = 0u;
        if (a.line_end[l1 - 1] + 1 - s >= kSqMaxRecord) return kSqNeedHost;
        u64 sep = s + 1; // the name's end: the first blank, tab or form feed
        while (sep < e0 && t[sep] != ' ' && t[sep] != '\t' && t[sep] != '\x0c') sep++;
        if (sep == s + 1) return kSqNeedHost; // (no name: the host writes it back as it stands; the id table holds no such read)
        const u32 name_len = (u32)(sep - s - 1), desc_len = sep < e0 ? (u32)(e0 - sep - 1) : 0u;
        const u64 base0 = a.base_before[l0];
        const u32 seq_len = (u32)(a.base_before[l1] - base0);

        const SeqVerdict v = seq_verdict(a, s + 1, name_len);
        if (v.what == kSeqDrop) return 0u;
        FaPiece p{};
        p.hdr = s, p.base0 = base0, p.line0 = l0 + 1, p.line1 = l1, p.name_len = name_len;
        if (EMIT) p.width = a.rec_width[r];
        if (v.what == kSeqCopy) {
            const u64 bytes = 1ull + name_len + (desc_len ? 1ull + desc_len : 0ull) + 1ull + seq_len + fa_rows(seq_len);
            if (bytes >= kSqMaxRecord) return kSqNeedHost;
            if (!EMIT) a.rec_pieces[r] = 1u, a.rec_bytes[r] = (u32)bytes;
            else {
                p.out = a.out0 + a.byte_off[r], p.len = (u32)bytes, p.flags = kSqCopy, p.desc_len = desc_len, p.p0 = 0u, p.p1 = seq_len;
                a.pieces[a.piece0 + a.piece_off[r]] = p;
            }
            return 0u;
        }
        return seq_cut<EMIT>(a, r, v, seq_len, [&](u32 p0, u32 p1, u32 k, u64 at) {
            const u32 L = p1 - p0;
            const u64 plen = 1ull + name_len + 2u + sq_digits(p0) + sq_digits(p1) + 1u + L + fa_rows(L);
            if (EMIT) {
                p.out = a.out0 + a.byte_off[r] + at, p.len = (u32)plen, p.flags = 0u, p.desc_len = 0u, p.p0 = p0, p.p1 = p1;
                a.pieces[a.piece0 + a.piece_off[r] + k] = p;
            }
            return plen;
        });
    }

    static FaPiece raw_piece(u64 at, u32 len) // (host) `len` bytes at `at` of SeqArgs::raw, first in the output
    {
        FaPiece p{};
        p.hdr = at, p.len = len, p.flags = kSqRaw;
        return p;
    }

    static __device__ __forceinline__ void at(const FaArgs &a, const FaPiece &p, u32 k, FaLine &ln, const unsigned char *&src, u32 &rem, u32 &lit)
    {
        if (p.flags & kSqRaw) { // the output tail of the window before, as it lies in that window's slot
            src = a.raw + p.hdr + k, rem = p.len - k;
            return;
        }
        const unsigned char *rec = a.text + p.hdr;
        src = nullptr, rem = 1, lit = '\n';
        if (k == 0) {
            lit = '>';
            return;
        }
        k -= 1;
        if (k < p.name_len) {
            src = rec + 1 + k, rem = p.name_len - k;
            return;
        }
        k -= p.name_len;
        if (p.flags & kSqCopy) {
            if (p.desc_len) { // whatever the separator was, a blank
                if (k == 0) {
                    lit = ' ';
                    return;
                }
                k -= 1;
                if (k < p.desc_len) {
                    src = rec + 1 + p.name_len + 1 + k, rem = p.desc_len - k;
                    return;
                }
                k -= p.desc_len;
            }
        } else {
            const u32 d0 = sq_digits(p.p0), d1 = sq_digits(p.p1);
            if (k < 2u + d0 + d1) {
                lit = k == 0 || k == d0 + 1u ? '_' : k <= d0 ? sq_digit_at(p.p0, d0, k - 1u) : sq_digit_at(p.p1, d1, k - d0 - 2u);
                return;
            }
            k -= 2u + d0 + d1;
        }
        if (k == 0) return; // the header's newline
        k -= 1;
        const u32 L = p.p1 - p.p0, row = k / (kFaWidth + 1u), col = k % (kFaWidth + 1u), at = row * kFaWidth + col;
        if (col == kFaWidth || at >= L) return; // a row's newline; the last row's
        if (p.width) { // (a.line_end[p.line0 - 1]: the header's newline)
            const u32 b = p.p0 + at, q = b / p.width, r = b - q * p.width;
            src = a.text + a.line_end[p.line0 - 1] + 1 + (u64)q * ((u64)p.width + 1u) + r;
            rem = min(min(p.width - r, kFaWidth - col), L - at);
            return;
        }
        const u64 B = p.base0 + p.p0 + at;
        fa_seek(a, p, B, ln);
        src = a.text + ln.start + (B - ln.b0);
        rem = (u32)min(min(ln.b1 - B, (u64)(kFaWidth - col)), (u64)(L - at));
    }
};

} // namespace yk

namespace {

constexpr u64 kGzBatchBlocks = 2048;          // blocks of 65 280 bytes per batch of the encoder
// whether a text that fits whole runs in windows all the same (the switch aside): decided by measurement, DESIGN 7k, 7l
constexpr bool kSeqWindowsWhenFits = false;

struct SeqEditScratch { // the editor's buffers; they stay with the engine (grow-only), go with yacrd_engine_trim / destroy
    static constexpr yacrd_engine::Slot kScratchSlot = yacrd_engine::kSeqEdit;
    DevBuf text, out, lengths, bad_off, bad_reg, tile_nl, tile_l0, line_end, rec_pieces, rec_bytes, piece_off, byte_off, pieces, ctl, part;
    EdTableOwner table; // the reads' names and types, the id table over them
    DevBuf ln_head, ln_bases, ln_rec, base_before, rec_line, rec_width; // FASTA: per line, per record
    PinBuf pin; // two output pieces + the control words
    DevBuf wtext[2], wout[2]; // a run in windows (SeqRun::run_windows): its two text slots, its two output slots
};

using yseg::Sink;

struct SeqJob {
    int op = 0;
    int n_threads = 0;
    const yacrd_report_table *table = nullptr;
    bool gzip = false;
    bool fasta = false; // '>' records of any number of lines, written again at 80 columns
    yacrd_gzip_stats *gzip_stats = nullptr;
    // BGZF in: the compressed file in host memory and its members as the host walked them; the run's `n` is the text they inflate to
    const char *bgzf = nullptr;
    u64 bgzf_bytes = 0;
    const std::vector<yif::InfMember> *members = nullptr;
    yacrd_gunzip_stats *gunzip_stats = nullptr;
    // plain gzip in (the _gz_ forms): the member as stream_inflate_open left it in HBM, sized and chained; the run's `n` is its text
    StreamInflate *stream = nullptr;
    yacrd_gunzip_stream_stats *stream_stats = nullptr;
};

// One edit on its way through the device: built once per call (run_seq_edit), its phases in the order they run.
struct SeqRun {
    yacrd_engine *e;
    const SeqJob &job;
    const TextSource &src;
    const u64 n;
    Sink &sink;
    yacrd_seq_edit_stats *stats;
    SeqEditScratch &S;
    u64 W = 0; // 0: the whole text at once; else the run goes window by window, this many new bytes each (run_windows)
    u64 R = 0, G = 0, name_bytes = 0, cap = 1024;
    u64 n_tiles = 0, n_lines = 0, n_rec = 0, n_pieces = 0, total = 0;
    size_t n_segs = 0;
    bool blit = false;
    yk::SqArgs ga{};
    yk::FaArgs fa{}; // (FASTA: what the kernels behind the line index take)
    volatile u64 *h_ctl = nullptr; // pinned: [0..3] what a phase brings home, [4..7] the way out's (the encoder's words), [8..11] the copy pass's of two windows
    Events ev;                     // pairs around the kernels of a phase (timing)
    size_t n_ev = 0;
    OutDevice od;                  // the way out of HBM (gpu_out.h; the order and the release rule: host/way_out.h)
    Out out{od, sink};
    double t_start = 0, t_table = 0, t_text = 0, out_busy_ms = 0;
    Events iev; // around the inflate kernel
    float inf_h2d_ms = 0, inf_kernel_ms = 0;

    // whether `need` more bytes of HBM are there, counting what the scratch already holds of them
    static bool fits(double need, double held)
    {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return true; // (the reserves then say)
        return need * 1.125 + (double)((size_t)64 << 20) <= (double)free_b + held;
    }
    bool room_failed = false; // the whole-text run found no room (run_seq_edit: a text of more than a window then runs in windows)
    int no_room()
    {
        room_failed = true;
        return no_room_message();
    }
    // (a window's tables: asked for only where a reserve would have to grow them)
    static bool room_for(double need, double held) { return need <= held || fits(need, held); }
    double held_line_tables() const { return (double)S.line_end.cap + (double)S.ln_head.cap + (double)S.ln_bases.cap + (double)S.ln_rec.cap + (double)S.base_before.cap; }
    double held_record_tables() const { return (double)S.rec_line.cap + (double)S.rec_width.cap + (double)S.piece_off.cap + (double)S.byte_off.cap; }
    static int no_room_message() { return fail(YACRD_EFALLBACK, "the text and its output do not fit this device's free memory: the host loop streams them"); }

    bool ev_open()
    {
        if (n_ev + 2 > ev.v.size() && !ev.add(2)) return false; // (a run in windows: its pairs are as many as its windows make them)
        return hipEventRecord(ev[n_ev], e->stream) == hipSuccess;
    }
    bool ev_close()
    {
        n_ev += 2;
        return hipEventRecord(ev[n_ev - 1], e->stream) == hipSuccess;
    }
    // the end of a phase: these device words -> h_ctl[0 .. k), the stream waited for; `ok`: what its event pair said
    int bring_words(bool ok, std::initializer_list<const void *> words)
    {
        size_t k = 0;
        for (const void *w : words) HIP_TRY(hipMemcpyAsync((void *)(h_ctl + k++), w, sizeof(u64), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(hipGetLastError());
        if (!ok) return fail(YACRD_ENODEV, "sequence editor: a HIP call failed");
        return YACRD_OK;
    }

    // a format's kernel arguments: the common part is filled once, in `ga`
    yk::SqArgs &args(yk::Fastq) { return ga; }
    yk::FaArgs &args(yk::Fasta)
    {
        static_cast<yk::SeqArgs &>(fa) = ga;
        return fa;
    }
    template <class Format, bool EMIT>
    void launch_plan()
    {
        if (n_rec) hipLaunchKernelGGL((yk::seq_plan_kernel<Format, EMIT>), dim3((u32)((n_rec + 255) / 256)), dim3(256), 0, e->stream, args(Format{}));
    }

    // the table's shape, the text's last byte, the sizes that follow from n
    int plan()
    {
        const yacrd_report_table &t = *job.table;
        R = t.n_reads;
        if (R >= 0x7FFFFFFFull) return fail(YACRD_EFALLBACK, "more reads than the device table holds");
        if (R && (!t.name_off || !t.names || !t.lengths || !t.bad_offsets || !t.read_type)) return fail(YACRD_EINVAL, "the report table is incomplete");
        if (R) {
            if (t.name_off[0] != 0 || t.bad_offsets[0] != 0) return fail(YACRD_EINVAL, "name_off / bad_offsets do not begin at 0");
            for (u64 r = 0; r < R; r++)
                if (t.name_off[r + 1] < t.name_off[r] || t.bad_offsets[r + 1] < t.bad_offsets[r])
                    return fail(YACRD_EINVAL, "name_off / bad_offsets do not rise");
            name_bytes = t.name_off[R], G = t.bad_offsets[R];
            if (G >= 0x7FFFFFFFull) return fail(YACRD_EFALLBACK, "more regions than the device table holds");
            if (G && !t.bad_regions) return fail(YACRD_EINVAL, "the report table is incomplete");
        }
        if (n && !job.bgzf && !job.stream) { // (BGZF / gzip in: the last byte comes back from the device behind the inflate, inflate_text / stream_text)
            char last = 0;
            if (!src.fetch(&last, 1, n - 1)) return fail(YACRD_EINVAL, "read error in the sequence file");
            if (last != '\n') return fail(YACRD_EFALLBACK, "the text's last line has no newline: the host loop's case");
        }
        if (n && job.bgzf && W) { // BGZF in windows: no launch has run yet — the last member that holds text, decoded on the host
            bool nl = true;
            u32 status = 0;
            const int rcl = bgzf_last_byte(reinterpret_cast<const unsigned char *>(job.bgzf), job.bgzf_bytes, job.members->data(), job.members->size(), &nl, &status);
            if (rcl == 1) return inflate_not_taken(status);
            if (rcl) return fail(YACRD_ENOMEM, "host allocation failed");
            if (!nl) return fail(YACRD_EFALLBACK, "the text's last line has no newline: the host loop's case");
        }
        while (cap < 2 * R) cap <<= 1;
        t_start = now_ms();
        if (W) { // in windows: the ring's slots, two of text and two of output (sized for a window that goes out as it came in), and a window's tables
            n_tiles = (2 * W + yk::kGpTile - 1) / yk::kGpTile;
            // FASTA: a window's tables too — 32 bytes a line; 36 bytes a record and 4 of rec_width —, here for the 2 W bytes a
            // window may hold, wrapped at 60 columns (2 W / 61 lines) with a record every ten lines: per line 32 bytes and a tenth
            // of a record's 40, the 4.0 below.  A window's own line and header counts decide when they are known (window_records:
            // a text of shorter lines or records may find no room there)
            const double fa_tables = job.fasta ? 2.0 * (double)W / 61.0 * (32.0 + 4.0) : 0.0;
            // BGZF in: the windows end where members end (bgzf_windows.h); the compressed slot and the largest slice of the member
            // table count, not the whole stream
            double bgzf_ring = 0.0;
            if (job.bgzf) {
                if (!ybw::window_cuts(job.members->data(), job.members->size(), W, cuts)) return fail(YACRD_ENOMEM, "host allocation failed");
                u64 slice = 0;
                for (const ybw::WindowCut &c : cuts) slice = std::max(slice, c.m1 - c.m0);
                if (slice >= 0x7FFFFFFFull) return fail(YACRD_EFALLBACK, "more BGZF members than the device decoder numbers");
                bgzf_ring = (double)W + 64.0 + (double)(slice + 1) * (double)sizeof(yif::InfMember);
            }
            const double ring = 2.0 * (2.0 * (double)W + 64.0) + 2.0 * (double)W + (double)W * 0.25 + fa_tables + bgzf_ring;
            const double held_w = (double)S.wtext[0].cap + (double)S.wtext[1].cap + (double)S.wout[0].cap + (double)S.wout[1].cap +
                                  (double)S.table.names.cap + (double)S.table.slots.cap + (double)S.bad_reg.cap +
                                  (job.fasta ? held_line_tables() + held_record_tables() : 0.0) + (job.bgzf ? (double)inflate_window_held(e) : 0.0);
            if (!fits(ring + (double)name_bytes + (double)cap * 4.0 + (double)R * 21.0 + (double)G * 8.0, held_w)) return no_room_message();
            return YACRD_OK;
        }
        n_tiles = (n + yk::kGpTile - 1) / yk::kGpTile;
        if (n_tiles >= 0x7FFFFFFFull) return fail(YACRD_EFALLBACK, "file too large for the device editor");
        n_segs = (size_t)((n + kTextChunk * kTextSeg - 1) / (kTextChunk * kTextSeg));
        const double held = (double)S.text.cap + (double)S.table.names.cap + (double)S.table.slots.cap + (double)S.bad_reg.cap + (double)S.tile_l0.cap;
        // (the output is at least... unknown yet: asked for again when it is; here the text, the table and the tiles' words)
        const double comp = job.bgzf ? (double)job.bgzf_bytes + (double)job.members->size() * (double)sizeof(yif::InfMember) : 0.0; // (the inflate scratch's)
        if (!fits((double)n + comp + (double)name_bytes + (double)cap * 4.0 + (double)R * 21.0 + (double)G * 8.0 + (double)n_tiles * 12.0, held)) return no_room();
        return YACRD_OK;
    }

    // the text's buffer, the table in HBM, the id table over the names; streams, events, the pinned pieces
    int upload_table()
    {
        const yacrd_report_table &t = *job.table;
        const void *mirror_before = S.text.p;
        if (!W) HIP_TRY(S.text.reserve((size_t)n + 64));
        blit = S.text.p != mirror_before; // a fresh mirror fills faster by copy kernel (gpu_paf.hip)
        HIP_TRY(S.tile_nl.reserve((size_t)(n_tiles + 1) * sizeof(u32)));
        HIP_TRY(S.tile_l0.reserve((size_t)(n_tiles + 2) * sizeof(u64)));
        HIP_TRY(S.ctl.reserve(4 * 64)); // (a run in windows: four windows' words in turn)
        HIP_TRY(hipMemsetAsync(S.ctl.p, 0, 4 * 64, e->stream));
        HIP_TRY(S.pin.reserve(2 * kOutPiece + 12 * sizeof(u64) + 2 * sizeof(yk::FaPiece))); // (the raw pieces of two windows, of the larger kind: run_windows)
        h_ctl = reinterpret_cast<volatile u64 *>(S.pin.as<char>() + 2 * kOutPiece);
        for (int i = 0; i < 12; i++) h_ctl[i] = 0;
        if (!od.make(job.gzip) || !ev.add(2 * n_segs + 10)) HIP_TRY(why_not_added());
        HIP_TRY(S.lengths.reserve((size_t)(R + 1) * sizeof(u32)));
        HIP_TRY(S.bad_off.reserve((size_t)(R + 1) * sizeof(u64)));
        HIP_TRY(S.bad_reg.reserve((size_t)(2 * G + 2) * sizeof(u32)));
        if (const int rc = S.table.upload(e, t.names, t.name_off, t.read_type, R, name_bytes, cap, &ga.tab)) return rc;
        if (R) {
            if (const int rch = h2d(e, S.lengths.p, t.lengths, (size_t)R * sizeof(u32))) return rch;
            if (const int rch = h2d(e, S.bad_off.p, t.bad_offsets, (size_t)(R + 1) * sizeof(u64))) return rch;
            if (G)
                if (const int rch = h2d(e, S.bad_reg.p, t.bad_regions, (size_t)(2 * G) * sizeof(u32))) return rch;
        }
        HIP_TRY(hipStreamSynchronize(e->stream));
        t_table = now_ms();
        ga.text = S.text.as<unsigned char>(), ga.n = n, ga.avail = n;
        ga.lengths = S.lengths.as<u32>(), ga.bad_off = S.bad_off.as<u64>(), ga.bad_reg = S.bad_reg.as<u32>();
        ga.tile_nl = S.tile_nl.as<u32>(), ga.tile_l0 = S.tile_l0.as<u64>();
        ga.ctl = S.ctl.as<unsigned long long>();
        ga.op = (u32)job.op;
        return YACRD_OK;
    }

    // BGZF in: the compressed file into HBM, its members inflated into the text buffer; the decoder's status and the text's last
    // byte come home; then the lines of every tile in one launch
    int inflate_text()
    {
        InflateDevice d;
        if (const int rc = inflate_device_open(e, job.bgzf_bytes, job.members->data(), job.members->size(), &d)) return rc;
        if (!iev.add(2)) HIP_TRY(why_not_added());
        HIP_TRY(hipMemsetAsync(S.text.as<char>() + n, 0, 64, e->stream));
        const double t0 = now_ms();
        TextSource comp;
        comp.mem = job.bgzf;
        const int moved = move_text(e, comp, 0, job.bgzf_bytes, reinterpret_cast<char *>(d.comp), d.fresh, job.n_threads, [](u64, u64, u64) {});
        if (moved == 3) return fail(YACRD_ENOMEM, "sequence text to HBM: no pinned memory");
        if (moved) return fail(YACRD_ENODEV, "sequence editor: a HIP call failed");
        inf_h2d_ms = (float)(now_ms() - t0);
        HIP_TRY(hipEventRecord(iev[0], e->stream));
        if (const int rc = inflate_device_run(e, d, e->stream, S.text.as<unsigned char>(), n)) return rc;
        HIP_TRY(hipEventRecord(iev[1], e->stream));
        HIP_TRY(hipMemcpyAsync((void *)(h_ctl + 2), d.status, sizeof(u32), hipMemcpyDeviceToHost, e->stream));
        if (n) HIP_TRY(hipMemcpyAsync((void *)(h_ctl + 3), S.text.as<char>() + (n - 1), 1, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(hipGetLastError());
        inf_kernel_ms = ev_ms(iev[0], iev[1]);
        if ((u32)h_ctl[2]) return inflate_not_taken((u32)h_ctl[2]);
        if (n && (char)(h_ctl[3] & 255u) != '\n') return fail(YACRD_EFALLBACK, "the text's last line has no newline: the host loop's case");
        ga.avail = n, ga.tile0 = 0;
        bool ok = ev_open();
        if (n_tiles) hipLaunchKernelGGL(yk::sq_lines_kernel, dim3((u32)n_tiles), dim3(yk::kGpT), 0, e->stream, ga);
        ok = ok && ev_close();
        t_text = now_ms();
        if (!ok) return fail(YACRD_ENODEV, "sequence editor: a HIP call failed");
        return YACRD_OK;
    }

    // plain gzip in: the member lies in HBM, sized and chained (stream_inflate_open); its symbols, windows and bytes into the text
    // buffer, the decoder's status and CRC checked behind them (stream_inflate_run waits), the text's last byte; then the lines
    int stream_text()
    {
        HIP_TRY(hipMemsetAsync(S.text.as<char>() + n, 0, 64, e->stream));
        if (const int rc = stream_inflate_run(e, *job.stream, S.text.as<unsigned char>())) return rc;
        if (n) {
            HIP_TRY(hipMemcpyAsync((void *)(h_ctl + 3), S.text.as<char>() + (n - 1), 1, hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
            if ((char)(h_ctl[3] & 255u) != '\n') return fail(YACRD_EFALLBACK, "the text's last line has no newline: the host loop's case");
        }
        ga.avail = n, ga.tile0 = 0;
        bool ok = ev_open();
        if (n_tiles) hipLaunchKernelGGL(yk::sq_lines_kernel, dim3((u32)n_tiles), dim3(yk::kGpT), 0, e->stream, ga);
        ok = ok && ev_close();
        t_text = now_ms();
        if (!ok) return fail(YACRD_ENODEV, "sequence editor: a HIP call failed");
        return YACRD_OK;
    }

    // the text into HBM; the lines of every segment counted as it lands
    int move_text_in()
    {
        HIP_TRY(hipMemsetAsync(S.text.as<char>() + n, 0, 64, e->stream));
        bool ok = true;
        const int moved = move_text(e, src, 0, n, S.text.as<char>(), blit, job.n_threads, [&](u64 seg_begin, u64 seg_end, u64 avail) {
            const u32 t0 = (u32)(seg_begin / yk::kGpTile), t1 = seg_end >= n ? (u32)n_tiles : (u32)(seg_end / yk::kGpTile);
            ga.avail = seg_end >= n ? n : std::min<u64>(avail, seg_end); // (a tile of this segment reads nothing behind it)
            ga.tile0 = t0;
            ok = ok && ev_open();
            if (t1 > t0) hipLaunchKernelGGL(yk::sq_lines_kernel, dim3(t1 - t0), dim3(yk::kGpT), 0, e->stream, ga);
            ok = ok && ev_close();
        });
        t_text = now_ms();
        if (moved == 2) return fail(YACRD_EINVAL, "read error in the sequence file");
        if (moved == 3) return fail(YACRD_ENOMEM, "sequence text to HBM: no pinned memory");
        if (moved || !ok) return fail(YACRD_ENODEV, "sequence editor: a HIP call failed");
        return YACRD_OK;
    }

    // the text into HBM (moved, or inflated there) with its tiles' lines counted; then the scan of the tiles' counts
    int move_and_count()
    {
        if (const int rc = job.bgzf ? inflate_text() : job.stream ? stream_text() : move_text_in()) return rc;
        ga.avail = n;
        bool ok = ev_open();
        if (const int rc = scan_u32_to_u64(e, S.tile_nl.as<u32>(), n_tiles, S.tile_l0.as<u64>(), S.part)) return rc;
        ok = ok && ev_close();
        if (const int rc = bring_words(ok, {S.tile_l0.as<u64>() + n_tiles, S.ctl.p})) return rc;
        n_lines = h_ctl[0];
        if (h_ctl[1] & yk::kSqNeedHost) return fail(YACRD_EFALLBACK, "the text holds a CR: the host loop decides");
        ga.n_lines = n_lines;
        if (job.fasta) return YACRD_OK; // (its records are counted on the device: size_fasta)
        if (n_lines % 4) return fail(YACRD_EFALLBACK, "the line count is no multiple of four: the host loop decides");
        n_rec = n_lines / 4;
        if (n_rec >= 0x7FFFFFFFull) return fail(YACRD_EFALLBACK, "more records than the device editor numbers");
        return YACRD_OK;
    }

    void launch_index()
    {
        ga.tile0 = 0;
        if (n_tiles) hipLaunchKernelGGL(yk::sq_index_kernel, dim3((u32)n_tiles), dim3(yk::kGpT), 0, e->stream, ga);
    }

    // FASTQ's front: the line index, in the bracket of the plan
    int size_fastq()
    {
        if (!fits((double)n_lines * 8.0 + (double)n_rec * 24.0, (double)S.line_end.cap + (double)S.piece_off.cap + (double)S.byte_off.cap)) return no_room();
        HIP_TRY(S.line_end.reserve((size_t)(n_lines + 1) * sizeof(u64)));
        ga.line_end = S.line_end.as<u64>();
        return size_records<yk::Fastq>([&] { launch_index(); });
    }

    // FASTA's front: index, mark and the two scans over the lines — how many records —, then heads and widths in the bracket of the plan
    int size_fasta()
    {
        const double line_tables = (double)n_lines * 32.0;
        if (!fits(line_tables, (double)S.line_end.cap + (double)S.ln_head.cap + (double)S.ln_bases.cap + (double)S.ln_rec.cap + (double)S.base_before.cap))
            return no_room();
        if (const int rc = reserve_line_tables()) return rc;
        const dim3 line_grid((u32)((n_lines + 255) / 256));
        bool ok = ev_open();
        launch_index();
        if (n_lines) hipLaunchKernelGGL(yk::fa_mark_kernel, line_grid, dim3(256), 0, e->stream, args(yk::Fasta{}));
        if (const int rc = scan_u32_to_u64(e, fa.head, n_lines, S.ln_rec.as<u64>(), S.part)) return rc;
        if (const int rc = scan_u32_to_u64(e, fa.bases, n_lines, S.base_before.as<u64>(), S.part)) return rc;
        ok = ok && ev_close();
        if (const int rc = bring_words(ok, {S.ln_rec.as<u64>() + n_lines, S.ctl.p})) return rc;
        n_rec = h_ctl[0];
        if (h_ctl[1] & yk::kSqNeedHost) return fail(YACRD_EFALLBACK, "a line longer than the device editor's offsets: the host loop decides");
        if (n_rec >= 0x7FFFFFFFull) return fail(YACRD_EFALLBACK, "more records than the device editor numbers");

        if (!fits((double)n_rec * 36.0, (double)S.rec_line.cap + (double)S.piece_off.cap + (double)S.byte_off.cap)) return no_room();
        HIP_TRY(S.rec_line.reserve((size_t)(n_rec + 1) * sizeof(u64)));
        HIP_TRY(S.rec_width.reserve((size_t)(n_rec + 1) * sizeof(u32)));
        fa.rec_line = S.rec_line.as<u64>(), fa.rec_width = S.rec_width.as<u32>(), fa.n_head = n_rec;
        return size_records<yk::Fasta>(
            [&] {
                if (n_lines) hipLaunchKernelGGL(yk::fa_heads_kernel, line_grid, dim3(256), 0, e->stream, args(yk::Fasta{}));
                if (n_rec) hipLaunchKernelGGL(yk::fa_widths_kernel, line_grid, dim3(256), 0, e->stream, args(yk::Fasta{}));
            });
    }

    // what the plan's status bit says, by format
    static const char *not_taken(yk::Fastq)
    {
        return "a record that is not \"@name[ desc]\\nseq\\n+\\nqual\\n\", a cut position beyond its read or a region with begin > end: the host loop decides";
    }
    static const char *not_taken(yk::Fasta)
    {
        return "bases in front of the first header, a header without a name, a cut position beyond its read or a region with begin > end: the host loop decides";
    }
    // the per-record tables both formats' plans fill, for n_rec records
    int reserve_record_tables()
    {
        HIP_TRY(S.rec_pieces.reserve((size_t)(n_rec + 1) * sizeof(u32)));
        HIP_TRY(S.rec_bytes.reserve((size_t)(n_rec + 1) * sizeof(u32)));
        HIP_TRY(S.piece_off.reserve((size_t)(n_rec + 2) * sizeof(u64)));
        HIP_TRY(S.byte_off.reserve((size_t)(n_rec + 2) * sizeof(u64)));
        ga.n_rec = n_rec;
        ga.rec_pieces = S.rec_pieces.as<u32>(), ga.rec_bytes = S.rec_bytes.as<u32>();
        ga.piece_off = S.piece_off.as<u64>(), ga.byte_off = S.byte_off.as<u64>();
        return YACRD_OK;
    }
    // FASTA's tables per line, for n_lines lines
    int reserve_line_tables()
    {
        HIP_TRY(S.line_end.reserve((size_t)(n_lines + 1) * sizeof(u64)));
        HIP_TRY(S.ln_head.reserve((size_t)(n_lines + 1) * sizeof(u32)));
        HIP_TRY(S.ln_bases.reserve((size_t)(n_lines + 1) * sizeof(u32)));
        HIP_TRY(S.ln_rec.reserve((size_t)(n_lines + 2) * sizeof(u64)));
        HIP_TRY(S.base_before.reserve((size_t)(n_lines + 2) * sizeof(u64)));
        ga.line_end = S.line_end.as<u64>();
        fa.head = S.ln_head.as<u32>(), fa.bases = S.ln_bases.as<u32>();
        fa.line_rec = S.ln_rec.as<u64>(), fa.base_before = S.base_before.as<u64>();
        return YACRD_OK;
    }

    // what both formats do once the records are numbered: in one bracket the format's own kernels (`front`), the plan and the
    // two scans; how many output records, how many bytes
    template <class Format, class Front>
    int size_records(Front &&front)
    {
        if (const int rc = reserve_record_tables()) return rc;
        bool ok = ev_open();
        front();
        launch_plan<Format, false>();
        if (const int rc = scan_u32_to_u64(e, ga.rec_pieces, n_rec, S.piece_off.as<u64>(), S.part)) return rc;
        if (const int rc = scan_u32_to_u64(e, ga.rec_bytes, n_rec, S.byte_off.as<u64>(), S.part)) return rc;
        ok = ok && ev_close();
        if (const int rc = bring_words(ok, {S.piece_off.as<u64>() + n_rec, S.byte_off.as<u64>() + n_rec, S.ctl.p})) return rc;
        n_pieces = h_ctl[0], total = h_ctl[1];
        if (h_ctl[2] & yk::kSqNeedHost) return fail(YACRD_EFALLBACK, not_taken(Format{}));
        if (n_pieces >= 0x7FFFFFFFull) return fail(YACRD_EFALLBACK, "more output records than the device editor numbers");
        return YACRD_OK;
    }

    // the line index and what is the format's own in front of the plan, then the plan and the two scans
    int size_output() { return job.fasta ? size_fasta() : size_fastq(); }

    // the output's buffers (the encoder's too), the piece descriptors, the copy pass
    template <class Format>
    int gather()
    {
        const u64 gz_blocks = job.gzip ? std::min<u64>(kGzBatchBlocks, (total + ydf::kBlock - 1) / ydf::kBlock + 1) : 0;
        using Piece = typename Format::Piece;
        if (!fits((double)total + (double)n_pieces * (double)sizeof(Piece) + (double)gz_blocks * (double)ydf::kSlot * 3.0, (double)S.out.cap + (double)S.pieces.cap)) return no_room();
        const u64 padded = (total + 15) & ~(u64)15;
        HIP_TRY(S.out.reserve((size_t)padded + 64));
        HIP_TRY(S.pieces.reserve((size_t)(n_pieces + 1) * sizeof(Piece)));
        if (job.gzip)
            if (const int rcg = od.open(e, gz_blocks, true)) return rcg;
        out.bind(S.pin.as<char>(), h_ctl + 4);
        ga.n_pieces = n_pieces, ga.total = total, ga.out = S.out.as<unsigned char>();
        args(Format{}).pieces = S.pieces.as<Piece>();
        bool ok = ev_open();
        if (total) {
            launch_plan<Format, true>();
            hipLaunchKernelGGL(yk::seq_copy_kernel<Format>, dim3((u32)((total + yk::kSqOutTile - 1) / yk::kSqOutTile)), dim3(yk::kGpT), 0, e->stream, args(Format{}));
        }
        ok = ok && ev_close();
        if (const int rc = bring_words(ok, {S.ctl.p, S.ctl.as<u64>() + 1})) return rc;
        if (h_ctl[0] || h_ctl[1] != total) return fail(YACRD_EINTERNAL, "sequence editor: the copy pass stored other bytes than the plan counted");
        return YACRD_OK;
    }
    int gather() { return job.fasta ? gather<yk::Fasta>() : gather<yk::Fastq>(); }

    // what the way out says (host/way_out.h) as this editor's code and message; a stop is the other thread's code.  A call
    // of the encoder's that failed: the whole-text run returns what the call said, the writer thread of a run in windows its own words
    int out_says(yout::Result r, const char **msg) const
    {
        *msg = "";
        if (r == yout::kDeviceFailed && out.on_way_home) return *msg = "sequence editor: a HIP call failed on the way home", YACRD_ENODEV;
        if (r == yout::kDeviceFailed && !W) return *msg = od.msg.c_str(), od.code;
        if (r == yout::kDeviceFailed) return *msg = od.no_event ? "sequence editor: a HIP event could not be created" : "sequence editor: a HIP call failed in the encoder", YACRD_ENODEV;
        if (r == yout::kSinkFailed) return *msg = "Error during writing of the output file", YACRD_EINVAL;
        if (r == yout::kBoundBroken && out.out_of_order) return *msg = "sequence editor: a batch was to be encoded with two still out", YACRD_EINTERNAL;
        if (r == yout::kBoundBroken) return *msg = "device deflate: more bytes than the members' slots hold", YACRD_EINTERNAL;
        return YACRD_OK;
    }

    // ==== the run in windows (text from a file or from memory; DESIGN 7k, FASTA: 7l) ==================================================
    // Window k's new bytes are text[kW, min((k + 1) W, n)); its text is the carry of window k - 1 — the bytes behind that
    // window's last whole record — and then its new bytes.  A text slot is [carry area: W][new bytes: W][64 zero bytes]: the
    // new bytes always land at offset W, the carry is moved on the device to END at W (sq_carry_kernel), so a window is bytes
    // [lo, hi) of its slot, lo = W - carry, and by induction begins on a record boundary: its records are its lines 4j .. 4j + 3.
    // FASTA: a window's whole records are those in front of its last header line — the record behind that line may go on in
    // the next window even where it ends with this one —, the carry begins at that line (fa_carry_kernel), and a window
    // begins with a header or, while no header has been seen, with what may stand in front of the first.
    //
    // Who runs beside whom.  THIS thread lands window k (move_text: its threads and copy streams), launches k's kernels on the
    // engine's stream and waits for it twice — line count; pieces, bytes, status, carry; FASTA waits once more in between, for
    // the header count that sizes the record tables, S'(k) —, then launches k's pieces and copy
    // passes and goes on to land window k + 1 WITHOUT waiting for them.  The WRITER thread takes the windows in order behind
    // the event of their copy pass: the bytes go home through the two pinned pieces into the sink or, gzip out, through the
    // encoder on its own stream first.  So window k + 1 lands while k is gathered and while k and k - 1 leave.
    //
    // Why nothing is freed or overwritten under a kernel (the engine's stream runs in order; S(k) is this thread's second wait
    // of window k, W1(k) its first — both leave the engine's stream empty):
    //   text slots, two   window k + 1 is written — its carry by k's carry kernel, its new bytes by the mover — into the slot
    //                     window k - 1 lay in.  Its last reader is the copy pass of k - 1.  The carry kernel of k is enqueued
    //                     behind that pass on the same stream; the mover starts behind S(k), which the pass precedes.
    //   a window's tables line_end, rec_*, *_off, pieces, tile_* are one set, reserved behind W1(k) (pieces: behind S(k)): every
    //                     kernel of window k - 1 has ended by then, and the writer never reads them.
    //   FASTA's tables    ln_head, ln_bases, ln_rec, base_before (per line) are reserved with line_end behind W1(k); rec_line,
    //                     rec_width and the rec_* / *_off above behind S'(k), which leaves the stream empty too: index, mark and
    //                     the line scans of window k have ended, and heads, widths, carry and plan — their first readers and
    //                     writers — are enqueued behind the reserve.  The copy pass of k reads line_end and base_before; it has
    //                     ended by W1(k + 1), in front of the next reserve of either.
    //   `part`            (the scans' scratch) is reserved inside a scan; the scans of a window follow W1(k), S'(k) or S(k - 1)
    //                     with no other scan in flight but one over as many elements.
    //   output slots, two slot k & 1 is read by the writer for window k and, gzip out, by the copy pass of window k + 1 (the
    //                     raw piece: k's ragged tail).  This thread reserves and refills it for window k + 2 behind S(k + 2) —
    //                     the copy pass of k + 1 has ended — and behind the writer's release of window k (host/way_out.h).
    //   control words     four sets in turn; a set is zeroed for window k + 4 behind the release of window k + 1.
    //
    // BGZF in.  The windows are the cuts of bgzf_windows.h: window k's new bytes are text[t0, t1) of cut k, at most
    // W and possibly none, and they are not moved but inflated: this thread lands the stream's bytes [c0, c1) in the compressed
    // slot (the mover, as above), brings the cut's slice of the member table up and launches inf_window_kernel and then
    // sq_lines_kernel over the new tiles on the engine's stream, which waits for the landing's copy events.  The decoder's
    // status word comes home with W1(k) and is read before the line count.  From W1(k) on the window is the one above.
    //   compressed slot,  written by the mover for window k + 1 behind S(k); its last reader is the inflate of window k, which
    //   one               was enqueued in front of W1(k): the engine's stream was empty at W1(k), at S'(k) and at S(k).  One slot
    //                     suffices for that reason: nothing is gained by landing k + 1 while k inflates that the text slots'
    //                     own order (land behind S(k)) would allow.
    //   member slice      (grow-only, in the inflate scratch) reserved and filled behind S(k - 1), in front of window k's inflate.
    //                     The engine's stream is NOT empty then — the pieces and copy pass of k - 1 are still enqueued —, but they
    //                     never read the slice: its last reader, the inflate of k - 1, has ended by W1(k - 1), so a reserve that
    //                     grows it frees nothing a kernel uses, and the refill is ordered on the same stream.
    //   text slots        the inflate of window k writes slot k & 1 from offset W on — on the engine's stream, behind the copy
    //                     pass of k - 2 (its last reader) and behind the carry kernel of k - 1, which wrote in front of W.
    //   status word       one for the run, zeroed by inflate_window_open; only ever raised (atomicMax).
    struct WinPost { // a window handed to the writer (when its output slot is let go: host/way_out.h)
        int slot;
        u64 len; // bytes in the output slot: the tail of the window before (gzip out) and this window's output
        bool last;
    };
    std::mutex win_mu;
    std::deque<WinPost> win_posted;
    std::atomic<size_t> win_n_posted{0}, win_released{0};
    std::atomic<bool> win_no_more{false};
    std::atomic<int> win_stop{0}; // the way home gives up (HomeLink::stop): this thread found a cause, or the writer did
    int w_rc = YACRD_OK;          // the writer's code and message: fail() speaks on the thread that calls it
    std::string w_msg;
    Streams lanes;                // the mover's copy streams: made by the first window, kept for the run
    Events cdone;                 // behind a window's copy pass and its words' way home, per output slot

    void writer_fail(int code, const char *msg)
    {
        if (w_rc == YACRD_OK) w_rc = code, w_msg = msg;
        win_stop = 1;
    }
    // the way out on the writer thread: its failures are kept, not spoken
    bool went(yout::Result r)
    {
        const char *msg;
        if (const int code = out_says(r, &msg)) writer_fail(code, msg);
        return r == yout::kWent;
    }
    // the writer thread: one, in order
    void window_writer()
    {
        if (hipSetDevice(e->device) != hipSuccess) writer_fail(YACRD_ENODEV, "sequence editor: a HIP call failed");
        for (size_t k = 0; !win_stop.load(); k++) {
            while (win_n_posted.load(std::memory_order_acquire) <= k && !win_no_more.load() && !win_stop.load()) {
                struct timespec ts = {0, 50000};
                nanosleep(&ts, nullptr);
            }
            if (win_n_posted.load(std::memory_order_acquire) <= k || win_stop.load()) break;
            WinPost p;
            {
                std::lock_guard<std::mutex> g(win_mu);
                p = win_posted[k];
            }
            if (hipEventSynchronize(cdone[(size_t)p.slot]) != hipSuccess) {
                writer_fail(YACRD_ENODEV, "sequence editor: a HIP call failed");
                break;
            }
            // the per-window check: what the copy pass stored against what the scans counted, before a byte of the window leaves
            if (h_ctl[8 + 2 * p.slot] || h_ctl[8 + 2 * p.slot + 1] != p.len) {
                writer_fail(YACRD_EINTERNAL, "sequence editor: the copy pass stored other bytes than the plan counted");
                break;
            }
            const double t0 = now_ms();
            const char *base = S.wout[p.slot].as<char>();
            if (!job.gzip) {
                if (!went(out.home(base, p.len))) break;
                win_released.store(k + 1, std::memory_order_release);
            } else {
                // every whole block of the slot (the last window: its tail too, and the EOF member), batch by batch; the batch
                // before comes home while this one is encoded — the last batch of a window while the next window's first is.
                // The slot is released by the fetch of its last batch; a window that encodes nothing, at once
                const u64 whole = p.last ? p.len : p.len / ydf::kBlock * ydf::kBlock;
                if (!went(out.text(reinterpret_cast<const unsigned char *>(base), whole, p.last, (long)k)) || (p.last && !went(out.drain()))) break;
            }
            out_busy_ms += now_ms() - t0;
        }
        od.quiet();
    }

    struct WinAt { // window k as its kernels see it: bytes [lo, hi) of text slot ts, tiles [t_lo, t_hi), its control words
        bool last;
        int ts;
        u64 lo, hi;
        u32 t_lo, t_hi;
        unsigned long long *ctl;
    };
    // A window's records numbered, by format.  Behind the first wait — n_lines is known, the engine's stream is empty — the
    // window's tables are sized; then the line index and what is the format's own in front of the plan, the carry kernel
    // last.  Leaves the plan's bracket open (`ok`).  FASTQ: n_rec follows from n_lines.
    int window_records(yk::Fastq, const WinAt &w, bool &ok)
    {
        if (w.last && n_lines % 4) return fail(YACRD_EFALLBACK, "the line count is no multiple of four: the host loop decides");
        n_rec = n_lines / 4;
        HIP_TRY(S.line_end.reserve((size_t)(n_lines + 1) * sizeof(u64)));
        if (const int rc = reserve_record_tables()) return rc;
        ga.line_end = S.line_end.as<u64>(), ga.n_lines = n_lines;
        ga.tile0 = w.t_lo;
        ok = ev_open();
        if (w.t_hi > w.t_lo) hipLaunchKernelGGL(yk::sq_index_kernel, dim3(w.t_hi - w.t_lo), dim3(yk::kGpT), 0, e->stream, ga); // (BGZF in: a window of no bytes at all)
        if (!w.last) { // (the last window: its lines are whole records and its last byte is a newline — nothing is left)
            yk::SqCarry c{ga.line_end, n_rec, w.lo, w.hi, W, ga.text, S.wtext[w.ts ^ 1].as<unsigned char>(), w.ctl};
            hipLaunchKernelGGL(yk::sq_carry_kernel, dim3(64), dim3(256), 0, e->stream, c);
        }
        return YACRD_OK;
    }
    // FASTA: index, mark and the two line scans, then a wait of its own — the window's headers H —: n_rec = H in the last
    // window and where a header's partial line ends the window, else H - 1 (the record behind the last header waits); then
    // heads, widths and the carry
    int window_records(yk::Fasta, const WinAt &w, bool &ok)
    {
        if (!room_for((double)n_lines * 32.0, held_line_tables())) return no_room_message();
        if (const int rc = reserve_line_tables()) return rc;
        ga.n_lines = n_lines, ga.n_rec = 0, ga.tile0 = w.t_lo;
        fa.hi = w.last ? 0 : w.hi;
        const dim3 line_grid((u32)((n_lines + 255) / 256));
        ok = ev_open();
        if (w.t_hi > w.t_lo) hipLaunchKernelGGL(yk::sq_index_kernel, dim3(w.t_hi - w.t_lo), dim3(yk::kGpT), 0, e->stream, ga);
        if (n_lines) hipLaunchKernelGGL(yk::fa_mark_kernel, line_grid, dim3(256), 0, e->stream, args(yk::Fasta{}));
        if (const int rc = scan_u32_to_u64(e, fa.head, n_lines, S.ln_rec.as<u64>(), S.part)) return rc;
        if (const int rc = scan_u32_to_u64(e, fa.bases, n_lines, S.base_before.as<u64>(), S.part)) return rc;
        ok = ok && ev_close();
        if (const int rc = bring_words(ok, {S.ln_rec.as<u64>() + n_lines, w.ctl, w.ctl + 3})) return rc;
        const u64 n_head = h_ctl[0];
        const bool open_head = h_ctl[2] != 0; // the partial last line is the next record's header: every record of the window is whole
        win_seen_head = win_seen_head || n_head != 0;
        if (h_ctl[1] & yk::kSqNeedHost) return fail(YACRD_EFALLBACK, "a line longer than the device editor's offsets: the host loop decides");
        n_rec = w.last || open_head || !n_head ? n_head : n_head - 1;
        if (!room_for((double)n_rec * 40.0, held_record_tables())) return no_room_message();
        HIP_TRY(S.rec_line.reserve((size_t)(n_rec + 1) * sizeof(u64)));
        HIP_TRY(S.rec_width.reserve((size_t)(n_rec + 1) * sizeof(u32)));
        if (const int rc = reserve_record_tables()) return rc;
        fa.rec_line = S.rec_line.as<u64>(), fa.rec_width = S.rec_width.as<u32>(), fa.n_head = n_head;
        ok = ev_open();
        if (n_lines) hipLaunchKernelGGL(yk::fa_heads_kernel, line_grid, dim3(256), 0, e->stream, args(yk::Fasta{}));
        if (n_lines && n_rec) hipLaunchKernelGGL(yk::fa_widths_kernel, line_grid, dim3(256), 0, e->stream, args(yk::Fasta{}));
        if (!w.last) {
            yk::FaCarry c{{ga.line_end, n_rec, w.lo, w.hi, W, ga.text, S.wtext[w.ts ^ 1].as<unsigned char>(), w.ctl}, fa.rec_line, n_head};
            hipLaunchKernelGGL(yk::fa_carry_kernel, dim3(64), dim3(256), 0, e->stream, c);
        }
        return YACRD_OK;
    }

    // BGZF in: window `c`'s bytes of the compressed stream into the one compressed slot, its members inflated into
    // the text slot's new bytes `dst` (one launch), the lines of the new tiles counted (one launch, avail = hi).  The engine's
    // code of what failed, like every phase.  No launch per landed chunk: the window is the unit.
    int inflate_window(const ybw::WindowCut &c, u64 k, char *dst, u64 hi, u32 w_tile, u32 t_hi, size_t chunk, bool &ok)
    {
        TextSource comp_src;
        comp_src.mem = job.bgzf;
        const double t0 = now_ms();
        // (c0 is any byte of the stream: the mover reads the source with memcpy into its pinned arena and stores from the slot's
        // first byte, which is 16-byte aligned — the copy kernel's only demand —, so nothing is rounded)
        const int moved = move_text(e, comp_src, c.c0, c.c1 - c.c0, reinterpret_cast<char *>(iw.comp), comp_fresh, job.n_threads, [](u64, u64, u64) {}, chunk, &lanes);
        comp_fresh = false;
        inf_h2d_ms += (float)(now_ms() - t0);
        if (const int rc = moved_code(moved)) return rc;
        if (iev.v.size() < 2 * (size_t)k + 2 && !iev.add(2 * (size_t)k + 2 - iev.v.size())) HIP_TRY(why_not_added());
        HIP_TRY(hipEventRecord(iev[2 * (size_t)k], e->stream));
        if (const int rc = inflate_device_run_window(e, iw, e->stream, job.members->data() + c.m0, c.m1 - c.m0, c.c0, c.c1, c.t0, c.t1,
                                                     reinterpret_cast<unsigned char *>(dst)))
            return rc;
        HIP_TRY(hipEventRecord(iev[2 * (size_t)k + 1], e->stream));
        n_iev = 2 * (size_t)k + 2;
        ga.avail = hi, ga.tile0 = w_tile;
        ok = ok && ev_open();
        if (t_hi > w_tile) hipLaunchKernelGGL(yk::sq_lines_kernel, dim3(t_hi - w_tile), dim3(yk::kGpT), 0, e->stream, ga);
        ok = ok && ev_close();
        return YACRD_OK;
    }
    // move_text's codes as the engine's, in one place
    static int moved_code(int moved)
    {
        if (moved == 2) return fail(YACRD_EINVAL, "read error in the sequence file");
        if (moved == 3) return fail(YACRD_ENOMEM, "sequence text to HBM: no pinned memory");
        if (moved) return fail(YACRD_ENODEV, "sequence editor: a HIP call failed");
        return YACRD_OK;
    }

    // window by window on this thread; the code of what it found, or the writer's
    template <class Format>
    int windows_loop()
    {
        using Piece = typename Format::Piece;
        const bool bz = job.bgzf != nullptr; // the new bytes are inflated into the slot, window cuts[k] (plan), not moved
        const u64 n_win = bz ? (u64)cuts.size() : (n + W - 1) / W;
        const size_t chunk = (size_t)std::min<u64>(kTextChunk, W);
        const u32 w_tile = (u32)(W / yk::kGpTile);
        u64 carry = 0, tail = 0, tail_at = 0; // of the window before: its carry; its ragged output tail and where it lies in its slot
        u64 sum_rec = 0, sum_pieces = 0, sum_total = 0, max_carry = 0;
        double text_ms = 0;
        for (u64 k = 0; k < n_win; k++) {
            if (win_stop.load()) return YACRD_OK; // (the writer's code: run_windows)
            const bool last = k + 1 == n_win;
            const int ts = (int)(k & 1), os = (int)(k & 1);
            const u64 n_new = bz ? cuts[k].t1 - cuts[k].t0 : std::min(W, n - k * W), lo = W - carry, hi = W + n_new; // (BGZF in: n_new <= W, 0 too)
            const u32 t_lo = (u32)(lo / yk::kGpTile), t_hi = (u32)((hi + yk::kGpTile - 1) / yk::kGpTile);
            unsigned long long *ctl = S.ctl.as<unsigned long long>() + 8 * (k & 3);
            char *slot = S.wtext[ts].as<char>();
            HIP_TRY(hipMemsetAsync(ctl, 0, 64, e->stream));
            HIP_TRY(hipMemsetAsync(slot + hi, 0, 64, e->stream));
            ga.text = reinterpret_cast<const unsigned char *>(slot), ga.n = hi, ga.lo = lo, ga.ctl = ctl;
            ga.raw = nullptr, ga.out0 = 0, ga.piece0 = 0;
            bool ok = ev_open();
            if (t_lo < w_tile) { // the carry's tiles
                ga.avail = W, ga.tile0 = t_lo;
                hipLaunchKernelGGL(yk::sq_lines_kernel, dim3(w_tile - t_lo), dim3(yk::kGpT), 0, e->stream, ga);
            }
            ok = ok && ev_close();
            const double tm = now_ms();
            const int rc_new = bz ? inflate_window(cuts[k], k, slot + W, hi, w_tile, t_hi, chunk, ok) : moved_code(move_text(
                e, src, k * W, n_new, slot + W, win_fresh[ts], job.n_threads,
                [&](u64 seg_begin, u64 seg_end, u64 avail) {
                    const bool end = seg_end >= n_new;
                    const u32 t0 = w_tile + (u32)(seg_begin / yk::kGpTile), t1 = end ? t_hi : w_tile + (u32)(seg_end / yk::kGpTile);
                    ga.avail = end ? hi : W + std::min<u64>(avail, seg_end); // (a tile of this segment reads nothing behind it)
                    ga.tile0 = t0;
                    ok = ok && ev_open();
                    if (t1 > t0) hipLaunchKernelGGL(yk::sq_lines_kernel, dim3(t1 - t0), dim3(yk::kGpT), 0, e->stream, ga);
                    ok = ok && ev_close();
                },
                chunk, &lanes));
            win_fresh[ts] = false;
            text_ms += now_ms() - tm;
            if (rc_new) return rc_new;
            if (!ok) return fail(YACRD_ENODEV, "sequence editor: a HIP call failed");
            // the scan of the tiles' counts; the first wait: lines (BGZF in: and the decoder's status word, read before anything the text says)
            ga.avail = hi;
            ok = ev_open();
            if (const int rc = scan_u32_to_u64(e, S.tile_nl.as<u32>() + t_lo, (u64)(t_hi - t_lo), S.tile_l0.as<u64>() + t_lo, S.part)) return rc;
            ok = ok && ev_close();
            if (bz) {
                if (const int rc = bring_words(ok, {S.tile_l0.as<u64>() + t_hi, ctl, iw.status})) return rc;
                if ((u32)h_ctl[2]) return inflate_not_taken((u32)h_ctl[2]);
            } else if (const int rc = bring_words(ok, {S.tile_l0.as<u64>() + t_hi, ctl}))
                return rc;
            n_lines = h_ctl[0];
            if (h_ctl[1] & yk::kSqNeedHost) return fail(YACRD_EFALLBACK, "the text holds a CR: the host loop decides");
            // the window's tables (the engine's stream is empty: nothing reads the ones they replace), its records, its carry
            if (const int rc = window_records(Format{}, WinAt{last, ts, lo, hi, t_lo, t_hi, ctl}, ok)) return rc;
            launch_plan<Format, false>();
            if (const int rc = scan_u32_to_u64(e, ga.rec_pieces, n_rec, S.piece_off.as<u64>(), S.part)) return rc;
            if (const int rc = scan_u32_to_u64(e, ga.rec_bytes, n_rec, S.byte_off.as<u64>(), S.part)) return rc;
            ok = ok && ev_close();
            // the second wait (FASTA: the third): pieces, bytes, status, carry
            if (const int rc = bring_words(ok, {S.piece_off.as<u64>() + n_rec, S.byte_off.as<u64>() + n_rec, ctl, ctl + 2})) return rc;
            const u64 w_pieces = h_ctl[0], w_total = h_ctl[1];
            if (h_ctl[2] & yk::kSqCarryLong) // (FASTA with no whole header line so far: what was carried is no record)
                return fail(YACRD_EFALLBACK, std::is_same<Format, yk::Fasta>::value && !win_seen_head
                                                 ? "more than two windows in front of the first header's newline: the host loop's case"
                                                 : "a record longer than a window: the host loop's case");
            if (h_ctl[2] & yk::kSqNeedHost) return fail(YACRD_EFALLBACK, not_taken(Format{}));
            carry = last ? 0 : h_ctl[3];
            max_carry = std::max(max_carry, carry);
            // the output slot: the writer has let go of what window k - 2 left in it
            while (k >= 2 && win_released.load(std::memory_order_acquire) < k - 1 && !win_stop.load()) {
                struct timespec tsl = {0, 20000};
                nanosleep(&tsl, nullptr);
            }
            if (win_stop.load()) return YACRD_OK;
            const u64 raw = job.gzip ? tail : 0, len = raw + w_total;
            if (w_pieces + 1 >= 0x7FFFFFFFull) return fail(YACRD_EFALLBACK, "more output records than the device editor numbers");
            HIP_TRY(S.wout[os].reserve((size_t)((len + 15) & ~(u64)15) + 64)); // (grow-only, by the scanned total: FASTA written again may be longer than its text)
            HIP_TRY(S.pieces.reserve((size_t)(w_pieces + 2) * sizeof(Piece)));
            args(Format{}).pieces = S.pieces.as<Piece>(), ga.out = S.wout[os].as<unsigned char>();
            ga.n_pieces = w_pieces + (raw ? 1 : 0), ga.total = len;
            ga.raw = S.wout[os ^ 1].as<unsigned char>(), ga.out0 = raw, ga.piece0 = raw ? 1u : 0u;
            if (raw) { // piece 0: the tail of the window before, where it lies in that window's slot
                Piece *p0 = reinterpret_cast<Piece *>(const_cast<u64 *>(h_ctl + 12)) + os; // (pinned; window k - 2's copy has ended)
                *p0 = Format::raw_piece(tail_at, (u32)raw);
                HIP_TRY(hipMemcpyAsync(S.pieces.p, p0, sizeof *p0, hipMemcpyHostToDevice, e->stream));
            }
            ok = ev_open();
            if (len) {
                launch_plan<Format, true>();
                hipLaunchKernelGGL(yk::seq_copy_kernel<Format>, dim3((u32)((len + yk::kSqOutTile - 1) / yk::kSqOutTile)), dim3(yk::kGpT), 0, e->stream, args(Format{}));
            }
            ok = ok && ev_close();
            HIP_TRY(hipMemcpyAsync((void *)(h_ctl + 8 + 2 * os), ctl, 2 * sizeof(u64), hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipEventRecord(cdone[(size_t)os], e->stream));
            if (!ok) return fail(YACRD_ENODEV, "sequence editor: a HIP call failed");
            {
                std::lock_guard<std::mutex> g(win_mu);
                win_posted.push_back(WinPost{os, len, last});
            }
            win_n_posted.store((size_t)k + 1, std::memory_order_release);
            tail_at = last ? 0 : len / ydf::kBlock * ydf::kBlock, tail = job.gzip ? len - tail_at : 0;
            sum_rec += n_rec, sum_pieces += w_pieces, sum_total += w_total;
        }
        n_rec = sum_rec, n_pieces = sum_pieces, total = sum_total;
        win_count = n_win, win_max_carry = max_carry, win_text_ms = text_ms;
        return YACRD_OK;
    }

    bool win_fresh[2] = {false, false}; // a text slot that is a new allocation fills faster by copy kernel, once
    double win_text_ms = 0;
    u64 win_count = 0, win_max_carry = 0;
    bool win_seen_head = false; // FASTA: a window so far had a whole header line
    std::vector<ybw::WindowCut> cuts; // BGZF in: the windows (plan)
    InflateWindow iw;                 // the compressed slot, the status word
    bool comp_fresh = false;
    size_t n_iev = 0; // the events of `iev` that were recorded: a pair per window's inflate

    // the ring, the writer thread, the windows; then what the two threads found
    int run_windows()
    {
        for (int i = 0; i < 2; i++) {
            const void *before = S.wtext[i].p;
            HIP_TRY(S.wtext[i].reserve((size_t)(2 * W + 64)));
            win_fresh[i] = S.wtext[i].p != before;
            HIP_TRY(S.wout[i].reserve(64));
        }
        if (job.bgzf) {
            if (const int rcw = inflate_window_open(e, W, &iw)) return rcw;
            comp_fresh = iw.fresh;
        }
        if (!cdone.add(2, hipEventDisableTiming)) HIP_TRY(why_not_added());
        if (job.gzip)
            if (const int rcg = od.open(e, std::min<u64>(kGzBatchBlocks, 2 * W / ydf::kBlock + 2), true)) return rcg;
        od.stop = &win_stop, od.slots_below = &win_released;
        out.bind(S.pin.as<char>(), h_ctl + 4);
        std::thread wt([this] { window_writer(); });
        int rc = job.fasta ? windows_loop<yk::Fasta>() : windows_loop<yk::Fastq>();
        if (rc != YACRD_OK) win_stop = 1;
        win_no_more = true;
        wt.join();
        (void)hipStreamSynchronize(e->stream);
        if (rc == YACRD_OK && w_rc != YACRD_OK) rc = fail(w_rc, w_msg);
        if (rc != YACRD_OK) return rc;
        if ((job.gzip ? out.got != out.sent : sink.at != total)) return fail(YACRD_EINTERNAL, "sequence editor: fewer bytes written than counted");
        e->seq_windows[0] = win_count, e->seq_windows[1] = win_max_carry;
        e->seq_windows[2] = S.wtext[0].cap + S.wtext[1].cap + (job.bgzf ? inflate_window_held(e) : 0), e->seq_windows[3] = S.wout[0].cap + S.wout[1].cap;
        fill_gzip_stats(job.gzip_stats, total, sink.at, out.members, out.stored, od.kernel_ms(), out_busy_ms, out.put_ms);
        if (job.gunzip_stats) { // as the whole-text run fills them (deliver), summed over the windows' landings and launches
            for (size_t i = 0; i + 1 < n_iev; i += 2) inf_kernel_ms += ev_ms(iev[i], iev[i + 1]);
            yacrd_gunzip_stats &u = *job.gunzip_stats; // (walk_ms: the caller's)
            u.in_bytes = job.bgzf_bytes, u.out_bytes = n, u.n_members = job.members->size();
            u.h2d_ms = inf_h2d_ms, u.kernel_ms = inf_kernel_ms, u.d2h_ms = 0.f;
        }
        if (stats) {
            stats->text_bytes = n, stats->out_bytes = total, stats->n_records = n_rec, stats->n_out_records = n_pieces;
            stats->text_ms = (float)win_text_ms, stats->table_ms = (float)(t_table - t_start);
            float km = 0;
            for (size_t i = 0; i + 1 < n_ev; i += 2) km += ev_ms(ev[i], ev[i + 1]);
            stats->kernel_ms = km, stats->out_ms = (float)out_busy_ms;
        }
        return YACRD_OK;
    }

    int deliver()
    {
        const double t0 = now_ms();
        if (!job.gzip && sink.fd < 0 && !sink.mem) { // the memory form: the size is known now
            sink.mem = (char *)std::malloc((size_t)total + 1);
            if (!sink.mem) return fail(YACRD_ENOMEM, "host allocation failed");
        }
        // gzip out: batch b comes home while b + 1 is encoded
        if (job.gzip) out.text(S.out.as<unsigned char>(), total, true, yout::kNoTag);
        const char *msg;
        int rc = out_says(job.gzip ? out.drain() : out.home(S.out.as<char>(), total), &msg);
        if (rc) rc = fail(rc, msg);
        else if (!job.gzip && sink.at != total) rc = fail(YACRD_EINTERNAL, "sequence editor: fewer bytes written than counted");
        out_busy_ms = now_ms() - t0;
        if (rc) return rc;
        fill_gzip_stats(job.gzip_stats, total, sink.at, out.members, out.stored, od.kernel_ms(), out_busy_ms, out.put_ms);
        if (job.gunzip_stats) {
            yacrd_gunzip_stats &u = *job.gunzip_stats; // (walk_ms: the caller's)
            u.in_bytes = job.bgzf_bytes, u.out_bytes = n, u.n_members = job.members->size();
            u.h2d_ms = inf_h2d_ms, u.kernel_ms = inf_kernel_ms, u.d2h_ms = 0.f;
        }
        if (job.stream_stats) *job.stream_stats = job.stream->stats; // (d2h_ms 0: the text stays in HBM)
        if (stats) {
            stats->text_bytes = n, stats->out_bytes = total, stats->n_records = n_rec, stats->n_out_records = n_pieces;
            stats->text_ms = (float)(t_text - t_table), stats->table_ms = (float)(t_table - t_start);
            float k = 0;
            for (size_t i = 0; i + 1 < n_ev; i += 2) k += ev_ms(ev[i], ev[i + 1]);
            stats->kernel_ms = k, stats->out_ms = (float)out_busy_ms;
        }
        return YACRD_OK;
    }
};

int run_seq_edit(yacrd_engine *e, const SeqJob &job, const TextSource &src, u64 n, Sink &sink, yacrd_seq_edit_stats *stats)
{
    DeviceGuard guard(e->device);
    SeqEditScratch *S = scratch_of<SeqEditScratch>(e);
    if (!S) return fail(YACRD_ENOMEM, "host allocation failed");
    // The route.  A FASTQ or FASTA — its text in a file, in host memory or, BGZF in, the Σ ISIZE bytes its
    // members inflate to — runs in windows when the text is longer than a window and either the switch names a window or the
    // whole-text run finds no room; every other text runs whole.  BGZF in: a window ends where a member ends (bgzf_windows.h)
    // and is at least two tiles, the largest frame and the largest ISIZE.
    const u64 sw = e->seq_window;
    for (u64 &w : e->seq_windows) w = 0;
    const bool may_window = sw != UINT64_MAX;
    u64 W = sw == 0 || sw == UINT64_MAX ? (u64)(kTextChunk * kTextSeg) : (sw + yk::kGpTile - 1) / yk::kGpTile * yk::kGpTile;
    if (job.bgzf) W = std::max<u64>(W, (ybw::kMinWindow + yk::kGpTile - 1) / yk::kGpTile * yk::kGpTile);
    bool windows = may_window && n > W && (sw != 0 || kSeqWindowsWhenFits);
    // plain gzip in: the whole-text run only (its spans are cut where blocks begin, not where a window would end)
    if (job.stream && windows) return fail(YACRD_EFALLBACK, "a gzip text that would run in windows: the host reader streams it");
    auto finish = [&](SeqRun &r, int rc) {
        (void)hipStreamSynchronize(e->stream); // (whatever failed: nothing of this call is in flight when its events go)
        r.od.quiet();
        (void)hipGetLastError();
        return rc;
    };
    if (!windows) {
        SeqRun r{e, job, src, n, sink, stats, *S};
        int rc = r.plan();
        if (rc == YACRD_OK) rc = r.upload_table();
        if (rc == YACRD_OK) rc = r.move_and_count();
        if (rc == YACRD_OK) rc = r.size_output();
        if (rc == YACRD_OK) rc = r.gather();
        if (rc == YACRD_OK) rc = r.deliver();
        rc = finish(r, rc);
        // no room: nothing has left the device yet, and what the run holds goes before the windows take their ring
        if (!(rc == YACRD_EFALLBACK && r.room_failed && may_window && n > W) || job.stream) return rc;
        windows = true;
        if (job.fasta) // the whole text's tables, 32 bytes a line: a window sizes its own
            for (DevBuf *b : {&S->line_end, &S->ln_head, &S->ln_bases, &S->ln_rec, &S->base_before, &S->rec_line, &S->rec_width}) b->release();
    }
    S->text.release(), S->out.release(); // (the whole-text run's: the ring is what a run in windows holds)
    if (job.bgzf) inflate_device_release_whole(e); // (and the whole stream's buffer and member table in the inflate scratch)
    SeqRun r{e, job, src, n, sink, stats, *S};
    r.W = W;
    int rc = r.plan();
    if (rc == YACRD_OK) rc = r.upload_table();
    if (rc == YACRD_OK) rc = r.run_windows();
    return finish(r, rc);
}

int seq_edit_args(bool fasta, yacrd_engine *e, int op, const yacrd_report_table *t, yacrd_seq_edit_stats *st)
{
    if (!e) return fail(YACRD_EINVAL, "null argument");
    if (!t) return fail(YACRD_EINVAL, fasta ? "the FASTA editor takes a table (the resident form is not built)"
                                             : "the FASTQ editor takes a table (the resident form is not built)");
    if (op < 0 || op > 3) return fail(YACRD_EINVAL, "op: 0 = scrubb, 1 = filter, 2 = extract, 3 = split");
    if (st) std::memset(st, 0, sizeof(*st));
    if (e->pending.active || e->host_pending) return fail(YACRD_EINVAL, "the engine has a submitted batch pending");
    return YACRD_OK;
}

// util::get_file_type by name (src/util.rs:39-55), as far as it says FASTQ or FASTA: every other type's mark wins over ".fa"
bool named_as(bool fasta, const char *path)
{
    const std::string name(path);
    auto has = [&](const char *x) { return name.find(x) != std::string::npos; };
    if (has(".m4") || has(".mhap") || has(".paf") || has(".yacrd")) return false;
    const bool fastq = has(".fastq") || has(".fq");
    return fasta ? !fastq && (has(".fasta") || has(".fa")) : fastq;
}

// One call of a form: its job, where the text comes from and where the bytes go.  The forms share their front (enter, text_in)
// and their way out (leave).
struct SeqCall {
    yacrd_seq_edit_stats *st;
    yacrd_gzip_stats *gs;
    yacrd_gunzip_stats *us;
    yacrd_gunzip_stream_stats *ss = nullptr;
    StreamInflate stream;
    yacrd_engine *gz_engine = nullptr; // plain gzip in: the engine whose stream scratch this call filled
    SeqJob job;
    std::vector<yif::InfMember> members;
    TextSource src;
    Sink sink;

    // the stats zeroed, the arguments checked, the job named
    int enter(bool fasta, yacrd_engine *e, int op, const yacrd_report_table *t, bool gzip)
    {
        if (gs) std::memset(gs, 0, sizeof(*gs));
        if (us) std::memset(us, 0, sizeof(*us));
        if (ss) std::memset(ss, 0, sizeof(*ss));
        if (const int rc = seq_edit_args(fasta, e, op, t, st)) return rc;
        job.op = op, job.table = t, job.fasta = fasta, job.gzip = gzip, job.gzip_stats = gs;
        return YACRD_OK;
    }
    // the text in memory.  BGZF in: `text`, `n` are the compressed file; the walk — before a file is made beside an out_path:
    // what is not BGZF leaves nothing — fills `members` and the job's BGZF fields, and `n` becomes the text's bytes
    // Plain gzip in (`gz`, the _gz_ forms): the member goes up and is sized and chained on the device here (stream_inflate_open),
    // also before a file is made: what is not one gzip member, or a payload not taken as far as sizing tells, leaves nothing
    int text_in(yacrd_engine *e, const char *text, uint64_t &n, bool bgzf, bool gz)
    {
        if (gz) {
            DeviceGuard guard(e->device);
            SeqEditScratch *S = scratch_of<SeqEditScratch>(e);
            if (!S) return fail(YACRD_ENOMEM, "host allocation failed");
            gz_engine = e; // (from here on a call that fails gives the compressed bytes and the symbols back: leave)
            // beside the symbols: the text itself and an output that may be as long (the run's own plan() asks again, with the tables)
            const int rc = stream_inflate_open(e, text, n, job.n_threads, 2.0, (double)S->text.cap + (double)S->out.cap, &stream);
            (void)hipStreamSynchronize(e->stream);
            (void)hipGetLastError();
            if (rc) return rc;
            job.stream = &stream, job.stream_stats = ss;
            text = "", n = stream.text_bytes;
        }
        if (bgzf) {
            const double t0 = now_ms();
            u64 total = 0;
            if (!ybw::walk(reinterpret_cast<const unsigned char *>(text), n, members, &total)) return fail(YACRD_EFALLBACK, "not BGZF: the host reader's");
            if (us) us->walk_ms = (float)(now_ms() - t0);
            job.bgzf = text ? text : "", job.bgzf_bytes = n, job.members = &members, job.gunzip_stats = us;
            text = "", n = total;
        }
        src.mem = text ? text : "";
        return YACRD_OK;
    }
    // the way out: a call that failed leaves zeroed stats and no memory
    int leave(int rc)
    {
        if (rc == YACRD_OK) return rc;
        if (st) std::memset(st, 0, sizeof(*st));
        if (gs) std::memset(gs, 0, sizeof(*gs));
        if (us) std::memset(us, 0, sizeof(*us));
        if (ss) std::memset(ss, 0, sizeof(*ss));
        // plain gzip in: the caller takes the host route next, which wants the memory the compressed bytes and the symbols hold
        if (gz_engine) stream_inflate_release(gz_engine);
        if (sink.fd < 0) std::free(sink.mem), sink.mem = nullptr;
        return rc;
    }
    // the run, into a file written beside its place and moved there when every byte is in it: a text that is not for this
    // path leaves nothing behind
    int run_to_file(yacrd_engine *e, uint64_t n, const char *out_path)
    {
        yseg::BesideFile file;
        if (!file.open(out_path)) return fail(YACRD_EFALLBACK, std::string("cannot create a file beside ") + out_path + ": the host loop words the error");
        sink.fd = file.fd;
        int rc = run_seq_edit(e, job, src, n, sink, st);
        if (rc == YACRD_OK && !file.commit()) rc = fail(YACRD_EINVAL, "Error during writing of the output file");
        return leave(rc);
    }
};

// the forms, for FASTQ and for FASTA: a file to a file; memory to memory, gzip out or not; memory to a file, gzip out
int edit_seq_file(bool fasta, yacrd_engine *e, int op, const char *in_path, const char *out_path, int n_threads, const yacrd_report_table *t,
                  yacrd_seq_edit_stats *st)
{
    SeqCall c{st, nullptr, nullptr};
    if (const int rca = c.enter(fasta, e, op, t, false)) return rca;
    if (!in_path || !out_path) return fail(YACRD_EINVAL, "null argument");
    if (!named_as(fasta, in_path))
        return fail(YACRD_EFALLBACK, fasta ? "not a FASTA file by its name: the host loop's case" : "not a FASTQ file by its name: the host loop's case");
    const int fd = ::open(in_path, O_RDONLY);
    if (fd < 0) return fail(YACRD_EFALLBACK, std::string("cannot open ") + in_path + ": the host loop words the error");
    FdGuard fdg{fd};
    struct stat sst, ost;
    if (fstat(fd, &sst) != 0 || !S_ISREG(sst.st_mode)) return fail(YACRD_EFALLBACK, "not a regular file: the host loop reads it");
    if (is_compressed_magic(fd)) return fail(YACRD_EFALLBACK, "a compressed file: inflate it and take the gzip form, or the host loop");
    if (lstat(out_path, &ost) == 0) {
        if (!S_ISREG(ost.st_mode)) return fail(YACRD_EFALLBACK, "the output is not a regular file: the host loop writes it");
        if (ost.st_dev == sst.st_dev && ost.st_ino == sst.st_ino) return fail(YACRD_EFALLBACK, "input and output are one file: the host loop's case");
    }
    c.job.n_threads = n_threads;
    c.src.fd = fd;
    return c.run_to_file(e, (u64)sst.st_size, out_path);
}

int edit_seq_mem(bool fasta, yacrd_engine *e, int op, const char *text, uint64_t n, const yacrd_report_table *t, char **out, uint64_t *out_bytes,
                 yacrd_seq_edit_stats *st, bool gzip = false, yacrd_gzip_stats *gs = nullptr, bool bgzf = false, yacrd_gunzip_stats *us = nullptr,
                 bool gz = false, yacrd_gunzip_stream_stats *ss = nullptr)
{
    SeqCall c{st, gs, us, ss};
    if (const int rca = c.enter(fasta, e, op, t, gzip)) return rca;
    if ((!text && n) || !out || !out_bytes) return fail(YACRD_EINVAL, "null argument");
    *out = nullptr, *out_bytes = 0;
    if (const int rcw = c.text_in(e, text, n, bgzf, gz)) return gz ? c.leave(rcw) : rcw;
    if (gzip) { // (plain: the run sizes the memory when it knows the output's bytes)
        c.sink.cap = (size_t)(n / 3 + 4096); // (the sink grows when the members need more)
        c.sink.mem = (char *)std::malloc((size_t)c.sink.cap);
        if (!c.sink.mem) return fail(YACRD_ENOMEM, "host allocation failed");
    }
    if (const int rc = c.leave(run_seq_edit(e, c.job, c.src, n, c.sink, st))) return rc;
    *out = c.sink.mem, *out_bytes = c.sink.at;
    return YACRD_OK;
}

int edit_seq_gzip_file(bool fasta, yacrd_engine *e, int op, const char *text, uint64_t n, const yacrd_report_table *t, const char *out_path,
                       yacrd_seq_edit_stats *st, yacrd_gzip_stats *gs, bool bgzf = false, yacrd_gunzip_stats *us = nullptr, bool gz = false,
                       yacrd_gunzip_stream_stats *ss = nullptr)
{
    SeqCall c{st, gs, us, ss};
    if (const int rca = c.enter(fasta, e, op, t, true)) return rca;
    if ((!text && n) || !out_path) return fail(YACRD_EINVAL, "null argument");
    if (const int rcw = c.text_in(e, text, n, bgzf, gz)) return gz ? c.leave(rcw) : rcw;
    struct stat ost;
    if (lstat(out_path, &ost) == 0 && !S_ISREG(ost.st_mode)) return fail(YACRD_EFALLBACK, "the output is not a regular file: the host loop writes it");
    return c.run_to_file(e, n, out_path);
}

} // namespace

extern "C" {

int yacrd_debug_seq_window(yacrd_engine *e, uint64_t window_bytes)
{
    if (!e) return fail(YACRD_EINVAL, "null argument");
    e->seq_window = window_bytes;
    return YACRD_OK;
}
void yacrd_debug_seq_windows(const yacrd_engine *e, uint64_t out[4])
{
    for (int i = 0; i < 4; i++) out[i] = e ? e->seq_windows[i] : 0;
}

int yacrd_engine_edit_fastq(yacrd_engine *e, int op, const char *in_path, const char *out_path, int n_threads, const yacrd_report_table *t,
                            yacrd_seq_edit_stats *st)
{
    return edit_seq_file(false, e, op, in_path, out_path, n_threads, t, st);
}
int yacrd_engine_edit_fastq_mem(yacrd_engine *e, int op, const char *text, uint64_t n, const yacrd_report_table *t, char **out, uint64_t *out_bytes,
                                yacrd_seq_edit_stats *st)
{
    return edit_seq_mem(false, e, op, text, n, t, out, out_bytes, st);
}
int yacrd_engine_edit_fastq_gzip_mem(yacrd_engine *e, int op, const char *text, uint64_t n, const yacrd_report_table *t, char **out,
                                     uint64_t *out_bytes, yacrd_seq_edit_stats *st, yacrd_gzip_stats *gs)
{
    return edit_seq_mem(false, e, op, text, n, t, out, out_bytes, st, true, gs);
}
int yacrd_engine_edit_fastq_gzip_file(yacrd_engine *e, int op, const char *text, uint64_t n, const yacrd_report_table *t, const char *out_path,
                                      yacrd_seq_edit_stats *st, yacrd_gzip_stats *gs)
{
    return edit_seq_gzip_file(false, e, op, text, n, t, out_path, st, gs);
}

int yacrd_engine_edit_fasta(yacrd_engine *e, int op, const char *in_path, const char *out_path, int n_threads, const yacrd_report_table *t,
                            yacrd_seq_edit_stats *st)
{
    return edit_seq_file(true, e, op, in_path, out_path, n_threads, t, st);
}
int yacrd_engine_edit_fasta_mem(yacrd_engine *e, int op, const char *text, uint64_t n, const yacrd_report_table *t, char **out, uint64_t *out_bytes,
                                yacrd_seq_edit_stats *st)
{
    return edit_seq_mem(true, e, op, text, n, t, out, out_bytes, st);
}
int yacrd_engine_edit_fasta_gzip_mem(yacrd_engine *e, int op, const char *text, uint64_t n, const yacrd_report_table *t, char **out,
                                     uint64_t *out_bytes, yacrd_seq_edit_stats *st, yacrd_gzip_stats *gs)
{
    return edit_seq_mem(true, e, op, text, n, t, out, out_bytes, st, true, gs);
}
int yacrd_engine_edit_fasta_gzip_file(yacrd_engine *e, int op, const char *text, uint64_t n, const yacrd_report_table *t, const char *out_path,
                                      yacrd_seq_edit_stats *st, yacrd_gzip_stats *gs)
{
    return edit_seq_gzip_file(true, e, op, text, n, t, out_path, st, gs);
}

int yacrd_engine_edit_fastq_bgzf_mem(yacrd_engine *e, int op, const char *bgzf, uint64_t n, const yacrd_report_table *t, char **out,
                                     uint64_t *out_bytes, yacrd_seq_edit_stats *st, yacrd_gzip_stats *gs, yacrd_gunzip_stats *us)
{
    return edit_seq_mem(false, e, op, bgzf, n, t, out, out_bytes, st, true, gs, true, us);
}
int yacrd_engine_edit_fastq_bgzf_file(yacrd_engine *e, int op, const char *bgzf, uint64_t n, const yacrd_report_table *t, const char *out_path,
                                      yacrd_seq_edit_stats *st, yacrd_gzip_stats *gs, yacrd_gunzip_stats *us)
{
    return edit_seq_gzip_file(false, e, op, bgzf, n, t, out_path, st, gs, true, us);
}
int yacrd_engine_edit_fasta_bgzf_mem(yacrd_engine *e, int op, const char *bgzf, uint64_t n, const yacrd_report_table *t, char **out,
                                     uint64_t *out_bytes, yacrd_seq_edit_stats *st, yacrd_gzip_stats *gs, yacrd_gunzip_stats *us)
{
    return edit_seq_mem(true, e, op, bgzf, n, t, out, out_bytes, st, true, gs, true, us);
}
int yacrd_engine_edit_fasta_bgzf_file(yacrd_engine *e, int op, const char *bgzf, uint64_t n, const yacrd_report_table *t, const char *out_path,
                                      yacrd_seq_edit_stats *st, yacrd_gzip_stats *gs, yacrd_gunzip_stats *us)
{
    return edit_seq_gzip_file(true, e, op, bgzf, n, t, out_path, st, gs, true, us);
}

// plain gzip in: the _bgzf_ forms' arguments with yacrd_gunzip_stream_stats in place of yacrd_gunzip_stats
int yacrd_engine_edit_fastq_gz_mem(yacrd_engine *e, int op, const char *gz, uint64_t n, const yacrd_report_table *t, char **out,
                                   uint64_t *out_bytes, yacrd_seq_edit_stats *st, yacrd_gzip_stats *gs, yacrd_gunzip_stream_stats *ss)
{
    return edit_seq_mem(false, e, op, gz, n, t, out, out_bytes, st, true, gs, false, nullptr, true, ss);
}
int yacrd_engine_edit_fastq_gz_file(yacrd_engine *e, int op, const char *gz, uint64_t n, const yacrd_report_table *t, const char *out_path,
                                    yacrd_seq_edit_stats *st, yacrd_gzip_stats *gs, yacrd_gunzip_stream_stats *ss)
{
    return edit_seq_gzip_file(false, e, op, gz, n, t, out_path, st, gs, false, nullptr, true, ss);
}
int yacrd_engine_edit_fasta_gz_mem(yacrd_engine *e, int op, const char *gz, uint64_t n, const yacrd_report_table *t, char **out,
                                   uint64_t *out_bytes, yacrd_seq_edit_stats *st, yacrd_gzip_stats *gs, yacrd_gunzip_stream_stats *ss)
{
    return edit_seq_mem(true, e, op, gz, n, t, out, out_bytes, st, true, gs, false, nullptr, true, ss);
}
int yacrd_engine_edit_fasta_gz_file(yacrd_engine *e, int op, const char *gz, uint64_t n, const yacrd_report_table *t, const char *out_path,
                                    yacrd_seq_edit_stats *st, yacrd_gzip_stats *gs, yacrd_gunzip_stream_stats *ss)
{
    return edit_seq_gzip_file(true, e, op, gz, n, t, out_path, st, gs, false, nullptr, true, ss);
}

} // extern "C"
