// gpu_report.hip — a `.yacrd` report read on the GPU: parse, dedupe and classify in HBM
// (include/yacrd_engine.h: yacrd_engine_ingest_report / _mem).
//
// Reference: FromReport (src/stack.rs:176-257; parse_bad_string, :217-241) behind src/main.rs:43-60 — a report stands in for
// the overlap file, the regions come from it and type_of_read is redone with this run's -n.  The host reader
// (host/editors.cc: yacrd_report_read) does that on one thread with a string per column and a hash probe per line; here
// the host only MOVES the text (gpu_text.h: the parser's mover) and fetches the arrays.  The rule is the host reader's, bit
// for bit: lines cut at '\n', one trailing '\r' stripped, empty lines skipped; `type \t id \t len \t body`, the type ignored,
// the id any bytes (none is legal), len non-empty decimal digits <= 2^32 - 1, the body everything behind the third tab; every
// ';'-separated piece needs two commas, its first field is not looked at, the second and third are non-empty decimal u32,
// whatever follows a third comma is ignored, an empty piece (a body that ends in ';') is corrupt.  An id seen again REPLACES
// the earlier row's length and regions and keeps its position; reads come out in first-appearance order.
// A '\r' that is not the last byte of its line is no more special here than there: it is part of the id, or of an ignored
// field, or a bad digit — reproduced, not a fall-back of its own.
//
// On the device:
//   count    per segment as it lands: a thread takes the line starts of its 128 bytes, a tile (32 KiB) its number of
//            non-empty lines; stream.hip's scan gives every tile the ordinal of its first line — ordinals are dense and in
//            file order, which is what lets "first" and "last" be a min and a max
//   parse    (the whole text, when the last byte has landed and the number of lines is known) a thread per line start:
//            the three tabs, len, the body validated piece by piece and its pieces counted; the id hashed (gp_hash) and
//            interned by text position in an open-addressing table (a slot holds the position of the id's first claimant,
//            ids are compared in the text); per slot atomicMin / atomicMax of the line's ordinal: first appearance, winner
//   number   a flag per line "I am my id's first line", scanned: the reads' numbers.  No sort: the ordinals are sorted
//   gather   the winner line of every id writes its read's length, region count, id and body positions
//   scan     region counts -> bad_offsets[R + 1], id lengths -> name_off[R + 1]
//   fill     a thread per read: the body parsed into bad_regions, the id copied into names
//   classify classify_csr_kernel (plan_compact.h) on the arrays where they lie
// The text is read three times (count; parse; fill reads winners' bodies and ids again), nothing but the result arrays
// and 44 bytes per line + 16 per table slot + 32 per read is written.  Every loop over text is bounded by the text's end.  A line that
// does not fit the rule sets a status bit and the call returns YACRD_EFALLBACK with nothing returned: the caller runs
// yacrd_report_read, which words the error with its line number.  Because parse and fill run over the whole text, no line
// can reach beyond what has landed; a line is never too long for this path, only slow (one thread walks it).
#include "engine_internal.h"
#include "gpu_text.h"

#include <cstdio>
#include <cstdlib>

using namespace yke;

namespace yk {

constexpr u32 kRpNeedHost = 1u, kRpTableFull = 2u;
constexpr u64 kRpEmpty = ~0ull;

struct RpLine { // per non-empty line, by ordinal
    u64 id_pos;   // the id's first byte (the byte behind the first tab)
    u64 body_pos; // the byte behind the third tab
    u32 len;
    u32 n_reg;
};

struct RpArgs {
    const unsigned char *text;
    u64 n;               // bytes of text
    u32 tile0, tile1;    // the launch's tiles
    u32 *tile_lines;     // per tile: non-empty lines that start in it
    const u64 *tile_ord; // per tile: ordinal of its first non-empty line
    RpLine *lines;
    u32 *line_slot; // per line: its id's table slot
    u32 *line_idlen;
    u64 *claim;     // per slot: id position of the first claimant, kRpEmpty = free
    u32 *first;     // per slot: smallest ordinal
    u32 *last;      // per slot: largest ordinal
    u32 mask;
    u64 n_lines;
    u32 *status;
};

// bit i of s[h]: a non-empty line starts at byte lo + 64 h + i — one that is neither "" nor "\r" up to its '\n' or the text's end (lo: a multiple of 128; the mirror is padded by 64 zero bytes,
// a 16-byte piece is loaded when its first byte lies in the text)
__device__ __forceinline__ void rp_starts(const unsigned char *t, u64 n, u64 lo, u64 s[2])
{
    s[0] = s[1] = 0;
    if (lo >= n) return;
    u64 nl[2] = {0, 0}, cr[2] = {0, 0};
#pragma unroll
    for (u32 j = 0; j < 8; j++) {
        if (lo + 16u * j >= n) break;
        const uint4 v = *reinterpret_cast<const uint4 *>(t + lo + 16u * j);
        nl[j >> 2] |= (u64)gp_eq16(v, '\n') << (16u * (j & 3u));
        cr[j >> 2] |= (u64)gp_eq16(v, '\r') << (16u * (j & 3u));
    }
    const u64 left = n - lo;
    const u64 v0 = left >= 64 ? ~0ull : ((1ull << left) - 1ull);
    const u64 v1 = left >= 128 ? ~0ull : left > 64 ? ((1ull << (left - 64)) - 1ull) : 0ull;
    const u64 prev = (lo == 0 || t[lo - 1] == '\n') ? 1ull : 0ull;
    // nn: the byte behind this one is a newline, or the text's end
    const u64 top = (left <= 128 || t[lo + 128] == '\n') ? 1ull : 0ull;
    u64 nn0 = (nl[0] >> 1) | (nl[1] << 63), nn1 = (nl[1] >> 1) | (top << 63);
    if (left <= 64) nn0 |= 1ull << (left - 1);
    else if (left <= 128) nn1 |= 1ull << (left - 65);
    s[0] = ((nl[0] << 1) | prev) & v0 & ~(nl[0] | (cr[0] & nn0));
    s[1] = ((nl[1] << 1) | (nl[0] >> 63)) & v1 & ~(nl[1] | (cr[1] & nn1));
}

// ---- count: non-empty lines per tile ------------------------------------------------------------------------------
__global__ __launch_bounds__(kGpT) void rp_count_kernel(RpArgs a)
{
    __shared__ u32 sc[kGpT / 64];
    const u32 gt = a.tile0 + blockIdx.x;
    const u64 lo = (u64)gt * (u64)kGpTile + (u64)threadIdx.x * 128u;
    u64 s[2];
    rp_starts(a.text, a.n, lo, s);
    u32 total = 0;
    (void)block_excl_add<kGpT>((u32)__popcll(s[0]) + (u32)__popcll(s[1]), sc, total);
    if (threadIdx.x == 0) a.tile_lines[gt] = total;
}

// decimal digits [p, q) -> v; false: empty, a byte that is no digit, or beyond u32
__device__ __forceinline__ bool rp_u32(const unsigned char *t, u64 p, u64 q, u32 &v)
{
    if (p >= q) return false;
    u64 x = 0;
    for (; p < q; p++) {
        const u32 d = (u32)t[p] - (u32)'0';
        if (d > 9u) return false;
        x = x * 10u + d;
        if (x > 0xFFFFFFFFull) return false;
    }
    v = (u32)x;
    return true;
}

// One piece "x,begin,end[,...]" that starts at p inside a body that ends at e (exclusive).  Returns the position of the
// ';' that ends it, or e; ok = false when it is corrupt.
__device__ __forceinline__ u64 rp_piece(const unsigned char *t, u64 p, u64 e, bool &ok, u32 &bgn, u32 &end)
{
    u64 c1 = e, c2 = e, c3 = e, q = p;
    u32 commas = 0;
    for (; q < e; q++) {
        const u32 c = t[q];
        if (c == ';') break;
        if (c == ',') {
            if (commas == 0) c1 = q;
            else if (commas == 1) c2 = q;
            else if (commas == 2) c3 = q;
            commas++;
        }
    }
    if (commas < 2) {
        ok = false;
        return q;
    }
    const u64 end_hi = commas >= 3 ? c3 : q;
    ok = rp_u32(t, c1 + 1, c2, bgn) && rp_u32(t, c2 + 1, end_hi, end);
    return q;
}

// ---- parse: every non-empty line's columns, its id interned ---------------------------------------------------------
__global__ __launch_bounds__(kGpT) void rp_parse_kernel(RpArgs a)
{
    __shared__ u32 sc[kGpT / 64];
    const u32 gt = a.tile0 + blockIdx.x;
    const u64 lo = (u64)gt * (u64)kGpTile + (u64)threadIdx.x * 128u;
    const unsigned char *t = a.text;
    u64 s[2];
    rp_starts(t, a.n, lo, s);
    u32 total = 0;
    u32 rank = block_excl_add<kGpT>((u32)__popcll(s[0]) + (u32)__popcll(s[1]), sc, total);
    u64 ord = a.tile_ord[gt] + rank;
    u32 status = 0;
    const GpBytes text{t};
#pragma unroll 1
    for (int h = 0; h < 2; h++) {
        u64 todo = s[h];
        while (todo) {
            const u32 bit = (u32)__builtin_ctzll(todo);
            todo &= todo - 1;
            const u64 p = lo + (u64)h * 64u + bit;
            const u64 o = ord++;
            if (o >= a.n_lines) { // (count and parse disagree: nothing is written)
                status |= kRpTableFull;
                continue;
            }
            // the line's end (exclusive), one trailing CR stripped, and its first three tabs
            u64 e = p, t1 = 0, t2 = 0, t3 = 0;
            u32 tabs = 0;
            for (; e < a.n; e++) {
                const u32 c = t[e];
                if (c == '\n') break;
                if (c == '\t') {
                    if (tabs == 0) t1 = e;
                    else if (tabs == 1) t2 = e;
                    else if (tabs == 2) t3 = e;
                    tabs++;
                }
            }
            if (e > p && t[e - 1] == '\r') e--; // (never a tab: the tabs found lie in front of it)
            RpLine ln;
            ln.id_pos = 0, ln.body_pos = 0, ln.len = 0, ln.n_reg = 0;
            u32 slot = 0, idlen = 0;
            bool ok = tabs >= 3 && rp_u32(t, t2 + 1, t3, ln.len);
            if (ok && t2 - t1 - 1 > 0x7FFFFFFFull) ok = false;
            if (ok) {
                ln.id_pos = t1 + 1, ln.body_pos = t3 + 1;
                idlen = (u32)(t2 - t1 - 1);
                // the body: pieces counted and checked
                if (ln.body_pos < e) {
                    u64 q = ln.body_pos;
                    for (;;) {
                        u32 b0, b1;
                        bool pok;
                        q = rp_piece(t, q, e, pok, b0, b1);
                        if (!pok) {
                            ok = false;
                            break;
                        }
                        ln.n_reg++;
                        if (q >= e) break;
                        q++; // behind the ';' (q == e now: an empty piece follows, corrupt)
                    }
                }
            }
            if (ok) {
                // intern: the slot whose claimant's id equals this line's
                u32 sl = (u32)gp_hash(text, ln.id_pos, idlen) & a.mask;
                u32 probes = 0;
                for (;;) {
                    u64 cur = a.claim[sl];
                    if (cur == kRpEmpty) {
                        cur = atomicCAS((unsigned long long *)&a.claim[sl], (unsigned long long)kRpEmpty, (unsigned long long)ln.id_pos);
                        if (cur == kRpEmpty) cur = ln.id_pos;
                    }
                    bool same = cur == ln.id_pos;
                    if (!same && cur + idlen < a.n && t[cur + idlen] == '\t') { // (an id holds no tab: the claimant's ends where ours does, or differs)
                        u32 i = 0;
                        while (i < idlen && t[cur + i] == t[ln.id_pos + i]) i++;
                        same = i == idlen;
                    }
                    if (same) break;
                    sl = (sl + 1u) & a.mask;
                    if (++probes > a.mask) { // (cannot happen: the table has two slots per line)
                        ok = false;
                        status |= kRpTableFull;
                        break;
                    }
                }
                slot = sl;
            }
            if (ok) {
                atomicMin(&a.first[slot], (u32)o);
                atomicMax(&a.last[slot], (u32)o);
            } else
                status |= kRpNeedHost;
            a.lines[o] = ln;
            a.line_slot[o] = slot;
            a.line_idlen[o] = idlen;
        }
    }
    status = wave_or(status);
    if (status && lane_id() == 0) atomicOr(a.status, status);
}

// ---- number: "this line is the first of its id" -------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rp_flag_kernel(const u32 *line_slot, const u32 *first, u64 n_lines, u32 *flag)
{
    const u64 o = (u64)blockIdx.x * 256u + threadIdx.x;
    if (o >= n_lines) return;
    flag[o] = first[line_slot[o]] == (u32)o ? 1u : 0u;
}

struct RpRead { // per read, from its winner line
    u64 id_pos, body_pos;
};

// ---- gather: every id's last line fills in its read -----------------------------------------------------------------------
__global__ __launch_bounds__(256) void rp_gather_kernel(const RpLine *lines, const u32 *line_slot, const u32 *line_idlen, const u32 *first,
                                                        const u32 *last, const u64 *number, u64 n_lines, RpRead *reads, u32 *lengths,
                                                        u32 *n_reg, u32 *name_len)
{
    const u64 o = (u64)blockIdx.x * 256u + threadIdx.x;
    if (o >= n_lines) return;
    const u32 sl = line_slot[o];
    if (last[sl] != (u32)o) return;
    const u64 r = number[first[sl]];
    const RpLine ln = lines[o];
    RpRead rd;
    rd.id_pos = ln.id_pos, rd.body_pos = ln.body_pos;
    reads[r] = rd;
    lengths[r] = ln.len;
    n_reg[r] = ln.n_reg;
    name_len[r] = line_idlen[o];
}

// ---- fill: the winners' bodies -> bad_regions, their ids -> names -------------------------------------------------------------
__global__ __launch_bounds__(256) void rp_fill_kernel(const unsigned char *t, u64 n, const RpRead *reads, const u32 *n_reg, const u64 *bad_off,
                                                      const u64 *name_off, u32 n_reads, uint2 *regions, unsigned char *names, u32 *status)
{
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_reads) return;
    const RpRead rd = reads[r];
    const u64 no = name_off[r], nlen = name_off[r + 1] - no;
    for (u64 i = 0; i < nlen && rd.id_pos + i < n; i++) names[no + i] = t[rd.id_pos + i];
    const u32 want = n_reg[r];
    if (want == 0u) return;
    u64 e = rd.body_pos;
    while (e < n && t[e] != '\n') e++;
    if (e > rd.body_pos && t[e - 1] == '\r') e--;
    u64 q = rd.body_pos;
    const u64 at = bad_off[r];
    u32 k = 0;
    bool ok = true;
    for (; k < want && q < e; k++) { // (bounded by the count of the parse pass: nothing is written beyond the read's share)
        u32 b0 = 0, b1 = 0;
        bool pok;
        q = rp_piece(t, q, e, pok, b0, b1);
        ok = ok && pok;
        regions[at + k] = make_uint2(b0, b1);
        q++;
    }
    if (!ok || k != want) atomicOr(status, 4u); // (the two passes disagree)
}

} // namespace yk

namespace {

struct ReportScratch { // the reader's buffers; they stay with the engine (grow-only), go with yacrd_engine_trim / destroy
    static constexpr yacrd_engine::Slot kScratchSlot = yacrd_engine::kReport;
    DevBuf text, tile_lines, tile_ord, lines, line_slot, line_idlen, claim, first, last, flag, number, reads, n_reg, name_len, name_off, names,
        ctl, part;
    double held() const // bytes of HBM the scratch holds now (read_report's "does it fit?")
    {
        double sum = 0;
        for (const DevBuf *b : {&text, &tile_lines, &tile_ord, &lines, &line_slot, &line_idlen, &claim, &first, &last, &flag, &number, &reads, &n_reg,
                                &name_len, &name_off, &names, &ctl, &part})
            sum += (double)b->cap;
        return sum;
    }
};

// (the text: plain, or a BGZF stream inflated in HBM as it lands — gpu_text.h: TextProducer)
int read_report(yacrd_engine *e, TextProducer tp, u64 n, int n_threads, double not_coverage, yacrd_result *out, yacrd_reads *reads,
                yacrd_ingest_stats *stats)
{
    DeviceGuard guard(e->device);
    ReportScratch *Sp = scratch_of<ReportScratch>(e);
    if (!Sp) return fail(YACRD_ENOMEM, "host allocation failed");
    ReportScratch &S = *Sp;
    e->mirror.valid = false; // (the engine's last ingest is no overlap ingest any more: no overlap text is resident)
    e->resident.valid = e->input.valid = false;
    const double t_start = now_ms();
    const u64 n_tiles = (n + yk::kGpTile - 1) / yk::kGpTile;
    if (n_tiles >= 0x7FFFFFFFull) return fail(YACRD_EFALLBACK, "file too large for the device report reader");
    {
        // HBM: the text, 32 bytes per line and 32 per two table slots (a line is rarely shorter than 20 bytes: about 4 x the
        // text at the worst), the arrays of the result.  Answered before anything is allocated.
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            const double have = (double)free_b + S.held() + (tp.bgzf ? (double)inflate_device_held(e) : 0.0);
            if (5.0 * (double)n + (tp.bgzf ? tp.bgzf->device_bytes() : 0.0) + (double)((size_t)256 << 20) > have)
                return fail(YACRD_EFALLBACK, "the report is too large to be read in this device's free memory: the host reader streams it");
        }
    }
    const void *mirror_before = S.text.p;
    HIP_TRY(S.text.reserve((size_t)n + 64));
    const bool blit = S.text.p != mirror_before; // (a fresh mirror fills faster by copy kernel: gpu_paf.hip)
    HIP_TRY(hipMemsetAsync(S.text.as<char>() + n, 0, 64, e->stream));
    HIP_TRY(S.tile_lines.reserve((size_t)(n_tiles + 1) * sizeof(u32)));
    HIP_TRY(S.tile_ord.reserve((size_t)(n_tiles + 2) * sizeof(u64)));
    HIP_TRY(S.ctl.reserve(64));
    HIP_TRY(hipMemsetAsync(S.ctl.p, 0, 64, e->stream));
    yk::RpArgs ga{};
    ga.text = S.text.as<unsigned char>();
    ga.n = n;
    ga.tile_lines = S.tile_lines.as<u32>();
    ga.tile_ord = S.tile_ord.as<u64>();
    ga.status = S.ctl.as<u32>();

    // ---- the text: every segment's lines are counted as it lands
    if (n || tp.bgzf) { // (a BGZF stream of no text still has members to be taken)
        int rc_open = YACRD_OK;
        const int bad = tp.move(e, 0, n, S.text.as<char>(), blit, n_threads, [&](u64 seg_begin, u64 seg_end, u64) {
            const u32 t0 = (u32)(seg_begin / yk::kGpTile), t1 = seg_end >= n ? (u32)n_tiles : (u32)(seg_end / yk::kGpTile);
            ga.tile0 = t0, ga.tile1 = t1;
            // (a line start's blankness looks one byte ahead: the chunk behind the segment has landed, gpu_text.h)
            if (t1 > t0) hipLaunchKernelGGL(yk::rp_count_kernel, dim3(t1 - t0), dim3(yk::kGpT), 0, e->stream, ga);
        }, &rc_open);
        if (rc_open) return rc_open;
        if (bad == 2) return fail(YACRD_EINVAL, "read error in the report");
        if (bad == 3) return fail(YACRD_ENOMEM, "report text to HBM: no pinned memory");
        if (bad) return fail(YACRD_ENODEV, "report text to HBM: a HIP call failed");
    }
    if (const int rcs = scan_u32_to_u64(e, S.tile_lines.as<u32>(), n_tiles, S.tile_ord.as<u64>(), S.part)) return rcs;
    u64 n_lines = 0;
    u32 inflate_status = 0; // (with the line count, before anything is sized from what the text says)
    if (const int rci = tp.fetch_inflate_status(e, &inflate_status)) return rci;
    HIP_TRY(hipMemcpyAsync(&n_lines, S.tile_ord.as<u64>() + n_tiles, sizeof(u64), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipGetLastError());
    const double t_text = now_ms();
    if (inflate_status) return inflate_not_taken(inflate_status);
    if (n_lines >= 0x7FFFFFFFull) return fail(YACRD_EFALLBACK, "too many lines for the device report reader");

    // ---- parse + intern
    u64 cap = 1024;
    while (cap < 2 * n_lines) cap <<= 1;
    HIP_TRY(S.lines.reserve((size_t)(n_lines + 1) * sizeof(yk::RpLine)));
    HIP_TRY(S.line_slot.reserve((size_t)(n_lines + 1) * sizeof(u32)));
    HIP_TRY(S.line_idlen.reserve((size_t)(n_lines + 1) * sizeof(u32)));
    HIP_TRY(S.flag.reserve((size_t)(n_lines + 1) * sizeof(u32)));
    HIP_TRY(S.number.reserve((size_t)(n_lines + 2) * sizeof(u64)));
    HIP_TRY(S.claim.reserve((size_t)cap * sizeof(u64)));
    HIP_TRY(S.first.reserve((size_t)cap * sizeof(u32)));
    HIP_TRY(S.last.reserve((size_t)cap * sizeof(u32)));
    HIP_TRY(hipMemsetAsync(S.claim.p, 0xFF, (size_t)cap * sizeof(u64), e->stream));
    HIP_TRY(hipMemsetAsync(S.first.p, 0xFF, (size_t)cap * sizeof(u32), e->stream));
    HIP_TRY(hipMemsetAsync(S.last.p, 0, (size_t)cap * sizeof(u32), e->stream));
    ga.lines = S.lines.as<yk::RpLine>();
    ga.line_slot = S.line_slot.as<u32>(), ga.line_idlen = S.line_idlen.as<u32>();
    ga.claim = S.claim.as<u64>(), ga.first = S.first.as<u32>(), ga.last = S.last.as<u32>();
    ga.mask = (u32)(cap - 1);
    ga.n_lines = n_lines;
    ga.tile0 = 0, ga.tile1 = (u32)n_tiles;
    const u32 lg = (u32)((n_lines + 255) / 256);
    if (n_lines) {
        hipLaunchKernelGGL(yk::rp_parse_kernel, dim3((u32)n_tiles), dim3(yk::kGpT), 0, e->stream, ga);
        hipLaunchKernelGGL(yk::rp_flag_kernel, dim3(lg), dim3(256), 0, e->stream, S.line_slot.as<u32>(), S.first.as<u32>(), n_lines, S.flag.as<u32>());
    }
    if (const int rcs = scan_u32_to_u64(e, S.flag.as<u32>(), n_lines, S.number.as<u64>(), S.part)) return rcs;
    u64 R = 0;
    u32 h_status = 0;
    HIP_TRY(hipMemcpyAsync(&R, S.number.as<u64>() + n_lines, sizeof(u64), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(&h_status, S.ctl.p, sizeof(u32), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipGetLastError());
    if (h_status & yk::kRpTableFull) return fail(YACRD_EINTERNAL, "device report reader: the count and the parse pass disagree");
    if (h_status & yk::kRpNeedHost)
        return fail(YACRD_EFALLBACK, "a line of the report is not `type, id, length, regions` as the reader wants them (columns, a digit, a "
                                     "number beyond u32, an empty piece): the host reader words the error");
    if (R > n_lines) return fail(YACRD_EINTERNAL, "device report reader: more reads than lines");
    const double t_parse = now_ms();

    // ---- the reads: winners gathered, offsets scanned, regions and names filled, types
    HIP_TRY(S.reads.reserve((size_t)(R + 1) * sizeof(yk::RpRead)));
    HIP_TRY(S.n_reg.reserve((size_t)(R + 1) * sizeof(u32)));
    HIP_TRY(S.name_len.reserve((size_t)(R + 1) * sizeof(u32)));
    HIP_TRY(S.name_off.reserve((size_t)(R + 2) * sizeof(u64)));
    HIP_TRY(e->in_len.reserve((size_t)(R + 1) * sizeof(u32)));
    HIP_TRY(e->bad_offsets.reserve((size_t)(R + 2) * sizeof(u64)));
    HIP_TRY(e->read_type.reserve((size_t)R + 64));
    e->has_result = false;
    if (n_lines)
        hipLaunchKernelGGL(yk::rp_gather_kernel, dim3(lg), dim3(256), 0, e->stream, S.lines.as<yk::RpLine>(), S.line_slot.as<u32>(),
                           S.line_idlen.as<u32>(), S.first.as<u32>(), S.last.as<u32>(), S.number.as<u64>(), n_lines, S.reads.as<yk::RpRead>(),
                           e->in_len.as<u32>(), S.n_reg.as<u32>(), S.name_len.as<u32>());
    if (const int rcs = scan_u32_to_u64(e, S.n_reg.as<u32>(), R, e->bad_offsets.as<u64>(), S.part)) return rcs;
    if (const int rcs = scan_u32_to_u64(e, S.name_len.as<u32>(), R, S.name_off.as<u64>(), S.part)) return rcs;
    u64 G = 0, name_bytes = 0;
    HIP_TRY(hipMemcpyAsync(&G, e->bad_offsets.as<u64>() + R, sizeof(u64), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(&name_bytes, S.name_off.as<u64>() + R, sizeof(u64), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (G > n || name_bytes > n) return fail(YACRD_EINTERNAL, "device report reader: more regions or name bytes than text");
    HIP_TRY(e->bad_regions.reserve((size_t)(G + 1) * sizeof(uint2)));
    HIP_TRY(S.names.reserve((size_t)name_bytes + 64));
    if (R) {
        hipLaunchKernelGGL(yk::rp_fill_kernel, dim3((u32)((R + 255) / 256)), dim3(256), 0, e->stream, ga.text, n, S.reads.as<yk::RpRead>(),
                           S.n_reg.as<u32>(), e->bad_offsets.as<u64>(), S.name_off.as<u64>(), (u32)R, e->bad_regions.as<uint2>(),
                           S.names.as<unsigned char>(), S.ctl.as<u32>());
        if (const int rcc = classify_on_device(e, e->bad_offsets.as<u64>(), e->bad_regions.as<uint2>(), e->in_len.as<u32>(), (u32)R, not_coverage,
                                               e->read_type.as<uint8_t>()))
            return rcc;
    }
    HIP_TRY(hipMemcpyAsync(&h_status, S.ctl.p, sizeof(u32), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipGetLastError());
    if (h_status) return fail(YACRD_EINTERNAL, "device report reader: the parse and the fill pass disagree");
    const double t_build = now_ms();

    // ---- home
    if (const int rch = reads_to_host(e, reads, (u32)R, n_lines, e->in_len.p, S.name_off.p, S.names.p, name_bytes)) return rch;
    e->last_reads = R, e->last_regions = G, e->has_result = true;
    const int rc = fetch_result(e, out);
    if (rc) {
        yacrd_reads_free(reads);
        yacrd_result_free(out);
        return rc;
    }
    if (stats) {
        stats->text_bytes = n;
        stats->n_records = n_lines;
        stats->n_reads = R;
        stats->text_ms = (float)(t_text - t_start);
        stats->parse_ms = (float)(t_parse - t_text);
        stats->build_ms = (float)(t_build - t_parse);
        stats->run_ms = 0.f; // (the types are part of build_ms: one launch behind the fill)
        stats->d2h_ms = (float)(now_ms() - t_build);
    }
    // the table stays where it is: a report can be written from it (gpu_report_write.hip)
    e->resident.names = S.names.as<unsigned char>(), e->resident.name_off = S.name_off.as<u64>(), e->resident.lengths = e->in_len.as<u32>();
    e->resident.n_reads = R, e->resident.valid = true;
    return YACRD_OK;
}

int report_args(yacrd_engine *e, yacrd_result *out, yacrd_reads *reads, yacrd_ingest_stats *stats)
{
    if (!e || !out || !reads) return fail(YACRD_EINVAL, "null argument");
    e->resident.valid = e->input.valid = false;
    zero_outputs(out, reads, stats);
    if (e->pending.active || e->host_pending) return fail(YACRD_EINVAL, "the engine has a submitted batch pending");
    return YACRD_OK;
}

} // namespace

extern "C" {

int yacrd_engine_ingest_report(yacrd_engine *e, const char *path, int n_threads, double not_coverage, yacrd_result *out, yacrd_reads *reads,
                               yacrd_ingest_stats *stats)
{
    if (const int rca = report_args(e, out, reads, stats)) return rca;
    if (!path) return fail(YACRD_EINVAL, "null argument");
    const int fd = ::open(path, O_RDONLY);
    if (fd < 0) return fail(YACRD_EFALLBACK, std::string("cannot open ") + path + ": the host reader words the error");
    FdGuard fdg{fd};
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) return fail(YACRD_EFALLBACK, "not a regular file: the host reader reads it");
    if (is_compressed_magic(fd))
        return fail(YACRD_EFALLBACK, "a compressed file: inflate it (yacrd_text_from_file + yacrd_engine_ingest_report_mem) or take the host reader");
    TextSource src;
    src.fd = fd;
    return read_report(e, src, (u64)st.st_size, n_threads, not_coverage, out, reads, stats);
}

int yacrd_engine_ingest_report_mem(yacrd_engine *e, const char *text, uint64_t n_bytes, int n_threads, double not_coverage, yacrd_result *out,
                                   yacrd_reads *reads, yacrd_ingest_stats *stats)
{
    if (const int rca = report_args(e, out, reads, stats)) return rca;
    if (!text && n_bytes) return fail(YACRD_EINVAL, "null argument");
    TextSource src;
    src.mem = text ? text : "";
    return read_report(e, src, n_bytes, n_threads, not_coverage, out, reads, stats);
}

int yacrd_engine_ingest_report_bgzf_mem(yacrd_engine *e, const char *bgzf, uint64_t n_bytes, int n_threads, double not_coverage, yacrd_result *out,
                                        yacrd_reads *reads, yacrd_ingest_stats *stats, yacrd_gunzip_stats *us)
{
    if (const int rca = report_args(e, out, reads, stats)) return rca;
    if (us) std::memset(us, 0, sizeof(*us));
    if (!bgzf && n_bytes) return fail(YACRD_EINVAL, "null argument");
    BgzfIn in;
    if (const int rcw = in.walk(bgzf, n_bytes)) return rcw;
    TextProducer tp;
    tp.bgzf = &in;
    const int rc = read_report(e, tp, in.text_bytes, n_threads, not_coverage, out, reads, stats);
    {
        DeviceGuard guard(e->device);
        (void)hipStreamSynchronize(e->stream); // (whatever failed: nothing of this call is in flight when its events go)
        (void)hipGetLastError();
        if (rc == YACRD_OK) in.stats(us);
    }
    return rc;
}

} // extern "C"
