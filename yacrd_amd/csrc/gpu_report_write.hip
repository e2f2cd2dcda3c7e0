// gpu_report_write.hip — the `.yacrd` report written on the GPU: sized, scanned and formatted in HBM
// (include/yacrd_engine.h: yacrd_engine_write_report / _mem).
//
// Reference: src/editor/mod.rs:61-83 (report), :102-107 (bad_region_format), :51-58 (as_str) behind src/main.rs:80-84.  The host
// writer (host/report.cc: yacrd_report_write) walks the reads on one thread, a division loop per number and a memcpy per id;
// here the host only brings the text home.  The format is the host writer's, byte for byte: one line per read, in table
// order, `{NotBad|Chimeric|NotCovered} \t id \t len \t piece;piece;... \n`, a piece `{end - begin as u32, wrapping},{begin},{end}`,
// plain decimal numbers, the id copied verbatim (any bytes, possibly none), no trailing ';', a read without regions ends "\t\n".
//
// On the device:
//   size   a thread per REGION: its read by binary search in bad_offsets (kept: owner[k]), the bytes of its piece, the ';' in
//          front of it counted in for every piece but its read's first (at most 33); a thread per READ: the bytes of its
//          head (type name, id, digits of len, three tabs) + 1 for the '\n'.  Digits are counted by compares.  The read pass
//          also checks the table: a type beyond 2, offsets that do not rise from 0 to the totals
//   scan   stream.hip's scan twice: P[k], the piece's position in the stream of pieces, H[r], the head's in the stream of heads.
//          Line r starts at H[r] + P[bad_offsets[r]]; piece k of read r at H[r + 1] - 1 + P[k] (the head's bytes but its '\n',
//          then the read's pieces in front of k).  The total, H[R] + P[G], is the text's size: one host sync, with the status
//   emit   heads: a thread per read writes type, id, len, the tabs and the line's '\n'; pieces: a thread per region writes its
//          piece back to front into the extent the size pass gave it.  A read of 100 000 regions is 100 000 threads' work
// Every store lies inside an extent the scans gave, and every thread sizes its text again before it stores: an extent that
// does not match, or that reaches beyond the total, sets a status bit (YACRD_EINTERNAL) and nothing is stored.  The arrays
// are read twice, 8 bytes per region and 12 per read are written beside the text.  The text then goes home in segments
// through two pinned buffers: segment i + 1 crosses the link while segment i is written.
#include "engine_internal.h"
#include "gpu_text.h"
#include "host/beside_file.h"
#include "host/segment_pump.h"

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <new>
#include <vector>

using namespace yke;

namespace yk {

constexpr u32 kRwBadType = 1u, kRwBadTable = 2u, kRwDisagree = 4u;

struct RwArgs {
    // the table
    const unsigned char *names;
    const u64 *name_off;
    const u32 *lengths;
    const u64 *bad_off;
    const uint2 *regions;
    const unsigned char *type;
    u32 n_reads;
    u64 n_regions, name_bytes;
    // the size pass and its scans
    u32 *piece_len, *owner, *head_len;
    const u64 *P, *H;
    // the text
    unsigned char *text;
    u64 total;
    u32 *status;
};

__device__ __forceinline__ u32 rw_digits(u32 v)
{
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) +
           (v >= 100000000u) + (v >= 1000000000u);
}
// the decimal digits of v, the last one at q[-1]; returns the first one's address
__device__ __forceinline__ unsigned char *rw_put_back(unsigned char *q, u32 v)
{
    do {
        *--q = (unsigned char)('0' + v % 10u);
        v /= 10u;
    } while (v);
    return q;
}
__device__ __forceinline__ u32 rw_piece_bytes(uint2 rg, bool first)
{
    return rw_digits(rg.y - rg.x) + rw_digits(rg.x) + rw_digits(rg.y) + 2u + (first ? 0u : 1u);
}
constexpr u64 rw_pack(const char *s, int n)
{
    u64 v = 0;
    for (int i = 0; i < n && i < 8; i++) v |= (u64)(unsigned char)s[i] << (8 * i);
    return v;
}
__device__ __forceinline__ u32 rw_type_bytes(u32 ty) { return ty == 0u ? 6u : ty == 1u ? 8u : 10u; }

// ---- size: a thread per region ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rw_piece_size_kernel(RwArgs a)
{
    const u64 k = (u64)blockIdx.x * 256u + threadIdx.x;
    if (k >= a.n_regions) return;
    // the last read whose regions begin at or in front of k (bad_off[0] = 0 <= k < bad_off[n_reads]: the read pass checks it;
    // whatever the offsets hold, lo and hi stay inside [0, n_reads])
    u32 lo = 0, hi = a.n_reads;
    while (hi - lo > 1u) {
        const u32 mid = lo + (hi - lo) / 2u;
        if (a.bad_off[mid] <= k) lo = mid;
        else hi = mid;
    }
    a.owner[k] = lo;
    a.piece_len[k] = rw_piece_bytes(a.regions[k], a.bad_off[lo] == k);
}

// ---- size: a thread per read; the table is checked here -----------------------------------------------------------------
__global__ __launch_bounds__(256) void rw_head_size_kernel(RwArgs a)
{
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.n_reads) return;
    u32 st = 0;
    const u32 ty = a.type[r];
    if (ty > 2u) st |= kRwBadType;
    const u64 o0 = a.bad_off[r], o1 = a.bad_off[r + 1], n0 = a.name_off[r], n1 = a.name_off[r + 1];
    if (o0 > o1 || o1 > a.n_regions || (r == 0u && o0 != 0) || (r + 1u == a.n_reads && o1 != a.n_regions)) st |= kRwBadTable;
    if (n0 > n1 || n1 > a.name_bytes || n1 - n0 > 0x7FFFFFFFull) st |= kRwBadTable;
    a.head_len[r] = st ? 0u : rw_type_bytes(ty) + (u32)(n1 - n0) + rw_digits(a.lengths[r]) + 4u;
    if (st) atomicOr(a.status, st);
}

// ---- emit: the heads and the line ends -----------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rw_head_emit_kernel(RwArgs a)
{
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.n_reads) return;
    const u64 h0 = a.H[r], h1 = a.H[r + 1], n0 = a.name_off[r], n1 = a.name_off[r + 1];
    const u64 line = h0 + a.P[a.bad_off[r]], next = h1 + a.P[a.bad_off[r + 1]];
    const u32 ty = a.type[r], len = a.lengths[r];
    const u32 tl = rw_type_bytes(ty), idl = (u32)(n1 - n0);
    const u64 want = (u64)tl + idl + rw_digits(len) + 4u;
    if (ty > 2u || n1 < n0 || n1 > a.name_bytes || want != h1 - h0 || next > a.total || next < line || next - line < want) {
        atomicOr(a.status, kRwDisagree); // (the size and the emit pass disagree: nothing is stored)
        return;
    }
    unsigned char *p = a.text + line;
    const u64 w = ty == 0u ? rw_pack("NotBad", 6) : ty == 1u ? rw_pack("Chimeric", 8) : rw_pack("NotCover", 8);
    for (u32 i = 0; i < (tl < 8u ? tl : 8u); i++) p[i] = (unsigned char)(w >> (8u * i));
    if (ty == 2u) p[8] = 'e', p[9] = 'd';
    p += tl;
    *p++ = '\t';
    const unsigned char *id = a.names + n0;
    for (u32 i = 0; i < idl; i++) p[i] = id[i];
    p += idl;
    *p++ = '\t';
    p += rw_digits(len);
    (void)rw_put_back(p, len);
    *p = '\t';
    a.text[next - 1] = '\n';
}

// ---- emit: a thread per region -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rw_piece_emit_kernel(RwArgs a)
{
    const u64 k = (u64)blockIdx.x * 256u + threadIdx.x;
    if (k >= a.n_regions) return;
    const u32 r = a.owner[k];
    if (r >= a.n_reads) {
        atomicOr(a.status, kRwDisagree);
        return;
    }
    const uint2 rg = a.regions[k];
    const bool first = a.bad_off[r] == k;
    const u64 p0 = a.P[k], p1 = a.P[k + 1];
    const u32 len = rw_piece_bytes(rg, first);
    const u64 start = a.H[r + 1] - 1u + p0; // (H[r + 1] >= 1: every head counts its line's '\n')
    if (p1 - p0 != len || a.H[r + 1] == 0 || start + len >= a.total || start + len < start) { // (>=: the '\n' lies behind)
        atomicOr(a.status, kRwDisagree);
        return;
    }
    unsigned char *q = a.text + start + len;
    q = rw_put_back(q, rg.y);
    *--q = ',';
    q = rw_put_back(q, rg.x);
    *--q = ',';
    q = rw_put_back(q, rg.y - rg.x); // (u32, wrapping: `b.1 - b.0` in release)
    if (!first) *--q = ';';
}

} // namespace yk

namespace {

constexpr u64 kReportSegment = (u64)64 << 20; // bytes of text per trip home

// YACRD_TEST_REPORT_SEGMENT=<bytes> (tests; include/yacrd_engine_debug.h), read at call time
u64 report_segment()
{
    const char *ev = std::getenv("YACRD_TEST_REPORT_SEGMENT");
    if (ev && *ev) {
        char *end = nullptr;
        const unsigned long long v = std::strtoull(ev, &end, 10);
        if (end && !*end && v >= 1 && v <= ((u64)1 << 30)) return (u64)v;
    }
    return kReportSegment;
}

struct ReportWriteScratch { // the writer's buffers; they stay with the engine (grow-only), go with yacrd_engine_trim / destroy
    static constexpr yacrd_engine::Slot kScratchSlot = yacrd_engine::kReportWrite;
    DevBuf names, name_off, lengths, bad_off, regions, type, piece_len, owner, head_len, P, H, text, ctl, part;
    PinBuf pin; // two segments
    Events ev;  // 3, made by the first call: in front of the upload, behind it, behind the kernels
    Events dma; // 2, untimed: a pinned buffer has landed
};

using yseg::Sink; // where the text goes: a file descriptor or memory sized for it (host/segment_pump.h)

// The table -> its text in S.text; *total its size.  Nothing has left the device when this returns.
int format_report(yacrd_engine *e, ReportWriteScratch &S, const yacrd_report_table *t, u64 *total, yacrd_report_write_stats *st)
{
    *total = 0;
    if (!S.ev.add(3 - S.ev.v.size()) || !S.dma.add(2 - S.dma.v.size(), hipEventDisableTiming)) HIP_TRY(why_not_added());
    yk::RwArgs a{};
    u64 R = 0, G = 0;
    HIP_TRY(hipEventRecord(S.ev[0], e->stream));
    if (!t) {
        if (!e->resident.valid || !e->has_result || e->resident.n_reads != e->last_reads || e->resident.lengths != e->in_len.as<u32>())
            return fail(YACRD_EFALLBACK, "no ingest's table is resident on this engine: hand the table over, or take the host writer");
        R = e->last_reads, G = e->last_regions;
        a.names = e->resident.names, a.name_off = e->resident.name_off, a.lengths = e->resident.lengths;
        a.bad_off = e->bad_offsets.as<u64>(), a.regions = e->bad_regions.as<uint2>(), a.type = e->read_type.as<unsigned char>();
        if (R >= 0x7FFFFFFFull || G >= 0x7FFFFFFFull) return fail(YACRD_EFALLBACK, "more reads or regions than the device report writer takes");
        if (R) HIP_TRY(hipMemcpyAsync(&a.name_bytes, a.name_off + R, sizeof(u64), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
    } else {
        R = t->n_reads;
        if (R && (!t->name_off || !t->lengths || !t->bad_offsets || !t->read_type)) return fail(YACRD_EINVAL, "the report table is incomplete");
        G = R ? t->bad_offsets[R] : 0;
        a.name_bytes = R ? t->name_off[R] : 0;
        if ((G && !t->bad_regions) || (a.name_bytes && !t->names)) return fail(YACRD_EINVAL, "the report table is incomplete");
        if (R >= 0x7FFFFFFFull || G >= 0x7FFFFFFFull) return fail(YACRD_EFALLBACK, "more reads or regions than the device report writer takes");
        if (R) {
            HIP_TRY(S.names.reserve((size_t)a.name_bytes + 64));
            HIP_TRY(S.name_off.reserve((size_t)(R + 1) * sizeof(u64)));
            HIP_TRY(S.lengths.reserve((size_t)R * sizeof(u32)));
            HIP_TRY(S.bad_off.reserve((size_t)(R + 1) * sizeof(u64)));
            HIP_TRY(S.regions.reserve((size_t)(G + 1) * sizeof(uint2)));
            HIP_TRY(S.type.reserve((size_t)R + 64));
            if (a.name_bytes)
                if (const int rch = h2d(e, S.names.p, t->names, (size_t)a.name_bytes)) return rch;
            if (const int rch = h2d(e, S.name_off.p, t->name_off, (size_t)(R + 1) * sizeof(u64))) return rch;
            if (const int rch = h2d(e, S.lengths.p, t->lengths, (size_t)R * sizeof(u32))) return rch;
            if (const int rch = h2d(e, S.bad_off.p, t->bad_offsets, (size_t)(R + 1) * sizeof(u64))) return rch;
            if (G)
                if (const int rch = h2d(e, S.regions.p, t->bad_regions, (size_t)G * sizeof(uint2))) return rch;
            if (const int rch = h2d(e, S.type.p, t->read_type, (size_t)R)) return rch;
        }
        a.names = S.names.as<unsigned char>(), a.name_off = S.name_off.as<u64>(), a.lengths = S.lengths.as<u32>();
        a.bad_off = S.bad_off.as<u64>(), a.regions = S.regions.as<uint2>(), a.type = S.type.as<unsigned char>();
    }
    HIP_TRY(hipEventRecord(S.ev[1], e->stream));
    a.n_reads = (u32)R, a.n_regions = G;
    if (st) st->n_reads = R, st->n_regions = G, st->resident = t ? 0u : 1u;
    if (!R) {
        HIP_TRY(hipEventRecord(S.ev[2], e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        return YACRD_OK;
    }
    // ---- size + scan
    HIP_TRY(S.piece_len.reserve((size_t)(G + 1) * sizeof(u32)));
    HIP_TRY(S.owner.reserve((size_t)(G + 1) * sizeof(u32)));
    HIP_TRY(S.head_len.reserve((size_t)(R + 1) * sizeof(u32)));
    HIP_TRY(S.P.reserve((size_t)(G + 2) * sizeof(u64)));
    HIP_TRY(S.H.reserve((size_t)(R + 2) * sizeof(u64)));
    HIP_TRY(S.ctl.reserve(64));
    HIP_TRY(hipMemsetAsync(S.ctl.p, 0, 64, e->stream));
    a.piece_len = S.piece_len.as<u32>(), a.owner = S.owner.as<u32>(), a.head_len = S.head_len.as<u32>();
    a.P = S.P.as<u64>(), a.H = S.H.as<u64>();
    a.status = S.ctl.as<u32>();
    const u32 rgrid = (u32)((R + 255) / 256), ggrid = (u32)((G + 255) / 256);
    hipLaunchKernelGGL(yk::rw_head_size_kernel, dim3(rgrid), dim3(256), 0, e->stream, a);
    if (G) hipLaunchKernelGGL(yk::rw_piece_size_kernel, dim3(ggrid), dim3(256), 0, e->stream, a);
    if (const int rcs = scan_u32_to_u64(e, S.head_len.as<u32>(), R, S.H.as<u64>(), S.part)) return rcs;
    if (const int rcs = scan_u32_to_u64(e, S.piece_len.as<u32>(), G, S.P.as<u64>(), S.part)) return rcs;
    u64 h_heads = 0, h_pieces = 0;
    u32 h_status = 0;
    HIP_TRY(hipMemcpyAsync(&h_heads, S.H.as<u64>() + R, sizeof(u64), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(&h_pieces, S.P.as<u64>() + G, sizeof(u64), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(&h_status, S.ctl.p, sizeof(u32), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipGetLastError());
    if (h_status & yk::kRwBadType) return fail(YACRD_EFALLBACK, "a read's type is none of the three: the host writer words the error");
    if (h_status & yk::kRwBadTable)
        return fail(YACRD_EFALLBACK, "bad_offsets or name_off do not rise from 0 to their totals: the host writer takes the table as it is");
    if (h_pieces > 33 * G || h_heads < 11 * R) return fail(YACRD_EINTERNAL, "device report writer: a size beyond what a line can hold");
    a.total = h_heads + h_pieces;
    // ---- emit
    HIP_TRY(S.text.reserve((size_t)a.total + 64)); // (YACRD_ENOMEM when it does not fit: nothing has been written)
    a.text = S.text.as<unsigned char>();
    hipLaunchKernelGGL(yk::rw_head_emit_kernel, dim3(rgrid), dim3(256), 0, e->stream, a);
    if (G) hipLaunchKernelGGL(yk::rw_piece_emit_kernel, dim3(ggrid), dim3(256), 0, e->stream, a);
    HIP_TRY(hipEventRecord(S.ev[2], e->stream));
    HIP_TRY(hipMemcpyAsync(&h_status, S.ctl.p, sizeof(u32), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipGetLastError());
    if (h_status) return fail(YACRD_EINTERNAL, "device report writer: the size and the emit pass disagree");
    *total = a.total;
    return YACRD_OK;
}

// S.text[0, total) -> the sink, a segment at a time: segment i + 1 crosses the link while segment i is written
int send_home(yacrd_engine *e, ReportWriteScratch &S, u64 total, Sink &sink, double *out_ms)
{
    if (!total) return YACRD_OK;
    const u64 seg = std::min<u64>(report_segment(), total);
    HIP_TRY(S.pin.reserve((size_t)(2 * seg)));
    // (the loop and its segment arithmetic: host/segment_pump.h, which a stand-alone program runs under the sanitizers)
    HomeLink dma{S.text.as<char>(), e->stream, {S.dma[0], S.dma[1]}};
    const int rc = yseg::pump(total, seg, S.pin.as<char>(), dma, sink, [&](auto put) {
        const double t0 = now_ms();
        put();
        *out_ms += now_ms() - t0;
    });
    if (rc == yseg::kLinkFailed) HIP_TRY(dma.bad);
    if (rc == yseg::kSinkFailed) return fail(YACRD_EINVAL, "Error while writing the yacrd report");
    return YACRD_OK;
}

int write_args(yacrd_engine *e, yacrd_report_write_stats *st)
{
    if (!e) return fail(YACRD_EINVAL, "null argument");
    if (st) std::memset(st, 0, sizeof(*st));
    if (e->pending.active || e->host_pending) return fail(YACRD_EINVAL, "the engine has a submitted batch pending");
    return YACRD_OK;
}

void fill_stats(ReportWriteScratch &S, u64 total, double out_ms, yacrd_report_write_stats *st)
{
    if (!st) return;
    st->text_bytes = total;
    st->up_ms = ev_ms(S.ev[0], S.ev[1]);
    st->kernel_ms = ev_ms(S.ev[1], S.ev[2]);
    st->out_ms = (float)out_ms;
    (void)hipGetLastError();
}

} // namespace

extern "C" {

int yacrd_engine_write_report(yacrd_engine *e, const yacrd_report_table *t, const char *out_path, yacrd_report_write_stats *st)
{
    if (const int rca = write_args(e, st)) return rca;
    if (!out_path) return fail(YACRD_EINVAL, "null argument");
    // the output: written beside its place and moved there when the last byte is in.  Anything but a new or a regular file
    // is the host writer's, and so is a place where no file can be created: it owns the message.
    // The host writer truncates an existing file in place; the rename below replaces it.  Where that would show — a file that
    // may not be written, or one with further hard links — the host writer takes it; an existing file's mode is kept.
    struct stat ost;
    const bool exists = lstat(out_path, &ost) == 0;
    if (exists && !S_ISREG(ost.st_mode)) return fail(YACRD_EFALLBACK, "the output is not a regular file: the host writer writes it");
    if (exists && (ost.st_nlink > 1 || ::access(out_path, W_OK) != 0))
        return fail(YACRD_EFALLBACK, "the output may not be written or has other hard links: the host writer writes it in place");
    // (the file is made first: a place where none can be created costs no pass over the table)
    yseg::BesideFile file; // (gone again on every way out but the last)
    if (!file.open(out_path, exists ? &ost : nullptr))
        return fail(YACRD_EFALLBACK, std::string("cannot create a file beside ") + out_path + ": the host writer words the error");
    DeviceGuard guard(e->device);
    ReportWriteScratch *Sp = scratch_of<ReportWriteScratch>(e);
    u64 total = 0;
    if (const int rcf = Sp ? format_report(e, *Sp, t, &total, st) : fail(YACRD_ENOMEM, "host allocation failed")) {
        (void)hipGetLastError();
        if (st) std::memset(st, 0, sizeof(*st));
        return rcf;
    }
    Sink sink;
    sink.fd = file.fd;
    double out_ms = 0;
    int rc = send_home(e, *Sp, total, sink, &out_ms);
    if (rc == YACRD_OK && !file.commit()) rc = fail(YACRD_EINVAL, "Error while writing the yacrd report");
    if (rc != YACRD_OK) {
        if (st) std::memset(st, 0, sizeof(*st));
        return rc;
    }
    fill_stats(*Sp, total, out_ms, st);
    return YACRD_OK;
}

int yacrd_engine_write_report_mem(yacrd_engine *e, const yacrd_report_table *t, char **out, uint64_t *out_bytes, yacrd_report_write_stats *st)
{
    if (const int rca = write_args(e, st)) return rca;
    if (!out || !out_bytes) return fail(YACRD_EINVAL, "null argument");
    *out = nullptr, *out_bytes = 0;
    DeviceGuard guard(e->device);
    ReportWriteScratch *Sp = scratch_of<ReportWriteScratch>(e);
    if (!Sp) return fail(YACRD_ENOMEM, "host allocation failed");
    u64 total = 0;
    int rc = format_report(e, *Sp, t, &total, st);
    Sink sink;
    if (rc == YACRD_OK) {
        sink.mem = (char *)std::malloc((size_t)total + 1);
        if (!sink.mem) rc = fail(YACRD_ENOMEM, "host allocation failed");
    }
    double out_ms = 0;
    if (rc == YACRD_OK) rc = send_home(e, *Sp, total, sink, &out_ms);
    if (rc != YACRD_OK) {
        (void)hipGetLastError();
        std::free(sink.mem);
        if (st) std::memset(st, 0, sizeof(*st));
        return rc;
    }
    *out = sink.mem, *out_bytes = total;
    fill_stats(*Sp, total, out_ms, st);
    return YACRD_OK;
}

} // extern "C"
