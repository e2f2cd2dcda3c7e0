// gpu_deflate.hip — gzip output compressed on the GPU: text in HBM -> a BGZF stream in HBM (include/yacrd_engine.h:
// yacrd_engine_gzip_mem, yacrd_gzip_writer_*).
//
//   encode   one 256-thread workgroup per block of 65 280 bytes: deflate_block.h (the block, its parse and every table
//            in LDS, 153 KiB: one workgroup per CU), the member into the block's 64 KiB slot, its size into sizes[]
//   scan     stream.hip's device-wide exclusive scan over the members' sizes
//   pack     a workgroup moves its member to its place in the stream: 16-byte stores at the DESTINATION's alignment, every
//            dword of them funnel-shifted out of two dwords of the slot; the last workgroup writes the EOF member
// The host side moves a segment (a whole number of blocks) through a pinned buffer to the device, lets it be compressed
// while the caller fills the next buffer, and fetches the members when the next segment is due.
#include "engine_internal.h"
#include "gpu_text.h"
#include "deflate_block.h"
#include "host/beside_file.h"
#include "host/segment_pump.h"

#include <cstdio>
#include <cstdlib>

using namespace yke;

namespace yk {

__global__ __launch_bounds__(256) void df_encode_kernel(const unsigned char *text, u64 n, unsigned char *slots, u32 *sizes,
                                                        unsigned long long *ctl)
{
    __shared__ ydf::DfShared sh;
    const u64 b = blockIdx.x;
    const u64 lo = b * (u64)ydf::kBlock;
    if (lo >= n) return; // (uniform)
    const u32 len = (u32)min((u64)ydf::kBlock, n - lo);
    __shared__ u32 wg_is_stored;
    ydf::df_encode_block(sh, text + lo, len, slots + b * (u64)ydf::kSlot, sizes + b, &wg_is_stored);
    if (threadIdx.x == 0 && wg_is_stored) atomicAdd(ctl, 1ull);
}

// member b: slots[b * 64 KiB, + sizes[b]) -> out[off[b], ...); workgroup n_members (when launched): the EOF member
__global__ __launch_bounds__(256) void df_pack_kernel(const unsigned char *slots, const u32 *sizes, const u64 *off, u32 n_members,
                                                      unsigned char *out)
{
    const u32 b = blockIdx.x;
    const u64 dst0 = off[b];
    if (b >= n_members) {
        if (threadIdx.x < ydf::kEofBytes) out[dst0 + threadIdx.x] = (unsigned char)ydf::df_eof_byte(threadIdx.x);
        return;
    }
    // a member is at most header + stored block + trailer bytes: 65 311.  The wide path below reads up to 4 bytes behind the
    // member (the fifth dword, when source and destination differ in alignment), which then still lies in the member's slot.
    constexpr u32 kMaxMember = ydf::kHdr + 5 + ydf::kBlock + ydf::kTrailer;
    static_assert(kMaxMember + 4 <= ydf::kSlot, "the pack's fifth dword stays in the slot");
    const u32 size = min(sizes[b], kMaxMember);
    const unsigned char *src = slots + (u64)b * ydf::kSlot;
    const u32 *sw = reinterpret_cast<const u32 *>(src);
    const u32 shift = (u32)(dst0 & 15u);
    unsigned char *base = out + (dst0 - shift);
    const u32 end = shift + size;
    for (u32 q = threadIdx.x * 16u; q < end; q += 256u * 16u) {
        if (q >= shift && q + 16u <= end) {
            const u32 s = q - shift, wi = s >> 2, r = (s & 3u) * 8u;
            u32 w[5];
#pragma unroll
            for (int j = 0; j < 4; j++) w[j] = sw[wi + j];
            w[4] = r ? sw[wi + 4] : 0u; // (bytes [4 wi + 16, 4 wi + 20) with 4 wi + 16 < s + 16 <= size <= kMaxMember)
            uint4 v;
            if (r) v = make_uint4((w[0] >> r) | (w[1] << (32 - r)), (w[1] >> r) | (w[2] << (32 - r)), (w[2] >> r) | (w[3] << (32 - r)),
                                  (w[3] >> r) | (w[4] << (32 - r)));
            else v = make_uint4(w[0], w[1], w[2], w[3]);
            *reinterpret_cast<uint4 *>(base + q) = v;
        } else
            for (u32 k = max(q, shift); k < min(q + 16u, end); k++) base[k] = src[k - shift];
    }
}

} // namespace yk

namespace {

constexpr u64 kDefaultSegBlocks = 512;
constexpr u64 kMaxSegBlocks = 16384; // 1 GiB of slots

struct GzScratch { // stays with the engine (grow-only); goes with yacrd_engine_trim / destroy
    static constexpr yacrd_engine::Slot kScratchSlot = yacrd_engine::kGzip;
    DevBuf text, slots, out, out2, sizes, off, part, ctl; // (out2: the overlap editor's second batch of members, gzip_device_open)
    PinBuf pin; // n_buffers input segments, one output segment, the control words
};
inline u64 out_bound(u64 blocks) { return blocks * (u64)ydf::kSlot + ydf::kEofBytes; }

} // namespace

namespace yke {

// THE DEVICE-RESIDENT STEP: d_text[0, n) -> a run of BGZF members in `d_out` (the EOF member behind them when `last`), on
// stream `st`, asynchronous; S.off[n_members] = the members' bytes.  n <= the segment the scratch was sized for; d_text is
// 16-byte aligned (a block's start in a longer text is: 65 280 = 16 x 4080).
static int gzip_on_device(yacrd_engine *e, GzScratch &S, hipStream_t st, const unsigned char *d_text, u64 n, bool last, unsigned char *d_out)
{
    const u32 nb = (u32)((n + ydf::kBlock - 1) / ydf::kBlock);
    if (nb) hipLaunchKernelGGL(yk::df_encode_kernel, dim3(nb), dim3(256), 0, st, d_text, n, S.slots.as<unsigned char>(), S.sizes.as<u32>(),
                               S.ctl.as<unsigned long long>());
    if (const int rc = scan_u32_to_u64(e, S.sizes.as<u32>(), nb, S.off.as<u64>(), S.part, st)) return rc;
    if (nb + (last ? 1u : 0u))
        hipLaunchKernelGGL(yk::df_pack_kernel, dim3(nb + (last ? 1u : 0u)), dim3(256), 0, st, S.slots.as<unsigned char>(), S.sizes.as<u32>(),
                           S.off.as<u64>(), nb, d_out);
    HIP_TRY(hipGetLastError());
    return YACRD_OK;
}

// ---- the same step for text that ALREADY lies in HBM (gpu_edit.hip: the kept bytes of an overlap file) ---------------------
// open takes every buffer for batches of up to max_blocks blocks — the members of two batches: one is fetched while the
// next is encoded — and holds the engine's gzip scratch like a writer does; nothing is allocated afterwards.
int gzip_device_open(yacrd_engine *e, u64 max_blocks, GzDevice *g)
{
    if (e->gzip_busy) return fail(YACRD_EINVAL, "the engine already has a gzip writer");
    GzScratch *S = scratch_of<GzScratch>(e);
    if (!S) return fail(YACRD_ENOMEM, "host allocation failed");
    const u64 blocks = std::min(std::max<u64>(max_blocks, 1), kMaxSegBlocks);
    HIP_TRY(S->slots.reserve((size_t)(blocks * ydf::kSlot)));
    HIP_TRY(S->out.reserve((size_t)out_bound(blocks) + 64));
    HIP_TRY(S->out2.reserve((size_t)out_bound(blocks) + 64));
    HIP_TRY(S->sizes.reserve((size_t)(blocks + 1) * sizeof(u32)));
    HIP_TRY(S->off.reserve((size_t)(blocks + 2) * sizeof(u64)));
    HIP_TRY(S->ctl.reserve(64));
    HIP_TRY(S->part.reserve((size_t)(blocks + 2) * sizeof(u64)));
    HIP_TRY(hipMemsetAsync(S->ctl.p, 0, 64, e->stream)); // (the caller waits for e->stream before its first batch)
    g->out[0] = S->out.as<unsigned char>(), g->out[1] = S->out2.as<unsigned char>();
    g->max_blocks = blocks;
    e->gzip_busy = true;
    return YACRD_OK;
}

// d_text[0, n) (n <= max_blocks blocks) -> members in g.out[which] on stream `st`, events k0 / k1 around the kernels; behind
// them on the stream the members' bytes (without the EOF member's) land in *h_bytes and the stored members so far in
// *h_stored: pinned memory.  Asynchronous.
int gzip_device_encode(yacrd_engine *e, const GzDevice &g, hipStream_t st, const unsigned char *d_text, u64 n, bool last, int which,
                       hipEvent_t k0, hipEvent_t k1, volatile u64 *h_bytes, volatile u64 *h_stored)
{
    GzScratch &S = *scratch_of<GzScratch>(e); // (gzip_device_open made it)
    const u64 nb = (n + ydf::kBlock - 1) / ydf::kBlock;
    if (nb > g.max_blocks) return fail(YACRD_EINTERNAL, "device deflate: a batch beyond the blocks its buffers were taken for");
    HIP_TRY(hipEventRecord(k0, st));
    if (const int rc = gzip_on_device(e, S, st, d_text, n, last, const_cast<unsigned char *>(g.out[which & 1]))) return rc;
    HIP_TRY(hipEventRecord(k1, st));
    HIP_TRY(hipMemcpyAsync((void *)h_bytes, S.off.as<u64>() + nb, sizeof(u64), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync((void *)h_stored, S.ctl.p, sizeof(u64), hipMemcpyDeviceToHost, st));
    return YACRD_OK;
}

void gzip_device_close(yacrd_engine *e) { e->gzip_busy = false; }

} // namespace yke

// text -> segments -> BGZF bytes into a file descriptor or into memory
struct yacrd_gzip_writer {
    yacrd_engine *e = nullptr;
    GzScratch *S = nullptr;
    u64 seg_bytes = 0;
    u32 n_buf = 2;
    char *pin_in = nullptr, *pin_out = nullptr;
    volatile u64 *h_ctl = nullptr; // [0] bytes of the members of the segment in flight, [1] stored members so far
    Events ev; // h2d begin, kernels begin, kernels end (they go with the writer, behind drop()'s wait)
    u32 cur = 0;      // the buffer being filled
    u64 fill = 0;     // bytes in it
    bool in_flight = false, flight_last = false;
    bool failed = false;
    yseg::BesideFile file; // where the bytes go: a file beside its place (the writer), or growing memory (yacrd_engine_gzip_mem)
    yseg::Sink sink;
    yacrd_gzip_stats st = {};

    // the segment in flight: wait for it, fetch its members, append them
    int collect()
    {
        if (!in_flight) return YACRD_OK;
        in_flight = false;
        HIP_TRY(hipStreamSynchronize(e->stream));
        st.h2d_ms += ev_ms(ev[0], ev[1]);
        st.kernel_ms += ev_ms(ev[1], ev[2]);
        const u64 bytes = h_ctl[0] + (flight_last ? ydf::kEofBytes : 0u);
        if (bytes > out_bound(seg_bytes / ydf::kBlock)) return fail(YACRD_EINTERNAL, "device deflate: more bytes than the members' slots hold");
        const double t0 = now_ms();
        if (bytes) HIP_TRY(hipMemcpy(pin_out, S->out.p, (size_t)bytes, hipMemcpyDeviceToHost));
        const double t1 = now_ms();
        if (!sink.put(pin_out, (size_t)bytes)) return fail(YACRD_EINVAL, "Error during writing of the output file");
        st.d2h_ms += (float)(t1 - t0), st.write_ms += (float)(now_ms() - t1);
        st.out_bytes += bytes;
        st.n_stored = h_ctl[1];
        return YACRD_OK;
    }
    // the buffer being filled goes to the device
    int submit(bool last)
    {
        if (const int rc = collect()) return rc;
        const char *src = pin_in + (size_t)cur * seg_bytes;
        HIP_TRY(hipEventRecord(ev[0], e->stream));
        if (fill) HIP_TRY(hipMemcpyAsync(S->text.p, src, (size_t)fill, hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipEventRecord(ev[1], e->stream));
        if (const int rc = gzip_on_device(e, *S, e->stream, S->text.as<unsigned char>(), fill, last, S->out.as<unsigned char>())) return rc;
        HIP_TRY(hipEventRecord(ev[2], e->stream));
        const u64 nb = (fill + ydf::kBlock - 1) / ydf::kBlock;
        HIP_TRY(hipMemcpyAsync((void *)h_ctl, S->off.as<u64>() + nb, sizeof(u64), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipMemcpyAsync((void *)(h_ctl + 1), S->ctl.p, sizeof(u64), hipMemcpyDeviceToHost, e->stream));
        st.in_bytes += fill, st.n_members += nb;
        in_flight = true, flight_last = last;
        cur = (cur + 1) % n_buf, fill = 0;
        // (with two buffers the one to be filled next flew one segment ago: collect() above has waited for it)
        return YACRD_OK;
    }
    int write(const char *p, u64 n)
    {
        while (n) {
            if (fill == seg_bytes)
                if (const int rc = submit(false)) return rc;
            const u64 k = std::min(n, seg_bytes - fill);
            std::memcpy(pin_in + (size_t)cur * seg_bytes + fill, p, (size_t)k);
            fill += k, p += k, n -= k;
        }
        return YACRD_OK;
    }
    int finish()
    {
        if (const int rc = submit(true)) return rc;
        return collect();
    }
    void drop()
    {
        if (e) {
            DeviceGuard guard(e->device);
            (void)hipStreamSynchronize(e->stream);
            (void)hipGetLastError();
            e->gzip_busy = false;
        }
        file.drop();
        std::free(sink.mem);
        sink.mem = nullptr;
    }
};

namespace {

// the engine's buffers for segments of seg_blocks blocks, and a writer over them (no sink yet)
int writer_setup(yacrd_engine *e, u64 segment_bytes, u32 n_buffers, yacrd_gzip_writer *w)
{
    if (e->pending.active || e->host_pending) return fail(YACRD_EINVAL, "the engine has a submitted batch pending");
    if (e->gzip_busy) return fail(YACRD_EINVAL, "the engine already has a gzip writer");
    u64 blocks = segment_bytes ? (segment_bytes + ydf::kBlock - 1) / ydf::kBlock : kDefaultSegBlocks;
    blocks = std::min(std::max<u64>(blocks, 1), kMaxSegBlocks);
    n_buffers = 2; // (one segment is in flight while the next is filled: more buffers would only pin more memory)
    GzScratch *S = scratch_of<GzScratch>(e);
    if (!S) return fail(YACRD_ENOMEM, "host allocation failed");
    e->gzip_busy = true, w->e = e; // (from here on the caller drops the writer when something fails)
    const u64 seg = blocks * ydf::kBlock;
    HIP_TRY(S->text.reserve((size_t)seg + 64));
    HIP_TRY(S->slots.reserve((size_t)(blocks * ydf::kSlot)));
    HIP_TRY(S->out.reserve((size_t)out_bound(blocks) + 64));
    HIP_TRY(S->sizes.reserve((size_t)(blocks + 1) * sizeof(u32)));
    HIP_TRY(S->off.reserve((size_t)(blocks + 2) * sizeof(u64)));
    HIP_TRY(S->ctl.reserve(64));
    HIP_TRY(S->part.reserve((size_t)(blocks + 2) * sizeof(u64))); // (the scan's partial sums: at most one per element; nothing is allocated after open)
    const size_t pin_need = (size_t)n_buffers * seg + (size_t)out_bound(blocks) + 64;
    if (S->pin.reserve(pin_need) != hipSuccess) {
        (void)hipGetLastError();
        return fail(YACRD_ENOMEM, "device deflate: no pinned memory");
    }
    HIP_TRY(hipMemsetAsync(S->ctl.p, 0, 64, e->stream));
    if (!w->ev.add(3)) HIP_TRY(why_not_added());
    w->S = S, w->seg_bytes = seg, w->n_buf = n_buffers;
    w->pin_in = S->pin.as<char>();
    w->pin_out = w->pin_in + (size_t)n_buffers * seg;
    w->h_ctl = reinterpret_cast<volatile u64 *>(w->pin_out + ((out_bound(blocks) + 15) & ~(u64)15));
    w->h_ctl[0] = w->h_ctl[1] = 0;
    return YACRD_OK;
}

} // namespace

extern "C" {

int yacrd_engine_gzip_mem(yacrd_engine *e, const char *data, uint64_t n_bytes, char **out, uint64_t *out_bytes, yacrd_gzip_stats *stats)
{
    if (!e || (!data && n_bytes) || !out || !out_bytes) return fail(YACRD_EINVAL, "null argument");
    *out = nullptr, *out_bytes = 0;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    DeviceGuard guard(e->device);
    yacrd_gzip_writer w;
    int rc = writer_setup(e, 0, 0, &w);
    if (rc == YACRD_OK) {
        w.sink.mem = (char *)std::malloc((size_t)(n_bytes / 2 + 4096)), w.sink.cap = w.sink.mem ? n_bytes / 2 + 4096 : 0; // (none: the sink grows from nothing)
        rc = w.write(data, n_bytes);
        if (rc == YACRD_OK) rc = w.finish();
        if (rc == YACRD_OK) {
            *out = w.sink.mem, *out_bytes = w.sink.at;
            w.sink.mem = nullptr;
            if (stats) *stats = w.st;
        }
    }
    w.drop();
    return rc;
}

int yacrd_gzip_writer_open(yacrd_engine *e, const char *out_path, uint64_t segment_bytes, uint32_t n_buffers, yacrd_gzip_writer **out)
{
    if (!e || !out_path || !out) return fail(YACRD_EINVAL, "null argument");
    *out = nullptr;
    DeviceGuard guard(e->device);
    yacrd_gzip_writer *w = new (std::nothrow) yacrd_gzip_writer();
    if (!w) return fail(YACRD_ENOMEM, "host allocation failed");
    int rc = writer_setup(e, segment_bytes, n_buffers, w);
    if (rc == YACRD_OK) {
        if (!w->file.open(out_path)) rc = fail(YACRD_EINVAL, std::string("cannot create a file beside ") + out_path);
        w->sink.fd = w->file.fd;
    }
    if (rc != YACRD_OK) {
        if (w->e) w->drop();
        delete w;
        return rc;
    }
    *out = w;
    return YACRD_OK;
}

int yacrd_gzip_writer_write(yacrd_gzip_writer *w, const char *p, uint64_t n)
{
    if (!w || (!p && n)) return fail(YACRD_EINVAL, "null argument");
    if (w->failed) return fail(YACRD_EINVAL, "the gzip writer has failed before");
    DeviceGuard guard(w->e->device);
    const int rc = w->write(p, n);
    if (rc != YACRD_OK) w->failed = true;
    return rc;
}

static int gzip_sink_write(void *ctx, const char *p, uint64_t n) { return yacrd_gzip_writer_write(static_cast<yacrd_gzip_writer *>(ctx), p, n); }

int yacrd_gzip_writer_sink(yacrd_gzip_writer *w, yacrd_byte_sink *sink)
{
    if (!w || !sink) return fail(YACRD_EINVAL, "null argument");
    sink->ctx = w, sink->write = gzip_sink_write;
    return YACRD_OK;
}

int yacrd_gzip_writer_close(yacrd_gzip_writer *w, yacrd_gzip_stats *stats)
{
    if (!w) return fail(YACRD_EINVAL, "null argument");
    if (stats) std::memset(stats, 0, sizeof(*stats));
    int rc = YACRD_OK;
    {
        DeviceGuard guard(w->e->device);
        rc = w->failed ? fail(YACRD_EINVAL, "the gzip writer has failed before") : w->finish();
    }
    if (rc == YACRD_OK && !w->file.commit()) rc = fail(YACRD_EINVAL, "Error during writing of the output file");
    if (rc == YACRD_OK && stats) *stats = w->st;
    w->drop();
    delete w;
    return rc;
}

void yacrd_gzip_writer_abort(yacrd_gzip_writer *w)
{
    if (!w) return;
    w->drop(); // (the file beside the output goes with it)
    delete w;
}

} // extern "C"
