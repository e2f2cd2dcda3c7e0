// gpu_gunzip_stream.hip — ONE plain gzip member inflated on the GPU: the member in host memory -> its text in HBM
// (include/yacrd_engine.h: yacrd_engine_gunzip_stream_mem; gpu_seq_edit.hip: the editors' _gz_ forms).  The decoder's text
// and its rules are inflate_stream.h's; the framing is gzip_walk.h's; DESIGN 7q argues the whole.
//
//   find      one wavefront per chunk of C compressed bytes (k >= 1): 64 candidate bits a step, judged in registers, the
//             first step with an accept ends the walk: at most 8 C / 64 steps
//   size      one wavefront per span: inflate_block.h's tables in LDS (4.7 KiB), nothing stored.  The host walks the chain
//             (str_chain) and launches one more span per proven block start that had none: at most kMaxRounds launches
//   symbols   one wavefront per true span, the same walk, one u16 per text byte at the span's place; a span reads back
//             what it has stored (one wavefront's accesses to an address are served in order), nobody else's
//   windows   ONE workgroup of 1 024 threads, spans in order, a barrier per span: the design's one serial chain (measured:
//             about 22 us a span, the largest step at one span per 32 KiB chunk: DESIGN 7q)
//   bytes     256 threads per tile of 4 096 text bytes, 16 bytes and one 16-byte store per thread; the tile's CRC-32 is
//             joined from the threads' by x^(8 n) in LDS, the text's from the tiles' by one atomic XOR per tile
// No workgroup waits for another inside a launch; every loop of every kernel eats a bit, makes a byte or counts to a bound
// that is known when it starts.  Every span, place and size a kernel takes from a table is checked against the buffers
// before a byte is read or stored.
#include "engine_internal.h"
#include "gpu_text.h"
#include "gzip_walk.h"
#include "inflate_stream.h"
#include "host/segment_pump.h"

#include <cstdio>
#include <cstdlib>

using namespace yke;

namespace yk {

__device__ __forceinline__ u64 gs_uni64(u64 x)
{
    return (u64)YI_UNI((u32)x) | ((u64)YI_UNI((u32)(x >> 32)) << 32);
}
__device__ __forceinline__ yis::Span gs_span(const yis::Span *p) // the same in every lane, and said so
{
    yis::Span s = *p;
    s.start_bit = gs_uni64(s.start_bit), s.stop_bit = gs_uni64(s.stop_bit), s.end_bit = gs_uni64(s.end_bit), s.out_off = gs_uni64(s.out_off);
    s.out_bytes = YI_UNI(s.out_bytes), s.n_blocks = YI_UNI(s.n_blocks), s.status = YI_UNI(s.status), s.saw_final = YI_UNI(s.saw_final);
    return s;
}

// finds[k - 1]: the first acceptable bit of chunk k, k in [1, n_chunks)
__global__ __launch_bounds__(64) void gs_find_kernel(const unsigned char *pay, u64 pay_bytes, u32 chunk, u64 n_chunks, u64 *finds)
{
    const u64 k = (u64)blockIdx.x + 1u;
    if (k >= n_chunks) return; // (uniform)
    const u64 lo = k * chunk, hi = lo + chunk < pay_bytes ? lo + chunk : pay_bytes; // (lo < pay_bytes: n_chunks is the payload's)
    const u64 f = yis::str_find(pay, pay_bytes, 8u * lo, 8u * hi);
    if (threadIdx.x == 0) finds[k - 1u] = f;
}

__global__ __launch_bounds__(64) void gs_size_kernel(const unsigned char *pay, u64 pay_bytes, yis::Span *spans, u32 n_spans)
{
    __shared__ yif::InfShared sh;
    if (blockIdx.x >= n_spans) return; // (uniform)
    yis::Span sp = gs_span(spans + blockIdx.x);
    const u32 st = yis::str_walk_span<false>(sh, pay, pay_bytes, sp, nullptr);
    if (threadIdx.x == 0) {
        sp.status = st;
        spans[blockIdx.x] = sp;
    }
}

// words[0]: the status (the largest wins); words[1]: the text's CRC-32, XORed together by the bytes step
__global__ __launch_bounds__(64) void gs_symbols_kernel(const unsigned char *pay, u64 pay_bytes, const yis::Span *spans, u32 n_spans,
                                                         yis::u16 *sym, u64 total, u32 *words)
{
    __shared__ yif::InfShared sh;
    if (blockIdx.x >= n_spans) return; // (uniform)
    yis::Span sp = gs_span(spans + blockIdx.x);
    u32 st = yis::kStrChain; // the table is the host's, from SIZE; what it says is checked against the scratch all the same
    if (sp.out_off <= total && sp.out_bytes <= total - sp.out_off) st = yis::str_walk_span<true>(sh, pay, pay_bytes, sp, sym + sp.out_off);
    if (st != yif::kInfOk && threadIdx.x == 0) atomicMax(words, st);
}

__global__ __launch_bounds__(1024) void gs_windows_kernel(const yis::Span *spans, u32 n_spans, yis::u16 *sym, u64 total, u32 *words)
{
    u32 st = 0;
    yis::str_windows(spans, n_spans, sym, total, &st);
    if (st) atomicMax(words, st);
}

__global__ __launch_bounds__(256) void gs_bytes_kernel(const yis::Span *spans, u32 n_spans, const yis::u16 *sym, u64 total, unsigned char *out,
                                                        u32 *words)
{
    __shared__ u32 tab[256], pw[yis::kTileThreads], tile_crc;
    const u32 tid = threadIdx.x;
    tab[tid] = yis::str_crc_entry(tid), pw[tid] = yis::str_xpow8((u64)yis::kThreadBytes * tid);
    if (tid == 0) tile_crc = 0;
    __syncthreads();
    const u64 n_tiles = (total + yis::kTile - 1u) / yis::kTile;
    for (u64 tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) { // (uniform)
        const u64 t0 = tile * yis::kTile, t1 = total - t0 < yis::kTile ? total : t0 + yis::kTile, x0 = t0 + (u64)tid * yis::kThreadBytes;
        u32 st = 0;
        const u32 c = yis::str_bytes_thread(spans, n_spans, sym, total, x0, tab, out, &st);
        if (st) atomicMax(words, st);
        u32 part = 0;
        if (x0 < t1) {
            const u64 my_end = t1 - x0 < yis::kThreadBytes ? t1 : x0 + yis::kThreadBytes;
            part = ydf::df_mulmod(t1 - t0 == yis::kTile ? pw[yis::kTileThreads - 1u - tid] : yis::str_xpow8(t1 - my_end), c);
        }
        for (int o = 32; o; o >>= 1) part ^= __shfl_xor(part, o);
        if ((tid & 63u) == 0 && part) atomicXor(&tile_crc, part);
        __syncthreads();
        if (tid == 0) {
            if (tile_crc) atomicXor(words + 1, ydf::df_mulmod(yis::str_xpow8(total - t1), tile_crc));
            tile_crc = 0;
        }
        __syncthreads();
    }
}

} // namespace yk

namespace {

constexpr size_t kHomePiece = (size_t)4 << 20; // what one copy home moves

struct GunzipStreamScratch { // stays with the engine (grow-only); goes with yacrd_engine_trim / destroy
    static constexpr yacrd_engine::Slot kScratchSlot = yacrd_engine::kGunzipStream;
    DevBuf comp, finds, spans, sym, words;
    DevBuf text;   // yacrd_engine_gunzip_stream_mem's (the editors inflate into their own text buffer)
    PinBuf tables; // the finds and the span tables on their way; the status word and the CRC
    PinBuf pin;    // two pieces of text on their way home
    u64 pay_off = 0, pay_bytes = 0;
};

u32 chunk_of(const yacrd_engine *e)
{
    u64 c = e->gunzip_chunk;
    if (!c)
        if (const char *env = std::getenv("YACRD_GUNZIP_CHUNK")) c = std::strtoull(env, nullptr, 10);
    if (!c) return yis::kDefaultChunk;
    return (u32)std::min<u64>(std::max<u64>(c, yis::kMinChunk), (u64)1 << 30);
}

int stream_not_taken(u32 status)
{
    return fail(YACRD_EFALLBACK, std::string("a gzip stream the device decoder does not take (") + yis::str_status_name(status) + "): the host reader's");
}

} // namespace

namespace yke {

int stream_inflate_open(yacrd_engine *e, const char *gz, u64 n_bytes, int n_threads, double text_copies, double held, StreamInflate *s)
{
    *s = StreamInflate{};
    yacrd_gunzip_stream_stats &st = s->stats;
    ygw::GzipFrame f;
    if (!ygw::walk(reinterpret_cast<const unsigned char *>(gz ? gz : ""), n_bytes, &f)) return fail(YACRD_EFALLBACK, "not a gzip member: the host reader's");
    if (f.payload_bytes > yis::kMaxPayload) return stream_not_taken(yis::kStrPayload);
    const u32 chunk = chunk_of(e);
    const u64 n_chunks = yis::str_chunks(f.payload_bytes, chunk);
    if (n_chunks >= 0x7FFFFFFFull) return fail(YACRD_EFALLBACK, "more chunks than the device decoder numbers");
    st.in_bytes = n_bytes, st.n_chunks = n_chunks, s->crc = f.crc;
    GunzipStreamScratch *S = scratch_of<GunzipStreamScratch>(e);
    if (!S) return fail(YACRD_ENOMEM, "host allocation failed");
    S->pay_off = f.payload_off, S->pay_bytes = f.payload_bytes;
    const void *before = S->comp.p;
    HIP_TRY(S->comp.reserve((size_t)n_bytes + 64));
    HIP_TRY(S->finds.reserve((size_t)n_chunks * sizeof(u64)));
    HIP_TRY(S->spans.reserve((size_t)(n_chunks + 1) * sizeof(yis::Span)));
    HIP_TRY(S->words.reserve(64));
    HIP_TRY(S->tables.reserve((size_t)(n_chunks + 1) * sizeof(yis::Span) + 64));
    HIP_TRY(hipMemsetAsync(S->words.p, 0, 64, e->stream));
    HIP_TRY(hipMemsetAsync(S->comp.as<char>() + n_bytes, 0, 64, e->stream));
    Events ev;
    if (!ev.add(4)) HIP_TRY(why_not_added());
    const double t0 = now_ms();
    TextSource src;
    src.mem = gz;
    const int moved = move_text(e, src, 0, n_bytes, S->comp.as<char>(), S->comp.p != before, n_threads, [](u64, u64, u64) {});
    if (moved == 3) return fail(YACRD_ENOMEM, "gzip stream to HBM: no pinned memory");
    if (moved) return fail(YACRD_ENODEV, "device gunzip: a HIP call failed");
    st.h2d_ms = (float)(now_ms() - t0);
    const unsigned char *pay = S->comp.as<unsigned char>() + f.payload_off;
    // FIND
    std::vector<u64> finds((size_t)(n_chunks - 1));
    HIP_TRY(hipEventRecord(ev[0], e->stream));
    if (n_chunks > 1) {
        hipLaunchKernelGGL(yk::gs_find_kernel, dim3((u32)(n_chunks - 1)), dim3(64), 0, e->stream, pay, f.payload_bytes, chunk, n_chunks, S->finds.as<u64>());
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ev[1], e->stream));
    if (n_chunks > 1) HIP_TRY(hipMemcpyAsync(S->tables.p, S->finds.p, finds.size() * sizeof(u64), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipGetLastError());
    st.find_ms = ev_ms(ev[0], ev[1]);
    if (n_chunks > 1) std::memcpy(finds.data(), S->tables.p, finds.size() * sizeof(u64));
    // SIZE, and the chain with its repair rounds: every round is one launch and one wait
    int hip_rc = YACRD_OK;
    auto size = [&](yis::Span *sp, size_t m) -> bool {
        auto go = [&]() -> int {
            if (m > n_chunks + 1) return fail(YACRD_EINTERNAL, "device gunzip: more spans than chunks"); // (a find per chunk, bit 0, or one fresh span)
            std::memcpy(S->tables.p, sp, m * sizeof(yis::Span));
            HIP_TRY(hipMemcpyAsync(S->spans.p, S->tables.p, m * sizeof(yis::Span), hipMemcpyHostToDevice, e->stream));
            HIP_TRY(hipEventRecord(ev[2], e->stream));
            hipLaunchKernelGGL(yk::gs_size_kernel, dim3((u32)m), dim3(64), 0, e->stream, pay, f.payload_bytes, S->spans.as<yis::Span>(), (u32)m);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipEventRecord(ev[3], e->stream));
            HIP_TRY(hipMemcpyAsync(S->tables.p, S->spans.p, m * sizeof(yis::Span), hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
            HIP_TRY(hipGetLastError());
            st.size_ms += ev_ms(ev[2], ev[3]);
            std::memcpy(sp, S->tables.p, m * sizeof(yis::Span));
            return YACRD_OK;
        };
        return (hip_rc = go()) == YACRD_OK;
    };
    std::vector<yis::Span> spans;
    yis::StreamCounts c;
    c.n_chunks = n_chunks;
    int status = 0;
    try {
        status = yis::str_chain(finds, f.payload_bytes, f.isize, size, spans, c);
    } catch (const std::bad_alloc &) {
        return fail(YACRD_ENOMEM, "host allocation failed");
    }
    if (status < 0) return hip_rc;
    if (status) return stream_not_taken((u32)status);
    st.n_spans = c.n_spans, st.n_false_starts = c.n_false_starts, st.rounds = c.rounds, st.n_blocks = c.n_blocks, st.out_bytes = c.out_bytes;
    s->text_bytes = c.out_bytes, s->n_true = spans.size(); // (<= n_chunks + rounds: the tables hold them, checked below)
    // room: the caller's buffers of the text's size, two bytes of symbol per text byte; the compressed bytes are held already
    const double total = (double)c.out_bytes;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess &&
        (text_copies + 2.0) * total * 1.125 + (double)((size_t)64 << 20) > (double)free_b + held + (double)S->sym.cap)
        return fail(YACRD_EFALLBACK, "the text and its symbols do not fit this device's free memory: the host reader streams it");
    HIP_TRY(S->sym.reserve((size_t)c.out_bytes * sizeof(yis::u16) + 64));
    HIP_TRY(S->spans.reserve(spans.size() * sizeof(yis::Span)));
    HIP_TRY(S->tables.reserve(spans.size() * sizeof(yis::Span) + 64));
    std::memcpy(S->tables.p, spans.data(), spans.size() * sizeof(yis::Span));
    HIP_TRY(hipMemcpyAsync(S->spans.p, S->tables.p, spans.size() * sizeof(yis::Span), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream)); // (the pinned table is free again)
    return YACRD_OK;
}

void stream_inflate_release(yacrd_engine *e)
{
    if (GunzipStreamScratch *S = static_cast<GunzipStreamScratch *>(e->scratch[GunzipStreamScratch::kScratchSlot].p)) S->comp.release(), S->sym.release();
}

int stream_inflate_run(yacrd_engine *e, StreamInflate &s, unsigned char *d_text)
{
    GunzipStreamScratch *S = scratch_of<GunzipStreamScratch>(e);
    if (!S || !S->comp.p || !S->spans.p || !S->words.p || !S->tables.p || s.n_true == 0 || s.n_true >= 0x7FFFFFFFull ||
        S->spans.cap < s.n_true * sizeof(yis::Span) || S->sym.cap < s.text_bytes * sizeof(yis::u16))
        return fail(YACRD_EINTERNAL, "device gunzip: the stream is not open");
    const unsigned char *pay = S->comp.as<unsigned char>() + S->pay_off;
    const yis::Span *spans = S->spans.as<yis::Span>();
    yis::u16 *sym = S->sym.as<yis::u16>();
    u32 *words = S->words.as<u32>();
    const u64 total = s.text_bytes;
    const u32 n = (u32)s.n_true;
    Events ev;
    if (!ev.add(4)) HIP_TRY(why_not_added());
    volatile u32 *h_words = reinterpret_cast<volatile u32 *>(S->tables.p);
    h_words[0] = h_words[1] = 0;
    HIP_TRY(hipEventRecord(ev[0], e->stream));
    hipLaunchKernelGGL(yk::gs_symbols_kernel, dim3(n), dim3(64), 0, e->stream, pay, S->pay_bytes, spans, n, sym, total, words);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[1], e->stream));
    hipLaunchKernelGGL(yk::gs_windows_kernel, dim3(1), dim3(1024), 0, e->stream, spans, n, sym, total, words);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev[2], e->stream));
    const u64 n_tiles = (total + yis::kTile - 1) / yis::kTile;
    if (n_tiles) {
        hipLaunchKernelGGL(yk::gs_bytes_kernel, dim3((u32)std::min<u64>(n_tiles, (u64)e->num_cu * 8u)), dim3(256), 0, e->stream, spans, n, sym, total, d_text, words);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(ev[3], e->stream));
    HIP_TRY(hipMemcpyAsync((void *)h_words, words, 2 * sizeof(u32), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipGetLastError());
    s.stats.symbols_ms = ev_ms(ev[0], ev[1]), s.stats.windows_ms = ev_ms(ev[1], ev[2]), s.stats.bytes_ms = ev_ms(ev[2], ev[3]);
    if (h_words[0]) return stream_not_taken(h_words[0]);
    if (h_words[1] != s.crc) return stream_not_taken(yif::kInfCrc);
    return YACRD_OK;
}

} // namespace yke

extern "C" {

int yacrd_engine_gunzip_stream_mem(yacrd_engine *e, const char *gz, uint64_t n_bytes, char **out, uint64_t *out_bytes, yacrd_gunzip_stream_stats *stats)
{
    if (!e || (!gz && n_bytes) || !out || !out_bytes) return fail(YACRD_EINVAL, "null argument");
    *out = nullptr, *out_bytes = 0;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (e->pending.active || e->host_pending) return fail(YACRD_EINVAL, "the engine has a submitted batch pending");
    DeviceGuard guard(e->device);
    StreamInflate s;
    char *res = nullptr;
    Events wev; // a piece has landed at home (two)
    auto run = [&]() -> int {
        GunzipStreamScratch *S = scratch_of<GunzipStreamScratch>(e);
        if (!S) return fail(YACRD_ENOMEM, "host allocation failed");
        if (const int rc = stream_inflate_open(e, gz, n_bytes, 0, 1.0, (double)S->text.cap, &s)) return rc;
        const u64 total = s.text_bytes;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (double)total * 1.125 + (double)((size_t)64 << 20) > (double)free_b + (double)S->text.cap)
            return fail(YACRD_EFALLBACK, "the text does not fit this device's free memory: the host reader streams it");
        res = (char *)std::malloc((size_t)total + 1);
        if (!res) return fail(YACRD_ENOMEM, "host allocation failed");
        HIP_TRY(S->text.reserve((size_t)total + 64));
        HIP_TRY(S->pin.reserve(2 * kHomePiece));
        if (!wev.add(2, hipEventDisableTiming)) HIP_TRY(why_not_added());
        if (const int rc = stream_inflate_run(e, s, S->text.as<unsigned char>())) return rc;
        const double t2 = now_ms();
        HomeLink dma{S->text.as<char>(), e->stream, {wev[0], wev[1]}};
        yseg::Sink sink;
        sink.mem = res; // (sized here: total bytes)
        const int rc = yseg::pump(total, kHomePiece, S->pin.as<char>(), dma, sink, [](auto put) { put(); });
        if (rc != yseg::kPumped || sink.at != total) return fail(YACRD_ENODEV, "device gunzip: a HIP call failed on the way home");
        s.stats.d2h_ms = (float)(now_ms() - t2);
        return YACRD_OK;
    };
    const int rc = run();
    (void)hipStreamSynchronize(e->stream); // (whatever failed: nothing of this call is in flight when its events go)
    (void)hipGetLastError();
    if (rc != YACRD_OK) {
        std::free(res);
        return rc;
    }
    *out = res, *out_bytes = s.text_bytes;
    if (stats) *stats = s.stats;
    return YACRD_OK;
}

int yacrd_debug_gunzip_chunk(yacrd_engine *e, uint32_t bytes)
{
    if (!e) return fail(YACRD_EINVAL, "null argument");
    if (bytes && bytes < yis::kMinChunk) return fail(YACRD_EINVAL, "the gunzip chunk is at least 1 024 bytes");
    e->gunzip_chunk = bytes;
    return YACRD_OK;
}

} // extern "C"
