// gpu_text.h — what the translation units that work on TEXT in HBM share: gpu_paf.hip (the device parser), gpu_edit.hip
// (filter / extract on overlap files), gpu_seq_edit.hip (the FASTQ and FASTA editors), gpu_report.hip (the report reader),
// gpu_report_write.hip (the report writer), gpu_deflate.hip and gpu_inflate.hip.  Where the text comes from (TextSource, FdGuard,
// the format rule), the mover (pread -> pinned 4 MiB chunks -> the mirror in HBM, a segment handed on as soon as it has
// landed), the way home (HomeLink: what the editors, the report writer and the inflater plug into host/segment_pump.h), the
// staged-window accessor, the byte matcher and the id hash; what an ingest's outputs share.
#pragma once
#include "engine_internal.h"
#include "bgzf_walk.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

namespace yk {

constexpr int kGpT = 256;           // threads per workgroup
constexpr int kGpTile = kGpT * 128; // bytes of text per workgroup: a thread takes the lines that START in its 128 bytes

// pinned host memory -> the mirror, by a kernel (used when the mirror is a fresh allocation: see move_text's callers)
static __global__ __launch_bounds__(256) void gp_blit_kernel(uint4 *__restrict__ dst, const uint4 *__restrict__ src, u64 n16)
{
    for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < n16; i += (u64)gridDim.x * 256u) dst[i] = src[i];
}

// text through a window staged in LDS; what lies outside the window comes from global memory
struct GpText {
    const unsigned char *lds, *glob;
    u64 t0, t1; // the staged window [t0, t1)
    __device__ __forceinline__ u32 operator[](u64 i) const { return i - t0 < t1 - t0 ? lds[i - t0] : glob[i]; }
};
// plain bytes in global memory, as a text
struct GpBytes {
    const unsigned char *p;
    __device__ __forceinline__ u32 operator[](u64 i) const { return p[i]; }
};

// bit k of the result: byte k of the 16 is `c`
__device__ __forceinline__ u32 gp_eq16(const uint4 &v, u32 c)
{
    const u32 w[4] = {v.x, v.y, v.z, v.w};
    const u32 cc = c * 0x01010101u;
    u32 m = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const u32 x = w[k] ^ cc;
        const u32 z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu); // 0x80 in every byte of x that is zero
        m |= ((((z >> 7) * 0x00204081u) >> 21) & 0xFu) << (4 * k);
    }
    return m;
}

template <class Text>
__device__ __forceinline__ u64 gp_hash(const Text &t, u64 p, u32 n)
{
    u64 h = 0xcbf29ce484222325ull ^ ((u64)n * 0x9E3779B97F4A7C15ull);
    for (u32 i = 0; i < n; i++) h = (h ^ t[p + i]) * 0x100000001b3ull;
    h ^= h >> 29;
    h *= 0xbf58476d1ce4e5b9ull;
    return h ^ (h >> 32);
}

} // namespace yk

namespace yke {

// gzip / bzip2 / xz (the magic bytes niffler looks at, src/util.rs:57-70)
inline bool is_compressed_magic(int fd)
{
    unsigned char mg[6] = {0};
    const ssize_t k = ::pread(fd, mg, sizeof mg, 0);
    return k >= 2 && ((mg[0] == 0x1f && mg[1] == 0x8b) || (k >= 3 && mg[0] == 'B' && mg[1] == 'Z' && mg[2] == 'h') ||
                      (k >= 6 && mg[0] == 0xFD && std::memcmp(mg + 1, "7zXZ", 4) == 0 && mg[5] == 0));
}

// 0 = by file name, like util::get_file_type (src/util.rs:39-55); 1 = PAF; 2 = M4 / MHAP
inline int overlap_format(const char *path, int format, bool &m4)
{
    if (format == 0) {
        if (!path) return fail(YACRD_EINVAL, "format 0 (by name) needs a file name");
        const std::string name(path);
        auto has = [&](const char *x) { return name.find(x) != std::string::npos; };
        format = (has(".m4") || has(".mhap")) ? 2 : has(".paf") ? 1 : 0;
        if (format == 0) return fail(YACRD_EINVAL, std::string("cannot tell the overlap format of ") + path);
    }
    if (format != 1 && format != 2) return fail(YACRD_EINVAL, "format: 0 = by name, 1 = PAF, 2 = M4");
    m4 = format == 2;
    return YACRD_OK;
}

struct FdGuard { // closes the input when the call returns
    int fd;
    ~FdGuard() { ::close(fd); }
};

// where the text comes from: a file (pread) or memory (a compressed file the host has inflated)
struct TextSource {
    int fd = -1;
    const char *mem = nullptr;
    // `len` bytes at `off` into dst; false = read error
    bool fetch(char *dst, size_t len, u64 off) const
    {
        if (mem) {
            std::memcpy(dst, mem + off, len);
            return true;
        }
        size_t got = 0;
        while (got < len) {
            const ssize_t k = ::pread(fd, dst + got, len - got, (off_t)(off + got));
            if (k < 0 && errno == EINTR) continue;
            if (k <= 0) return false;
            got += (size_t)k;
        }
        return true;
    }
};

// What the overlap editor (gpu_edit.hip) asks of a text before its first launch, and what an ingest records with the mirror it
// leaves (gpu_paf.hip): the field count of the first non-empty line (0: there is none) and whether the text's last byte is a
// newline.  (a text that is not in host memory: bgzf_text_ends, host/inflate_sample.cc, gives the same answers)
inline bool first_line_fields(const TextSource &src, u64 n, char delim, u32 &n_fields, bool &ends_in_newline)
{
    n_fields = 0, ends_in_newline = true;
    if (!n) return true;
    char last = 0;
    if (!src.fetch(&last, 1, n - 1)) return false;
    ends_in_newline = last == '\n';
    std::vector<char> buf((size_t)std::min<u64>(n, (u64)1 << 20));
    bool in_line = false;
    u32 nf = 0;
    for (u64 off = 0; off < n; off += buf.size()) {
        const size_t len = (size_t)std::min<u64>(buf.size(), n - off);
        if (!src.fetch(buf.data(), len, off)) return false;
        for (size_t i = 0; i < len; i++) {
            const char c = buf[i];
            if (c == '\n') {
                if (in_line) {
                    n_fields = nf;
                    return true;
                }
                continue;
            }
            if (!in_line) in_line = true, nf = 1;
            if (c == delim) nf++;
        }
    }
    if (in_line) n_fields = nf;
    return true;
}

// the way home of a text that lies in HBM: the link yseg::pump (host/segment_pump.h) drives.  src[at, at + len) is copied to a
// pinned piece on `stream`, with the event of that piece behind it.  `stop`, where given, is a word another thread sets to
// end the run: wait then gives up without touching `bad`, which holds the HIP error of a call that failed.
struct HomeLink {
    const char *src;
    hipStream_t stream;
    hipEvent_t landed[2];
    const std::atomic<int> *stop = nullptr;
    hipError_t bad = hipSuccess;
    bool start(u64 i, char *dst, u64 at, size_t len)
    {
        bad = hipMemcpyAsync(dst, src + at, len, hipMemcpyDeviceToHost, stream);
        if (bad == hipSuccess) bad = hipEventRecord(landed[i & 1], stream);
        return bad == hipSuccess;
    }
    bool wait(u64 i) { return !(stop && stop->load()) && (bad = hipEventSynchronize(landed[i & 1])) == hipSuccess; }
    void drain() { (void)hipStreamSynchronize(stream); }
};

// what an ingest (overlaps or a report) hands back, empty
inline void zero_outputs(yacrd_result *out, yacrd_reads *reads, yacrd_ingest_stats *stats)
{
    std::memset(out, 0, sizeof(*out));
    std::memset(reads, 0, sizeof(*reads));
    if (stats) std::memset(stats, 0, sizeof(*stats));
}

// the reads' lengths, name offsets and names from HBM into `reads`, allocated here: copies enqueued on the engine's stream.
// Whatever fails, `reads` is left empty.  (static, like gp_blit_kernel above: a unit's own copy, so that the library exports
// what it did before)
static int reads_to_host(yacrd_engine *e, yacrd_reads *reads, u32 n_reads, u64 n_records, const void *d_lengths, const void *d_name_off,
                         const void *d_names, u64 name_bytes)
{
    reads->n_reads = n_reads;
    reads->n_records = n_records;
    reads->lengths = (uint32_t *)std::malloc(((size_t)n_reads + 1) * sizeof(uint32_t));
    reads->name_off = (uint64_t *)std::malloc(((size_t)n_reads + 1) * sizeof(uint64_t));
    reads->names = (char *)std::malloc((size_t)name_bytes + 1);
    auto copies = [&]() -> int {
        if (!reads->lengths || !reads->name_off || !reads->names) return fail(YACRD_ENOMEM, "host allocation failed");
        if (n_reads) HIP_TRY(hipMemcpyAsync(reads->lengths, d_lengths, (size_t)n_reads * sizeof(u32), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipMemcpyAsync(reads->name_off, d_name_off, ((size_t)n_reads + 1) * sizeof(u64), hipMemcpyDeviceToHost, e->stream));
        if (name_bytes) HIP_TRY(hipMemcpyAsync(reads->names, d_names, (size_t)name_bytes, hipMemcpyDeviceToHost, e->stream));
        return YACRD_OK;
    };
    const int rc = copies();
    if (rc) yacrd_reads_free(reads);
    return rc;
}

constexpr size_t kTextChunk = (size_t)4 << 20; // what one pread and one copy move
constexpr size_t kTextSeg = 32;                // chunks per segment handed on (128 MiB)
static_assert(kTextChunk % yk::kGpTile == 0, "segments begin on tile boundaries");

// Bytes [begin, begin + n) of `src` -> mirror[0, n): threads pread chunks into the engine's pinned arena, every chunk crosses
// PCIe at once into the mirror (by copy kernel when `blit`: a fresh allocation; by hipMemcpyAsync into a warm one);
// THIS thread calls on_segment(seg_begin, seg_end, avail) — byte offsets into the mirror, seg_end a chunk boundary that
// may lie beyond n — for every kTextSeg chunks as soon as they and the chunk behind them have landed (`avail`: the bytes
// [0, avail) have), with the engine's stream made to wait for those chunks' copy events: what on_segment launches on
// e->stream sees the text, the host waits for nothing.  Returns 0, 1 (a HIP call failed), 2 (read error) or 3 (no pinned memory).
// `chunk`: what one pread and one copy move, a multiple of the tile and at most kTextChunk (the sequence editor's windows may
// be smaller than a chunk: gpu_seq_edit.hip).  `lanes`: copy streams the caller keeps between calls (a run that moves its text
// in many calls makes them once); without it the call makes its own and destroys them.
template <class OnSegment>
int move_text(yacrd_engine *e, const TextSource &src, u64 begin, u64 n, char *mirror, bool blit, int n_threads, OnSegment &&on_segment,
              size_t chunk = kTextChunk, Streams *lanes = nullptr)
{
    // (the pinned arena stays with the engine: pinning 100 MB costs more than moving 367 MB through it)
    const size_t kChunk = chunk;
    constexpr size_t kSeg = kTextSeg;
    const size_t n_chunks = (size_t)((n + kChunk - 1) / kChunk);
    unsigned T = n_threads > 0 ? (unsigned)n_threads : 6u; // (more threads only get in each other's way: 367 MB in 10 ms with 4-8)
    T = (unsigned)std::max<size_t>(1, std::min<size_t>(std::min(T, 32u), std::max<size_t>(n_chunks, 1)));
    const size_t n_buf = (size_t)2 * T;
    if (e->paf_arena.reserve(n_buf * kChunk) != hipSuccess) return 3;
    char *arena = e->paf_arena.as<char>();
    Events ev; // one per chunk: recorded behind its copy
    Streams own;
    Streams &copy = lanes ? *lanes : own;
    std::unique_ptr<std::atomic<int>[]> landed(new std::atomic<int>[n_chunks + 1]);
    for (size_t c = 0; c <= n_chunks; c++) landed[c].store(0);
    std::atomic<size_t> next(0);
    std::atomic<int> bad(0);
    if ((copy.v.size() < T && !copy.add(T - copy.v.size())) || !ev.add(n_chunks, hipEventDisableTiming)) bad = 1;
    auto work = [&](unsigned t) { // thread t owns buffers 2t and 2t + 1: one fills while the other flies
        if (hipSetDevice(e->device) != hipSuccess) bad = 1;
        long prev[2] = {-1, -1}; // the chunk that last flew from each buffer
        for (int turn = 0; !bad.load(); turn ^= 1) {
            const size_t c = next.fetch_add(1);
            if (c >= n_chunks) break;
            const size_t b = (size_t)2 * t + (size_t)turn;
            if (prev[turn] >= 0 && hipEventSynchronize(ev[(size_t)prev[turn]]) != hipSuccess) bad = 1;
            char *dst = arena + b * kChunk;
            const size_t off = c * kChunk, clen = (size_t)std::min<u64>(kChunk, n - off);
            if (!src.fetch(dst, clen, begin + (u64)off)) bad = 2;
            if (bad.load()) break;
            if (blit && (clen & 15)) std::memset(dst + clen, 0, 16 - (clen & 15)); // (the file's last piece: zeros, not leftovers, behind it)
            if (blit) { // (the arena's buffers are 4 MiB: whole 16-byte pieces; the mirror is padded by 64 bytes)
                hipLaunchKernelGGL(yk::gp_blit_kernel, dim3(256), dim3(256), 0, copy[t], reinterpret_cast<uint4 *>(mirror + off),
                                   reinterpret_cast<const uint4 *>(dst), (u64)((clen + 15) / 16));
                if (hipEventRecord(ev[c], copy[t]) != hipSuccess) bad = 1;
            } else if (hipMemcpyAsync(mirror + off, dst, clen, hipMemcpyHostToDevice, copy[t]) != hipSuccess ||
                       hipEventRecord(ev[c], copy[t]) != hipSuccess)
                bad = 1;
            prev[turn] = (long)c;
            landed[c].store(1, std::memory_order_release); // (its event is recorded: the dispatcher may wait on it)
        }
        (void)hipStreamSynchronize(copy[t]);
    };
    std::vector<std::thread> th;
    if (!bad.load())
        for (unsigned t = 0; t < T; t++) th.emplace_back(work, t);
    // the dispatcher
    size_t waited = 0;
    for (size_t c0 = 0; c0 < n_chunks && !bad.load(); c0 += kSeg) {
        const size_t c1 = std::min(c0 + kSeg, n_chunks), need = std::min(c1 + 1, n_chunks);
        while (waited < need && !bad.load()) {
            if (!landed[waited].load(std::memory_order_acquire)) {
                struct timespec ts = {0, 20000};
                nanosleep(&ts, nullptr);
                continue;
            }
            if (hipStreamWaitEvent(e->stream, ev[waited], 0) != hipSuccess) bad = 1;
            waited++;
        }
        if (bad.load()) break;
        on_segment((u64)c0 * kChunk, (u64)c1 * kChunk, std::min<u64>(n, (u64)need * kChunk));
    }
    for (auto &x : th) x.join(); // (every thread has waited for its stream)
    own.clear();
    if (bad.load()) (void)hipStreamSynchronize(e->stream); // (kernels may still wait on events about to go, with `ev`)
    (void)hipGetLastError();
    return bad.load();
}

// What a reader of text (the device parser, the report reader) takes its text from: plain text through move_text, or — with
// `bgzf` — a BGZF stream in host memory, inflated in HBM as it lands (move_bgzf_text, gpu_inflate.hip).  The walk is the entry
// point's; `move` holds what the inflate leaves behind for the reader: the status word's place and the timed events.
struct BgzfIn {
    const char *comp = nullptr;
    u64 comp_bytes = 0, text_bytes = 0;
    std::vector<yif::InfMember> members;
    float walk_ms = 0.f;
    BgzfMove move;
    // not BGZF: YACRD_EFALLBACK
    int walk(const char *bgzf, u64 n_bytes)
    {
        const double t0 = now_ms();
        comp = bgzf ? bgzf : "", comp_bytes = n_bytes;
        if (!ybw::walk(reinterpret_cast<const unsigned char *>(comp), n_bytes, members, &text_bytes)) return fail(YACRD_EFALLBACK, "not BGZF: the host reader's");
        walk_ms = (float)(now_ms() - t0);
        return YACRD_OK;
    }
    // first_line_fields' answers for the inflated text, from the first members and the last one, decoded on the host (at most
    // 1 MiB and 64 KiB of text).  YACRD_EFALLBACK: one of them is not taken (the device would say the same), or the first
    // non-empty line outgrows the sample
    int text_ends(char delim, u32 &n_fields, bool &ends_in_newline) const
    {
        u32 status = 0;
        const int rc = bgzf_text_ends(reinterpret_cast<const unsigned char *>(comp), comp_bytes, members.data(), members.size(), (u64)1 << 20,
                                      (unsigned char)delim, &n_fields, &ends_in_newline, &status);
        if (rc == 1) return inflate_not_taken(status);
        if (rc == 2) return fail(YACRD_EFALLBACK, "the first line is longer than the sample decoded on the host: the host loop words the error");
        if (rc) return fail(YACRD_ENOMEM, "host allocation failed");
        return YACRD_OK;
    }
    // device bytes the inflate wants beside the text
    double device_bytes() const { return (double)comp_bytes + (double)(members.size() + 1) * sizeof(yif::InfMember) + 128.0; }
    // (behind a synchronisation of the engine's stream)
    void stats(yacrd_gunzip_stats *us) const
    {
        if (!us) return;
        us->in_bytes = comp_bytes, us->out_bytes = text_bytes, us->n_members = members.size();
        us->walk_ms = walk_ms, us->h2d_ms = move.h2d_ms, us->kernel_ms = move.kernel_ms(), us->d2h_ms = 0.f;
    }
};
struct TextProducer {
    TextSource src;
    BgzfIn *bgzf = nullptr;
    TextProducer() = default;
    TextProducer(const TextSource &s) : src(s) {}
    // text[0, n) -> mirror: move_text's contract and codes either way (plain text: bytes [begin, begin + n) of the source)
    template <class OnSegment>
    int move(yacrd_engine *e, u64 begin, u64 n, char *mirror, bool blit, int n_threads, OnSegment &&on_segment, int *rc_open)
    {
        *rc_open = YACRD_OK;
        if (!bgzf) return move_text(e, src, begin, n, mirror, blit, n_threads, on_segment);
        return move_bgzf_text(e, bgzf->comp, bgzf->comp_bytes, bgzf->members, reinterpret_cast<unsigned char *>(mirror), n, n_threads, on_segment,
                              bgzf->move, rc_open);
    }
    // the decoder's status word on its way to *h_status, enqueued on the engine's stream: read it behind the next synchronisation
    int fetch_inflate_status(yacrd_engine *e, u32 *h_status) const
    {
        *h_status = 0;
        if (bgzf && bgzf->move.d.status) HIP_TRY(hipMemcpyAsync(h_status, bgzf->move.d.status, sizeof(u32), hipMemcpyDeviceToHost, e->stream));
        return YACRD_OK;
    }
};

} // namespace yke
