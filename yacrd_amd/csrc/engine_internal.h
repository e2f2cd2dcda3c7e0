// engine_internal.h — host-side internals shared by the translation units of libyacrd_hip.so: engine.hip (batch runs, the
// engine's life), stream.hip (streaming ingest + CSR build on the GPU) and the text paths gpu_paf.hip, gpu_edit.hip,
// gpu_deflate.hip, gpu_inflate.hip, gpu_report.hip, gpu_report_write.hip, gpu_seq_edit.hip.  The error slot; the OWNERS of every HIP resource the library takes:
// DevBuf (device memory), PinBuf (pinned memory), Events, Streams.  Each frees what it holds when it goes, none is copied, and
// no translation unit calls the runtime's allocate / create / free / destroy functions itself (yacrd_pinned_alloc / _free, whose
// memory is the caller's, excepted); the two buffer types count the bytes they hold (live_bytes).  Then the clocks, the engine
// itself, whose members are such owners in the order their destruction needs, with its registry of the text paths' scratch, and
// the run context.
#pragma once
#include "../../include/yacrd_engine_debug.h"

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <atomic>
#include <chrono>
#include <functional>
#include <new>
#include <string>
#include <vector>

#include "bgzf_sizes.h" // (what a batch of GzDevice is counted in, below)
#include "device_common.h"

namespace yif {
struct InfMember; // (inflate_block.h: one member of a BGZF stream, as bgzf_walk.h finds it)
}

namespace yke {

// message of the last error on the calling thread (yacrd_last_error)
std::string &err_slot();
inline int fail(int code, const std::string &msg)
{
    err_slot() = msg;
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess)                                                                  \
            return yke::fail(_e == hipErrorOutOfMemory ? YACRD_ENOMEM : YACRD_ENODEV,          \
                             std::string(#expr) + ": " + hipGetErrorString(_e));              \
    } while (0)

// Bytes of device / pinned memory DevBuf / PinBuf hold right now, process-wide (yacrd_debug_live_bytes: tests).  Touched only
// where an allocation or a free happens.
inline std::atomic<uint64_t> *live_bytes() // [0] device, [1] pinned
{
    static std::atomic<uint64_t> held[2];
    return held;
}

// What DevBuf and PinBuf share: a block of `cap` bytes at `p` that goes when its holder does.  Moves, never copies.
template <class Mem>
struct OwnedBuf {
    void *p = nullptr;
    size_t cap = 0;
    OwnedBuf() = default;
    OwnedBuf(const OwnedBuf &) = delete;
    OwnedBuf &operator=(const OwnedBuf &) = delete;
    OwnedBuf(OwnedBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    OwnedBuf &operator=(OwnedBuf &&o) noexcept
    {
        if (this != &o) {
            release();
            p = o.p, cap = o.cap;
            o.p = nullptr, o.cap = 0;
        }
        return *this;
    }
    ~OwnedBuf() { release(); }
    // exactly `bytes` (nothing held after a failure)
    hipError_t reserve_exact(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        release();
        const hipError_t e = Mem::alloc(&p, bytes);
        if (e == hipSuccess) live_bytes()[Mem::kCounter] += (cap = bytes);
        else p = nullptr;
        return e;
    }
    void release()
    {
        if (!p) return;
        (void)Mem::free(p);
        live_bytes()[Mem::kCounter] -= cap;
        p = nullptr;
        cap = 0;
    }
    template <class T>
    T *as() const
    {
        return reinterpret_cast<T *>(p);
    }
};
struct DevMem {
    static constexpr int kCounter = 0;
    static hipError_t alloc(void **p, size_t n) { return hipMalloc(p, n); }
    static hipError_t free(void *p) { return hipFree(p); }
};
struct PinMem {
    static constexpr int kCounter = 1;
    static hipError_t alloc(void **p, size_t n) { return hipHostMalloc(p, n); }
    static hipError_t free(void *p) { return hipHostFree(p); }
};

// device memory, grow-only: an eighth of slack so a slightly larger batch fits, the exact size where that does not
struct DevBuf : OwnedBuf<DevMem> {
    hipError_t reserve(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        return reserve_exact(bytes + bytes / 8 + 256) == hipSuccess ? hipSuccess : reserve_exact(bytes);
    }
};

// pinned host memory, grow-only: exactly the bytes asked for (pinning costs by the byte), nothing after a failed reserve
struct PinBuf : OwnedBuf<PinMem> {
    hipError_t reserve(size_t bytes) { return reserve_exact(bytes); }
};

// the events / streams of one call: what was created goes when the holder does
struct Events {
    std::vector<hipEvent_t> v;
    Events() = default;
    Events(const Events &) = delete;
    Events &operator=(const Events &) = delete;
    // n more events; false: one could not be created
    bool add(size_t n, unsigned flags = hipEventDefault)
    {
        for (; n; n--) {
            hipEvent_t x = nullptr;
            if (hipEventCreateWithFlags(&x, flags) != hipSuccess) return false;
            v.push_back(x);
        }
        return true;
    }
    hipEvent_t operator[](size_t i) const { return v[i]; }
    ~Events()
    {
        for (hipEvent_t x : v) (void)hipEventDestroy(x);
    }
};
struct Streams {
    std::vector<hipStream_t> v;
    Streams() = default;
    Streams(const Streams &) = delete;
    Streams &operator=(const Streams &) = delete;
    bool add(size_t n)
    {
        for (; n; n--) {
            hipStream_t x = nullptr;
            if (hipStreamCreateWithFlags(&x, hipStreamNonBlocking) != hipSuccess) return false;
            v.push_back(x);
        }
        return true;
    }
    hipStream_t operator[](size_t i) const { return v[i]; }
    void clear()
    {
        for (hipStream_t x : v) (void)hipStreamDestroy(x);
        v.clear();
    }
    ~Streams() { clear(); }
};

// the error behind an add() or a reserve() that just failed on this thread (never hipSuccess)
inline hipError_t why_not_added()
{
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : hipErrorUnknown;
}

enum { EV_START = 0, EV_PLAN, EV_S0, EV_SMALL, EV_MED, EV_GEN, EV_COMPACT, EV_X0, EV_X1, EV_H2D0, EV_H2D1, EV_D2H0, EV_D2H1, EV_PLAN0, EV_COUNT }; // yacrd_engine::ev (EV_PLAN0: in front of the plan on the side stream, a direct run)
enum { EVS_DONE = 0, EVS_FORK, EVS_JOIN, EVS_COUNT };                                                                                // yacrd_engine::ev_sync

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
        else prev = -1;
    }
    ~DeviceGuard()
    {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

inline double now_ms() // host wall clock
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

inline float ev_ms(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, a, b) != hipSuccess) return 0.f;
    return ms;
}

} // namespace yke


// (Rounds 4-5 had a FusedLane here: the persistent screen + fallback launches of the engines that share a device took turns.
// Since round 6 no workgroup of that launch waits for another — screen_wg.h — and engines launch it side by side.)

// What one launch sequence covers, per size class.
struct LaunchSet {
    u32 n[12];     // reads used to size the grid; 0 = class not launched
    u32 hint[12];  // the class's size as far as the host knows it (its count, or the prediction + a margin): grids of kernels that cover a list of any length
    u32 first[12]; // first list entry the launch covers (remainder launches)
    u64 iv[12];    // intervals (to pick the dominant class)
};

// One batch on its way through run_on_device (engine.hip): built once, handed to every phase of the launch sequence.
struct Run {
    // the batch
    const u64 *d_off = nullptr;
    const uint2 *d_iv = nullptr;
    const u32 *d_len = nullptr;
    uint64_t n_reads64 = 0, n_iv = 0;
    u32 n_reads = 0;
    uint32_t cov = 0;
    double not_cov = 0;
    // decoded flags
    bool full = false;        // YACRD_F_TIMING_FULL
    bool tight_grids = false; // predicted register classes get grids with a margin, not grids for every read
    u32 prefilter = 0;        // SweepArgs.prefilter
    bool one_launch = false;  // the batch goes out as one_batch_kernel (one_batch.h)
    bool long_form = false;   // the plan and the follow-on step take their long-batch forms (yacrd_engine::long_min_reads, as reserve_buffers found it)
    // the control block in use, its scan-state words, and what the plan zeroes of the other block
    yk::Counters *ctr = nullptr;
    u32 nb = 0, ob_slabs = 0;
    size_t ctrl_bytes = 0, other_bytes = 0;
    // lists of read ids, one stride of n_reads each: the classes, then ...
    u32 *lists = nullptr;
    u32 *rej_small = nullptr, *rej_med = nullptr, *rej_big = nullptr; // ... what the register / M1 / M2 and larger sweeps reject,
    u32 *over_med = nullptr;                                          // M2 reads beyond the 256-thread kernel's keys,
    u32 *fb_med[2] = {}, *fb_big = nullptr, *fb_stream[2] = {};       // what the screens leave of M1 / M2 / BIG, and the first of two screens of M1 / M2
    u32 *list_of(int cls) const { return lists + (size_t)cls * n_reads; }
    u32 mrec_cap1 = 0, mrec_cap2 = 0; // records of plan_kernel for M1 / M2 (plan_compact.h)
    yk::SweepArgs base{};             // what every launch's SweepArgs start from (engine.hip: base_sweep_args)
    // what is launched: the plan's counts (c0, after a sync) or the previous run's (predicted)
    bool predicted = false;
    yk::Counters c0{};
    LaunchSet ls{};
    u32 big_n = 0; // reads / intervals beyond the workgroup classes the device-wide screen is launched for
    u64 big_iv = 0;
    bool big_beside = false; // ... on the side stream
    // DIRECT (engine.hip: choose_direct): the long launch takes the H16 reads by index and goes out first on the engine's stream;
    // the plan and the other register classes run beside it on the side stream, joined in front of the workgroup classes
    bool direct = false;
    // kernel-level timing: event indices bracketing each class (-1 = not recorded)
    int cls_b[12], cls_e[12];
    int n_cls_ev = 0, dom_cls = -1;
    hipStream_t cls_ev_stream = nullptr; // the stream of the last class mark (a mark is shared by neighbours on one stream only)
    bool timing_on = false;
    // what went out
    bool fused_marked = false, screened = false, big_screened = false;
};

// A batch that was submitted without waiting for it (yacrd_engine_submit_device, or the one-launch form before its wait).
struct Pending {
    bool active = false;
    bool one_launch = false;
    Run run;
};

struct yacrd_engine {
    Pending pending;
    int device = 0;
    uint32_t flags = 0;
    // Order matters to ~yacrd_engine: members go last-declared first, so every buffer below is freed before the events, and
    // the events before the streams the buffers were used on (yacrd_engine_destroy has waited for both streams by then).
    yke::Streams streams;           // owns the two below
    hipStream_t stream = nullptr;   // streams[0]
    hipStream_t side = nullptr;     // streams[1], made by the first batch that needs it: the device-wide screen's launches, beside the workgroup classes', or a direct run's plan and minor register classes, beside its long launch (run_on_device)
    yke::Events ev;      // EV_*: the phases of a run, h2d and d2h (default flags: timed)
    yke::Events ev_cls;  // 24, brackets around class kernels (timed)
    yke::Events ev_sync; // EVS_DONE: hipEventBlockingSync, the final wait of YACRD_F_BLOCKING_WAIT; EVS_FORK: stream -> side (behind the plan; a direct run: in front of everything); EVS_JOIN: side -> stream (in front of the follow-on step); none timed
    int num_cu = 256;
    bool fused_off = false; // this run: the workgroup classes down the three-launch chain (a fused launch gave up: Counters::fused_gave_up)
    int num_xcc = 0; // XCDs of this device / partition (one_batch_kernel's read-to-XCD map assumes 8)
    int screen_fused_wgs_per_cu = 0; // workgroups of screen_wg_fused_kernel a CU holds at once (its grid must be resident as a whole)

    // inputs staged by yacrd_engine_run
    yke::DevBuf in_off, in_iv, in_len;
    // work buffers
    yke::DevBuf dlist; // the follow-on step's list of marked reads (long batches: finish_compact.h, mark_list_kernel)
    uint32_t compact_calls = 0; // launch_compact calls of the current run (a redo starts the list over)
    yke::DevBuf mrec; // the workgroup classes' records (plan_compact.h)
    yke::DevBuf lists, ctrl2[2], stage, counts, closed, gen_sizes, gen_scratch_off, gen_scratch, big_tab, big_keys, big_redo, bt_tab, bt_hist, bt_cur, bt_keys, bs_seg, bs_chunk, bs_hist;
    // two control blocks (counters + scan state), used alternately: the plan kernel of a run zeroes
    // the other one for the next run.  ctrl_clean[i] = leading bytes of block i known to be zero.
    size_t ctrl_clean[2] = {0, 0};
    int ctrl_cur = 0;
    // results
    yke::DevBuf bad_offsets, bad_regions, read_type;
    yke::PinBuf h_ctr_mem;
    yk::Counters *h_ctr() const { return h_ctr_mem.as<yk::Counters>(); }

    uint64_t last_reads = 0, last_regions = 0;
    size_t last_list_stride = 0; // reads per class list of the current run (lists = [class][read])
    bool has_result = false;
    // class counts of the previous run: the prediction that lets the next one skip the plan sync
    yk::Counters pred{};
    uint64_t pred_reads = 0, pred_iv = 0;
    bool pred_valid = false;
    yacrd_timing timing = {};
    yacrd_timing timing_sum = {};
    uint64_t timing_runs = 0;
    uint32_t run_seq = 0; // runs since creation (YACRD_F_TIMING_SAMPLED times every 8th)
    uint32_t wide_left = 0;    // batches the screen still takes in its one-item build WITH the second looks (sliding windows) before the default builds are tried again
    uint32_t last_items = 1;   // groups of list entries per wavefront the last screen ran with
    bool last_wide = false;    // ... and whether it was the build with the second looks
    bool one_launch_off = false; // (while a batch the one-launch form could not take is run again on the default path)
    int last_build = -1, prev_build = -1; // build of the register classes' launch in the last run / the one before (-1: none; 0 sorting, 1 / 2 screening with one / two items, 3 second looks)
    bool miss_pending = false;            // the run in progress is the synchronous re-run of a batch whose prediction did not hold
    uint64_t direct_runs = 0;  // runs that went out direct (yacrd_debug_direct_runs)
    // the last run's reads beyond 16 384 intervals by the tier that decided them (yacrd_debug_big_routes): [0] device-wide
    // screen (conclude_run), [1] thinned and swept in LDS, [2] entered the segmented sort, [3] handed to the exact kernel
    uint64_t big_routes[4] = {0, 0, 0, 0};
    uint32_t nodefer_left = 0; // batches the sorting build of the fused launch still takes before the screen is tried again
    // pinned bounce buffers for pageable inputs (yke::h2d), allocated on first use; an event per
    // buffer says when its DMA is done and it may be refilled
    static constexpr int kBounce = 12;
    static constexpr size_t kBounceBytes = (size_t)4 << 20;
    yke::Events bounce_ev; // one per buffer that exists: buffers are made in order, each with its event or not at all
    yke::PinBuf bounce[kBounce];
    bool bounce_busy[kBounce] = {};
    yke::PinBuf h_out; // pinned staging for the results on their way home (fetch_result)
    // a batch submitted from host buffers (yacrd_engine_submit): collect() fetches the result
    bool host_pending = false;
    yke::PinBuf paf_arena; // what text passes through on its way to HBM (gpu_text.h: move_text)
    // the mirror a one-engine device parse of a whole overlap text left in HBM (gpu_paf.hip: still inside its scratch).  With
    // from_file, which file it was: the overlap editor (gpu_edit.hip) edits from it when it is handed the same file, instead of
    // moving the text again; a text that came from memory or from a BGZF stream has no file identity and never passes for one.
    // With facts, what the editor's plan asks of the text (gpu_text.h: first_line_fields), taken when the ingest had the text,
    // the file or the stream at hand: the _resident_ forms edit from the mirror with nothing but these.  Cleared (valid) by
    // the first statement of everything that rewrites or frees the parser's text, and of every ingest: the resident text is
    // the last successful overlap ingest's.
    struct {
        const unsigned char *p = nullptr; // n bytes + 64 of padding
        uint64_t n = 0, dev = 0, ino = 0;
        int64_t mtime_s = 0, mtime_ns = 0;
        bool valid = false, from_file = false;
        bool facts = false, m4 = false, ends_nl = true;
        uint32_t n_fields = 0;
    } mirror;
    // the read table the engine's last ingest left in HBM (gpu_paf.hip with one engine, gpu_report.hip): names, name_off and
    // lengths where that ingest's scratch (and in_len) hold them; with bad_offsets / bad_regions / read_type they are all a
    // report is made of (gpu_report_write.hip).  Set by a successful ingest as its last step.  Cleared by the FIRST statement
    // of every entry point that may rewrite or move one of those buffers, before any reserve or copy, whether the call then
    // succeeds or not: run, submit, their device, batch and partitioned forms, a stream's or group's finish, every ingest,
    // classify, trim.
    struct {
        const unsigned char *names = nullptr;
        const u64 *name_off = nullptr; // n_reads + 1
        const u32 *lengths = nullptr;
        uint64_t n_reads = 0;
        bool valid = false;
    } resident;
    // the input CSR the engine's last call left in ITS OWN in_off / in_iv / in_len (yacrd_debug_last_input_csr brings it home:
    // tests compare it with a reference, interval by interval).  Set as the last step of a successful call that filled those
    // buffers itself: run, submit + collect, a stream's or group's finish, the device parser with one engine or several.
    // Cleared, like `resident`, by the first statement of every entry point that may rewrite, move or release them or that
    // sweeps somebody else's pointers (the device and batch forms, ingest_report, classify, trim), so a failed call leaves none.
    struct {
        uint64_t n_reads = 0, n_iv = 0;
        bool valid = false;
    } input;
    // what the text paths keep between calls (their own types, whose members own their device and pinned buffers, events and
    // streams; nothing in them outlives a call except capacity), made on first use by yke::scratch_of; yacrd_engine_trim and
    // yacrd_engine_destroy delete them (drop_scratch), the next use after a trim makes a fresh one
    enum Slot { kPaf = 0, kEdit, kGzip, kReport, kReportWrite, kSeqEdit, kInflate, kGunzipStream, kSlots };
    struct {
        void *p = nullptr;
        void (*destroy)(void *) = nullptr;
    } scratch[kSlots];
    void drop_scratch(int k)
    {
        if (scratch[k].p) scratch[k].destroy(scratch[k].p);
        scratch[k].p = nullptr;
    }
    // the FASTQ editor's windows (gpu_seq_edit.hip): the switch yacrd_debug_seq_window set (0: the policy; UINT64_MAX: never
    // windows; else the window's bytes) and what yacrd_debug_seq_windows reports of the last sequence edit
    uint64_t seq_window = 0;
    uint64_t seq_windows[4] = {0, 0, 0, 0};
    // the overlap editor's windows (gpu_edit.hip): the switch yacrd_debug_edit_window set, with the same three meanings,
    // and what yacrd_debug_edit_windows reports of the last overlap edit
    uint64_t edit_window = 0;
    uint64_t edit_windows[4] = {0, 0, 0, 0};
    // batches of this many reads and more take the long-batch forms of the plan and the follow-on step (engine.hip:
    // split_min_reads is the default; yacrd_debug_long_min_reads sets it, tests)
    uint64_t long_min_reads = 0;
    // the plain-gzip decoder's chunk (gpu_gunzip_stream.hip): what yacrd_debug_gunzip_chunk set; 0: YACRD_GUNZIP_CHUNK, or the default
    uint32_t gunzip_chunk = 0;
    bool gzip_busy = false; // a yacrd_gzip_writer or an edit to gzip holds the kGzip slot: trim leaves it alone
};


namespace yke {
// the engine's scratch of type T, in the slot T names as kScratchSlot (nullptr: no host memory)
template <class T>
T *scratch_of(yacrd_engine *e)
{
    auto &s = e->scratch[T::kScratchSlot];
    if (!s.p && (s.p = new (std::nothrow) T())) s.destroy = [](void *p) { delete static_cast<T *>(p); };
    return static_cast<T *>(s.p);
}
// the whole launch sequence over a CSR resident in HBM (engine.hip)
int run_on_device(yacrd_engine *e, const u64 *d_off, const uint2 *d_iv, const u32 *d_len,
                  uint64_t n_reads64, uint64_t n_iv, uint32_t cov, double not_cov, bool defer = false);
// kernel #2 on a region CSR where it lies in HBM (engine.hip: classify_csr_kernel on the engine's stream; asynchronous)
int classify_on_device(yacrd_engine *e, const u64 *d_bad_offsets, const uint2 *d_bad_regions, const u32 *d_len, u32 n_reads, double not_cov,
                       uint8_t *d_read_type);
// D2H of the last result into a freshly allocated yacrd_result
int fetch_result(yacrd_engine *e, yacrd_result *out);
// overlap records in HBM -> the engine's input CSR (stream.hip; blocking), and a u32 -> u64 exclusive scan
struct RecSlab {
    const yk::OvlRec *recs;
    uint64_t n;
};
int csr_from_records(yacrd_engine *e, const RecSlab *slabs, size_t n_slabs, const u32 *d_map, u64 n_handles, u64 n_reads,
                     DevBuf &cnt, DevBuf &part, DevBuf &err, hipEvent_t done, u64 *n_intervals = nullptr,
                     bool counted = false, u64 iv_bound = 0);
int scan_u32_to_u64(yacrd_engine *e, const u32 *in, u64 n, u64 *out, DevBuf &part, hipStream_t st = nullptr /* the engine's */);
// host -> HBM at PCIe rate: direct DMA when `src` is pinned, otherwise through the engine's pinned
// bounce buffers filled by a few copy threads; asynchronous on e->stream only for pinned sources
int h2d(yacrd_engine *e, void *dst, const void *src, size_t bytes);
// text that lies in HBM -> BGZF members in HBM, batch by batch (gpu_deflate.hip; used by gpu_edit.hip)
struct GzDevice {
    const unsigned char *out[2] = {nullptr, nullptr}; // a batch's members, end to end; batches alternate between the two
    u64 max_blocks = 0;                               // blocks of ydf::kBlock bytes a batch may hold
};
int gzip_device_open(yacrd_engine *e, u64 max_blocks, GzDevice *g);
int gzip_device_encode(yacrd_engine *e, const GzDevice &g, hipStream_t st, const unsigned char *d_text, u64 n, bool last, int which,
                       hipEvent_t k0, hipEvent_t k1, volatile u64 *h_bytes, volatile u64 *h_stored);
void gzip_device_close(yacrd_engine *e);
struct GzHold { // the engine's encoder buffers are one edit's, from its gzip_device_open until it ends
    yacrd_engine *e = nullptr;
    ~GzHold()
    {
        if (e) gzip_device_close(e);
    }
};
// what an editor that deflated its output where it lay reports: `busy_ms` the way out as a whole, `put_ms` the sink's part of it
inline void fill_gzip_stats(yacrd_gzip_stats *g, u64 in_bytes, u64 out_bytes, u64 members, u64 stored, float kernel_ms, double busy_ms, double put_ms)
{
    if (!g) return;
    g->in_bytes = in_bytes, g->out_bytes = out_bytes, g->n_members = members, g->n_stored = stored;
    g->h2d_ms = 0.f, g->kernel_ms = kernel_ms; // (the text lies in HBM already)
    g->d2h_ms = (float)(busy_ms > put_ms ? busy_ms - put_ms : 0.0), g->write_ms = (float)put_ms; // (d2h: with the waits for the encoder)
}
// a BGZF stream that lies in HBM -> its text in HBM (gpu_inflate.hip; used by gpu_seq_edit.hip).  open takes the engine's
// inflate scratch for a stream of comp_bytes and the members the host's walk found (bgzf_walk.h), uploads the member table and
// zeroes the status word on the engine's stream; the caller then moves the stream's bytes to d.comp (comp_bytes + 64 bytes
// are there, 16-byte aligned).  run launches the decoder on stream `st`: member m's text to d_text + members[m].out_off,
// nothing beyond d_text[0, text_bytes); asynchronous.  Behind it *d.status is 0, or the largest yif::InfStatus a member that
// was not taken gave: the text is then not to be used.  Nothing is held between calls but capacity.
struct InflateDevice {
    unsigned char *comp = nullptr;
    const yif::InfMember *members = nullptr;
    u32 *status = nullptr;
    u64 comp_bytes = 0, n_members = 0;
    bool fresh = false; // `comp` is a new allocation (move_text's `blit`)
};
int inflate_device_open(yacrd_engine *e, u64 comp_bytes, const yif::InfMember *members, u64 n_members, InflateDevice *d);
int inflate_device_run(yacrd_engine *e, const InflateDevice &d, hipStream_t st, unsigned char *d_text, u64 text_bytes);
// the same for members [m0, m1) of the table alone (inflate_device_run: all of them): what move_bgzf_text launches as the stream lands
int inflate_device_run_range(yacrd_engine *e, const InflateDevice &d, hipStream_t st, unsigned char *d_text, u64 text_bytes, u64 m0, u64 m1);
// device bytes the inflate scratch holds (the stream's buffer and the member table): what a caller's does-it-fit check may count as free
u64 inflate_device_held(yacrd_engine *e);
// the message of a status word that is not 0 (YACRD_EFALLBACK)
int inflate_not_taken(u32 status);
// A BGZF stream in host memory -> its text at d_text[0, text_bytes) in HBM, inflated while it lands (gpu_inflate.hip; used by
// gpu_paf.hip and gpu_report.hip).  move_text (gpu_text.h) carries the COMPRESSED bytes into the inflate scratch; for every
// segment of them that has landed the planner (bgzf_plan.h) names the members that have become complete, which are launched
// on e->stream — it waits for the chunks' copy events already — and the text segments that are whole behind that launch,
// each handed to on_text_segment(t0, t1, avail) under move_text's contract: what the consumer launches on e->stream sees the
// text, the host waits for nothing.  Returns move_text's codes (0; 1 a HIP call failed, or *rc the code of an open that
// failed; 2; 3).  Behind the stream *bm.d.status is the decoder's status word (inflate_device_run), for the caller to read
// with its own first synchronisation and BEFORE it sizes anything from what the text says; bm.kernel_ms() after that.
// (the record-room estimate of a text that is not in host memory: host/inflate_sample.cc)
bool bgzf_head_lines(const unsigned char *comp, uint64_t comp_bytes, const yif::InfMember *members, uint64_t n_members, uint64_t max_text,
                     uint64_t *text, uint64_t *lines);
// (what the overlap editor's plan asks of a text that is not in host memory — the first non-empty line's field count, the
// last byte — from the first members and the last one: host/inflate_sample.cc.  0; 1 a member not taken, *status the cause;
// 2 the first non-empty line is not complete inside max_text bytes and the text goes on; 3 no memory)
int bgzf_text_ends(const unsigned char *comp, uint64_t comp_bytes, const yif::InfMember *members, uint64_t n_members, uint64_t max_text,
                   unsigned char delim, uint32_t *n_fields, bool *ends_nl, uint32_t *status);
// (bgzf_text_ends' second answer alone — whether the text's last byte is a newline — from the last member that holds text:
// what a BGZF FASTQ / FASTA in windows asks before its first launch.  0; 1 that member not taken, *status the cause; 3 no memory)
int bgzf_last_byte(const unsigned char *comp, uint64_t comp_bytes, const yif::InfMember *members, uint64_t n_members, bool *ends_nl,
                   uint32_t *status);
// A BGZF text inflated window by window (gpu_inflate.hip; used by gpu_seq_edit.hip; the cuts: bgzf_windows.h).
// open takes, in the engine's inflate scratch, ONE compressed slot of W + 64 bytes (16-byte aligned) and zeroes the status
// word on the engine's stream (release_whole, before it: the whole-stream buffer and table of inflate_device_open go).  Per
// window the caller lands the stream's bytes [c0, c1) at w.comp and calls run_window with the window's slice of the member
// table — its offsets absolute, as the walk gave them — and the window's bases: the slice goes up into a grow-only table,
// 64 zero bytes are put behind the slot's c1 - c0 bytes, and the decoder is launched on stream `st`: member m's text to
// d_text + (out_off - t0), nothing beyond d_text[0, t1 - t0).  The kernel checks every member against the window's extents
// before it reads or stores a byte: one outside them leaves kInfTable in the status word.  The inflate of the window before
// — the last reader of the slot and of the table — must have ended when the caller lands the next window's bytes and calls
// run_window (the caller's waits: gpu_seq_edit.hip argues it); other work may still be enqueued on the stream.
struct InflateWindow {
    unsigned char *comp = nullptr;
    u32 *status = nullptr;
    u64 W = 0;
    bool fresh = false; // `comp` is a new allocation (move_text's `blit`)
};
void inflate_device_release_whole(yacrd_engine *e);
int inflate_window_open(yacrd_engine *e, u64 W, InflateWindow *w);
int inflate_device_run_window(yacrd_engine *e, const InflateWindow &w, hipStream_t st, const yif::InfMember *slice, u64 n_slice, u64 c0, u64 c1,
                              u64 t0, u64 t1, unsigned char *d_text);
// device bytes the window form holds: the compressed slot and the member table
u64 inflate_window_held(yacrd_engine *e);
struct BgzfMove {
    InflateDevice d;
    Events ev; // a timed pair around every launch
    size_t n_ev = 0, n_launches = 0;
    float h2d_ms = 0.f;
    float kernel_ms() const;
};
int move_bgzf_text(yacrd_engine *e, const char *comp_src, u64 comp_bytes, const std::vector<yif::InfMember> &members, unsigned char *d_text,
                   u64 text_bytes, int n_threads, const std::function<void(u64, u64, u64)> &on_text_segment, BgzfMove &bm, int *rc);
// ONE plain gzip member in host memory -> its text in HBM (gpu_gunzip_stream.hip; inflate_stream.h: the five steps; used by
// gpu_seq_edit.hip's _gz_ forms).  Mirrors inflate_device_open / _run.  open walks the header (gzip_walk.h), moves the
// compressed bytes up through move_text, FINDs block starts per chunk, SIZEs the spans with the chain's repair rounds, checks
// ISIZE, and takes the symbol scratch (2 bytes per text byte): behind it s->text_bytes is the text's exact size and the
// chain is proven, before a byte is stored.  `text_copies`: how many buffers of the text's size the caller will take beside the
// symbols (the primitive: its text; an editor: its text and an output that may be as long) and `held` the device bytes it already
// holds for them: where (text_copies + 2) x text does not fit beside the compressed bytes, YACRD_EFALLBACK, with nothing reserved.
// stream_inflate_release frees the compressed bytes and the symbols at once (a caller that hands the input on to the host route).
// run enqueues SYMBOLS, WINDOWS and BYTES on the engine's stream into d_text (16-byte aligned, text_bytes of it are written),
// brings the status word and the CRC home and WAITS: YACRD_OK means the text is the member's, checked against the trailer;
// the status is read before the caller sizes anything from the text.  YACRD_EFALLBACK: not one gzip member, or a payload the
// decoder does not take (the message names the cause).  Nothing is held between calls but capacity (slot kGunzipStream).
struct StreamInflate {
    u64 text_bytes = 0, n_true = 0;
    u32 crc = 0;
    yacrd_gunzip_stream_stats stats = {};
};
int stream_inflate_open(yacrd_engine *e, const char *gz, u64 n_bytes, int n_threads, double text_copies, double held, StreamInflate *s);
void stream_inflate_release(yacrd_engine *e);
int stream_inflate_run(yacrd_engine *e, StreamInflate &s, unsigned char *d_text);
} // namespace yke
