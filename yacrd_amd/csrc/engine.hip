// engine.hip — C ABI of include/yacrd_engine.h: buffer management, launch sequence, timing.
//
// Launch sequence per run (one HIP stream per engine):
//   plan (also zeroes the other control block for the next run) -> [sync: class counts, unless predicted]
//   -> sweeps of the non-empty classes
//   -> exact general path (LDS scratch for rejected reads; global scratch for huge reads)
//   -> compact_classify (single-pass scan) -> sync.
//   Rare redo: degenerate reads too large for LDS, or bad_regions too small.
// A long batch of mostly H16 reads goes out DIRECT (choose_direct): the long launch first, by read index, on the engine's
// stream; plan, counts and the other register classes beside it on the side stream; joined in front of the rest.
// Several engines may share a device (one host thread each): their batches pipeline.
// run_on_device is that sequence as a list of phases; each phase takes the engine and the Run (engine_internal.h).
#include "engine_internal.h"

#include <time.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "device_common.h"
#include "plan_compact.h"
#include "sweep_big.h"
#include "sweep_wave.h"
#include "sweep_big_trim.h"
#include "sweep_general.h"
#include "sweep_lds.h"
#include "finish_compact.h"
#include "screen_wg.h"
#include "screen_stream.h"
#include "screen_big.h"
#include "one_batch.h"

using namespace yke;

// One reader for the A/B and test knobs of the environment (each is looked up once per process, by its accessor below).
static uint64_t env_u64(const char *name, uint64_t dflt)
{
    const char *v = std::getenv(name);
    return v ? std::strtoull(v, nullptr, 10) : dflt;
}

// The deferring build of the fused launch (healthy-read screen) is used from this many intervals in the
// classes R16 + H16 on (YACRD_DEFER_MIN_IV overrides, for A/B), unless the previous batches deferred more
// than a quarter of what they screened: then the sorting build runs for kProbeEvery - 1 batches before the
// screen is tried again.
static uint64_t defer_min_intervals()
{
    static const uint64_t v = env_u64("YACRD_DEFER_MIN_IV", 4000000ull);
    return v;
}
static constexpr uint32_t kProbeEvery = 16;

// Batches of this many reads and more take the follow-on step as kernels of its own (finish_compact.h: mark_list_kernel +
// deferred_list_kernel + scan_compact_kernel) and the plan as plan_kernel<4>; YACRD_SPLIT_MIN_READS overrides (A/B: 0 = always, a
// huge number = never).  The default of yacrd_engine::long_min_reads, which yacrd_debug_long_min_reads sets per engine (tests).
static uint64_t split_min_reads()
{
    static const uint64_t v = env_u64("YACRD_SPLIT_MIN_READS", (uint64_t)yk::kPlanSmallReads);
    return v;
}

// YACRD_FUSED_SHARE / YACRD_TEST_FUSED_GRID_MULT (A/B, tests): reads per workgroup and turn of screen_wg_fused_kernel (0: the
// default), and a multiple of its grid
static uint64_t fused_share_override()
{
    static const uint64_t v = std::min<uint64_t>(env_u64("YACRD_FUSED_SHARE", 0), 4096);
    return v;
}
static uint64_t fused_grid_mult()
{
    static const uint64_t v = std::max<uint64_t>(1, env_u64("YACRD_TEST_FUSED_GRID_MULT", 1));
    return v;
}

namespace yke {
std::string &err_slot()
{
    thread_local std::string s;
    return s;
}
} // namespace yke

namespace {

// What every launch's SweepArgs start from: the batch, the stage / counts / closed arrays, the control block; no list; what a
// sweep rejects goes to the register classes' rejection list, what overflows an LDS sweep to over_med.  Built once per run
// (Run::base); a launch site takes a copy and sets what its kernel needs on the copy.
yk::SweepArgs base_sweep_args(const yacrd_engine *e, const Run &R)
{
    yk::SweepArgs sa;
    sa.off = R.d_off, sa.iv = R.d_iv, sa.len = R.d_len, sa.cov = R.cov, sa.prefilter = R.prefilter;
    sa.list = nullptr, sa.list_n = nullptr, sa.rec = nullptr, sa.first = 0;
    sa.stage = e->stage.as<uint2>(), sa.counts = e->counts.as<u32>(), sa.closed = e->closed.as<uint2>(), sa.ctr = R.ctr;
    sa.rej_list = R.rej_small, sa.rej_count = &R.ctr->rej_small;
    sa.over_list = R.over_med, sa.over_count = &R.ctr->over_med;
    return sa;
}
// ... and over one list
yk::SweepArgs list_sweep_args(const Run &R, const u32 *list, const u32 *list_n)
{
    yk::SweepArgs sa = R.base;
    sa.list = list;
    sa.list_n = list_n;
    return sa;
}

// scan + compact + classify (finish_compact.h, one_batch.h): the run's inputs, stage / counts, the register classes' rejection
// list (the follow-on kernel's sort appends to it), the outputs
yk::CompactArgs2 compact_args(const yacrd_engine *e, const Run &R)
{
    yk::CompactArgs2 ca;
    ca.sweep = R.base;
    ca.sweep.over_list = nullptr;
    ca.sweep.over_count = nullptr;
    ca.scan_state = reinterpret_cast<u64 *>(R.ctr + 1);
    ca.n_reads = R.n_reads;
    ca.not_cov = R.not_cov;
    ca.bad_offsets = e->bad_offsets.as<u64>();
    ca.bad_regions = e->bad_regions.as<uint2>();
    ca.region_cap = (u64)(e->bad_regions.cap / sizeof(uint2));
    ca.read_type = e->read_type.as<uint8_t>();
    ca.host_ctr = e->h_ctr();
    return ca;
}

// The follow-on step: finish the deferred reads + scan + compact + classify, and the totals come home.
int launch_compact(yacrd_engine *e, const Run &R)
{
    const u32 n_reads = R.n_reads;
    const yk::CompactArgs2 ca = compact_args(e, R);
    if (R.long_form) {
        if (R.screened) {
            // the marks listed, the list dealt out evenly over a grid that is resident as a whole (finish_compact.h)
            const u32 slabs = (n_reads + yk::kMarkReads - 1) / yk::kMarkReads;
            yk::DeferList dl;
            dl.shard_cap = (slabs / yk::kDeferShards + 1u) * (u32)yk::kMarkReads;
            HIP_TRY(e->dlist.reserve((size_t)yk::kDeferShards * dl.shard_cap * sizeof(u32)));
            dl.list = e->dlist.as<u32>();
            dl.count = reinterpret_cast<u32 *>(ca.scan_state + R.nb);
            if (e->compact_calls++) // (a redo of the follow-on step: the list starts over)
                HIP_TRY(hipMemsetAsync(dl.count, 0, (size_t)yk::kDeferShards * yk::kDeferShardStride * sizeof(u32), e->stream));
            hipLaunchKernelGGL(yk::mark_list_kernel, dim3(slabs), dim3(yk::kMarkThreads), 0, e->stream, ca.sweep.counts, n_reads, dl);
            hipLaunchKernelGGL(yk::deferred_list_kernel, dim3((u32)e->num_cu * (u32)(YK_LIST_OCC * 256 / yk::kListThreads)), dim3(yk::kListThreads), 0,
                               e->stream, ca.sweep, dl);
        }
        // (eight reads per thread: 65.1 us against 55.6 on configs[4], profiles/r05/m_*: half the tickets, but twice the latency chain per thread)
        hipLaunchKernelGGL(yk::scan_compact_kernel<4>, dim3((n_reads + 4 * yk::kScanThreads - 1) / (4 * yk::kScanThreads)), dim3(yk::kScanThreads), 0, e->stream, ca);
        return YACRD_OK;
    }
    // The counter block goes home from inside the kernel (its last slab: finish_compact.h): no copy command —
    // a 4 us dispatch of its own — behind it.  (Rounds 2-3 tried this with a ticket per workgroup to find the
    // last one to FINISH: 1 953 same-address tickets on 2 M reads cost more than the copy.  The slab that ends
    // the batch needs no ticket: its look-back has seen everyone else's aggregate.)
    hipLaunchKernelGGL(yk::finish_compact_kernel, dim3((n_reads + yk::kScanBlock - 1) / yk::kScanBlock), dim3(yk::kScanBlock), 0, e->stream, ca);
    return YACRD_OK;
}

// Sizes / offsets of `count` listed reads, to the host (one sync).
int gather_reads(yacrd_engine *e, const u64 *d_off, const u32 *d_len, const u32 *d_list, u32 count,
                 hipStream_t stream, std::vector<yk::GatherOut> &out)
{
    HIP_TRY(e->gen_sizes.reserve((size_t)count * sizeof(yk::GatherOut)));
    hipLaunchKernelGGL(yk::gather_general_sizes_kernel, dim3((count + 255) / 256), dim3(256), 0,
                       stream, d_off, d_len, d_list, count, e->gen_sizes.as<yk::GatherOut>());
    out.resize(count);
    HIP_TRY(hipMemcpyAsync(out.data(), e->gen_sizes.p, (size_t)count * sizeof(yk::GatherOut),
                           hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    for (const auto &g : out)
        if (g.n >= 0x7FFFFFFFull) return fail(YACRD_EINVAL, "a read has >= 2^31 - 1 intervals");
    return YACRD_OK;
}

// Global-memory exact path over `count` reads listed at d_list (host knows the count).  Those beyond 16 384 intervals are
// counted in big_routes[3]: the lists it is given also hold smaller reads (rej_big: the LDS classes' rejections; the whole
// batch under YACRD_F_FORCE_GENERAL).
int run_general_global(yacrd_engine *e, const u64 *d_off, const uint2 *d_iv, const u32 *d_len,
                       const u32 *d_list, u32 count, u32 cov, hipStream_t stream)
{
    std::vector<yk::GatherOut> info;
    int rc = gather_reads(e, d_off, d_len, d_list, count, stream, info);
    if (rc) return rc;
    for (const auto &g : info)
        if (2 * g.n > (u64)yk::kMedium2Events) e->big_routes[3]++;
    HIP_TRY(e->gen_scratch_off.reserve((size_t)count * sizeof(u64)));
    std::vector<u64> offs(count);
    u64 tot = 0;
    for (u32 i = 0; i < count; i++) {
        offs[i] = tot;
        tot += 3 * info[i].n + 2;
    }
    HIP_TRY(e->gen_scratch.reserve((size_t)tot * sizeof(u64)));
    HIP_TRY(hipMemcpyAsync(e->gen_scratch_off.p, offs.data(), (size_t)count * sizeof(u64),
                           hipMemcpyHostToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream)); // `offs` must outlive the copy
    yk::GeneralArgs ga;
    ga.off = d_off;
    ga.iv = d_iv;
    ga.len = d_len;
    ga.list = d_list;
    ga.scratch_off = e->gen_scratch_off.as<u64>();
    ga.scratch = e->gen_scratch.as<u64>();
    ga.cov = cov;
    ga.stage = e->stage.as<uint2>();
    ga.counts = e->counts.as<u32>();
    hipLaunchKernelGGL(yk::sweep_general_kernel, dim3(count), dim3(yk::kGenThreads), 0, stream, ga);
    return YACRD_OK;
}

// Reads with more than 16 384 intervals that the trimming filter could not thin: device-wide
// segmented sort + chunked sweep (sweep_big.h).  Reads that turn out to hold a degenerate interval
// are appended to `redo` for the exact general kernel.
int run_big_sort(yacrd_engine *e, const uint2 *d_iv, const std::vector<yk::GatherOut> &info, u32 cov,
                 hipStream_t stream, std::vector<u32> &redo)
{
    const u32 count = (u32)info.size();
    e->big_routes[2] += count;
    std::vector<yk::BigSeg> segs(count);
    std::vector<u32> chunk_seg;
    u64 key_off = 0;
    u32 max_P = 0;
    for (u32 i = 0; i < count; i++) {
        u64 P = yk::kBigC;
        while (P < 2 * info[i].n) P <<= 1;
        if (P > 0x80000000ull) return fail(YACRD_EINVAL, "a read has more than 2^30 intervals");
        yk::BigSeg &sg = segs[i];
        sg.key_off = key_off;
        sg.iv_off = info[i].iv_off;
        sg.P = (u32)P;
        sg.n = (u32)info[i].n;
        sg.len = info[i].len;
        sg.read = info[i].read;
        sg.chunk_off = (u32)chunk_seg.size();
        sg.pad = 0;
        for (u64 c = 0; c < P / yk::kBigC; c++) chunk_seg.push_back(i);
        key_off += P;
        max_P = std::max(max_P, (u32)P);
    }
    const size_t n_chunks = chunk_seg.size();
    if (n_chunks >= 0x7FFFFFFFull / (yk::kBigC / 2)) return fail(YACRD_EINVAL, "big path: too many keys");
    const size_t tab_bytes = (size_t)count * sizeof(yk::BigSeg) + n_chunks * sizeof(u32) +
                             9 * n_chunks * sizeof(u32) + (size_t)count * sizeof(u32) + 64;
    HIP_TRY(e->big_tab.reserve(tab_bytes));
    HIP_TRY(e->big_keys.reserve((size_t)key_off * sizeof(u32)));
    char *base = e->big_tab.as<char>();
    yk::BigArgs a;
    a.seg = reinterpret_cast<yk::BigSeg *>(base);
    u32 *w = reinterpret_cast<u32 *>(base + (size_t)count * sizeof(yk::BigSeg));
    a.chunk_seg = w;
    w += n_chunks;
    u32 **per_chunk[] = {&a.c_delta, &a.c_depth_in, &a.c_mf, &a.c_ml, &a.c_mf_in,
                         &a.c_ml_in, &a.c_cnt, &a.c_pos, &a.c_cand};
    for (u32 **pp : per_chunk) {
        *pp = w;
        w += n_chunks;
    }
    a.seg_bad = w;
    a.keys = e->big_keys.as<u32>();
    a.iv = d_iv;
    a.n_chunks = (u32)n_chunks;
    a.n_segs = count;
    a.cov = cov;
    a.stage = e->stage.as<uint2>();
    a.counts = e->counts.as<u32>();
    HIP_TRY(hipMemcpyAsync((void *)a.seg, segs.data(), (size_t)count * sizeof(yk::BigSeg),
                           hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync((void *)a.chunk_seg, chunk_seg.data(), n_chunks * sizeof(u32),
                           hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(a.seg_bad, 0, (size_t)count * sizeof(u32), stream));
    hipLaunchKernelGGL(yk::big_fill_kernel, dim3((u32)n_chunks), dim3(yk::kBigT), 0, stream, a);
    yk::launch_big(a, max_P, stream);
    std::vector<u32> bad(count);
    HIP_TRY(hipMemcpyAsync(bad.data(), a.seg_bad, (size_t)count * sizeof(u32), hipMemcpyDeviceToHost,
                           stream));
    HIP_TRY(hipStreamSynchronize(stream)); // host tables must outlive the copies
    HIP_TRY(hipGetLastError());
    for (u32 i = 0; i < count; i++)
        if (bad[i]) redo.push_back(info[i].read);
    return YACRD_OK;
}

int run_big(yacrd_engine *e, const u64 *d_off, const uint2 *d_iv, const u32 *d_len,
            const u32 *d_list, u32 count, u32 cov, hipStream_t stream)
{
    std::vector<yk::GatherOut> info;
    int rc = gather_reads(e, d_off, d_len, d_list, count, stream, info);
    if (rc) return rc;
    std::vector<u32> redo; // reads for the exact general path (an interval the keys cannot express)

    // ---- first attempt: thin the reads with the device-wide pile-trimming filter (sweep_big_trim.h);
    // what fits one workgroup's LDS afterwards is swept there, the rest takes the segmented sort below
    if (!(e->flags & YACRD_F_NO_PREFILTER)) {
        std::vector<yk::BtSeg> bs(count);
        std::vector<u32> chunk_seg;
        for (u32 i = 0; i < count; i++) {
            yk::BtSeg &b = bs[i];
            b.iv_off = info[i].iv_off;
            b.n = (u32)info[i].n;
            b.len = info[i].len;
            b.read = info[i].read;
            b.chunk_off = (u32)chunk_seg.size();
            b.flags = 0;
            b.m_new = 0;
            b.n_zl = 0;
            b.pad = 0;
            for (u64 c = 0; c < (info[i].n + yk::kBtChunk - 1) / yk::kBtChunk; c++) chunk_seg.push_back(i);
        }
        const size_t n_chunks = chunk_seg.size();
        const size_t tab_words = (size_t)count * 3 * yk::kBtSeq;
        HIP_TRY(e->bt_tab.reserve((size_t)count * sizeof(yk::BtSeg) + n_chunks * sizeof(u32) + 64));
        HIP_TRY(e->bt_hist.reserve(tab_words * sizeof(u32)));
        HIP_TRY(e->bt_cur.reserve((2 * tab_words + (size_t)count * (3 * yk::kBtSeq / 32)) * sizeof(u32)));
        HIP_TRY(e->bt_keys.reserve((size_t)count * yk::kBtCap * sizeof(u32)));
        yk::BtArgs ba;
        ba.seg = e->bt_tab.as<yk::BtSeg>();
        ba.chunk_seg = reinterpret_cast<const u32 *>(e->bt_tab.as<char>() + (size_t)count * sizeof(yk::BtSeg));
        ba.iv = d_iv;
        ba.n_chunks = (u32)n_chunks;
        ba.n_segs = count;
        ba.cov = cov;
        ba.hist = e->bt_hist.as<u32>();
        ba.cur = e->bt_cur.as<u32>();
        ba.lim = e->bt_cur.as<u32>() + tab_words;
        ba.drop = e->bt_cur.as<u32>() + 2 * tab_words;
        ba.tkeys = e->bt_keys.as<u32>();
        ba.stage = e->stage.as<uint2>();
        ba.counts = e->counts.as<u32>();
        HIP_TRY(hipMemcpyAsync((void *)ba.seg, bs.data(), (size_t)count * sizeof(yk::BtSeg),
                               hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync((void *)ba.chunk_seg, chunk_seg.data(), n_chunks * sizeof(u32),
                               hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemsetAsync(ba.hist, 0, tab_words * sizeof(u32), stream));
        yk::Counters *ctr = e->ctrl2[e->ctrl_cur].as<yk::Counters>();
        u32 *rej = e->lists.as<u32>() + (size_t)(yk::CLS_COUNT + 2) * e->last_list_stride;
        hipLaunchKernelGGL(yk::bt_hist_kernel, dim3((u32)n_chunks), dim3(yk::kBtT), 0, stream, ba);
        hipLaunchKernelGGL(yk::bt_plan_kernel, dim3(count), dim3(yk::kBtT), 0, stream, ba);
        hipLaunchKernelGGL(yk::bt_scatter_kernel, dim3((u32)n_chunks), dim3(yk::kBtT), 0, stream, ba);
        hipLaunchKernelGGL(yk::bt_sweep_kernel, dim3(count), dim3(1024), 0, stream, ba, rej, &ctr->rej_big);
        HIP_TRY(hipMemcpyAsync(bs.data(), (void *)ba.seg, (size_t)count * sizeof(yk::BtSeg),
                               hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream)); // host tables must outlive the copies
        HIP_TRY(hipGetLastError());
        std::vector<yk::GatherOut> rest;
        for (u32 i = 0; i < count; i++) {
            if (bs[i].flags & yk::BT_TRIMMED) {
                e->big_routes[1]++; // (bt_sweep_kernel may still have rejected it: then it is in rej_big as well)
                continue;
            }
            if (bs[i].flags & yk::BT_BAD) redo.push_back(info[i].read);
            else rest.push_back(info[i]);
        }
        info.swap(rest);
        count = (u32)info.size();
    }
    if (count) {
        rc = run_big_sort(e, d_iv, info, cov, stream, redo);
        if (rc) return rc;
    }
    if (!redo.empty()) { // degenerate interval in a huge read: exact path, single workgroup each
        HIP_TRY(e->big_redo.reserve(redo.size() * sizeof(u32)));
        HIP_TRY(hipMemcpyAsync(e->big_redo.p, redo.data(), redo.size() * sizeof(u32),
                               hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        rc = run_general_global(e, d_off, d_iv, d_len, e->big_redo.as<u32>(), (u32)redo.size(), cov, stream);
        if (rc) return rc;
    }
    return YACRD_OK;
}

// The run's final wait: spinning (hipStreamSynchronize) or, with YACRD_F_BLOCKING_WAIT, polling
// an event and sleeping in between (hipEventSynchronize spins as well, blocking-sync flag or not).
int wait_for_stream(yacrd_engine *e)
{
    if (e->flags & YACRD_F_BLOCKING_WAIT) {
        HIP_TRY(hipEventRecord(e->ev_sync[EVS_DONE], e->stream));
        for (;;) {
            const hipError_t q = hipEventQuery(e->ev_sync[EVS_DONE]);
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) HIP_TRY(q);
            struct timespec ts = {0, 20000};
            nanosleep(&ts, nullptr);
        }
    } else {
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    HIP_TRY(hipGetLastError());
    return YACRD_OK;
}

int conclude_run(yacrd_engine *e, const Run &R, float extra_ms);
int finish_pending(yacrd_engine *e);

// ---- the phases of a run, in launch order.  Each takes the engine and the run; what a kernel is handed can be read off
// its launch site: a copy of R.base with that launch's fields set.

// Every buffer of the run, the control block of this run (zeroed) and the list pointers.
int reserve_buffers(yacrd_engine *e, Run &R)
{
    const u32 n_reads = R.n_reads;
    const uint64_t n_reads64 = R.n_reads64;
    // (scan-state words: one per slab of the follow-on kernel; one_batch_kernel: one per slab + its arrival counters)
    R.ob_slabs = (n_reads + yk::kObSlab - 1) / yk::kObSlab;
    R.nb = R.one_launch ? 2 * R.ob_slabs : (n_reads + yk::kScanBlock - 1) / yk::kScanBlock;
    constexpr int kLists = yk::CLS_COUNT + 9; // class lists + three rejection lists + M2 overflow + what the screens leave of M1 / M2 / BIG + what the one-wavefront screen leaves of M1 / M2
    HIP_TRY(e->lists.reserve((size_t)kLists * n_reads * sizeof(u32)));
    // (long batches: + the shard counters of the follow-on step's list of marked reads, behind the scan words)
    R.long_form = n_reads64 >= e->long_min_reads;
    const size_t shard_ctr_bytes = (!R.one_launch && R.long_form) ? (size_t)yk::kDeferShards * yk::kDeferShardStride * sizeof(u32) : 0;
    R.ctrl_bytes = (sizeof(yk::Counters) + (size_t)R.nb * sizeof(u64) + shard_ctr_bytes + 255) & ~(size_t)255;
    e->compact_calls = 0;
    e->ctrl_cur ^= 1;
    const int cur = e->ctrl_cur, other = cur ^ 1;
    for (int i = 0; i < 2; i++) {
        const void *before = e->ctrl2[i].p;
        HIP_TRY(e->ctrl2[i].reserve(R.ctrl_bytes));
        if (e->ctrl2[i].p != before) e->ctrl_clean[i] = 0; // fresh allocation: nothing zeroed yet
    }
    HIP_TRY(e->stage.reserve((size_t)(R.n_iv + 2 * n_reads64) * sizeof(uint2)));
    HIP_TRY(e->counts.reserve((size_t)n_reads * sizeof(u32)));
    HIP_TRY(e->closed.reserve((size_t)n_reads * sizeof(uint2)));
    HIP_TRY(e->read_type.reserve((size_t)n_reads));
    if (e->bad_regions.cap < (size_t)(4 * n_reads64 + 1024) * sizeof(uint2))
        HIP_TRY(e->bad_regions.reserve((size_t)(4 * n_reads64 + 1024) * sizeof(uint2)));

    // (a read of M1 has more than 512 intervals, one of M2 more than 4 096: that many records at most)
    R.mrec_cap1 = (u32)std::min<u64>(n_reads64, R.n_iv / 513 + 1), R.mrec_cap2 = (u32)std::min<u64>(n_reads64, R.n_iv / 4097 + 1);
    HIP_TRY(e->mrec.reserve(((size_t)R.mrec_cap1 + R.mrec_cap2) * sizeof(uint4)));
    R.lists = e->lists.as<u32>();
    e->last_list_stride = n_reads;
    R.rej_small = R.list_of(yk::CLS_COUNT), R.rej_med = R.list_of(yk::CLS_COUNT + 1);
    R.rej_big = R.list_of(yk::CLS_COUNT + 2), R.over_med = R.list_of(yk::CLS_COUNT + 3);
    R.fb_med[0] = R.list_of(yk::CLS_COUNT + 4), R.fb_med[1] = R.list_of(yk::CLS_COUNT + 5);
    R.fb_big = R.list_of(yk::CLS_COUNT + 6);
    R.fb_stream[0] = R.list_of(yk::CLS_COUNT + 7), R.fb_stream[1] = R.list_of(yk::CLS_COUNT + 8);
    R.ctr = e->ctrl2[cur].as<yk::Counters>();
    R.base = base_sweep_args(e, R);

    // The control block (counters + scan state) must start out zero.  The engine alternates
    // between two blocks and the plan kernel of a run zeroes the other one, so in steady state no
    // run starts with a fill (hipMemsetAsync = two fill kernels + their launch gaps).
    if (e->ctrl_clean[cur] < R.ctrl_bytes) HIP_TRY(hipMemsetAsync(R.ctr, 0, R.ctrl_bytes, e->stream));
    e->ctrl_clean[cur] = 0;
    R.other_bytes = std::min<size_t>(e->ctrl2[other].cap, (size_t)1 << 30) & ~(size_t)3;
    return YACRD_OK;
}

// YACRD_F_ONE_LAUNCH: the whole batch as one kernel (one_batch.h).
int launch_one_batch(yacrd_engine *e, Run &R)
{
    const int other = e->ctrl_cur ^ 1;
    yk::OneBatchArgs oa;
    oa.c = compact_args(e, R);
    oa.slab_ctr = oa.c.scan_state + R.ob_slabs;
    oa.n_slabs = R.ob_slabs;
    oa.zero = e->ctrl2[other].as<u32>();
    oa.zero_words = (u32)(R.other_bytes / 4);
    e->h_ctr()->ob_unsupported = 0; // (written from the device only when set)
    e->h_ctr()->scan_ticket = 0;    // (the slab that ends the batch sends the counters home: nb tickets then)
    // (one wavefront per kObReads reads; slabs go round the XCDs, so the grid is whole rounds of eight slabs)
    hipLaunchKernelGGL(yk::one_batch_kernel, dim3(((R.ob_slabs + 7) / 8) * 8 * (u32)(yk::kObSlab / yk::kObReads)), dim3(64), 0, e->stream, oa);
    e->ctrl_clean[other] = R.other_bytes;
    if (R.full) HIP_TRY(hipEventRecord(e->ev[EV_COMPACT], e->stream));
    return YACRD_OK;
}

// plan: bin reads by size class (it also zeroes the other control block for the next run).
int launch_plan(yacrd_engine *e, Run &R)
{
    const int other = e->ctrl_cur ^ 1;
    const u32 n_reads = R.n_reads;
    const u32 plan_mode = (u32)((e->flags & YACRD_F_FORCE_GENERAL) ? 1
                                : (e->flags & (YACRD_F_WAVE_ONLY | YACRD_F_FORCE_LDS_SORT)) ? 2
                                : (e->flags & YACRD_F_NO_HALVES) ? 3 : 0);
    if (R.direct) { // beside the long launch, on the side stream: 256-thread workgroups (plan_compact.h), H16 counted only
        constexpr u32 per_wg = (u32)(yk::kPlanSidePer * yk::kPlanSideBlock);
        if (R.full) HIP_TRY(hipEventRecord(e->ev[EV_PLAN0], e->side));
        hipLaunchKernelGGL((yk::plan_kernel<yk::kPlanSidePer, yk::kPlanSideBlock>), dim3((n_reads + per_wg - 1) / per_wg), dim3(yk::kPlanSideBlock), 0, e->side,
                           R.d_off, n_reads, R.lists, R.ctr, plan_mode | yk::kPlanDirect, e->ctrl2[other].as<u32>(), (u32)(R.other_bytes / 4),
                           e->counts.as<u32>(), e->mrec.as<uint4>(), R.mrec_cap1, R.mrec_cap2);
        e->ctrl_clean[other] = R.other_bytes;
        if (R.full) HIP_TRY(hipEventRecord(e->ev[EV_PLAN], e->side));
        return YACRD_OK;
    }
    if (!R.long_form)
        hipLaunchKernelGGL((yk::plan_kernel<1, yk::kPlanSmallBlock>), dim3((n_reads + yk::kPlanSmallBlock - 1) / yk::kPlanSmallBlock),
                           dim3(yk::kPlanSmallBlock), 0, e->stream, R.d_off, n_reads, R.lists, R.ctr, plan_mode, e->ctrl2[other].as<u32>(), (u32)(R.other_bytes / 4), e->counts.as<u32>(), e->mrec.as<uint4>(), R.mrec_cap1, R.mrec_cap2);
    else // (eight reads per thread — 611 workgroups instead of 1 221 on configs[4] — measured 32.0 us against 29.9: profiles/r05/m_*)
        hipLaunchKernelGGL(yk::plan_kernel<4>, dim3((n_reads + 4 * yk::kPlanBlock - 1) / (4 * yk::kPlanBlock)),
                           dim3(yk::kPlanBlock), 0, e->stream, R.d_off, n_reads, R.lists, R.ctr, plan_mode,
                           e->ctrl2[other].as<u32>(), (u32)(R.other_bytes / 4), e->counts.as<u32>(), e->mrec.as<uint4>(), R.mrec_cap1, R.mrec_cap2);
    e->ctrl_clean[other] = R.other_bytes;
    if (R.full) HIP_TRY(hipEventRecord(e->ev[EV_PLAN], e->stream));
    return YACRD_OK;
}

// Only classes that hold reads are launched (an empty launch costs ~4 us and there are twelve
// classes), so the host needs the class counts.  Normally that is one sync right here.  When the
// previous run on this engine had the same shape (reads, intervals, flags) its class set is used as
// a PREDICTION instead: the sweeps are launched without waiting, sized for n_reads, and the
// prediction is validated against the real counts at the final sync (a class that was not predicted
// is launched then and the compaction redone).  Streams of similar batches never pay the
// mid-pipeline sync.
bool prediction_holds(const yacrd_engine *e, const Run &R)
{
    // (round 6: a batch that holds reads beyond the workgroup classes is predicted too — until then it always waited for the
    // plan's counts, ~20 us of configs[3]'s step —: the device-wide screen is launched for the previous run's count and intervals
    // of such reads, which must come out the same, and must have left nothing to the host-driven sort)
    const bool big_predictable = !(e->flags & YACRD_F_NO_PREFILTER) && e->pred.fb_big == 0;
    return e->pred_valid && e->pred_reads == R.n_reads64 && e->pred_iv == R.n_iv &&
           (e->pred.n[yk::CLS_GENERAL] == 0 || big_predictable) &&
           !(e->flags & (YACRD_F_FORCE_GENERAL | YACRD_F_NO_PREDICTION));
}

// Whether this run's long launch goes out DIRECT (screen_reg.h: screen_block_rows; Run::direct).  Legal where the register
// classes' launch is the long-launch build — deferring, two items, no second looks, the default prefilter and plan mode —;
// worth it where nearly every row of the launch holds an H16 read and nothing needs the host between the plan and the
// follow-on step.  A wrong guess costs idle rows, never a result.  R.predicted is set.
bool choose_direct(yacrd_engine *e, const Run &R)
{
    const uint32_t f = e->flags;
    if (f & YACRD_F_NO_SCREEN_DIRECT) return false;
    // flags that pin another path or another build, and the counting prefilter (one more writer of the control block)
    if (f & (YACRD_F_FORCE_GENERAL | YACRD_F_WAVE_ONLY | YACRD_F_FORCE_LDS_SORT | YACRD_F_NO_HALVES | YACRD_F_NO_PREFILTER |
             YACRD_F_COUNT_PREFILTERED | YACRD_F_NO_DEFER | YACRD_F_SCREEN_ITEMS_1 | YACRD_F_SCREEN_WIDE))
        return false;
    const bool forced = (f & YACRD_F_SCREEN_DIRECT) != 0;
    if (!forced) {
        // the build launch_register_classes would choose must be the two-items one
        if (!(f & YACRD_F_ALWAYS_DEFER) && e->nodefer_left != 0) return false;
        if (!(f & YACRD_F_SCREEN_ITEMS_2) && e->wide_left != 0) return false;
        if (R.n_reads64 < (uint64_t)yk::kPlanSmallReads) return false;
        if (R.predicted) {
            const yk::Counters &p = e->pred;
            const u64 fused_iv = p.iv[yk::CLS_R16] + p.iv[yk::CLS_H16];
            if (!(f & YACRD_F_SCREEN_ITEMS_2) && fused_iv < 40000000ull) return false;
            if (!(f & YACRD_F_ALWAYS_DEFER) && fused_iv < defer_min_intervals()) return false;
            if (8 * (u64)p.n[yk::CLS_H16] < 7 * R.n_reads64) return false;
            if (p.n[yk::CLS_MED1] || p.n[yk::CLS_MED2] || p.n[yk::CLS_GENERAL]) return false;
        } else {
            // no counts yet: the mean read is H16 and the batch is long enough for the two-items build whatever its classes hold
            if (!(f & YACRD_F_SCREEN_ITEMS_2) && R.n_iv < 40000000ull) return false;
            if (!(f & YACRD_F_ALWAYS_DEFER) && R.n_iv < defer_min_intervals()) return false;
            if (!(R.n_iv > 128 * R.n_reads64 && R.n_iv <= 256 * R.n_reads64)) return false;
        }
    }
    if (e->side == nullptr) {
        if (e->streams.add(1)) e->side = e->streams[1];
        else (void)hipGetLastError(); // (no side stream: the list form, as ever)
    }
    return e->side != nullptr;
}

// (a direct run: the counter copy and the wait are the side stream's, the long launch is already running)
int size_launches(yacrd_engine *e, Run &R)
{
    const uint64_t n_reads64 = R.n_reads64;
    LaunchSet &ls = R.ls;
    if (R.predicted) {
        // Register-sort classes: one workgroup per 4..16 reads, so the grid is sized for the
        // predicted count plus a margin (idle workgroups are not free: 19 000 of them cost ~3 us);
        // reads beyond the grid are swept by a remainder launch after the validation.  The LDS
        // classes run grid-stride loops and need no margin.
        for (int cls = 0; cls < yk::CLS_GENERAL; cls++) {
            const u64 p = e->pred.n[cls];
            const u64 cap = (cls <= yk::CLS_W16 && R.tight_grids) ? ((p + p / 8 + 64 + 15) & ~(u64)15)
                                                                 : n_reads64;
            ls.n[cls] = p ? (u32)std::min<u64>(cap, (n_reads64 + 15) & ~(u64)15) : 0;
            ls.hint[cls] = p ? (u32)std::min<u64>(p + p / 8 + 64, n_reads64) : 0;
            ls.iv[cls] = e->pred.iv[cls];
        }
        R.big_n = e->pred.n[yk::CLS_GENERAL], R.big_iv = e->pred.iv[yk::CLS_GENERAL];
    } else {
        const hipStream_t hs = R.direct ? e->side : e->stream;
        HIP_TRY(hipMemcpyAsync(e->h_ctr(), R.ctr, sizeof(yk::Counters), hipMemcpyDeviceToHost, hs));
        HIP_TRY(hipStreamSynchronize(hs));
        R.c0 = *e->h_ctr();
        for (int cls = 0; cls < yk::CLS_GENERAL; cls++) {
            ls.n[cls] = R.c0.n[cls];
            ls.hint[cls] = R.c0.n[cls];
            ls.iv[cls] = R.c0.iv[cls];
        }
        R.big_n = R.c0.n[yk::CLS_GENERAL], R.big_iv = R.c0.iv[yk::CLS_GENERAL];
    }
    if (R.direct) {
        // the direct launch covers every read of the batch: H16 is never "missing" or "larger than its grid" (recover,
        // finish_pending), whatever the plan counts, and its list — which nobody wrote — is never asked for
        ls.n[yk::CLS_H16] = (u32)std::min<u64>((n_reads64 + 15) & ~(u64)15, 0xFFFFFFFFull);
        ls.hint[yk::CLS_H16] = R.n_reads;
    }
    for (int cls = 0; cls < yk::CLS_GENERAL; cls++)
        if (ls.n[cls] && (R.dom_cls < 0 || ls.iv[cls] > ls.iv[R.dom_cls])) R.dom_cls = cls;
    return YACRD_OK;
}

// Kernel-level timing.  An event costs ~3 us of stream time, so by default only the class
// with the most intervals (the dominant kernel) is bracketed; YACRD_F_TIMING_FULL brackets
// every launched class and the phases.
// `hs`: the stream the class is launched on (the engine's; a direct run's minor register classes: the side stream).
hipError_t before_class(yacrd_engine *e, Run &R, int cls, hipStream_t hs)
{
    if (!R.timing_on || !(R.full || cls == R.dom_cls)) return hipSuccess;
    if (R.n_cls_ev > 0 && R.full && R.cls_ev_stream == hs) { // the previous class's end mark is this one's begin mark
        R.cls_b[cls] = R.n_cls_ev - 1;
        return hipSuccess;
    }
    R.cls_b[cls] = R.n_cls_ev;
    R.cls_ev_stream = hs;
    return hipEventRecord(e->ev_cls[R.n_cls_ev++], hs);
}
hipError_t mark_class(yacrd_engine *e, Run &R, int cls, hipStream_t hs)
{
    if (!R.timing_on || !(R.full || cls == R.dom_cls)) return hipSuccess;
    R.cls_e[cls] = R.n_cls_ev;
    R.cls_ev_stream = hs;
    return hipEventRecord(e->ev_cls[R.n_cls_ev++], hs);
}

// The register-sort classes of `set`: the row / half-wavefront classes R2..H16 in one launch, the one-read-per-wavefront
// classes W2..W16 a launch each.  (What they reject is looked at after the final sync.)  `again`: a second pass.
// A direct run (launch_direct_screen has the H16 reads): the first pass goes out on the side stream, in the long-launch build.
int launch_register_classes(yacrd_engine *e, Run &R, const LaunchSet &set, bool again)
{
    yk::Counters *ctr = R.ctr;
    const bool fuse = !(e->flags & YACRD_F_FORCE_LDS_SORT);
    const hipStream_t hs = (R.direct && !again) ? e->side : e->stream;
    if (fuse) {
        yk::FusedArgs fa;
        fa.base = R.base; // (list / list_n / first: per class, from the table below)
        // R16 / H16: the healthy-read screen, the rest left to finish_compact_kernel — unless the last
        // batches failed the screen too often (e->nodefer_left: see conclude_run)
        const u64 fused_iv = set.iv[yk::CLS_R16] + set.iv[yk::CLS_H16];
        const bool defer = R.direct || (R.prefilter && !(e->flags & YACRD_F_NO_DEFER) &&
                                        ((e->flags & YACRD_F_ALWAYS_DEFER) ||
                                         (fused_iv >= defer_min_intervals() && e->nodefer_left == 0)));
        // two groups of list entries per wavefront in the screened classes when the launch streams from
        // HBM (more than the 256 MiB Infinity Cache holds): twice the loads in flight per wavefront
        // ... unless the last screened batch left more than a tenth of its reads to the sort: then the one-item build WITH
        // the second looks (sliding windows, screen_reg.h) takes the next kProbeEvery - 1 — dovetail ends spread by
        // hundreds of positions need them (configs[1] at sigma = 100: 79 % decided against 95 %; configs[2] at 300: 79 %
        // against 97 %), reads that do not are a tenth faster without (conclude_run: wide_left)
        const bool wide = defer && !R.direct && !(e->flags & YACRD_F_SCREEN_ITEMS_2) && ((e->flags & YACRD_F_SCREEN_WIDE) || e->wide_left > 0);
        const int items = !defer ? 1
                          : (wide || (e->flags & YACRD_F_SCREEN_ITEMS_1)) ? 1
                          : (R.direct || (e->flags & YACRD_F_SCREEN_ITEMS_2) || fused_iv >= 40000000ull) ? 2 : 1;
        e->last_items = (uint32_t)items;
        e->last_wide = wide;
        if (!again) e->last_build = !defer ? 0 : wide ? 3 : items;
        fa.base.over_list = nullptr; // (the deferring build marks its reads in counts[])
        fa.base.over_count = nullptr;
        fa.n_entries = 0;
        fa.direct = 0, fa.n_reads = R.n_reads;
        u32 blocks = 0;
        bool has_dom = false;
        for (int cls = yk::CLS_R2; cls <= yk::CLS_H16; cls++) {
            if (!set.n[cls] || (R.direct && cls == yk::CLS_H16)) continue; // (a direct run's H16 reads: launch_direct_screen)
            const u32 per = yk::sweep_group_reads_per_block(cls, defer ? yk::kDeferWaves : yk::kFusedWaves) *
                            (cls >= yk::CLS_R16 ? (u32)items : 1u);
            blocks += (set.n[cls] + per - 1) / per;
            fa.cls[fa.n_entries] = (u32)cls;
            fa.block_end[fa.n_entries] = blocks;
            fa.list[fa.n_entries] = R.list_of(cls);
            fa.list_n[fa.n_entries] = &ctr->n[cls];
            fa.first[fa.n_entries] = set.first[cls];
            fa.n_entries++;
            has_dom |= cls == R.dom_cls;
        }
        if (fa.n_entries) {
            const bool mark = R.timing_on && (R.full || has_dom) && !R.direct; // (a direct run's bracket is the long launch's)
            // the launch's build, chosen once: sorting; screening with one item, with the second looks, with two items
            void (*kernel)(yk::FusedArgs) = yk::sweep_small_fused_kernel;
            u32 threads = 64 * yk::kFusedWaves;
            if (defer && items == 2) kernel = yk::sweep_small_fused_defer2_kernel, threads = 64;
            else if (defer && wide) kernel = yk::sweep_small_fused_defer_wide_kernel, threads = 64 * yk::kDeferWaves;
            else if (defer) kernel = yk::sweep_small_fused_defer_kernel, threads = 64 * yk::kDeferWaves;
            // start / stop events attached to the launch itself (hipExtLaunchKernelGGL): the
            // kernel's own dispatch timestamps, no event packets before and after it.
            // (Until round 6 engines that share a device — batches pipelined over several engines — could take turns with
            // this launch, a GPU-side wait on the previous engine's end-of-sweep event: the hand-over cost ~10 us per batch
            // (configs[1], three engines: 47.0 us per batch with turns, 38.8 without), and a sweep that fills the GPU leaves
            // the next one little room to overlap anyway (its bracket grows by ~1 us: what the roofline then reports is on
            // the safe side).)
            hipExtLaunchKernelGGL(kernel, dim3(blocks), dim3(threads), 0, hs, mark ? e->ev_cls[22] : (hipEvent_t) nullptr,
                                  mark ? e->ev_cls[23] : (hipEvent_t) nullptr, 0, fa);
            if (mark) R.fused_marked = true;
            if (defer && (set.n[yk::CLS_R16] || set.n[yk::CLS_H16])) R.screened = true;
        }
    }
    for (int cls = fuse ? yk::CLS_W2 : yk::CLS_R2; cls <= yk::CLS_W16; cls++) { // register sort per lane group
        if (!set.n[cls]) continue;
        HIP_TRY(before_class(e, R, cls, hs));
        yk::SweepArgs sa = list_sweep_args(R, R.list_of(cls), &ctr->n[cls]);
        sa.first = set.first[cls];
        if (!fuse) { // YACRD_F_FORCE_LDS_SORT
            const u32 grid = (u32)std::min<uint64_t>(set.n[cls], (uint64_t)e->num_cu * 32);
            hipLaunchKernelGGL((yk::sweep_lds_kernel<64, (int)yk::kSmallEvents>), dim3(grid), dim3(64), 0, hs, sa);
        } else {
            switch (cls) {
            case yk::CLS_W2: yk::launch_sweep_group<64, 2>(sa, set.n[cls], hs); break;
            case yk::CLS_W4: yk::launch_sweep_group<64, 4>(sa, set.n[cls], hs); break;
            case yk::CLS_W8: yk::launch_sweep_group<64, 8>(sa, set.n[cls], hs); break;
            default: yk::launch_sweep_group<64, 16>(sa, set.n[cls], hs); break;
            }
        }
        HIP_TRY(mark_class(e, R, cls, hs));
    }
    // (a direct run's first pass: run_on_device records the mark behind the join)
    if (R.full && R.timing_on && hs == e->stream) HIP_TRY(hipEventRecord(e->ev[EV_SMALL], e->stream));
    return YACRD_OK;
}

// A direct run's long launch: every H16 read of the batch by its index, four rows per wavefront (screen_reg.h:
// screen_block_rows), on the engine's stream and in front of everything else — it reads no list and no class count.
void launch_direct_screen(yacrd_engine *e, Run &R)
{
    yk::FusedArgs fa;
    fa.base = R.base;
    fa.base.over_list = nullptr;
    fa.base.over_count = nullptr;
    fa.n_entries = 1;
    fa.cls[0] = (u32)yk::CLS_H16;
    fa.block_end[0] = R.n_reads / 4u + (R.n_reads % 4u ? 1u : 0u);
    fa.first[0] = 0;
    fa.list[0] = nullptr;
    fa.list_n[0] = nullptr;
    fa.direct = 1, fa.n_reads = R.n_reads;
    const bool mark = R.timing_on; // (start / stop events attached to the launch: no packets of their own)
    hipExtLaunchKernelGGL(yk::sweep_small_fused_defer2_kernel, dim3(fa.block_end[0]), dim3(64), 0, e->stream, mark ? e->ev_cls[22] : (hipEvent_t) nullptr,
                          mark ? e->ev_cls[23] : (hipEvent_t) nullptr, 0, fa);
    if (mark) R.fused_marked = true;
    R.screened = true;
    e->last_items = 2, e->last_wide = false, e->last_build = 2;
    e->direct_runs++;
}

// A workgroup class (k = 0: M1, 1: M2), the screen and its fallback fused.  Two launches (round 6, profiles/r06/m_*): the
// SCREEN alone — screen_wg_kernel: 100 VGPRs, 8 KB of LDS, no scratch, one read per workgroup handed out by the dispatcher:
// 0.118-0.128 ms on configs[3] — appends what it cannot decide (a fiftieth of the generator's reads) to a list, and
// screen_wg_fused_kernel takes THAT list: table again, filtered exact sweep, the whole-read sort for what is left.  With the
// fallback code inside the screening launch the same screens took 0.163 ms before a single fallback read ran (128 VGPRs,
// 88 bytes of scratch written by every workgroup, 74 KB of LDS), and 0.212 with them.
// YACRD_F_STREAM_SCREEN (A/B): the first launch is the one-wavefront-per-read screen (screen_stream.h).
int launch_workgroup_class_fused_screen(yacrd_engine *e, Run &R, const LaunchSet &set, int k, bool again)
{
    yk::Counters *ctr = R.ctr;
    const int cls = k == 0 ? yk::CLS_MED1 : yk::CLS_MED2;
    if (again) { // (a second pass over the class: the lists start over)
        HIP_TRY(hipMemsetAsync(&ctr->fb_stream[k], 0, sizeof(u32), e->stream));
        HIP_TRY(hipMemsetAsync(&ctr->fb_med[k], 0, sizeof(u32), e->stream));
    }
    {
        yk::SweepArgs ss = list_sweep_args(R, R.list_of(cls), &ctr->n[cls]); // (rej_*: the base's, no screen rejects a read)
        ss.over_list = R.fb_stream[k];
        ss.over_count = &ctr->fb_stream[k];
        const u32 want = std::max<u32>(set.hint[cls], 1u);
        if (e->flags & YACRD_F_STREAM_SCREEN) {
            hipLaunchKernelGGL(yk::screen_stream_kernel, dim3((u32)std::min<uint64_t>(want, (uint64_t)e->num_cu * 96)), dim3(64), 0, e->stream, ss);
        } else {
            ss.rec = e->mrec.as<uint4>() + (k == 0 ? 0u : R.mrec_cap1);
            hipLaunchKernelGGL(yk::screen_wg_kernel, dim3((u32)std::min<uint64_t>(want, (uint64_t)e->num_cu * 64)), dim3(yk::kWsT), 0, e->stream, ss);
        }
    }
    yk::ScreenFusedArgs fa;
    fa.sweep = list_sweep_args(R, R.fb_stream[k], &ctr->fb_stream[k]); // (over_*: over_med, the base's)
    fa.sweep.rej_list = k == 0 ? R.rej_med : R.rej_big;
    fa.sweep.rej_count = k == 0 ? &ctr->rej_med : &ctr->rej_big;
    fa.n_fallback = &ctr->fb_med[k];
    // (its list is what the screen left: one read per workgroup, a stride loop should the list be longer than the grid.
    //  YACRD_TEST_FUSED_GRID_MULT / YACRD_FUSED_SHARE, tests / A/B: a multiple of that grid, reads per workgroup and turn)
    const u64 known = std::max<u32>(set.hint[cls], 1u);
    u64 share = 1;
    if (fused_share_override()) share = std::min<u64>(fused_share_override(), (u64)yk::kFusedShareMax);
    fa.share = (u32)share;
    const u32 gs = (u32)std::min<u64>(std::min<u64>((known + share - 1) / share, (u64)e->num_cu * 4) * fused_grid_mult(), 0x7FFFFFFFull);
    hipLaunchKernelGGL(yk::screen_wg_fused_kernel, dim3(gs), dim3(yk::kWsT), 0, e->stream, fa);
    if (k == 1) { // what does not fit the in-kernel fallback's 16 384 events even filtered (usually nothing)
        yk::SweepArgs so = list_sweep_args(R, R.over_med, &ctr->over_med); // (over_*: over_med again — cannot happen: 32 768 events hold every M2 read)
        so.rej_list = R.rej_big;
        so.rej_count = &ctr->rej_big;
        const u32 grid = (u32)std::min<uint64_t>(set.n[cls], (uint64_t)e->num_cu);
        hipLaunchKernelGGL((yk::sweep_lds_kernel<1024, (int)yk::kMedium2Events>), dim3(grid), dim3(1024), 0, e->stream, so);
    }
    return YACRD_OK;
}

// A workgroup class down the chain of separate launches (round 3's; YACRD_F_NO_FUSED_SCREEN, YACRD_F_NO_PREFILTER, and the
// re-run after a fused launch gave up): the screen, then the trimming filter + LDS sort over what it leaves.
int launch_workgroup_class_chain(yacrd_engine *e, Run &R, const LaunchSet &set, int k, bool again)
{
    yk::Counters *ctr = R.ctr;
    const int cls = k == 0 ? yk::CLS_MED1 : yk::CLS_MED2;
    const u32 *list = R.list_of(cls), *list_n = &ctr->n[cls];
    if (R.prefilter) {
        if (again) HIP_TRY(hipMemsetAsync(&ctr->fb_med[k], 0, sizeof(u32), e->stream)); // (its entries are done)
        yk::SweepArgs ss = list_sweep_args(R, list, list_n); // (rej_*: the base's, the screen rejects no read)
        ss.over_list = R.fb_med[k];
        ss.over_count = &ctr->fb_med[k];
        const u32 gs = (u32)std::min<uint64_t>(set.n[cls], (uint64_t)e->num_cu * 4);
        hipLaunchKernelGGL(yk::screen_wg_kernel, dim3(gs), dim3(yk::kWsT), 0, e->stream, ss);
        list = R.fb_med[k], list_n = &ctr->fb_med[k];
    }
    yk::SweepArgs sa = list_sweep_args(R, list, list_n); // (over_*: over_med, the base's)
    sa.rej_list = k == 0 ? R.rej_med : R.rej_big;
    sa.rej_count = k == 0 ? &ctr->rej_med : &ctr->rej_big;
    if (k == 0) {
        const u32 grid = (u32)std::min<uint64_t>(set.n[cls], (uint64_t)e->num_cu * 4);
        hipLaunchKernelGGL((yk::sweep_lds_kernel<256, (int)yk::kMedium1Events>), dim3(grid), dim3(256), 0, e->stream, sa);
        return YACRD_OK;
    }
    yk::SweepArgs so = sa; // the 1024-thread kernel's: the class as it stands, or what the 256-thread kernel leaves
    if (R.prefilter) {
        // first through the 256-thread kernel (five workgroups per CU): a read whose
        // filtered keys fit its 8192-key array is done there, the others land in over_med
        const u32 g256 = (u32)std::min<uint64_t>(set.n[cls], (uint64_t)e->num_cu * 5);
        hipLaunchKernelGGL((yk::sweep_lds_kernel<256, (int)yk::kMedium1Events>), dim3(g256), dim3(256), 0, e->stream, sa);
        so.list = R.over_med;
        so.list_n = &ctr->over_med;
    }
    const u32 grid = (u32)std::min<uint64_t>(set.n[cls], (uint64_t)e->num_cu);
    hipLaunchKernelGGL((yk::sweep_lds_kernel<1024, (int)yk::kMedium2Events>), dim3(grid), dim3(1024), 0, e->stream, so);
    return YACRD_OK;
}

// One read per workgroup: M1 and M2.  First the healthy-read screen (screen_wg.h: the read in registers, one pass,
// closed form); what it cannot finish lands in a fallback list for the trimming filter + LDS sort.
int launch_workgroup_classes(yacrd_engine *e, Run &R, const LaunchSet &set, bool again)
{
    const bool fused_screen = R.prefilter && !(e->flags & YACRD_F_NO_FUSED_SCREEN) && !e->fused_off && e->screen_fused_wgs_per_cu > 0;
    for (int k = 0; k < 2; k++) {
        const int cls = k == 0 ? yk::CLS_MED1 : yk::CLS_MED2;
        if (!set.n[cls]) continue;
        HIP_TRY(before_class(e, R, cls, e->stream));
        const int rc = fused_screen ? launch_workgroup_class_fused_screen(e, R, set, k, again)
                                    : launch_workgroup_class_chain(e, R, set, k, again);
        if (rc) return rc;
        HIP_TRY(mark_class(e, R, cls, e->stream));
    }
    if (R.full && R.timing_on) HIP_TRY(hipEventRecord(e->ev[EV_MED], e->stream));
    return YACRD_OK;
}

// What the M1 sweeps rejected (a degenerate interval): the exact path with its scratch in LDS.
void launch_rejected_medium(yacrd_engine *e, Run &R, const LaunchSet &set)
{
    if (!set.n[yk::CLS_MED1]) return;
    yk::SweepArgs sa = list_sweep_args(R, R.rej_med, &R.ctr->rej_med);
    sa.rej_list = R.rej_big;
    sa.rej_count = &R.ctr->rej_big;
    hipLaunchKernelGGL((yk::sweep_general_lds_kernel<1024, 4096>), dim3(e->num_cu), dim3(1024), 0, e->stream, sa);
}

// sweeps of the classes in `set`
int launch_sweeps(yacrd_engine *e, Run &R, const LaunchSet &set, bool again = false)
{
    int rc = launch_register_classes(e, R, set, again);
    if (!rc) rc = launch_workgroup_classes(e, R, set, again);
    if (!rc) launch_rejected_medium(e, R, set);
    return rc;
}

// `count` reads beyond the LDS classes, `iv_big` intervals in all (the plan's counts, or the previous run's: a prediction the
// final sync checks).  The device-wide healthy-read screen (screen_big.h) on stream `hs`; what it cannot decide lands in fb_big
// and takes the trimming filter / the segmented sort after the final sync.
// YACRD_F_FORCE_GENERAL / YACRD_F_NO_PREFILTER: the host-driven paths directly, on the engine's stream.
int launch_device_wide_screen_on(yacrd_engine *e, Run &R, u32 count, u64 iv_big, hipStream_t hs)
{
    yk::Counters *ctr = R.ctr;
    e->big_routes[1] = e->big_routes[2] = e->big_routes[3] = 0; // (a second pass, behind a missed prediction, starts over)
    if (e->flags & YACRD_F_FORCE_GENERAL)
        return run_general_global(e, R.d_off, R.d_iv, R.d_len, R.list_of(yk::CLS_GENERAL), count, R.cov, e->stream);
    if (!R.prefilter)
        return run_big(e, R.d_off, R.d_iv, R.d_len, R.list_of(yk::CLS_GENERAL), count, R.cov, e->stream);
    const u64 max_chunks = iv_big / yk::kBsChunk + count;
    if (max_chunks >= 0x7FFFFFFFull) return fail(YACRD_EINVAL, "too many intervals in reads beyond 16384");
    HIP_TRY(e->bs_seg.reserve((size_t)count * sizeof(yk::BsSeg)));
    HIP_TRY(e->bs_chunk.reserve((size_t)max_chunks * sizeof(u32)));
    HIP_TRY(e->bs_hist.reserve((size_t)count * 2 * yk::kBsBins * sizeof(u32)));
    yk::BsArgs ba;
    ba.off = R.d_off, ba.iv = R.d_iv, ba.len = R.d_len;
    ba.list = R.list_of(yk::CLS_GENERAL);
    ba.list_n = &ctr->n[yk::CLS_GENERAL];
    ba.seg = e->bs_seg.as<yk::BsSeg>();
    ba.chunk_seg = e->bs_chunk.as<u32>();
    ba.n_chunks = &ctr->bs_chunks;
    ba.hist = e->bs_hist.as<u32>();
    ba.max_chunks = (u32)max_chunks, ba.max_segs = count;
    ba.cov = R.cov, ba.count_healthy = R.prefilter == 2 ? 1u : 0u;
    ba.stage = R.base.stage, ba.counts = R.base.counts;
    ba.fb_list = R.fb_big, ba.fb_count = &ctr->fb_big;
    ba.ctr = ctr;
    if (R.big_screened) HIP_TRY(hipMemsetAsync(&ctr->fb_big, 0, sizeof(u32), hs)); // (a second pass: its entries are done)
    HIP_TRY(hipMemsetAsync(ba.hist, 0, (size_t)count * 2 * yk::kBsBins * sizeof(u32), hs));
    hipLaunchKernelGGL(yk::bs_setup_kernel, dim3(1), dim3(1024), 0, hs, ba);
    hipLaunchKernelGGL(yk::bs_minmax_kernel, dim3((u32)max_chunks), dim3(yk::kBsT), 0, hs, ba);
    hipLaunchKernelGGL(yk::bs_hist_kernel, dim3((u32)max_chunks), dim3(yk::kBsT), 0, hs, ba);
    hipLaunchKernelGGL(yk::bs_verdict_kernel, dim3(count), dim3(yk::kBsVT), 0, hs, ba);
    R.big_screened = true;
    return YACRD_OK;
}
// The device-wide screen's four short launches (a dozen microseconds each, dependent, a few hundred workgroups) go out on a
// stream of their own BESIDE the other classes' sweeps (round 6): behind them, as until round 5, they were 45 us of
// configs[3]'s 0.31 ms with the device mostly idle.  Fork behind the plan (launch_device_wide_screen, called in front of the
// sweeps), join in front of the follow-on step (join_device_wide_screen, called behind them).
int launch_device_wide_screen(yacrd_engine *e, Run &R)
{
    // (a direct run's side stream and fork / join events are taken: its device-wide screen goes out behind the join)
    const bool can_fork = R.big_n != 0 && R.prefilter && !(e->flags & YACRD_F_FORCE_GENERAL) && !R.direct;
    if (can_fork && e->side == nullptr) {
        if (e->streams.add(1)) e->side = e->streams[1];
        else (void)hipGetLastError(); // (no side stream: the launches go out behind the other classes', as until round 5)
    }
    R.big_beside = can_fork && e->side != nullptr;
    if (!R.big_beside) return YACRD_OK;
    HIP_TRY(hipEventRecord(e->ev_sync[EVS_FORK], e->stream));
    HIP_TRY(hipStreamWaitEvent(e->side, e->ev_sync[EVS_FORK], 0));
    const int rc = launch_device_wide_screen_on(e, R, R.big_n, R.big_iv, e->side);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(e->ev_sync[EVS_JOIN], e->side));
    return YACRD_OK;
}
int join_device_wide_screen(yacrd_engine *e, Run &R)
{
    if (R.big_beside) HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_sync[EVS_JOIN], 0));
    else if (R.big_n) return launch_device_wide_screen_on(e, R, R.big_n, R.big_iv, e->stream);
    return YACRD_OK;
}

// Reads a register sweep (or the follow-on kernel's sort) rejected — an interval the keys cannot
// express: the exact path with its scratch in LDS.  Rare, so nothing is launched for them before their number is known.
void launch_rejected_small(yacrd_engine *e, Run &R)
{
    yk::SweepArgs sa = list_sweep_args(R, R.rej_small, &R.ctr->rej_small);
    sa.rej_list = R.rej_med; // cannot happen (n <= 512), kept well defined
    sa.rej_count = &R.ctr->rej_med;
    // (a single wavefront per read was tried: 23.9 us vs 20.2 us — the stages are latency
    // chains, more threads shorten each one)
    hipLaunchKernelGGL((yk::sweep_general_lds_kernel<256, 512>), dim3(e->num_cu * 2), dim3(256), 0, e->stream, sa);
}

// Everything after the final sync, the rare slow paths: a class the prediction missed; degenerate reads too large for the
// LDS exact path; what the device-wide screen left; region overflow.  Each ends with a redo of the compaction (its time: extra_ms).
int recover(yacrd_engine *e, Run &R, float &extra_ms)
{
    yk::Counters *ctr = R.ctr;
    int rc = YACRD_OK;
    bool redo = false;
    if (R.predicted) {
        R.c0 = *e->h_ctr(); // the plan's real counts
        const yk::Counters &c0 = R.c0;
        LaunchSet missing{};
        bool any_missing = false;
        for (int cls = 0; cls < yk::CLS_GENERAL; cls++)
            if (c0.n[cls] > R.ls.n[cls]) { // class not predicted, or larger than its grid
                missing.first[cls] = (cls <= yk::CLS_W16 && R.tight_grids) ? R.ls.n[cls] : 0;
                missing.n[cls] = c0.n[cls] - missing.first[cls];
                missing.hint[cls] = missing.n[cls];
                any_missing = true;
            }
        const bool big_mismatch = c0.n[yk::CLS_GENERAL] != R.big_n || c0.iv[yk::CLS_GENERAL] != R.big_iv;
        if (any_missing || big_mismatch) {
            e->miss_pending = true; // (the prediction did not hold: yacrd_timing.prediction_misses)
            HIP_TRY(hipEventRecord(e->ev[EV_X0], e->stream));
            // (the device-wide screen's first pass counted the reads it decided — of the min(real, predicted) it looked at,
            // all but its fallback list — and the second pass counts every one again: take the first count back)
            if (big_mismatch && R.big_screened && R.prefilter == 2)
                HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)&ctr->prefiltered,
                                          (int)(c0.prefiltered - (std::min(c0.n[yk::CLS_GENERAL], R.big_n) - c0.fb_big)), 1, e->stream));
            if (any_missing && (rc = launch_sweeps(e, R, missing, true))) return rc;
            if (big_mismatch && c0.n[yk::CLS_GENERAL] &&
                (rc = launch_device_wide_screen_on(e, R, c0.n[yk::CLS_GENERAL], c0.iv[yk::CLS_GENERAL], e->stream))) return rc;
            // the rejection counters may have grown: bring them home before looking at rej_big
            HIP_TRY(hipMemcpyAsync(e->h_ctr(), ctr, sizeof(yk::Counters), hipMemcpyDeviceToHost, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
            redo = true;
        }
    }
    // (A redo of the follow-on kernel may reject more reads: the loop below looks again.)
    u32 rej_small_done = 0;
    if (e->h_ctr()->rej_small) {
        if (!redo) HIP_TRY(hipEventRecord(e->ev[EV_X0], e->stream));
        launch_rejected_small(e, R);
        rej_small_done = e->h_ctr()->rej_small;
        redo = true;
    }
    if (R.big_screened && e->h_ctr()->fb_big) { // BIG reads the screen could not decide: trimming filter / segmented sort
        if (!redo) HIP_TRY(hipEventRecord(e->ev[EV_X0], e->stream));
        rc = run_big(e, R.d_off, R.d_iv, R.d_len, R.fb_big, e->h_ctr()->fb_big, R.cov, e->stream);
        if (rc) return rc;
        // (its rejections — a degenerate interval in a huge read — went the exact way inside run_big; the other
        // rejection counters may have grown)
        HIP_TRY(hipMemcpyAsync(e->h_ctr(), ctr, sizeof(yk::Counters), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        redo = true;
    }
    const u32 n_rej_big = e->h_ctr()->rej_big;
    if (n_rej_big) {
        if (!redo) HIP_TRY(hipEventRecord(e->ev[EV_X0], e->stream));
        rc = run_general_global(e, R.d_off, R.d_iv, R.d_len, R.rej_big, n_rej_big, R.cov, e->stream);
        if (rc) return rc;
        redo = true;
    }
    for (int attempt = 0; attempt < 4; attempt++) {
        if (!redo && e->h_ctr()->rej_small > rej_small_done) { // the redone follow-on kernel rejected reads of its own
            HIP_TRY(hipEventRecord(e->ev[EV_X0], e->stream));
            launch_rejected_small(e, R);
            rej_small_done = e->h_ctr()->rej_small;
            redo = true;
        }
        if (!redo) {
            if (!e->h_ctr()->region_overflow) break;
            HIP_TRY(e->bad_regions.reserve((size_t)(e->h_ctr()->total_regions + 16) * sizeof(uint2)));
            HIP_TRY(hipEventRecord(e->ev[EV_X0], e->stream));
        }
        redo = false;
        // reset the scan state, the ticket and the overflow flag (keep the class counters)
        HIP_TRY(hipMemsetAsync(&ctr->region_overflow, 0, 3 * sizeof(u32), e->stream));
        HIP_TRY(hipMemsetAsync(ctr + 1, 0, (size_t)R.nb * sizeof(u64), e->stream));
        rc = launch_compact(e, R);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(e->ev[EV_X1], e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(hipGetLastError());
        extra_ms += ev_ms(e->ev[EV_X0], e->ev[EV_X1]);
    }
    if (e->h_ctr()->region_overflow) return fail(YACRD_EINTERNAL, "bad_regions overflow persisted");
    if (e->h_ctr()->rej_small > rej_small_done) return fail(YACRD_EINTERNAL, "rejected reads persisted");
    return YACRD_OK;
}

} // namespace

namespace yke {
// A workgroup of the fused workgroup screen ran out of looks at its queue slot (screen_wg.h: the grid was not resident as a
// whole): whatever the batch's kernels wrote is void — the batch from the start, the workgroup classes down the three-launch chain.
static int rerun_without_fused(yacrd_engine *e, const Run R) // (a copy: the re-run may reuse e->pending)
{
    e->fused_off = true;
    e->pred_valid = false;
    const int rc = run_on_device(e, R.d_off, R.d_iv, R.d_len, R.n_reads64, R.n_iv, R.cov, R.not_cov, false);
    e->fused_off = false;
    return rc;
}

// The batch is out, its final wait and conclusion are finish_pending's: now, or when the caller comes back for it (`defer`).
// (The one place that fills e->pending.)
static int hand_over(yacrd_engine *e, const Run &R, bool defer)
{
    e->pending = Pending{true, R.one_launch, R};
    return defer ? YACRD_OK : finish_pending(e);
}

// Launch sequence per run: see the head of this file.  `defer` (yacrd_engine_submit_device): return without the final wait
// where the batch allows it; finish_pending has the rest.
int run_on_device(yacrd_engine *e, const u64 *d_off, const uint2 *d_iv, const u32 *d_len,
                  uint64_t n_reads64, uint64_t n_iv, uint32_t cov, double not_cov, bool defer)
{
    if (n_reads64 >= 0xFFFFFFFFull) return fail(YACRD_EINVAL, "n_reads must be < 2^32 - 1");
    if (e->pending.active) return fail(YACRD_EINVAL, "a submitted batch is pending: yacrd_engine_wait first");
    e->has_result = false;
    e->resident.valid = e->input.valid = false; // (in_len and the result arrays are about to be rewritten)
    e->timing = yacrd_timing{};
    for (uint64_t &r : e->big_routes) r = 0;

    HIP_TRY(e->bad_offsets.reserve((n_reads64 + 1) * sizeof(u64)));
    if (n_reads64 == 0) {
        HIP_TRY(hipMemsetAsync(e->bad_offsets.p, 0, sizeof(u64), e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        e->last_reads = 0;
        e->last_regions = 0;
        e->has_result = true;
        return YACRD_OK;
    }

    Run R;
    R.d_off = d_off, R.d_iv = d_iv, R.d_len = d_len;
    R.n_reads64 = n_reads64, R.n_reads = (u32)n_reads64, R.n_iv = n_iv, R.cov = cov, R.not_cov = not_cov;
    R.full = (e->flags & YACRD_F_TIMING_FULL) != 0;
    R.tight_grids = !(e->flags & YACRD_F_FORCE_LDS_SORT);
    R.prefilter = (e->flags & YACRD_F_NO_PREFILTER) ? 0u : (e->flags & YACRD_F_COUNT_PREFILTERED) ? 2u : 1u;
    for (int i = 0; i < 12; i++) R.cls_b[i] = R.cls_e[i] = -1;
    // YACRD_F_ONE_LAUNCH: a short batch as one kernel (one_batch.h) — unless a debug flag pins another path
    // — and only where its look-back's progress argument holds (one_batch.h): the slabs at the front of an XCD's
    // contiguous eighth wait for the XCD before it, so up to 7/8 of the slab-finishing wavefronts sit in wave slots for
    // most of the launch; that needs the 8-XCD part and far more resident slots than waiters.  The cap on the reads is
    // the kernel's own (32-bit deferred-interval sum), not the follow-on step's A/B knob.
    const uint64_t ob_waiters = (n_reads64 + yk::kObSlab - 1) / yk::kObSlab * 7 / 8;
    R.one_launch = (e->flags & YACRD_F_ONE_LAUNCH) && !e->one_launch_off && n_reads64 < (uint64_t)yk::kObMaxReads &&
                   e->num_xcc == 8 && 2 * ob_waiters <= (uint64_t)e->num_cu * 4 * YK_OB_OCC &&
                   !(e->flags & (YACRD_F_FORCE_GENERAL | YACRD_F_WAVE_ONLY | YACRD_F_FORCE_LDS_SORT | YACRD_F_NO_HALVES |
                                 YACRD_F_NO_PREFILTER | YACRD_F_NO_DEFER));

    int rc = reserve_buffers(e, R);
    if (rc) return rc;
    if (R.full) HIP_TRY(hipEventRecord(e->ev[EV_START], e->stream));
    if (R.one_launch) {
        rc = launch_one_batch(e, R);
        return rc ? rc : hand_over(e, R, defer);
    }
    R.timing_on = !(e->flags & YACRD_F_NO_TIMING);
    if ((e->flags & YACRD_F_TIMING_SAMPLED) && !R.full && (e->run_seq++ % 8u) != 0) R.timing_on = false;
    R.predicted = prediction_holds(e, R);
    R.direct = choose_direct(e, R);
    struct MissGuard { // (a miss found by THIS call is reported by its conclude_run and forgotten when the call returns)
        yacrd_engine *e;
        bool before;
        ~MissGuard() { e->miss_pending = before; }
    } miss_guard{e, e->miss_pending};
    struct SideGuard { // (no way out between the fork and the join leaves the side stream's kernels writing what the next call may free)
        yacrd_engine *e;
        const Run &R;
        bool joined = false;
        ~SideGuard()
        {
            if ((R.big_beside || R.direct) && !joined) (void)hipStreamSynchronize(e->side);
        }
    } side_guard{e, R};
    e->prev_build = e->last_build;
    e->last_build = -1;
    if (R.direct) {
        // DIRECT: the long launch first, on the engine's stream; beside it, behind the fork, the plan (an unpredicted run:
        // and the host's wait for its counts) and the other register classes; the engine's stream joins them in front of
        // the workgroup classes, the device-wide screen and the follow-on step.  Ordering is by the two events alone.
        HIP_TRY(hipEventRecord(e->ev_sync[EVS_FORK], e->stream));
        if (R.full) HIP_TRY(hipEventRecord(e->ev[EV_S0], e->stream));
        launch_direct_screen(e, R);
        HIP_TRY(hipStreamWaitEvent(e->side, e->ev_sync[EVS_FORK], 0));
        rc = launch_plan(e, R);
        if (!rc) rc = size_launches(e, R);
        if (!rc) rc = launch_register_classes(e, R, R.ls, false);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(e->ev_sync[EVS_JOIN], e->side));
        HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_sync[EVS_JOIN], 0));
        side_guard.joined = true;
        if (R.full && R.timing_on) HIP_TRY(hipEventRecord(e->ev[EV_SMALL], e->stream));
        rc = launch_workgroup_classes(e, R, R.ls, false);
        if (!rc) launch_rejected_medium(e, R, R.ls);
        if (!rc) rc = join_device_wide_screen(e, R); // (nothing was forked for it: its launches go out here)
        if (rc) return rc;
    } else {
        rc = launch_plan(e, R);
        if (!rc) rc = size_launches(e, R);
        if (rc) return rc;
        if (R.full) HIP_TRY(hipEventRecord(e->ev[EV_S0], e->stream));
        rc = launch_device_wide_screen(e, R);
        if (!rc) rc = launch_sweeps(e, R, R.ls);
        if (!rc) rc = join_device_wide_screen(e, R);
        if (rc) return rc;
        side_guard.joined = true;
    }
    if (R.full) HIP_TRY(hipEventRecord(e->ev[EV_GEN], e->stream));
    rc = launch_compact(e, R); // the follow-on step: scan + compact + classify
    if (rc) return rc;
    if (R.full) HIP_TRY(hipEventRecord(e->ev[EV_COMPACT], e->stream));
    if (defer && R.predicted) return hand_over(e, R, defer); // yacrd_engine_submit_device: the caller waits later
    // (spinning on the pinned counter block instead of this call was tried: 0.0816 vs 0.078 ms/step)
    rc = wait_for_stream(e);
    if (rc) return rc;
    R.timing_on = false;
    if (e->h_ctr()->fused_gave_up && !e->fused_off) return rerun_without_fused(e, R);
    float extra_ms = 0.f;
    rc = recover(e, R, extra_ms);
    if (rc) return rc;
    return conclude_run(e, R, extra_ms);
}
} // namespace yke

namespace {

// Folds the run's yacrd_timing (e->timing) into the running totals: millisecond fields and event counters add, count fields
// follow the last run, h2d_ms / d2h_ms are kept (their callers add them: yacrd_engine_run, yacrd_engine_collect).
void fold_timing(yacrd_engine *e)
{
    const yacrd_timing &t = e->timing;
    yacrd_timing &ts = e->timing_sum;
    const yacrd_timing keep = ts;
    ts = t; // count fields follow the last run
    ts.h2d_ms = keep.h2d_ms;
    ts.d2h_ms = keep.d2h_ms;
    ts.plan_ms = keep.plan_ms + t.plan_ms;
    ts.sweep_small_ms = keep.sweep_small_ms + t.sweep_small_ms;
    ts.sweep_medium_ms = keep.sweep_medium_ms + t.sweep_medium_ms;
    ts.sweep_general_ms = keep.sweep_general_ms + t.sweep_general_ms;
    ts.compact_ms = keep.compact_ms + t.compact_ms;
    ts.total_ms = keep.total_ms + t.total_ms;
    for (int i = 0; i < 12; i++) ts.class_ms[i] = keep.class_ms[i] + t.class_ms[i];
    ts.fused_ms = keep.fused_ms + t.fused_ms;
    ts.screened = keep.screened + t.screened;
    ts.one_launch = keep.one_launch + t.one_launch;
    ts.fused_reruns = keep.fused_reruns + t.fused_reruns;
    ts.screen_wide = keep.screen_wide + t.screen_wide;
    ts.predicted = keep.predicted + t.predicted;
    ts.prediction_misses = keep.prediction_misses + t.prediction_misses;
    ts.build_switches = keep.build_switches + t.build_switches;
    ts.sorting_build = keep.sorting_build + t.sorting_build;
    ts.timed_runs = keep.timed_runs + t.timed_runs;
    e->timing_runs++;
}

// Bookkeeping after a run's last sync: result sizes, the next run's prediction, timing.
int conclude_run(yacrd_engine *e, const Run &R, float extra_ms)
{
    const bool full = R.full, predicted = R.predicted, screened = R.screened;
    const yk::Counters c1 = *e->h_ctr();
    const yk::Counters c0 = predicted ? c1 : R.c0; // class counts are final either way
    e->last_reads = R.n_reads;
    e->last_regions = c1.total_regions;
    e->has_result = true;
    e->big_routes[0] = R.big_screened ? (uint64_t)c0.n[yk::CLS_GENERAL] - c1.fb_big : 0; // (the last pass's fallback list)
    e->pred = c1;
    e->pred_reads = R.n_reads64;
    e->pred_iv = R.n_iv;
    e->pred_valid = true;

    yacrd_timing &t = e->timing;
    // An event costs ~3 us of stream time: by default only the dominant kernel is bracketed
    // (class_ms / fused_ms); phases and the whole-pipeline time need YACRD_F_TIMING_FULL.
    t.plan_ms = t.sweep_small_ms = t.sweep_medium_ms = t.sweep_general_ms = t.compact_ms = 0.f;
    t.total_ms = 0.f;
    if (full) {
        // (a direct run: the plan's own bracket on the side stream — it runs beside the long launch, not in front of it)
        t.plan_ms = ev_ms(e->ev[R.direct ? EV_PLAN0 : EV_START], e->ev[EV_PLAN]);
        t.sweep_small_ms = ev_ms(e->ev[EV_S0], e->ev[EV_SMALL]);
        t.sweep_medium_ms = ev_ms(e->ev[EV_SMALL], e->ev[EV_MED]);
        t.sweep_general_ms = ev_ms(e->ev[EV_MED], e->ev[EV_GEN]);
        t.compact_ms = ev_ms(e->ev[EV_GEN], e->ev[EV_COMPACT]);
        t.total_ms = ((predicted || R.direct) ? ev_ms(e->ev[EV_START], e->ev[EV_COMPACT])
                                : t.plan_ms + ev_ms(e->ev[EV_S0], e->ev[EV_COMPACT])) + extra_ms;
    }
    t.n_small = 0;
    t.iv_small = 0;
    for (int cls = yk::CLS_R2; cls <= yk::CLS_W16; cls++) {
        t.n_small += c0.n[cls];
        t.iv_small += c0.iv[cls];
    }
    t.n_medium = (uint64_t)c0.n[yk::CLS_MED1] + c0.n[yk::CLS_MED2];
    t.n_general = (uint64_t)c0.n[yk::CLS_GENERAL] + c1.rej_small + c1.rej_med + c1.rej_big;
    t.iv_medium = c0.iv[yk::CLS_MED1] + c0.iv[yk::CLS_MED2];
    t.iv_general = c0.iv[yk::CLS_GENERAL];
    static_assert(yk::CLS_GENERAL == 11, "yacrd_timing.class_* follows the CLS_ order");
    for (int cls = 0; cls <= yk::CLS_GENERAL; cls++) {
        t.class_reads[cls] = c0.n[cls];
        t.class_intervals[cls] = c0.iv[cls];
        t.class_ms[cls] = 0.f;
        if (cls < yk::CLS_GENERAL && R.cls_b[cls] >= 0 && R.cls_e[cls] >= 0)
            t.class_ms[cls] = ev_ms(e->ev_cls[R.cls_b[cls]], e->ev_cls[R.cls_e[cls]]);
    }
    t.class_ms[yk::CLS_GENERAL] = (full && c0.n[yk::CLS_GENERAL]) ? t.sweep_general_ms : 0.f;
    t.fused_ms = 0.f;
    t.timed_runs = R.fused_marked ? 1u : 0u;
    for (int cls = 0; cls < yk::CLS_GENERAL; cls++)
        if (R.cls_b[cls] >= 0 && R.cls_e[cls] >= 0) t.timed_runs = 1u;
    t.deferred_reads = c1.deferred;
    t.deferred_intervals = c1.deferred_iv;
    // The next batch's build of the fused launch: when this one screened and more than a quarter of what it
    // screened had to be sorted after all, the sorting build takes the next kProbeEvery - 1 batches.
    if (screened) {
        const uint64_t looked_at = (uint64_t)c0.n[yk::CLS_R16] + c0.n[yk::CLS_H16];
        // (a one-look batch that left more than a tenth is followed by the build with the second looks first: only when
        // THAT leaves more than a quarter does the sorting build take over)
        const bool can_widen = !e->last_wide && !(e->flags & YACRD_F_SCREEN_ITEMS_2);
        e->nodefer_left = (!(e->flags & YACRD_F_ALWAYS_DEFER) && !can_widen && 4 * (uint64_t)c1.deferred > looked_at) ? kProbeEvery - 1 : 0;
        if (!e->last_wide) e->wide_left = 10 * (uint64_t)c1.deferred > looked_at ? kProbeEvery - 1 : 0;
        else if (e->wide_left) e->wide_left--;
    } else if (e->nodefer_left) {
        e->nodefer_left--;
    }
    t.screened = screened ? 1u : 0u;
    t.screen_items = screened ? e->last_items : 0u;
    t.screen_wide = (screened && e->last_wide) ? 1u : 0u;
    t.fused_reruns = e->fused_off ? 1u : 0u;
    t.predicted = predicted ? 1u : 0u;
    t.prediction_misses = e->miss_pending ? 1u : 0u;
    t.build_switches = (e->last_build >= 0 && e->prev_build >= 0 && e->last_build != e->prev_build) ? 1u : 0u;
    t.sorting_build = e->last_build == 0 ? 1u : 0u;
    t.fused_reads = t.fused_intervals = 0;
    t.prefiltered_reads = c1.prefiltered;
    if (R.fused_marked) t.fused_ms = ev_ms(e->ev_cls[22], e->ev_cls[23]);
    if (!(e->flags & YACRD_F_FORCE_LDS_SORT)) {
        // what the one launch of the classes R2..H16 holds (whether or not this run timed it)
        for (int cls = yk::CLS_R2; cls <= yk::CLS_H16; cls++) {
            t.fused_reads += c0.n[cls];
            t.fused_intervals += c0.iv[cls];
        }
    }

    fold_timing(e);
    return YACRD_OK;
}

// Second half of yacrd_engine_submit_device: wait, check the prediction the launches were sized
// with, conclude.  Anything the prediction did not cover (a class beyond its grid, reads for the
// device-wide or the exact path, a region overflow) sends the batch through the synchronous,
// unpredicted path once more: rare, and that path has every redo.
int finish_pending(yacrd_engine *e)
{
    Pending &p = e->pending;
    if (!p.active) return YACRD_OK;
    p.active = false;
    const Run R = p.run; // (a copy: a batch that is run again may be handed over again)
    int rc = wait_for_stream(e);
    if (rc) return rc;
    if (p.one_launch) {
        // a read beyond 256 intervals, one the sort rejected (the exact path's) or more regions than bad_regions holds:
        // the default path has every redo — the batch takes it from the start
        const yk::Counters c1 = *e->h_ctr();
        if (c1.ob_unsupported || c1.rej_small || c1.region_overflow || c1.scan_ticket != R.ob_slabs) {
            if (c1.region_overflow) HIP_TRY(e->bad_regions.reserve((size_t)(c1.total_regions + 16) * sizeof(uint2)));
            e->one_launch_off = true;
            rc = run_on_device(e, R.d_off, R.d_iv, R.d_len, R.n_reads64, R.n_iv, R.cov, R.not_cov);
            e->one_launch_off = false;
            return rc;
        }
        e->last_reads = R.n_reads64;
        e->last_regions = c1.total_regions;
        e->has_result = true;
        yacrd_timing &t = e->timing;
        t = yacrd_timing{};
        if (R.full) t.total_ms = ev_ms(e->ev[EV_START], e->ev[EV_COMPACT]);
        t.n_small = R.n_reads64, t.iv_small = R.n_iv;
        t.deferred_reads = c1.deferred, t.deferred_intervals = c1.deferred_iv, t.prefiltered_reads = c1.prefiltered;
        t.screened = 1u, t.screen_items = (uint32_t)yk::kObItems, t.one_launch = 1u;
        fold_timing(e);
        return YACRD_OK;
    }
    const yk::Counters c = *e->h_ctr();
    if (c.fused_gave_up && !e->fused_off) return yke::rerun_without_fused(e, R);
    bool ok = !c.rej_small && c.n[yk::CLS_GENERAL] == R.big_n && c.iv[yk::CLS_GENERAL] == R.big_iv && !c.fb_big && !c.rej_big && !c.region_overflow;
    for (int cls = 0; cls < yk::CLS_GENERAL; cls++) ok = ok && c.n[cls] <= R.ls.n[cls];
    if (!ok) {
        e->pred_valid = false;
        e->miss_pending = true; // (yacrd_timing.prediction_misses: the re-run's conclude_run reports it)
        const int rcm = run_on_device(e, R.d_off, R.d_iv, R.d_len, R.n_reads64, R.n_iv, R.cov, R.not_cov);
        e->miss_pending = false;
        return rcm;
    }
    return conclude_run(e, R, 0.f);
}

} // namespace

namespace yke {
// host -> HBM at PCIe rate.  A pinned source (yacrd_pinned_alloc, hipHostMalloc, hipHostRegister)
// is one direct DMA, asynchronous on the engine's stream.  A pageable source would make the runtime
// stage it through its own pinned buffers from ONE thread (9.6 GB/s measured for configs[1]'s 80 MB):
// here a few threads copy 4 MiB pieces into the engine's pinned bounce buffers and enqueue their
// DMAs, so memcpy and PCIe overlap.  On return the source is no longer needed in either case.
int h2d(yacrd_engine *e, void *dst, const void *src, size_t bytes)
{
    if (!bytes) return YACRD_OK;
    hipPointerAttribute_t at;
    const bool pinned = hipPointerGetAttributes(&at, src) == hipSuccess && at.type == hipMemoryTypeHost;
    if (!pinned) (void)hipGetLastError(); // an unregistered pointer is reported as an error: not one
    if (pinned || bytes < ((size_t)1 << 20)) {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e->stream));
        return YACRD_OK;
    }
    constexpr size_t kPiece = yacrd_engine::kBounceBytes;
    for (size_t b = e->bounce_ev.v.size(); b < (size_t)yacrd_engine::kBounce; b++) { // (buffer b exists iff its event does)
        HIP_TRY(e->bounce[b].reserve(kPiece));
        if (!e->bounce_ev.add(1, hipEventDisableTiming)) {
            e->bounce[b].release();
            HIP_TRY(why_not_added());
        }
    }
    const size_t n_pieces = (bytes + kPiece - 1) / kPiece;
    const int T = (int)std::min<size_t>(yacrd_engine::kBounce / 2, n_pieces);
    std::vector<hipError_t> errs((size_t)T, hipSuccess);
    auto work = [&](int t) {
        if (hipSetDevice(e->device) != hipSuccess) {
            errs[t] = hipErrorInvalidDevice;
            return;
        }
        int turn = 0;
        for (size_t piece = (size_t)t; piece < n_pieces; piece += (size_t)T, turn ^= 1) {
            const int b = 2 * t + turn; // two buffers per thread: one fills while the other flies
            if (e->bounce_busy[b]) {
                const hipError_t w = hipEventSynchronize(e->bounce_ev[b]);
                if (w != hipSuccess) errs[t] = w;
            }
            const size_t at2 = piece * kPiece, n = std::min(kPiece, bytes - at2);
            std::memcpy(e->bounce[b].p, (const char *)src + at2, n);
            hipError_t c = hipMemcpyAsync((char *)dst + at2, e->bounce[b].p, n, hipMemcpyHostToDevice, e->stream);
            if (c == hipSuccess) c = hipEventRecord(e->bounce_ev[b], e->stream);
            if (c != hipSuccess) errs[t] = c;
            e->bounce_busy[b] = true;
        }
    };
    {
        std::vector<std::thread> th;
        for (int t = 1; t < T; t++) th.emplace_back(work, t);
        work(0);
        for (auto &x : th) x.join();
    }
    for (hipError_t er : errs) HIP_TRY(er);
    return YACRD_OK;
}

int classify_on_device(yacrd_engine *e, const u64 *d_bad_offsets, const uint2 *d_bad_regions, const u32 *d_len, u32 n_reads, double not_cov,
                       uint8_t *d_read_type)
{
    if (n_reads)
        hipLaunchKernelGGL(yk::classify_csr_kernel, dim3((n_reads + 255u) / 256u), dim3(256), 0, e->stream, d_bad_offsets, d_bad_regions, d_len,
                           n_reads, not_cov, d_read_type);
    HIP_TRY(hipGetLastError());
    return YACRD_OK;
}

int fetch_result(yacrd_engine *e, yacrd_result *out)
{
    if (!out) return fail(YACRD_EINVAL, "out is null");
    std::memset(out, 0, sizeof(*out));
    if (e->pending.active) return fail(YACRD_EINVAL, "a submitted batch is pending: yacrd_engine_wait first");
    if (!e->has_result) return fail(YACRD_EINVAL, "no result to fetch");
    const uint64_t R = e->last_reads, G = e->last_regions;
    out->bad_offsets = (uint64_t *)std::malloc((size_t)(R + 1) * sizeof(uint64_t));
    out->bad_regions = (uint32_t *)std::malloc((size_t)(2 * G + 2) * sizeof(uint32_t));
    out->read_type = (uint8_t *)std::malloc((size_t)R + 1);
    if (!out->bad_offsets || !out->bad_regions || !out->read_type) {
        yacrd_result_free(out);
        return fail(YACRD_ENOMEM, "host allocation failed");
    }
    // D2H lands in the engine's pinned staging block (direct DMA; into the pageable result arrays
    // the runtime stages at ~10 GB/s) and is copied out from there; results beyond 1 GiB go direct.
    const size_t b_off = (size_t)(R + 1) * sizeof(uint64_t), b_reg = (size_t)G * sizeof(uint2), b_typ = (size_t)R;
    const size_t o_reg = (b_off + 63) & ~(size_t)63, o_typ = (o_reg + b_reg + 63) & ~(size_t)63;
    const size_t need = o_typ + b_typ + 64;
    bool staged = need <= ((size_t)1 << 30);
    if (staged && need > e->h_out.cap && e->h_out.reserve(need + need / 4) != hipSuccess) {
        (void)hipGetLastError();
        staged = false;
    }
    char *h = e->h_out.as<char>();
    void *t_off = staged ? (void *)h : (void *)out->bad_offsets;
    void *t_reg = staged ? (void *)(h + o_reg) : (void *)out->bad_regions;
    void *t_typ = staged ? (void *)(h + o_typ) : (void *)out->read_type;
    HIP_TRY(hipEventRecord(e->ev[EV_D2H0], e->stream));
    HIP_TRY(hipMemcpyAsync(t_off, e->bad_offsets.p, b_off, hipMemcpyDeviceToHost, e->stream));
    if (G) HIP_TRY(hipMemcpyAsync(t_reg, e->bad_regions.p, b_reg, hipMemcpyDeviceToHost, e->stream));
    if (R) HIP_TRY(hipMemcpyAsync(t_typ, e->read_type.p, b_typ, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipEventRecord(e->ev[EV_D2H1], e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (staged) {
        std::memcpy(out->bad_offsets, t_off, b_off);
        if (G) std::memcpy(out->bad_regions, t_reg, b_reg);
        if (R) std::memcpy(out->read_type, t_typ, b_typ);
    }
    e->timing.d2h_ms = ev_ms(e->ev[EV_D2H0], e->ev[EV_D2H1]);
    out->n_reads = R;
    out->n_regions = G;
    return YACRD_OK;
}
} // namespace yke

extern "C" {

int yacrd_abi_version(void) { return YACRD_ABI_VERSION; }

uint64_t yacrd_debug_last_counters(const yacrd_engine *e, void *dst, uint64_t bytes)
{
    if (e && dst && e->h_ctr()) std::memcpy(dst, e->h_ctr(), (size_t)std::min<uint64_t>(bytes, sizeof(yk::Counters)));
    return sizeof(yk::Counters);
}

/* include/yacrd_engine_debug.h: the input CSR of the engine's last call, from in_off / in_iv / in_len (tests) */
int yacrd_debug_last_input_csr(yacrd_engine *e, uint64_t *n_reads, uint64_t *n_intervals, uint64_t *offsets, uint32_t *intervals,
                               uint32_t *lengths)
{
    if (!e || !n_reads || !n_intervals) return fail(YACRD_EINVAL, "null argument");
    if (e->pending.active || e->host_pending) return fail(YACRD_EINVAL, "the engine has a submitted batch pending");
    if (!e->input.valid) return fail(YACRD_EINVAL, "the engine's last call left no input CSR of its own");
    const uint64_t R = e->input.n_reads, I = e->input.n_iv;
    if (offsets && ((I && !intervals) || (R && !lengths))) return fail(YACRD_EINVAL, "null argument");
    // (the record was made from what the build's scan summed: never read past what the call reserved)
    if ((R && ((R + 1) * sizeof(u64) > e->in_off.cap || R * sizeof(u32) > e->in_len.cap)) || (I && I * sizeof(uint2) > e->in_iv.cap))
        return fail(YACRD_EINTERNAL, "the input CSR's record does not fit the engine's input buffers");
    *n_reads = R, *n_intervals = I;
    if (!offsets) return YACRD_OK;
    DeviceGuard guard(e->device);
    offsets[0] = 0; // (a batch without reads stages nothing)
    if (R) HIP_TRY(hipMemcpyAsync(offsets, e->in_off.p, (size_t)(R + 1) * sizeof(u64), hipMemcpyDeviceToHost, e->stream));
    if (I) HIP_TRY(hipMemcpyAsync(intervals, e->in_iv.p, (size_t)I * sizeof(uint2), hipMemcpyDeviceToHost, e->stream));
    if (R) HIP_TRY(hipMemcpyAsync(lengths, e->in_len.p, (size_t)R * sizeof(u32), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return YACRD_OK;
}

/* include/yacrd_engine_debug.h: what DevBuf / PinBuf hold, process-wide (tests) */
uint64_t yacrd_debug_direct_runs(const yacrd_engine *e) { return e ? e->direct_runs : 0; }
uint64_t yacrd_debug_compute_units(const yacrd_engine *e) { return e ? (uint64_t)e->num_cu : 0; }
/* include/yacrd_engine_debug.h: the batch size from which this engine takes the long-batch forms (tests) */
int yacrd_debug_long_min_reads(yacrd_engine *e, uint64_t n)
{
    if (!e) return fail(YACRD_EINVAL, "null argument");
    if (e->pending.active || e->host_pending) return fail(YACRD_EINVAL, "the engine has a submitted batch pending");
    e->long_min_reads = n == UINT64_MAX ? split_min_reads() : n;
    return YACRD_OK;
}
void yacrd_debug_big_routes(const yacrd_engine *e, uint64_t out[4])
{
    for (int i = 0; i < 4; i++) out[i] = e ? e->big_routes[i] : 0;
}

void yacrd_debug_live_bytes(uint64_t out[2])
{
    out[0] = yke::live_bytes()[0].load();
    out[1] = yke::live_bytes()[1].load();
}

const char *yacrd_last_error(void) { return yke::err_slot().c_str(); }

int yacrd_engine_create(const yacrd_engine_cfg *cfg, yacrd_engine **out)
{
    if (!out) return fail(YACRD_EINVAL, "out is null");
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
        return fail(YACRD_ENODEV, "no HIP device visible (libyacrd_hip needs an MI355X / gfx950)");
    int dev = cfg ? cfg->device_id : -1;
    if (dev < 0) HIP_TRY(hipGetDevice(&dev));
    if (dev >= count) return fail(YACRD_EINVAL, "device_id out of range");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(YACRD_ENODEV, std::string("device is ") + prop.gcnArchName +
                                      ", this library is built for gfx950 only");
    DeviceGuard guard(dev);
    yacrd_engine *e = new (std::nothrow) yacrd_engine();
    if (!e) return fail(YACRD_ENOMEM, "host allocation failed");
    e->device = dev;
    e->flags = cfg ? cfg->flags : 0;
    e->long_min_reads = split_min_reads();
    e->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    {
        int xcc = 0;
        if (hipDeviceGetAttribute(&xcc, hipDeviceAttributeNumberOfXccs, dev) != hipSuccess) xcc = 0;
        (void)hipGetLastError();
        e->num_xcc = xcc;
    }
    {
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, yk::screen_wg_fused_kernel, yk::kWsT, 0) == hipSuccess && per_cu > 0)
            e->screen_fused_wgs_per_cu = std::min(per_cu, 4);
        (void)hipGetLastError();
    }
    // (e->side is made by the first batch that needs it: a stream is a hardware queue's worth of scheduling state, and engines
    //  that pipeline short batches — three per device in bench.py — should not double their number for nothing)
    const bool made = e->streams.add(1) && e->ev.add(EV_COUNT) && e->ev_cls.add(24) &&
                      e->ev_sync.add(1, hipEventBlockingSync | hipEventDisableTiming) && e->ev_sync.add(2, hipEventDisableTiming);
    if (!made || e->h_ctr_mem.reserve(sizeof(yk::Counters)) != hipSuccess) {
        yacrd_engine_destroy(e); // (safe on a half-made engine: the owners hold what was made)
        return fail(YACRD_ENODEV, std::string("engine setup: ") + hipGetErrorString(why_not_added()));
    }
    e->stream = e->streams[0];
    *out = e;
    return YACRD_OK;
}

// the text paths' scratch goes back to the device (yke::scratch_of makes it anew on next use); the batch path's buffers, the
// pinned arena and a kGzip slot somebody holds stay
int yacrd_engine_trim(yacrd_engine *e)
{
    if (!e) return fail(YACRD_EINVAL, "engine is null");
    if (e->pending.active || e->host_pending) return fail(YACRD_EINVAL, "the engine has a submitted batch pending");
    DeviceGuard guard(e->device);
    e->mirror.valid = false;
    e->resident.valid = e->input.valid = false;
    for (int k = 0; k < yacrd_engine::kSlots; k++)
        if (!(k == yacrd_engine::kGzip && e->gzip_busy)) e->drop_scratch(k);
    return YACRD_OK;
}

void yacrd_engine_destroy(yacrd_engine *e)
{
    if (!e) return;
    DeviceGuard guard(e->device);
    if (e->stream) (void)hipStreamSynchronize(e->stream);
    if (e->side) (void)hipStreamSynchronize(e->side);
    for (int k = 0; k < yacrd_engine::kSlots; k++) e->drop_scratch(k);
    delete e; // buffers, then events, then streams: the member order of yacrd_engine
}

// what a caller of the device forms gets: the last result where it lies in HBM
static void fill_device_result(const yacrd_engine *e, yacrd_device_result *out)
{
    if (!out) return;
    out->n_reads = e->last_reads;
    out->n_regions = e->last_regions;
    out->d_bad_offsets = e->bad_offsets.p;
    out->d_bad_regions = e->bad_regions.p;
    out->d_read_type = e->read_type.p;
}

int yacrd_engine_run_device(yacrd_engine *e, const void *d_offsets, const void *d_intervals,
                            const void *d_lengths, uint64_t n_reads, uint64_t n_intervals,
                            uint32_t coverage, double not_coverage, yacrd_device_result *out)
{
    if (!e) return fail(YACRD_EINVAL, "engine is null");
    e->resident.valid = e->input.valid = false; // (first: everything below may rewrite or move in_len and the result arrays)
    if (n_reads && (!d_offsets || !d_lengths)) return fail(YACRD_EINVAL, "null device input");
    if (n_intervals && !d_intervals) return fail(YACRD_EINVAL, "null device intervals");
    if (e->host_pending) return fail(YACRD_EINVAL, "a submitted batch is pending: collect it first");
    DeviceGuard guard(e->device);
    int rc = run_on_device(e, (const u64 *)d_offsets, (const uint2 *)d_intervals,
                           (const u32 *)d_lengths, n_reads, n_intervals, coverage, not_coverage);
    if (rc) return rc;
    fill_device_result(e, out);
    return YACRD_OK;
}

int yacrd_engine_submit_device(yacrd_engine *e, const void *d_offsets, const void *d_intervals,
                               const void *d_lengths, uint64_t n_reads, uint64_t n_intervals,
                               uint32_t coverage, double not_coverage)
{
    if (!e) return fail(YACRD_EINVAL, "engine is null");
    e->resident.valid = e->input.valid = false; // (first: everything below may rewrite or move in_len and the result arrays)
    if (n_reads && (!d_offsets || !d_lengths)) return fail(YACRD_EINVAL, "null device input");
    if (n_intervals && !d_intervals) return fail(YACRD_EINVAL, "null device intervals");
    if (e->host_pending) return fail(YACRD_EINVAL, "a submitted batch is pending: collect it first");
    DeviceGuard guard(e->device);
    return run_on_device(e, (const u64 *)d_offsets, (const uint2 *)d_intervals,
                         (const u32 *)d_lengths, n_reads, n_intervals, coverage, not_coverage, true);
}

int yacrd_engine_wait(yacrd_engine *e, yacrd_device_result *out)
{
    if (!e) return fail(YACRD_EINVAL, "engine is null");
    DeviceGuard guard(e->device);
    int rc = finish_pending(e);
    if (rc) return rc;
    if (!e->has_result) return fail(YACRD_EINVAL, "nothing was submitted");
    fill_device_result(e, out);
    return YACRD_OK;
}

int yacrd_engines_run_device_batches(yacrd_engine *const *engines, uint32_t n_engines,
                                     const yacrd_device_batch *batches, uint32_t n_batches,
                                     yacrd_batch_done_fn done, void *user, yacrd_device_result *last)
{
    if (!engines || n_engines == 0 || (!batches && n_batches)) return fail(YACRD_EINVAL, "bad argument");
    for (uint32_t j = 0; j < n_engines; j++)
        if (!engines[j]) return fail(YACRD_EINVAL, "engine is null");
    for (uint32_t j = 0; j < n_engines; j++) engines[j]->resident.valid = engines[j]->input.valid = false;
    std::vector<int64_t> inflight(n_engines, -1); // batch in flight on each engine
    yacrd_device_result res{};
    auto finish = [&](uint32_t j) -> int {
        int rc = yacrd_engine_wait(engines[j], &res);
        if (rc) return rc;
        const uint32_t b = (uint32_t)inflight[j];
        inflight[j] = -1;
        if (done && done(user, b, engines[j], &res)) return fail(YACRD_EINVAL, "the batch callback asked to stop");
        return YACRD_OK;
    };
    int rc = YACRD_OK;
    for (uint32_t i = 0; i < n_batches && rc == YACRD_OK; i++) {
        const uint32_t j = i % n_engines;
        if (inflight[j] >= 0) rc = finish(j);
        if (rc) break;
        const yacrd_device_batch &b = batches[i];
        rc = yacrd_engine_submit_device(engines[j], b.d_offsets, b.d_intervals, b.d_lengths, b.n_reads,
                                        b.n_intervals, b.coverage, b.not_coverage);
        if (rc == YACRD_OK) inflight[j] = i;
    }
    // drain in batch order (also after an error: no engine is left with a pending batch)
    for (uint32_t k = 0; k < n_engines; k++) {
        uint32_t j = 0;
        int64_t lo = -1;
        for (uint32_t q = 0; q < n_engines; q++)
            if (inflight[q] >= 0 && (lo < 0 || inflight[q] < lo)) lo = inflight[q], j = q;
        if (lo < 0) break;
        const int rc2 = finish(j);
        if (rc == YACRD_OK) rc = rc2;
        inflight[j] = -1;
    }
    if (rc == YACRD_OK && last) *last = res;
    return rc;
}

// validate a host CSR and enqueue its way to HBM on the engine's stream (shared by run / submit)
static int stage_host_inputs(yacrd_engine *e, const uint64_t *offsets, const uint32_t *intervals,
                             const uint32_t *lengths, uint64_t n_reads, uint64_t *n_iv_out)
{
    if (n_reads && (!offsets || !lengths)) return fail(YACRD_EINVAL, "null input");
    const uint64_t n_iv = n_reads ? offsets[n_reads] : 0;
    if (n_reads && offsets[0] != 0) return fail(YACRD_EINVAL, "offsets[0] must be 0");
    for (uint64_t r = 0; r < n_reads; r++)
        if (offsets[r + 1] < offsets[r]) return fail(YACRD_EINVAL, "offsets must be non-decreasing");
    if (n_iv && !intervals) return fail(YACRD_EINVAL, "null intervals");
    HIP_TRY(e->in_off.reserve((size_t)(n_reads + 1) * sizeof(uint64_t)));
    HIP_TRY(e->in_iv.reserve((size_t)(n_iv + 1) * sizeof(uint2)));
    HIP_TRY(e->in_len.reserve((size_t)(n_reads + 1) * sizeof(uint32_t)));
    HIP_TRY(hipEventRecord(e->ev[EV_H2D0], e->stream));
    int rc = YACRD_OK;
    if (n_reads) {
        rc = h2d(e, e->in_off.p, offsets, (size_t)(n_reads + 1) * sizeof(uint64_t));
        if (!rc) rc = h2d(e, e->in_len.p, lengths, (size_t)n_reads * sizeof(uint32_t));
    }
    if (!rc && n_iv) rc = h2d(e, e->in_iv.p, intervals, (size_t)n_iv * sizeof(uint2));
    if (rc) return rc;
    HIP_TRY(hipEventRecord(e->ev[EV_H2D1], e->stream));
    *n_iv_out = n_iv;
    return YACRD_OK;
}

// the end of a batch that came from host buffers (run, collect): the h2d time, the result, the d2h time; the input CSR that
// stage_host_inputs left in in_off / in_iv / in_len (e->input.n_reads / n_iv: set by the caller) counts from here on
static int bring_home(yacrd_engine *e, yacrd_result *out)
{
    e->timing.h2d_ms = ev_ms(e->ev[EV_H2D0], e->ev[EV_H2D1]);
    e->timing_sum.h2d_ms += e->timing.h2d_ms;
    const int rc = fetch_result(e, out);
    if (rc) return rc;
    e->timing_sum.d2h_ms += e->timing.d2h_ms;
    e->input.valid = true;
    return YACRD_OK;
}

int yacrd_engine_run(yacrd_engine *e, const uint64_t *offsets, const uint32_t *intervals,
                     const uint32_t *lengths, uint64_t n_reads, uint32_t coverage,
                     double not_coverage, yacrd_result *out)
{
    if (!e) return fail(YACRD_EINVAL, "engine is null");
    e->resident.valid = e->input.valid = false; // (first: everything below may rewrite or move in_len and the result arrays)
    if (!out) return fail(YACRD_EINVAL, "out is null");
    std::memset(out, 0, sizeof(*out));
    if (e->pending.active) return fail(YACRD_EINVAL, "a submitted batch is pending: yacrd_engine_wait first");
    // (a submit that completed synchronously leaves pending.active false: the result buffers still
    // belong to that batch until it is collected)
    if (e->host_pending) return fail(YACRD_EINVAL, "a submitted batch is pending: collect it first");
    DeviceGuard guard(e->device);
    uint64_t n_iv = 0;
    int rc = stage_host_inputs(e, offsets, intervals, lengths, n_reads, &n_iv);
    if (rc) return rc;
    rc = run_on_device(e, e->in_off.as<u64>(), e->in_iv.as<uint2>(), e->in_len.as<u32>(), n_reads,
                       n_iv, coverage, not_coverage);
    if (rc) return rc;
    e->input.n_reads = n_reads, e->input.n_iv = n_iv;
    return bring_home(e, out);
}

int yacrd_engine_submit(yacrd_engine *e, const uint64_t *offsets, const uint32_t *intervals,
                        const uint32_t *lengths, uint64_t n_reads, uint32_t coverage,
                        double not_coverage)
{
    if (!e) return fail(YACRD_EINVAL, "engine is null");
    e->resident.valid = e->input.valid = false; // (first: everything below may rewrite or move in_len and the result arrays)
    if (e->pending.active || e->host_pending)
        return fail(YACRD_EINVAL, "a submitted batch is pending: collect it first");
    DeviceGuard guard(e->device);
    uint64_t n_iv = 0;
    int rc = stage_host_inputs(e, offsets, intervals, lengths, n_reads, &n_iv);
    if (rc) return rc;
    rc = run_on_device(e, e->in_off.as<u64>(), e->in_iv.as<uint2>(), e->in_len.as<u32>(), n_reads,
                       n_iv, coverage, not_coverage, true);
    if (rc) return rc;
    e->input.n_reads = n_reads, e->input.n_iv = n_iv; // (valid once the batch is collected)
    e->host_pending = true;
    return YACRD_OK;
}

int yacrd_engine_collect(yacrd_engine *e, yacrd_result *out)
{
    if (!e) return fail(YACRD_EINVAL, "engine is null");
    if (!out) return fail(YACRD_EINVAL, "out is null");
    std::memset(out, 0, sizeof(*out));
    if (!e->host_pending) return fail(YACRD_EINVAL, "nothing was submitted");
    e->host_pending = false;
    DeviceGuard guard(e->device);
    int rc = finish_pending(e);
    return rc ? rc : bring_home(e, out);
}

void *yacrd_pinned_alloc(size_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1) != hipSuccess) {
        (void)hipGetLastError();
        yke::err_slot() = "hipHostMalloc failed";
        return nullptr;
    }
    return p;
}

void yacrd_pinned_free(void *p)
{
    if (p) (void)hipHostFree(p);
}

int yacrd_engine_fetch(yacrd_engine *e, yacrd_result *out)
{
    if (!e) return fail(YACRD_EINVAL, "engine is null");
    DeviceGuard guard(e->device);
    return fetch_result(e, out);
}

void yacrd_result_free(yacrd_result *r)
{
    if (!r) return;
    std::free(r->bad_offsets);
    std::free(r->bad_regions);
    std::free(r->read_type);
    std::memset(r, 0, sizeof(*r));
}

int yacrd_engine_last_timing(const yacrd_engine *e, yacrd_timing *t)
{
    if (!e || !t) return fail(YACRD_EINVAL, "null argument");
    *t = e->timing;
    return YACRD_OK;
}

int yacrd_engine_timing_total(yacrd_engine *e, yacrd_timing *sum, uint64_t *n_runs, int reset)
{
    if (!e) return fail(YACRD_EINVAL, "null argument");
    if (sum) *sum = e->timing_sum;
    if (n_runs) *n_runs = e->timing_runs;
    if (reset) {
        e->timing_sum = yacrd_timing{};
        e->timing_runs = 0;
        e->run_seq = 0; // YACRD_F_TIMING_SAMPLED: the next run is a timed one
    }
    return YACRD_OK;
}

int yacrd_engine_event_overhead(yacrd_engine *e, float *ms)
{
    if (!e || !ms) return fail(YACRD_EINVAL, "null argument");
    DeviceGuard guard(e->device);
    // an empty bracket: what two event records add to the span they enclose
    constexpr int kPairs = 32;
    double sum = 0;
    for (int i = 0; i < kPairs + 4; i++) {
        HIP_TRY(hipEventRecord(e->ev_cls[22], e->stream));
        HIP_TRY(hipEventRecord(e->ev_cls[23], e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (i >= 4) sum += ev_ms(e->ev_cls[22], e->ev_cls[23]); // the first few warm the path up
    }
    *ms = (float)(sum / kPairs);
    return YACRD_OK;
}

int yacrd_partition_reads(const uint64_t *offsets, uint64_t n_reads, uint32_t n_parts,
                          uint64_t *cuts)
{
    if (!cuts || n_parts == 0 || (n_reads && !offsets)) return fail(YACRD_EINVAL, "bad argument");
    // Balance by work ~ intervals + a per-read constant (a read costs a wavefront even when tiny).
    const uint64_t per_read = 8;
    const uint64_t total = (n_reads ? offsets[n_reads] : 0) + per_read * n_reads;
    cuts[0] = 0;
    uint64_t r = 0;
    for (uint32_t p = 1; p < n_parts; p++) {
        const uint64_t target = total / n_parts * p + (total % n_parts) * p / n_parts;
        uint64_t lo = r, hi = n_reads; // first read index whose prefix work >= target
        while (lo < hi) {
            const uint64_t mid = (lo + hi) / 2;
            if (offsets[mid] + per_read * mid >= target) hi = mid;
            else lo = mid + 1;
        }
        r = lo;
        cuts[p] = r;
    }
    cuts[n_parts] = n_reads;
    return YACRD_OK;
}

int yacrd_engines_run_partitioned(yacrd_engine *const *engines, uint32_t n_engines,
                                  const uint64_t *offsets, const uint32_t *intervals,
                                  const uint32_t *lengths, uint64_t n_reads, uint32_t coverage,
                                  double not_coverage, yacrd_result *out)
{
    if (!engines || n_engines == 0 || !out) return fail(YACRD_EINVAL, "bad argument");
    std::memset(out, 0, sizeof(*out));
    for (uint32_t p = 0; p < n_engines; p++)
        if (!engines[p]) return fail(YACRD_EINVAL, "null engine");
    for (uint32_t p = 0; p < n_engines; p++) engines[p]->resident.valid = engines[p]->input.valid = false;
    std::vector<uint64_t> cuts(n_engines + 1);
    int rc = yacrd_partition_reads(offsets, n_reads, n_engines, cuts.data());
    if (rc) return rc;

    std::vector<yacrd_result> parts(n_engines);
    std::vector<int> codes(n_engines, YACRD_OK);
    std::vector<std::string> errs(n_engines);
    auto work = [&](uint32_t p) {
        const uint64_t r0 = cuts[p], r1 = cuts[p + 1];
        const uint64_t base = n_reads ? offsets[r0] : 0;
        std::vector<uint64_t> loc(r1 - r0 + 1);
        for (uint64_t r = r0; r <= r1; r++) loc[r - r0] = offsets[r] - base;
        codes[p] = yacrd_engine_run(engines[p], loc.data(), intervals ? intervals + 2 * base : nullptr,
                                    lengths ? lengths + r0 : nullptr, r1 - r0, coverage,
                                    not_coverage, &parts[p]);
        if (codes[p]) errs[p] = yke::err_slot(); // thread-local message of this worker
    };
    {
        std::vector<std::thread> th;
        for (uint32_t p = 1; p < n_engines; p++) th.emplace_back(work, p);
        work(0);
        for (auto &t : th) t.join();
    }
    for (uint32_t p = 0; p < n_engines; p++)
        if (codes[p]) {
            const int code = codes[p];
            const std::string msg = "partition " + std::to_string(p) + ": " + errs[p];
            for (auto &r : parts) yacrd_result_free(&r);
            return fail(code, msg);
        }
    uint64_t G = 0;
    for (auto &r : parts) G += r.n_regions;
    out->bad_offsets = (uint64_t *)std::malloc((size_t)(n_reads + 1) * sizeof(uint64_t));
    out->bad_regions = (uint32_t *)std::malloc((size_t)(2 * G + 2) * sizeof(uint32_t));
    out->read_type = (uint8_t *)std::malloc((size_t)n_reads + 1);
    if (!out->bad_offsets || !out->bad_regions || !out->read_type) {
        for (auto &r : parts) yacrd_result_free(&r);
        yacrd_result_free(out);
        return fail(YACRD_ENOMEM, "host allocation failed");
    }
    uint64_t g0 = 0;
    for (uint32_t p = 0; p < n_engines; p++) {
        const uint64_t r0 = cuts[p], nr = cuts[p + 1] - cuts[p];
        for (uint64_t r = 0; r < nr; r++) out->bad_offsets[r0 + r] = g0 + parts[p].bad_offsets[r];
        if (parts[p].n_regions)
            std::memcpy(out->bad_regions + 2 * g0, parts[p].bad_regions,
                        (size_t)parts[p].n_regions * 2 * sizeof(uint32_t));
        if (nr) std::memcpy(out->read_type + r0, parts[p].read_type, (size_t)nr);
        g0 += parts[p].n_regions;
        yacrd_result_free(&parts[p]);
    }
    out->bad_offsets[n_reads] = G;
    out->n_reads = n_reads;
    out->n_regions = G;
    return YACRD_OK;
}

int yacrd_engine_classify(yacrd_engine *e, const uint64_t *bad_offsets, const uint32_t *bad_regions,
                          const uint32_t *lengths, uint64_t n_reads, double not_coverage,
                          uint8_t *read_type)
{
    if (!e) return fail(YACRD_EINVAL, "engine is null");
    e->resident.valid = e->input.valid = false;
    if (n_reads == 0) return YACRD_OK;
    if (!bad_offsets || !lengths || !read_type) return fail(YACRD_EINVAL, "null argument");
    if (n_reads >= 0xFFFFFFFFull) return fail(YACRD_EINVAL, "n_reads must be < 2^32 - 1");
    const uint64_t G = bad_offsets[n_reads];
    if (G && !bad_regions) return fail(YACRD_EINVAL, "null regions");
    DeviceGuard guard(e->device);
    DevBuf d_off, d_reg, d_len, d_type; // (this call's own: freed on every way out)
    HIP_TRY(d_off.reserve((size_t)(n_reads + 1) * sizeof(u64)));
    HIP_TRY(d_reg.reserve((size_t)(G + 1) * sizeof(uint2)));
    HIP_TRY(d_len.reserve((size_t)n_reads * sizeof(u32)));
    HIP_TRY(d_type.reserve((size_t)n_reads));
    HIP_TRY(hipMemcpyAsync(d_off.p, bad_offsets, (size_t)(n_reads + 1) * sizeof(u64),
                           hipMemcpyHostToDevice, e->stream));
    if (G)
        HIP_TRY(hipMemcpyAsync(d_reg.p, bad_regions, (size_t)G * sizeof(uint2),
                               hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(d_len.p, lengths, (size_t)n_reads * sizeof(u32),
                           hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(yk::classify_csr_kernel, dim3((u32)((n_reads + 255) / 256)), dim3(256), 0,
                       e->stream, d_off.as<u64>(), d_reg.as<uint2>(), d_len.as<u32>(),
                       (u32)n_reads, not_coverage, d_type.as<uint8_t>());
    HIP_TRY(hipMemcpyAsync(read_type, d_type.p, (size_t)n_reads, hipMemcpyDeviceToHost,
                           e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipGetLastError());
    return YACRD_OK;
}

} // extern "C"
