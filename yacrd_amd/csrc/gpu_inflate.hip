// gpu_inflate.hip — BGZF inflated on the GPU: a stream in HBM -> its text in HBM (include/yacrd_engine.h:
// yacrd_engine_gunzip_mem; gpu_seq_edit.hip: the editors' _bgzf_ forms; gpu_paf.hip / gpu_report.hip: the _bgzf_mem ingests,
// through move_bgzf_text below, which decodes the members of every landed segment while the rest of the stream is on its way).
//
//   walk     on the host (bgzf_walk.h, no zlib): every member's payload, sizes and place in the text; what is not BGZF is
//            the host reader's (YACRD_EFALLBACK)
//   decode   one 64-thread workgroup — one wavefront — per member: inflate_block.h.  Only the code tables lie in LDS (4.7 KiB)
//            and the kernel takes 50 VGPRs: 32 wavefronts per CU.  The member's text is written where it belongs in HBM, one
//            byte per store — members begin at any byte, and no dword that holds bytes of two members is ever written as
//            one — and a match reads back what this wavefront has stored: one wavefront's accesses to an address are served
//            in order, nobody else reads the bytes before the kernel ends.  (The whole member in LDS, 70 KiB and two
//            wavefronts per CU, was built first and took five times as long: DESIGN §7h.)  The payload is read 256 bytes
//            at a time into the wavefront's registers.
// A member that is not taken (inflate_block.h: InfStatus) leaves its status in one word (the largest wins); its part of the
// text then holds whatever was decoded until then, and the caller does not use the text.
#include "engine_internal.h"
#include "gpu_text.h"
#include "bgzf_plan.h"
#include "bgzf_walk.h"
#include "inflate_block.h"
#include "host/segment_pump.h"

#include <cstdio>
#include <cstdlib>

using namespace yke;

namespace yk {

// members [m0, m1) of the table, one workgroup each
__global__ __launch_bounds__(64) void inf_kernel(const unsigned char *comp, u64 comp_bytes, const yif::InfMember *members, u32 m0, u32 m1,
                                                  unsigned char *text, u64 text_bytes, u32 *status)
{
    __shared__ yif::InfShared sh;
    const u32 m = m0 + blockIdx.x; // (m1 < 2^31: inflate_device_open)
    if (m >= m1) return; // (uniform)
    const yif::InfMember mm = members[m];
    const u32 lane = threadIdx.x;
    const u32 csize = YI_UNI(mm.csize), n = YI_UNI(mm.isize);
    u32 st = yif::kInfTable; // the table is the host's, from these bytes; what it says is checked against the buffers all the same
    if (n <= yif::kMaxOut && mm.in_off <= comp_bytes && comp_bytes - mm.in_off >= (u64)csize + 8u && mm.out_off <= text_bytes &&
        text_bytes - mm.out_off >= n) {
        const unsigned char *p = comp + mm.in_off;
        const u32 crc = (u32)p[csize] | ((u32)p[csize + 1] << 8) | ((u32)p[csize + 2] << 16) | ((u32)p[csize + 3] << 24);
        st = yif::inf_decode_member(sh, p, csize, n, YI_UNI(crc), text + mm.out_off);
    }
    if (st != yif::kInfOk && lane == 0) atomicMax(status, st);
}

// The same for one WINDOW of a text: `members` is the window's slice of the table, n_members of them, with the
// offsets the walk gave — absolute in the stream and in the text; `comp` holds the stream's bytes [c0, c0 + comp_bytes) and
// `text` takes the text's bytes [t0, t0 + text_bytes).  Every member is checked against the WINDOW's extents before a byte
// is read or stored: one that does not lie inside both leaves kInfTable, never an access out of range.
__global__ __launch_bounds__(64) void inf_window_kernel(const unsigned char *comp, u64 c0, u64 comp_bytes, const yif::InfMember *members, u32 n_members,
                                                         unsigned char *text, u64 t0, u64 text_bytes, u32 *status)
{
    __shared__ yif::InfShared sh;
    const u32 m = blockIdx.x;
    if (m >= n_members) return; // (uniform)
    const yif::InfMember mm = members[m];
    const u32 lane = threadIdx.x;
    const u32 csize = YI_UNI(mm.csize), n = YI_UNI(mm.isize);
    u32 st = yif::kInfTable;
    if (n <= yif::kMaxOut && mm.in_off >= c0 && mm.out_off >= t0) {
        const u64 in = mm.in_off - c0, out = mm.out_off - t0; // (in the slots)
        if (in <= comp_bytes && comp_bytes - in >= (u64)csize + 8u && out <= text_bytes && text_bytes - out >= n) {
            const unsigned char *p = comp + in;
            const u32 crc = (u32)p[csize] | ((u32)p[csize + 1] << 8) | ((u32)p[csize + 2] << 16) | ((u32)p[csize + 3] << 24);
            st = yif::inf_decode_member(sh, p, csize, n, YI_UNI(crc), text + out);
        }
    }
    if (st != yif::kInfOk && lane == 0) atomicMax(status, st);
}

} // namespace yk

namespace {

constexpr size_t kHomePiece = (size_t)4 << 20; // what one copy home moves

struct InflateScratch { // stays with the engine (grow-only); goes with yacrd_engine_trim / destroy
    static constexpr yacrd_engine::Slot kScratchSlot = yacrd_engine::kInflate;
    DevBuf comp, members, status;
    DevBuf text; // yacrd_engine_gunzip_mem's (the editors inflate into their own text buffer)
    DevBuf wcomp, wmembers; // a text in windows (inflate_window_open): the one compressed slot, the window's slice of the table
    PinBuf pin;  // two pieces on their way home, the status word
};

} // namespace

namespace yke {

int inflate_device_open(yacrd_engine *e, u64 comp_bytes, const yif::InfMember *members, u64 n_members, InflateDevice *d)
{
    if (n_members >= 0x7FFFFFFFull) return fail(YACRD_EFALLBACK, "more BGZF members than the device decoder numbers");
    InflateScratch *S = scratch_of<InflateScratch>(e);
    if (!S) return fail(YACRD_ENOMEM, "host allocation failed");
    const void *before = S->comp.p;
    HIP_TRY(S->comp.reserve((size_t)comp_bytes + 64));
    HIP_TRY(S->members.reserve((size_t)(n_members + 1) * sizeof(yif::InfMember)));
    HIP_TRY(S->status.reserve(64));
    HIP_TRY(hipMemsetAsync(S->status.p, 0, 64, e->stream));
    HIP_TRY(hipMemsetAsync(S->comp.as<char>() + comp_bytes, 0, 64, e->stream));
    if (n_members)
        if (const int rc = h2d(e, S->members.p, members, (size_t)n_members * sizeof(yif::InfMember))) return rc;
    d->comp = S->comp.as<unsigned char>(), d->members = S->members.as<yif::InfMember>(), d->status = S->status.as<u32>();
    d->comp_bytes = comp_bytes, d->n_members = n_members, d->fresh = S->comp.p != before;
    return YACRD_OK;
}

int inflate_device_run_range(yacrd_engine *e, const InflateDevice &d, hipStream_t st, unsigned char *d_text, u64 text_bytes, u64 m0, u64 m1)
{
    (void)e;
    if (m0 > m1 || m1 > d.n_members) return fail(YACRD_EINTERNAL, "device inflate: a member range outside the table");
    if (m1 > m0)
        hipLaunchKernelGGL(yk::inf_kernel, dim3((u32)(m1 - m0)), dim3(64), 0, st, d.comp, d.comp_bytes, d.members, (u32)m0, (u32)m1, d_text,
                           text_bytes, d.status);
    HIP_TRY(hipGetLastError());
    return YACRD_OK;
}

int inflate_device_run(yacrd_engine *e, const InflateDevice &d, hipStream_t st, unsigned char *d_text, u64 text_bytes)
{
    return inflate_device_run_range(e, d, st, d_text, text_bytes, 0, d.n_members);
}

u64 inflate_device_held(yacrd_engine *e)
{
    const auto &s = e->scratch[InflateScratch::kScratchSlot];
    const InflateScratch *S = static_cast<const InflateScratch *>(s.p);
    return S ? (u64)S->comp.cap + (u64)S->members.cap : 0;
}

void inflate_device_release_whole(yacrd_engine *e)
{
    if (InflateScratch *S = static_cast<InflateScratch *>(e->scratch[InflateScratch::kScratchSlot].p)) S->comp.release(), S->members.release();
}

int inflate_window_open(yacrd_engine *e, u64 W, InflateWindow *w)
{
    InflateScratch *S = scratch_of<InflateScratch>(e);
    if (!S) return fail(YACRD_ENOMEM, "host allocation failed");
    const void *before = S->wcomp.p;
    HIP_TRY(S->wcomp.reserve((size_t)W + 64));
    HIP_TRY(S->wmembers.reserve(64 * sizeof(yif::InfMember)));
    HIP_TRY(S->status.reserve(64));
    HIP_TRY(hipMemsetAsync(S->status.p, 0, 64, e->stream));
    w->comp = S->wcomp.as<unsigned char>(), w->status = S->status.as<u32>(), w->W = W, w->fresh = S->wcomp.p != before;
    return YACRD_OK;
}

int inflate_device_run_window(yacrd_engine *e, const InflateWindow &w, hipStream_t st, const yif::InfMember *slice, u64 n_slice, u64 c0, u64 c1,
                              u64 t0, u64 t1, unsigned char *d_text)
{
    InflateScratch *S = scratch_of<InflateScratch>(e);
    if (!S || S->wcomp.as<unsigned char>() != w.comp) return fail(YACRD_EINTERNAL, "device inflate: the window's slot is not open");
    if (c1 < c0 || c1 - c0 > w.W || t1 < t0 || t1 - t0 > w.W || n_slice >= 0x7FFFFFFFull)
        return fail(YACRD_EINTERNAL, "device inflate: a window larger than its slots");
    HIP_TRY(S->wmembers.reserve((size_t)(n_slice + 1) * sizeof(yif::InfMember))); // (grow-only; its last reader, the inflate of the window before, has ended: the header's contract)
    HIP_TRY(hipMemsetAsync(w.comp + (c1 - c0), 0, 64, st));
    if (!n_slice) return YACRD_OK;
    if (st == e->stream) {
        if (const int rc = h2d(e, S->wmembers.p, slice, (size_t)n_slice * sizeof(yif::InfMember))) return rc;
    } else
        HIP_TRY(hipMemcpyAsync(S->wmembers.p, slice, (size_t)n_slice * sizeof(yif::InfMember), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(yk::inf_window_kernel, dim3((u32)n_slice), dim3(64), 0, st, w.comp, c0, c1 - c0, S->wmembers.as<yif::InfMember>(), (u32)n_slice,
                       d_text, t0, t1 - t0, w.status);
    HIP_TRY(hipGetLastError());
    return YACRD_OK;
}

u64 inflate_window_held(yacrd_engine *e)
{
    const auto &s = e->scratch[InflateScratch::kScratchSlot];
    const InflateScratch *S = static_cast<const InflateScratch *>(s.p);
    return S ? (u64)S->wcomp.cap + (u64)S->wmembers.cap : 0;
}

float BgzfMove::kernel_ms() const
{
    float k = 0;
    for (size_t i = 0; i + 1 < n_ev; i += 2) k += ev_ms(ev[i], ev[i + 1]);
    return k;
}

int move_bgzf_text(yacrd_engine *e, const char *comp_src, u64 comp_bytes, const std::vector<yif::InfMember> &members, unsigned char *d_text,
                   u64 text_bytes, int n_threads, const std::function<void(u64, u64, u64)> &on_text_segment, BgzfMove &bm, int *rc_out)
{
    static_assert(ybw::kPlanChunk == kTextChunk && ybw::kPlanSeg == kTextSeg, "the planner's segments are move_text's");
    *rc_out = YACRD_OK;
    if ((*rc_out = inflate_device_open(e, comp_bytes, members.data(), members.size(), &bm.d))) return 1;
    // one pair of timed events around every launch: a launch per landed segment of the stream, and one to end with
    const size_t n_pairs = (size_t)((comp_bytes + kTextChunk * kTextSeg - 1) / (kTextChunk * kTextSeg)) + 2;
    if (!bm.ev.add(2 * n_pairs)) {
        *rc_out = fail(YACRD_ENODEV, "device inflate: no events");
        return 1;
    }
    // (measurements only: the whole stream up first, then one launch — what the segment-wise launches are compared with)
    const char *whole_env = std::getenv("YACRD_BGZF_ONE_LAUNCH");
    const bool whole = whole_env && whole_env[0] == '1';
    ybw::SegmentPlan plan(members.data(), members.size(), text_bytes);
    int bad = 0; // a HIP call of a launch failed
    auto landed = [&](u64 have) {
        ybw::PlanStep s;
        while (!bad && plan.next(have, s)) {
            if (s.m1 > s.m0) {
                if (bm.n_ev + 2 > bm.ev.v.size() || hipEventRecord(bm.ev[bm.n_ev], e->stream) != hipSuccess ||
                    inflate_device_run_range(e, bm.d, e->stream, d_text, text_bytes, s.m0, s.m1) != YACRD_OK ||
                    hipEventRecord(bm.ev[bm.n_ev + 1], e->stream) != hipSuccess) {
                    bad = 1;
                    break;
                }
                bm.n_ev += 2, bm.n_launches++;
            }
            if (s.t1 > s.t0) on_text_segment(s.t0, s.t1, s.avail);
        }
    };
    const double t0 = now_ms();
    TextSource src;
    src.mem = comp_src;
    const int moved = move_text(e, src, 0, comp_bytes, reinterpret_cast<char *>(bm.d.comp), bm.d.fresh, n_threads, [&](u64, u64, u64 avail) {
        if (!whole || avail == comp_bytes) landed(avail);
    });
    bm.h2d_ms = (float)(now_ms() - t0);
    if (moved) return moved;
    landed(comp_bytes); // (a stream of no bytes has no segment; otherwise nothing is left to do)
    if (bad || !plan.done()) {
        (void)hipStreamSynchronize(e->stream);
        (void)hipGetLastError();
        return 1;
    }
    return 0;
}

int inflate_not_taken(u32 status)
{
    return fail(YACRD_EFALLBACK, std::string("a BGZF member the device decoder does not take (") + yif::inf_status_name(status) + "): the host reader's");
}

} // namespace yke

extern "C" {

int yacrd_engine_gunzip_mem(yacrd_engine *e, const char *bgzf, uint64_t n_bytes, char **out, uint64_t *out_bytes, yacrd_gunzip_stats *stats)
{
    if (!e || (!bgzf && n_bytes) || !out || !out_bytes) return fail(YACRD_EINVAL, "null argument");
    *out = nullptr, *out_bytes = 0;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    if (e->pending.active || e->host_pending) return fail(YACRD_EINVAL, "the engine has a submitted batch pending");
    DeviceGuard guard(e->device);
    yacrd_gunzip_stats s = {};
    const double t0 = now_ms();
    std::vector<yif::InfMember> members;
    u64 total = 0;
    if (!ybw::walk(reinterpret_cast<const unsigned char *>(bgzf), n_bytes, members, &total)) return fail(YACRD_EFALLBACK, "not BGZF: the host reader's");
    s.walk_ms = (float)(now_ms() - t0);
    s.in_bytes = n_bytes, s.out_bytes = total, s.n_members = members.size();
    char *res = (char *)std::malloc((size_t)total + 1);
    if (!res) return fail(YACRD_ENOMEM, "host allocation failed");
    Events ev, wev; // around the kernel (timed); a piece has landed at home (two)
    auto run = [&]() -> int {
        if (members.empty()) return YACRD_OK;
        InflateDevice d;
        if (const int rc = inflate_device_open(e, n_bytes, members.data(), members.size(), &d)) return rc;
        InflateScratch &S = *scratch_of<InflateScratch>(e); // (open made it)
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (double)total * 1.125 + (double)((size_t)64 << 20) > (double)free_b + (double)S.text.cap)
            return fail(YACRD_EFALLBACK, "the text does not fit this device's free memory: the host reader streams it");
        HIP_TRY(S.text.reserve((size_t)total + 64));
        HIP_TRY(S.pin.reserve(2 * kHomePiece + 64));
        volatile u32 *h_status = reinterpret_cast<volatile u32 *>(S.pin.as<char>() + 2 * kHomePiece);
        *h_status = 0;
        if (!ev.add(2) || !wev.add(2, hipEventDisableTiming)) HIP_TRY(why_not_added());
        const double t1 = now_ms();
        TextSource src;
        src.mem = bgzf;
        const int moved = move_text(e, src, 0, n_bytes, reinterpret_cast<char *>(d.comp), d.fresh, 0, [](u64, u64, u64) {});
        if (moved == 3) return fail(YACRD_ENOMEM, "BGZF stream to HBM: no pinned memory");
        if (moved) return fail(YACRD_ENODEV, "device inflate: a HIP call failed");
        s.h2d_ms = (float)(now_ms() - t1);
        HIP_TRY(hipEventRecord(ev[0], e->stream));
        if (const int rc = inflate_device_run(e, d, e->stream, S.text.as<unsigned char>(), total)) return rc;
        HIP_TRY(hipEventRecord(ev[1], e->stream));
        HIP_TRY(hipMemcpyAsync((void *)h_status, d.status, sizeof(u32), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(hipGetLastError());
        s.kernel_ms = ev_ms(ev[0], ev[1]);
        if (*h_status) return inflate_not_taken(*h_status);
        const double t2 = now_ms();
        HomeLink dma{S.text.as<char>(), e->stream, {wev[0], wev[1]}};
        yseg::Sink sink;
        sink.mem = res; // (sized here: total bytes)
        const int rc = yseg::pump(total, kHomePiece, S.pin.as<char>(), dma, sink, [](auto put) { put(); });
        if (rc != yseg::kPumped || sink.at != total) return fail(YACRD_ENODEV, "device inflate: a HIP call failed on the way home");
        s.d2h_ms = (float)(now_ms() - t2);
        return YACRD_OK;
    };
    const int rc = run();
    (void)hipStreamSynchronize(e->stream); // (whatever failed: nothing of this call is in flight when its events go)
    (void)hipGetLastError();
    if (rc != YACRD_OK) {
        std::free(res);
        return rc;
    }
    *out = res, *out_bytes = total;
    if (stats) *stats = s;
    return YACRD_OK;
}

} // extern "C"
