// gpu_out.h — the HIP side of host/way_out.h: what the editors (gpu_edit.hip, gpu_seq_edit.hip) plug into the way out of HBM.
// The order of the batches, the release rule and why two buffers and two pairs of words are enough: way_out.h.
#pragma once
#include "gpu_text.h"
#include "bgzf_sizes.h"
#include "host/way_out.h"

namespace yke {

constexpr size_t kOutPiece = (size_t)4 << 20; // what one copy home moves (_PIECE of the tests)

struct OutDevice {
    static constexpr u64 kBlock = ydf::kBlock, kSlot = ydf::kSlot, kEofBytes = ydf::kEofBytes;
    yacrd_engine *e = nullptr;
    const std::atomic<int> *stop = nullptr;      // a word another thread sets to end the run (HomeLink::stop), where there is one
    std::atomic<size_t> *slots_below = nullptr;  // where given: the caller's output slots below this number are let go (released)
    Streams side;      // [0] the way home; [1] the encoder (gzip out)
    Events landed;     // a pinned piece has landed (two; no timing)
    Events gev, gdone; // per batch, added as it is encoded: the pair around its kernels (timing); behind its sizes' way home (no timing)
    GzDevice gz;
    GzHold gz_hold;
    // what the encoder's call that failed said: its code and message (a HIP call's: as HIP_TRY words them)
    int code = YACRD_OK;
    std::string msg;
    bool no_event = false; // ... it was the creation of a batch's events

    // the streams and the pieces' events; false: one could not be created
    bool make(bool gzip) { return side.add(gzip ? 2 : 1) && landed.add(2, hipEventDisableTiming); }
    // gzip out: the engine's encoder buffers, for batches of at most max_blocks blocks, are this run's until it ends.
    // `wait`: for the engine's stream (gzip_device_open's memset precedes the first batch, which runs on another stream)
    int open(yacrd_engine *engine, u64 max_blocks, bool wait)
    {
        e = engine;
        if (const int rc = gzip_device_open(e, max_blocks, &gz)) return rc;
        gz_hold.e = e;
        if (wait) HIP_TRY(hipStreamSynchronize(e->stream));
        return YACRD_OK;
    }

    HomeLink link(const char *base) const { return HomeLink{base, side[0], {landed[0], landed[1]}, stop}; }
    bool hip(hipError_t r, const char *call)
    {
        if (r == hipSuccess) return true;
        code = r == hipErrorOutOfMemory ? YACRD_ENOMEM : YACRD_ENODEV, msg = std::string(call) + ": " + hipGetErrorString(r);
        return false;
    }
    bool encode(size_t b, const unsigned char *text, u64 len, bool last, int which, volatile u64 *words)
    {
        if (!gev.add(2) || !gdone.add(1, hipEventDisableTiming)) return no_event = true, hip(why_not_added(), "hipEventCreateWithFlags");
        // (a batch beyond max_blocks blocks is refused in there)
        if ((code = gzip_device_encode(e, gz, side[1], text, len, last, which, gev[2 * b], gev[2 * b + 1], words, words + 1)) != YACRD_OK)
            return msg = err_slot(), false;
        return hip(hipEventRecord(gdone[b], side[1]), "hipEventRecord(gdone[b], side[1])");
    }
    bool wait_done(size_t b) { return hip(hipEventSynchronize(gdone[b]), "hipEventSynchronize(gdone[b])"); }
    const unsigned char *out(int which) const { return gz.out[which]; }
    void released(long tag)
    {
        if (slots_below) slots_below->store((size_t)tag + 1, std::memory_order_release);
    }
    bool stopped() const { return stop && stop->load(); }
    void quiet()
    {
        for (hipStream_t s : side.v) (void)hipStreamSynchronize(s);
    }
    // the encoder's kernels, summed over the batches
    float kernel_ms() const
    {
        float ms = 0.f;
        for (size_t i = 0; i + 1 < gev.v.size(); i += 2) ms += ev_ms(gev[i], gev[i + 1]);
        return ms;
    }
};

struct Out : yout::WayOut<OutDevice> {
    Out(OutDevice &d, yseg::Sink &sink) : yout::WayOut<OutDevice>{d, sink, nullptr, kOutPiece} {}
    // behind OutDevice::open: the two pinned pieces (the run's scratch holds them) and, gzip out, four pinned words
    void bind(char *pieces, volatile u64 *four_words) { halves = pieces, words = four_words, max_blocks = dev.gz.max_blocks; }
};

} // namespace yke
