// way_out.h — the way out of HBM that every editor's run ends in, whole text or windows (gpu_edit.hip, gpu_seq_edit.hip): a
// stretch of output that lies in device memory goes home through the two pinned pieces (segment_pump.h) into the sink or,
// gzip out, through the device encoder first — in batches of at most max_blocks blocks on a stream of the encoder's own, one
// batch coming home while the next is encoded.  Plain C++, no device call: gpu_out.h plugs HIP into `Dev`,
// tools/way_out_check.cc a memcpy (the stand-alone program that runs this order under -fsanitize=address,undefined).
//
// THE RULE, stated here once.  Batch b uses the encoder's output buffer b & 1 and the pair of pinned size words b & 1.  A
// batch may be encoded only when every batch but the one before it has been fetched: sent - got <= 1 in front of encode, so
// fetch(b - 2) — the last reader of buffer and words b & 1: it waited for that batch's "done" event, read the words behind
// the wait and brought the buffer's bytes home before it returned — precedes encode(b).  That is why two buffers and two
// pairs of words serve any number of batches.  The EOF member follows the last batch and no other.  An output slot of the
// caller's (`tag`) is released by the fetch of the batch that carries its tag, behind the wait for that batch: the encoder has
// read the slot.  Plain output has no batch: a slot is released when its home() has returned.
//
//   Dev::kBlock, kSlot, kEofBytes   text bytes per block; the most a block's member takes; the EOF member's bytes
//   Dev::link(base)                 the yseg::pump link that copies from base (HomeLink)
//   Dev::encode(b, text, len, last, which, words)   begin batch b: text[0, len) -> members in buffer `which`, the EOF member
//                                   behind them when `last`; behind them on the encoder's stream the members' bytes land in
//                                   words[0], the stored members so far in words[1], and the batch's "done" event; false: failed
//   Dev::wait_done(b)               batch b's "done" event has passed; false: failed
//   Dev::out(which)                 the encoder's buffer
//   Dev::released(tag)              the caller's slot `tag` is read by nothing of the way out any more
//   Dev::stopped()                  another thread has ended the run
//   Dev::quiet()                    nothing of the way out is in flight any more
#pragma once

#include "segment_pump.h"

#include <chrono>

namespace yout {

enum Result { kWent = 0, kDeviceFailed, kSinkFailed, kBoundBroken, kStopped };
constexpr long kNoTag = -1;

template <class Dev>
struct WayOut {
    Dev &dev;
    yseg::Sink &sink;
    char *halves;   // the two pinned pieces, end to end
    uint64_t piece; // bytes of one
    volatile uint64_t *words = nullptr; // gzip out: two pairs of pinned words
    uint64_t max_blocks = 0;            // gzip out: blocks a batch may hold
    // what went wrong first; every call after it returns it and starts nothing
    Result verdict = kWent;
    bool on_way_home = false;  // ... in a copy home (kDeviceFailed)
    bool out_of_order = false; // ... a batch was to be encoded with two still out (kBoundBroken; else: more bytes than the slots hold)
    uint64_t members = 0, stored = 0, text_bytes = 0; // members encoded (no EOF member), stored ones, text bytes encoded
    size_t sent = 0, got = 0;                         // batches encoded / fetched
    double put_ms = 0;                                // the sink's part of the way home
    long tag_of[2] = {kNoTag, kNoTag};
    uint64_t eof_of[2] = {0, 0};

    bool ready()
    {
        if (verdict == kWent && dev.stopped()) verdict = kStopped;
        return verdict == kWent;
    }
    uint64_t per() const { return max_blocks * Dev::kBlock; }

    // base[0, len) -> the sink through the two pieces: one flies while the other is written
    Result home(const char *base, uint64_t len)
    {
        if (!ready()) return verdict;
        auto link = dev.link(base);
        const int rc = yseg::pump(len, piece, halves, link, sink, [&](auto put) {
            const auto t0 = std::chrono::steady_clock::now();
            put();
            put_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        });
        if (rc == yseg::kLinkFailed) verdict = dev.stopped() ? kStopped : kDeviceFailed, on_way_home = true;
        if (rc == yseg::kSinkFailed) verdict = kSinkFailed;
        return verdict;
    }

    // one batch, at most per() bytes, into buffer sent & 1; `tag`: the caller's slot this batch is the last to read
    Result encode(const unsigned char *text, uint64_t len, bool last, long tag)
    {
        if (!ready()) return verdict;
        if (sent - got > 1) return out_of_order = true, verdict = kBoundBroken; // (the rule; a batch of more than per() bytes is the device's to refuse)
        const int w = (int)(sent & 1);
        words[2 * w] = words[2 * w + 1] = 0;
        if (!dev.encode(sent, text, len, last, w, words + 2 * w)) return verdict = kDeviceFailed;
        tag_of[w] = tag, eof_of[w] = last ? Dev::kEofBytes : 0u;
        members += (len + Dev::kBlock - 1) / Dev::kBlock;
        text_bytes += len, sent++;
        return kWent;
    }

    // the oldest batch not yet fetched -> the sink
    Result fetch()
    {
        if (!ready() || got == sent) return verdict;
        const int w = (int)(got & 1);
        if (!dev.wait_done(got)) return verdict = kDeviceFailed; // (the event, not the stream: the next batch is being encoded on it)
        const uint64_t bytes = words[2 * w] + eof_of[w];
        if (bytes > max_blocks * Dev::kSlot + Dev::kEofBytes) return verdict = kBoundBroken;
        stored = words[2 * w + 1];
        if (tag_of[w] != kNoTag) dev.released(tag_of[w]);
        got++;
        return home(reinterpret_cast<const char *>(dev.out(w)), bytes);
    }
    Result fetch_but(size_t keep)
    {
        while (verdict == kWent && got + keep < sent) fetch();
        return verdict;
    }

    // a stretch of any length, split at per(): each part is encoded with the batch before it fetched behind it, the last part
    // carries `tag`; a `last` stretch of no bytes makes the batch that is the EOF member alone.  A stretch that makes no batch
    // fetches what is still out, and its slot is released at once: nothing of it is the encoder's to read.  (The overlap
    // editor's runs size max_blocks so that a stretch of theirs is one batch; before there was one way out they refused a longer
    // one as an internal error, here it is cut like any other.)
    Result text(const unsigned char *base, uint64_t len, bool last, long tag)
    {
        const uint64_t nb = (len + per() - 1) / per() + (last && !len ? 1u : 0u);
        for (uint64_t b = 0; b < nb && verdict == kWent; b++) {
            const uint64_t from = b * per(), part = len - from < per() ? len - from : per();
            if (encode(base + from, part, last && b + 1 == nb, b + 1 == nb ? tag : kNoTag) == kWent) fetch_but(1);
        }
        if (!nb && fetch_but(0) == kWent && tag != kNoTag) dev.released(tag);
        return verdict;
    }

    // everything that is still out comes home; whatever happened, nothing is in flight behind it
    Result drain()
    {
        fetch_but(0);
        dev.quiet();
        return verdict;
    }
};

} // namespace yout
