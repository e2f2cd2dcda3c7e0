// way_out_check.cc — host/way_out.h (the order in which the editors' output leaves the device: the copies home, the encoder's
// batches, the release of the caller's output slots) on its own, meant for -fsanitize=address,undefined: a memcpy stands in
// for the DMA and a toy encoder for the device's, so nothing here touches a GPU.
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/way_out_check.cc -o way_out_check
//   ./way_out_check
//
// The toy encoder makes of a block of kBlock = 5 text bytes a member of one marker byte, the block's length, and the bytes;
// the EOF member is two bytes.  It reads its text and writes its buffer and the two size words only when the batch's "done"
// event is waited for — the latest moment the real one may — so a slot released, a buffer reused or a word read too early is
// a wrong byte or a sanitizer report, not luck.  Every buffer is an allocation of exactly its size: the two pieces, the two
// encoder buffers (max_blocks slots and the EOF member), every stretch of text, every window's output slot — which is freed
// the moment the way out reports it released.  Shapes: max_blocks 1, 2, 3; pieces of 1, 7 and more bytes than any stretch;
// whole texts of 0, 1, per - 1, per, per + 1, 2 per, 2 per + 1 and 5 per + 3 bytes (per = max_blocks blocks); windows that
// encode 0, 0, 3, 0, 1 blocks, several batches and then none, and an empty last one; the same with plain output.  Then every
// run again with a failure at every call in turn: the device fails, the sink fails, another thread stops the run.
// Exit status 0: every byte and every order agreed.
#include "../yacrd_amd/csrc/host/way_out.h"

#include <cstdio>
#include <fcntl.h>
#include <memory>
#include <string>
#include <vector>

namespace {

#define REQUIRE(cond)                                                                                                   \
    do {                                                                                                                \
        if (!(cond)) {                                                                                                  \
            std::fprintf(stderr, "way_out_check: line %d: %s\n", __LINE__, #cond);                                      \
            std::abort();                                                                                               \
        }                                                                                                               \
    } while (0)

enum Mode { kNone, kDevice, kSink, kStop };

struct Fake {
    static constexpr uint64_t kBlock = 5, kSlot = 7, kEofBytes = 2;
    struct Batch {
        const unsigned char *text;
        uint64_t len;
        bool last, waited;
        int which;
        volatile uint64_t *words;
        uint64_t bytes, copied; // its members (and the EOF member); of them copied out of the buffer and landed
    };
    uint64_t max_blocks;
    yseg::Sink *sink;
    std::unique_ptr<char[]> buf[2];
    std::vector<Batch> batches;
    uint64_t stored = 0;
    // the copy in hand (one home at a time)
    const char *base = nullptr;
    uint64_t started = 0, landed = 0, in_flight = 0;
    std::vector<uint64_t> seg_len;
    // failure injection: call `fail_at` (copies started and waited for, batches begun and waited for, counted together)
    Mode mode = kNone;
    long fail_at = -1, calls = 0, starts_since = 0, encodes_since = 0;
    int bad_fd = -1;
    bool stop = false, struck = false, reported = false; // struck: the failure has happened; reported: a call has returned it
    // the driver's: what a release means to it
    long last_tag = -1;
    void (*on_release)(void *, long) = nullptr;
    void *driver = nullptr;

    explicit Fake(uint64_t mb, yseg::Sink *s) : max_blocks(mb), sink(s)
    {
        for (auto &b : buf) b.reset(new char[mb * kSlot + kEofBytes]);
    }
    bool strike() // this call is the one that fails
    {
        if (calls++ != fail_at) return false;
        struck = true;
        if (mode == kStop) stop = true;
        if (mode == kSink) sink->fd = bad_fd; // (every put from here on fails)
        return mode == kDevice;
    }
    int batch_in(int which) const
    {
        for (size_t b = batches.size(); b-- > 0;)
            if (batches[b].which == which) return (int)b;
        return -1;
    }
    bool fetched(int b) const { return b < 0 || (batches[b].waited && batches[b].copied == batches[b].bytes); }

    struct Link {
        Fake *f;
        bool start(uint64_t i, char *dst, uint64_t at, size_t len)
        {
            REQUIRE(!f->reported && i == f->started && f->started - f->landed <= 1);
            // (behind a failure: the copy pump starts ahead of the put that fails, or ahead of the wait that sees the stop)
            if (f->struck) REQUIRE(++f->starts_since <= (f->mode == kSink ? 2 : 1) && f->mode != kDevice);
            if (f->strike()) return false;
            std::memcpy(dst, f->base + at, len); // (a piece cut too long, a buffer not the batch's: a sanitizer report)
            f->seg_len.push_back(len), f->started++, f->in_flight++;
            return true;
        }
        bool wait(uint64_t i)
        {
            REQUIRE(!f->reported);
            if (f->stop) return false;
            REQUIRE(i == f->landed && i < f->started);
            if (f->strike()) return false;
            for (int w = 0; w < 2; w++)
                if (f->base == f->buf[w].get()) f->batches[(size_t)f->batch_in(w)].copied += f->seg_len[i];
            f->landed++, f->in_flight--;
            return true;
        }
        void drain() { f->in_flight -= f->started - f->landed, f->landed = f->started; }
    };
    Link link(const char *from)
    {
        REQUIRE(started == landed);
        base = from, started = landed = 0, seg_len.clear();
        return Link{this};
    }
    bool encode(size_t b, const unsigned char *text, uint64_t len, bool last, int which, volatile uint64_t *words)
    {
        REQUIRE(!reported && b == batches.size() && which == (int)(b & 1) && len <= max_blocks * kBlock);
        if (struck) REQUIRE(mode == kSink && ++encodes_since <= 1); // (the first batch has nothing behind it to bring home)
        REQUIRE(fetched(batch_in(which)));               // the buffer and the pair of words: their batch before has come home
        REQUIRE(b < 2 || words == batches[b - 2].words); // ... and the pair is the one of b & 1, zeroed
        REQUIRE(b < 1 || words != batches[b - 1].words);
        REQUIRE(words[0] == 0 && words[1] == 0);
        for (const Batch &x : batches) REQUIRE(!x.last); // the EOF member: behind the last batch alone
        if (strike()) return false;
        batches.push_back(Batch{text, len, last, false, which, words, 0, 0});
        in_flight++;
        return true;
    }
    bool wait_done(size_t b)
    {
        REQUIRE(!reported && b < batches.size() && !batches[b].waited && (b == 0 || batches[b - 1].waited));
        if (strike()) return false;
        Batch &x = batches[b];
        char *o = buf[x.which].get();
        for (uint64_t at = 0; at < x.len; at += kBlock) { // (reads the text now: a slot released before this wait is gone)
            const uint64_t k = x.len - at < kBlock ? x.len - at : kBlock;
            *o++ = '#', *o++ = (char)('0' + k);
            std::memcpy(o, x.text + at, k), o += k;
            if (k < kBlock) stored++;
        }
        x.words[0] = (uint64_t)(o - buf[x.which].get()), x.words[1] = stored;
        if (x.last) *o++ = 'E', *o++ = 'F';
        x.bytes = (uint64_t)(o - buf[x.which].get()), x.waited = true, in_flight--;
        return true;
    }
    const unsigned char *out(int which) const { return reinterpret_cast<const unsigned char *>(buf[which].get()); }
    void released(long tag)
    {
        REQUIRE(!reported && tag > last_tag); // once, in rising order
        last_tag = tag;
        on_release(driver, tag);
    }
    bool stopped() const { return stop; }
    void quiet() { in_flight = 0, landed = started; }
};

using Way = yout::WayOut<Fake>;

std::string members_of(const std::string &text, bool last)
{
    std::string o;
    for (size_t at = 0; at < text.size(); at += Fake::kBlock) {
        const std::string blk = text.substr(at, Fake::kBlock);
        o += '#', o += (char)('0' + blk.size()), o += blk;
    }
    return last ? o + "EF" : o;
}

// one run: the windows' stretches in turn (a whole text is one window that is the last), gzip out or plain
struct Run {
    uint64_t max_blocks, piece;
    bool gzip;
    std::vector<uint64_t> lens; // what each window hands over
    Mode mode = kNone;
    long fail_at = -1;
    // what it found
    long calls = 0;
    yout::Result result = yout::kWent;

    std::vector<std::unique_ptr<unsigned char[]>> slot;
    std::vector<long> batch_of; // per window: the batch that carries its tag, -1: none, -2: not handed over yet
    Way *way = nullptr;
    Fake *fake = nullptr;
    long in_hand = -1;
    size_t sent_before = 0;

    Run(uint64_t mb, uint64_t pc, bool gz, const std::vector<uint64_t> &l, Mode m = kNone, long at = -1)
        : max_blocks(mb), piece(pc), gzip(gz), lens(l), mode(m), fail_at(at)
    {
    }
    static void on_release(void *self, long tag) { static_cast<Run *>(self)->release(tag); }
    void release(long tag)
    {
        REQUIRE(tag >= 0 && (size_t)tag < slot.size() && slot[(size_t)tag]);
        if (tag == in_hand) REQUIRE(way->sent == sent_before && way->got == way->sent); // released at once: it made no batch
        else REQUIRE(batch_of[(size_t)tag] >= 0 && fake->batches[(size_t)batch_of[(size_t)tag]].waited); // behind its batch's wait
        slot[(size_t)tag].reset();
    }
    bool note(yout::Result r)
    {
        if (r != yout::kWent) fake->reported = true, result = r;
        return r == yout::kWent;
    }
    void go()
    {
        yseg::Sink sink;
        sink.cap = 1, sink.mem = (char *)std::malloc(1);
        REQUIRE(sink.mem);
        Fake f(gzip ? max_blocks : 1, &sink);
        f.mode = mode, f.fail_at = fail_at, f.on_release = on_release, f.driver = this;
        f.bad_fd = ::open("/dev/null", O_RDONLY);
        REQUIRE(f.bad_fd >= 0);
        std::unique_ptr<char[]> halves(new char[2 * piece]);
        volatile uint64_t words[4] = {9, 9, 9, 9}; // (the way out zeroes a pair in front of its batch)
        Way w{f, sink, halves.get(), piece, words, gzip ? max_blocks : 0};
        way = &w, fake = &f;
        std::string want;
        unsigned char next = 0;
        slot.resize(lens.size()), batch_of.assign(lens.size(), -2);
        for (size_t k = 0; k < lens.size(); k++) { // (a careless caller: it goes on after a failure, and nothing may start)
            const bool last = k + 1 == lens.size();
            slot[k].reset(new unsigned char[lens[k] ? lens[k] : 1]);
            std::string text;
            for (uint64_t i = 0; i < lens[k]; i++) text += (char)(slot[k][i] = (unsigned char)('a' + next++ % 26));
            want += gzip ? members_of(text, last) : text;
            in_hand = (long)k, sent_before = w.sent;
            if (!gzip) {
                if (note(w.home(reinterpret_cast<const char *>(slot[k].get()), lens[k]))) slot[k].reset();
                continue;
            }
            note(w.text(slot[k].get(), lens[k], last, (long)k));
            batch_of[k] = w.sent > sent_before ? (long)w.sent - 1 : -1;
            in_hand = -1;
            if (batch_of[k] >= 0 && result == yout::kWent) REQUIRE(slot[k] && w.sent - w.got == 1); // its last batch is still out
        }
        in_hand = -1;
        const yout::Result end = w.drain();
        REQUIRE(f.in_flight == 0 && f.started == f.landed); // nothing is out behind drain, whatever happened
        if (result == yout::kWent) result = end;
        calls = f.calls;
        const std::string got(sink.mem, sink.at);
        if (result == yout::kWent) {
            REQUIRE(got == want && w.got == w.sent);
            for (auto &s : slot) REQUIRE(!s || !gzip); // every slot was released (plain: by this driver)
            if (gzip) {
                REQUIRE(!f.batches.empty() && f.batches.back().last && w.stored == f.stored);
                uint64_t total = 0, members = 0;
                for (uint64_t l : lens) total += l, members += (l + Fake::kBlock - 1) / Fake::kBlock;
                REQUIRE(w.text_bytes == total && w.members == members);
            }
            REQUIRE(mode == kNone || mode == kStop || fail_at >= calls);
        } else {
            REQUIRE(want.compare(0, got.size(), got) == 0); // what did arrive is a prefix: in order, nothing twice
            REQUIRE(f.struck && result == (mode == kDevice ? yout::kDeviceFailed : mode == kSink ? yout::kSinkFailed : yout::kStopped));
        }
        ::close(f.bad_fd);
        sink.fd = -1;
        std::free(sink.mem);
        way = nullptr, fake = nullptr, slot.clear();
    }
};

} // namespace

int main()
{
    uint64_t runs = 0, failed_runs = 0;
    for (uint64_t mb : {1, 2, 3}) {
        const uint64_t per = mb * Fake::kBlock;
        std::vector<std::vector<uint64_t>> shapes;
        for (uint64_t n : {(uint64_t)0, (uint64_t)1, per - 1, per, per + 1, 2 * per, 2 * per + 1, 5 * per + 3}) shapes.push_back({n});
        const uint64_t B = Fake::kBlock;
        shapes.push_back({0, 0, 3 * B, 0, 1 * B});      // a tail handed through windows that encode nothing
        shapes.push_back({(2 * mb + 1) * B, 0, B + 2}); // several batches, then none; a ragged last window
        shapes.push_back({2 * per, per, 0});            // an empty last window: the EOF member alone
        shapes.push_back({0, 0});
        for (const auto &lens : shapes)
            for (uint64_t piece : {(uint64_t)1, (uint64_t)7, 6 * per + 64})
                for (bool gzip : {true, false}) {
                    Run clean(mb, piece, gzip, lens);
                    clean.go();
                    if (clean.result != yout::kWent) return std::fprintf(stderr, "way_out_check: a clean run failed\n"), 1;
                    runs++;
                    for (Mode m : {kDevice, kSink, kStop})
                        for (long at = 0; at < clean.calls; at++) {
                            Run r(mb, piece, gzip, lens, m, at);
                            r.go();
                            if (r.result == yout::kWent && m != kStop) return std::fprintf(stderr, "way_out_check: a failure went unnoticed\n"), 1;
                            failed_runs++;
                        }
                }
    }
    std::printf("%llu runs, %llu more with a failure at every call in turn: every byte and every order agreed\n", (unsigned long long)runs,
                (unsigned long long)failed_runs);
    return 0;
}
