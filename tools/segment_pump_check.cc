// segment_pump_check.cc — host/segment_pump.h (the loop that brings the text of the device report writer and of the device
// overlap editor home, and the sink it ends in) and host/beside_file.h on their own, meant for
// -fsanitize=address,undefined: a memcpy stands in for the DMA, so nothing here touches a GPU.
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/segment_pump_check.cc -o segment_pump_check
//   ./segment_pump_check report1.yacrd report2.yacrd ...
//
// Every file is pumped at segment sizes 1, 2, 3, 7, 4096, 4097, size - 1, size, size + 1 and 64 MiB, once into memory and once
// into a file, and must come out as it went in.  The halves are allocated at exactly 2 x seg bytes and the source at exactly
// its size, so a segment cut one byte too long is a sanitizer report, not a lucky read.  Then, without any file named: the
// growing memory sink from a capacity of 1 byte; a file sink fed by two pumps that start at a non-zero offset of their text
// (the editor's case: one pump per segment into one sink); BesideFile's modes, commit and clean-up in a directory of its own
// under $TMPDIR (or /tmp).  Exit status 0: every byte agreed.
#include "../yacrd_amd/csrc/host/beside_file.h"
#include "../yacrd_amd/csrc/host/segment_pump.h"

#include <cstdio>
#include <cstdlib>
#include <dirent.h>
#include <fcntl.h>
#include <memory>
#include <string>
#include <vector>

namespace {

struct Copy { // the link: a plain copy out of the source, "in flight" until wait
    const char *text;
    uint64_t total, started = 0, landed = 0;
    bool start(uint64_t i, char *dst, uint64_t at, size_t len)
    {
        if (i != started || at + len > total) return false; // (segments start in order and end inside the text)
        std::memcpy(dst, text + at, len);
        started++;
        return true;
    }
    bool wait(uint64_t i) { return i == landed++ && i < started; }
    void drain() {}
};

bool slurp(const char *path, std::vector<char> &out)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    char buf[1 << 16];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) out.insert(out.end(), buf, buf + k);
    std::fclose(f);
    return true;
}

#define CHECK(cond, what)                                                                                              \
    do {                                                                                                               \
        if (!(cond)) return std::fprintf(stderr, "%s: %s\n", what, #cond), false;                                      \
    } while (0)

// a text of `total` bytes that repeats nowhere near a power of two
std::unique_ptr<char[]> pattern(uint64_t total)
{
    std::unique_ptr<char[]> t(new char[total ? total : 1]);
    for (uint64_t i = 0; i < total; i++) t[i] = (char)('!' + (i * 2654435761u >> 7) % 90);
    return t;
}

// the growing memory sink from a capacity of 1 byte, and from no memory at all (what a failed first malloc leaves)
bool growing_sink(uint64_t &pumps)
{
    for (uint64_t total : {(uint64_t)0, (uint64_t)1, (uint64_t)4095, (uint64_t)4096, (uint64_t)4097, (uint64_t)((3u << 20) + 5)}) {
        const std::unique_ptr<char[]> text = pattern(total);
        for (uint64_t seg : {(uint64_t)1, (uint64_t)4096, (uint64_t)1 << 20}) {
            if (seg == 1 && total > 5000) continue; // (a put per byte of megabytes is slow, not different)
            const uint64_t held = seg < total ? seg : total;
            std::unique_ptr<char[]> halves(new char[held ? 2 * held : 1]);
            for (bool from_nothing : {false, true}) {
                yseg::Sink sink;
                if (!from_nothing) {
                    sink.cap = 1, sink.mem = (char *)std::malloc(1);
                    CHECK(sink.mem, "growing sink");
                }
                Copy link{text.get(), total};
                const int rc = yseg::pump(total, seg, halves.get(), link, sink, [](auto put) { put(); });
                const bool ok = rc == yseg::kPumped && sink.at == total && sink.cap >= total &&
                                (!total || std::memcmp(sink.mem, text.get(), total) == 0);
                std::free(sink.mem);
                CHECK(ok, "growing sink");
                pumps++;
            }
        }
    }
    return true;
}

// base[from, upto) per segment into ONE file sink: the link is handed base + from, the pump's offsets are relative to it
bool pumps_from_an_offset(const std::string &dir, uint64_t &pumps)
{
    const uint64_t piece = 4096;
    for (uint64_t cut : {(uint64_t)1, piece - 1, piece, piece + 1, 2 * piece + 1}) {
        for (uint64_t rest : {(uint64_t)0, (uint64_t)1, piece - 1, piece, piece + 1, 2 * piece + 1}) {
            const uint64_t total = cut + rest;
            const std::unique_ptr<char[]> text = pattern(total);
            std::unique_ptr<char[]> halves(new char[2 * piece]);
            std::string tmp = dir + "/two.XXXXXX";
            yseg::Sink sink;
            sink.fd = mkstemp(&tmp[0]);
            CHECK(sink.fd >= 0, "pumps from an offset");
            int rc = yseg::kPumped;
            uint64_t from = 0;
            for (uint64_t upto : {cut, total}) { // (the second text is exactly what lies behind `from`: one byte more is a report)
                std::unique_ptr<char[]> part(new char[upto - from ? upto - from : 1]);
                std::memcpy(part.get(), text.get() + from, upto - from);
                Copy link{part.get(), upto - from};
                if (rc == yseg::kPumped) rc = yseg::pump(upto - from, piece, halves.get(), link, sink, [](auto put) { put(); });
                from = upto, pumps++;
            }
            std::unique_ptr<char[]> got(new char[total]);
            const bool ok = rc == yseg::kPumped && sink.at == total && (uint64_t)lseek(sink.fd, 0, SEEK_END) == total &&
                            pread(sink.fd, got.get(), total, 0) == (ssize_t)total && std::memcmp(got.get(), text.get(), total) == 0;
            close(sink.fd), unlink(tmp.c_str());
            CHECK(ok, "pumps from an offset");
        }
    }
    return true;
}

size_t entries(const std::string &dir)
{
    size_t k = 0;
    if (DIR *d = opendir(dir.c_str())) {
        while (const dirent *x = readdir(d))
            if (std::strcmp(x->d_name, ".") && std::strcmp(x->d_name, "..")) k++;
        closedir(d);
    }
    return k;
}

bool beside_file(const std::string &dir)
{
    const mode_t um = umask(0);
    umask(um);
    const std::string out = dir + "/out.txt";
    struct stat st;
    { // a new file: the mode open(2) would have given it
        yseg::BesideFile f;
        CHECK(f.open(out.c_str()) && f.fd >= 0 && entries(dir) == 1, "BesideFile, new");
        CHECK(write(f.fd, "abc", 3) == 3 && f.commit(), "BesideFile, new");
    }
    CHECK(entries(dir) == 1 && stat(out.c_str(), &st) == 0 && st.st_size == 3 && (st.st_mode & 07777) == (0666 & ~um), "BesideFile, new");
    { // over a 0640 file whose stat is handed in: 0640 stays; without the stat the mode is a new file's
        CHECK(chmod(out.c_str(), 0640) == 0 && stat(out.c_str(), &st) == 0, "BesideFile, existing");
        yseg::BesideFile f;
        CHECK(f.open(out.c_str(), &st) && write(f.fd, "defg", 4) == 4 && f.commit(), "BesideFile, existing");
        CHECK(entries(dir) == 1 && stat(out.c_str(), &st) == 0 && st.st_size == 4 && (st.st_mode & 07777) == 0640, "BesideFile, existing");
        yseg::BesideFile g;
        CHECK(g.open(out.c_str()) && g.commit() && stat(out.c_str(), &st) == 0 && st.st_size == 0 && (st.st_mode & 07777) == (0666 & ~um),
              "BesideFile, existing without its stat");
    }
    CHECK(unlink(out.c_str()) == 0 && entries(dir) == 0, "BesideFile");
    { // not committed: neither the file nor its sibling stays
        yseg::BesideFile f;
        CHECK(f.open(out.c_str()) && write(f.fd, "x", 1) == 1 && entries(dir) == 1, "BesideFile, dropped");
    }
    CHECK(entries(dir) == 0, "BesideFile, dropped");
    { // an existing file survives a drop as it was
        CHECK(close(open(out.c_str(), O_CREAT | O_WRONLY, 0600)) == 0, "BesideFile, dropped over a file");
        {
            yseg::BesideFile f;
            CHECK(f.open(out.c_str()) && write(f.fd, "x", 1) == 1, "BesideFile, dropped over a file");
            f.drop();
            CHECK(f.fd < 0 && !f.commit(), "BesideFile, dropped over a file");
        }
        CHECK(entries(dir) == 1 && stat(out.c_str(), &st) == 0 && st.st_size == 0 && unlink(out.c_str()) == 0, "BesideFile, dropped over a file");
    }
    { // a directory that does not exist
        yseg::BesideFile f;
        CHECK(!f.open((dir + "/none/out.txt").c_str()) && f.fd < 0 && !f.commit(), "BesideFile, no directory");
    }
    CHECK(entries(dir) == 0, "BesideFile, no directory");
    return true;
}

} // namespace

int main(int argc, char **argv)
{
    uint64_t pumps = 0;
    for (int a = 1; a < argc; a++) {
        std::vector<char> in;
        if (!slurp(argv[a], in)) return std::fprintf(stderr, "cannot read %s\n", argv[a]), 2;
        const uint64_t total = in.size();
        std::unique_ptr<char[]> text(new char[total ? total : 1]); // exactly the text: one byte beyond is a report
        if (total) std::memcpy(text.get(), in.data(), total);
        std::vector<uint64_t> segs = {1, 2, 3, 7, 4096, 4097, total, total + 1, (uint64_t)64 << 20};
        if (total > 1) segs.push_back(total - 1);
        if (total > 200000) segs.erase(segs.begin(), segs.begin() + 3); // (a put per byte of a large file into a file is slow, not different)
        for (uint64_t seg : segs) {
            if (!seg) continue;
            const uint64_t held = seg < total ? seg : total;
            for (int to_file = 0; to_file < 2; to_file++) {
                std::unique_ptr<char[]> halves(new char[held ? 2 * held : 1]);
                std::unique_ptr<char[]> got(new char[total ? total : 1]);
                yseg::Sink sink;
                std::string tmp = std::string(argv[a]) + ".pump.XXXXXX";
                if (to_file) {
                    sink.fd = mkstemp(&tmp[0]);
                    if (sink.fd < 0) return std::fprintf(stderr, "cannot create %s\n", tmp.c_str()), 2;
                } else
                    sink.mem = got.get();
                Copy link{text.get(), total};
                uint64_t puts = 0;
                const int rc = yseg::pump(total, seg, halves.get(), link, sink, [&](auto put) { put(), puts++; });
                bool ok = rc == yseg::kPumped && puts == (total ? (total + held - 1) / held : 0);
                if (to_file) {
                    ok = ok && (uint64_t)lseek(sink.fd, 0, SEEK_END) == total && pread(sink.fd, got.get(), total, 0) == (ssize_t)total;
                    close(sink.fd), unlink(tmp.c_str());
                }
                ok = ok && std::memcmp(got.get(), text.get(), total) == 0;
                if (!ok) return std::fprintf(stderr, "%s: segment %llu, %s: rc %d, %llu puts: the text differs\n", argv[a], (unsigned long long)seg, to_file ? "file" : "memory", rc, (unsigned long long)puts), 1;
                pumps++;
            }
        }
    }
    const char *base = std::getenv("TMPDIR");
    std::string dir = std::string(base && *base ? base : "/tmp") + "/segment_pump_check.XXXXXX";
    if (!mkdtemp(&dir[0])) return std::fprintf(stderr, "cannot create %s\n", dir.c_str()), 2;
    uint64_t extra = 0;
    const bool ok = growing_sink(extra) && pumps_from_an_offset(dir, extra) && beside_file(dir);
    if (rmdir(dir.c_str()) != 0 || !ok) return std::fprintf(stderr, "%s: %s\n", dir.c_str(), ok ? "not empty at the end" : "left for a look"), 1;
    std::printf("%d texts, %llu pumps: every byte agreed; %llu pumps into a growing sink and from an offset, BesideFile: as specified\n", argc - 1,
                (unsigned long long)pumps, (unsigned long long)extra);
    return 0;
}
