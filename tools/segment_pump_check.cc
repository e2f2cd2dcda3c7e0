// segment_pump_check.cc — host/segment_pump.h (the loop that brings the device report writer's text home) on its own, meant
// for -fsanitize=address,undefined: a memcpy stands in for the DMA, so nothing here touches a GPU.
//
//   c++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tools/segment_pump_check.cc -o segment_pump_check
//   ./segment_pump_check report1.yacrd report2.yacrd ...
//
// Every file is pumped at segment sizes 1, 2, 3, 7, 4096, 4097, size - 1, size, size + 1 and 64 MiB, once into memory and once
// into a file, and must come out as it went in.  The halves are allocated at exactly 2 x seg bytes and the source at exactly
// its size, so a segment cut one byte too long is a sanitizer report, not a lucky read.  Exit status 0: every byte agreed.
#include "../yacrd_amd/csrc/host/segment_pump.h"

#include <cstdio>
#include <cstdlib>
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
    std::printf("%d texts, %llu pumps: every byte agreed\n", argc - 1, (unsigned long long)pumps);
    return 0;
}
