// cli.cc — `yacrd` drop-in command line over the MI355X engine.
//
// Same flags, defaults, file-type rules and outputs as the reference binary
// (src/cli.rs:33-137, src/main.rs:36-137):
//   yacrd -i <overlaps.paf|.m4|.mhap|report.yacrd> -o <report.yacrd> [-t N] [-c COV] [-n RATIO]
//         [--read-buffer-size N] [-d PREFIX] [--ondisk-buffer-size N]
//         [scrubb|filter|extract|split -i <in> -o <out>]
// Additive flags only: --gpus N (default 1): an input beyond one GPU's memory is partitioned over N GPUs by id handle.
// The bad-region computation and the read classification run on the GPU through
// include/yacrd_engine.h; there is no CPU fallback — without a gfx950 device this exits non-zero.
#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../../../include/yacrd_engine.h"
#include "../../../include/yacrd_engine_debug.h" // (YACRD_SEQ_WINDOW: the FASTQ and FASTA editors' window, an A/B and test switch)
#include "../../../include/yacrd_host.h"

namespace {

const char *kVersion = "1.0.0 Magby";

[[noreturn]] void die(const std::string &msg, int code = 1)
{
    std::fprintf(stderr, "Error: %s\n", msg.c_str());
    std::exit(code);
}

void usage(FILE *f)
{
    std::fprintf(f,
                 "yacrd %s (MI355X engine)\n"
                 "USAGE:\n    yacrd [OPTIONS] --input <INPUT> --output <OUTPUT> [SUBCOMMAND]\n\n"
                 "OPTIONS:\n"
                 "    -i, --input <INPUT>                  overlap file (.paf|.m4|.mhap) or yacrd report (.yacrd)\n"
                 "    -o, --output <OUTPUT>                path output file\n"
                 "    -t, --thread <THREADS>               host threads for the overlap parse [default: 1, like the\n"
                 "                                         reference's rayon pool]; 0 = every usable CPU, which is what\n"
                 "                                         you want: the parse is the whole wall clock\n"
                 "    -c, --coverage <COVERAGE>            if coverage reach this value region is marked as bad [default: 0]\n"
                 "    -n, --not-coverage <NOT_COVERAGE>    bad-region ratio above which a read is NotCovered [default: 0.8]\n"
                 "        --read-buffer-size <N>           accepted for compatibility [default: 8192]\n"
                 "    -d, --ondisk <PREFIX>                accepted for compatibility (HBM + host RAM hold the overlaps)\n"
                 "        --ondisk-buffer-size <N>         accepted for compatibility [default: 64000000]\n"
                 "        --gpus <N>                       GPUs to partition the reads over [default: 1]\n"
                 "    -h, --help    -V, --version\n\n"
                 "SUBCOMMANDS (each takes -i <input> -o <output>):\n"
                 "    scrubb     all bad region of read is removed\n"
                 "    filter     record mark as chimeric or NotCovered is filter\n"
                 "    extract    record mark as chimeric or NotCovered is extract\n"
                 "    split      record mark as chimeric or NotCovered is split\n",
                 kVersion);
}

bool parse_u64(const char *s, unsigned long long &v)
{
    if (!*s) return false;
    errno = 0;
    char *end = nullptr;
    if (*s == '-') return false;
    v = std::strtoull(s, &end, 10);
    return errno == 0 && end && *end == '\0';
}

bool has(const std::string &s, const char *needle) { return s.find(needle) != std::string::npos; }

// a regular file that begins with the gzip magic, mapped as it is for the engine's _bgzf_mem forms (which tell BGZF from plain gzip)
struct GzipMap {
    void *m = MAP_FAILED;
    size_t n = 0;
    bool open(const char *path)
    {
        const int fd = ::open(path, O_RDONLY);
        struct stat st;
        if (fd >= 0 && ::fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size >= 2) {
            unsigned char mg[2] = {0, 0};
            if (::pread(fd, mg, 2, 0) == 2 && mg[0] == 0x1f && mg[1] == 0x8b) {
                n = (size_t)st.st_size;
                m = ::mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
            }
        }
        if (fd >= 0) ::close(fd);
        return m != MAP_FAILED;
    }
    const char *data() const { return static_cast<const char *>(m); }
    ~GzipMap()
    {
        if (m != MAP_FAILED) ::munmap(m, n);
    }
};

void print_device_inflate(const yacrd_gunzip_stats &us)
{
    std::fprintf(stderr, "[info] device inflate: %llu members, %llu -> %llu bytes, walk %.1f ms, h2d %.1f ms, kernels %.1f ms\n",
                 (unsigned long long)us.n_members, (unsigned long long)us.in_bytes, (unsigned long long)us.out_bytes, us.walk_ms, us.h2d_ms,
                 us.kernel_ms);
}

// whether a gzip file's first member carries BGZF's `BC` subfield: such a file is the _bgzf_ route's, and what that route
// hands back of it is not retried as plain gzip (it would go up again only to end as "bytes left over")
bool first_member_is_bgzf(const unsigned char *p, size_t n)
{
    if (n < 12 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4)) return false;
    const size_t end = 12 + ((size_t)p[10] | ((size_t)p[11] << 8));
    for (size_t q = 12; q + 4 <= end && q + 4 <= n;) {
        const size_t slen = (size_t)p[q + 2] | ((size_t)p[q + 3] << 8);
        if (p[q] == 'B' && p[q + 1] == 'C' && slen == 2) return true;
        q += 4 + slen;
    }
    return false;
}

void print_device_gunzip(const yacrd_gunzip_stream_stats &zs)
{
    std::fprintf(stderr, "[info] device gunzip: %llu -> %llu bytes, %llu chunks, %llu spans (%llu false starts, %llu rounds), %llu blocks, h2d %.1f ms, "
                         "find %.1f ms, size %.1f ms, symbols %.1f ms, windows %.1f ms, bytes %.1f ms\n",
                 (unsigned long long)zs.in_bytes, (unsigned long long)zs.out_bytes, (unsigned long long)zs.n_chunks, (unsigned long long)zs.n_spans,
                 (unsigned long long)zs.n_false_starts, (unsigned long long)zs.rounds, (unsigned long long)zs.n_blocks, zs.h2d_ms, zs.find_ms, zs.size_ms,
                 zs.symbols_ms, zs.windows_ms, zs.bytes_ms);
}

} // namespace

int main(int argc, char **argv)
{
    std::string input, output, sub, sub_in, sub_out, ondisk;
    unsigned long long threads = 1, coverage = 0, gpus = 1, tmp = 0;
    double not_coverage = 0.8;

    int i = 1;
    auto value = [&](const char *flag) -> const char * {
        if (i + 1 >= argc) die(std::string("The argument '") + flag + "' requires a value", 2);
        return argv[++i];
    };
    for (; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "-h" || a == "--help") {
            usage(stdout);
            return 0;
        } else if (a == "-V" || a == "--version") {
            std::printf("yacrd %s\n", kVersion);
            return 0;
        } else if (a == "-i" || a == "--input") input = value("--input");
        else if (a == "-o" || a == "--output") output = value("--output");
        else if (a == "-t" || a == "--thread") {
            if (!parse_u64(value("--thread"), threads)) die("Invalid value for '--thread'", 2);
        } else if (a == "-c" || a == "--coverage") {
            if (!parse_u64(value("--coverage"), coverage)) die("Invalid value for '--coverage'", 2);
        } else if (a == "-n" || a == "--not-coverage") {
            char *end = nullptr;
            const char *v = value("--not-coverage");
            not_coverage = std::strtod(v, &end);
            if (!*v || (end && *end)) die("Invalid value for '--not-coverage'", 2);
        } else if (a == "--read-buffer-size") {
            if (!parse_u64(value("--read-buffer-size"), tmp)) die("Invalid value for '--read-buffer-size'", 2);
        } else if (a == "-d" || a == "--ondisk") ondisk = value("--ondisk");
        else if (a == "--ondisk-buffer-size") (void)value("--ondisk-buffer-size");
        else if (a == "--gpus") {
            if (!parse_u64(value("--gpus"), gpus) || gpus == 0) die("Invalid value for '--gpus'", 2);
        } else if (a == "scrubb" || a == "filter" || a == "extract" || a == "split") {
            sub = a;
            for (i++; i < argc; i++) {
                const std::string b = argv[i];
                if (b == "-i" || b == "--input") sub_in = value("--input");
                else if (b == "-o" || b == "--output") sub_out = value("--output");
                else die("Found argument '" + b + "' which wasn't expected in subcommand " + sub, 2);
            }
            if (sub_in.empty() || sub_out.empty())
                die("The following required arguments were not provided: --input --output (" + sub + ")", 2);
        } else {
            die("Found argument '" + a + "' which wasn't expected", 2);
        }
    }
    if (input.empty() || output.empty()) {
        usage(stderr);
        die("The following required arguments were not provided: --input <INPUT> --output <OUTPUT>", 2);
    }
    if (!ondisk.empty())
        std::fprintf(stderr, "[INFO] --ondisk is accepted for compatibility; overlaps are kept in "
                             "host memory and HBM (same results, reference tests/run.rs:120-160)\n");

    // YACRD_CLI_TIMING=1: wall clock of every stage on stderr (tools/e2e_scrubb_full.py)
    const bool timing = std::getenv("YACRD_CLI_TIMING") != nullptr;
    auto t_last = std::chrono::steady_clock::now();
    auto stage = [&](const char *what) {
        const auto now = std::chrono::steady_clock::now();
        if (timing) std::fprintf(stderr, "[timing] %s %.3f s\n", what, std::chrono::duration<double>(now - t_last).count());
        t_last = now;
    };

    // ---- engines (one per GPU)
    std::vector<yacrd_engine *> engines;
    // YACRD_GPUS_ON_DEVICE=<d>: every engine on device d (how the N > 1 path is tested on a one-GPU box)
    const char *same_dev = std::getenv("YACRD_GPUS_ON_DEVICE");
    for (unsigned long long g = 0; g < gpus; g++) {
        // a process runs ONE batch per engine: a short one goes out as one kernel launch (csrc/one_batch.h; anything that
        // launch does not take falls back to the default path inside the engine); YACRD_CLI_NO_ONE_LAUNCH=1 for A/B
        const char *no_one = std::getenv("YACRD_CLI_NO_ONE_LAUNCH");
        const uint32_t eflags = (no_one && *no_one && *no_one != '0') ? YACRD_F_DEFAULT : YACRD_F_ONE_LAUNCH;
        yacrd_engine_cfg cfg = {same_dev && *same_dev ? (int32_t)std::atoi(same_dev) : (int32_t)g, eflags};
        yacrd_engine *e = nullptr;
        if (yacrd_engine_create(&cfg, &e) != YACRD_OK) die(yacrd_last_error());
        engines.push_back(e);
    }
    const uint32_t cov32 = coverage > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)coverage;
    stage("engine_create");

    yacrd_csr *csr = nullptr;
    yacrd_report *rep = nullptr;
    yacrd_result res{};
    std::vector<uint8_t> rep_types;
    yacrd_badparts_view bp{};
    yacrd_csr_view view{};
    yacrd_reads dev_reads{};
    bool table_resident = false; // this invocation's input went through a one-engine device ingest: its table lies in engines[0]'s HBM
    yacrd_text text{}; // a compressed input, inflated (empty otherwise); lives as long as what was parsed from it

    // src/main.rs:43-60: a .yacrd input bypasses detection (FromReport), anything else is overlaps
    const bool m4 = has(input, ".m4") || has(input, ".mhap"), paf = has(input, ".paf");
    // A gzip input of the detection with ONE engine is mapped as it is and offered to the engine's _bgzf_mem form first: a BGZF
    // file crosses the link compressed and is inflated in HBM while it lands, the host inflates nothing.  Whatever
    // that form hands back (YACRD_EFALLBACK: plain gzip, a member the device decoder does not take, the parser's / the reader's
    // own causes; no memory) leaves nothing behind and takes the route below, unchanged.  bzip2, xz and --gpus N > 1 never try
    // it; YACRD_NO_DEVICE_INFLATE=1 skips it, as for the sequence editors.  When a sub-command will edit this very file, the host
    // inflate stays — the sequence editors want the detection's host text, and inflating twice costs more than the link saves —
    // unless that sub-command is the device overlap editor with the device deflate (filter / extract on this gzip PAF / M4):
    // it edits the text the ingest leaves inflated in HBM (yacrd_engine_edit_overlaps_resident_file), so the file
    // goes up compressed once and only BGZF members come home.
    // The default, by DESIGN 7i's rows (the slowest `ingest` of three with it against the fastest of three without): a `.yacrd`
    // report takes it (113-133 ms against 155-157 ms on the 5 M-read report); an overlap file takes it with
    // YACRD_DEVICE_INFLATE=1 only (110-158 ms against 145-198 ms on the 367 MB PAF: the slowest is not under the fastest).
    // The combined route of 7j (ingest compressed, edit resident) and the editor's own _bgzf_ form for another BGZF file are the
    // default by the same rule (DESIGN 7j's table, tools/edit_overlaps_bench.py --bgzf-in --parent-bin on that PAF, the stages
    // inflate + detect + edit): 0.254-0.262 s against the parent's 0.322-0.354 s on the detection's own file, 0.333-0.336 s
    // against 0.451-0.467 s on a copy of it.
    const char *no_inf_in = std::getenv("YACRD_NO_DEVICE_INFLATE"), *yes_inf_in = std::getenv("YACRD_DEVICE_INFLATE");
    const bool report_in = !m4 && !paf && has(input, ".yacrd");
    // the device overlap editor with the device deflate will run on sub_in (if it is gzip; the editor's section looks)
    const bool sub_dev_ovl_gz = [&] {
        const char *no_ed = std::getenv("YACRD_NO_DEVICE_EDITOR"), *no_df = std::getenv("YACRD_NO_DEVICE_DEFLATE");
        return (sub == "filter" || sub == "extract") && (has(sub_in, ".m4") || has(sub_in, ".mhap") || has(sub_in, ".paf")) &&
               !(no_ed && *no_ed == '1') && !(no_df && *no_df == '1');
    }();
    const bool inflate_on = engines.size() == 1 && !(no_inf_in && *no_inf_in == '1');
    const bool ovl_inflate_on = inflate_on && yes_inf_in && *yes_inf_in == '1';
    bool sub_same_file = false;
    if (!sub.empty()) {
        struct stat sa, sb;
        sub_same_file = ::stat(input.c_str(), &sa) == 0 && ::stat(sub_in.c_str(), &sb) == 0 && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino;
    }
    bool bgzf_route = inflate_on && (report_in || ovl_inflate_on || (sub_dev_ovl_gz && sub_same_file));
    if (bgzf_route && sub_same_file && !sub_dev_ovl_gz) bgzf_route = false;
    bool ovl_resident = false; // the detection's overlap text lies inflated in engines[0]'s HBM (and nowhere on the host)

    if (!m4 && !paf && has(input, ".yacrd")) {
        // The report's text goes to HBM and the device parses it, keeps every id's last row at its first position, fills the
        // region CSR and classifies it with this invocation's -n (yacrd_engine_ingest_report; a compressed report is inflated
        // first and takes the _mem form, as a compressed overlap file does).  Whatever that reader does not take — a corrupt
        // line above all — comes back as YACRD_EFALLBACK and takes the host reader below, which words the error with its
        // line number.  YACRD_NO_DEVICE_REPORT=1: the host reader (A/B).
        int dev_rep = YACRD_EFALLBACK;
        const char *no_rep = std::getenv("YACRD_NO_DEVICE_REPORT");
        if (!(no_rep && *no_rep == '1')) {
            const char *ct = std::getenv("YACRD_COPY_THREADS");
            const int copy_threads = ct && *ct ? std::max(0, std::atoi(ct)) : 0;
            yacrd_ingest_stats is{};
            yacrd_gunzip_stats us{};
            GzipMap gm;
            if (bgzf_route && gm.open(input.c_str())) {
                dev_rep = yacrd_engine_ingest_report_bgzf_mem(engines[0], gm.data(), gm.n, copy_threads, not_coverage, &res, &dev_reads, &is, &us);
                if (dev_rep == YACRD_ENOMEM) {
                    for (yacrd_engine *en : engines) (void)yacrd_engine_trim(en);
                    dev_rep = YACRD_EFALLBACK;
                }
                if (dev_rep != YACRD_OK && dev_rep != YACRD_EFALLBACK) die(yacrd_last_error());
            }
            const bool dev_inflate = dev_rep == YACRD_OK;
            int rct = 0;
            if (!dev_inflate) {
                rct = yacrd_text_from_file(input.c_str(), threads == 1 ? 0 : (int)threads, &text);
                stage("inflate");
                // (rct 1, a file that cannot be read or inflated: the host reader below words that error too)
                dev_rep = rct == 1 ? YACRD_EFALLBACK : rct == 0 ? yacrd_engine_ingest_report_mem(engines[0], text.data, text.n, copy_threads, not_coverage, &res, &dev_reads, &is)
                                   : yacrd_engine_ingest_report(engines[0], input.c_str(), copy_threads, not_coverage, &res, &dev_reads, &is);
            }
            if (dev_rep == YACRD_ENOMEM) {
                std::fprintf(stderr, "[INFO] device report reader: %s; falling back to the host reader\n", yacrd_last_error());
                for (yacrd_engine *en : engines) (void)yacrd_engine_trim(en);
                dev_rep = YACRD_EFALLBACK;
            }
            if (dev_rep != YACRD_OK && dev_rep != YACRD_EFALLBACK) die(yacrd_last_error());
            if (dev_rep == YACRD_OK && timing)
                std::fprintf(stderr, "[info] device report reader: %llu reads from %llu lines, %llu bytes%s, text %.1f ms, parse %.1f ms, build %.1f ms, "
                                     "d2h %.1f ms\n",
                             (unsigned long long)is.n_reads, (unsigned long long)is.n_records, (unsigned long long)is.text_bytes,
                             dev_inflate ? " (inflated in HBM)" : rct == 0 ? " (inflated)" : "", is.text_ms, is.parse_ms, is.build_ms, is.d2h_ms);
            if (dev_inflate && timing) print_device_inflate(us);
        }
        if (dev_rep == YACRD_OK) {
            table_resident = true;
            bp.n_reads = view.n_reads = dev_reads.n_reads;
            bp.name_off = view.name_off = dev_reads.name_off;
            bp.names = view.names = dev_reads.names;
            bp.lengths = view.lengths = dev_reads.lengths;
            bp.bad_offsets = res.bad_offsets;
            bp.bad_regions = res.bad_regions;
            bp.read_type = res.read_type;
        } else {
            if (yacrd_report_read(input.c_str(), &rep)) die(yacrd_host_last_error());
            yacrd_report_get(rep, &bp);
            rep_types.resize((size_t)bp.n_reads + 1);
            // type_of_read with this invocation's -n, on the GPU (kernel #2)
            if (yacrd_engine_classify(engines[0], bp.bad_offsets, bp.bad_regions, bp.lengths, bp.n_reads,
                                      not_coverage, rep_types.data()) != YACRD_OK)
                die(yacrd_last_error());
            bp.read_type = rep_types.data();
            view.n_reads = bp.n_reads;
            view.name_off = bp.name_off;
            view.names = bp.names;
            view.lengths = bp.lengths;
        }
    } else {
        int dev_parse = YACRD_EFALLBACK;
        // YACRD_NO_DEVICE_PARSER=1: the host parser for everything (A/B, tools/e2e_cli_paf.py)
        const char *no_dev = std::getenv("YACRD_NO_DEVICE_PARSER");
        // (--gpus N > 1: every GPU moves and parses a byte range of the text over its own link and sweeps a range of the reads,
        // yacrd_engines_ingest_overlaps; an input beyond the GPUs' memory — the call estimates every device's need, its ranges
        // and the records it gathers from the others, before it allocates anything, and an allocation that fails later after all
        // comes back as an error too — is routed to all N by the host parser's stream group)
        if ((paf || m4) && !(no_dev && *no_dev == '1')) {
            // one GPU, PAF or M4 text: the host only moves the file to HBM, the device parses it, numbers the reads,
            // builds the CSR and runs the engine (yacrd_engine_ingest_overlaps).  Whatever is not a plain file of
            // plain records (compressed, quoted fields, lone CRs, 0x integers, malformed lines ...) comes back as
            // YACRD_EFALLBACK and takes the host parser below, which knows the whole syntax and the messages.
            // The threads that move the file into pinned memory are not the reference's rayon pool: their number does
            // not follow -t (default 1 = 8 GB/s of a 56 GB/s link); the engine's own default (6) unless
            // YACRD_COPY_THREADS says otherwise.
            const char *ct = std::getenv("YACRD_COPY_THREADS");
            const int copy_threads = ct && *ct ? std::max(0, std::atoi(ct)) : 0;
            // a gzip / bzip2 / xz file (src/util.rs:57-70 sniffs every input): inflated into memory first — BGZF members on
            // every usable CPU, any other stream on one thread, which then is the wall clock whichever parser follows
            yacrd_gunzip_stats us{};
            GzipMap gm;
            if (bgzf_route && gm.open(input.c_str())) {
                dev_parse = yacrd_engine_ingest_overlaps_bgzf_mem(engines[0], gm.data(), gm.n, m4 ? 2 : 1, copy_threads, cov32, not_coverage, &res,
                                                                  &dev_reads, nullptr, &us);
                if (dev_parse == YACRD_ENOMEM) {
                    for (yacrd_engine *en : engines) (void)yacrd_engine_trim(en);
                    dev_parse = YACRD_EFALLBACK;
                }
                if (dev_parse != YACRD_OK && dev_parse != YACRD_EFALLBACK) die(yacrd_last_error());
                if (dev_parse == YACRD_OK && timing) print_device_inflate(us);
                ovl_resident = dev_parse == YACRD_OK;
            }
            if (dev_parse != YACRD_OK) {
                const int rct = yacrd_text_from_file(input.c_str(), threads == 1 ? 0 : (int)threads, &text);
                if (rct == 1) die(yacrd_host_last_error());
                stage("inflate");
                if (rct == 0)
                    dev_parse = yacrd_engines_ingest_overlaps_mem(engines.data(), (uint32_t)engines.size(), text.data, text.n, m4 ? 2 : 1,
                                                                  copy_threads, cov32, not_coverage, &res, &dev_reads, nullptr);
                else
                    dev_parse = yacrd_engines_ingest_overlaps(engines.data(), (uint32_t)engines.size(), input.c_str(), m4 ? 2 : 1, copy_threads,
                                                              cov32, not_coverage, &res, &dev_reads, nullptr);
            }
            if (dev_parse == YACRD_ENOMEM) { // HBM ran out on the way (the parse wants ~2.6 x the file): the streamed host parse needs a fifth
                std::fprintf(stderr, "[INFO] device parser: %s; falling back to the host parser\n", yacrd_last_error());
                for (yacrd_engine *en : engines) (void)yacrd_engine_trim(en);
                dev_parse = YACRD_EFALLBACK;
            }
            if (dev_parse != YACRD_OK && dev_parse != YACRD_EFALLBACK) die(yacrd_last_error());
        }
        if (dev_parse == YACRD_OK) {
            if (std::getenv("YACRD_CLI_TIMING")) std::fprintf(stderr, "[info] device parser: %zu engine(s)\n", engines.size());
            table_resident = engines.size() == 1;
            view.n_reads = dev_reads.n_reads;
            view.name_off = dev_reads.name_off;
            view.names = dev_reads.names;
            view.lengths = dev_reads.lengths;
        } else {
            // The parser's records cross PCIe from pinned buffers while it is still parsing — routed by
            // handle mod N to the GPUs of their two reads (yacrd_stream_group_*; with one GPU the sink is the
            // stream's own) — every GPU builds the CSR of its reads in HBM and runs on it, no collective
            // (reads are independent, src/stack.rs:61); results come back in first-appearance order.
            yacrd_stream_group *grp = nullptr;
            if (yacrd_stream_group_open(engines.data(), (uint32_t)engines.size(), 0, 0, &grp) != YACRD_OK)
                die(yacrd_last_error());
            yacrd_rec_sink sink;
            yacrd_stream_group_sink(grp, &sink);
            // (a compressed input the device parser handed over is parsed from the text already inflated)
            if (text.data ? yacrd_ingest_stream_memory(text.data, (size_t)text.n, m4 ? 2 : 1, (int)threads, &sink, &csr)
                          : yacrd_ingest_stream(input.c_str(), 0, (int)threads, &sink, &csr))
                die(yacrd_host_last_error());
            yacrd_csr_get(csr, &view);
            const uint32_t *map = nullptr;
            uint64_t n_handles = 0;
            if (yacrd_csr_handle_map(csr, &map, &n_handles)) die(yacrd_host_last_error());
            if (yacrd_stream_group_finish(grp, map, n_handles, view.lengths, view.n_reads, cov32, not_coverage,
                                          &res) != YACRD_OK)
                die(yacrd_last_error());
            yacrd_stream_group_close(grp);
        }
        bp.n_reads = view.n_reads;
        bp.name_off = view.name_off;
        bp.names = view.names;
        bp.lengths = view.lengths;
        bp.bad_offsets = res.bad_offsets;
        bp.bad_regions = res.bad_regions;
        bp.read_type = res.read_type;
    }

    stage("detect");
    // src/main.rs:62-84: the report, one line per read
    // The device formats it (yacrd_engine_write_report): from the table the ingest left in HBM when this invocation's input
    // went through a one-engine device ingest, else from the host arrays, uploaded to engines[0].  Whatever that writer does
    // not take — a type beyond 2, an output that is no regular file or cannot be created — comes back with nothing written
    // and takes the host writer below, which owns the messages.  (It leaves the parser's mirror alone: an edit_overlaps
    // below may still start from it.)  YACRD_NO_DEVICE_REPORT_WRITER=1: the host writer (A/B).  The device writer is the
    // default because DESIGN 7e's measured table has its slowest warm run ahead of the host writer's fastest at 5 M reads.
    int dev_write = YACRD_EFALLBACK;
    {
        const char *no_rw = std::getenv("YACRD_NO_DEVICE_REPORT_WRITER");
        if (!(no_rw && *no_rw == '1')) {
            const yacrd_report_table rt = {view.n_reads, view.name_off, view.names, view.lengths, bp.bad_offsets, bp.bad_regions, bp.read_type};
            yacrd_report_write_stats ws{};
            dev_write = yacrd_engine_write_report(engines[0], table_resident ? nullptr : &rt, output.c_str(), &ws);
            if (dev_write == YACRD_ENOMEM) {
                std::fprintf(stderr, "[INFO] device report writer: %s; falling back to the host writer\n", yacrd_last_error());
                for (yacrd_engine *en : engines) (void)yacrd_engine_trim(en);
                dev_write = YACRD_EFALLBACK;
            }
            if (dev_write != YACRD_OK && dev_write != YACRD_EFALLBACK) die(yacrd_last_error());
            if (dev_write == YACRD_OK && timing)
                std::fprintf(stderr, "[info] device report writer: %llu reads, %llu regions, %llu bytes, %s, upload %.1f ms, kernels %.1f ms, out %.1f ms\n",
                             (unsigned long long)ws.n_reads, (unsigned long long)ws.n_regions, (unsigned long long)ws.text_bytes,
                             ws.resident ? "resident table" : "table uploaded", ws.up_ms, ws.kernel_ms, ws.out_ms);
        }
    }
    if (dev_write != YACRD_OK) {
        if (timing) std::fprintf(stderr, "[info] host report writer\n");
        if (yacrd_report_write(output.c_str(), &view, bp.bad_offsets, bp.bad_regions, bp.read_type)) die(yacrd_host_last_error());
    }
    stage("report");

    // src/main.rs:86-118: optional post operation
    if (!sub.empty()) {
        const int op = sub == "scrubb" ? YACRD_OP_SCRUBB
                                       : sub == "filter" ? YACRD_OP_FILTER
                                                         : sub == "extract" ? YACRD_OP_EXTRACT : YACRD_OP_SPLIT;
        // filter / extract on a PAF / M4 / MHAP: the text goes to HBM, the device decides and packs what is kept
        // (yacrd_engine_edit_overlaps; from the parser's mirror when it is the file the detection just read).  Whatever that
        // path does not take — compressed, quoted, CRs, a line of another shape — comes back with nothing written and takes
        // the host loop below, which knows the whole syntax and the messages.  YACRD_NO_DEVICE_EDITOR=1: the host loop (A/B).
        int dev_edit = YACRD_EFALLBACK;
        const char *no_ed = std::getenv("YACRD_NO_DEVICE_EDITOR");
        const char *no_df = std::getenv("YACRD_NO_DEVICE_DEFLATE");
        const bool sub_ovl = has(sub_in, ".m4") || has(sub_in, ".mhap") || has(sub_in, ".paf");
        const bool dev_ed = sub_ovl && (op == YACRD_OP_FILTER || op == YACRD_OP_EXTRACT) && !(no_ed && *no_ed == '1');
        // YACRD_EDIT_WINDOW=<bytes>: the overlap editor's window (yacrd_debug_edit_window; A/B and tests, like YACRD_SEQ_WINDOW below)
        if (const char *ew = std::getenv("YACRD_EDIT_WINDOW"))
            if (dev_ed && *ew) (void)yacrd_debug_edit_window(engines[0], std::strtoull(ew, nullptr, 10));
        // (how the last overlap edit ran: its windows, 0 for the whole text at once — the info lines end in it)
        auto edit_windows_of = [](const yacrd_engine *en) {
            uint64_t w4[4] = {0, 0, 0, 0};
            yacrd_debug_edit_windows(en, w4);
            return w4[0];
        };
        // ... and on a gzip one (what minimap2 | gzip leaves): the inflated text goes to HBM — the detection's, when it read this
        // very file and still holds it, else inflated here, BGZF member-parallel — and the kept bytes are deflated where the
        // device packs them: only BGZF members come back (yacrd_engine_edit_overlaps_gzip_file).  What it does not take, no
        // memory for it, YACRD_NO_DEVICE_EDITOR=1 or YACRD_NO_DEVICE_DEFLATE=1: the host loop into the gzip writer below.
        // With the device inflate on (one engine; see the route decision above for the default), a BGZF file is not inflated on
        // the host at all.  The detection's own file: its text lies inflated in HBM behind yacrd_engine_ingest_overlaps_bgzf_mem,
        // and yacrd_engine_edit_overlaps_resident_file edits it there.  Another BGZF file: mapped and offered to
        // yacrd_engine_edit_overlaps_bgzf_file, which inflates it in HBM as it lands.  YACRD_EFALLBACK or no memory from either
        // (plain gzip above all) leaves nothing behind and takes the route below, unchanged: inflate on the host, then
        // yacrd_engine_edit_overlaps_gzip_file, then the host loop.
        if (dev_ed && !(no_df && *no_df == '1') && yacrd_file_compression(sub_in.c_str()) == 1) {
            const yacrd_type_table tt = {bp.n_reads, bp.name_off, bp.names, bp.read_type};
            const int sub_fmt_ovl = has(sub_in, ".m4") || has(sub_in, ".mhap") ? 2 : 1;
            yacrd_edit_stats es{};
            yacrd_gzip_stats gs{};
            // what a device call handed back: no memory is a fallback too, behind a trim; any other error ends the run
            auto settled = [&](int rc, const char *to) {
                if (rc == YACRD_ENOMEM) {
                    std::fprintf(stderr, "[INFO] device editor + deflate: %s; falling back to %s\n", yacrd_last_error(), to);
                    for (yacrd_engine *en : engines) (void)yacrd_engine_trim(en);
                    rc = YACRD_EFALLBACK;
                }
                if (rc != YACRD_OK && rc != YACRD_EFALLBACK) die(yacrd_last_error());
                return rc;
            };
            // (on stdout: a stderr line that begins "[info] device editor" is the plain editor's — what reads the timing
            // output tells the two paths apart by it — and no sub-command writes data to stdout)
            auto report = [&](double inflate_ms, bool text_reused, bool resident, bool dev_inflate) {
                if (!timing) return;
                std::fprintf(stdout, "[info] device editor + deflate: %llu of %llu lines kept, %llu of %llu bytes -> %llu bytes, %llu members "
                                     "(%llu stored), inflate %.1f ms, text %.1f ms, table %.1f ms, editor kernels %.1f ms, encoder kernels %.1f ms, "
                                     "out %.1f ms, text_reused=%d resident=%d device_inflate=%d windows=%llu\n",
                             (unsigned long long)es.n_kept, (unsigned long long)es.n_lines, (unsigned long long)es.kept_bytes,
                             (unsigned long long)es.text_bytes, (unsigned long long)gs.out_bytes, (unsigned long long)gs.n_members,
                             (unsigned long long)gs.n_stored, inflate_ms, es.text_ms, es.table_ms, es.kernel_ms, gs.kernel_ms, es.out_ms,
                             text_reused ? 1 : 0, resident ? 1 : 0, dev_inflate ? 1 : 0, (unsigned long long)edit_windows_of(engines[0]));
            };
            // done on the device, nothing inflated on the host: the text the ingest left in HBM, or another BGZF file as it is
            if (ovl_resident && sub_same_file) {
                dev_edit = settled(yacrd_engine_edit_overlaps_resident_file(engines[0], op, &tt, 1, sub_out.c_str(), &es, &gs), "the host inflate");
                if (dev_edit == YACRD_OK) report(0.0, true, true, true);
            } else if (inflate_on && !sub_same_file) {
                GzipMap gm;
                yacrd_gunzip_stats us{};
                if (gm.open(sub_in.c_str())) {
                    dev_edit = settled(yacrd_engine_edit_overlaps_bgzf_file(engines[0], op, gm.data(), gm.n, sub_fmt_ovl, &tt, 1, sub_out.c_str(), &es, &gs, &us),
                                       "the host inflate");
                    if (dev_edit == YACRD_OK && timing) print_device_inflate(us);
                    if (dev_edit == YACRD_OK) report(0.0, false, false, true);
                }
            }
            // else the route of before: the detection's host text, or the file inflated here
            if (dev_edit != YACRD_OK) {
                const auto t_in = std::chrono::steady_clock::now();
                yacrd_text own{};
                const yacrd_text *tx = nullptr;
                if (text.data && sub_same_file) tx = &text;
                else {
                    const int rct = yacrd_text_from_file(sub_in.c_str(), threads == 1 ? 0 : (int)threads, &own);
                    if (rct == 1) die(yacrd_host_last_error());
                    if (rct == 0) tx = &own;
                }
                const double inflate_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_in).count();
                if (tx) {
                    dev_edit = settled(yacrd_engine_edit_overlaps_gzip_file(engines[0], op, tx->data, tx->n, sub_fmt_ovl, &tt, sub_out.c_str(), &es, &gs),
                                       "the host loop");
                    if (dev_edit == YACRD_OK) report(tx == &text ? 0.0 : inflate_ms, tx == &text, false, false);
                }
                yacrd_text_free(&own);
            }
        } else if (dev_ed) {
            const yacrd_type_table tt = {bp.n_reads, bp.name_off, bp.names, bp.read_type};
            yacrd_edit_stats es{};
            const char *ct = std::getenv("YACRD_COPY_THREADS");
            dev_edit = yacrd_engine_edit_overlaps(engines[0], op, sub_in.c_str(), sub_out.c_str(), 0, ct && *ct ? std::max(0, std::atoi(ct)) : 0,
                                                  &tt, &es);
            if (dev_edit == YACRD_ENOMEM) {
                std::fprintf(stderr, "[INFO] device editor: %s; falling back to the host loop\n", yacrd_last_error());
                for (yacrd_engine *en : engines) (void)yacrd_engine_trim(en);
                dev_edit = YACRD_EFALLBACK;
            }
            if (dev_edit != YACRD_OK && dev_edit != YACRD_EFALLBACK) die(yacrd_last_error());
            if (dev_edit == YACRD_OK && timing)
                std::fprintf(stderr, "[info] device editor: %llu of %llu lines kept, %llu of %llu bytes, text %.1f ms, table %.1f ms, kernels %.1f ms, "
                                     "out %.1f ms, mirror_reused=%u windows=%llu\n",
                             (unsigned long long)es.n_kept, (unsigned long long)es.n_lines, (unsigned long long)es.kept_bytes,
                             (unsigned long long)es.text_bytes, es.text_ms, es.table_ms, es.kernel_ms, es.out_ms, es.mirror_reused,
                             (unsigned long long)edit_windows_of(engines[0]));
        }
        // All four sub-commands on a FASTQ: the text goes to HBM, the device cuts it into records, decides, sizes and gathers the
        // output (yacrd_engine_edit_fastq).  A gzip FASTQ is inflated here — BGZF member-parallel; the detection's text when it
        // read this very file — and the output is deflated where the device gathers it: only BGZF members come back
        // (yacrd_engine_edit_fastq_gzip_file).  Whatever that path does not take — anything but canonical four-line records, a
        // cut position beyond its read — comes back with nothing written and takes the host loop below, which owns the syntax
        // and the messages.  bzip2 / xz, YACRD_NO_DEVICE_EDITOR=1 (and, for gzip, YACRD_NO_DEVICE_DEFLATE=1): the host.
        // A FASTA — what the host calls one by its name — goes the same way through yacrd_engine_edit_fasta[_gzip_file]: records
        // of any number of lines, written again 80 bases a line.
        const bool sub_seq = !sub_ovl && !has(sub_in, ".yacrd") && !(no_ed && *no_ed == '1');
        const bool sub_fq = sub_seq && (has(sub_in, ".fastq") || has(sub_in, ".fq"));
        const bool sub_fa = sub_seq && !sub_fq && (has(sub_in, ".fasta") || has(sub_in, ".fa"));
        const char *sub_fmt = sub_fa ? "fasta" : "fastq";
        const int sub_comp = sub_fq || sub_fa ? yacrd_file_compression(sub_in.c_str()) : -1;
        if ((sub_fq || sub_fa) && (sub_comp == 0 || (sub_comp == 1 && !(no_df && *no_df == '1')))) {
            const yacrd_report_table rt = {bp.n_reads, bp.name_off, bp.names, bp.lengths, bp.bad_offsets, bp.bad_regions, bp.read_type};
            yacrd_seq_edit_stats ss{};
            yacrd_gzip_stats gs{};
            yacrd_gunzip_stats us{};
            yacrd_gunzip_stream_stats zs{};
            double inflate_ms = 0;
            bool text_reused = false, dev_inflate = false, dev_gunzip = false;
            // YACRD_SEQ_WINDOW=<bytes>: the FASTQ and FASTA editors' window (yacrd_debug_seq_window; A/B and tests, like YACRD_NO_DEVICE_EDITOR)
            if (const char *sw = std::getenv("YACRD_SEQ_WINDOW"))
                if (*sw) (void)yacrd_debug_seq_window(engines[0], std::strtoull(sw, nullptr, 10));
            if (sub_comp == 1) {
                const auto t_in = std::chrono::steady_clock::now();
                yacrd_text own{};
                const yacrd_text *tx = nullptr;
                struct stat sa, sb;
                if (text.data && ::stat(input.c_str(), &sa) == 0 && ::stat(sub_in.c_str(), &sb) == 0 && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino)
                    tx = &text, text_reused = true;
                // A BGZF file the detection does not already hold inflated is mapped as it is and inflated on the device
                // (yacrd_engine_edit_fastq_bgzf_file: the call itself tells BGZF from plain gzip): no host inflate, and the text
                // crosses the link compressed.  Any other return than OK — plain gzip, a member the device decoder does not take,
                // a text the editor hands back, no memory — leaves nothing behind and takes the path below, unchanged.
                // The default, by DESIGN §7h's rows: the slowest `edit` of three with it is under the fastest of three without, on
                // scrubb and filter, FASTQ and FASTA.  YACRD_NO_DEVICE_INFLATE=1: the path below outright.
                // What that call hands back as YACRD_EFALLBACK goes, with YACRD_DEVICE_GUNZIP=1, to the plain-gzip form over the
                // same bytes (yacrd_engine_edit_fastq_gz_file: one gzip member decoded from block starts found in parallel,
                // DESIGN §7q), and only then below.  Opt-in: §7q's rows meet §7h's rule for the default; the switch is a change of its own.
                // A file whose first member is BGZF is the route's above alone: it is not sent up a second time.
                const char *no_inf = std::getenv("YACRD_NO_DEVICE_INFLATE"), *yes_gz = std::getenv("YACRD_DEVICE_GUNZIP");
                if (!tx && !(no_inf && *no_inf == '1')) {
                    const int fd = ::open(sub_in.c_str(), O_RDONLY);
                    struct stat sf;
                    if (fd >= 0 && ::fstat(fd, &sf) == 0 && S_ISREG(sf.st_mode) && sf.st_size > 0) {
                        void *m = ::mmap(nullptr, (size_t)sf.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
                        if (m != MAP_FAILED) {
                            dev_edit = (sub_fa ? yacrd_engine_edit_fasta_bgzf_file : yacrd_engine_edit_fastq_bgzf_file)(
                                engines[0], op, static_cast<const char *>(m), (uint64_t)sf.st_size, &rt, sub_out.c_str(), &ss, &gs, &us);
                            dev_inflate = dev_edit == YACRD_OK;
                            if (dev_edit == YACRD_EFALLBACK && yes_gz && *yes_gz == '1' &&
                                !first_member_is_bgzf(static_cast<const unsigned char *>(m), (size_t)sf.st_size)) {
                                dev_edit = (sub_fa ? yacrd_engine_edit_fasta_gz_file : yacrd_engine_edit_fastq_gz_file)(
                                    engines[0], op, static_cast<const char *>(m), (uint64_t)sf.st_size, &rt, sub_out.c_str(), &ss, &gs, &zs);
                                dev_gunzip = dev_edit == YACRD_OK;
                            }
                            ::munmap(m, (size_t)sf.st_size);
                            if (dev_edit == YACRD_ENOMEM)
                                for (yacrd_engine *en : engines) (void)yacrd_engine_trim(en);
                            if (!dev_inflate && !dev_gunzip) dev_edit = YACRD_EFALLBACK;
                        }
                    }
                    if (fd >= 0) ::close(fd);
                }
                if (!dev_inflate && !dev_gunzip) {
                    if (!tx && yacrd_text_from_file(sub_in.c_str(), threads == 1 ? 0 : (int)threads, &own) == 0)
                        tx = &own; // (a file that cannot be inflated: the host loop below words the error)
                    inflate_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_in).count();
                    if (tx) dev_edit = (sub_fa ? yacrd_engine_edit_fasta_gzip_file : yacrd_engine_edit_fastq_gzip_file)(engines[0], op, tx->data, tx->n, &rt, sub_out.c_str(), &ss, &gs);
                }
                yacrd_text_free(&own);
            } else {
                const char *ct = std::getenv("YACRD_COPY_THREADS");
                dev_edit = (sub_fa ? yacrd_engine_edit_fasta : yacrd_engine_edit_fastq)(engines[0], op, sub_in.c_str(), sub_out.c_str(), ct && *ct ? std::max(0, std::atoi(ct)) : 0, &rt, &ss);
            }
            if (dev_edit == YACRD_ENOMEM) {
                std::fprintf(stderr, "[INFO] device %s editor: %s; falling back to the host loop\n", sub_fmt, yacrd_last_error());
                for (yacrd_engine *en : engines) (void)yacrd_engine_trim(en);
                dev_edit = YACRD_EFALLBACK;
            }
            if (dev_edit != YACRD_OK && dev_edit != YACRD_EFALLBACK) die(yacrd_last_error());
            if (dev_edit == YACRD_OK && timing) {
                uint64_t sw4[4] = {0, 0, 0, 0}; // (how the edit ran: its windows, 0 for the whole text at once)
                yacrd_debug_seq_windows(engines[0], sw4);
                std::fprintf(stderr, "[info] device %s editor: %llu records -> %llu, %llu bytes -> %llu bytes, text %.1f ms, table %.1f ms, "
                                     "kernels %.1f ms, out %.1f ms, windows=%llu\n",
                             sub_fmt, (unsigned long long)ss.n_records, (unsigned long long)ss.n_out_records, (unsigned long long)ss.text_bytes,
                             (unsigned long long)ss.out_bytes, ss.text_ms, ss.table_ms, ss.kernel_ms, ss.out_ms, (unsigned long long)sw4[0]);
                if (dev_inflate)
                    print_device_inflate(us);
                if (dev_gunzip) print_device_gunzip(zs);
                if (sub_comp == 1) // (the encoder's line as the host loop's writer words it: the output lay in HBM, nothing went up)
                    std::fprintf(stderr, "[info] device deflate: %llu -> %llu bytes, %llu members (%llu stored), h2d %.1f ms, kernels %.1f ms, "
                                         "d2h %.1f ms, write %.1f ms, inflate %.1f ms, text_reused=%d\n",
                                 (unsigned long long)gs.in_bytes, (unsigned long long)gs.out_bytes, (unsigned long long)gs.n_members,
                                 (unsigned long long)gs.n_stored, gs.h2d_ms, gs.kernel_ms, gs.d2h_ms, gs.write_ms, text_reused ? 0.0 : inflate_ms,
                                 text_reused ? 1 : 0);
            }
        }
        // A gzip input writes gzip (the reference's contract): the host loop inflates and edits as before, and the edited bytes
        // leave through a yacrd_gzip_writer — compressed on the device into BGZF — instead of zlib's one thread.  No memory for
        // it, bzip2 / xz, YACRD_NO_DEVICE_DEFLATE=1: the host path below, unchanged.
        if (dev_edit != YACRD_OK && !(no_df && *no_df == '1') && yacrd_file_compression(sub_in.c_str()) == 1) {
            yacrd_gzip_writer *gw = nullptr;
            const int rco = yacrd_gzip_writer_open(engines[0], sub_out.c_str(), 0, 0, &gw);
            if (rco == YACRD_ENOMEM) {
                std::fprintf(stderr, "[INFO] device deflate: %s; falling back to zlib\n", yacrd_last_error());
                for (yacrd_engine *en : engines) (void)yacrd_engine_trim(en);
            } else if (rco != YACRD_OK) die(yacrd_last_error());
            else {
                yacrd_byte_sink sink{};
                (void)yacrd_gzip_writer_sink(gw, &sink);
                if (yacrd_edit_file_to(op, sub_in.c_str(), &bp, 0, &sink)) {
                    const std::string why = yacrd_host_last_error(), why_dev = yacrd_last_error();
                    yacrd_gzip_writer_abort(gw);
                    die((why_dev.empty() || why != "Error during writing of the output file" ? why : why_dev).c_str());
                }
                yacrd_gzip_stats gs{};
                if (yacrd_gzip_writer_close(gw, &gs) != YACRD_OK) die(yacrd_last_error());
                if (timing)
                    std::fprintf(stderr, "[info] device deflate: %llu -> %llu bytes, %llu members (%llu stored), h2d %.1f ms, kernels %.1f ms, "
                                         "d2h %.1f ms, write %.1f ms\n",
                                 (unsigned long long)gs.in_bytes, (unsigned long long)gs.out_bytes, (unsigned long long)gs.n_members,
                                 (unsigned long long)gs.n_stored, gs.h2d_ms, gs.kernel_ms, gs.d2h_ms, gs.write_ms);
                dev_edit = YACRD_OK;
            }
        }
        if (dev_edit != YACRD_OK && yacrd_edit_file(op, sub_in.c_str(), sub_out.c_str(), &bp)) die(yacrd_host_last_error());
        stage("edit");
    }

    yacrd_result_free(&res);
    yacrd_reads_free(&dev_reads);
    yacrd_text_free(&text);
    if (csr) yacrd_csr_free(csr);
    if (rep) yacrd_report_free(rep);
    for (yacrd_engine *e : engines) yacrd_engine_destroy(e);
    return 0;
}
