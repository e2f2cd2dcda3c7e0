// gpu_paf.hip — PAF text -> read types with the PARSE on the GPU (include/yacrd_engine.h:
// yacrd_engine_ingest_paf).
//
// Reference: Reads2Ovl::init_paf (src/reads2ovl/mod.rs:83-113; one csv record = one PafRecord,
// src/io.rs:23-34: nine leading tab-separated columns, the rest ignored) feeding
// FullMemory::add_overlap_and_length (src/reads2ovl/fullmemory.rs:82-90: a read's length is the first one
// seen; reads are numbered by first appearance here, the reference's order is a hash map's).
//
// The host parser (host/paf_csr.cc) is bound by its id table: two hash lookups per line, cache misses the CPUs
// cannot hide (133 M overlaps/s on 16 CPUs).  Here the host only MOVES the text: threads pread fixed chunks of
// the file into pinned buffers, every chunk crosses PCIe at once (hipMemcpyAsync) into a mirror of the file in
// HBM; the calling thread hands every 128 MiB of landed text to the scan + parse kernels (the engine's stream waits
// for the chunks' copy events, the host for nothing).  On the device:
//   scan     newlines counted (the number of records to expect), '"' / lone CR looked for
//   parse    32 KiB of text staged in LDS per workgroup; a thread takes the lines that START in its 128 bytes: nine
//            fields checked as the host's fast path checks them, both ids hashed and looked up in an open-addressing table whose slots name the text
//            position of the id's FIRST CLAIMANT (an id is compared against the text itself: no copies), the
//            smallest position of every id kept with atomicMin; one 24-byte overlap record per line
//   number   occupied slots sorted by first position (radix_sort.h) = first-appearance numbering; the
//            length that follows the id at that position = the read's length; names gathered for the host
//   build    csr_build.h's count / scan / scatter on the records, then the engine's launch sequence
// Whatever the fast path does not take — a quote, a lone CR, a 0x integer, a malformed line, a length beyond
// u32 — makes the call return YACRD_EFALLBACK: the caller runs the host parser, which knows the csv crate's
// whole syntax and the error messages.  Plain files only (the codecs live in the host library).
#include "engine_internal.h"
#include "gpu_text.h"
#include "radix_sort.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>


using namespace yke;

namespace yk {

struct GpArgs {
    const unsigned char *text;
    u64 n;              // bytes
    u64 *claim;         // [cap]: 0 = empty, else text position of the id that claimed the slot + 1
    u64 *first_pos;     // [cap]: smallest (byte offset * 2 + side) at which the slot's id was seen
    u32 *slot_cnt;      // [cap]: intervals of the slot's id (one per record side): the CSR build's count pass, done here
    u32 mask;           // cap - 1
    OvlRec *recs;
    u64 rec_cap;
    unsigned long long *n_recs;
    u32 *status;        // bit 0: the text needs the host parser; bit 1: the id table is full
    unsigned long long *n_lines; // newline-terminated lines + an unterminated last one
    // the part of the text one launch works on (the parse runs segment by segment while later chunks still cross PCIe)
    u64 begin, end;     // scan: bytes [begin, end); parse: the tiles from begin / kGpTile on (its grid = their number)
    u64 avail;          // bytes [0, avail) of the mirror have landed (== n for the last segment)
    u32 delim;          // the field delimiter: '\t' (PAF) or ' ' (M4: src/reads2ovl/mod.rs:116-117)
    u32 partial;        // the mirror ends in front of the file's end (a range + its overhang): a record that reaches the mirror's end is not whole
    u32 skip_head;      // the mirror is a byte RANGE of the file and the byte in front of it is no newline: position 0 lies
                        // inside a line that belongs to the range before (yacrd_engines_ingest_overlaps)
};

constexpr u32 kNeedHost = 1u, kTableFull = 2u;

// ---- pass 1: how many lines, and is there anything the fast path must not see ------------------------------
__global__ __launch_bounds__(kGpT) void gp_scan_kernel(GpArgs a)
{
    const u64 stride = (u64)gridDim.x * kGpT * 16u;
    u32 lines = 0, special = 0;
    for (u64 base = a.begin + ((u64)blockIdx.x * kGpT + threadIdx.x) * 16u; base < a.end; base += stride) {
        // 16 bytes per thread and step (segments begin on chunk boundaries; the mirror is padded: reads beyond n see
        // zeros, reads beyond an inner segment's end see the next chunk, which has landed)
        const uint4 v = *reinterpret_cast<const uint4 *>(a.text + base);
        const u32 w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const u64 i = base + (u64)k;
            const u32 c = (w[k >> 2] >> ((k & 3) * 8)) & 0xFFu;
            if (i < a.end) {
                lines += c == '\n' ? 1u : 0u;
                special |= c == '"' ? 1u : 0u;
                if (c == '\r') { // fine only as the first half of CRLF
                    const u32 nx = i + 1 < a.n ? a.text[i + 1] : 0u;
                    special |= nx != '\n' ? 1u : 0u;
                }
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) lines += (u32)__shfl_xor((int)lines, d, 64);
    special = wave_or(special);
    if (lane_id() == 0) {
        if (lines) atomicAdd(a.n_lines, (unsigned long long)lines);
        if (special) atomicOr(a.status, kNeedHost);
    }
    if (a.end == a.n && blockIdx.x == 0 && threadIdx.x == 0 && a.n && a.text[a.n - 1] != '\n') atomicAdd(a.n_lines, 1ull);
}

// ---- pass 2: parse ---------------------------------------------------------------------------------------------
// A workgroup stages 32 KiB of text (+ 1 KiB beyond it) in LDS with coalesced 16-byte loads; a thread then takes
// the lines that START in its 128 bytes and reads their first nine fields byte by byte from LDS (byte loads from
// global memory, one cache line per lane and instruction, ran this kernel at 24 GB/s).  A record needs nothing
// behind its ninth field, so a line of any length costs its start only; fields that reach beyond the staged
// window (ids of hundreds of bytes) are read from global memory.
constexpr int kGpOver = 1024; // (kGpTile, GpText and gp_hash: gpu_text.h)
// decimal u64 with an optional '+', at least one digit, then the delimiter (or, for the last field, the line's end);
// clears `ok` when the field is anything else.  `le` = the text's end: a line ends at '\n' (or "\r\n").
__device__ __forceinline__ u64 gp_uint(const GpText &t, u64 &q, u64 n, u64 limit, bool last, bool &ok, u32 dl)
{
    u64 i = q;
    u32 c = i < n ? t[i] : '\n';
    if (c == '+') {
        i++;
        c = i < n ? t[i] : '\n';
    }
    const u64 b = i;
    u64 v = 0;
    bool good = true;
    while (c - '0' <= 9u) {
        const u32 d = c - '0';
        good = good && v <= (0xFFFFFFFFFFFFFFFFull - d) / 10u;
        v = v * 10u + d;
        i++;
        c = i < n ? t[i] : '\n';
    }
    good = good && i != b && v <= limit;
    if (c == dl) {
        i++;
    } else { // the line's end: '\n', or '\r' in front of one (a lone CR never gets here: the scan refused it)
        good = good && last && (c == '\n' || c == '\r');
    }
    q = i;
    ok = ok && good;
    return v;
}
// the slot of the id at text position p (n bytes, hash h): claimed for it if it is new.  ~0u = table full.
__device__ __forceinline__ u32 gp_intern(const GpArgs &a, const GpText &t, u64 p, u32 n, u64 h)
{
    const unsigned char *g = a.text;
    u32 s = (u32)h & a.mask;
    // (a bounded walk: a table that is nearly full — more distinct ids than it was sized for, e.g. a read-to-reference
    // PAF with a new query id on every line — would otherwise cost every later lookup a walk over all of it before
    // the file is handed to the host parser anyway)
    const u32 max_probes = min(a.mask, 1024u);
    for (u32 probes = 0; probes <= max_probes; probes++, s = (s + 1u) & a.mask) {
        u64 w = __hip_atomic_load(&a.claim[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (w == 0) {
            const u64 old = atomicCAS((unsigned long long *)&a.claim[s], 0ull, (unsigned long long)(p + 1));
            if (old == 0) return s;
            w = old;
        }
        const u64 c = w - 1; // the claimant's id starts there and ends at a delimiter (or it would not have been parsed)
        if (c == p) return s;
        bool same = c + n < a.avail && g[c + n] == a.delim; // (a shorter id near the end of what has landed: not this one)
        for (u32 i = 0; same && i < n; i++) same = g[c + i] == t[p + i];
        if (same) return s;
    }
    return ~0u;
}

// M4 = false: PafRecord (src/io.rs:23-34: a la sa ea strand b lb sb eb ...); true: M4Record (src/io.rs:36-50:
// a b error shared strand_a sa ea la strand_b sb eb lb ...), space-separated.
template <bool M4>
__global__ __launch_bounds__(kGpT) void gp_parse_kernel(GpArgs a)
{
    const u32 dl = a.delim;
    __shared__ __attribute__((aligned(16))) unsigned char win[kGpTile + kGpOver];
    const u64 tile0 = a.begin + (u64)blockIdx.x * (u64)kGpTile; // (a.begin is a multiple of the tile size)
    if (tile0 >= a.n) return;
    // Bytes at and beyond `n` are not looked at: the text's end for the last segment, what has landed so far for the
    // others (their lines end long before it; one that does not is the host parser's: flagged below).
    const u64 n = a.avail;
    {
        // the window, 16 bytes per thread and step (the mirror is padded by 64 zero bytes and the last step is clipped
        // to whole 16-byte pieces inside it; an inner segment's `avail` is a chunk boundary)
        const u64 lim = a.avail == a.n ? ((a.n + 63) & ~(u64)15) : a.avail;
        const u64 want = min((u64)(kGpTile + kGpOver), lim - tile0);
        for (u64 i = (u64)threadIdx.x * 16u; i < want; i += (u64)kGpT * 16u)
            *reinterpret_cast<uint4 *>(win + i) = *reinterpret_cast<const uint4 *>(a.text + tile0 + i);
    }
    __syncthreads();
    GpText t;
    t.lds = win;
    t.glob = a.text;
    t.t0 = tile0;
    t.t1 = min(n, tile0 + (u64)(kGpTile + kGpOver));
    const u64 lo = tile0 + (u64)threadIdx.x * 128u;
    if (lo >= n) return;
    const u64 hi = min(n, lo + 128u);
    u32 status = 0;
    // lines that start in [lo, hi): position 0, or the byte after a newline
    u64 p = lo;
    if (lo != 0) {
        u64 q = lo - 1;
        while (q < hi && (q < tile0 ? (u32)a.text[q] : t[q]) != '\n') q++;
        p = q + 1; // (>= hi when no line starts here)
    } else if (a.skip_head) { // (a range that begins inside a line: that line is the previous range's)
        u64 q = 0;
        while (q < hi && t[q] != '\n') q++;
        p = q + 1;
    }
    while (p < hi) {
        // the line's first byte decides: empty lines are skipped (csv), "\r\n" alone is one as well
        const u32 c0 = t[p];
        u64 next = p; // where to look for the next line start: filled in below
        bool ok = false;
        u64 la = 0, lb = 0, sa = 0, ea = 0, sb = 0, eb = 0, ia = p, ib = p;
        u32 na = 0, nb = 0;
        if (c0 == '\n') { // an empty line: the next one starts right behind it
            p = p + 1;
            continue;
        } else if (c0 == '\r' && p + 1 < n && t[p + 1] == '\n') {
            p = p + 2;
            continue;
        } else {
            ok = true;
            u64 q = p;
            // an id: up to the delimiter (an id that runs into the line's end makes the record too short)
            auto take_id = [&](u64 &start, u32 &len) {
                start = q;
                u32 c = q < n ? t[q] : '\n';
                while (c != dl && c != '\n') {
                    q++;
                    c = q < n ? t[q] : '\n';
                }
                ok = ok && c == dl;
                len = (u32)(q - start);
                q++;
            };
            // a strand: exactly one UTF-8 scalar (serde char), judged by its lead byte like the host
            auto take_char = [&]() {
                u64 tb = q;
                u32 c = tb < n ? t[tb] : '\n';
                const u32 lead = c;
                while (c != dl && c != '\n') {
                    tb++;
                    c = tb < n ? t[tb] : '\n';
                }
                const u32 want = lead < 0x80u ? 1u : (lead >> 5) == 6u ? 2u : (lead >> 4) == 14u ? 3u : (lead >> 3) == 30u ? 4u : 0u;
                ok = ok && c == dl && want != 0u && tb - q == (u64)want;
                q = tb + 1;
            };
            // M4's error rate: the plain decimal forms only — [+-] digits [. digits] [e [+-] digits] with a digit on
            // both sides of the point — whatever else Rust's f64::from_str takes (inf, nan, ".5", "1.") is the host's
            auto take_f64 = [&]() {
                u32 c = q < n ? t[q] : '\n';
                auto step = [&]() {
                    q++;
                    c = q < n ? t[q] : '\n';
                };
                auto digits = [&]() {
                    u32 k = 0;
                    while (c - '0' <= 9u) {
                        k++;
                        step();
                    }
                    return k;
                };
                if (c == '+' || c == '-') step();
                bool good = digits() != 0u;
                if (c == '.') {
                    step();
                    good = good && digits() != 0u;
                }
                if (c == 'e' || c == 'E') {
                    step();
                    if (c == '+' || c == '-') step();
                    good = good && digits() != 0u;
                }
                ok = ok && good && c == dl;
                q++;
            };
            if constexpr (!M4) {
                take_id(ia, na);
                la = gp_uint(t, q, n, ~0ull, false, ok, dl);
                sa = gp_uint(t, q, n, 0xFFFFFFFFull, false, ok, dl);
                ea = gp_uint(t, q, n, 0xFFFFFFFFull, false, ok, dl);
                if (ok) take_char();
                if (ok) take_id(ib, nb);
                lb = gp_uint(t, q, n, ~0ull, false, ok, dl);
                sb = gp_uint(t, q, n, 0xFFFFFFFFull, false, ok, dl);
                eb = gp_uint(t, q, n, 0xFFFFFFFFull, true, ok, dl);
            } else {
                take_id(ia, na);
                if (ok) take_id(ib, nb);
                if (ok) take_f64();
                (void)gp_uint(t, q, n, ~0ull, false, ok, dl); // _shared_min: u64
                if (ok) take_char();
                sa = gp_uint(t, q, n, 0xFFFFFFFFull, false, ok, dl);
                ea = gp_uint(t, q, n, 0xFFFFFFFFull, false, ok, dl);
                la = gp_uint(t, q, n, ~0ull, false, ok, dl);
                if (ok) take_char();
                sb = gp_uint(t, q, n, 0xFFFFFFFFull, false, ok, dl);
                eb = gp_uint(t, q, n, 0xFFFFFFFFull, false, ok, dl);
                lb = gp_uint(t, q, n, ~0ull, true, ok, dl);
            }
            ok = ok && la <= 0xFFFFFFFFull && lb <= 0xFFFFFFFFull; // (the engine's limit; the host parser says so)
            if (!ok) status |= kNeedHost;
            if (q >= n && (n < a.n || a.partial)) status |= kNeedHost; // (a record that reaches into text still on its way, or beyond a range's overhang: megabytes long)
            next = q; // the rest of the line holds nothing for the record: its newline is looked for below
        }
        u32 s1 = 0, s2 = 0;
        if (ok) {
            s1 = gp_intern(a, t, ia, na, gp_hash(t, ia, na));
            s2 = gp_intern(a, t, ib, nb, gp_hash(t, ib, nb));
            if (s1 == ~0u || s2 == ~0u) {
                status |= kTableFull;
                ok = false;
            }
        }
        // One slot per record, handed out per wavefront: the lanes that have a record now ask together.
        const u64 m = __builtin_amdgcn_ballot_w64(ok);
        if (ok) {
            const u32 leader = (u32)__builtin_ctzll(m);
            u64 base = 0;
            if (lane_id() == leader) base = atomicAdd(a.n_recs, (unsigned long long)__builtin_popcountll(m));
            base = ((u64)(u32)__builtin_amdgcn_readlane((int)(u32)(base >> 32), (int)leader) << 32) |
                   (u32)__builtin_amdgcn_readlane((int)(u32)base, (int)leader);
            const u64 at = base + (u64)__builtin_popcountll(m & ((1ull << lane_id()) - 1ull));
            const u64 pa = p * 2u, pb = p * 2u + 1u;
            if (pa < __hip_atomic_load(&a.first_pos[s1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                atomicMin((unsigned long long *)&a.first_pos[s1], (unsigned long long)pa);
            if (pb < __hip_atomic_load(&a.first_pos[s2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                atomicMin((unsigned long long *)&a.first_pos[s2], (unsigned long long)pb);
            if (s1 == s2) {
                atomicAdd(&a.slot_cnt[s1], 2u);
            } else {
                atomicAdd(&a.slot_cnt[s1], 1u);
                atomicAdd(&a.slot_cnt[s2], 1u);
            }
            if (at < a.rec_cap) {
                OvlRec r;
                r.a = s1, r.b = s2, r.sa = (u32)sa, r.ea = (u32)ea, r.sb = (u32)sb, r.eb = (u32)eb;
                a.recs[at] = r;
            }
        }
        // the next line start inside this thread's bytes, if any
        while (next < hi && t[next] != '\n') next++;
        p = next + 1;
        if (next >= hi) break;
    }
    if (status) atomicOr(a.status, status);
}

// ---- pass 3: the reads -------------------------------------------------------------------------------------------
// A workgroup walks its share of the table, gathers the occupied slots in LDS and asks for room in the output once
// per kCollectBuf of them: the table is 0.5-5 % full, and one returning atomic per wavefront that meets an occupied
// slot (600 k of them for 600 k reads, performed one after the other at the memory side: ~8 ns each) made this
// kernel 5.9 ms of a 110 ms call.  (The order of the output does not matter: it is sorted next.)
constexpr u32 kCollectBuf = 1024;
__global__ __launch_bounds__(256) void gp_collect_kernel(const u64 *claim, const u64 *first_pos, u32 cap, u64 *keys,
                                                         u32 *slots, u32 *n_out)
{
    __shared__ u64 s_key[kCollectBuf + 256];
    __shared__ u32 s_slot[kCollectBuf + 256];
    __shared__ u32 s_n, s_base;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const u64 per = ((u64)cap + gridDim.x - 1) / gridDim.x;
    const u64 lo = (u64)blockIdx.x * per, hi = min((u64)cap, lo + per);
    auto flush = [&]() { // (every thread of the workgroup)
        __syncthreads();
        const u32 n = s_n;
        if (threadIdx.x == 0 && n) s_base = atomicAdd(n_out, n);
        __syncthreads();
        for (u32 i = threadIdx.x; i < n; i += 256u) {
            keys[s_base + i] = s_key[i];
            slots[s_base + i] = s_slot[i];
        }
        __syncthreads();
        if (threadIdx.x == 0) s_n = 0;
        __syncthreads();
    };
    for (u64 s0 = lo; s0 < hi; s0 += 256u) { // (uniform trip count)
        const u64 s = s0 + threadIdx.x;
        const bool used = s < hi && claim[s] != 0;
        const u64 m = __builtin_amdgcn_ballot_w64(used);
        if (m) {
            u32 base = 0;
            if (lane_id() == (u32)__builtin_ctzll(m)) base = atomicAdd(&s_n, (u32)__builtin_popcountll(m));
            base = (u32)__builtin_amdgcn_readlane((int)base, (int)__builtin_ctzll(m));
            if (used) {
                const u32 at = base + (u32)__builtin_popcountll(m & ((1ull << lane_id()) - 1ull));
                s_key[at] = first_pos[s];
                s_slot[at] = (u32)s;
            }
        }
        __syncthreads();
        if (s_n >= kCollectBuf) flush(); // (uniform: s_n is read behind a barrier)
    }
    flush();
}
// read g (first-appearance order) = the id first seen at keys[g]: its slot -> g, its length (PAF: the field after
// the id; M4: the 8th / 12th field of the line), the extent of its name, its number of intervals
__global__ __launch_bounds__(256) void gp_number_kernel(const unsigned char *t, const u64 *keys, const u32 *slots,
                                                        u32 n_reads, u32 *handle_map, u32 *lengths, u32 *name_len,
                                                        u64 *name_at, const u32 *slot_cnt, u32 *cnt, u32 delim)
{
    const u32 g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_reads) return;
    handle_map[slots[g]] = g;
    cnt[g] = slot_cnt[slots[g]];
    const u64 pos = keys[g];
    const bool m4 = delim == ' ', second = (pos & 1u) != 0;
    const int id_field = m4 ? (second ? 1 : 0) : (second ? 5 : 0), len_field = m4 ? (second ? 11 : 7) : (second ? 6 : 1);
    u64 q = pos >> 1; // the line's start
    for (int f = 0; f < id_field; f++) {
        while (t[q] != delim) q++;
        q++;
    }
    const u64 id0 = q;
    while (t[q] != delim) q++;
    name_at[g] = id0;
    name_len[g] = (u32)(q - id0);
    q++;
    for (int f = id_field + 1; f < len_field; f++) {
        while (t[q] != delim) q++;
        q++;
    }
    if (t[q] == '+') q++;
    u64 v = 0;
    while ((u32)t[q] - '0' <= 9u) v = v * 10u + ((u32)t[q++] - '0');
    lengths[g] = (u32)v; // (checked <= u32 by the parse)
}
__global__ __launch_bounds__(256) void gp_names_kernel(const unsigned char *t, const u64 *name_at, const u64 *name_off,
                                                       u32 n_reads, unsigned char *names)
{
    const u32 g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_reads) return;
    const u64 from = name_at[g], to = name_off[g], n = name_off[g + 1] - to;
    for (u64 i = 0; i < n; i++) names[to + i] = t[from + i];
}


// ==== several engines, one file: the reads of the engines' byte ranges merged (yacrd_engines_ingest_overlaps) ============
// Every engine has parsed a byte range of the text (parse_range) and numbered the reads IT saw.  The same read shows up in
// many ranges; the merge engine gets every range's read list — name, first position in the file, first length, number of
// intervals: a few dozen bytes per read and range, against the gigabytes of text that never leave their device — and
// interns the names once more, in a table whose slots name list ENTRIES.  Then, as for one engine: occupied slots
// sorted by first position = first-appearance numbering over the whole file; a read's length is the one seen at that
// position (src/reads2ovl/fullmemory.rs:82-90).  Every entry learns its read's number, every engine rewrites its records
// from table slots to those numbers, and the reads are dealt out to the engines as contiguous ranges of numbers.
struct GmArgs {
    const unsigned char *names; // every range's names, end to end
    const u64 *noff;            // [M + 1] entry -> its name's extent in `names`
    const u64 *fp;              // [M] first position in the FILE * 2 + side
    const u32 *len, *cnt;       // [M] the length seen there; intervals of the read inside the range
    u64 M;
    u64 *claim, *first_pos;     // [cap]: entry + 1 of the slot's first claimant; smallest first position
    u32 *slot_cnt;              // [cap]
    u32 mask;
    u32 *entry_slot;            // [M]
    u32 *status;
};
__global__ __launch_bounds__(256) void gm_shift_kernel(u64 *fp, u64 *noff, u64 n, u64 fp_add, u64 noff_add)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i < n) fp[i] += fp_add, noff[i] += noff_add;
}
__global__ __launch_bounds__(256) void gm_intern_kernel(GmArgs a)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= a.M) return;
    const u64 p = a.noff[i];
    const u32 n = (u32)(a.noff[i + 1] - p);
    u64 h = 0xcbf29ce484222325ull ^ ((u64)n * 0x9E3779B97F4A7C15ull);
    for (u32 k = 0; k < n; k++) h = (h ^ a.names[p + k]) * 0x100000001b3ull;
    h ^= h >> 29;
    h *= 0xbf58476d1ce4e5b9ull;
    h ^= h >> 32;
    u32 s = (u32)h & a.mask, found = ~0u;
    for (u32 probes = 0; probes <= a.mask; probes++, s = (s + 1u) & a.mask) {
        u64 w = __hip_atomic_load(&a.claim[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (w == 0) {
            const u64 old = atomicCAS((unsigned long long *)&a.claim[s], 0ull, (unsigned long long)(i + 1));
            if (old == 0) {
                found = s;
                break;
            }
            w = old;
        }
        const u64 c = w - 1, q = a.noff[c];
        bool same = (u32)(a.noff[c + 1] - q) == n;
        for (u32 k = 0; same && k < n; k++) same = a.names[q + k] == a.names[p + k];
        if (same) {
            found = s;
            break;
        }
    }
    if (found == ~0u) { // (cannot happen: the table has twice as many slots as there are entries)
        atomicOr(a.status, kTableFull);
        return;
    }
    a.entry_slot[i] = found;
    atomicMin((unsigned long long *)&a.first_pos[found], (unsigned long long)a.fp[i]);
    atomicAdd(&a.slot_cnt[found], a.cnt[i]);
}
// read g of the whole file = the name first seen at keys[g]: its slot -> g, its intervals, where its name lies
__global__ __launch_bounds__(256) void gm_number_kernel(GmArgs a, const u32 *slots, u32 n_reads, u32 *slot_read, u32 *cnt,
                                                        u32 *name_len, u64 *name_at)
{
    const u32 g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_reads) return;
    const u32 s = slots[g];
    slot_read[s] = g;
    cnt[g] = a.slot_cnt[s];
    const u64 c = a.claim[s] - 1;
    name_at[g] = a.noff[c];
    name_len[g] = (u32)(a.noff[c + 1] - a.noff[c]);
}
// every entry: its read's number; the entry that saw the read first gives it its length
__global__ __launch_bounds__(256) void gm_entry_kernel(GmArgs a, const u32 *slot_read, u32 *entry_read, u32 *lengths)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= a.M) return;
    const u32 s = a.entry_slot[i], g = slot_read[s];
    entry_read[i] = g;
    if (a.fp[i] == a.first_pos[s]) lengths[g] = a.len[i];
}
// on every engine: table slot -> the range's read -> the file's read; then the records' handles
__global__ __launch_bounds__(256) void gm_slot_read_kernel(u32 *slot_map, u64 cap, const u32 *range_read_to_file)
{
    const u64 s = (u64)blockIdx.x * 256u + threadIdx.x;
    if (s >= cap) return;
    const u32 l = slot_map[s];
    if (l != 0xFFFFFFFFu) slot_map[s] = range_read_to_file[l];
}
__global__ __launch_bounds__(256) void gm_rewrite_kernel(OvlRec *recs, u64 n, const u32 *slot_map)
{
    for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < n; i += (u64)gridDim.x * 256u) {
        uint2 *ab = reinterpret_cast<uint2 *>(recs + i);
        const uint2 v = *ab;
        *ab = make_uint2(slot_map[v.x], slot_map[v.y]);
    }
}
// the reads [lo, hi) are this engine's (numbered from 0 here), every other one lives elsewhere
__global__ __launch_bounds__(256) void gm_own_kernel(u32 *own, u32 n_reads, u32 lo, u32 hi)
{
    const u32 g = blockIdx.x * 256u + threadIdx.x;
    if (g < n_reads) own[g] = (g >= lo && g < hi) ? g - lo : (u32)YACRD_HANDLE_ELSEWHERE;
}

} // namespace yk

namespace {


// (first position, slot) pairs by first position, on the engine's stream: radix_sort.h, as many eight-bit passes as keys
// below `key_bound` need.  The passes go back and forth between the two pairs of arrays (the inputs are scratch: clobbered);
// an odd number of them, so that the last one lands in the outputs.
int sort_by_first_position(yacrd_engine *e, u64 *keys, u64 *keys_out, u32 *slots, u32 *slots_out, u32 n, u64 key_bound, DevBuf &tmp,
                           DevBuf &part)
{
    int bits = 1;
    while (bits < 64 && (key_bound >> bits) != 0) bits++;
    int passes = (bits + 7) / 8;
    passes |= 1;
    const u32 tiles = (u32)(((u64)n + yk::kRsTile - 1) / yk::kRsTile);
    const size_t cells = (size_t)256 * tiles;
    const size_t first_at = (cells * sizeof(u32) + 255) & ~(size_t)255;
    HIP_TRY(tmp.reserve(first_at + (cells + 1) * sizeof(u64) + 64));
    u32 *hist = tmp.as<u32>();
    u64 *first = reinterpret_cast<u64 *>(tmp.as<char>() + first_at);
    u64 *ka = keys, *kb = keys_out;
    u32 *va = slots, *vb = slots_out;
    for (int p = 0; p < passes; p++) {
        const u32 shift = (u32)std::min(8 * p, 56); // (a pass beyond the key's bits sees digit 0 everywhere: a stable copy)
        const bool beyond = 8 * p >= 64;
        hipLaunchKernelGGL(yk::rs_hist_kernel, dim3(tiles), dim3(yk::kRsThreads), 0, e->stream, ka, (u64)n, beyond ? 63u : shift, tiles, hist);
        if (const int rcs = scan_u32_to_u64(e, hist, (u64)cells, first, part)) return rcs;
        hipLaunchKernelGGL(yk::rs_scatter_kernel, dim3(tiles), dim3(yk::kRsThreads), 0, e->stream, ka, va, (u64)n, beyond ? 63u : shift, tiles,
                           first, kb, vb);
        std::swap(ka, kb);
        std::swap(va, vb);
    }
    return YACRD_OK;
}

// the 64-byte control block the kernels count into: lines, records, status bits, number of reads
struct Ctl {
    DevBuf buf;
    struct Words { // a copy on the host (status and n_reads are 32-bit on the device: the upper halves stay zero)
        unsigned long long lines = 0, records = 0, status = 0, n_reads = 0;
    };
    unsigned long long *lines() const { return buf.as<unsigned long long>(); }
    unsigned long long *records() const { return lines() + 1; }
    u32 *status() const { return reinterpret_cast<u32 *>(lines() + 2); }
    u32 *n_reads() const { return reinterpret_cast<u32 *>(lines() + 3); }
    // what the kernels on the engine's stream have counted (the stream is waited for)
    int read(yacrd_engine *e, Words &h, bool last_error = true) const
    {
        HIP_TRY(hipMemcpyAsync(&h, buf.p, sizeof(h), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (last_error) HIP_TRY(hipGetLastError());
        return YACRD_OK;
    }
};

// the open-addressing id table (GpArgs / GmArgs say what a slot holds)
struct IdTable {
    DevBuf claim, first_pos, slot_cnt;
    u64 cap = 0;
    int reserve(u64 slots)
    {
        HIP_TRY(claim.reserve((size_t)slots * sizeof(u64)));
        HIP_TRY(first_pos.reserve((size_t)slots * sizeof(u64)));
        HIP_TRY(slot_cnt.reserve((size_t)slots * sizeof(u32)));
        cap = slots;
        return YACRD_OK;
    }
    // an empty table, and the control words its kernels count into at zero
    int reset(hipStream_t stream, const Ctl &ctl)
    {
        HIP_TRY(hipMemsetAsync(ctl.buf.p, 0, 64, stream));
        HIP_TRY(hipMemsetAsync(claim.p, 0, (size_t)cap * sizeof(u64), stream));
        HIP_TRY(hipMemsetAsync(first_pos.p, 0xFF, (size_t)cap * sizeof(u64), stream));
        HIP_TRY(hipMemsetAsync(slot_cnt.p, 0, (size_t)cap * sizeof(u32), stream));
        return YACRD_OK;
    }
};

// one numbering of reads by first appearance: a table's occupied slots (keys = first positions), the same sorted, and per
// read where its name lies (length, position in the text it is taken from, offsets in `names`) and its intervals
struct ReadList {
    DevBuf keys, keys2, slots, slots2, name_len, name_at, name_off, names, cnt;
    // (the kernels read a few elements beyond the last read's)
    int reserve_reads(u32 n_reads)
    {
        HIP_TRY(name_len.reserve((size_t)(n_reads + 4) * sizeof(u32)));
        HIP_TRY(name_at.reserve((size_t)(n_reads + 1) * sizeof(u64)));
        HIP_TRY(name_off.reserve((size_t)(n_reads + 2) * sizeof(u64)));
        HIP_TRY(cnt.reserve((size_t)(n_reads + 4) * sizeof(u32)));
        return YACRD_OK;
    }
};

struct Scratch { // the call's device buffers; they stay with the engine (grow-only), the whole object goes with yacrd_engine_trim / destroy
    static constexpr yacrd_engine::Slot kScratchSlot = yacrd_engine::kPaf;
    Ctl ctl;
    IdTable ids;    // the range's
    ReadList range; // the range's reads: lengths in e->in_len
    DevBuf text, recs, tmp, map, part, err, gather, gmap;
    // the merge engine's (yacrd_engines_ingest_overlaps): every range's reads end to end (m_*), the file's table and reads
    IdTable file_ids;
    ReadList file; // lengths in g_len
    DevBuf m_fp, m_len, m_cnt, m_noff, m_names, m_slot, m_read, g_slot_read, g_len;

    // What every numbering shares (a range's in parse_range, the file's in GroupRun::merge); the caller's checks come behind
    // collect, its number kernel behind sort_collected.
    // table -> list.keys / slots: the occupied slots and their first positions; `h`: the control words, h.n_reads slots
    int collect(yacrd_engine *e, IdTable &t, ReadList &l, Ctl::Words &h)
    {
        HIP_TRY(l.keys.reserve((size_t)t.cap * sizeof(u64) + 64));
        HIP_TRY(l.slots.reserve((size_t)t.cap * sizeof(u32) + 64));
        hipLaunchKernelGGL(yk::gp_collect_kernel, dim3((u32)std::min<u64>((t.cap + 255) / 256, (u64)e->num_cu * 8)), dim3(256), 0, e->stream,
                           t.claim.as<u64>(), t.first_pos.as<u64>(), (u32)t.cap, l.keys.as<u64>(), l.slots.as<u32>(), ctl.n_reads());
        return ctl.read(e, h, false);
    }
    // -> list.keys2 / slots2: the same by first position (keys below key_bound)
    int sort_collected(yacrd_engine *e, ReadList &l, u32 n_reads, u64 key_bound)
    {
        HIP_TRY(l.keys2.reserve((size_t)n_reads * sizeof(u64) + 64));
        HIP_TRY(l.slots2.reserve((size_t)n_reads * sizeof(u32) + 64));
        if (!n_reads) return YACRD_OK;
        return sort_by_first_position(e, l.keys.as<u64>(), l.keys2.as<u64>(), l.slots.as<u32>(), l.slots2.as<u32>(), n_reads, key_bound, tmp, part);
    }
    // list.name_len / name_at (the number kernel's) -> list.name_off, and list.names gathered from `text`
    int pack_names(yacrd_engine *e, const unsigned char *text, ReadList &l, u32 n_reads, u64 *name_bytes)
    {
        if (const int rcs = scan_u32_to_u64(e, l.name_len.as<u32>(), (u64)n_reads, l.name_off.as<u64>(), part)) return rcs;
        HIP_TRY(hipMemcpyAsync(name_bytes, l.name_off.as<u64>() + n_reads, sizeof(u64), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(l.names.reserve((size_t)*name_bytes + 64));
        if (n_reads)
            hipLaunchKernelGGL(yk::gp_names_kernel, dim3((n_reads + 255) / 256), dim3(256), 0, e->stream, text, l.name_at.as<u64>(),
                               l.name_off.as<u64>(), n_reads, l.names.as<unsigned char>());
        return YACRD_OK;
    }
};


} // namespace

extern "C" {

void yacrd_reads_free(yacrd_reads *r)
{
    if (!r) return;
    std::free(r->lengths);
    std::free(r->name_off);
    std::free(r->names);
    std::memset(r, 0, sizeof(*r));
}

int yacrd_engine_ingest_paf(yacrd_engine *e, const char *path, int n_threads, uint32_t coverage, double not_coverage,
                            yacrd_result *out, yacrd_reads *reads, yacrd_ingest_stats *stats)
{
    return yacrd_engine_ingest_overlaps(e, path, 1, n_threads, coverage, not_coverage, out, reads, stats);
}

} // extern "C"

namespace {

// Bytes [begin, begin + len) of the text -> on the engine: the overlap records of the lines that START there (handles = id-table
// slots), the table S.ids, and the range's reads numbered by first appearance INSIDE the range: S.map (slot -> read) and, in
// S.range, keys2 (first positions * 2 + side, relative to `begin`), cnt (intervals), name_off / names; e->in_len (lengths).  The whole file for
// one engine; a range per engine for several (yacrd_engines_ingest_overlaps), cut on chunk boundaries.
struct RangeOut {
    u64 n_recs = 0, cap = 0, name_bytes = 0;
    u32 R = 0;
    double t_start = 0, t_text = 0, t_parse = 0;
};
int parse_range(yacrd_engine *e, TextProducer &tp, u64 file_n, u64 begin, u64 len, bool skip_head, bool m4, int n_threads, RangeOut &ro)
{
    const TextSource &src = tp.src;
    if (tp.bgzf && (begin || len != file_n)) return fail(YACRD_EINTERNAL, "device parser: a BGZF text is parsed whole");
    // (no text on the host to take the line density from: the first members, at most 1 MiB of text, are decoded here — 13 ms
    // on one thread, beside the allocations below)
    struct HeadSample {
        std::thread th;
        u64 text = 0, lines = 0;
        bool ok = false;
        ~HeadSample()
        {
            if (th.joinable()) th.join();
        }
    } head_sample;
    if (tp.bgzf)
        head_sample.th = std::thread([&head_sample, bz = tp.bgzf] {
            head_sample.ok = bgzf_head_lines(reinterpret_cast<const unsigned char *>(bz->comp), bz->comp_bytes, bz->members.data(), bz->members.size(),
                                             (u64)1 << 20, &head_sample.text, &head_sample.lines);
        });
    DeviceGuard guard(e->device);
    Scratch *Sp = scratch_of<Scratch>(e);
    if (!Sp) return fail(YACRD_ENOMEM, "host allocation failed");
    Scratch &S = *Sp;
    e->mirror.valid = false; // (the mirror is about to be rewritten)
    e->resident.valid = e->input.valid = false;
    // the mirror holds the range and, behind it, up to one chunk more of the file: a line that starts in the range ends there
    // (or the parse says so: kNeedHost)
    constexpr u64 kOverhang = (u64)4 << 20;
    const u64 n = std::min<u64>(file_n, begin + len + (begin + len < file_n ? kOverhang : 0)) - begin; // bytes in the mirror
    const u64 parse_end = len; // lines that start at or behind it are the next range's
    ro.t_start = now_ms();
    {
        // The parse on the device wants the text, a 24-byte record per line, the id table, the CSR and the region
        // slots in HBM at once: ~2.6 x the file (measured: 37.2 GB of text -> 96 GB).  An input beyond that goes to
        // the host parser, whose streamed records need ~0.5 x: answered here, before anything is allocated.
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
            // (a BGZF stream: its compressed bytes and the member table lie in HBM beside the text)
            const double have = (double)free_b + (double)S.text.cap + (double)S.recs.cap + (double)e->stage.cap +
                                (double)e->in_iv.cap + (double)S.gather.cap + (tp.bgzf ? (double)inflate_device_held(e) : 0.0);
            if (2.6 * (double)n + (tp.bgzf ? tp.bgzf->device_bytes() : 0.0) + (double)((size_t)256 << 20) > have)
                return fail(YACRD_EFALLBACK, "the file is too large to be parsed in this device's free memory: the host parser streams it");
        }
    }

    // ---- what does not depend on the text's content: the mirror, the id table, the control words
    const void *mirror_before = S.text.p;
    HIP_TRY(S.text.reserve((size_t)n + 64));
    // Fresh HBM is slow to fill, whoever fills it: the text of a 37 GB file takes 0.70 s to get into a mirror that
    // is being reused and 2.2-2.4 s (hipMemcpyAsync; 5.1 s in a process's first call) or 0.85-2.4 s (copy kernels;
    // 2.1 s in a first call) into one that was allocated for this call — same box, same run, profiles/r03_e2e_large.log.
    // So the buffers stay with the engine (yacrd_engine_trim gives them back), chunks go by copy kernel into a fresh
    // mirror and by hipMemcpyAsync, 15 % faster once the memory is warm, into a reused one.
    const bool blit = S.text.p != mirror_before;
    HIP_TRY(hipMemsetAsync(S.text.as<char>() + n, 0, 64, e->stream)); // (the scan reads 16 bytes at a time)
    u64 cap = (u64)1 << 20;
    while (cap < n / 64 && cap < ((u64)1 << 31)) cap <<= 1; // ids are a small fraction of the lines; a full table = fallback
    if (const int rct = S.ids.reserve(cap)) return rct;
    HIP_TRY(S.ctl.buf.reserve(64));
    if (const int rct = S.ids.reset(e->stream, S.ctl)) return rct;
    // Room for the records: the number of lines is only known when the last byte has been scanned, and the parse
    // does not wait for that — so from the line density of the file's first MiB plus a quarter (never more than
    // one record per 17 bytes); a parse that outgrows it is repeated with the exact number below.
    u64 rec_cap = n / 17 + 2;
    if (tp.bgzf) { // (a member that is not taken, or no line in the sample: the bound)
        head_sample.th.join();
        if (head_sample.ok && head_sample.lines)
            rec_cap = std::min<u64>(rec_cap, (u64)((double)n / (double)head_sample.text * (double)head_sample.lines * 1.25) + 4096);
    } else {
        const size_t sample = (size_t)std::min<u64>(n, (u64)1 << 20);
        std::vector<char> head(sample + 1);
        if (!src.fetch(head.data(), sample, begin)) return fail(YACRD_EINVAL, "read error in the overlap file");
        u64 nl = 0;
        for (const char *q = head.data(), *end = q + sample; (q = (const char *)std::memchr(q, '\n', (size_t)(end - q))) != nullptr; q++) nl++;
        if (nl) rec_cap = std::min<u64>(rec_cap, (u64)((double)n / (double)sample * (double)nl * 1.25) + 4096);
    }
    HIP_TRY(S.recs.reserve((size_t)rec_cap * sizeof(yk::OvlRec)));
    yk::GpArgs ga{};
    ga.text = S.text.as<unsigned char>();
    ga.n = n;
    ga.n_lines = S.ctl.lines();
    ga.n_recs = S.ctl.records();
    ga.status = S.ctl.status();
    ga.claim = S.ids.claim.as<u64>();
    ga.first_pos = S.ids.first_pos.as<u64>();
    ga.slot_cnt = S.ids.slot_cnt.as<u32>();
    ga.mask = (u32)(cap - 1);
    ga.recs = S.recs.as<yk::OvlRec>();
    ga.rec_cap = rec_cap;
    ga.delim = m4 ? (u32)' ' : (u32)'\t';
    ga.skip_head = skip_head ? 1u : 0u;
    ga.partial = begin + n < file_n ? 1u : 0u;
    if ((n + yk::kGpTile - 1) / yk::kGpTile >= 0x7FFFFFFFull) return fail(YACRD_EFALLBACK, "file too large for the device parser");
    // scan + parse of the bytes [begin, end) on the engine's stream (begin on a tile boundary)
    auto launch_segment = [&](u64 begin, u64 end, u64 avail) {
        ga.begin = begin, ga.end = end, ga.avail = avail;
        const u32 scan_grid = (u32)std::min<u64>(((end - begin) / (yk::kGpT * 16u)) + 1, (u64)e->num_cu * 16);
        hipLaunchKernelGGL(yk::gp_scan_kernel, dim3(scan_grid), dim3(yk::kGpT), 0, e->stream, ga);
        const u64 tiles = (end - begin + yk::kGpTile - 1) / yk::kGpTile;
        if (tiles && m4) hipLaunchKernelGGL(yk::gp_parse_kernel<true>, dim3((u32)tiles), dim3(yk::kGpT), 0, e->stream, ga);
        else if (tiles) hipLaunchKernelGGL(yk::gp_parse_kernel<false>, dim3((u32)tiles), dim3(yk::kGpT), 0, e->stream, ga);
    };

    // ---- the text: pread chunks -> pinned buffers -> HBM, all chunks in flight at once; THIS thread hands every
    // segment of kSeg chunks to the scan + parse kernels as soon as it (and the chunk behind it: a tile's overhang,
    // the byte after a CR) has landed — the engine's stream waits for the chunks' copy events, the host for nothing
    {
        // (128 MiB per scan + parse launch.  The two kernels take 0.9 ms for 367 MB, so what the overlap buys is small;
        // segments of 16 / 32 MiB got in the way of the copy threads: tools/paf_matrix.py, profiles/r03/paf_matrix.log)
        // (a BGZF stream: the segments are the inflated text's, each behind the launches that decoded it)
        int rc_open = YACRD_OK;
        const int bad = tp.move(e, begin, n, S.text.as<char>(), blit, n_threads, [&](u64 seg_begin, u64 seg_end, u64 avail) {
            if (seg_begin < parse_end) launch_segment(seg_begin, std::min<u64>(parse_end, seg_end), avail);
        }, &rc_open);
        if (rc_open) return rc_open;
        if (bad == 2) return fail(YACRD_EINVAL, "read error in the overlap file");
        if (bad == 3) return fail(YACRD_ENOMEM, "PAF text to HBM: no pinned memory");
        if (bad) return fail(YACRD_ENODEV, "PAF text to HBM: a HIP call failed");
    }
    ro.t_text = now_ms();

    // ---- what the scan and the parse found
    // (the inflate's status word first: a text decoded from a member that was not taken may say anything)
    Ctl::Words found;
    u32 inflate_status = 0;
    if (const int rci = tp.fetch_inflate_status(e, &inflate_status)) return rci;
    if (const int rcc = S.ctl.read(e, found)) return rcc;
    if (inflate_status) return inflate_not_taken(inflate_status);
    if ((u32)found.status & yk::kNeedHost)
        return fail(YACRD_EFALLBACK, "the text holds a '\"', a lone CR or a line that is not a plain PAF / M4 record (too few "
                                     "columns, a 0x integer, a length beyond u32, an error rate written as inf or .5 ...): the "
                                     "host parser decides");
    if ((u32)found.status & yk::kTableFull) return fail(YACRD_EFALLBACK, "more read ids than the device table holds");
    if (found.lines >= 0x7FFFFFFFull * 2) return fail(YACRD_EFALLBACK, "too many lines for the device parser");
    const u64 n_recs = found.records;
    if (n_recs > found.lines + 2) return fail(YACRD_EINTERNAL, "device parser: more records than lines");
    if (n_recs > rec_cap) { // the estimate fell short (line lengths far from uniform): once more, with room for every record
        rec_cap = n_recs + 1;
        HIP_TRY(S.recs.reserve((size_t)rec_cap * sizeof(yk::OvlRec)));
        ga.recs = S.recs.as<yk::OvlRec>();
        ga.rec_cap = rec_cap;
        if (const int rct = S.ids.reset(e->stream, S.ctl)) return rct;
        launch_segment(0, parse_end, n);
        if (const int rcc = S.ctl.read(e, found)) return rcc;
        if (((u32)found.status & (yk::kNeedHost | yk::kTableFull)) || found.records != n_recs)
            return fail(YACRD_EINTERNAL, "device parser: the second parse disagrees with the first");
    }
    // ---- the reads: occupied slots by first position, numbered, their names packed
    ReadList &L = S.range;
    if (const int rcc = S.collect(e, S.ids, L, found)) return rcc;
    const u32 R = ro.R = (u32)found.n_reads;
    ro.t_parse = now_ms();
    if ((u64)R * 2 > cap && R > 1024) return fail(YACRD_EFALLBACK, "more read ids than the device table holds comfortably");
    if (const int rcs = S.sort_collected(e, L, R, 2 * n + 2)) return rcs;
    HIP_TRY(S.map.reserve((size_t)cap * sizeof(u32)));
    if (const int rcr = L.reserve_reads(R)) return rcr;
    HIP_TRY(e->in_len.reserve((size_t)(R + 1) * sizeof(u32)));
    HIP_TRY(hipMemsetAsync(L.cnt.p, 0, (size_t)(R + 4) * sizeof(u32), e->stream));
    HIP_TRY(hipMemsetAsync(S.map.p, 0xFF, (size_t)cap * sizeof(u32), e->stream));
    if (R)
        hipLaunchKernelGGL(yk::gp_number_kernel, dim3((R + 255) / 256), dim3(256), 0, e->stream, ga.text, L.keys2.as<u64>(), L.slots2.as<u32>(),
                           R, S.map.as<u32>(), e->in_len.as<u32>(), L.name_len.as<u32>(), L.name_at.as<u64>(), S.ids.slot_cnt.as<u32>(), L.cnt.as<u32>(), ga.delim);
    ro.n_recs = n_recs, ro.cap = cap;
    return S.pack_names(e, ga.text, L, R, &ro.name_bytes);
}

int ingest_text(yacrd_engine *e, TextProducer tp, u64 n, bool m4, int n_threads, uint32_t coverage, double not_coverage,
                yacrd_result *out, yacrd_reads *reads, yacrd_ingest_stats *stats)
{
    DeviceGuard guard(e->device);
    RangeOut ro;
    if (const int rcp = parse_range(e, tp, n, 0, n, false, m4, n_threads, ro)) return rcp;
    Scratch &S = *scratch_of<Scratch>(e); // (parse_range made it)
    // the reads, to the host (while the CSR is built)
    if (const int rch = reads_to_host(e, reads, ro.R, ro.n_recs, e->in_len.p, S.range.name_off.p, S.range.names.p, ro.name_bytes)) return rch;
    // ---- CSR on the device (csr_build.h through stream.hip's helper), then the engine
    const RecSlab slab{S.recs.as<yk::OvlRec>(), ro.n_recs};
    u64 n_iv = 0; // (what the build's scan summed: two per record)
    int rc = csr_from_records(e, &slab, 1, S.map.as<u32>(), ro.cap, ro.R, S.range.cnt, S.part, S.err, nullptr, &n_iv, true);
    const double t_build = now_ms();
    if (!rc) rc = run_on_device(e, e->in_off.as<u64>(), e->in_iv.as<uint2>(), e->in_len.as<u32>(), ro.R, 2 * ro.n_recs, coverage, not_coverage);
    const double t_run = now_ms();
    const bool ran = rc == YACRD_OK;
    if (ran) rc = fetch_result(e, out);
    if (ran && stats) {
        stats->text_bytes = n;
        stats->n_records = ro.n_recs;
        stats->n_reads = ro.R;
        stats->text_ms = (float)(ro.t_text - ro.t_start);
        stats->parse_ms = (float)(ro.t_parse - ro.t_text);
        stats->build_ms = (float)(t_build - ro.t_parse);
        stats->run_ms = (float)(t_run - t_build);
        stats->d2h_ms = (float)(now_ms() - t_run);
    }
    if (rc) {
        yacrd_reads_free(reads);
        return rc;
    }
    // the table stays where it is: a report can be written from it (gpu_report_write.hip)
    e->resident.names = S.range.names.as<unsigned char>(), e->resident.name_off = S.range.name_off.as<u64>(), e->resident.lengths = e->in_len.as<u32>();
    e->resident.n_reads = ro.R, e->resident.valid = true;
    e->input.n_reads = ro.R, e->input.n_iv = n_iv, e->input.valid = true;
    return YACRD_OK;
}

} // namespace

// ---- several engines, one file --------------------------------------------------------------------------------------
namespace {
// ---- device memory of engine `from` -> device memory of engine `to`, on `to`'s stream ---------------------------------------
// (the source is complete: its stream was waited for; the caller's current device is `to`'s).  Three routes:
//   same device                   hipMemcpyAsync, device to device
//   two devices, peer access      hipMemcpyPeerAsync: xGMI carries it
//   two devices, no peer access   staged through two pinned host buffers: device -> host on `from`'s device, host -> device
//                                 on `to`'s stream (the runtime would do the same, one pageable piece at a time)
// Which of the last two a PAIR of devices takes is found once, when a group first uses the pair (hipDeviceCanAccessPeer +
// hipDeviceEnablePeerAccess in both directions; anything but success / "already enabled" = staged).  This builder has never
// seen two GPUs in one box (missing #2), so the routes can be FORCED on one device, where the tests run:
// YACRD_TEST_FORCE_PEER_COPY=peer sends every cross-engine copy through hipMemcpyPeerAsync (source device = destination
// device is legal), =staged through the host bounce; tests/test_gpu_ingest_group.py runs the group under both.
enum PeerRoute { kRouteSame = 0, kRoutePeer = 1, kRouteStaged = 2 };
int forced_peer_route()
{
    static const int v = [] {
        const char *ev = std::getenv("YACRD_TEST_FORCE_PEER_COPY");
        if (!ev || !*ev) return -1;
        if (!std::strcmp(ev, "peer") || !std::strcmp(ev, "1")) return (int)kRoutePeer;
        if (!std::strcmp(ev, "staged") || !std::strcmp(ev, "host")) return (int)kRouteStaged;
        return -1;
    }();
    return v;
}
std::mutex g_peer_mu;
signed char g_peer_route[64][64]; // 0: not looked at yet; else PeerRoute + 1
std::atomic<unsigned long long> g_peer_copies[3]; // copies per route (yacrd_debug_peer_copy_counts: the tests look)
PeerRoute route_between(int to_dev, int from_dev)
{
    const int forced = forced_peer_route();
    if (to_dev == from_dev) return forced >= 0 ? (PeerRoute)forced : kRouteSame;
    if (forced == (int)kRouteStaged) return kRouteStaged;
    if (to_dev < 0 || from_dev < 0 || to_dev >= 64 || from_dev >= 64) return kRouteStaged;
    std::lock_guard<std::mutex> lock(g_peer_mu);
    signed char &slot = g_peer_route[to_dev][from_dev];
    if (slot) return (PeerRoute)(slot - 1);
    PeerRoute r = kRouteStaged;
    int can_a = 0, can_b = 0;
    if (hipDeviceCanAccessPeer(&can_a, to_dev, from_dev) == hipSuccess && hipDeviceCanAccessPeer(&can_b, from_dev, to_dev) == hipSuccess &&
        can_a && can_b) {
        bool ok = true;
        for (int k = 0; k < 2 && ok; k++) { // both directions: the merge pulls towards engine 0, the deal pushes away from it
            const int self = k == 0 ? to_dev : from_dev, peer = k == 0 ? from_dev : to_dev;
            DeviceGuard guard(self);
            const hipError_t er = hipDeviceEnablePeerAccess(peer, 0);
            if (er != hipSuccess && er != hipErrorPeerAccessAlreadyEnabled) ok = false;
            (void)hipGetLastError(); // ("already enabled" is sticky otherwise)
        }
        if (ok) r = kRoutePeer;
    } else {
        (void)hipGetLastError();
    }
    slot = (signed char)(r + 1);
    g_peer_route[from_dev][to_dev] = slot;
    return r;
}
// the staged route: two pinned buffers per destination engine, a piece flies host -> device while the next one is fetched
struct StageBuf {
    PinBuf pin[2];
    Events ev; // one per buffer
    bool busy[2] = {false, false};
    Streams from; // one, on the source's device: made and destroyed with that device current
    int from_dev = -1;
    ~StageBuf()
    {
        if (from.v.empty()) return;
        DeviceGuard guard(from_dev);
        from.clear();
    }
};
constexpr size_t kStagePiece = (size_t)16 << 20;
hipError_t copy_staged(yacrd_engine *to, void *dst, yacrd_engine *from, const void *src, size_t bytes)
{
    StageBuf sb; // (per call: the route is a fallback, its setup cost is not what matters on it)
    for (int i = 0; i < 2; i++) {
        const hipError_t er = sb.pin[i].reserve(std::min(bytes, kStagePiece));
        if (er != hipSuccess) return er;
    }
    if (!sb.ev.add(2, hipEventDisableTiming)) return why_not_added();
    sb.from_dev = from->device;
    {
        DeviceGuard guard(from->device);
        if (!sb.from.add(1)) return why_not_added();
    }
    int turn = 0;
    for (size_t at = 0; at < bytes; at += kStagePiece, turn ^= 1) {
        const size_t m = std::min(kStagePiece, bytes - at);
        if (sb.busy[turn]) {
            const hipError_t er = hipEventSynchronize(sb.ev[turn]); // the buffer's last host -> device copy has left it
            if (er != hipSuccess) return er;
        }
        {
            DeviceGuard guard(from->device); // device -> host runs on the SOURCE device's stream
            hipError_t er = hipMemcpyAsync(sb.pin[turn].p, (const char *)src + at, m, hipMemcpyDeviceToHost, sb.from[0]);
            if (er == hipSuccess) er = hipStreamSynchronize(sb.from[0]);
            if (er != hipSuccess) return er;
        }
        hipError_t er = hipMemcpyAsync((char *)dst + at, sb.pin[turn].p, m, hipMemcpyHostToDevice, to->stream);
        if (er == hipSuccess) er = hipEventRecord(sb.ev[turn], to->stream);
        if (er != hipSuccess) return er;
        sb.busy[turn] = true;
    }
    return hipStreamSynchronize(to->stream); // (the pinned buffers go away with `sb`)
}
hipError_t copy_between(yacrd_engine *to, void *dst, yacrd_engine *from, const void *src, size_t bytes)
{
    if (!bytes) return hipSuccess;
    const PeerRoute r = route_between(to->device, from->device);
    g_peer_copies[(int)r]++;
    if (r == kRouteSame) return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, to->stream);
    if (r == kRoutePeer) return hipMemcpyPeerAsync(dst, to->device, src, from->device, bytes, to->stream);
    return copy_staged(to, dst, from, src, bytes);
}

// the engines' partial results; what is still held when the holder goes is freed
struct Parts {
    std::vector<yacrd_result> v;
    ~Parts() { for (auto &r : v) yacrd_result_free(&r); }
};

// One file over N engines (yacrd_engines_ingest_overlaps): what the phases share, and the phases in the order
// ingest_text_group calls them.
struct GroupRun {
    yacrd_engine *const *E;
    const uint32_t N;
    const u64 n;                        // bytes of text
    uint32_t A = 0;                     // engines that parse a range (every engine sweeps)
    std::vector<u64> B;                 // [N + 1] engine d parses the bytes [B[d], B[d + 1])
    std::vector<RangeOut> ro;           // [A] what parse_range left on every parsing engine
    std::vector<u64> eb, nb;            // [A + 1] where a range's reads / name bytes begin among all ranges', end to end
    u32 Rg = 0;                         // reads of the whole file
    std::vector<u32> h_rcnt, cut;       // [Rg] their intervals; [N + 1] engine o sweeps the reads [cut[o], cut[o + 1])
    Parts parts;                        // [N] what every engine's sweep found
    std::vector<double> t_built, t_ran; // [N]
    double t0 = 0, t_parsed = 0, t_merged = 0;
    Scratch &scratch(uint32_t d) const { return *scratch_of<Scratch>(E[d]); } // (there from cut_ranges on)

    // fn(d) on `count` host threads, one per engine; the first failure wins, a real error before "not for the device parser"
    template <class Fn>
    int run_all(uint32_t count, Fn &&fn)
    {
        std::vector<int> codes(count, YACRD_OK);
        std::vector<std::string> errs(count);
        std::vector<std::thread> th;
        for (uint32_t d = 1; d < count; d++)
            th.emplace_back([&, d] {
                codes[d] = fn(d);
                if (codes[d]) errs[d] = err_slot();
            });
        codes[0] = fn(0);
        if (codes[0]) errs[0] = err_slot();
        for (auto &t : th) t.join();
        for (uint32_t d = 0; d < count; d++)
            if (codes[d] && codes[d] != YACRD_EFALLBACK) return fail(codes[d], "engine " + std::to_string(d) + ": " + errs[d]);
        for (uint32_t d = 0; d < count; d++)
            if (codes[d]) return fail(codes[d], errs[d]);
        return (int)YACRD_OK;
    }

    // ---- byte ranges: whole 4 MiB chunks (the parse's segments begin on tile boundaries), the same number for every engine
    // (YACRD_TEST_RANGE_BYTES, tests: a smaller grain — a multiple of the parse's 32 KiB tiles — so that small texts are cut too)
    int cut_ranges()
    {
        static const u64 kChunk = [] {
            const char *ev = std::getenv("YACRD_TEST_RANGE_BYTES");
            const u64 v = ev ? std::strtoull(ev, nullptr, 10) : 0;
            return (v >= (u64)yk::kGpTile && v % (u64)yk::kGpTile == 0) ? v : ((u64)4 << 20);
        }();
        const u64 chunks = (n + kChunk - 1) / kChunk, per = (chunks + N - 1) / N;
        B = std::vector<u64>(N + 1);
        for (uint32_t d = 0; d <= N; d++) B[d] = std::min<u64>(n, (u64)d * per * kChunk);
        while (A < N && B[A] < B[A + 1]) A++;
        for (uint32_t d = 0; d < N; d++)
            if (!scratch_of<Scratch>(E[d])) return fail(YACRD_ENOMEM, "host allocation failed"); // (every later scratch_of finds it)
        return YACRD_OK;
    }

    // ---- does it fit?  Answered before anything is allocated or moved (parse_range's own check knows only
    // its range).  Per DEVICE: what its engines' ranges need for the parse (text, records, id table, CSR and region slots of
    // as many reads: ~2.6 x the range, parse_range) plus the records every one of its engines gathers from ranges parsed on
    // OTHER devices (24 bytes per line, ~0.32 x their text at 75 bytes a line; engines of one device read each other's
    // records in place).  An input beyond that is the host parser's (its stream group needs ~0.5 x the file over all GPUs).
    int fits()
    {
        std::vector<int> seen;
        for (uint32_t d = 0; d < N; d++) {
            const int dev = E[d]->device;
            if (std::find(seen.begin(), seen.end(), dev) != seen.end()) continue;
            seen.push_back(dev);
            double here = 0, held = 0;
            uint32_t engines_here = 0;
            for (uint32_t k = 0; k < N; k++)
                if (E[k]->device == dev) {
                    Scratch &Sk = scratch(k);
                    here += (double)(B[k + 1] - B[k]);
                    held += (double)Sk.text.cap + (double)Sk.recs.cap + (double)E[k]->stage.cap + (double)E[k]->in_iv.cap + (double)Sk.gather.cap;
                    engines_here++;
                }
            const double need = 2.6 * here + 0.32 * ((double)n - here) * engines_here + (double)((size_t)256 << 20) * engines_here;
            DeviceGuard guard(dev);
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > (double)free_b + held)
                return fail(YACRD_EFALLBACK, "the file is too large to be parsed in the GPUs' free memory (ranges + the records gathered "
                                             "from the other GPUs): the host parser streams it");
        }
        return YACRD_OK;
    }

    // ---- every parsing engine: its range (a range whose first byte continues a line leaves that line to the range before)
    int parse(const TextSource &src, bool m4, int n_threads)
    {
        std::vector<char> head_skip(A, 0);
        for (uint32_t d = 1; d < A; d++) {
            char c = 0;
            if (!src.fetch(&c, 1, B[d] - 1)) return fail(YACRD_EINVAL, "read error in the overlap file");
            head_skip[d] = c != '\n';
        }
        t0 = now_ms();
        ro = std::vector<RangeOut>(A);
        // the threads that move text are shared out (engines on one device share its link as well)
        const int copy_threads = std::max(1, (n_threads > 0 ? n_threads : 8) / (int)A);
        const int rc = run_all(A, [&](uint32_t d) -> int {
            TextProducer plain(src);
            const int r = parse_range(E[d], plain, n, B[d], B[d + 1] - B[d], head_skip[d] != 0, m4, copy_threads, ro[d]);
            if (r) return r;
            DeviceGuard guard(E[d]->device);
            HIP_TRY(hipStreamSynchronize(E[d]->stream)); // (the names kernel: other engines read what this one made)
            return YACRD_OK;
        });
        t_parsed = now_ms();
        return rc;
    }

    // ---- engine 0: the ranges' reads end to end (an entry each), interned by name into the file's table; the file's reads
    // numbered by first position; every entry's read; the reads to the host
    int merge(yacrd_reads *reads)
    {
        yacrd_engine *e0 = E[0];
        Scratch &S0 = scratch(0);
        ReadList &L = S0.file;
        eb = std::vector<u64>(A + 1, 0), nb = std::vector<u64>(A + 1, 0);
        for (uint32_t d = 0; d < A; d++) eb[d + 1] = eb[d] + ro[d].R, nb[d + 1] = nb[d] + ro[d].name_bytes;
        const u64 M = eb[A], NB = nb[A];
        if (M >= 0x7FFFFFFFull) return fail(YACRD_EFALLBACK, "too many read ids for the device parser");
        u64 capG = 1024;
        while (capG < 2 * M) capG <<= 1;
        DeviceGuard guard(e0->device);
        HIP_TRY(S0.m_fp.reserve((size_t)(M + 1) * sizeof(u64)));
        HIP_TRY(S0.m_len.reserve((size_t)(M + 1) * sizeof(u32)));
        HIP_TRY(S0.m_cnt.reserve((size_t)(M + 1) * sizeof(u32)));
        HIP_TRY(S0.m_noff.reserve((size_t)(M + 2) * sizeof(u64)));
        HIP_TRY(S0.m_names.reserve((size_t)NB + 64));
        HIP_TRY(S0.m_slot.reserve((size_t)(M + 1) * sizeof(u32)));
        HIP_TRY(S0.m_read.reserve((size_t)(M + 1) * sizeof(u32)));
        if (const int rct = S0.file_ids.reserve(capG)) return rct;
        HIP_TRY(S0.g_slot_read.reserve((size_t)capG * sizeof(u32)));
        HIP_TRY(S0.ctl.buf.reserve(64));
        for (uint32_t d = 0; d < A; d++) {
            Scratch &Sd = scratch(d);
            const size_t R = ro[d].R;
            HIP_TRY(copy_between(e0, S0.m_fp.as<u64>() + eb[d], E[d], Sd.range.keys2.p, R * sizeof(u64)));
            HIP_TRY(copy_between(e0, S0.m_len.as<u32>() + eb[d], E[d], E[d]->in_len.p, R * sizeof(u32)));
            HIP_TRY(copy_between(e0, S0.m_cnt.as<u32>() + eb[d], E[d], Sd.range.cnt.p, R * sizeof(u32)));
            HIP_TRY(copy_between(e0, S0.m_noff.as<u64>() + eb[d], E[d], Sd.range.name_off.p, R * sizeof(u64)));
            HIP_TRY(copy_between(e0, S0.m_names.as<char>() + nb[d], E[d], Sd.range.names.p, (size_t)ro[d].name_bytes));
            if (R)
                hipLaunchKernelGGL(yk::gm_shift_kernel, dim3((u32)((R + 255) / 256)), dim3(256), 0, e0->stream, S0.m_fp.as<u64>() + eb[d],
                                   S0.m_noff.as<u64>() + eb[d], (u64)R, 2 * B[d], nb[d]);
        }
        HIP_TRY(hipMemcpyAsync(S0.m_noff.as<u64>() + M, &NB, sizeof(u64), hipMemcpyHostToDevice, e0->stream));
        if (const int rct = S0.file_ids.reset(e0->stream, S0.ctl)) return rct;
        yk::GmArgs gm{};
        gm.names = S0.m_names.as<unsigned char>(), gm.noff = S0.m_noff.as<u64>(), gm.fp = S0.m_fp.as<u64>();
        gm.len = S0.m_len.as<u32>(), gm.cnt = S0.m_cnt.as<u32>(), gm.M = M;
        gm.claim = S0.file_ids.claim.as<u64>(), gm.first_pos = S0.file_ids.first_pos.as<u64>(), gm.slot_cnt = S0.file_ids.slot_cnt.as<u32>();
        gm.mask = (u32)(capG - 1);
        gm.entry_slot = S0.m_slot.as<u32>();
        gm.status = S0.ctl.status();
        const u32 mg = (u32)((M + 255) / 256);
        if (M) hipLaunchKernelGGL(yk::gm_intern_kernel, dim3(mg), dim3(256), 0, e0->stream, gm);
        Ctl::Words h;
        if (const int rcc = S0.collect(e0, S0.file_ids, L, h)) return rcc;
        HIP_TRY(hipGetLastError());
        if ((u32)h.status) return fail(YACRD_EINTERNAL, "device parser: the merge table overflowed");
        Rg = (u32)h.n_reads;
        if (const int rcs = S0.sort_collected(e0, L, Rg, 2 * n + 2)) return rcs;
        if (const int rcr = L.reserve_reads(Rg)) return rcr;
        HIP_TRY(S0.g_len.reserve((size_t)(Rg + 1) * sizeof(u32)));
        if (Rg) {
            hipLaunchKernelGGL(yk::gm_number_kernel, dim3((Rg + 255) / 256), dim3(256), 0, e0->stream, gm, L.slots2.as<u32>(), Rg,
                               S0.g_slot_read.as<u32>(), L.cnt.as<u32>(), L.name_len.as<u32>(), L.name_at.as<u64>());
            hipLaunchKernelGGL(yk::gm_entry_kernel, dim3(mg), dim3(256), 0, e0->stream, gm, S0.g_slot_read.as<u32>(), S0.m_read.as<u32>(),
                               S0.g_len.as<u32>());
        }
        u64 name_bytes = 0;
        if (const int rcn = S0.pack_names(e0, gm.names, L, Rg, &name_bytes)) return rcn;
        u64 n_records = 0;
        for (uint32_t d = 0; d < A; d++) n_records += ro[d].n_recs;
        if (const int rch = reads_to_host(e0, reads, Rg, n_records, S0.g_len.p, L.name_off.p, L.names.p, name_bytes)) return rch;
        h_rcnt.resize((size_t)Rg + 1);
        if (Rg) HIP_TRY(hipMemcpyAsync(h_rcnt.data(), L.cnt.p, (size_t)Rg * sizeof(u32), hipMemcpyDeviceToHost, e0->stream));
        HIP_TRY(hipStreamSynchronize(e0->stream));
        return YACRD_OK;
    }

    // ---- who sweeps what: contiguous ranges of read numbers with about the same number of intervals each (every engine,
    // also one that had no text to parse)
    void deal()
    {
        cut = std::vector<u32>(N + 1, Rg);
        u64 total = 0;
        for (u32 g = 0; g < Rg; g++) total += h_rcnt[g];
        u64 run = 0;
        uint32_t o = 1;
        cut[0] = 0;
        for (u32 g = 0; g < Rg && o < N; g++) {
            while (o < N && run >= (total * o + N - 1) / N) cut[o++] = g;
            run += h_rcnt[g];
        }
        // (cut[o..N] stay Rg: engines behind the last cut own nothing)
    }

    // ---- every parsing engine: its records from table slots to the file's read numbers
    int rewrite()
    {
        const int rc = run_all(A, [&](uint32_t d) -> int {
            yacrd_engine *e = E[d];
            DeviceGuard guard(e->device);
            Scratch &S = scratch(d);
            const size_t R = ro[d].R;
            HIP_TRY(S.gmap.reserve((size_t)(std::max<u64>(R, Rg) + 4) * sizeof(u32)));
            HIP_TRY(copy_between(e, S.gmap.p, E[0], scratch(0).m_read.as<u32>() + eb[d], R * sizeof(u32)));
            hipLaunchKernelGGL(yk::gm_slot_read_kernel, dim3((u32)((ro[d].cap + 255) / 256)), dim3(256), 0, e->stream, S.map.as<u32>(), ro[d].cap,
                               S.gmap.as<u32>());
            if (ro[d].n_recs)
                hipLaunchKernelGGL(yk::gm_rewrite_kernel, dim3((u32)std::min<u64>((ro[d].n_recs + 255) / 256, (u64)e->num_cu * 16)), dim3(256), 0,
                                   e->stream, S.recs.as<yk::OvlRec>(), ro[d].n_recs, S.map.as<u32>());
            HIP_TRY(hipStreamSynchronize(e->stream));
            HIP_TRY(hipGetLastError());
            return YACRD_OK;
        });
        t_merged = now_ms();
        return rc;
    }

    // ---- every engine: the records of ALL ranges (its own in place, the others' copied over when they live on another
    // device), the halves that name its reads kept (csr_build.h: YACRD_HANDLE_ELSEWHERE), CSR, sweep
    int build_and_sweep(uint32_t coverage, double not_coverage)
    {
        Scratch &S0 = scratch(0); // (the merge's: every read's length and intervals)
        parts.v = std::vector<yacrd_result>(N);
        t_built = std::vector<double>(N, 0), t_ran = std::vector<double>(N, 0);
        return run_all(N, [&](uint32_t o) -> int {
            yacrd_engine *e = E[o];
            DeviceGuard guard(e->device);
            Scratch &S = scratch(o);
            const u32 lo = cut[o], hi = cut[o + 1], Ro = hi - lo;
            std::vector<RecSlab> slabs(A);
            u64 foreign = 0;
            // (records parsed by an engine of THIS device are read where they lie; under YACRD_TEST_FORCE_PEER_COPY every other
            // engine counts as another device's, so that the gather and its copies run on a one-GPU box)
            auto elsewhere = [&](uint32_t d) { return E[d]->device != e->device || (forced_peer_route() >= 0 && E[d] != e); };
            for (uint32_t d = 0; d < A; d++)
                if (elsewhere(d)) foreign += ro[d].n_recs;
            HIP_TRY(S.gather.reserve((size_t)foreign * sizeof(yk::OvlRec) + 64));
            u64 at = 0;
            for (uint32_t d = 0; d < A; d++) {
                Scratch &Sd = scratch(d);
                if (!elsewhere(d)) {
                    slabs[d] = RecSlab{Sd.recs.as<yk::OvlRec>(), ro[d].n_recs};
                } else {
                    yk::OvlRec *dst = S.gather.as<yk::OvlRec>() + at;
                    HIP_TRY(copy_between(e, dst, E[d], Sd.recs.p, (size_t)ro[d].n_recs * sizeof(yk::OvlRec)));
                    slabs[d] = RecSlab{dst, ro[d].n_recs};
                    at += ro[d].n_recs;
                }
            }
            HIP_TRY(S.gmap.reserve((size_t)(Rg + 4) * sizeof(u32)));
            if (Rg) hipLaunchKernelGGL(yk::gm_own_kernel, dim3((Rg + 255) / 256), dim3(256), 0, e->stream, S.gmap.as<u32>(), Rg, lo, hi);
            HIP_TRY(e->in_len.reserve((size_t)(Ro + 1) * sizeof(u32)));
            HIP_TRY(copy_between(e, e->in_len.p, E[0], S0.g_len.as<u32>() + lo, (size_t)Ro * sizeof(u32)));
            // (the merge has summed every read's intervals over the ranges: the CSR build's count pass — one more pass over
            // every range's records on every engine — is not needed)
            HIP_TRY(S.range.cnt.reserve((size_t)(Ro + 4) * sizeof(u32)));
            HIP_TRY(copy_between(e, S.range.cnt.p, E[0], S0.file.cnt.as<u32>() + lo, (size_t)Ro * sizeof(u32)));
            u64 n_iv = 0, own_iv = 0; // (the engine's CSR holds the intervals of ITS reads: the merge has their counts)
            for (u32 g = lo; g < hi; g++) own_iv += h_rcnt[g];
            int r = csr_from_records(e, slabs.data(), slabs.size(), S.gmap.as<u32>(), Rg, Ro, S.range.cnt, S.part, S.err, nullptr, &n_iv, true,
                                     own_iv + 1);
            if (r) return r;
            t_built[o] = now_ms();
            r = run_on_device(e, e->in_off.as<u64>(), e->in_iv.as<uint2>(), e->in_len.as<u32>(), Ro, n_iv, coverage, not_coverage);
            if (r) return r;
            t_ran[o] = now_ms();
            r = fetch_result(e, &parts.v[o]);
            if (!r) e->input.n_reads = Ro, e->input.n_iv = n_iv, e->input.valid = true;
            return r;
        });
    }

    // ---- the results, end to end: the ranges are in first-appearance order already
    int stitch(yacrd_result *out)
    {
        Parts mine; // (they go when this returns)
        mine.v.swap(parts.v);
        u64 G = 0;
        for (auto &r : mine.v) G += r.n_regions;
        out->bad_offsets = (uint64_t *)std::malloc(((size_t)Rg + 1) * sizeof(uint64_t));
        out->bad_regions = (uint32_t *)std::malloc((size_t)(2 * G + 2) * sizeof(uint32_t));
        out->read_type = (uint8_t *)std::malloc((size_t)Rg + 1);
        if (!out->bad_offsets || !out->bad_regions || !out->read_type) {
            yacrd_result_free(out);
            return fail(YACRD_ENOMEM, "host allocation failed");
        }
        u64 g0 = 0;
        for (uint32_t o = 0; o < N; o++) {
            const yacrd_result &part = mine.v[o];
            const u32 lo = cut[o], Ro = cut[o + 1] - lo;
            if (part.n_reads != Ro) {
                yacrd_result_free(out);
                return fail(YACRD_EINTERNAL, "device parser: an engine returned another number of reads than it was given");
            }
            for (u32 l = 0; l < Ro; l++) out->bad_offsets[lo + l] = g0 + part.bad_offsets[l];
            if (part.n_regions) std::memcpy(out->bad_regions + 2 * g0, part.bad_regions, (size_t)part.n_regions * 2 * sizeof(uint32_t));
            if (Ro) std::memcpy(out->read_type + lo, part.read_type, Ro);
            g0 += part.n_regions;
        }
        out->bad_offsets[Rg] = g0;
        out->n_reads = Rg;
        out->n_regions = g0;
        return YACRD_OK;
    }

    void fill_stats(const yacrd_reads *reads, yacrd_ingest_stats *stats) const
    {
        stats->text_bytes = n;
        stats->n_records = reads->n_records;
        stats->n_reads = Rg;
        double tt = 0;
        for (uint32_t d = 0; d < A; d++) tt = std::max(tt, ro[d].t_text - ro[d].t_start);
        stats->text_ms = (float)tt;
        stats->parse_ms = (float)std::max(0.0, (t_parsed - t0) - tt);
        double tb = 0, tr = 0;
        for (uint32_t o = 0; o < N; o++) tb = std::max(tb, t_built[o] - t_merged), tr = std::max(tr, t_ran[o] - t_built[o]);
        stats->build_ms = (float)((t_merged - t_parsed) + tb);
        stats->run_ms = (float)tr;
        stats->d2h_ms = (float)std::max(0.0, now_ms() - t_merged - tb - tr);
    }
};

int ingest_text_group(yacrd_engine *const *E, uint32_t N, const TextSource &src, u64 n, bool m4, int n_threads, uint32_t coverage,
                      double not_coverage, yacrd_result *out, yacrd_reads *reads, yacrd_ingest_stats *stats)
{
    GroupRun g{E, N, n};
    if (const int rc = g.cut_ranges()) return rc;
    if (const int rc = g.fits()) return rc;
    if (g.A < 2) return ingest_text(E[0], src, n, m4, n_threads, coverage, not_coverage, out, reads, stats);
    if (const int rc = g.parse(src, m4, n_threads)) return rc;
    if (const int rc = g.merge(reads)) return rc;
    g.deal();
    if (const int rc = g.rewrite()) return rc;
    int rc = g.build_and_sweep(coverage, not_coverage);
    if (!rc) rc = g.stitch(out);
    if (rc) { // (a failed call leaves no engine with an input CSR to show: yacrd_debug_last_input_csr)
        for (uint32_t d = 0; d < N; d++) E[d]->input.valid = false;
        return rc;
    }
    if (stats) g.fill_stats(reads, stats);
    return YACRD_OK;
}

// The overlap file of an ingest, open for the call: a regular file, and text — gzip / bzip2 / xz is not: the caller inflates
// the file (yacrd_text_from_file, libyacrd_host) and hands the text to `mem_form`, or takes the host parser.
struct OverlapFile {
    struct stat st;
    bool m4 = false; // (overlap_format's, set by the entry point before the file is opened)
    TextSource src;
    int open(const char *path, const char *mem_form)
    {
        src.fd = ::open(path, O_RDONLY);
        if (src.fd < 0) return fail(YACRD_EINVAL, std::string("cannot open ") + path);
        if (fstat(src.fd, &st) != 0 || !S_ISREG(st.st_mode)) return fail(YACRD_EFALLBACK, "not a regular file: the host parser reads it");
        if (is_compressed_magic(src.fd))
            return fail(YACRD_EFALLBACK, std::string("a compressed file: inflate it (yacrd_text_from_file + ") + mem_form + ") or take the host parser");
        return YACRD_OK;
    }
    ~OverlapFile()
    {
        if (src.fd >= 0) ::close(src.fd);
    }
};

// A one-engine ingest has left the whole text in the parser's scratch: the overlap editor may start from it (gpu_edit.hip).
// `st`: the file it was, or nullptr for a text from memory or a BGZF stream — no file identity, never taken for a file.
// `facts`: n_fields and ends_nl are first_line_fields' answers for the text (the _resident_ forms need them).
void record_mirror(yacrd_engine *e, u64 n, bool m4, const struct stat *st, bool facts, u32 n_fields, bool ends_nl)
{
    auto &m = e->mirror;
    m.p = scratch_of<Scratch>(e)->text.as<unsigned char>(); // (ingest_text made the scratch)
    m.n = n, m.m4 = m4;
    m.from_file = st != nullptr;
    m.dev = st ? (u64)st->st_dev : 0, m.ino = st ? (u64)st->st_ino : 0;
    m.mtime_s = st ? (int64_t)st->st_mtim.tv_sec : 0, m.mtime_ns = st ? (int64_t)st->st_mtim.tv_nsec : 0;
    m.facts = facts, m.n_fields = n_fields, m.ends_nl = ends_nl;
    m.valid = m.p != nullptr;
}
} // namespace

extern "C" {

/* tests: cross-engine copies since the library was loaded, by route — same device / hipMemcpyPeerAsync / staged through the host */
void yacrd_debug_peer_copy_counts(uint64_t out[3])
{
    for (int i = 0; i < 3; i++) out[i] = g_peer_copies[i].load();
}

int yacrd_engine_ingest_overlaps(yacrd_engine *e, const char *path, int format, int n_threads, uint32_t coverage,
                                 double not_coverage, yacrd_result *out, yacrd_reads *reads, yacrd_ingest_stats *stats)
{
    if (!e || !path || !out || !reads) return fail(YACRD_EINVAL, "null argument");
    e->mirror.valid = false; // (the resident overlap text is the last SUCCESSFUL ingest's)
    e->resident.valid = e->input.valid = false;
    OverlapFile f;
    if (const int rcf = overlap_format(path, format, f.m4)) return rcf;
    zero_outputs(out, reads, stats);
    if (e->pending.active || e->host_pending) return fail(YACRD_EINVAL, "the engine has a submitted batch pending");
    if (const int rcf = f.open(path, "yacrd_engine_ingest_overlaps_mem")) return rcf;
    const int rc = ingest_text(e, f.src, (u64)f.st.st_size, f.m4, n_threads, coverage, not_coverage, out, reads, stats);
    if (rc == YACRD_OK) { // the whole file lies in the mirror: the overlap editor may start from it (gpu_edit.hip)
        u32 n_fields = 0;
        bool ends_nl = true;
        const bool facts = first_line_fields(f.src, (u64)f.st.st_size, f.m4 ? ' ' : '\t', n_fields, ends_nl);
        record_mirror(e, (u64)f.st.st_size, f.m4, &f.st, facts, n_fields, ends_nl);
    }
    return rc;
}

int yacrd_engine_ingest_overlaps_mem(yacrd_engine *e, const char *text, uint64_t n, int format, int n_threads, uint32_t coverage,
                                     double not_coverage, yacrd_result *out, yacrd_reads *reads, yacrd_ingest_stats *stats)
{
    if (!e || (!text && n) || !out || !reads) return fail(YACRD_EINVAL, "null argument");
    e->mirror.valid = false; // (the resident overlap text is the last SUCCESSFUL ingest's)
    e->resident.valid = e->input.valid = false;
    bool m4 = false;
    if (const int rcf = overlap_format(nullptr, format, m4)) return rcf;
    zero_outputs(out, reads, stats);
    if (e->pending.active || e->host_pending) return fail(YACRD_EINVAL, "the engine has a submitted batch pending");
    TextSource src;
    src.mem = text ? text : "";
    const int rc = ingest_text(e, src, n, m4, n_threads, coverage, not_coverage, out, reads, stats);
    if (rc == YACRD_OK) { // (the text is still the caller's to read: what the resident editor asks of it, now)
        u32 n_fields = 0;
        bool ends_nl = true;
        const bool facts = first_line_fields(src, n, m4 ? ' ' : '\t', n_fields, ends_nl);
        record_mirror(e, n, m4, nullptr, facts, n_fields, ends_nl);
    }
    return rc;
}

int yacrd_engine_ingest_overlaps_bgzf_mem(yacrd_engine *e, const char *bgzf, uint64_t n_bytes, int format, int n_threads, uint32_t coverage,
                                          double not_coverage, yacrd_result *out, yacrd_reads *reads, yacrd_ingest_stats *stats, yacrd_gunzip_stats *us)
{
    if (!e || (!bgzf && n_bytes) || !out || !reads) return fail(YACRD_EINVAL, "null argument");
    e->mirror.valid = false; // (the resident overlap text is the last SUCCESSFUL ingest's)
    e->resident.valid = e->input.valid = false;
    bool m4 = false;
    if (const int rcf = overlap_format(nullptr, format, m4)) return rcf;
    zero_outputs(out, reads, stats);
    if (us) std::memset(us, 0, sizeof(*us));
    if (e->pending.active || e->host_pending) return fail(YACRD_EINVAL, "the engine has a submitted batch pending");
    BgzfIn in;
    if (const int rcw = in.walk(bgzf, n_bytes)) return rcw;
    TextProducer tp;
    tp.bgzf = &in;
    const int rc = ingest_text(e, tp, in.text_bytes, m4, n_threads, coverage, not_coverage, out, reads, stats);
    {
        DeviceGuard guard(e->device);
        (void)hipStreamSynchronize(e->stream); // (whatever failed: nothing of this call is in flight when its events go)
        (void)hipGetLastError();
        if (rc == YACRD_OK) in.stats(us);
    }
    if (rc == YACRD_OK) { // (no text on the host: the first members and the last one, decoded there)
        u32 n_fields = 0;
        bool ends_nl = true;
        u32 status = 0; // (the helper itself, not BgzfIn::text_ends: a sample that cannot say leaves this call's success, and the last error, as they are)
        const bool facts = bgzf_text_ends(reinterpret_cast<const unsigned char *>(in.comp), in.comp_bytes, in.members.data(), in.members.size(),
                                          (u64)1 << 20, (unsigned char)(m4 ? ' ' : '\t'), &n_fields, &ends_nl, &status) == 0;
        record_mirror(e, in.text_bytes, m4, nullptr, facts, n_fields, ends_nl);
    }
    return rc;
}

static int group_args(yacrd_engine *const *engines, uint32_t n_engines, yacrd_result *out, yacrd_reads *reads, yacrd_ingest_stats *stats)
{
    if (!engines || !n_engines || !out || !reads) return fail(YACRD_EINVAL, "null argument");
    for (uint32_t d = 0; d < n_engines; d++) {
        if (!engines[d]) return fail(YACRD_EINVAL, "engine is null");
        engines[d]->mirror.valid = false; // (a group leaves no engine with the whole text)
        engines[d]->resident.valid = engines[d]->input.valid = false; // (an engine that parses no range still gets its reads' lengths in in_len)
        if (engines[d]->pending.active || engines[d]->host_pending) return fail(YACRD_EINVAL, "an engine has a submitted batch pending");
        for (uint32_t k = 0; k < d; k++)
            if (engines[k] == engines[d]) return fail(YACRD_EINVAL, "the same engine twice");
    }
    zero_outputs(out, reads, stats);
    return YACRD_OK;
}

int yacrd_engines_ingest_overlaps(yacrd_engine *const *engines, uint32_t n_engines, const char *path, int format, int n_threads,
                                  uint32_t coverage, double not_coverage, yacrd_result *out, yacrd_reads *reads, yacrd_ingest_stats *stats)
{
    if (const int rca = group_args(engines, n_engines, out, reads, stats)) return rca;
    if (n_engines == 1) return yacrd_engine_ingest_overlaps(engines[0], path, format, n_threads, coverage, not_coverage, out, reads, stats);
    if (!path) return fail(YACRD_EINVAL, "null argument");
    OverlapFile f;
    if (const int rcf = overlap_format(path, format, f.m4)) return rcf;
    if (const int rcf = f.open(path, "yacrd_engines_ingest_overlaps_mem")) return rcf;
    const int rc = ingest_text_group(engines, n_engines, f.src, (u64)f.st.st_size, f.m4, n_threads, coverage, not_coverage, out, reads, stats);
    if (rc) yacrd_reads_free(reads);
    return rc;
}

int yacrd_engines_ingest_overlaps_mem(yacrd_engine *const *engines, uint32_t n_engines, const char *text, uint64_t n, int format,
                                      int n_threads, uint32_t coverage, double not_coverage, yacrd_result *out, yacrd_reads *reads,
                                      yacrd_ingest_stats *stats)
{
    if (const int rca = group_args(engines, n_engines, out, reads, stats)) return rca;
    if (n_engines == 1)
        return yacrd_engine_ingest_overlaps_mem(engines[0], text, n, format, n_threads, coverage, not_coverage, out, reads, stats);
    if (!text && n) return fail(YACRD_EINVAL, "null argument");
    bool m4 = false;
    if (const int rcf = overlap_format(nullptr, format, m4)) return rcf;
    TextSource src;
    src.mem = text ? text : "";
    const int rc = ingest_text_group(engines, n_engines, src, n, m4, n_threads, coverage, not_coverage, out, reads, stats);
    if (rc) yacrd_reads_free(reads);
    return rc;
}

/* include/yacrd_engine_debug.h: the device parser's sort on its own (tests) */
int yacrd_debug_sort_pairs(yacrd_engine *e, uint64_t *keys, uint32_t *vals, uint64_t n, uint64_t key_bound)
{
    if (!e || (n && (!keys || !vals))) return fail(YACRD_EINVAL, "null argument");
    if (n >= 0x7FFFFFFFull) return fail(YACRD_EINVAL, "too many pairs");
    DeviceGuard guard(e->device);
    DevBuf k0, k1, v0, v1, tmp, part;
    HIP_TRY(k0.reserve((size_t)n * sizeof(u64) + 64));
    HIP_TRY(k1.reserve((size_t)n * sizeof(u64) + 64));
    HIP_TRY(v0.reserve((size_t)n * sizeof(u32) + 64));
    HIP_TRY(v1.reserve((size_t)n * sizeof(u32) + 64));
    if (!n) return YACRD_OK;
    HIP_TRY(hipMemcpyAsync(k0.p, keys, (size_t)n * sizeof(u64), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync(v0.p, vals, (size_t)n * sizeof(u32), hipMemcpyHostToDevice, e->stream));
    if (const int rcs = sort_by_first_position(e, k0.as<u64>(), k1.as<u64>(), v0.as<u32>(), v1.as<u32>(), (u32)n, key_bound, tmp, part)) return rcs;
    HIP_TRY(hipMemcpyAsync(keys, k1.p, (size_t)n * sizeof(u64), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(vals, v1.p, (size_t)n * sizeof(u32), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipGetLastError());
    return YACRD_OK;
}

} // extern "C"
