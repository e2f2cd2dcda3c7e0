// screen_reg.h — the healthy-read screen of the register classes (<= 256 intervals): reads that
// are bad in front of their (c+1)-th smallest start and behind their (c+1)-th largest end and nowhere else are
// finished in closed form from one counting pass over LDS bins, no sort; every other read is left to the sort
// (finish_compact.h, one_batch.h).  healthy_screen is one read's screen, screen_reads the loads and verdicts of
// ITEMS reads per lane group, screen_block the fused launch's workgroup (sweep_wave.h).  The larger classes'
// screens are screen_wg.h, screen_big.h and screen_stream.h.
#pragma once
#include "device_common.h"
#include "wave_ops.h"

namespace yk {

// ---- the healthy-read screen of the deferring build (tests/formulation.py::
// window_screen_regions is the emulation, fuzzed against the oracle) -----------------------------------
// With a = the (c+1)-th smallest start and b = the (c+1)-th largest end of a plain read: if every start
// beyond the first c + 1 finds more than c intervals open, the reference (src/stack.rs:61-139) assigns
// first_covered at the first c + 1 starts (heap sizes 0..c, nothing popped yet: :83-89), never opens a
// gap afterwards, and its tail loop (:93-105) pops down to c open intervals, i.e. ends on the (c+1)-th
// largest end (or breaks on an end == len, which then is that end as well).  The read is bad in front
// of a and behind b and nowhere else: the HEALTHY read, 96-97 % of a well-covered data set.
// a, b and the test come from ONE counting pass, no sort:
//   * W one-position bins counted from the read's smallest start pmin upwards (starts only, low half
//     of a counter) and from its largest end pmax downwards (ends only, high half) — the windows the
//     two order statistics lie in when the dovetail overlaps end within a few dozen positions of each
//     other (at exactly 0 / len in SURVEY.md §8d's clamped generator, spread by the overlapper's
//     chain ends in real data);
//   * NB coarse bins of 2^sh positions, NB / LANES per lane, for every other event (one per lane, except in the
//     long launch's H16 form: 32 blocks on 16 lanes, below).
// Every interval must be at least W long (anything shorter: deferred): then no end lies inside the head
// window and no start inside the tail window, in event order the read is [head window: F starts]
// [coarse bins][tail window: G ends], and a coarse-counted start of bin i has at least
// F + (starts of bins < i) - (ends of bins <= i) intervals open in front of it.  A read is healthy when
// F >= c + 1, G >= c + 1 and that bound exceeds c in every coarse bin that holds a start.
// One LDS atomic per event (four copies of every counter by lane & 3 so that piled positions do not
// serialise the atomics of a row), one packed row scan per table.  Every other read — low coverage
// somewhere inside: the reads yacrd is looking for — is marked in its region-count slot (kDeferredMark)
// and sorted by the follow-on kernel (finish_compact.h), which finds the marks.  (A list appended to with one global atomic per read was the first
// attempt: the same-address atomics, performed at the memory side on this 8-XCD part, took ~7 ns each
// one after the other and doubled the kernel's duration.)
// Only for wavefronts whose intervals are all plain (start < end <= len) and at least W long.
#ifndef YK_SCREEN_WINDOW
#define YK_SCREEN_WINDOW 32
#endif
constexpr int kScreenWindow = YK_SCREEN_WINDOW; // W: positions per window (a multiple of 32)
// per group: W head-window bins + NB coarse blocks + W tail-window bins, 16 bytes (four copies) each
constexpr int kScreenTabWords = (64 / 16) * (16 + 2 * kScreenWindow) * 4;
// H16 ROWS (the long launch's H16 form): an H16 read on ONE 16-lane row, sixteen intervals per lane, so that
// a wavefront screens its four reads as one item and pays the per-item instructions (addresses, zeroing, window reads,
// the row scans, the verdict) once per four reads instead of once per two.  The read keeps its 32 coarse blocks, two
// per lane: with 16 blocks (NB = LANES) the depth test fails on 29 % more of the clamped generator's reads and on twice
// as many at sigma = 100, and those go to the follow-on sort.  Table, sh, a, b, F, G and the depth test are the 32-lane
// form's, so both forms decide and defer the same reads.  Four groups of 2 W + 32 bins:
constexpr int kScreenTabWordsRows = (64 / 16) * (32 + 2 * kScreenWindow) * 4;
template <int WPB, int WORDS = kScreenTabWords> // wavefronts per workgroup; words per wavefront (a kernel of 32-lane groups only needs 768)
__device__ __forceinline__ u32 *wave_screen_scratch()
{
    __shared__ __attribute__((aligned(16))) u32 s_tab[WPB][WORDS];
    return s_tab[threadIdx.x >> 6];
}

// whether any lane of this lane's group has its bit set in a wavefront ballot
template <int LANES>
__device__ __forceinline__ bool group_any(u64 ballot)
{
    if (LANES == 64) return ballot != 0;
    return ((u32)(ballot >> (lane_id() & (u32)(64 - LANES))) & (u32)((1ull << (LANES & 63)) - 1ull)) != 0u;
}

struct HealthyRead {
    u32 a, b; // the (c+1)-th smallest start, the (c+1)-th largest end
    i32 F, G; // starts counted up to the end of the head window, ends from the start of the tail window on
};
// Windows that slide (round 4; tests/formulation.py::slid_window_screen_regions is the emulation, fuzzed against the
// oracle).  The (c+1)-th smallest start of a read whose dovetail overlaps end within sigma positions of each other
// lies ~0.2 sigma (ONT depth, -c 4) .. 0.1 sigma (Sequel depth) behind the smallest one: inside W = 32 positions for
// SURVEY.md 8d's sigma = 30, beyond them for a fifth of configs[1]'s reads at sigma = 100 and for most at 300 (what
// minimap2's chain ends look like: VERDICT r3).  A wider table costs every read (W = 64: 9 KB of LDS per wavefront
// instead of 5, occupancy 5 -> 4 by LDS alone: 0.61 -> 0.78 ms on configs[2], profiles/r04/a_ab_window64.log), so
// instead a read whose window came up short is screened AGAIN with that window moved on by W, what the window has
// passed carried as a count: P starts in front of the head window, Q ends behind the tail window.  In event order
// the read is [P][head window][coarse blocks][tail window][Q] as long as no end lies at or before the head window's
// last position and no start at or behind the tail window's first: checked per slide on the read's smallest end
// and largest start.  Only wavefronts that hold such a read take the extra passes.
#ifndef YK_SCREEN_SLIDES
#define YK_SCREEN_SLIDES 4
#endif
constexpr int kScreenSlides = YK_SCREEN_SLIDES;
// Built, measured and removed after 1714e90 (the code is in history up to that commit; emulations: tests/formulation.py):
//   * window bins of 2^WB positions in the build with the second looks — the windows reach W << WB positions with the same table, a and b
//     are resolved inside their bin by counting.  Bit-exact (104 parity tests, 3 M fuzzed reads with the second looks forced), and a
//     trade, not a gain: WB = 2 (windows of 128 positions: most reads need no slide) takes configs[1] at sigma = 300 from 53.4 to 48.4 us
//     per batch (the screen alone 41.1 -> 36.4 us, frac 0.24 -> 0.27; 600 more reads have an interval shorter than the window: 95.3 ->
//     94.7 % decided) and at sigma = 100 from 32.3 to 36.3 (alone 27.1 -> 30.4: the resolve and 80 registers + 24 bytes of scratch
//     instead of 62 cost the reads that needed no slide anyway); WB = 1: 51.0 / 32.9 (profiles/r06/T_wb.log).
//   * windows that JUMP: a window that came up short goes to the next event it has not seen instead of W positions on (formulation.py
//     jump, fuzzed + enumerated: never fewer reads decided, fewer passes — 2.4 -> 2.0 for the slowest of a wavefront's four reads at
//     sigma = 300).  Bit-exact (122 parity tests, 3.4 M fuzzed reads), and the two reductions per slide cost what the saved passes
//     gain: configs[1] at sigma = 300 54.4 -> 52.6 us per batch (kernel 65.2 -> 63.5, 4 696 -> 4 551 reads left), at 100 32.6 -> 33.9,
//     configs[2] at 300 1.03 -> 1.07 ms (profiles/r06/Q_jump.log).
//   * SPOT CHECKS behind a screen that failed on a block's depth only, in the build with the second looks (formulation.py::_sub_screen
//     (spot = 8, at most eight starts), fuzzed + exhaustive over small multisets: test_formulation.py::test_slid_window_*): the few coarse-counted
//     starts of the failing blocks looked at one by one.  Bit-exact (the -m gpu parity files + 3.6 M fuzzed reads with the second looks
//     forced, profiles/r06/A_*, B_*), and they do what they are for — configs[1] decided 88.7 -> 94.8 % at sigma = 300, 94.9 -> 97.1 %
//     at 100, the follow-on sorts half as many reads — but the screen pays more than the follow-on gains: its launch 64 -> 77 us at
//     sigma 300 and 33 -> 47 at 100 (a wavefront enters when ANY of its four reads wants), the pipelined batch 56 -> 60 and 34 -> 36 us;
//     only one batch at a time gains (119 -> 116).  (On the read's intervals where they are: behind a call that loaded them again the
//     check cost the screen 12 us of 64 at sigma 300, profiles/r06/A_*.)
//   * the OTHER closed form, for a read with one stretch of low coverage inside — a chimera: regions (0, a), (x, y), (b, len)
//     (formulation.py::hole_fast_regions, hole_screen_regions the derivation).  Bit-exact (GPU tests, fuzz) and it decides 77 % of
//     what the screen otherwise defers (configs[2]: 47 608 -> 11 032 reads, the deferred sweep 145 -> 68 us) — but its ~1000
//     instructions are spent by every wave-item that holds such a read, 4.5-9 % of them, inside the kernel that is already short of
//     VALU issue slots: the screen 0.613 -> 0.711 ms on configs[2], 1.43 -> 1.81 ms on configs[4], the step 0.816 -> 0.853 / 1.77 ->
//     2.06 ms (profiles/r04/e_ab_hole_form.log).
// Which builds carry the second looks: only sweep_small_fused_defer_wide_kernel.  The two-items build has no registers for
// them (a spilled load at its very start, or occupancy 5: 0.625 -> 0.66 ms on configs[2], profiles/r04/d_*; behind a call that
// reloads the read the call's arguments spill the same load, and the one-item build gets slower still: profiles/r04/n_*), and
// the plain one-item build is a tenth faster without them.  The engine switches (engine.hip: wide_left).

// The screen works on the raw positions (no event keys are made): v[j] = two intervals (x, y) and
// (z, w) of this lane, real0[j] / real1[j] = whether those slots belong to the read (the others hold
// copies and are not counted), pmin / pmax = the group's smallest start / largest end.
// The verdict and hr are valid in the group's LAST lane (it owns the inclusive scan totals).
//
// Bins.  With dx = position - pmin, span = pmax - pmin, T = span - W and 2^sh >= W, both maps are plain
// arithmetic (no compare, no select: five instructions and one LDS atomic per event):
//   start -> min(dx, W) + (dx >> sh)                bins 0..W-1: one position each (the head window);
//                                                   W + i: the rest of coarse block i of 2^sh positions
//   end   -> W + (dx >> sh) + max(dx - T, 0)        W + i: block i up to T; above that every position of
//                                                   the tail window has a bin of its own (the map rises
//                                                   by at least one per position there)
// Starts never lie in the tail window and ends never in the head window (every interval is at least W
// long), so bin W + i holds the coarse-counted starts and ends of block i, and what the bins above
// W + (T >> sh) hold besides are ends of the tail window that precede the block: counting them there
// errs on the safe side, and no start lives in those blocks anyway.
// Counters hold starts in bits 0..9 and ends in bits 10..19 (a read of these classes has <= 256
// intervals), which leaves the upper bits of the coarse bins' scan for the two window indices.
// SLID: pmin / pmax are the head window's first and the tail window's last position (the read's smallest start +
// h0, its largest end - t0), events outside [pmin, pmax] are not counted, P / Q stand for them.
// emin (SLID): the read's smallest end.  Starts behind the head window but in front of it — the RAMP — find nothing
// popped yet and every earlier start still open: more than c once a has passed, so they are never low; they are
// counted like the window's starts (open in front of every coarse-counted start), not into a coarse block.
// smax (SLID, round 6): the read's largest start.  THE RAMP'S MIRROR: an end behind it is popped after every start has
// arrived — no start finds it gone — so the ends between smax and the tail window are not counted into their coarse
// blocks (where all of a block's ends count as popped before the block's starts).  Dovetail ends spread by hundreds of
// positions fill the read's last blocks with such ends: 8 % of configs[1]'s reads at sigma = 300 failed the depth test on
// them alone (tests/formulation.py: tail_ramp; emulation on the generator's reads 91.3 -> 98.3 % decided).
// NB: coarse blocks of the read (a multiple of LANES; a lane owns NB / LANES consecutive ones).  PAIRS: 16-byte pairs of
// intervals per lane (the caller's array extent).
template <int LANES, int WPB, bool SLID = false, int TABW = kScreenTabWords, int NB = LANES, int PAIRS = 4>
__device__ __forceinline__ bool healthy_screen(const uint4 (&v)[PAIRS], const bool (&real0)[PAIRS], const bool (&real1)[PAIRS],
                                               u32 len, i32 c, u32 pmin, u32 pmax, HealthyRead &hr, u32 P = 0, u32 Q = 0,
                                               u32 emin = 0, u32 smax = 0xFFFFFFFFu)
{
    constexpr int W = kScreenWindow, NBIN = 2 * W + NB, GROUPS = 64 / LANES, PER = W / LANES, ZPER = NBIN / LANES,
                  CPL = NB / LANES;
    constexpr u32 kEnd = 1u << 10, kField = kEnd - 1u;
    static_assert(W % LANES == 0 && PER >= 1 && W <= 64, "window bins per lane; a window index has six bits");
    static_assert(NB % LANES == 0 && NBIN % LANES == 0 && GROUPS * NBIN * 4 <= TABW, "scratch");
    static_assert(PAIRS * 2 * LANES <= 256, "a counter field has ten bits");
    const u32 lane = lane_id(), lig = lane & (u32)(LANES - 1), grp = lane / (u32)LANES;
    u32 *tab = wave_screen_scratch<WPB, TABW>() + grp * (u32)(NBIN * 4);
    uint4 *bins = reinterpret_cast<uint4 *>(tab);
    char *tb = reinterpret_cast<char *>(tab);

    // smallest shift with (len >> sh) < NB, but blocks of at least W positions
    const i32 bits = 32 - (i32)__builtin_clz(len | 1u) - ilog2c(NB) + (len != 0 ? 0 : -1);
    const u32 sh = (u32)max(bits, ilog2c(W));
    const u32 span = pmax - pmin, T = span - (u32)W;

#pragma unroll
    for (int q = 0; q < ZPER; q++) bins[lig + (u32)(LANES * q)] = make_uint4(0u, 0u, 0u, 0u);
    wave_lds_sync();

    // ---- count.  Byte offset of a counter = bin * 16 + (lane & 3) * 4 (four copies of every counter, so
    // that piled positions do not serialise the atomics of a row).  The slots beyond the read are masked
    // out (counted into a bin of their own their atomics piled up on four addresses).
    const u32 cp = (lig & 3u) * 4u;
    u32 one = 1u, one_end = kEnd; // kept in registers (the compiler re-materialises them per atomic otherwise)
    if constexpr (!SLID) asm volatile("" : "+v"(one), "+v"(one_end)); // (the rare second look gives the two registers back)
    u32 ramp = 0; // (SLID) this lane's starts between the head window and the read's smallest end
    auto count = [&](u32 s, u32 e, bool real) {
        const u32 ds = s - pmin, dx = e - pmin;
        const u32 is = min(ds, (u32)W) + (ds >> sh);
        const u32 ie = (dx >> sh) + __builtin_elementwise_sub_sat(dx, T) + (u32)W;
        if constexpr (SLID) { // (what the windows have passed is not counted: P and Q stand for it)
            const bool in_ramp = ds >= (u32)W && s < emin;
            ramp += (real && s >= pmin && in_ramp) ? 1u : 0u;
            if (real && s >= pmin && !in_ramp) atomicAdd(reinterpret_cast<u32 *>(tb + ((is << 4) + cp)), one);
            // (the ramp's mirror: an end behind the read's largest start and in front of the tail window is in no block's count)
            if (real && e <= pmax && !(e > smax && dx <= T)) atomicAdd(reinterpret_cast<u32 *>(tb + ((ie << 4) + cp)), one_end);
        } else if (real) {
            atomicAdd(reinterpret_cast<u32 *>(tb + ((is << 4) + cp)), one);
            atomicAdd(reinterpret_cast<u32 *>(tb + ((ie << 4) + cp)), one_end);
        }
    };
#pragma unroll
    for (int j = 0; j < PAIRS; j++) {
        count(v[j].x, v[j].y, real0[j]);
        count(v[j].z, v[j].w, real1[j]);
    }
    wave_lds_sync();

    // ---- the windows: where the counts of starts (from pmin upwards) and of ends (from pmax downwards)
    // reach c + 1.  Window position d = lig * PER + q: the start bin d, the end bin of pmax - d.
    u32 f[PER], fw = 0;
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const u32 d = lig * (u32)PER + q;
        const u32 it = min((u32)(2 * W) - d + ((span - d) >> sh), (u32)(NBIN - 1)); // (clipped: an irregular group's span is anything)
        const uint4 h4 = bins[d], t4 = bins[it];
        f[q] = ((h4.x + h4.y + h4.z + h4.w) & kField) | ((t4.x + t4.y + t4.z + t4.w) & (kField << 10));
        fw += f[q];
    }
    // this lane's coarse blocks lig * CPL + q, starts | ends << 10 each
    u32 wb[CPL], w = 0;
#pragma unroll
    for (int q = 0; q < CPL; q++) {
        const uint4 c4 = bins[(u32)W + lig * (u32)CPL + q];
        wb[q] = (c4.x + c4.y + c4.z + c4.w) & ((kField << 10) | kField);
        w += wb[q];
    }
    const u32 fincl = gscan_add<LANES>(fw); // last lane: F | G << 10
    // a - pmin = the number of window positions whose running count of starts is still below c + 1 (the
    // counts only grow), pmax - b likewise for the ends: both fields at once — adding 512 - (c + 1) to a
    // field (counts <= 256) sets its bit 9 exactly when the count has reached c + 1.
    u32 reached = 0;
    {
        const u32 k1 = (u32)min(c + 1, 0x1FF);
        // counts in front of this lane's bins, biased (SLID: P <= c starts and Q <= c ends are already in)
        u32 run = fincl - fw + (SLID ? ((512u - k1 + P) | ((512u - k1 + Q) << 10)) : (512u - k1) * (1u | kEnd));
#pragma unroll
        for (int q = 0; q < PER; q++) {
            run += f[q];
            reached += run & (0x200u | (0x200u << 10));
        }
    }
    // bins that have NOT reached it, in the upper bits of the coarse scan: starts at bit 20, ends at bit 26
    const u32 cand = (((u32)PER - ((reached >> 9) & 7u)) << 20) | (((u32)PER - (reached >> 19)) << 26);
    // ---- the coarse bins: a block that holds a coarse-counted start must have more than c intervals
    // open at its head even after all of its ends: F + (starts before it) - (ends up to its last one) > c.
    // One scan over the lanes' sums for the counts and the two window indices (each set in one lane only); a lane with
    // several blocks walks them from its exclusive total and hands the scan of minima the shallowest one.
    const u32 wincl = gscan_add<LANES>(w | cand);
    u32 run = wincl - w, xl = 0xFFFFFFFFu;
#pragma unroll
    for (int q = 0; q < CPL; q++) {
        const u32 ex = run;
        run += wb[q];
        const i32 x = (i32)(ex & kField) - (i32)((run >> 10) & kField); // starts before - ends through this block
        xl = min(xl, (wb[q] & kField) != 0u ? (u32)(x + 0x10000) : 0xFFFFFFFFu);
    }
    const u32 xm = gscan_min<LANES>(xl);
    // (meaningful in the group's last lane from here on)
    const i32 F = (i32)(fincl & kField) + (SLID ? (i32)P : 0), G = (i32)(fincl >> 10) + (SLID ? (i32)Q : 0);
    hr.F = F, hr.G = G;
    hr.a = pmin + ((wincl >> 20) & 63u); // (a window that never reaches c + 1 overflows these fields: F > c
    hr.b = pmax - (wincl >> 26);         // or G > c fails then)
    i32 open0 = F; // intervals open in front of every coarse-counted start
    if constexpr (SLID) open0 += (i32)gscan_add<LANES>(ramp);
    const bool deep = xm == 0xFFFFFFFFu || (i32)(xm - 0x10000u) + open0 > c;
    return deep && F > c && G > c;
}

// ---- the screen over ITEMS consecutive groups of list entries per wavefront (one-wavefront workgroups)
// Every level of the dependent chain — list entries, offsets / lengths, intervals — is fetched for all
// ITEMS at once, so a wavefront has ITEMS x 8 interval loads per lane in flight (8 KB at ITEMS = 2) and
// pays each round trip once per ITEMS groups: what an HBM-resident input needs to keep the memory
// system busy (configs[2]: ... ).  The screens then run one after the other on the same LDS table.
// Where the screen's verdicts go (the group's last lane calls): the fused launch answers through counts[] / closed[]
// in global memory (device_common.h: kClosedForm, kDeferredMark) for the follow-on kernel to find; the one-launch form
// of a short batch (one_batch.h) keeps them in its workgroup's LDS.
struct VerdictsToGlobal {
    const SweepArgs &a;
    bool own_count = false; // the direct launch (screen_block_rows): the plan left the read's count word alone, kClosedForm is written here
    __device__ __forceinline__ void closed(u32 r, u32 ra, u32 rb, u32 len) const
    {
        // counts[r] says kClosedForm since the plan kernel: ONE store per decided read, its (a, b) — or, for a read with no
        // bad region at all, the count 0 in four bytes
        if (ra != 0 || rb != len) {
            a.closed[r] = make_uint2(ra, rb);
            if (own_count) a.counts[r] = kClosedForm;
        } else a.counts[r] = 0;
        if (a.prefilter == 2) atomicAdd(&a.ctr->prefiltered, 1u);
    }
    __device__ __forceinline__ void deferred(u32 r) const { a.counts[r] = kDeferredMark; }
};

// (extent and length of the reads, when the caller has them already: one_batch.h)
template <int ITEMS>
struct ReadsKnown {
    u64 o[ITEMS];
    u32 n[ITEMS], len[ITEMS];
};

// ITEMS reads per lane group, given by their ids (active[t]: this group has a t-th read; a t with no active group in the
// wavefront ends the loop).  WPB: wavefronts per workgroup (each has a table of its own in LDS).  K: events per lane
// (K / 4 pairs of intervals), NB: the read's coarse blocks, NT: the launch streams its intervals from HBM (non-temporal
// loads), TABW: words of the wavefront's table (one size per kernel: every form in it shares the table).
template <int LANES, int ITEMS, bool WIDE, int WPB = 1, int K = 16, int NB = LANES, bool NT = (ITEMS >= 2),
          int TABW = kScreenTabWords, class Sink>
__device__ __forceinline__ void screen_reads(const SweepArgs &a, const u32 (&r)[ITEMS], const bool (&active)[ITEMS], const Sink &sink,
                                             const ReadsKnown<ITEMS> *known = nullptr)
{
    static_assert(K % 4 == 0, "a lane takes its intervals in pairs");
    const u32 lane = lane_id(), lig = lane & (u32)(LANES - 1);
    const i32 c = (i32)min(a.cov, 0x3FFFFFFFu);
    u32 n[ITEMS], len[ITEMS];
    u64 o[ITEMS];
#pragma unroll
    for (int t = 0; t < ITEMS; t++) {
        o[t] = 0, n[t] = 0, len[t] = 0;
        if (known) { // (a constant once inlined)
            if (active[t]) o[t] = known->o[t], n[t] = known->n[t], len[t] = known->len[t];
        } else if (active[t]) {
            const ulonglong2 oo = load_extent(a.off + r[t]); // off[r], off[r + 1]: one load
            o[t] = oo.x;
            n[t] = (u32)(oo.y - oo.x);
            len[t] = a.len[r[t]];
        }
    }
    // The screen does not care which lane holds which interval, so a lane takes its intervals two at a
    // time (16-byte loads: half the memory instructions and address arithmetic).  Pair P = lig + LANES*j
    // holds intervals 2P and 2P + 1; the load is clamped to the read's last pair (n - 2, n - 1), whose
    // second half is interval 2P itself when 2P = n - 1.  (8-byte aligned 16-byte loads are fine for
    // global memory; a read with fewer than two intervals — not in these classes — is left to the
    // follow-on kernel.)
    uint4 v[ITEMS][K / 4];
#pragma unroll
    for (int t = 0; t < ITEMS; t++) {
        const bool two = n[t] >= 2u;
        const uint2 *src = two ? a.iv + o[t] : reinterpret_cast<const uint2 *>(a.off);
        const u32 last2 = two ? n[t] - 2u : 0u;
#pragma unroll
        for (int j = 0; j < K / 4; j++)
            v[t][j] = load_pair<NT>(src + min(2u * (lig + (u32)LANES * j), last2));
    }
#pragma unroll
    for (int t = 0; t < ITEMS; t++) {
        if (t > 0 && __builtin_amdgcn_ballot_w64(active[t]) == 0) break; // uniform: nothing left for this item
        const u32 len_c = min(len[t], kMaxKeyPos);
        // The read's smallest start and largest end, from the raw positions of every slot: a slot beyond
        // the read's last interval holds a copy of one of its intervals (the clamped load), so it cannot
        // change either.  An end beyond the read (or beyond the key range) shows in the largest one.
        // Also, for the test below: the largest start and the smallest (end - start) as a signed number.
        u32 smin = v[t][0].x, emax = v[t][0].y, smax = v[t][0].x;
        i32 tmin = 0x7FFFFFFF;
#pragma unroll
        for (int j = 0; j < K / 4; j++) {
            smin = min(smin, min(v[t][j].x, v[t][j].z));
            smax = max(smax, max(v[t][j].x, v[t][j].z));
            emax = max(emax, max(v[t][j].y, v[t][j].w));
            tmin = min(tmin, min((i32)(v[t][j].y - v[t][j].x), (i32)(v[t][j].w - v[t][j].z)));
        }
        const int last_addr = (int)((lane | (u32)(LANES - 1)) << 2);
        const u32 pmin = (u32)__builtin_amdgcn_ds_bpermute(last_addr, (int)gscan_min<LANES>(smin));
        const u32 pmax = (u32)__builtin_amdgcn_ds_bpermute(last_addr, (int)gscan_max<LANES>(emax));
        // not plain (start >= end, an end beyond the read or the key range), or an interval shorter than
        // the screen's windows: left to the sort.  With every position <= kMaxKeyPos < 2^30, end - start
        // as a signed number is below W exactly for those intervals.  The slots beyond the read hold
        // copies of its own intervals, so no mask is needed here.
        const bool irregular = n[t] < 2u || pmax > len_c || smax > kMaxKeyPos || tmin < (i32)kScreenWindow;
        // per group: such a read counts nothing (its positions may lie outside the table) and is never healthy
        const bool girr = group_any<LANES>(__builtin_amdgcn_ballot_w64(irregular));
        const u32 n_eff = girr ? 0u : n[t];
        bool real0[K / 4], real1[K / 4];
#pragma unroll
        for (int j = 0; j < K / 4; j++) {
            const u32 i0 = 2u * (lig + (u32)LANES * j);
            real0[j] = i0 + 1u < n_eff; // .xy is interval i0 only when i0 + 1 exists too
            real1[j] = i0 < n_eff;
        }
        HealthyRead hr;
        bool healthy = healthy_screen<LANES, WPB, false, TABW, NB>(v[t], real0, real1, len[t], c, pmin, pmax, hr) && !girr;
        if constexpr (kScreenSlides > 0 && WIDE) {
            // a window that came up short of c + 1 (verdict in the group's last lane): slide it (see kScreenSlides).
            // st = need | F << 1 | G << 11 of the last screen (counts clipped to their ten bits)
            auto state_of = [&](bool nd, const HealthyRead &h) {
                return (nd ? 1u : 0u) | ((u32)min(max(h.F, 0), 1023) << 1) | ((u32)min(max(h.G, 0), 1023) << 11);
            };
            // ... or one that holds so few of the read's starts (fewer than ~3 (c + 1): spread dovetails) that the depth
            // test may have failed for want of the ramp: looked at once more where it stands, the ramp counted
            u32 st = state_of(!healthy && !girr && (i32)n[t] > c && (hr.F <= 3 * c + 6 || hr.G <= c), hr);
            if (__builtin_amdgcn_ballot_w64((st & 1u) != 0 && lig == (u32)(LANES - 1)) != 0) { // (uniform in the wavefront; rare)
                u32 emin = v[t][0].y, smax2 = v[t][0].x; // (re-derived here: kept from above they cost the common path registers)
#pragma unroll
                for (int j = 0; j < K / 4; j++) {
                    emin = min(emin, min(v[t][j].y, v[t][j].w));
                    smax2 = max(smax2, max(v[t][j].x, v[t][j].z));
                }
                // room in front of the smallest end / behind the largest start, in positions from pmin / pmax
                const u32 gemin = (u32)__builtin_amdgcn_ds_bpermute(last_addr, (int)gscan_min<LANES>(emin));
                const u32 room_h = gemin - pmin;
                const u32 gsmax = (u32)__builtin_amdgcn_ds_bpermute(last_addr, (int)gscan_max<LANES>(smax2));
                const u32 room_t = pmax - gsmax;
                u32 ht = 0, PQ = 0; // h0 | t0 << 16 (positions), P | Q << 16 (counts)
#pragma unroll 1
                for (int slide = 0; slide < kScreenSlides; slide++) {
                    const u32 g = (u32)__builtin_amdgcn_ds_bpermute(last_addr, (int)st); // the last lane's verdict and counts, to its group
                    const bool gneed = (g & 1u) != 0;
                    const u32 gF = (g >> 1) & 1023u, gG = g >> 11;
                    if (gneed && (i32)gF <= c) ht += (u32)kScreenWindow, PQ = (PQ & 0xFFFF0000u) | gF;
                    if (gneed && (i32)gG <= c) ht += (u32)kScreenWindow << 16, PQ = (PQ & 0xFFFFu) | (gG << 16);
                    const u32 h0 = ht & 0xFFFFu, t0 = ht >> 16;
                    // no end at or before the head window's last position, no start at or behind the tail window's
                    // first, and the two windows apart
                    const bool go = gneed && room_h >= h0 + (u32)kScreenWindow && room_t >= t0 + (u32)kScreenWindow &&
                                    pmax - pmin >= h0 + t0 + 2u * (u32)kScreenWindow;
                    if (__builtin_amdgcn_ballot_w64(go) == 0) break; // (uniform)
                    bool r0[K / 4], r1[K / 4];
#pragma unroll
                    for (int j = 0; j < K / 4; j++) r0[j] = real0[j] && go, r1[j] = real1[j] && go;
                    wave_lds_sync(); // (the table is zeroed again)
                    HealthyRead h2;
                    const bool ok2 = healthy_screen<LANES, WPB, true, TABW, NB>(v[t], r0, r1, len[t], c, pmin + h0, pmax - t0, h2, PQ & 0xFFFFu, PQ >> 16, gemin, gsmax);
                    st = go ? state_of(!ok2 && (h2.F <= c || h2.G <= c), h2) : 0u; // (meaningful in the group's last lane)
                    if (go) healthy = ok2, hr.a = h2.a, hr.b = h2.b, hr.F = h2.F, hr.G = h2.G;
                }
            }
        }
        if (lig == (u32)(LANES - 1) && active[t]) { // the group's last lane has the verdict
            if (healthy || (!girr && (i32)n[t] <= c)) {
                // never more than c intervals open: the whole read is bad = (0, a) with a = len
                const u32 ra = (i32)n[t] <= c ? len[t] : hr.a, rb = (i32)n[t] <= c ? len[t] : hr.b;
                sink.closed(r[t], ra, rb, len[t]);
            } else {
                sink.deferred(r[t]);
            }
        }
        if (t + 1 < ITEMS) wave_lds_sync(); // the next item zeroes the table
    }
}

template <int LANES, int ITEMS, bool WIDE = false, int K = 16, int NB = LANES, bool NT = (ITEMS >= 2), int TABW = kScreenTabWords>
__device__ __forceinline__ void screen_block(const SweepArgs &a, u32 block)
{
    constexpr u32 GROUPS = 64 / LANES;
    const u32 grp = lane_id() / (u32)LANES;
    const u32 list_n = *a.list_n;
    const u32 idx0 = a.first + block * (u32)ITEMS * GROUPS;
    if (idx0 >= list_n) return; // grids may be sized for more reads than the class holds
    u32 r[ITEMS];
    bool active[ITEMS];
#pragma unroll
    for (int t = 0; t < ITEMS; t++) {
        const u32 idx = idx0 + (u32)t * GROUPS + grp;
        active[t] = idx < list_n;
        r[t] = active[t] ? a.list[idx] : 0u;
    }
    screen_reads<LANES, ITEMS, WIDE, 1, K, NB, NT, TABW>(a, r, active, VerdictsToGlobal{a});
}

// Whether a read of n intervals is of class H16: plan_kernel's mode-0 rule 256 < 2 n <= 512 (plan_compact.h), as the direct
// launch below states it on a read's extent.
constexpr u32 kH16MinIntervals = 129, kH16MaxIntervals = 256;
__device__ __forceinline__ bool is_h16(u64 n) { return n >= (u64)kH16MinIntervals && n <= (u64)kH16MaxIntervals; }

// The long launch's workgroup of H16 ROWS: one wavefront, four reads, a 16-lane row each (screen_block<16, 1, false, 32, 32,
// true> with the extents fetched here).  Two ways to its reads:
//   * from the plan's class list, rows = list entries first + 4 block .. + 3: list entry, then extent and length, then
//     intervals — three dependent round trips;
//   * DIRECT, by the read index: rows = reads first + 4 block .. + 3, a row whose read is not H16 idle.  Two
//     round trips, no list and no list length read, so the launch does not wait for the plan: the engine starts it first and
//     runs the plan and the other classes beside it (engine.hip).  The plan then leaves an H16 read's count word to this
//     launch (VerdictsToGlobal::own_count).  A batch that is mostly H16 loses little to idle rows; any batch comes out right.
// Either way a row's read goes through the same screen_reads form: the same reads are decided and deferred.
template <int TABW>
__device__ __forceinline__ void screen_block_rows(const SweepArgs &a, u32 block, bool direct, u32 n_reads)
{
    const u32 grp = lane_id() / 16u;
    u32 r[1] = {0u};
    bool active[1] = {false};
    ReadsKnown<1> k;
    k.o[0] = 0, k.n[0] = 0, k.len[0] = 0;
    if (direct) { // (uniform)
        const u32 r0 = a.first + block * 4u;
        if (r0 >= n_reads) return;
        r[0] = r0 + grp;
        if (r[0] < n_reads) {
            const ulonglong2 oo = load_extent(a.off + r[0]); // off[r], off[r + 1]: one load
            k.len[0] = a.len[r[0]];                           // (beside the extent, not behind it: of an idle row as well)
            active[0] = is_h16(oo.y - oo.x);
            k.o[0] = oo.x, k.n[0] = (u32)(oo.y - oo.x);
        }
        if (__builtin_amdgcn_ballot_w64(active[0]) == 0) return; // uniform: no H16 read among the four
    } else {
        const u32 list_n = *a.list_n;
        const u32 idx0 = a.first + block * 4u;
        if (idx0 >= list_n) return; // grids may be sized for more reads than the class holds
        active[0] = idx0 + grp < list_n;
        if (active[0]) {
            r[0] = a.list[idx0 + grp];
            const ulonglong2 oo = load_extent(a.off + r[0]);
            k.len[0] = a.len[r[0]];
            k.o[0] = oo.x, k.n[0] = (u32)(oo.y - oo.x);
        }
    }
    screen_reads<16, 1, false, 1, 32, 32, true, TABW>(a, r, active, VerdictsToGlobal{a, direct}, &k);
}

} // namespace yk
