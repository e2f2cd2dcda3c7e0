// sweep_wave.h — small classes (<= 1024 events): one, two or four reads per wavefront, sorted in
// registers; a coverage pre-filter in front of the sort for the 16-keys-per-lane classes, or — in
// long launches — a screen that finishes healthy reads in closed form and leaves the sort to a
// the follow-on kernel for the rest (healthy_screen; finish_compact.h).
//
// Same event formulation as sweep_lds.h (reference src/stack.rs:61-139 for regular reads), but
// the dominant cost — sorting the 2n event keys — runs as a bitonic network over VGPRs:
//   * a lane holds K consecutive keys of the sequence (element index = lane*K + r), so strides
//     < K are register-to-register min/max and the post-sort scans are lane-sequential;
//   * strides >= K exchange between lanes: DPP moves for lane xor 1, 2, 8 (VALU only),
//     ds_swizzle for xor 4, 16 and ds_bpermute for xor 32 (the LDS crossbar is otherwise idle,
//     no LDS memory is touched), each followed by ONE v_med3_u32: med3(x, partner, 0) = min,
//     med3(x, partner, ~0) = max, the third operand being a per-lane constant that encodes
//     "upper lane of the pair" xor "descending block".
// The sort touches no LDS memory and no barrier: a 256-thread workgroup is four independent
// wavefronts (the pre-filter keeps a small histogram and its survivors in LDS, per wavefront).
// Pads are end-like keys (0xFFFFFFFE) and depth compares are signed, so nothing after the sort
// needs a validity mask (a read without intervals falls out as [(0,len)] on its own).
// Reads of <= 128 intervals use 16-lane groups: four reads per wavefront (see sweep_group_read).
#pragma once
#include <type_traits>

#include "device_common.h"

namespace yk {

constexpr u32 kPadKey = 0xFFFFFFFEu;

__device__ __forceinline__ u32 umed3(u32 a, u32 b, u32 c)
{
    return max(min(a, b), min(max(a, b), c)); // -> v_med3_u32
}

// DPP controls (gfx9): quad_perm[1,0,3,2], quad_perm[2,3,0,1], row_ror:8, row_shr:n, wave_shr:1
constexpr int DPP_XOR1 = 0xB1, DPP_XOR2 = 0x4E, DPP_ROR8 = 0x128;
constexpr int DPP_ROW_SHR1 = 0x111, DPP_ROW_SHR2 = 0x112, DPP_ROW_SHR4 = 0x114,
              DPP_ROW_SHR8 = 0x118, DPP_WAVE_SHR1 = 0x138, DPP_BCAST15 = 0x142,
              DPP_BCAST31 = 0x143;

// value of lane ^ D: DPP for xor 1/2/8, LDS crossbar (ds_swizzle / ds_bpermute) for 4/16/32.
// (The crossbar for every stride — fewest VALU instructions — was an A/B switch until round 6.)
template <int D>
__device__ __forceinline__ u32 lane_xor(u32 x, u32 bperm_addr32)
{
    if constexpr (D == 32) return (u32)__builtin_amdgcn_ds_bpermute((int)bperm_addr32, (int)x);
    else if constexpr (D == 4 || D == 16)
        return (u32)__builtin_amdgcn_ds_swizzle((int)x, (D << 10) | 0x1F);
    else if constexpr (D == 1) return (u32)__builtin_amdgcn_mov_dpp((int)x, DPP_XOR1, 0xF, 0xF, false);
    else if constexpr (D == 2) return (u32)__builtin_amdgcn_mov_dpp((int)x, DPP_XOR2, 0xF, 0xF, false);
    else return (u32)__builtin_amdgcn_mov_dpp((int)x, DPP_ROR8, 0xF, 0xF, false);
}

// wave64 inclusive scans on DPP (row_shr 1/2/4/8, row_bcast 15/31); identity 0
#define YK_DPP0(v, ctrl, rm) (u32) __builtin_amdgcn_update_dpp(0, (int)(v), ctrl, rm, 0xF, true)
__device__ __forceinline__ u32 wscan_add(u32 v)
{
    v += YK_DPP0(v, DPP_ROW_SHR1, 0xF);
    v += YK_DPP0(v, DPP_ROW_SHR2, 0xF);
    v += YK_DPP0(v, DPP_ROW_SHR4, 0xF);
    v += YK_DPP0(v, DPP_ROW_SHR8, 0xF);
    v += YK_DPP0(v, DPP_BCAST15, 0xA);
    v += YK_DPP0(v, DPP_BCAST31, 0xC);
    return v;
}
__device__ __forceinline__ u32 wscan_max(u32 v)
{
    v = max(v, YK_DPP0(v, DPP_ROW_SHR1, 0xF));
    v = max(v, YK_DPP0(v, DPP_ROW_SHR2, 0xF));
    v = max(v, YK_DPP0(v, DPP_ROW_SHR4, 0xF));
    v = max(v, YK_DPP0(v, DPP_ROW_SHR8, 0xF));
    v = max(v, YK_DPP0(v, DPP_BCAST15, 0xA));
    v = max(v, YK_DPP0(v, DPP_BCAST31, 0xC));
    return v;
}
__device__ __forceinline__ u32 wshift_up1(u32 v) { return YK_DPP0(v, DPP_WAVE_SHR1, 0xF); }

// 16-lane (DPP row) inclusive scans: four reads per wavefront, one per row
__device__ __forceinline__ u32 rscan_add(u32 v)
{
    v += YK_DPP0(v, DPP_ROW_SHR1, 0xF);
    v += YK_DPP0(v, DPP_ROW_SHR2, 0xF);
    v += YK_DPP0(v, DPP_ROW_SHR4, 0xF);
    v += YK_DPP0(v, DPP_ROW_SHR8, 0xF);
    return v;
}
__device__ __forceinline__ u32 rscan_max(u32 v)
{
    v = max(v, YK_DPP0(v, DPP_ROW_SHR1, 0xF));
    v = max(v, YK_DPP0(v, DPP_ROW_SHR2, 0xF));
    v = max(v, YK_DPP0(v, DPP_ROW_SHR4, 0xF));
    v = max(v, YK_DPP0(v, DPP_ROW_SHR8, 0xF));
    return v;
}
__device__ __forceinline__ u32 rscan_min(u32 v) // identity ~0: shifted-in lanes must not win
{
    v = min(v, (u32)__builtin_amdgcn_update_dpp(-1, (int)v, DPP_ROW_SHR1, 0xF, 0xF, false));
    v = min(v, (u32)__builtin_amdgcn_update_dpp(-1, (int)v, DPP_ROW_SHR2, 0xF, 0xF, false));
    v = min(v, (u32)__builtin_amdgcn_update_dpp(-1, (int)v, DPP_ROW_SHR4, 0xF, 0xF, false));
    v = min(v, (u32)__builtin_amdgcn_update_dpp(-1, (int)v, DPP_ROW_SHR8, 0xF, 0xF, false));
    return v;
}
__device__ __forceinline__ u32 rshift_up1(u32 v) { return YK_DPP0(v, DPP_ROW_SHR1, 0xF); }

struct LaneConst {
    u32 k[7];   // k[i] = (lane & (1<<i)) ? ~0u : 0u for i < 6; k[6] = 0
    u32 addr32; // byte address of lane ^ 32 for ds_bpermute
};

__device__ __forceinline__ LaneConst make_lane_const(u32 lane)
{
    LaneConst lc;
#pragma unroll
    for (int i = 0; i < 6; i++) lc.k[i] = (lane & (1u << i)) ? 0xFFFFFFFFu : 0u;
    lc.k[6] = 0;
    lc.addr32 = (lane ^ 32u) << 2;
    return lc;
}

constexpr int ilog2c(int v) { return v <= 1 ? 0 : 1 + ilog2c(v >> 1); }

// ---- bitonic sort of LANES*K keys held as x[K] per lane, element index = lane_in_group*K + r --
// LANES = 64: one sequence per wavefront; LANES = 16: four independent sequences, one per DPP row.
template <int LANES, int K, int M, int J>
__device__ __forceinline__ void bitonic_step(u32 (&x)[K], const LaneConst &lc)
{
    constexpr int P = LANES * K;
    constexpr bool lane_dir = (M >= K) && (M < P); // direction bit lives in the lane id
    const u32 dirm = lane_dir ? lc.k[ilog2c(M / K)] : 0u;
    if constexpr (J >= K) { // partner in another lane
        constexpr int D = J / K;
        const u32 sel = lc.k[ilog2c(D)] ^ dirm; // ~0: this lane keeps the larger key
#pragma unroll
        for (int r = 0; r < K; r++) {
            const u32 t = lane_xor<D>(x[r], lc.addr32);
            x[r] = umed3(x[r], t, sel);
        }
    } else { // partner in another register of the same lane
#pragma unroll
        for (int r = 0; r < K; r++) {
            if ((r & J) == 0) {
                const u32 a = x[r], b = x[r | J];
                if constexpr (M < K) {
                    const bool desc = (r & M) != 0;
                    x[r] = desc ? max(a, b) : min(a, b);
                    x[r | J] = desc ? min(a, b) : max(a, b);
                } else if constexpr (lane_dir) {
                    x[r] = umed3(a, b, dirm);
                    x[r | J] = umed3(a, b, ~dirm);
                } else {
                    x[r] = min(a, b);
                    x[r | J] = max(a, b);
                }
            }
        }
    }
}
template <int LANES, int K, int M, int J>
__device__ __forceinline__ void bitonic_level(u32 (&x)[K], const LaneConst &lc)
{
    bitonic_step<LANES, K, M, J>(x, lc);
    if constexpr (J > 1) bitonic_level<LANES, K, M, J / 2>(x, lc);
}
template <int LANES, int K, int M>
__device__ __forceinline__ void bitonic_sort(u32 (&x)[K], const LaneConst &lc)
{
    bitonic_level<LANES, K, M, M / 2>(x, lc);
    if constexpr (M < LANES * K) bitonic_sort<LANES, K, M * 2>(x, lc);
}

// ---- one read per group of LANES lanes, K keys per lane ------------------------------------
// LANES = 64: one read per wavefront.  LANES = 16: four reads per wavefront, one per DPP row — every
// cross-lane step then stays inside a row (10 cross-lane sort stages instead of 21, 4-step scans
// instead of 6) and is shared by four reads.  Arguments are per lane but uniform inside a group.
// The last lane of the group owns the inclusive scan totals and finishes the read.
// 32-lane groups (two reads per wavefront) are row scans plus the row_bcast:15 step.
template <int LANES>
__device__ __forceinline__ u32 gscan_add(u32 v)
{
    if (LANES == 64) return wscan_add(v);
    v = rscan_add(v);
    if (LANES == 32) v += YK_DPP0(v, DPP_BCAST15, 0xA);
    return v;
}
template <int LANES>
__device__ __forceinline__ u32 gscan_max(u32 v)
{
    if (LANES == 64) return wscan_max(v);
    v = rscan_max(v);
    if (LANES == 32) v = max(v, YK_DPP0(v, DPP_BCAST15, 0xA));
    return v;
}
template <int LANES>
__device__ __forceinline__ u32 gshift_up1(u32 v)
{
    if (LANES == 16) return rshift_up1(v);
    const u32 t = wshift_up1(v);
    if (LANES == 32) return (lane_id() == 32u) ? 0u : t; // lane 32 opens the second group
    return t;
}
template <int LANES>
__device__ __forceinline__ u32 gscan_min(u32 v)
{
    v = rscan_min(v);
    if (LANES >= 32)
        v = min(v, (u32)__builtin_amdgcn_update_dpp(-1, (int)v, DPP_BCAST15, 0xA, 0xF, false));
    if (LANES == 64)
        v = min(v, (u32)__builtin_amdgcn_update_dpp(-1, (int)v, DPP_BCAST31, 0xC, 0xF, false));
    return v;
}

// ---- everything after the event keys are in registers: sort, sweep, regions out ---------------
// m = number of real keys of the group (the rest are pads); zl_check = the wavefront holds >= 2
// zero-length intervals (duplicates must be looked for after the sort).
template <int LANES, int K>
__device__ __forceinline__ void sweep_group_keys(u32 (&x)[K], u32 m, u32 len, i32 c,
                                                 bool active, u32 r, u64 badmask, u64 zmask,
                                                 bool zl_check, const SweepArgs &a,
                                                 const LaneConst &lc)
{
    const u32 lane = lane_id(), lig = lane & (u32)(LANES - 1);
    // the read's region slot, looked up again where it is needed (rarely, and by few lanes):
    // kept as a pointer it costs two registers from the loads to the last line
    auto slot_of = [&]() {
        u32 rr = r;
        asm volatile("" : "+v"(rr)); // keeps the address arithmetic here instead of hoisted and spilled
        return a.stage + (a.off[rr] + 2 * (u64)rr);
    };

    bitonic_sort<LANES, K, 2>(x, lc);

    // two zero-length intervals at one position cannot be expressed by the keys: after the sort
    // they are adjacent equal class-1 keys.  Only looked for when the wavefront saw >= 2 of them.
    if (zl_check) {
        bool dup = false;
#pragma unroll
        for (int q = 0; q + 1 < K; q++) dup |= x[q] == x[q + 1] && (x[q] & 3u) == 1u && x[q] != 1u;
        const u32 prev = gshift_up1<LANES>(x[K - 1]);
        dup |= lig != 0 && prev == x[0] && (prev & 3u) == 1u && prev != 1u;
        badmask |= __builtin_amdgcn_ballot_w64(dup);
    }
    const bool group_bad = LANES == 64   ? badmask != 0
                           : LANES == 32 ? (u32)(badmask >> (lane & 32u)) != 0
                                         : ((u32)(badmask >> (lane & 48u)) & 0xFFFFu) != 0;

    // ---- pass 1: depth carried into each lane
    u32 n_starts = 0; // net depth change of the lane = starts - ends = 2 * starts - K
#pragma unroll
    for (int q = 0; q < K; q++) n_starts += x[q] & 1u;
    const u32 delta = 2u * n_starts - (u32)K;
    const u32 dincl = gscan_add<LANES>(delta);
    const i32 depth_in = (i32)(dincl - delta);

    // ---- pass 2: last flagged end / last low start of the lane (keys ascend, so last = max)
    // Passes 2 and 3 (straight-line per variant so the per-key depth / flag values are shared):
    //   pass 2  last flagged end / last low start of the lane (keys ascend, so last = max)
    //   pass 3  regions closed in this lane; tail rule candidates (stack.rs:93-105)
    // Flagged ends are carried between lanes in the flipped domain tk = key ^ 2
    // (device_common.h).  A wavefront without zero-length intervals (all but ~0.1 % of them) only
    // holds classes 0 and 3, where "effective" is plain "flagged" and the loops stay in the true
    // key domain (ZL = false).
    // an end is in the tail when every start precedes it: starts before = (index + depth) / 2
    const u32 tail_base = m - lig * (u32)K;
    const u32 len_key = len > kMaxKeyPos ? 0xFFFFFFFFu : (len << kKeyShift);
    u32 mf_incl, ml_incl, mf_in, ml_in;
    u32 cnt = 0, fb = 0, fe = 0, cand = kNoKey;
    // The loops carry dd = depth + (index inside the lane): one instruction per key (dd += 2 *
    // start bit) instead of a select and an add; "depth > c" becomes dd > c + q with c + q a
    // scalar, and the tail test (starts before == all starts) dd == tail_base.
    auto passes = [&](auto zl_tag) {
        constexpr bool ZL = decltype(zl_tag)::value;
        u32 mf = 0, ml = 0;
        i32 dd = depth_in;
#pragma unroll
        for (int q = 0; q < K; q++) {
            const u32 key = x[q], bit = key & 1u;
            const bool is_s = bit != 0, gt = dd > c + q;
            ml = (is_s && !gt) ? key : ml;
            if (ZL) mf = (!is_s && gt) ? max(mf, key ^ 2u) : mf;
            else mf = (!is_s && gt) ? key : mf;
            dd += (i32)(bit << 1);
        }
        if (!ZL) mf = mf ? (mf ^ 2u) : 0u;
        mf_incl = gscan_max<LANES>(mf);
        ml_incl = gscan_max<LANES>(ml);
        mf_in = max(gshift_up1<LANES>(mf_incl), kNoFlag);
        ml_in = gshift_up1<LANES>(ml_incl);

        u32 tc = ZL ? mf_in : (mf_in ^ 2u); // ZL: flipped domain; else true key, "none" = 3
        u32 cml = ml_in;
        dd = depth_in;
#pragma unroll
        for (int q = 0; q < K; q++) {
            const u32 key = x[q], bit = key & 1u;
            const bool is_s = bit != 0, gt = dd > c + q;
            const bool fl = !is_s && gt, low = is_s && !gt;
            const bool eff = ZL ? (fl && (key ^ 2u) > tc) : fl;
            const u32 begin = ZL ? (tc ^ 2u) : tc;
            const bool close = eff && cml > begin;
            cnt += close ? 1u : 0u;
            fb = close ? begin : fb;
            fe = close ? cml : fe;
            const bool tail = fl && ((u32)dd == tail_base) && key >= len_key;
            cand = min(cand, tail ? (key >> kKeyShift) : kNoKey);
            tc = eff ? (ZL ? (key ^ 2u) : key) : tc;
            cml = low ? key : cml;
            dd += (i32)(bit << 1);
        }
    };
    if (zmask == 0) passes(std::false_type{}); // wave-uniform
    else passes(std::true_type{});
    i32 d;

    const bool live = active && !group_bad;
    u32 g_closed = 0;
    if (__builtin_amdgcn_ballot_w64(cnt != 0) != 0) {
        const u32 cincl = gscan_add<LANES>(cnt);
        g_closed = cincl; // meaningful on the group's last lane
        u32 pos = cincl - cnt;
        if (live && cnt == 1) {
            slot_of()[pos] = make_uint2(fb >> kKeyShift, fe >> kKeyShift);
        } else if (live && cnt > 1) { // several regions close inside one lane: replay it
            uint2 *slot = slot_of();
            u32 tc = mf_in, cml = ml_in;
            d = depth_in;
#pragma unroll
            for (int q = 0; q < K; q++) {
                const u32 key = x[q];
                const bool is_s = (key & 1u) != 0, gt = d > c;
                const bool fl = !is_s && gt, low = is_s && !gt;
                const bool eff = fl && (key ^ 2u) > tc;
                if (eff && cml > (tc ^ 2u))
                    slot[pos++] = make_uint2((tc ^ 2u) >> kKeyShift, cml >> kKeyShift);
                tc = eff ? (key ^ 2u) : tc;
                cml = low ? key : cml;
                d += is_s ? 1 : -1;
            }
        }
    }
    u32 min_ge = kNoKey;
    if (__builtin_amdgcn_ballot_w64(cand != kNoKey) != 0) min_ge = gscan_min<LANES>(cand);
    if (lig == LANES - 1 && active) { // the group's last lane holds every inclusive total
        if (group_bad) {
            a.rej_list[atomicAdd(a.rej_count, 1u)] = r;
            a.counts[r] = 0;
        } else {
            a.counts[r] = finish_read(slot_of(), g_closed, mf_incl ? (mf_incl ^ 2u) : 0u, ml_incl, min_ge, len);
        }
    }
}

// ---- coverage pre-filter (emulated and fuzzed in tests/formulation.py) -----------
// Most of a well-covered read lies deeper than `c`: nothing there can open, close or bound a bad
// region.  The read is cut into NB = LANES bins of 2^sh positions (one bin per lane).  A bin is
// *safe* when more than c intervals span it completely (start in an earlier bin, end in a later
// one): every event inside then has depth_before > c, so its starts are never low and its flagged
// ends are always superseded by a later flagged end outside (the spanning intervals still have
// to end before the depth can reach c).  Every event in a safe bin is dropped; each maximal run
// of safe bins is stood in for by |net| start (net > 0) or end (net < 0) keys at the run's first
// position, net = depth after the run - depth before it, so the depth of every surviving event is
// unchanged.  The per-bin counts come from an LDS histogram (starts | ends << 16, LDS atomics:
// the LDS pipe is otherwise idle here) and one packed row scan.  Survivors are compacted through
// LDS; if every group of the wavefront keeps <= LANES*K/2 keys the caller sorts K/2 keys per lane.
// Exactness does not depend on the bins (any under-estimate of "safe" is fine); reference
// semantics: src/stack.rs:61-139 via the event formulation above.  Only called for wavefronts
// whose intervals all end at or before their read's length (bin index < NB without a clip).
__device__ __forceinline__ void wave_lds_sync()
{
    // LDS operations of one wavefront execute in order; this only stops the compiler from moving
    // LDS accesses across the point where lanes exchange data through LDS.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// LDS scratch of one wavefront for the filter: per group LANES coarse bins + the pads' bin + two
// one-position bins, four counters each (one per lane & 3: the reads' hot bins would otherwise
// serialise the LDS atomics of a row), then the compacted keys of every group.
constexpr int kFilterTabWords = 304, kFilterKeyWords = 512;
template <int WPB> // wavefronts per workgroup
__device__ __forceinline__ u32 *wave_filter_scratch()
{
    __shared__ __attribute__((aligned(16))) u32 s_scratch[WPB][kFilterTabWords + kFilterKeyWords];
    return s_scratch[threadIdx.x >> 6];
}

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
//   * NB = LANES coarse bins of 2^sh positions, one per lane, for every other event.
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
// per group: W head-window bins + LANES coarse blocks + W tail-window bins, 16 bytes (four copies) each
constexpr int kScreenTabWords = (64 / 16) * (16 + 2 * kScreenWindow) * 4;
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
#ifndef YK_WIDE_WB
// log2 of the positions per window bin in the build with the second looks (healthy_screen: WB): the windows reach W << WB positions with
// the same table, a and b are resolved inside their bin by counting.  Built, bit-exact (104 parity tests, 3 M fuzzed reads with the second
// looks forced), and a trade, not a gain: WB = 2 (windows of 128 positions: most reads need no slide) takes configs[1] at sigma = 300 from
// 53.4 to 48.4 us per batch (the screen alone 41.1 -> 36.4 us, frac 0.24 -> 0.27; 600 more reads have an interval shorter than the window:
// 95.3 -> 94.7 % decided) and at sigma = 100 from 32.3 to 36.3 (alone 27.1 -> 30.4: the resolve and 80 registers + 24 bytes of scratch
// instead of 62 cost the reads that needed no slide anyway); WB = 1: 51.0 / 32.9 (profiles/r06/T_wb.log).  OFF.
#define YK_WIDE_WB 0
#endif
#ifndef YK_SCREEN_JUMP
// A window that came up short goes to the next event it has not seen instead of W positions on (screen_reads: the slides; emulation:
// formulation.py jump, fuzzed + enumerated: never fewer reads decided, fewer passes — 2.4 -> 2.0 for the slowest of a wavefront's four
// reads at sigma = 300).  Built, bit-exact (122 parity tests, 3.4 M fuzzed reads), and the two reductions per slide cost what the
// saved passes gain: configs[1] at sigma = 300 54.4 -> 52.6 us per batch (kernel 65.2 -> 63.5, 4 696 -> 4 551 reads left), at 100
// 32.6 -> 33.9, configs[2] at 300 1.03 -> 1.07 ms (profiles/r06/Q_jump.log).  OFF.
#define YK_SCREEN_JUMP 0
#endif
#ifndef YK_SPOT_CHECKS
// Spot checks behind a screen that failed on a block's depth only (spot_check_call below; the build with the second looks).
// Built, bit-exact (the -m gpu parity files + 3.6 M fuzzed reads with the second looks forced, profiles/r06/A_*, B_*), and they do
// what they are for — configs[1] decided 88.7 -> 94.8 % at sigma = 300, 94.9 -> 97.1 % at 100, the follow-on sorts half as many
// reads — but the screen pays more than the follow-on gains: its launch 64 -> 77 us at sigma 300 and 33 -> 47 at 100 (a
// wavefront enters when ANY of its four reads wants), the pipelined batch 56 -> 60 and 34 -> 36 us; only one batch at a
// time gains (119 -> 116).  OFF; -DYK_SPOT_CHECKS=1 builds them (behind a call that loads the read again, YK_SPOT_INLINE
// = __attribute__((noinline)) with the call's old signature, they cost the same).
#define YK_SPOT_CHECKS 0
#endif
#ifndef YK_SPOT_MAX
#define YK_SPOT_MAX 8
#endif
#ifndef YK_SPOT_INLINE
#define YK_SPOT_INLINE __forceinline__ // (on the read's intervals where they are: behind a call that loaded them again the check cost the screen 12 us of 64 at sigma 300, profiles/r06/A_*)
#endif
#ifndef YK_HOLE_FORM
// The closed form for a read with one stretch of low coverage inside (hole_form below): bit-exact (GPU tests, fuzz) and
// it decides 77 % of what the screen otherwise defers (configs[2]: 47 608 -> 11 032 reads, the deferred sweep 145 -> 68 us)
// — but its ~1000 instructions are spent by every wave-item that holds such a read, 4.5-9 % of them, inside the kernel
// that is already short of VALU issue slots: the screen 0.613 -> 0.711 ms on configs[2], 1.43 -> 1.81 ms on configs[4], the
// step 0.816 -> 0.853 / 1.77 -> 2.06 ms (profiles/r04/e_ab_hole_form.log).  Off; -DYK_HOLE_FORM=1 builds it.
#define YK_HOLE_FORM 0
#endif
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
// WB (round 6, YK_WIDE_WB; the build with the second looks only): a window bin is 2^WB positions wide — the windows reach W << WB positions
// with the same table — and a / b are resolved inside their bin by counting (resolve below).  Every interval must then be W << WB long.
template <int LANES, int WPB, bool SLID = false, int TABW = kScreenTabWords, int WB = 0>
__device__ __forceinline__ bool healthy_screen(const uint4 (&v)[4], const bool (&real0)[4], const bool (&real1)[4],
                                               u32 len, i32 c, u32 pmin, u32 pmax, HealthyRead &hr, u32 P = 0, u32 Q = 0,
                                               u32 emin = 0, u32 smax = 0xFFFFFFFFu)
{
    constexpr int NB = LANES, W = kScreenWindow, NBIN = 2 * W + NB, GROUPS = 64 / LANES, PER = W / LANES,
                  ZPER = NBIN / LANES;
    constexpr u32 kEnd = 1u << 10, kField = kEnd - 1u;
    static_assert(W % LANES == 0 && PER >= 1 && W <= 64, "window bins per lane; a window index has six bits");
    static_assert(NBIN % LANES == 0 && GROUPS * NBIN * 4 <= TABW, "scratch");
    const u32 lane = lane_id(), lig = lane & (u32)(LANES - 1), grp = lane / (u32)LANES;
    u32 *tab = wave_screen_scratch<WPB, TABW>() + grp * (u32)(NBIN * 4);
    uint4 *bins = reinterpret_cast<uint4 *>(tab);
    char *tb = reinterpret_cast<char *>(tab);

    // smallest shift with (len >> sh) < NB, but blocks of at least W positions
    const i32 bits = 32 - (i32)__builtin_clz(len | 1u) - ilog2c(NB) + (len != 0 ? 0 : -1);
    constexpr u32 WW = (u32)W << WB; // positions a window covers
    const u32 sh = (u32)max(bits, ilog2c(W) + WB);
    const u32 span = pmax - pmin, T = span - WW;

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
        u32 is, ie;
        if constexpr (WB == 0) {
            is = min(ds, (u32)W) + (ds >> sh);
            ie = (dx >> sh) + __builtin_elementwise_sub_sat(dx, T) + (u32)W;
        } else { // (a tail bin's block term comes from the bin's first position from the top: one bin per 2^WB positions)
            is = min(ds >> WB, (u32)W) + (ds >> sh);
            const u32 dbin = (span - dx) >> WB;
            ie = dx > T ? (u32)(2 * W) - dbin + ((span - (dbin << WB)) >> sh) : (u32)W + (dx >> sh);
        }
        if constexpr (SLID) { // (what the windows have passed is not counted: P and Q stand for it)
            const bool in_ramp = ds >= WW && s < emin;
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
    for (int j = 0; j < 4; j++) {
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
        const u32 it = min((u32)(2 * W) - d + ((span - (d << WB)) >> sh), (u32)(NBIN - 1)); // (clipped: an irregular group's span is anything)
        const uint4 h4 = bins[d], t4 = bins[it];
        f[q] = ((h4.x + h4.y + h4.z + h4.w) & kField) | ((t4.x + t4.y + t4.z + t4.w) & (kField << 10));
        fw += f[q];
    }
    const uint4 c4 = bins[(u32)W + lig];
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
    // One scan for the counts and the two window indices (each set in one lane only).
    const u32 w = (c4.x + c4.y + c4.z + c4.w) & ((kField << 10) | kField);
    const u32 wincl = gscan_add<LANES>(w | cand);
    const u32 ex = wincl - w;
    const i32 x = (i32)(ex & kField) - (i32)((wincl >> 10) & kField); // starts before - ends through this block
    const u32 xm = gscan_min<LANES>((w & kField) != 0u ? (u32)(x + 0x10000) : 0xFFFFFFFFu);
    // (meaningful in the group's last lane from here on)
    const i32 F = (i32)(fincl & kField) + (SLID ? (i32)P : 0), G = (i32)(fincl >> 10) + (SLID ? (i32)Q : 0);
    hr.F = F, hr.G = G;
    hr.a = pmin + (((wincl >> 20) & 63u) << WB); // (a window that never reaches c + 1 overflows these fields: F > c
    hr.b = pmax - ((wincl >> 26) << WB);         // or G > c fails then)
    if constexpr (WB > 0) {
        // resolve: a is the smallest x of its bin's 2^WB positions with (passed starts) + (counted starts <= x) >= c + 1, b the largest
        // y of its bin's with (passed ends) + (counted ends >= y) >= c + 1: the counts of all but the last position of either bin, ten
        // bits each, in one group sum per side
        static_assert(WB <= 2, "three ten-bit counts per word");
        const int last_addr = (int)((lane | (u32)(LANES - 1)) << 2);
        const u32 a0 = (u32)__builtin_amdgcn_ds_bpermute(last_addr, (int)hr.a), b0 = (u32)__builtin_amdgcn_ds_bpermute(last_addr, (int)hr.b);
        u32 ca = 0, cb = 0;
        auto tally = [&](u32 s_, u32 e_, bool real) {
            const bool s_in = real && s_ >= pmin, e_in = real && e_ <= pmax;
#pragma unroll
            for (int i = 0; i < (1 << WB) - 1; i++) {
                ca += (s_in && s_ <= a0 + (u32)i) ? (1u << (10 * i)) : 0u;
                cb += (e_in && e_ >= b0 - (u32)i) ? (1u << (10 * i)) : 0u;
            }
        };
#pragma unroll
        for (int j = 0; j < 4; j++) {
            tally(v[j].x, v[j].y, real0[j]);
            tally(v[j].z, v[j].w, real1[j]);
        }
        const u32 ta = gscan_add<LANES>(ca), tb = gscan_add<LANES>(cb); // (the group's last lane: the totals)
        u32 da = 0, db = 0;
#pragma unroll
        for (int i = 0; i < (1 << WB) - 1; i++) {
            da += ((i32)(((ta >> (10 * i)) & kField) + P) <= c) ? 1u : 0u;
            db += ((i32)(((tb >> (10 * i)) & kField) + Q) <= c) ? 1u : 0u;
        }
        hr.a += da, hr.b -= db;
    }
    i32 open0 = F; // intervals open in front of every coarse-counted start
    if constexpr (SLID) open0 += (i32)gscan_add<LANES>(ramp);
    const bool deep = xm == 0xFFFFFFFFu || (i32)(xm - 0x10000u) + open0 > c;
    return deep && F > c && G > c;
}

// ---- the bin filter without trimming (round 1): used by the builds that do not
// defer (sweep_small_fused_kernel for short launches, the one-read-per-wavefront class), where the
// 16-keys-per-lane fallback is part of the code path and this leaner filter fits 96 registers ------
template <int LANES, int K, int WPB>
__device__ __forceinline__ bool prefilter(const u32 (&x)[K], u32 n, u32 len, i32 c, u32 (&y)[K / 2],
                                          u32 &m_out)
{
    static_assert(K == 16, "a lane reads its K/2 = 8 compacted keys as two 16-byte vectors");
    constexpr int NB = LANES, CAP = LANES * K / 2, GROUPS = 64 / LANES;
    static_assert(GROUPS * (NB + 1) * 4 <= kFilterTabWords && GROUPS * CAP <= kFilterKeyWords, "scratch");
    const u32 lane = lane_id(), lig = lane & (u32)(LANES - 1), grp = lane / (u32)LANES;
    u32 *scratch = wave_filter_scratch<WPB>();
    u32 *tab = scratch + grp * (u32)((NB + 1) * 4);        // (NB bins + one for the pads) x 4 copies
    u32 *keys = scratch + kFilterTabWords + grp * (u32)CAP;
    uint4 *my_bin = reinterpret_cast<uint4 *>(tab) + lig;
    uint4 *my_keys = reinterpret_cast<uint4 *>(keys) + lig * 2u;

    // smallest shift with (len >> sh) < NB: the bin holding `len` and every later one stay unsafe
    const i32 bits = 32 - (i32)__builtin_clz(len | 1u) - ilog2c(NB) + (len != 0 ? 0 : -1);
    const u32 sh = (u32)max(bits, 0), ksh = sh + kKeyShift;

    // ---- histogram: starts in the low half of a counter, ends in the high half (LDS atomics).
    // The compacted-key area starts out as pads.
    *my_bin = make_uint4(0u, 0u, 0u, 0u);
    my_keys[0] = make_uint4(kPadKey, kPadKey, kPadKey, kPadKey);
    my_keys[1] = make_uint4(kPadKey, kPadKey, kPadKey, kPadKey);
    wave_lds_sync();
    u32 *cell0 = tab + (lig & 3u);        // this lane's copy of bin 0
    u32 *pad_cell = cell0 + NB * 4;
    u32 *cell[K];
#pragma unroll
    for (int q = 0; q < K; q++) {
        const bool real = lig + (u32)LANES * (q / 2) < n;
        u32 *p = cell0 + (x[q] >> ksh) * 4u; // positions <= len: the bin is inside the table
        cell[q] = real ? p : pad_cell;
        atomicAdd(cell[q], (q & 1) ? 0x10000u : 1u);
    }
    wave_lds_sync();
    const uint4 w4 = *my_bin;
    const u32 w = w4.x + w4.y + w4.z + w4.w;
    const u32 incl = gscan_add<LANES>(w); // packed: both halves scanned at once
    const i32 S = (i32)(w & 0xFFFFu), E = (i32)(w >> 16);
    const i32 cs = (i32)(incl & 0xFFFFu), ce = (i32)(incl >> 16);
    const i32 depth_after = cs - ce, depth_at = depth_after - (S - E);
    const bool safe = (cs - S) - ce > c && lig < (len >> sh);
    const u64 sball = __builtin_amdgcn_ballot_w64(safe);
    if (sball == 0) return false; // wave-uniform: nothing to drop
    // the group's safe bits, bit b = bin b (zeros beyond the group)
    const u64 smask = LANES == 64 ? sball
                                  : (sball >> (lane & (u32)(64 - LANES))) & ((1ull << (LANES & 63)) - 1ull);
    const bool head = safe && (((smask << 1) >> lig) & 1ull) == 0;
    const bool tail = safe && (((smask >> 1) >> lig) & 1ull) == 0;
    const u32 hv = gscan_max<LANES>(head ? (((lig + 1u) << 16) | (u32)depth_at) : 0u);
    const i32 net = tail ? depth_after - (i32)(hv & 0xFFFFu) : 0;
    const u32 nsyn = min((u32)(net < 0 ? -net : net), (u32)CAP + 1u);
    const u32 synkey = (((hv >> 16) - 1u) << ksh) | (net > 0 ? 3u : 0u);

    // ---- slots: a bin's survivors go to [base, base + S + E), a run's stand-ins to the tail
    // lane's range; counters of safe bins (and of the pads) start at CAP = "nowhere"
    const u32 mine = safe ? nsyn : (u32)(S + E);
    const u32 rincl = gscan_add<LANES>(mine);
    const u32 m = (u32)__builtin_amdgcn_ds_bpermute((int)((lane | (u32)(LANES - 1)) << 2), (int)rincl);
    if (__builtin_amdgcn_ballot_w64(m > (u32)CAP) != 0) return false; // some group keeps too much
    const u32 base = rincl - mine;
    {
        uint4 b4;
        b4.x = base;
        b4.y = b4.x + (w4.x & 0xFFFFu) + (w4.x >> 16);
        b4.z = b4.y + (w4.y & 0xFFFFu) + (w4.y >> 16);
        b4.w = b4.z + (w4.z & 0xFFFFu) + (w4.z >> 16);
        *my_bin = safe ? make_uint4(CAP, CAP, CAP, CAP) : b4;
        if (lig < 4u) tab[NB * 4 + lig] = (u32)CAP;
    }
#pragma unroll 1
    for (u32 t = 0; t < nsyn; t++) keys[base + t] = synkey;
    wave_lds_sync();
    // slot requests go out in batches of 8, all in flight before the first store needs its answer
    // (16 at once cost eight more registers than the rest of the kernel needs)
#pragma unroll
    for (int q0 = 0; q0 < K; q0 += 8) {
        u32 pos[8];
#pragma unroll
        for (int q = 0; q < 8; q++) pos[q] = atomicAdd(cell[q0 + q], 1u);
#pragma unroll
        for (int q = 0; q < 8; q++) {
            if (pos[q] < (u32)CAP) keys[pos[q]] = x[q0 + q];
        }
    }
    wave_lds_sync();
    const uint4 lo = my_keys[0], hi = my_keys[1];
    y[0] = lo.x, y[1] = lo.y, y[2] = lo.z, y[3] = lo.w;
    y[4] = hi.x, y[5] = hi.y, y[6] = hi.z, y[7] = hi.w;
    m_out = m;
    return true;
}

// ---- one read per group of LANES lanes: loads, keys, (pre-filter,) sweep ------------------------
template <int LANES, int K, int WPB = 4>
__device__ __forceinline__ void sweep_group_read(const uint2 *__restrict__ iv, u32 n, u32 len,
                                                 u32 cov, bool active, u32 r,
                                                 const SweepArgs &a, const LaneConst &lc)
{
    const u32 lane = lane_id(), lig = lane & (u32)(LANES - 1);
    const i32 c = (i32)min(cov, 0x3FFFFFFFu); // depths are <= 1024: every larger c behaves the same, and c + q cannot overflow

    // ---- coalesced interval loads (8 B/lane), keys straight into registers
    u32 x[K];
    u32 bad = 0, nz = 0;
    bool plain;
    {
        // Every load is issued before the first use (one memory latency per read, not K/2), from
        // one base pointer with the index clamped to the read's last interval: no per-load
        // branches or address arithmetic; the duplicates are turned into pads below.  A group
        // without intervals reads the first offsets instead (always mapped).
        const uint2 *src = n ? iv : reinterpret_cast<const uint2 *>(a.off);
        const u32 last = n ? n - 1u : 0u;
        uint2 v[K / 2];
#pragma unroll
        for (int j = 0; j < K / 2; j++) v[j] = src[min(lig + (u32)LANES * j, last)];
        // Plain intervals (start < end <= min(len, kMaxKeyPos)) need two instructions per key;
        // a wavefront that holds anything else (zero-length, start > end, an end beyond the read,
        // huge positions: ~0.1 % of them) re-derives its keys with the class and rejection logic
        // of make_event_keys and sorts everything (the pre-filter relies on positions <= len).
        const u32 len_c = min(len, kMaxKeyPos);
        u32 irregular = 0;
#pragma unroll
        for (int j = 0; j < K / 2; j++) {
            const bool real = lig + (u32)LANES * j < n;
            irregular |= (real && (v[j].x >= v[j].y || v[j].y > len_c)) ? 1u : 0u;
            x[2 * j] = real ? ((v[j].x << kKeyShift) | 3u) : kPadKey;
            x[2 * j + 1] = real ? (v[j].y << kKeyShift) : kPadKey;
        }
        plain = __builtin_amdgcn_ballot_w64(irregular != 0) == 0; // wave-uniform
        if (!plain) {
#pragma unroll
            for (int j = 0; j < K / 2; j++) {
                u32 ks, ke, b = 0, z = 0;
                make_event_keys(v[j], ks, ke, b, z);
                const bool real = lig + (u32)LANES * j < n;
                x[2 * j] = real ? ks : kPadKey;
                x[2 * j + 1] = real ? ke : kPadKey;
                bad |= real ? b : 0u;
                nz += real ? z : 0u;
            }
        }
    }
    const u64 badmask = __builtin_amdgcn_ballot_w64(bad != 0);
    const u64 zmask = __builtin_amdgcn_ballot_w64(nz != 0);
    if (LANES == 64 && badmask != 0) { // wave-uniform: skip the work, queue for the exact path
        if (lig == LANES - 1 && active) {
            a.rej_list[atomicAdd(a.rej_count, 1u)] = r;
            a.counts[r] = 0;
        }
        return;
    }
    // two zero-length intervals at one position: only looked for when the wavefront saw >= 2
    const bool zl_check = (zmask & (zmask - 1)) != 0 || __builtin_amdgcn_ballot_w64(nz > 2) != 0;

    if constexpr (K == 16) {
        if (a.prefilter && plain) { // uniform
            u32 y[K / 2], mf;
            if (prefilter<LANES, K, WPB>(x, n, len, c, y, mf)) {
                if (a.prefilter == 2 && lig == 0 && active) atomicAdd(&a.ctr->prefiltered, 1u);
                sweep_group_keys<LANES, K / 2>(y, mf, len, c, active, r, badmask, zmask, zl_check, a, lc);
                return;
            }
        }
    }
    sweep_group_keys<LANES, K>(x, 2 * n, len, c, active, r, badmask, zmask, zl_check, a, lc);
}

// ---- the OTHER closed form: a read with one stretch of low coverage inside (round 4) ---------------------------------
// tests/formulation.py::hole_fast_regions is the emulation (hole_screen_regions the derivation), both fuzzed against
// the oracle.  A chimera — the read yacrd exists to find — is two healthy reads back to back: the intervals that end at
// or before loR, the first start that finds c or fewer intervals open behind the covered part (L), those that start at
// or behind it (R), and k <= c that span it.  The reference's sweep (src/stack.rs:61-139) stops flagging ends on the
// left where the ends counted down from hiL = L's largest end, the k included, reach c + 1 (x: the pops from there on
// leave c or fewer in the heap, :77-79), finds the heap at k when R's first start arrives, opens a gap (x, s) at each
// of R's first c + 1 - k starts (:83-89; merged by equal begin to (x, y), :119-136) and goes on as on a healthy read:
// the regions are (0, a), (x, y), (b, len) with a, b the FIRST screen's — it found them and failed on the depth test
// of a coarse block.  What the hole adds is looked at where it lies, with the first screen's table still in LDS:
//   1. istar = the first coarse block whose depth bound failed; only it and its successor may have;
//   2. 64 sub-bins over those two blocks, the depth D0 in front of them (> c) carried through; jstar = the first
//      sub-bin that holds a start and whose bound (its own ends first) is <= c; loR = its smallest start;
//   3. hiL = the largest end <= loR, k = the intervals across loR, no start of the left half within W of hiL, no end
//      within W behind loR;
//   4. x and y from W one-position bins below hiL / above loR (k carried);
//   5. behind jstar every sub-bin that may hold a start at or behind R's smallest end must be deep again (the starts
//      in front of that end are the ramp: nothing popped yet).
// A wrong guess anywhere costs the closed form, nothing else: the read is left to the sort.
// want: this group tries (uniform in the group); gF: the first screen's F, to the whole group.  Returns the verdict
// (uniform in the group); x, y are meaningful in the group's last lane.
template <int LANES, int WPB>
__device__ __forceinline__ bool hole_form(const uint4 (&v)[4], const bool (&real0)[4], const bool (&real1)[4], u32 len, i32 c,
                                          u32 pmin, u32 pmax, i32 gF, bool want, u32 &x_out, u32 &y_out)
{
    constexpr int NB = LANES, W = kScreenWindow, NBIN = 2 * W + NB, ZPER = NBIN / LANES, NSUB = 64, PERF = NSUB / LANES,
                  PER = W / LANES;
    constexpr u32 kEnd = 1u << 10, kField = kEnd - 1u;
    static_assert(NSUB * 4 <= NBIN * 4 && 2 * W <= NBIN * 4, "the sub-bins (four copies) and the two windows fit the group's table");
    const u32 lane = lane_id(), lig = lane & (u32)(LANES - 1), grp = lane / (u32)LANES;
    const int last_addr = (int)((lane | (u32)(LANES - 1)) << 2);
    u32 *tab = wave_screen_scratch<WPB>() + grp * (u32)(NBIN * 4);
    uint4 *bins = reinterpret_cast<uint4 *>(tab);
    char *tb = reinterpret_cast<char *>(tab);
    const i32 bits = 32 - (i32)__builtin_clz(len | 1u) - ilog2c(NB) + (len != 0 ? 0 : -1);
    const u32 sh = (u32)max(bits, ilog2c(W)), fsh = sh + 1u - (u32)ilog2c(NSUB);
    const u32 gshift = lane & (u32)(64 - LANES);
    const u64 gmask = LANES == 64 ? ~0ull : ((1ull << (LANES & 63)) - 1ull);
    auto to_group = [&](u32 x) { return (u32)__builtin_amdgcn_ds_bpermute(last_addr, (int)x); }; // the last lane's value (an inclusive scan's total)
    bool ok = want;

    // ---- 1. the first screen's coarse blocks (bins W .. W + NB - 1, still in the table): which bounds failed
    u32 istar;
    {
        const uint4 c4 = bins[(u32)W + lig];
        const u32 w = (c4.x + c4.y + c4.z + c4.w) & ((kField << 10) | kField);
        const u32 wincl = gscan_add<LANES>(w);
        const i32 x = (i32)((wincl - w) & kField) - (i32)((wincl >> 10) & kField); // starts before - ends through this block
        const bool failed = ok && (w & kField) != 0u && !(x + gF > c);
        const u64 fm = (__builtin_amdgcn_ballot_w64(failed) >> gshift) & gmask;
        istar = fm ? (u32)__builtin_ctzll(fm) : 0u;
        ok = ok && fm != 0 && istar >= 1u && (fm >> istar) <= 3ull;
    }
    if (__builtin_amdgcn_ballot_w64(ok) == 0) return false; // (uniform in the wavefront)
    const u32 B0 = pmin + (istar << sh);

    // ---- 2. sub-bins over the blocks istar, istar + 1
    wave_lds_sync();
#pragma unroll
    for (int q = 0; q < ZPER; q++) bins[lig + (u32)(LANES * q)] = make_uint4(0u, 0u, 0u, 0u);
    wave_lds_sync();
    const u32 cp = (lig & 3u) * 4u;
    u32 d0 = 0; // starts - ends in front of B0 (two's complement)
    auto count = [&](u32 s, u32 e, bool real) {
        const u32 js = (s - B0) >> fsh, je = (e - B0) >> fsh; // (a position below B0 wraps far beyond the 64 sub-bins)
        d0 += (real && s < B0) ? 1u : 0u;
        d0 -= (real && e < B0) ? 1u : 0u;
        if (real && ok && js < (u32)NSUB) atomicAdd(reinterpret_cast<u32 *>(tb + ((js << 4) + cp)), 1u);
        if (real && ok && je < (u32)NSUB) atomicAdd(reinterpret_cast<u32 *>(tb + ((je << 4) + cp)), kEnd);
    };
#pragma unroll
    for (int j = 0; j < 4; j++) {
        count(v[j].x, v[j].y, real0[j]);
        count(v[j].z, v[j].w, real1[j]);
    }
    wave_lds_sync();
    const i32 D0 = (i32)to_group(gscan_add<LANES>(d0));
    ok = ok && D0 > c;
    u32 fs[PERF], fe[PERF];
    i32 dq[PERF]; // the depth entering each of this lane's sub-bins
    u32 jcand = (u32)NSUB;
    {
        u32 tot = 0;
#pragma unroll
        for (int q = 0; q < PERF; q++) {
            const uint4 b4 = bins[lig * (u32)PERF + q];
            const u32 w = b4.x + b4.y + b4.z + b4.w;
            fs[q] = w & kField, fe[q] = (w >> 10) & kField;
            tot += w & ((kField << 10) | kField);
        }
        const u32 incl = gscan_add<LANES>(tot), ex = incl - tot;
        i32 D = D0 + (i32)(ex & kField) - (i32)((ex >> 10) & kField);
#pragma unroll
        for (int q = 0; q < PERF; q++) {
            dq[q] = D;
            if (jcand == (u32)NSUB && fs[q] != 0u && D - (i32)fe[q] <= c) jcand = lig * (u32)PERF + q;
            D += (i32)fs[q] - (i32)fe[q];
        }
    }
    const u32 jstar = to_group(gscan_min<LANES>(ok ? jcand : (u32)NSUB)); // (gscan_min is an inclusive scan: the last lane holds the group's)
    ok = ok && jstar < (u32)NSUB;
    if (__builtin_amdgcn_ballot_w64(ok) == 0) return false;
    u32 lo_c = 0xFFFFFFFFu;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if (real0[j] && ((v[j].x - B0) >> fsh) == jstar) lo_c = min(lo_c, v[j].x);
        if (real1[j] && ((v[j].z - B0) >> fsh) == jstar) lo_c = min(lo_c, v[j].z);
    }
    const u32 loR = to_group(gscan_min<LANES>(lo_c));

    // ---- 3. the halves: L's largest end, the intervals across loR, R's smallest end
    u32 hi_c = 0, kc = 0, er_c = 0xFFFFFFFFu;
    bool anyL = false;
    auto halves = [&](u32 s, u32 e, bool real) {
        if (real && e <= loR) hi_c = max(hi_c, e), anyL = true;
        kc += (real && s < loR && e > loR) ? 1u : 0u;
        if (real && e > loR) er_c = min(er_c, e);
    };
#pragma unroll
    for (int j = 0; j < 4; j++) {
        halves(v[j].x, v[j].y, real0[j]);
        halves(v[j].z, v[j].w, real1[j]);
    }
    const u32 hiL = to_group(gscan_max<LANES>(hi_c));
    const i32 k = (i32)to_group(gscan_add<LANES>(kc));
    const u32 emin_r = to_group(gscan_min<LANES>(er_c));
    const bool hasL = ((__builtin_amdgcn_ballot_w64(anyL) >> gshift) & gmask) != 0;
    // a start of the left half within W of hiL (or between hiL and loR): not this closed form
    bool near = false;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        near |= real0[j] && v[j].x < loR && v[j].x + (u32)W > hiL;
        near |= real1[j] && v[j].z < loR && v[j].z + (u32)W > hiL;
    }
    const bool anynear = ((__builtin_amdgcn_ballot_w64(near) >> gshift) & gmask) != 0;
    ok = ok && hasL && k <= c && !anynear && emin_r != 0xFFFFFFFFu && emin_r - loR >= (u32)W &&
         B0 + ((jstar + 1u) << fsh) - 1u < emin_r; // (the sub-bin of loR ends in front of R's smallest end: its starts are ramp)
    if (__builtin_amdgcn_ballot_w64(ok) == 0) return false;

    // ---- 5. behind jstar: deep again wherever a start may lie at or behind R's smallest end
    {
        bool shallow = false;
#pragma unroll
        for (int q = 0; q < PERF; q++) {
            const u32 j = lig * (u32)PERF + q;
            shallow |= j > jstar && fs[q] != 0u && B0 + ((j + 1u) << fsh) - 1u >= emin_r && !(dq[q] - (i32)fe[q] > c);
        }
        ok = ok && ((__builtin_amdgcn_ballot_w64(shallow) >> gshift) & gmask) == 0;
    }
    if (__builtin_amdgcn_ballot_w64(ok) == 0) return false;

    // ---- 4. x and y: W one-position bins downwards from hiL (ends, high half) and upwards from loR (starts, low half):
    // bin d of the first W words = position hiL - d, of the next W = loR + d.  One copy: a pile sits on few positions.
    wave_lds_sync();
#pragma unroll
    for (int q = 0; q < ZPER; q++) bins[lig + (u32)(LANES * q)] = make_uint4(0u, 0u, 0u, 0u);
    wave_lds_sync();
    auto windows = [&](u32 s, u32 e, bool real) {
        const u32 dl = hiL - e, dr = s - loR; // (an end above hiL / a start below loR wraps beyond W)
        if (real && ok && dl < (u32)W) atomicAdd(tab + dl, kEnd);
        if (real && ok && dr < (u32)W) atomicAdd(tab + (u32)W + dr, 1u);
    };
#pragma unroll
    for (int j = 0; j < 4; j++) {
        windows(v[j].x, v[j].y, real0[j]);
        windows(v[j].z, v[j].w, real1[j]);
    }
    wave_lds_sync();
    u32 f[PER], fw = 0;
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const u32 d = lig * (u32)PER + q;
        f[q] = (tab[(u32)W + d] & kField) | (tab[d] & (kField << 10));
        fw += f[q];
    }
    const u32 fincl = gscan_add<LANES>(fw);
    u32 reached = 0;
    {
        const u32 k1 = (u32)min(c + 1, 0x1FF) - (u32)k; // (k <= c: at least one)
        u32 run = fincl - fw + (512u - k1) * (1u | kEnd);
#pragma unroll
        for (int q = 0; q < PER; q++) {
            run += f[q];
            reached += run & (0x200u | (0x200u << 10));
        }
    }
    const u32 cand = (((u32)PER - ((reached >> 9) & 7u)) << 20) | (((u32)PER - (reached >> 19)) << 26);
    const u32 wincl = gscan_add<LANES>(cand);
    // (meaningful in the group's last lane from here on)
    const i32 FR = (i32)(fincl & kField) + k, GL = (i32)(fincl >> 10) + k;
    y_out = loR + ((wincl >> 20) & 63u);
    x_out = hiL - (wincl >> 26);
    return ok && FR > c && GL > c;
}

// hole_form behind a CALL that loads the read's intervals AGAIN: kept in registers through the screen for the one
// wave-item in twenty that needs them here, they pushed the two-items build of the screen over its register budget
// (spilled loads at the kernel's very start).  The call takes scalars only; what it reads lies in L2 (the screen has
// just read it).  want: this group tries (uniform in the group; its reads are plain, every interval >= W long, so
// every slot below n is real).  Returns (verdict, x, y), meaningful in the group's last lane.
template <int LANES>
__device__ __attribute__((noinline)) uint4 hole_form_call(const u64 *off, const uint2 *iv, u32 r, u32 len, i32 c, u32 pmin, u32 pmax,
                                                          i32 gF, u32 want)
{
    constexpr int K = 16;
    const u32 lig = lane_id() & (u32)(LANES - 1);
    u32 n = 0;
    const uint2 *src = reinterpret_cast<const uint2 *>(off); // (a group that does not try reads the offsets: always mapped)
    if (want) {
        const ulonglong2 oo = load_extent(off + r);
        n = (u32)(oo.y - oo.x);
        src = iv + oo.x;
    }
    const u32 last2 = n >= 2u ? n - 2u : 0u;
    uint4 v[K / 4];
    bool real0[K / 4], real1[K / 4];
#pragma unroll
    for (int j = 0; j < K / 4; j++) {
        const u32 i0 = 2u * (lig + (u32)LANES * j);
        v[j] = load_pair(src + min(i0, last2));
        real0[j] = i0 + 1u < n; // (.xy is interval i0 only when i0 + 1 exists too: see screen_block)
        real1[j] = i0 < n;
    }
    u32 x = 0, y = 0;
    const bool ok = hole_form<LANES, 1>(v, real0, real1, len, c, pmin, pmax, gF, want != 0u && n >= 2u, x, y);
    return make_uint4(ok ? 1u : 0u, x, y, 0u);
}

// ---- SPOT CHECKS behind a screen that failed on a block's depth only (round 6; the build with the second looks) ----------
// tests/formulation.py::_sub_screen(spot = kSpotMax) is the emulation (fuzzed against the oracle + exhaustive over small
// multisets: tests/test_formulation.py::test_slid_window_*).  The block test counts ALL of a block's ends as before its
// starts.  At ONT depth with dovetail ends spread by hundreds of positions (configs[1] at sigma = 300) that is too coarse:
// the ends that used to pile inside the tail window's one-position bins fill a whole coarse block now, an internal start
// in that block fails the test, and 269 of 273 healthy reads the screen left to the sort in a sample of 3 000 were of
// this kind (the closed form held).  So the few coarse-counted starts of the FAILING blocks are looked at one by one: a
// start s has at least (starts at positions < s) - (ends at positions <= s) intervals open in front of it (the ends at
// or before s are popped first: src/stack.rs:72-83); more than c for each of them, and no start beyond the first c + 1 is
// low after all: the screen's (0, a) / (b, len) stand.  Decided reads: 88.5 % -> 95.1 % at sigma = 300, 94.7 % -> 97.1 %
// at 100 (emulation on the generator's reads; GPU: 88.7 -> 94.8 %, 94.9 -> 97.1 %).
// It builds the table again (what the second looks left in LDS is another group's as often as not).
// v / real0 / real1: the read's intervals where the screen has them; lo / hi: the head window's first / the tail window's
// last position of the last screen; gF: its F (passed starts included); want: this group tries (uniform in the group; its read
// is plain, every interval >= W long).  Returns 1 (uniform in the group) when every candidate start has more than c
// intervals open in front of it.
constexpr int kSpotMax = YK_SPOT_MAX;
template <int LANES, int WPB, int TABW = kScreenTabWords>
__device__ YK_SPOT_INLINE u32 spot_check_call(const uint4 (&v)[4], const bool (&real0)[4], const bool (&real1)[4], u32 len, i32 c, u32 lo, u32 hi,
                                              i32 gF, u32 want)
{
    constexpr int K = 16, NB = LANES, W = kScreenWindow, NBIN = 2 * W + NB, ZPER = NBIN / LANES;
    constexpr u32 kEnd = 1u << 10, kField = kEnd - 1u;
    const u32 lane = lane_id(), lig = lane & (u32)(LANES - 1), grp = lane / (u32)LANES;
    const int last_addr = (int)((lane | (u32)(LANES - 1)) << 2);
    const u32 gshift = lane & (u32)(64 - LANES);
    constexpr u64 gmask = LANES == 64 ? ~0ull : ((1ull << (LANES & 63)) - 1ull);
    auto to_group = [&](u32 x) { return (u32)__builtin_amdgcn_ds_bpermute(last_addr, (int)x); }; // the last lane's value
    auto group_bits = [&](bool b) { return (u64)(__builtin_amdgcn_ballot_w64(b) >> gshift) & gmask; };
    u32 st_[K / 2], en_[K / 2];
    bool real[K / 2];
#pragma unroll
    for (int j = 0; j < K / 4; j++) {
        st_[2 * j] = v[j].x, en_[2 * j] = v[j].y, st_[2 * j + 1] = v[j].z, en_[2 * j + 1] = v[j].w;
        real[2 * j] = want != 0u && real0[j];
        real[2 * j + 1] = want != 0u && real1[j];
    }
    // the read's smallest end (the ramp: starts behind the head window and in front of it are open in front of everything)
    u32 emin = 0xFFFFFFFFu;
#pragma unroll
    for (int q = 0; q < K / 2; q++) emin = min(emin, real[q] ? en_[q] : 0xFFFFFFFFu);
    const u32 gemin = to_group(gscan_min<LANES>(emin));
    // ---- the table again, as healthy_screen<SLID> counts it
    const i32 bits = 32 - (i32)__builtin_clz(len | 1u) - ilog2c(NB) + (len != 0 ? 0 : -1);
    const u32 sh = (u32)max(bits, ilog2c(W));
    const u32 T = (hi - lo) - (u32)W;
    u32 *tab = wave_screen_scratch<WPB, TABW>() + grp * (u32)(NBIN * 4);
    uint4 *bins = reinterpret_cast<uint4 *>(tab);
    char *tb = reinterpret_cast<char *>(tab);
    wave_lds_sync(); // (whoever read the table last is done)
#pragma unroll
    for (int q = 0; q < ZPER; q++) bins[lig + (u32)(LANES * q)] = make_uint4(0u, 0u, 0u, 0u);
    wave_lds_sync();
    const u32 cp = (lig & 3u) * 4u;
    u32 ramp = 0;
    u32 coarse = 0; // a bit per coarse-counted start: inside [lo, hi], behind the head window, not in the ramp
#pragma unroll
    for (int q = 0; q < K / 2; q++) {
        const u32 ds = st_[q] - lo, dx = en_[q] - lo;
        const u32 is = min(ds, (u32)W) + (ds >> sh);
        const u32 ie = (dx >> sh) + __builtin_elementwise_sub_sat(dx, T) + (u32)W;
        const bool in_ramp = ds >= (u32)W && st_[q] < gemin;
        const bool s_in = real[q] && st_[q] >= lo;
        ramp += (s_in && in_ramp) ? 1u : 0u;
        coarse |= (s_in && !in_ramp && ds >= (u32)W) ? (1u << q) : 0u;
        if (s_in && !in_ramp) atomicAdd(reinterpret_cast<u32 *>(tb + ((is << 4) + cp)), 1u);
        if (real[q] && en_[q] <= hi) atomicAdd(reinterpret_cast<u32 *>(tb + ((ie << 4) + cp)), kEnd);
    }
    wave_lds_sync();
    // ---- the failing blocks: a block that holds a coarse-counted start and not more than c intervals open after all its ends
    const uint4 c4 = bins[(u32)W + lig];
    const u32 w = (c4.x + c4.y + c4.z + c4.w) & ((kField << 10) | kField);
    const u32 wincl = gscan_add<LANES>(w);
    const i32 x = (i32)((wincl - w) & kField) - (i32)((wincl >> 10) & kField); // starts before - ends through this block
    const i32 open0 = gF + (i32)to_group(gscan_add<LANES>(ramp));
    const u64 fmask = group_bits(want != 0u && (w & kField) != 0u && !(x + open0 > c));
    // ---- the candidates: this lane's coarse-counted starts in failing blocks, a bit each
    u32 cm = 0;
#pragma unroll
    for (int q = 0; q < K / 2; q++)
        cm |= (((coarse >> q) & 1u) != 0u && ((fmask >> min((st_[q] - lo) >> sh, (u32)(LANES - 1))) & 1ull) != 0) ? (1u << q) : 0u;
    const u32 total = to_group(gscan_add<LANES>((u32)__builtin_popcount(cm)));
    bool ok = want != 0u && total <= (u32)kSpotMax;
    if (!ok) cm = 0;
#pragma unroll 1
    for (int it = 0; it < kSpotMax; it++) {
        const u64 gb = group_bits(cm != 0u);
        if (__builtin_amdgcn_ballot_w64(gb != 0) == 0) break; // (uniform in the wavefront)
        const u32 first = gb ? (u32)__builtin_ctzll(gb) : 0u; // the group's first lane with a candidate
        u32 mine = 0;
#pragma unroll
        for (int q = K / 2 - 1; q >= 0; q--) mine = ((cm >> q) & 1u) ? st_[q] : mine; // (its lowest candidate)
        const u32 sc = (u32)__builtin_amdgcn_ds_bpermute((int)(((lane & ~(u32)(LANES - 1)) + first) << 2), (int)mine);
        if (lig == first) cm &= cm - 1u;
        u32 cnt = 0; // (starts in front of sc) - (ends at or in front of it), this lane's
#pragma unroll
        for (int q = 0; q < K / 2; q++) cnt += ((real[q] && st_[q] < sc) ? 1u : 0u) - ((real[q] && en_[q] <= sc) ? 1u : 0u);
        const i32 depth = (i32)to_group(gscan_add<LANES>(cnt));
        if (gb != 0 && !(depth > c)) ok = false, cm = 0;
    }
    return ok ? 1u : 0u;
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
    __device__ __forceinline__ void closed(u32 r, u32 ra, u32 rb, u32 len) const
    {
        // counts[r] says kClosedForm since the plan kernel: ONE store per decided read, its (a, b) — or, for a read with no
        // bad region at all, the count 0 in four bytes
        if (ra != 0 || rb != len) a.closed[r] = make_uint2(ra, rb);
        else a.counts[r] = 0;
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
template <int LANES, int ITEMS, bool WIDE, int WPB = 1, class Sink>
__device__ __forceinline__ void screen_reads(const SweepArgs &a, const u32 (&r)[ITEMS], const bool (&active)[ITEMS], const Sink &sink,
                                             const ReadsKnown<ITEMS> *known = nullptr);

template <int LANES, int ITEMS, bool WIDE = false>
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
    screen_reads<LANES, ITEMS, WIDE>(a, r, active, VerdictsToGlobal{a});
}

// ITEMS reads per lane group, given by their ids (active[t]: this group has a t-th read; a t with no active group in the
// wavefront ends the loop).  WPB: wavefronts per workgroup (each has a table of its own in LDS).
template <int LANES, int ITEMS, bool WIDE, int WPB, class Sink>
__device__ __forceinline__ void screen_reads(const SweepArgs &a, const u32 (&r)[ITEMS], const bool (&active)[ITEMS], const Sink &sink,
                                             const ReadsKnown<ITEMS> *known)
{
    constexpr int K = 16;
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
            v[t][j] = load_pair<(ITEMS >= 2)>(src + min(2u * (lig + (u32)LANES * j), last2)); // (two items: the launch streams from HBM)
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
        constexpr int WBW = (kScreenSlides > 0 && WIDE) ? YK_WIDE_WB : 0; // (window bins of 2^WBW positions in the build with the second looks)
        constexpr u32 kWinPos = (u32)kScreenWindow << WBW;                // positions a window covers
        static_assert(WBW == 0 || (!YK_SPOT_CHECKS && !YK_HOLE_FORM && !YK_SCREEN_JUMP), "they count one-position windows");
        const bool irregular = n[t] < 2u || pmax > len_c || smax > kMaxKeyPos || tmin < (i32)kWinPos;
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
        bool healthy = healthy_screen<LANES, WPB, false, kScreenTabWords, WBW>(v[t], real0, real1, len[t], c, pmin, pmax, hr) && !girr;
        u32 ht_used = 0; // (the last screen's windows: h0 | t0 << 16)
        bool table_intact = true, hole_done = false; // (the first screen's coarse blocks are still in LDS; this group's read got its hole form)
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
                table_intact = false;
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
                    bool reach = true; // (the windows' offsets fit their sixteen bits and there is an event to go to)
#if YK_SCREEN_JUMP
                    // WINDOWS THAT JUMP: a window that came up short goes to the next event it has not seen — the head window begins AT
                    // the smallest start behind it, the tail window ends AT the largest end in front of it — nothing lies in between,
                    // so what it has passed is what it counted, and every pass gains at least one event (formulation.py: jump)
                    {
                        const u32 thr_h = pmin + (ht & 0xFFFFu) + (u32)kScreenWindow, thr_t = pmax - (ht >> 16) - (u32)kScreenWindow;
                        u32 ns = 0xFFFFFFFFu, pe = 0u;
#pragma unroll
                        for (int j = 0; j < K / 4; j++) {
                            ns = min(ns, min(v[t][j].x >= thr_h ? v[t][j].x : 0xFFFFFFFFu, v[t][j].z >= thr_h ? v[t][j].z : 0xFFFFFFFFu));
                            pe = max(pe, max(v[t][j].y <= thr_t ? v[t][j].y : 0u, v[t][j].w <= thr_t ? v[t][j].w : 0u));
                        }
                        const u32 gns = (u32)__builtin_amdgcn_ds_bpermute(last_addr, (int)gscan_min<LANES>(ns));
                        const u32 gpe = (u32)__builtin_amdgcn_ds_bpermute(last_addr, (int)gscan_max<LANES>(pe));
                        if (gneed && (i32)gF <= c) {
                            const u32 h = gns - pmin;
                            reach = reach && gns != 0xFFFFFFFFu && h <= 0xFFFFu;
                            ht = (ht & 0xFFFF0000u) | (h & 0xFFFFu), PQ = (PQ & 0xFFFF0000u) | gF;
                        }
                        if (gneed && (i32)gG <= c) {
                            const u32 tt = pmax - gpe;
                            reach = reach && gpe != 0u && tt <= 0xFFFFu;
                            ht = (ht & 0xFFFFu) | (tt << 16), PQ = (PQ & 0xFFFFu) | (gG << 16);
                        }
                    }
#else
                    if (gneed && (i32)gF <= c) ht += kWinPos, PQ = (PQ & 0xFFFF0000u) | gF;
                    if (gneed && (i32)gG <= c) ht += kWinPos << 16, PQ = (PQ & 0xFFFFu) | (gG << 16);
#endif
                    const u32 h0 = ht & 0xFFFFu, t0 = ht >> 16;
                    // no end at or before the head window's last position, no start at or behind the tail window's
                    // first, and the two windows apart
                    const bool go = gneed && reach && room_h >= h0 + kWinPos && room_t >= t0 + kWinPos &&
                                    pmax - pmin >= h0 + t0 + 2u * kWinPos;
                    if (__builtin_amdgcn_ballot_w64(go) == 0) break; // (uniform)
                    bool r0[K / 4], r1[K / 4];
#pragma unroll
                    for (int j = 0; j < K / 4; j++) r0[j] = real0[j] && go, r1[j] = real1[j] && go;
                    wave_lds_sync(); // (the table is zeroed again)
                    HealthyRead h2;
                    const bool ok2 = healthy_screen<LANES, WPB, true, kScreenTabWords, WBW>(v[t], r0, r1, len[t], c, pmin + h0, pmax - t0, h2, PQ & 0xFFFFu, PQ >> 16, gemin, gsmax);
                    st = go ? state_of(!ok2 && (h2.F <= c || h2.G <= c), h2) : 0u; // (meaningful in the group's last lane)
                    if (go) healthy = ok2, hr.a = h2.a, hr.b = h2.b, hr.F = h2.F, hr.G = h2.G, ht_used = ht;
                }
            }
#if YK_SPOT_CHECKS
            // the last screen found a and b and failed on a block's depth: its few coarse-counted starts one by one (spot_check_call)
            {
                const u32 pk = (u32)__builtin_amdgcn_ds_bpermute(
                    last_addr, (int)(((!healthy && !girr && (i32)n[t] > c && hr.F > c && hr.G > c && active[t]) ? 1u : 0u) | ((u32)min(max(hr.F, 0), 1023) << 1)));
                if (__builtin_amdgcn_ballot_w64((pk & 1u) != 0) != 0) { // (uniform in the wavefront; rare)
                    table_intact = false;
                    const u32 okv = spot_check_call<LANES, WPB>(v[t], real0, real1, len[t], c, pmin + (ht_used & 0xFFFFu), pmax - (ht_used >> 16),
                                                                 (i32)(pk >> 1), pk & 1u);
                    if (okv != 0u) healthy = true; // (uniform in the group: a and b stand)
                }
            }
#endif
        }
        if constexpr (YK_HOLE_FORM) {
            // the first screen found a and b and failed on a block's depth: one stretch of low coverage inside? (hole_form)
            const u32 pk = (u32)__builtin_amdgcn_ds_bpermute(
                last_addr, (int)(((!healthy && !girr && (i32)n[t] > c && hr.F > c && hr.G > c && pmax - pmin >= 2u * (u32)kScreenWindow) ? 1u : 0u) |
                                 ((u32)min(hr.F, 1023) << 1)));
            if (table_intact && __builtin_amdgcn_ballot_w64((pk & 1u) != 0) != 0) { // (uniform in the wavefront)
                const uint4 hv = hole_form_call<LANES>(a.off, a.iv, r[t], len[t], c, pmin, pmax, (i32)(pk >> 1), pk & 1u);
                const bool hole = hv.x != 0u;
                const u32 hx = hv.y, hy = hv.z;
                if (hole && lig == (u32)(LANES - 1) && active[t]) { // (three regions: through the read's slot, not closed[])
                    u32 rr = r[t];
                    asm volatile("" : "+v"(rr)); // (the offset is loaded again here, rarely, instead of kept in registers from the top)
                    uint2 *slot = a.stage + (a.off[rr] + 2 * (u64)rr);
                    u32 g = 0;
                    if (hr.a != 0u) slot[g++] = make_uint2(0u, hr.a);
                    slot[g++] = make_uint2(hx, hy);
                    if (hr.b != len[t]) slot[g++] = make_uint2(hr.b, len[t]);
                    a.counts[r[t]] = g;
                    if (a.prefilter == 2) atomicAdd(&a.ctr->prefiltered, 1u);
                }
                if (hole) healthy = false, hole_done = true;
            }
        }
        if (hole_done) {
            // (its regions are written)
        } else if (lig == (u32)(LANES - 1) && active[t]) { // the group's last lane has the verdict
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

// Body of one workgroup (four wavefronts, 4 * 64/LANES reads) of class (LANES, K).
template <int LANES, int K, int WPB = 4>
__device__ __forceinline__ void sweep_group_block(const SweepArgs &a, u32 block)
{
    const u32 lane = lane_id();
    const LaneConst lc = make_lane_const(lane);

    constexpr u32 GROUPS = 64 / LANES; // reads per wavefront
    const u32 list_n = *a.list_n;
    const u32 wave = block * (u32)WPB + (threadIdx.x >> 6);
    if (a.first + wave * GROUPS >= list_n) return; // grids may be sized for more reads than the class holds
    const u32 idx = a.first + wave * GROUPS + lane / (u32)LANES;
    const bool active = idx < list_n;
    u32 r = 0, n = 0, len = 0;
    u64 o = 0;
    if (active) {
        r = a.list[idx];
        o = a.off[r];
        n = (u32)(a.off[r + 1] - o);
        len = a.len[r];
    }
    sweep_group_read<LANES, K, WPB>(a.iv + o, n, len, a.cov, active, r, a, lc);
}

// One kernel per (LANES, K): small K keep small register footprints.
template <int LANES, int K>
__global__ __launch_bounds__(256) void sweep_group_kernel(SweepArgs a)
{
    sweep_group_block<LANES, K>(a, blockIdx.x);
}

template <int LANES, int K>
inline void launch_sweep_group(const SweepArgs &sa, u32 n_reads, hipStream_t stream)
{
    constexpr u32 per_block = 4u * (64 / LANES); // reads per 256-thread workgroup
    const u32 grid = (n_reads + per_block - 1) / per_block;
    hipLaunchKernelGGL((sweep_group_kernel<LANES, K>), dim3(grid ? grid : 1), dim3(256), 0, stream, sa);
}

// ---- every register-sort class in ONE launch ------------------------------------------------
// The classes R2..H16 are independent; launched one after the other each pays its own ramp-up
// and drain (~4-7 us for the minor ones on configs[1]).  Here the grid is the concatenation of
// the per-class grids and a workgroup looks up its class (<= 5 uniform compares).
#ifndef YK_DEFER_WAVES
#define YK_DEFER_WAVES 1
#endif
#ifndef YK_DEFER_OCC
#define YK_DEFER_OCC 6
#endif
// wavefronts per workgroup of the fused launch: the deferring build runs one-wavefront workgroups (a
// slot is free again as soon as its wavefront ends, not when the slowest of four does)
constexpr int kFusedWaves = 4, kDeferWaves = YK_DEFER_WAVES, kDeferOcc = YK_DEFER_OCC;
static_assert(kDeferWaves == 1, "screen_block indexes list entries by workgroup: one wavefront each");
struct FusedArgs {
    SweepArgs base;           // list / list_n filled per class from the table below
    u32 n_entries;
    u32 cls[5];               // CLS_R2 .. CLS_H16
    u32 block_end[5];         // running end of the per-class grids
    u32 first[5];             // SweepArgs.first per class
    const u32 *list[5];
    const u32 *list_n[5];
};

template <bool DEFER, int WPB, int ITEMS = 1, bool WIDE = false>
__device__ __forceinline__ void sweep_small_fused_body(const FusedArgs &f)
{
    // Workgroups are dealt out to the 8 XCDs round robin (XCD = blockIdx.x mod 8); reads that are
    // neighbours in a class list are neighbours in memory and share cache lines at their boundaries,
    // so every XCD (its own L2) gets one contiguous eighth of the grid instead of every 8th workgroup.
    u32 g = blockIdx.x;
#ifndef YK_NO_XCD_REMAP
    {
        const u32 nb = gridDim.x, x = g & 7u, q = nb >> 3, rem = nb & 7u;
        g = x * q + min(x, rem) + (g >> 3);
    }
#endif
    u32 e = 0, first = 0;
    while (e + 1 < f.n_entries && g >= f.block_end[e]) {
        first = f.block_end[e];
        e++;
    }
    SweepArgs a = f.base;
    a.list = f.list[e];
    a.list_n = f.list_n[e];
    a.first = f.first[e];
    const u32 b = g - first;
    switch (f.cls[e]) { // the one-read-per-wavefront classes stay separate kernels (registers)
    case CLS_R2: sweep_group_block<16, 2, WPB>(a, b); break;
    case CLS_R4: sweep_group_block<16, 4, WPB>(a, b); break;
    case CLS_R8: sweep_group_block<16, 8, WPB>(a, b); break;
    case CLS_R16:
        if constexpr (DEFER) screen_block<16, ITEMS, WIDE>(a, b);
        else sweep_group_block<16, 16, WPB>(a, b);
        break;
    default:
        if constexpr (DEFER) screen_block<32, ITEMS, WIDE>(a, b);
        else sweep_group_block<32, 16, WPB>(a, b);
        break;
    }
}
// Two builds.  DEFER: the classes R16 / H16 run the healthy-read screen (one counting pass + closed
// form) and mark every other read in counts[] for finish_compact_kernel; no sort for
// those classes in this kernel: 56 registers, one-wavefront workgroups, bound by the memory system
// (configs[1]: 47.9 -> 17.5 us, configs[2]: 1.90 -> 0.65 ms).  The other build sorts every read behind
// the bin filter: for batches whose reads mostly fail the screen (the engine looks at the previous
// batch's deferral rate) and for very short launches.
// (__launch_bounds__' second argument: wavefronts per SIMD)
__global__ __launch_bounds__(64 * kDeferWaves, kDeferOcc) void sweep_small_fused_defer_kernel(FusedArgs f)
{
    sweep_small_fused_body<true, kDeferWaves>(f);
}
// the one-item build WITH the second looks (sliding windows + ramp, §"Windows that slide"): what the engine launches after a
// batch that left more than a tenth of its screened reads to the sort.  They cost the build four registers and a tenth of its
// speed on reads that never need them (configs[1]: 24.4 -> 26.7 us per pipelined batch, profiles/r04/n_*), so the default
// builds do not carry them.
__global__ __launch_bounds__(64 * kDeferWaves, kDeferOcc) void sweep_small_fused_defer_wide_kernel(FusedArgs f)
{
    sweep_small_fused_body<true, kDeferWaves, 1, true>(f);
}
// the same with two groups of list entries per wavefront in the screened classes (long launches from HBM)
#ifndef YK_DEFER2_OCC
#define YK_DEFER2_OCC YK_DEFER_OCC
#endif
__global__ __launch_bounds__(64, YK_DEFER2_OCC) void sweep_small_fused_defer2_kernel(FusedArgs f)
{
    sweep_small_fused_body<true, 1, 2>(f);
}
__global__ __launch_bounds__(64 * kFusedWaves, 5) void sweep_small_fused_kernel(FusedArgs f)
{
    sweep_small_fused_body<false, kFusedWaves>(f);
}

inline u32 sweep_group_reads_per_block(int cls, int waves = 4)
{
    return ((cls <= CLS_R16) ? 4u : (cls == CLS_H16) ? 2u : 1u) * (u32)waves;
}

} // namespace yk
