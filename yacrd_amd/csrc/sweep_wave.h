// sweep_wave.h — small classes (<= 1024 events): one, two or four reads per wavefront, sorted in
// registers; a coverage pre-filter in front of the sort for the 16-keys-per-lane classes, or — in
// long launches — a screen that finishes healthy reads in closed form and leaves the sort to a
// the follow-on kernel for the rest (screen_reg.h: healthy_screen; finish_compact.h).
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
#include "screen_reg.h"
#include "wave_ops.h"

namespace yk {

constexpr u32 kPadKey = 0xFFFFFFFEu;

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
#ifndef YK_DEFER_OCC
#define YK_DEFER_OCC 6
#endif
// wavefronts per workgroup of the fused launch: the deferring build runs one-wavefront workgroups (a
// slot is free again as soon as its wavefront ends, not when the slowest of four does)
constexpr int kFusedWaves = 4, kDeferWaves = 1, kDeferOcc = YK_DEFER_OCC;
static_assert(kDeferWaves == 1, "screen_block indexes list entries by workgroup: one wavefront each");
struct FusedArgs {
    SweepArgs base;           // list / list_n filled per class from the table below
    u32 n_entries;
    u32 cls[5];               // CLS_R2 .. CLS_H16
    u32 block_end[5];         // running end of the per-class grids
    u32 first[5];             // SweepArgs.first per class
    const u32 *list[5];
    const u32 *list_n[5];
    u32 direct;               // the long launch's H16 rows by read index (screen_reg.h: screen_block_rows): one entry, CLS_H16, no list
    u32 n_reads;              // ... the batch's reads
};

template <bool DEFER, int WPB, int ITEMS = 1, bool WIDE = false>
__device__ __forceinline__ void sweep_small_fused_body(const FusedArgs &f)
{
    // Workgroups are dealt out to the 8 XCDs round robin (XCD = blockIdx.x mod 8); reads that are
    // neighbours in a class list are neighbours in memory and share cache lines at their boundaries,
    // so every XCD (its own L2) gets one contiguous eighth of the grid instead of every 8th workgroup.
    u32 g = blockIdx.x;
    {
        const u32 nb = gridDim.x, x = g & 7u, q = nb >> 3, rem = nb & 7u;
        g = x * q + min(x, rem) + (g >> 3);
    }
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
    // the long launch (two items, no second looks): H16 reads four per wavefront on 16-lane rows (screen_reg.h: H16 ROWS);
    // R16 keeps its two items of four reads on the same, larger table
    constexpr bool ROWS = DEFER && ITEMS == 2 && !WIDE;
    constexpr int TABW = ROWS ? kScreenTabWordsRows : kScreenTabWords;
    switch (f.cls[e]) { // the one-read-per-wavefront classes stay separate kernels (registers)
    case CLS_R2: sweep_group_block<16, 2, WPB>(a, b); break;
    case CLS_R4: sweep_group_block<16, 4, WPB>(a, b); break;
    case CLS_R8: sweep_group_block<16, 8, WPB>(a, b); break;
    case CLS_R16:
        if constexpr (DEFER) screen_block<16, ITEMS, WIDE, 16, 16, (ITEMS >= 2), TABW>(a, b);
        else sweep_group_block<16, 16, WPB>(a, b);
        break;
    default:
        if constexpr (ROWS) screen_block_rows<TABW>(a, b, f.direct != 0u, f.n_reads);
        else if constexpr (DEFER) screen_block<32, ITEMS, WIDE>(a, b);
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
