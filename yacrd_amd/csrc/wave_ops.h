// wave_ops.h — wavefront primitives of the register-sort classes and the screens: lane exchanges on DPP and the
// LDS crossbar, wave64 / 16-lane-row / lane-group scans, the per-lane constants of the bitonic network (LaneConst),
// the bitonic sort over keys held in registers, and the compiler-only fence around a wavefront's LDS exchanges.
// Touches no memory: sweep_wave.h (the sorts), screen_reg.h (the screen) and the workgroup classes build on it.
#pragma once
#include "device_common.h"

namespace yk {

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

__device__ __forceinline__ void wave_lds_sync()
{
    // LDS operations of one wavefront execute in order; this only stops the compiler from moving
    // LDS accesses across the point where lanes exchange data through LDS.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

} // namespace yk
