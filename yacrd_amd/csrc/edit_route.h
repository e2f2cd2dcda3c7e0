// edit_route.h — how an overlap edit runs (gpu_edit.hip): the whole text at once, in windows of W bytes, or not on
// the device at all.  Plain C++, no HIP: shared by the engine library and the host library (host/inflate_host.cc:
// yacrd_edit_window_route, for the tests without a GPU).  The decision is a pure function of four inputs; what the device
// holds in a run in windows follows from W alone.
#pragma once
#include <cstdint>

namespace yer {

constexpr uint64_t kTile = 32768;                    // gpu_text.h: kGpTile
constexpr uint64_t kChunkMax = (uint64_t)4 << 20;    // gpu_text.h: kTextChunk
constexpr uint64_t kWindowDefault = (uint64_t)128 << 20; // the mover's segment (gpu_edit.hip: kSegBytes)
constexpr uint64_t kGzBlock = 65280;                 // deflate_block.h: ydf::kBlock
// Every text of more than one window in windows, also where the whole text fits?  Decided by measurement, by the rule the
// CLI's routes are decided by: true only if the slowest run in windows is under the fastest whole-text run on both files of
// DESIGN 7b.  Measured (DESIGN 7n's table): on a par, not under — false.
constexpr bool kEdWindowsWhenFits = false;
// The same question for a BGZF text, by the same rule.  Not measured under its fastest whole-text run — false.
constexpr bool kEdBgzfWindowsWhenFits = false;

enum Route { kWhole = 0, kWindows = 1, kFallback = 2 };

// the window the switch names (yacrd_debug_edit_window: 0 the policy, UINT64_MAX never windows, else rounded up to a tile)
inline uint64_t window_of(uint64_t sw)
{
    if (sw == 0 || sw == UINT64_MAX) return kWindowDefault;
    if (sw > UINT64_MAX - kTile) return UINT64_MAX / kTile * kTile;
    return (sw + kTile - 1) / kTile * kTile;
}
// what one pread and one copy move, and how far a window's marks see into the next one
inline uint64_t chunk_of(uint64_t W) { return W < kChunkMax ? W : kChunkMax; }

// n: bytes of text; sw: the switch; whole_fits: the whole-text run finds room; ring_fits: the ring of a run in windows does
inline Route route(uint64_t n, uint64_t sw, bool whole_fits, bool ring_fits, bool when_fits = kEdWindowsWhenFits)
{
    const uint64_t W = window_of(sw);
    if (n <= W || sw == UINT64_MAX) return whole_fits ? kWhole : kFallback; // (at most one window, or never windows: as before)
    if (sw != 0 || when_fits || !whole_fits) return ring_fits ? kWindows : kFallback;
    return kWhole;
}

// a text slot: [16 front pad: its last byte is the byte in front of the window][W new bytes][C look-ahead][64 zero bytes]
inline uint64_t text_slot_bytes(uint64_t W) { return 16 + W + chunk_of(W) + 64; }
// an output slot: a window keeps at most its own W bytes and the newline the text's last line may lack; gzip out: behind
// the ragged tail of the window before (less than a block)
inline uint64_t out_slot_bytes(uint64_t W, bool gzip) { return W + (gzip ? kGzBlock : 0) + 64; }

} // namespace yer
