// bgzf_sizes.h — the sizes of a BGZF stream that the encoder (deflate_block.h, also compiled for the host) and the host
// code that sizes buffers for its members (gpu_deflate.hip, gpu_edit.hip through engine_internal.h) agree on.  Plain C++.
#pragma once
#include <stdint.h>

namespace ydf {

constexpr uint32_t kBlock = 65280;  // bytes of text per member (bgzip's 0xff00)
constexpr uint32_t kSlot = 65536;   // a member never exceeds this
constexpr uint32_t kEofBytes = 28;  // the EOF member

} // namespace ydf
