// deflate_host.cc — the device encoder's text (../deflate_block.h) compiled for the host: one thread plays the 256 of a
// workgroup, phase by phase.  It is the yardstick of the GPU's bytes (tests compare them) and lets the code-length
// construction be checked without a GPU; nobody's fast path.
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>

#include "../../../include/yacrd_host.h"
#include "../deflate_block.h"
#include "host_common.h"

extern "C" {

int yacrd_bgzf_encode_host(const char *data, uint64_t n, char **out, uint64_t *out_bytes)
{
    if ((!data && n) || !out || !out_bytes) return yh::fail("bad argument");
    *out = nullptr, *out_bytes = 0;
    const uint64_t n_blocks = (n + ydf::kBlock - 1) / ydf::kBlock;
    std::unique_ptr<ydf::DfShared> sh(new (std::nothrow) ydf::DfShared());
    char *res = (char *)std::malloc((size_t)(n_blocks * ydf::kSlot + ydf::kEofBytes));
    void *slot = nullptr, *src = nullptr;
    if (posix_memalign(&slot, 16, ydf::kSlot) != 0) slot = nullptr;
    if (posix_memalign(&src, 16, ydf::kSlot) != 0) src = nullptr;
    if (!sh || !res || !slot || !src) {
        std::free(res), std::free(slot), std::free(src);
        return yh::fail("host allocation failed");
    }
    uint64_t at = 0;
    for (uint64_t b = 0; b < n_blocks; b++) {
        const uint32_t len = (uint32_t)std::min<uint64_t>(ydf::kBlock, n - b * ydf::kBlock);
        std::memcpy(src, data + b * ydf::kBlock, len);
        uint32_t member = 0, stored = 0;
        ydf::df_encode_block(*sh, (const ydf::u8 *)src, len, (ydf::u8 *)slot, &member, &stored);
        std::memcpy(res + at, slot, member);
        at += member;
    }
    for (uint32_t j = 0; j < ydf::kEofBytes; j++) res[at++] = (char)ydf::df_eof_byte(j);
    std::free(slot), std::free(src);
    *out = res, *out_bytes = at;
    return 0;
}

void yacrd_bytes_free(char *p) { std::free(p); }

int yacrd_deflate_code_lengths(const uint32_t *freq, uint32_t n, uint32_t limit, uint8_t *len)
{
    if (!freq || !len || n < 2 || n > ydf::kLit || limit < 5 || limit > 15 || (1u << limit) < n) return yh::fail("bad argument");
    std::unique_ptr<ydf::DfShared> sh(new (std::nothrow) ydf::DfShared());
    if (!sh) return yh::fail("host allocation failed");
    ydf::df_code_lengths(*sh, freq, n, limit, len);
    return 0;
}

} // extern "C"
