// edit_table.h — the name table the editors share: gpu_edit.hip (overlap files) and gpu_seq_edit.hip (FASTQ and FASTA).  The
// reads' names uploaded once (EdTableOwner, which holds the buffers); an open-addressing table keyed by the name bytes
// (gp_hash), a slot names a read, an id is compared against the uploaded bytes.  ed_lookup answers the read's type, ed_find
// the read itself.
#pragma once
#include "gpu_text.h"

namespace yk {

struct EdTable {
    const unsigned char *names; // the reads' names, back to back
    const u64 *name_off;        // [n_reads + 1]
    const unsigned char *type;  // [n_reads]
    u32 *slots;                 // [mask + 1]: 0 = empty, else read + 1
    u32 mask;
    u32 n_reads;
};

static __global__ __launch_bounds__(256) void ed_table_kernel(EdTable t)
{
    const u32 r = blockIdx.x * 256u + threadIdx.x;
    if (r >= t.n_reads) return;
    const u64 o = t.name_off[r];
    const GpBytes names{t.names};
    u32 s = (u32)gp_hash(names, o, (u32)(t.name_off[r + 1] - o)) & t.mask;
    while (atomicCAS(&t.slots[s], 0u, r + 1u) != 0u) s = (s + 1u) & t.mask; // (names are unique: no slot is ours already)
}

// the type of the read named text[p, p + len): 0 (NotBad) when the table does not hold it
__device__ __forceinline__ u32 ed_lookup(const EdTable &tab, const GpText &t, u64 p, u32 len)
{
    u32 s = (u32)gp_hash(t, p, len) & tab.mask;
    for (;;) {
        const u32 v = tab.slots[s];
        if (v == 0u) return 0u;
        const u64 o = tab.name_off[v - 1u];
        if (tab.name_off[v] - o == (u64)len) {
            u32 i = 0;
            while (i < len && (u32)tab.names[o + i] == t[p + i]) i++;
            if (i == len) return tab.type[v - 1u];
        }
        s = (s + 1u) & tab.mask;
    }
}

// the read named t[p, p + len): kEdNoRead when the table does not hold it
constexpr u32 kEdNoRead = 0xFFFFFFFFu;
template <class Text>
__device__ __forceinline__ u32 ed_find(const EdTable &tab, const Text &t, u64 p, u32 len)
{
    u32 s = (u32)gp_hash(t, p, len) & tab.mask;
    for (;;) {
        const u32 v = tab.slots[s];
        if (v == 0u) return kEdNoRead;
        const u64 o = tab.name_off[v - 1u];
        if (tab.name_off[v] - o == (u64)len) {
            u32 i = 0;
            while (i < len && (u32)tab.names[o + i] == t[p + i]) i++;
            if (i == len) return v - 1u;
        }
        s = (s + 1u) & tab.mask;
    }
}

} // namespace yk

namespace yke {

// The table's buffers in HBM: a member of an editor's scratch, so they stay with the engine and go with yacrd_engine_trim /
// destroy.  upload: R reads' names (name_bytes of them), name offsets and types -> HBM and the table of `cap` slots (a power of
// two, >= 2 R) over the names, on the engine's stream; the caller waits for the stream.  No read or no name byte: nothing of
// that is copied, and without a read nothing is launched.
struct EdTableOwner {
    DevBuf names, name_off, types, slots;
    int upload(yacrd_engine *e, const char *h_names, const uint64_t *h_name_off, const uint8_t *h_type, u64 R, u64 name_bytes, u64 cap, yk::EdTable *tab)
    {
        HIP_TRY(names.reserve((size_t)name_bytes + 64));
        HIP_TRY(name_off.reserve((size_t)(R + 1) * sizeof(u64)));
        HIP_TRY(types.reserve((size_t)R + 64));
        HIP_TRY(slots.reserve((size_t)cap * sizeof(u32)));
        HIP_TRY(hipMemsetAsync(slots.p, 0, (size_t)cap * sizeof(u32), e->stream));
        tab->names = names.as<unsigned char>(), tab->name_off = name_off.as<u64>(), tab->type = types.as<unsigned char>();
        tab->slots = slots.as<u32>(), tab->mask = (u32)(cap - 1), tab->n_reads = (u32)R;
        if (!R) return YACRD_OK;
        if (name_bytes)
            if (const int rch = h2d(e, names.p, h_names, (size_t)name_bytes)) return rch;
        if (const int rch = h2d(e, name_off.p, h_name_off, (size_t)(R + 1) * sizeof(u64))) return rch;
        if (const int rch = h2d(e, types.p, h_type, (size_t)R)) return rch;
        hipLaunchKernelGGL(yk::ed_table_kernel, dim3((u32)((R + 255) / 256)), dim3(256), 0, e->stream, *tab);
        return YACRD_OK;
    }
};

} // namespace yke
