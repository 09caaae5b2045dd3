// mrec_kidx.h -- the frozen key index's layout and its one probe loop, shared by mrec_kidx.hip (build, find) and the keyed lookups
// over records (mrec_q8.hip).  Contract: include/mrec.h, "frozen key index".
//
// One caller-owned, 256-byte-aligned buffer: [KidxHeader, padded to 256 bytes | S slots of 16 bytes {int64 key, int32 row, int32 0}],
// the live index's slot (MapSlot, mrec_hash.hip); row -1 = empty.  S = scratch_cap(n); home slot = mrec_hash_key((int64)key) & (S - 1),
// linear probing.  Never mutated after mrec_kidx_build, so a probe step is ONE 16-byte load and needs no atomics.
#ifndef MREC_KIDX_H_
#define MREC_KIDX_H_
#include "mrec_common.h"

// S - 1 of the index built at `mem` by mrec_kidx_build, as the HOST recorded it when it issued the build: MREC_OK, or MREC_EUNSUPPORTED
// for a buffer that is not 256-byte aligned or that no build was issued for (the magic word itself lives in device memory, which a
// capturable entry cannot read; the kernels check it again, see kidx_cap).  The slot count the kernels index with is this host value,
// never a word read from the buffer.
int mrec_kidx_host_mask(const void* mem, uint32_t* mask_out);

namespace {

constexpr uint32_t kKidxMagic = 0x5844494Bu;     // "KIDX"
constexpr int kKidxHdr = 256;                    // bytes in front of the slots

struct KidxHeader {
    uint32_t magic;
    int32_t max_probe;    // device-written: the longest displacement + 1 of any stored key (0: an empty index)
    int64_t S;
    int64_t n;            // keys handed to the build (key -1 and negative rows among them, which it skipped)
};

// The probe cap of a launch: max_probe, held to S; 0 -- every key misses -- where the header is not the one the host recorded.
__device__ __forceinline__ int kidx_cap(const uint8_t* __restrict__ mem, uint32_t mask) {
    const KidxHeader* const h = (const KidxHeader*)mem;
    const int mp = h->max_probe;
    const bool ok = h->magic == kKidxMagic && h->S == (int64_t)mask + 1 && mp > 0;
    return ok ? ((uint32_t)mp > mask ? (int)mask + 1 : mp) : 0;
}

// The row of `key`, or -1: at most `cap` slots from the key's home, ending early at an empty slot.  The trip count is bounded by cap
// whatever the buffer holds; the slot number by mask.  Key -1 (the padding key) is never stored and never probed.
__device__ __forceinline__ int kidx_probe(const uint8_t* __restrict__ mem, uint32_t mask, int cap, int64_t key) {
    const uint4* const slot = (const uint4*)(mem + kKidxHdr);
    uint32_t s = mrec_hash_key(key) & mask;
    int row = -1;
    if (key == -1) cap = 0;
    for (int it = 0; it < cap; ++it) {
        const uint4 w = slot[s];
        const int r = (int)w.z;
        if (r == -1) break;
        if (w.x == (uint32_t)key && w.y == (uint32_t)((uint64_t)key >> 32)) { row = r; break; }
        s = (s + 1) & mask;
    }
    return row;
}

}  // namespace
#endif /* MREC_KIDX_H_ */
