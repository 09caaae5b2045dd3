// mrec_kidx.hip -- the frozen key index for gfx950: a read-only key -> row index over n unique int64 keys, built once for serving
// (layout and probe loop: mrec_kidx.h; the entries' contract: include/mrec.h, "frozen key index").
//
// The live index of mrec_hash.hip serves training: it inserts, erases, counts hits and rebuilds itself, and its probes must tolerate
// tombstones and concurrent inserts.  A frozen model has none of that.  What is left is the slot array alone, in the live index's
// slot format and with its hash, so that the host model of tests/_map_model.py (home_slot, fill_slots) states this index too:
//
// k_kidx_clear   every slot {key 0, row -1, 0} as one 16-byte store, a grid stride over S; thread 0 of the launch writes the header
//                (magic, max_probe = 0, S, n) and zeroes the rest of its 256 bytes.  A kernel, not a memset: the build is capturable.
// k_kidx_insert  one thread a key, a grid stride over n.  The thread walks from the key's home and claims the first empty slot with a
//                compare-and-swap of the slot's `row` from -1; slots only move -1 -> row inside the launch, so a lost CAS means
//                "taken" and the walk steps on.  The key is stored behind the claim with a plain store: no thread of this launch
//                reads a key (a claimed slot is passed by on its row word alone), and every later launch is ordered behind this one.
//                The claim's displacement + 1 goes into the header's max_probe with atomicMax -- the one word a probe loop needs to
//                bound a MISS: no key lies further from its home than that, so a probe that has looked at max_probe slots without
//                meeting an empty one is done.  Key -1 (the padding key, embedding.py:53) and negative rows are skipped.
//                Live keys <= S / 2, so an empty slot exists; the walk is bounded by S all the same.
// k_kidx_find    one thread a key, probe only (kidx_probe): one 16-byte slot load a step, int32 keys widened before hashing.
#include "mrec_kidx.h"

#include <mutex>
#include <unordered_map>

namespace {

constexpr int KB = 256;

struct KidxSlot { int64_t key; int row; int pad; };

__global__ __launch_bounds__(KB) void k_kidx_clear(uint8_t* __restrict__ mem, int64_t S, int64_t n) {
    const int64_t t0 = (int64_t)blockIdx.x * KB + threadIdx.x;
    uint4* const slot = (uint4*)(mem + kKidxHdr);
    for (int64_t s = t0; s < S; s += (int64_t)gridDim.x * KB) slot[s] = make_uint4(0u, 0u, 0xFFFFFFFFu, 0u);
    if (t0 < kKidxHdr / 16) {
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
        if (t0 == 0) w = make_uint4(kKidxMagic, 0u, (uint32_t)S, (uint32_t)((uint64_t)S >> 32));
        if (t0 == 1) w = make_uint4((uint32_t)n, (uint32_t)((uint64_t)n >> 32), 0u, 0u);
        ((uint4*)mem)[t0] = w;
    }
}

__global__ __launch_bounds__(KB) void k_kidx_insert(uint8_t* __restrict__ mem, uint32_t mask, const int64_t* __restrict__ keys,
                                                    const int* __restrict__ rows, int64_t n) {
    KidxHeader* const hdr = (KidxHeader*)mem;
    KidxSlot* const slot = (KidxSlot*)(mem + kKidxHdr);
    for (int64_t i = (int64_t)blockIdx.x * KB + threadIdx.x; i < n; i += (int64_t)gridDim.x * KB) {
        const int64_t key = keys[i];
        const int row = rows ? rows[i] : (int)i;
        if (key == -1 || row < 0) continue;
        uint32_t s = mrec_hash_key(key) & mask;
        for (uint32_t it = 0; it <= mask; ++it) {
            if (atomicCAS(&slot[s].row, -1, row) == -1) {
                slot[s].key = key;
                atomicMax(&hdr->max_probe, (int)(it < 0x7FFFFFFFu ? it + 1 : 0x7FFFFFFFu));
                break;
            }
            s = (s + 1) & mask;
        }
    }
}

template <class K>
__global__ __launch_bounds__(KB) void k_kidx_find(const uint8_t* __restrict__ mem, uint32_t mask, const K* __restrict__ keys, int64_t n,
                                                  int* __restrict__ rows_out) {
    const int cap = kidx_cap(mem, mask);
    for (int64_t i = (int64_t)blockIdx.x * KB + threadIdx.x; i < n; i += (int64_t)gridDim.x * KB)
        rows_out[i] = kidx_probe(mem, mask, cap, (int64_t)keys[i]);
}

// buffers a build was issued for -> their S - 1 (mrec_kidx.h: mrec_kidx_host_mask)
std::mutex g_kidx_mu;
std::unordered_map<const void*, uint32_t> g_kidx_built;

constexpr int64_t kKidxMaxKeys = int64_t(1) << 30;      // S <= 2^31: slot numbers and displacements fit 32 bits

}  // namespace

int mrec_kidx_host_mask(const void* mem, uint32_t* mask_out) {
    if ((((uintptr_t)mem) & 255) != 0) return MREC_EUNSUPPORTED;
    std::lock_guard<std::mutex> lock(g_kidx_mu);
    const auto it = g_kidx_built.find(mem);
    if (it == g_kidx_built.end()) return MREC_EUNSUPPORTED;
    *mask_out = it->second;
    return MREC_OK;
}

MREC_API int mrec_kidx_bytes(int64_t n, size_t* out) {
    if (n < 0 || !out) return MREC_EINVAL;
    if (n > kKidxMaxKeys) return MREC_EUNSUPPORTED;
    *out = (size_t)kKidxHdr + (size_t)16 * scratch_cap(n);
    return MREC_OK;
}

MREC_API int mrec_kidx_build(void* mem, size_t mem_bytes, const int64_t* keys, const int32_t* rows, int64_t n, void* stream) {
    size_t need = 0;
    if (const int rc = mrec_kidx_bytes(n, &need)) return rc;
    if (!mem || (n > 0 && !keys) || mem_bytes < need) return MREC_EINVAL;
    if ((((uintptr_t)mem) & 255) != 0) return MREC_EUNSUPPORTED;
    const int64_t S = (int64_t)scratch_cap(n);
    const uint32_t mask = (uint32_t)(S - 1);
    {
        std::lock_guard<std::mutex> lock(g_kidx_mu);
        g_kidx_built[mem] = mask;
    }
    k_kidx_clear<<<stream_grid(S), KB, 0, (hipStream_t)stream>>>((uint8_t*)mem, S, n);
    MREC_LAUNCH_CHECK();
    k_kidx_insert<<<stream_grid(n), KB, 0, (hipStream_t)stream>>>((uint8_t*)mem, mask, keys, rows, n);
    MREC_LAUNCH_CHECK();
    return MREC_OK;
}

MREC_API int mrec_kidx_release(const void* mem) {
    std::lock_guard<std::mutex> lock(g_kidx_mu);
    g_kidx_built.erase(mem);
    return MREC_OK;
}

MREC_API int mrec_kidx_find(const void* mem, const void* keys, int32_t key_bytes, int64_t n, int32_t* rows_out, void* stream) {
    if ((key_bytes != 4 && key_bytes != 8) || n < 0) return MREC_EINVAL;
    if (n == 0) return MREC_OK;
    if (!mem || !keys || !rows_out) return MREC_EINVAL;
    uint32_t mask = 0;
    if (const int rc = mrec_kidx_host_mask(mem, &mask)) return rc;
    return by_key(keys, key_bytes, [&](auto* kp) {
        k_kidx_find<<<stream_grid(n), KB, 0, (hipStream_t)stream>>>((const uint8_t*)mem, mask, kp, n, rows_out);
        MREC_LAUNCH_CHECK();
        return (int)MREC_OK;
    });
}
