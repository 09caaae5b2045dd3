// mrec_common.h -- shared host/device helpers for libmrec_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mrec.h"

#define MREC_API extern "C" __attribute__((visibility("default")))

extern int g_mrec_last_hip_error;

#define MREC_HIP_CHECK(expr)                       \
    do {                                           \
        hipError_t _e = (expr);                    \
        if (_e != hipSuccess) {                    \
            g_mrec_last_hip_error = (int)_e;       \
            return MREC_EHIP;                      \
        }                                          \
    } while (0)

#define MREC_LAUNCH_CHECK() MREC_HIP_CHECK(hipGetLastError())

static inline size_t mrec_align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Bump allocator over the caller's workspace; every block 256-B aligned.  Without a workspace (the default constructor) it only
// counts: every take() answers nullptr and `off` ends as the bytes the same takes need of a real one -- so a layout is written once,
// as the takes that carve it, and its size query runs those takes.
struct MrecArena {
    char* base;
    size_t cap;
    size_t off;
    bool ok;
    MrecArena() : base(nullptr), cap(SIZE_MAX), off(0), ok(true) {}
    MrecArena(void* ws, size_t bytes) : base((char*)ws), cap(bytes), off(0), ok(true) {}
    template <class T>
    T* take(size_t count) {
        size_t b = mrec_align_up(count * sizeof(T), 256);
        if (off + b > cap) { ok = false; off += b; return nullptr; }
        T* p = base ? (T*)(base + off) : nullptr;
        off += b;
        return p;
    }
};

static inline int64_t mrec_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Slots of an open-addressing table over n keys at load <= 0.5: the power of two >= max(1024, 2 n).  The Unique's and the lookup's
// scratch tables and the key index's slot array (KeyIndex.n_slots in ops.py restates it).
static inline uint64_t scratch_cap(int64_t n) {
    uint64_t cap = 1024;
    while (cap < (uint64_t)n * 2) cap <<= 1;
    return cap;
}

static inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

// Grid of a grid-stride kernel of 256-thread workgroups: one thread per item, capped at 4096 workgroups.
static inline unsigned stream_grid(int64_t work_items) {
    int64_t b = mrec_cdiv(work_items, 256);
    if (b > 256 * 16) b = 256 * 16;
    if (b < 1) b = 1;
    return (unsigned)b;
}

// Host type dispatch: an argument that selects a template parameter is decided in ONE place, and f -- a generic lambda -- gets the typed
// pointer.  by_key: the width of an id / key 4 / 8 -> const int32_t* / const int64_t*.  by_out: the kind of a lookup's output rows
// 0 / 1 / 2 -> float* / bf16o_t* / f16o_t* (fp32, bf16, IEEE half: tags; the kernels' vstore overloads round, once, to nearest even).
// Where both are nested, the kernels are laid out in the code object in the order of the nesting: keep it and two builds compare byte
// for byte.
namespace { struct bf16o_t { uint16_t v; }; struct f16o_t { uint16_t v; }; }
template <class F>
static inline int by_key(const void* ids, int id_bytes, F&& f) {
    if (id_bytes == 4) return f((const int32_t*)ids);
    if (id_bytes == 8) return f((const int64_t*)ids);
    return MREC_EINVAL;
}
template <class F>
static inline int by_out(void* out, int out_kind, F&& f) {
    if (out_kind == 0) return f((float*)out);
    if (out_kind == 1) return f((bf16o_t*)out);
    if (out_kind == 2) return f((f16o_t*)out);
    return MREC_EINVAL;
}

constexpr int kWave = 64;

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// fp32 -> bf16, round to nearest even
__device__ __forceinline__ uint16_t f2bf(float x) { __bf16 b = (__bf16)x; return __builtin_bit_cast(uint16_t, b); }

__host__ __device__ __forceinline__ uint64_t mrec_mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ uint32_t mrec_hash32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ uint32_t mrec_hash_key(int32_t k) { return mrec_hash32((uint32_t)k); }
__device__ __forceinline__ uint32_t mrec_hash_key(int64_t k) {
    uint64_t h = mrec_mix64((uint64_t)k);
    return (uint32_t)(h ^ (h >> 32));
}

// Wave-level inclusive scan (sum) over 64 lanes.
__device__ __forceinline__ int wave_incl_scan(int x) {
    const int l = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        int y = __shfl_up(x, d, 64);
        if (l >= d) x += y;
    }
    return x;
}

// Block-level exclusive scan for 256-thread blocks; returns exclusive prefix, *total = block sum.
// smem must hold >= 8 ints.
__device__ __forceinline__ int block_excl_scan_256(int x, int* smem, int* total) {
    const int w = threadIdx.x >> 6, l = lane_id();
    int incl = wave_incl_scan(x);
    if (l == 63) smem[w] = incl;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        int s = smem[i];
        if (i < w) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + incl - x;
}

// Decoupled look-back over per-tile counts (one status word per tile: flag << 30 | value; flag 1 = the tile's own count,
// 2 = inclusive prefix).  Tiles are dispatched in index order and only ever wait for lower-numbered tiles, so the wait always
// ends.  The words are zero when the kernel starts, and whoever runs BEHIND the scanning kernel clears them again, which is what
// keeps a primed workspace primed: k_radix_hist / k_dedup_inv behind k_dedup_rank, k_map_finish behind k_map_place; k_map_evict's
// are zeroed by a memset in front of it.
constexpr unsigned kFlagA = 1u << 30, kFlagP = 2u << 30, kFlagMask = 3u << 30;

__device__ __forceinline__ int lookback_excl(unsigned* status, int tile) {
    const int l = lane_id();
    int excl = 0;
    for (int base = tile - 1;; base -= 64) {
        const int idx = base - l;
        unsigned st;
        do {
            st = (idx >= 0) ? __hip_atomic_load(&status[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : kFlagP;
        } while (__any((st & kFlagMask) == 0));
        const uint64_t pm = __ballot((st & kFlagMask) == kFlagP);
        const int firstp = pm ? __ffsll((long long)pm) - 1 : 63; // nearest predecessor with an inclusive prefix (the virtual
        int c = (l <= firstp) ? (int)(st & ~kFlagMask) : 0;      // tiles below 0 carry one); none in this round: add all 64
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
        excl += c;
        if (pm) break;
    }
    return excl;
}

// One 256-thread workgroup per tile, c = this thread's flagged items: returns their rank among all tiles' (exclusive), *tile_total
// = the tile's count; afterwards *s_excl (shared) holds the count of all lower tiles, so the last tile knows the grand total.
__device__ __forceinline__ int tile_excl_scan_256(int c, unsigned* status, int* sm, int* s_excl, int* tile_total) {
    int tot;
    const int pre = block_excl_scan_256(c, sm, &tot);
    if (threadIdx.x < 64) {
        const int t = blockIdx.x;
        int excl = 0;
        if (t == 0) {
            if (threadIdx.x == 0) __hip_atomic_store(&status[0], kFlagP | (unsigned)tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            if (threadIdx.x == 0) __hip_atomic_store(&status[t], kFlagA | (unsigned)tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            excl = lookback_excl(status, t);
            if (threadIdx.x == 0) __hip_atomic_store(&status[t], kFlagP | (unsigned)(excl + tot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (threadIdx.x == 0) *s_excl = excl;
    }
    __syncthreads();
    *tile_total = tot;
    return *s_excl + pre;
}

// ---- max_norm (nn.ClipByNorm over a looked-up row) ----------------------------------------------------------------------
/* max_norm: finite and > 0 (else MREC_EINVAL); D % 4 == 0 and D <= max_d (else MREC_EUNSUPPORTED) -- checked before any launch */
static inline int clip_check(float max_norm, int32_t D, int32_t max_d) {
    if (!(max_norm > 0.0f) || !(max_norm <= 3.402823466e38f)) return MREC_EINVAL;
    if (D <= 0) return MREC_EINVAL;
    if (D % 4 || D > max_d) return MREC_EUNSUPPORTED;
    return MREC_OK;
}

// Lane-group geometry shared by the row kernels: lpr lanes per row, G = 64/lpr groups per wave.
namespace { struct RowGeom { int lpr; int G; }; }

// A row of D = 4 nd columns sits in nd consecutive lanes of a lane-group, four columns each; `lane0` is the hardware lane of deep
// lane 0 and `ds` this lane's deep lane number (the wide lane, where a group has one, passes any ds and ignores the result; it is
// never read).  mrec_group_sum adds one value per deep lane in an order fixed by the deep lane numbers alone -- a butterfly over
// ds: at distance m a block of m deep lanes adds the sum of its partner block (read from any of that block's lanes: they all hold
// the same bits), a + b and b + a being the same float -- so every deep lane of the group ends with the same bits, and the lookup
// (k_gather_rows*, whose odd lane-groups of the w16 form put the wide lane first) and the sparse apply (wide lane last) get the
// same sum of squares for the same row: the clip decision of the forward and of the backward is one decision.
__device__ __forceinline__ float mrec_group_sum(float v, int ds, int nd, int lane0) {
    for (int m = 1; m < nd; m <<= 1) {
        const int p = ds ^ m;
        const bool has = (p & ~(m - 1)) < nd;                       // the partner block holds at least one deep lane
        const int src = lane0 + (p < nd ? p : nd - 1);              // (its last one where p lies past the row)
        const float o = __int_as_float(__builtin_amdgcn_ds_bpermute(src << 2, __float_as_int(v)));
        if (has) v = v + o;
    }
    return v;
}
// sum of squares of the row: the lane's four columns in column order, then mrec_group_sum
__device__ __forceinline__ float mrec_row_sumsq(const float4& x, int ds, int nd, int lane0) {
    float s = x.x * x.x;
    s = s + x.y * x.y;
    s = s + x.z * x.z;
    s = s + x.w * x.w;
    return mrec_group_sum(s, ds, nd, lane0);
}
// the clip decision: n = sqrt(n2) > c (a tie is not clipped; a zero row never is); *scale = c / n where it is
__device__ __forceinline__ bool mrec_clip_scale(float n2, float c, float* scale) {
    const float n = sqrtf(n2);
    *scale = c / n;
    return n > c;
}
// the clip's Jacobian over a completed gradient sum: lanes ds = 0 .. nd - 1 of the lane-group hold row x (the pre-update p, what the
// lookup read) and the sum g, and every one of them calls; g becomes (c / n) (g - (x.g / n^2) x) where n = |x| > c -- n^2 in
// mrec_row_sumsq's order and the decision mrec_clip_scale's, so it is the lookup's -- and stays as it is otherwise.  True where
// the row was clipped.  One body for the sparse apply (clip_grad, mrec_apply.hip) and the dense optimizers' group sums
// (k_clip_group_sums, mrec_dense_optim.hip).
__device__ __forceinline__ bool mrec_clip_jacobian(float4& g, const float4& x, float c, int ds, int nd, int lane0) {
    const float n2 = mrec_row_sumsq(x, ds, nd, lane0);
    float d = x.x * g.x;
    d = d + x.y * g.y;
    d = d + x.z * g.z;
    d = d + x.w * g.w;
    d = mrec_group_sum(d, ds, nd, lane0);
    float s;
    const bool hit = mrec_clip_scale(n2, c, &s);
    if (hit) {
        const float t = d / n2;
        g.x = s * (g.x - t * x.x);
        g.y = s * (g.y - t * x.y);
        g.z = s * (g.z - t * x.z);
        g.w = s * (g.w - t * x.w);
    }
    return hit;
}
