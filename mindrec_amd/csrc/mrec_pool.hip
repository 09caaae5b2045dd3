// mrec_pool.hip -- the multi-hot lookup: a bag of L ids per sample, looked up, multiplied by a mask and reduced over the bag
// (Gather -> Mul(mask) -> ReduceMean / ReduceSum), for gfx950.
//
// Reference call sites: models/wide_and_deep_multitable/src/wide_and_deep.py:301-346 (six fields over the 20 900 x 64 table
// `emb64_multi`: Gather -> Mul(mask) -> ReduceMean(axis 1)) and :377-418 (the wide side: Gather -> Mul(mask) -> ReduceSum).
//
//   out[b, 0:D] = reduce_{l = 0 .. L-1, ascending}  table[ids[b, l], :] * mask[b, l]        (mode 0: sum)
//               = (that sum) / (float)L                                                     (mode 1: mean)
//
// The mean divides by L, NOT by the number of unmasked slots: that is what ReduceMean over axis 1 does in the reference (the mask
// zeroes a slot's row, it does not take the slot out of the count).  The division is IEEE (correctly rounded).
// An id outside [0, V) contributes a +0.0 row, multiplied and added like any other (the rule of mrec_gather_rows).  fp32
// accumulation: slot 0's product starts the sum, every later slot is product then add (no fma: -ffp-contract=off), strictly in
// ascending slot order; 16-bit outputs are rounded once, at the end.  Every output is therefore bit-reproducible on the host
// (tests/_pool_ref.py), and L = 1 / mode 0 is mrec_gather_rows bit for bit.
//
// TWO entries, ONE kernel.  mrec_gather_pool_fields pools F bags of lengths L_0 .. L_{F-1} per sample (k_gather_pool_fields below,
// with the mapping of its work items and why); mrec_gather_pool, bags of one length L, is that with F = 1 and field_len = {L} --
// the same launch path, the same arithmetic (F == 1 selects the kernel's ONE instantiations, which find their bag without a
// division).  Both take id_bytes / out_kind arguments (the style of mrec_gather_rows_wide) instead of six names each: the six
// instantiations differ in two template arguments, and a caller that holds a tensor holds its element size.
//
// A third entry, mrec_gather_pool_fields_keyed, is the fields form over the rows of a hash table (MapParameter), where a key that is
// not in the table reads as its default row: a kernel of its own, k_gather_pool_fields_keyed, at the end of this file.
// max_norm (mrec_gather_pool_fields_clip, mrec_gather_pool_fields_keyed_clip: every looked-up row clipped before its mask product) is
// a third kernel, k_gather_pool_fields_clip, behind that one: the two above keep their symbols and their code.
//
// Shape of the kernel: k_gather_rows' (mrec_gather.hip).  lpr = D / 4 lanes per bag on the float4 path (D % 4 == 0, 16-byte
// aligned rows), G = 64 / lpr bags per wave; a lane-group keeps PB row loads in flight: the PB ids and mask values of a batch of
// slots, then the PB rows, all requested unconditionally (a slot past the bag's end reads the bag's last id, an id out of range
// reads row 0, a bag past the end reads the last bag; the values are dropped by selects) and needed in straight-line code, then the
// adds in slot order.  The one store comes last.  Everything else (D % 4 != 0, misaligned rows or outputs, D == 1: the wide
// weights) takes the same kernel at one column per lane.  Rows wider than a wave (D > 256 on the float4 path, D > 64 on the scalar
// one) are walked in column blocks by the same lane-group.
#include "mrec_common.h"
#include "mrec_optim.h"
#include "mrec_dense_adam.h"
#include "mrec_rng.h"

#include <type_traits>

namespace {

template <int VEC> struct Vf;
template <> struct Vf<4> { float4 v; };
template <> struct Vf<1> { float v; };

__device__ __forceinline__ Vf<4> vload(const float* p, Vf<4>*) { Vf<4> r; r.v = *(const float4*)p; return r; }
__device__ __forceinline__ Vf<1> vload(const float* p, Vf<1>*) { Vf<1> r; r.v = *p; return r; }
__device__ __forceinline__ Vf<4> vscale(Vf<4> x, float s) { x.v.x *= s; x.v.y *= s; x.v.z *= s; x.v.w *= s; return x; }
__device__ __forceinline__ Vf<1> vscale(Vf<1> x, float s) { x.v *= s; return x; }
__device__ __forceinline__ Vf<4> vadd(Vf<4> a, const Vf<4>& b) {
    a.v.x = a.v.x + b.v.x; a.v.y = a.v.y + b.v.y; a.v.z = a.v.z + b.v.z; a.v.w = a.v.w + b.v.w;
    return a;
}
__device__ __forceinline__ Vf<1> vadd(Vf<1> a, const Vf<1>& b) { a.v = a.v + b.v; return a; }
__device__ __forceinline__ Vf<4> vdiv(Vf<4> x, float d) { x.v.x = x.v.x / d; x.v.y = x.v.y / d; x.v.z = x.v.z / d; x.v.w = x.v.w / d; return x; }
__device__ __forceinline__ Vf<1> vdiv(Vf<1> x, float d) { x.v = x.v / d; return x; }
// "this value is needed here" (see k_gather_rows, mrec_gather.hip)
__device__ __forceinline__ void vtouch(Vf<4>& r) { asm volatile("" : "+v"(r.v.x), "+v"(r.v.y), "+v"(r.v.z), "+v"(r.v.w)); }
__device__ __forceinline__ void vtouch(Vf<1>& r) { asm volatile("" : "+v"(r.v)); }
__device__ __forceinline__ Vf<4> vzero(Vf<4>*) { Vf<4> r; r.v = make_float4(0.f, 0.f, 0.f, 0.f); return r; }
__device__ __forceinline__ Vf<1> vzero(Vf<1>*) { Vf<1> r; r.v = 0.f; return r; }

// output rows: fp32, bf16 or IEEE half (round-to-nearest-even, once), as the lookup's (mrec_gather.hip; the tags: mrec_common.h)
__device__ __forceinline__ unsigned f2h2(float lo, float hi) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 v = {(_Float16)lo, (_Float16)hi};
    return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ void vstore(float* p, const Vf<4>& x) { *(float4*)p = x.v; }
__device__ __forceinline__ void vstore(float* p, const Vf<1>& x) { *p = x.v; }
__device__ __forceinline__ void vstore(bf16o_t* p, const Vf<4>& x) {
    uint2 u;
    u.x = (unsigned)f2bf(x.v.x) | ((unsigned)f2bf(x.v.y) << 16);
    u.y = (unsigned)f2bf(x.v.z) | ((unsigned)f2bf(x.v.w) << 16);
    *(uint2*)p = u;
}
__device__ __forceinline__ void vstore(bf16o_t* p, const Vf<1>& x) { p->v = f2bf(x.v); }
__device__ __forceinline__ void vstore(f16o_t* p, const Vf<4>& x) { *(uint2*)p = make_uint2(f2h2(x.v.x, x.v.y), f2h2(x.v.z, x.v.w)); }
__device__ __forceinline__ void vstore(f16o_t* p, const Vf<1>& x) { p->v = __builtin_bit_cast(uint16_t, (_Float16)x.v); }

struct PoolGeom { int lpr; int G; };      // lanes per bag, bags per wave

// F bags of lengths L_0 .. L_{F-1} per sample, back to back in a row of Ls = sum L_f ids (the reference's multi-hot fields have one
// bag length EACH: src/datasets.py:290-313, input_shape_dict), pooled per field into columns f * D .. (f + 1) * D - 1 of the sample's
// output row (the Concat at wide_and_deep.py:348-349).  One launch.  (mrec_gather_pool: F = 1, the sample is the bag.)
//
// Work-item mapping: a lane-group's work item is bag w = b * F + f -- SAMPLE-major, field-minor.  Neighbouring lane-groups of a wave
// then take neighbouring fields of one sample and go on into the next sample: their ids (and mask values) are one contiguous stretch
// of the [B, Ls] arrays -- G consecutive bags of a wave cover about G * Ls / F consecutive ids, the same cache lines -- and with
// ldo == F * D their output rows are one contiguous stretch too.  The other choice, field-major (a wave = G samples of ONE field),
// gives every lane-group of a wave the same trip count, but each lane-group's ids then sit Ls ids from its neighbour's: every id or
// mask line a wave touches is fetched for L_f of its Ls entries, by F different waves at different times.  The id and mask reads are
// the start of the kernel's chain of dependent loads (id -> row), so the mapping that fetches each of their lines once was chosen;
// the price is that lane-groups of one wave run different numbers of PB-deep batches (ceil(L_f / PB): 1 for every field of the
// reference's shapes at PB = 8), which costs nothing but idle lanes -- the kernel has no barriers.
// The per-field (offset, length) pairs travel BY VALUE in the kernel's arguments, one 32-bit word per field (offset < 4096 and
// length <= 4096 fit 16 bits each): no table in device memory, no copy, no allocation -- the entry stays capturable.  A lane reads
// its field's word by a per-lane index: a cached load from the argument segment, once per lane.
// Arithmetic: the file header's, per bag (slot 0 starts the sum, product then add in ascending slot order, one IEEE division by
// (float)L_f -- the FIELD's length -- for the mean, 16-bit outputs rounded once).
// PB: slots in flight per lane-group (2 for bags of one or two slots, 8 for longer ones: 8 float4 rows = 32 registers)
// ONE: F == 1, the sample is the bag (every mrec_gather_pool call): b = w, offset 0, length Ls -- without the division by F and the
// per-lane load from the argument segment, which cost 17 % where the table sits in cache; the rest is one text.
struct PoolFields { unsigned w[MREC_POOL_MAX_FIELDS]; };      // w[f] = off_f | L_f << 16

template <int VEC, int PB, class K, class OT, bool ONE>
__global__ __launch_bounds__(256) void k_gather_pool_fields(const float* __restrict__ table, int64_t V, int64_t ld, const K* __restrict__ ids,
                                                            const float* __restrict__ mask, unsigned nbags, unsigned F, int Ls, int mode,
                                                            OT* __restrict__ out, int64_t ldo, int D, PoolGeom gm, const PoolFields pf) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / gm.lpr, sub = lane - grp * gm.lpr;
    if (grp >= gm.G) return;                                      // spare lanes; this kernel has no barriers
    const unsigned w = (blockIdx.x * 4u + (unsigned)wave) * (unsigned)gm.G + (unsigned)grp;      // (nbags = B * F < 2^31: no wrap)
    const unsigned wc = w < nbags ? w : nbags - 1u;               // a bag past the end reads the last bag, and stores nothing
    const unsigned b = ONE ? wc : wc / F, f = wc - b * F;
    const unsigned fw = ONE ? (unsigned)Ls << 16 : pf.w[f];
    const int off = (int)(fw & 0xFFFFu), L = (int)(fw >> 16);
    const K* __restrict__ idb = ids + (int64_t)b * Ls + off;
    const float* __restrict__ mb = mask ? mask + (int64_t)b * Ls + off : nullptr;
    OT* __restrict__ ob = out + (int64_t)b * ldo + (int64_t)f * D;
    const int llast = L - 1;
    const float fl = (float)L;
    for (int col = sub * VEC; col < D; col += gm.lpr * VEC) {
        Vf<VEC> acc = vzero((Vf<VEC>*)nullptr);
        for (int l0 = 0; l0 < L; l0 += PB) {                      // (L is the FIELD's: lane-groups of a wave may walk different numbers of batches)
            int64_t row[PB];
            float mk[PB];
            Vf<VEC> x[PB];
            bool okr[PB];
#pragma unroll
            for (int k = 0; k < PB; ++k) {
                const int lc = l0 + k < L ? l0 + k : llast;       // (a slot past the bag's end reads the bag's last id: inside the bag)
                row[k] = (int64_t)idb[lc];
                mk[k] = mb ? mb[lc] : 1.0f;
            }
#pragma unroll
            for (int k = 0; k < PB; ++k) {
                okr[k] = row[k] >= 0 && row[k] < V;
                x[k] = vload(table + (okr[k] ? row[k] : 0) * ld + col, (Vf<VEC>*)nullptr);
            }
#pragma unroll
            for (int k = 0; k < PB; ++k) {
                vtouch(x[k]);
                if (!okr[k]) x[k] = vzero((Vf<VEC>*)nullptr);
            }
#pragma unroll
            for (int k = 0; k < PB; ++k) {
                if (l0 + k < L) {
                    const Vf<VEC> p = mb ? vscale(x[k], mk[k]) : x[k];
                    acc = (l0 + k == 0) ? p : vadd(acc, p);       // slot 0 starts the sum (L = 1: the lookup's product, bit for bit)
                }
            }
        }
        if (mode == 1) acc = vdiv(acc, fl);
        if (w < nbags) vstore(ob + col, acc);
    }
}

// The launch of all three pooled kernels: float4 lanes (vec) where the rows, and the 4-element quads of every field's output block, are
// aligned (D % 4 == 0: f * D too), else a column per lane; lpr lanes per bag, at most a wave; four waves of G bags per workgroup.
struct PoolLaunch { bool vec; PoolGeom gm; unsigned blocks; };
inline PoolLaunch pool_launch(int32_t D, int64_t ld, int64_t ldo, const void* table, const void* out, size_t out_bytes, int64_t B, int32_t F) {
    const uintptr_t oa = out_bytes == 2 ? 7 : 15;
    PoolLaunch p;
    p.vec = D % 4 == 0 && ld % 4 == 0 && ldo % 4 == 0 && al16(table) && (((uintptr_t)out) & oa) == 0;
    const int cols = p.vec ? D / 4 : D;
    p.gm.lpr = cols < 64 ? cols : 64;
    p.gm.G = 64 / p.gm.lpr;
    p.blocks = (unsigned)mrec_cdiv(B * F, (int64_t)4 * p.gm.G);
    return p;
}

template <class K, class OT>
int pool_impl(const float* table, int64_t V, int64_t ld, int32_t D, const K* ids, int64_t B, int32_t F, int32_t Ls, int32_t maxL,
              const PoolFields& pf, const float* mask, int32_t mode, OT* out, int64_t ldo, hipStream_t st) {
    const auto [vec, gm, blocks] = pool_launch(D, ld, ldo, table, out, sizeof(OT), B, F);
    const int64_t nbags = B * F;
#define MREC_POOL_LAUNCH1(VECN, PBN, ONE)                                                                                             \
    k_gather_pool_fields<VECN, PBN, K, OT, ONE><<<blocks, 256, 0, st>>>(table, V, ld, ids, mask, (unsigned)nbags, (unsigned)F, (int)Ls,       \
                                                                       (int)mode, out, ldo, (int)D, gm, pf)
#define MREC_POOL_LAUNCH(VECN, PBN) do { if (F == 1) MREC_POOL_LAUNCH1(VECN, PBN, true); else MREC_POOL_LAUNCH1(VECN, PBN, false); } while (0)
    if (vec) {
        if (maxL <= 2) MREC_POOL_LAUNCH(4, 2); else MREC_POOL_LAUNCH(4, 8);
    } else {
        if (maxL <= 2) MREC_POOL_LAUNCH(1, 2); else MREC_POOL_LAUNCH(1, 8);
    }
#undef MREC_POOL_LAUNCH
#undef MREC_POOL_LAUNCH1
    MREC_LAUNCH_CHECK();
    return MREC_OK;
}

// what both entries check first, and what both do last (pf: the bags of a sample, Ls ids, the longest maxL)
inline bool pool_args_ok(int32_t id_bytes, int32_t out_kind, int32_t mode, int64_t B, int32_t D, int64_t V, int64_t ld) {
    return (id_bytes == 4 || id_bytes == 8) && out_kind >= 0 && out_kind <= 2 && (mode == 0 || mode == 1) && B >= 0 && D > 0 && V >= 0 && ld >= D;
}
int pool_run(const float* table, int64_t V, int64_t ld, int32_t D, const void* ids, int32_t id_bytes, int64_t B, int32_t F, int32_t Ls,
             int32_t maxL, const PoolFields& pf, const float* mask, int32_t mode, void* out, int32_t out_kind, int64_t ldo, void* stream) {
    if (B * F > (int64_t(1) << 31) - 1) return MREC_EUNSUPPORTED;      // (bags are numbered in 32 bits)
    if (B == 0) return MREC_OK;
    if (V == 0) return MREC_EINVAL;      // rows are read unconditionally at clamped addresses: an empty table has no valid one
    if (!table || !ids || !out) return MREC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    return by_key(ids, id_bytes, [&](auto* ip) {
        return by_out(out, out_kind, [&](auto* op) { return pool_impl(table, V, ld, D, ip, B, F, Ls, maxL, pf, mask, mode, op, ldo, st); });
    });
}

// ===== the KEYED form: the pooled lookup over the rows of a hash table (MapParameter) ==================================================
// ids are the int32 row numbers the map's index gave for the sample's keys (KeyIndex.lookup: -1 for a key that is not in the table --
// not inserted by this call, or dropped because the table is full), keys the keys themselves.  MapTensorGet reads such a key as its
// DEFAULT row, not as zeros, so a slot whose row is outside [0, V) contributes mrec_map_default2 of its key (mrec_rng.h: the text
// mrec_map_fill_missing writes those rows with, the same values in the same columns), generated in registers for the columns the
// lane holds.  Everything else is k_gather_pool_fields, statement for statement: sample-major bags, PB slots in flight, the rows
// requested unconditionally at clamped addresses, product then add in ascending slot order, one division, one store; no barriers, LDS
// or atomics.  The key of a slot is loaded only where its row is missing -- in the stage that requests the rows, so it adds no level to
// the chain of dependent loads, and a lookup of resident keys reads no key at all -- and the generator (a logarithm, a root and a
// sine / cosine pair per two columns) runs under the same condition.
// A kernel of its own, with its own instantiations: k_gather_pool_fields above keeps its symbols and its code.
struct MapDefault { uint64_t seed; float sigma; float fill; };

__device__ __forceinline__ Vf<4> vdefault(const MapDefault& d, int64_t key, int col, Vf<4>*) {      // (col is a multiple of 4)
    Vf<4> r;
    mrec_map_default2(d.seed, d.sigma, d.fill, key, col >> 1, r.v.x, r.v.y);
    mrec_map_default2(d.seed, d.sigma, d.fill, key, (col >> 1) + 1, r.v.z, r.v.w);
    return r;
}
__device__ __forceinline__ Vf<1> vdefault(const MapDefault& d, int64_t key, int col, Vf<1>*) {
    float z0, z1;
    mrec_map_default2(d.seed, d.sigma, d.fill, key, col >> 1, z0, z1);
    Vf<1> r;
    r.v = (col & 1) ? z1 : z0;
    return r;
}

template <int VEC, int PB, class K, class OT, bool ONE>
__global__ __launch_bounds__(256) void k_gather_pool_fields_keyed(const float* __restrict__ table, int64_t V, int64_t ld,
                                                                  const int32_t* __restrict__ ids, const K* __restrict__ keys,
                                                                  const float* __restrict__ mask, unsigned nbags, unsigned F, int Ls, int mode,
                                                                  OT* __restrict__ out, int64_t ldo, int D, PoolGeom gm, const MapDefault dv,
                                                                  const PoolFields pf) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / gm.lpr, sub = lane - grp * gm.lpr;
    if (grp >= gm.G) return;                                      // spare lanes; this kernel has no barriers
    const unsigned w = (blockIdx.x * 4u + (unsigned)wave) * (unsigned)gm.G + (unsigned)grp;      // (nbags = B * F < 2^31: no wrap)
    const unsigned wc = w < nbags ? w : nbags - 1u;               // a bag past the end reads the last bag, and stores nothing
    const unsigned b = ONE ? wc : wc / F, f = wc - b * F;
    const unsigned fw = ONE ? (unsigned)Ls << 16 : pf.w[f];
    const int off = (int)(fw & 0xFFFFu), L = (int)(fw >> 16);
    const int32_t* __restrict__ idb = ids + (int64_t)b * Ls + off;
    const K* __restrict__ kb = keys + (int64_t)b * Ls + off;
    const float* __restrict__ mb = mask ? mask + (int64_t)b * Ls + off : nullptr;
    OT* __restrict__ ob = out + (int64_t)b * ldo + (int64_t)f * D;
    const int llast = L - 1;
    const float fl = (float)L;
    for (int col = sub * VEC; col < D; col += gm.lpr * VEC) {
        Vf<VEC> acc = vzero((Vf<VEC>*)nullptr);
        for (int l0 = 0; l0 < L; l0 += PB) {
            int64_t row[PB], key[PB];
            float mk[PB];
            Vf<VEC> x[PB];
            bool okr[PB];
#pragma unroll
            for (int k = 0; k < PB; ++k) {
                const int lc = l0 + k < L ? l0 + k : llast;       // (a slot past the bag's end reads the bag's last id: inside the bag)
                row[k] = (int64_t)idb[lc];
                mk[k] = mb ? mb[lc] : 1.0f;
            }
#pragma unroll
            for (int k = 0; k < PB; ++k) {
                okr[k] = row[k] >= 0 && row[k] < V;
                x[k] = vload(table + (okr[k] ? row[k] : 0) * ld + col, (Vf<VEC>*)nullptr);
                key[k] = 0;
                if (!okr[k] && l0 + k < L) key[k] = (int64_t)kb[l0 + k];      // (the slot's own key: l0 + k < L, inside the bag)
            }
#pragma unroll
            for (int k = 0; k < PB; ++k) {
                vtouch(x[k]);
                if (!okr[k]) x[k] = (l0 + k < L) ? vdefault(dv, key[k], col, (Vf<VEC>*)nullptr) : vzero((Vf<VEC>*)nullptr);
            }
#pragma unroll
            for (int k = 0; k < PB; ++k) {
                if (l0 + k < L) {
                    const Vf<VEC> p = mb ? vscale(x[k], mk[k]) : x[k];
                    acc = (l0 + k == 0) ? p : vadd(acc, p);       // slot 0 starts the sum
                }
            }
        }
        if (mode == 1) acc = vdiv(acc, fl);
        if (w < nbags) vstore(ob + col, acc);
    }
}

template <class K, class OT>
int pool_keyed_impl(const float* table, int64_t V, int64_t ld, int32_t D, const int32_t* ids, const K* keys, int64_t B, int32_t F,
                    int32_t Ls, int32_t maxL, const PoolFields& pf, const float* mask, int32_t mode, const MapDefault& dv, OT* out,
                    int64_t ldo, hipStream_t st) {
    const auto [vec, gm, blocks] = pool_launch(D, ld, ldo, table, out, sizeof(OT), B, F);
    const int64_t nbags = B * F;
#define MREC_POOLK_LAUNCH1(VECN, PBN, ONE)                                                                                            \
    k_gather_pool_fields_keyed<VECN, PBN, K, OT, ONE><<<blocks, 256, 0, st>>>(table, V, ld, ids, keys, mask, (unsigned)nbags, (unsigned)F,    \
                                                                             (int)Ls, (int)mode, out, ldo, (int)D, gm, dv, pf)
#define MREC_POOLK_LAUNCH(VECN, PBN) do { if (F == 1) MREC_POOLK_LAUNCH1(VECN, PBN, true); else MREC_POOLK_LAUNCH1(VECN, PBN, false); } while (0)
    if (vec) {
        if (maxL <= 2) MREC_POOLK_LAUNCH(4, 2); else MREC_POOLK_LAUNCH(4, 8);
    } else {
        if (maxL <= 2) MREC_POOLK_LAUNCH(1, 2); else MREC_POOLK_LAUNCH(1, 8);
    }
#undef MREC_POOLK_LAUNCH
#undef MREC_POOLK_LAUNCH1
    MREC_LAUNCH_CHECK();
    return MREC_OK;
}

// ===== max_norm: the pooled lookup with nn.ClipByNorm over every looked-up row ========================================================
// HashEmbeddingLookup(max_norm=c) / nn.EmbeddingLookup(max_norm=c) (mindspore_rec/ops/embedding.py:156-161,202-205) clip each row
// BEFORE the `* mask`; over bags that is Gather -> ClipByNorm -> Mul(mask) -> ReduceMean / ReduceSum.  The kernel is the two above,
// statement for statement, with one stage more: once the PB rows of a batch of slots have landed and the rows that are not the table's
// have been replaced -- a zero row in the dense form, the key's default row in the keyed form (MapTensorGet returns it and
// ClipByNorm follows) -- every slot in flight takes mrec_row_sumsq, then mrec_clip_scale, and is scaled where n > c: the arithmetic
// of k_gather_rows' clip instantiations (mrec_gather.hip), operation for operation, so a row reads the same bits through either
// lookup and the sparse apply's Jacobian (clip_grad, mrec_apply.hip) takes the same decision.  A zero row has n = 0 and is never
// clipped.  Then product, slot-order adds, one division, one store, as above.
// Float4 rows only and ONE column block: D % 4 == 0, D <= 256, so a bag's lane-group is nd = D / 4 lanes that hold the whole row
// (lpr == nd), the butterfly's partners are lanes lane0 .. lane0 + nd - 1 of the bag's OWN lane-group (lane0 = lane - sub), which
// share L and so sit in the same iteration of the l0 loop: lane-groups of a wave that walk different numbers of batches never read
// each other, and the spare lanes that left at the top are nobody's partner.
// One kernel for both forms: KEY = void is the dense form (ids of type I, no keys, no default), else the keyed form (I = int32_t).
template <int PB, class I, class KEY, class OT, bool ONE>
__global__ __launch_bounds__(256) void k_gather_pool_fields_clip(const float* __restrict__ table, int64_t V, int64_t ld,
                                                                 const I* __restrict__ ids, const KEY* __restrict__ keys,
                                                                 const float* __restrict__ mask, unsigned nbags, unsigned F, int Ls, int mode,
                                                                 OT* __restrict__ out, int64_t ldo, int D, PoolGeom gm, float c,
                                                                 const MapDefault dv, const PoolFields pf) {
    constexpr bool KEYED = !std::is_void<KEY>::value;
    typedef typename std::conditional<KEYED, KEY, int32_t>::type KT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / gm.lpr, sub = lane - grp * gm.lpr;
    if (grp >= gm.G) return;                                      // spare lanes; this kernel has no barriers
    const unsigned w = (blockIdx.x * 4u + (unsigned)wave) * (unsigned)gm.G + (unsigned)grp;      // (nbags = B * F < 2^31: no wrap)
    const unsigned wc = w < nbags ? w : nbags - 1u;               // a bag past the end reads the last bag, and stores nothing
    const unsigned b = ONE ? wc : wc / F, f = wc - b * F;
    const unsigned fw = ONE ? (unsigned)Ls << 16 : pf.w[f];
    const int off = (int)(fw & 0xFFFFu), L = (int)(fw >> 16);
    const I* __restrict__ idb = ids + (int64_t)b * Ls + off;
    const KT* __restrict__ kb = KEYED ? (const KT*)keys + (int64_t)b * Ls + off : nullptr;
    const float* __restrict__ mb = mask ? mask + (int64_t)b * Ls + off : nullptr;
    OT* __restrict__ ob = out + (int64_t)b * ldo + (int64_t)f * D;
    const int llast = L - 1;
    const float fl = (float)L;
    const int col = sub * 4;                                      // (the lane-group holds the whole row: lpr == D / 4)
    const int nd = gm.lpr, lane0 = lane - sub;
    Vf<4> acc = vzero((Vf<4>*)nullptr);
    for (int l0 = 0; l0 < L; l0 += PB) {
        int64_t row[PB], key[PB];
        float mk[PB];
        Vf<4> x[PB];
        bool okr[PB];
#pragma unroll
        for (int k = 0; k < PB; ++k) {
            const int lc = l0 + k < L ? l0 + k : llast;           // (a slot past the bag's end reads the bag's last id: inside the bag)
            row[k] = (int64_t)idb[lc];
            mk[k] = mb ? mb[lc] : 1.0f;
        }
#pragma unroll
        for (int k = 0; k < PB; ++k) {
            okr[k] = row[k] >= 0 && row[k] < V;
            x[k] = vload(table + (okr[k] ? row[k] : 0) * ld + col, (Vf<4>*)nullptr);
            key[k] = 0;
            if constexpr (KEYED) {
                if (!okr[k] && l0 + k < L) key[k] = (int64_t)kb[l0 + k];      // (the slot's own key: l0 + k < L, inside the bag)
            }
        }
#pragma unroll
        for (int k = 0; k < PB; ++k) {
            vtouch(x[k]);
            if (!okr[k]) {
                if constexpr (KEYED) x[k] = (l0 + k < L) ? vdefault(dv, key[k], col, (Vf<4>*)nullptr) : vzero((Vf<4>*)nullptr);
                else x[k] = vzero((Vf<4>*)nullptr);
            }
        }
#pragma unroll
        for (int k = 0; k < PB; ++k) {                            // (every lane of the lane-group, every slot in flight: no branch around the butterfly)
            float s;
            if (mrec_clip_scale(mrec_row_sumsq(x[k].v, sub, nd, lane0), c, &s)) x[k] = vscale(x[k], s);
        }
#pragma unroll
        for (int k = 0; k < PB; ++k) {
            if (l0 + k < L) {
                const Vf<4> p = mb ? vscale(x[k], mk[k]) : x[k];
                acc = (l0 + k == 0) ? p : vadd(acc, p);           // slot 0 starts the sum
            }
        }
    }
    if (mode == 1) acc = vdiv(acc, fl);
    if (w < nbags) vstore(ob + col, acc);
}

/* max_norm: finite and > 0 (else MREC_EINVAL) -- clip_check's first half (mrec_common.h) */
inline bool pool_clip_ok(float max_norm) { return max_norm > 0.0f && max_norm <= 3.402823466e38f; }

template <class I, class KEY, class OT>
int pool_clip_impl(const float* table, int64_t V, int64_t ld, int32_t D, const I* ids, const KEY* keys, int64_t B, int32_t F, int32_t Ls,
                   int32_t maxL, const PoolFields& pf, const float* mask, int32_t mode, const MapDefault& dv, float c, OT* out, int64_t ldo,
                   hipStream_t st) {
    const auto [vec, gm, blocks] = pool_launch(D, ld, ldo, table, out, sizeof(OT), B, F);      // (float4 rows, D <= 256: lpr == D / 4)
    (void)vec;                                           // (true: checked by pool_clip_run)
    const int64_t nbags = B * F;
#define MREC_POOLC_LAUNCH1(PBN, ONE)                                                                                                  \
    k_gather_pool_fields_clip<PBN, I, KEY, OT, ONE><<<blocks, 256, 0, st>>>(table, V, ld, ids, keys, mask, (unsigned)nbags, (unsigned)F,     \
                                                                           (int)Ls, (int)mode, out, ldo, (int)D, gm, c, dv, pf)
#define MREC_POOLC_LAUNCH(PBN) do { if (F == 1) MREC_POOLC_LAUNCH1(PBN, true); else MREC_POOLC_LAUNCH1(PBN, false); } while (0)
    if (maxL <= 2) MREC_POOLC_LAUNCH(2); else MREC_POOLC_LAUNCH(8);
#undef MREC_POOLC_LAUNCH
#undef MREC_POOLC_LAUNCH1
    MREC_LAUNCH_CHECK();
    return MREC_OK;
}

// what both _clip entries do behind their own argument checks (keys == nullptr / key_bytes == 0: the dense form, ids of id_bytes)
int pool_clip_run(const float* table, int64_t V, int64_t ld, int32_t D, const void* ids, int32_t id_bytes, const void* keys,
                  int32_t key_bytes, int64_t B, int32_t F, int32_t Ls, int32_t maxL, const PoolFields& pf, const float* mask, int32_t mode,
                  const MapDefault& dv, float c, void* out, int32_t out_kind, int64_t ldo, void* stream) {
    if (B * F > (int64_t(1) << 31) - 1) return MREC_EUNSUPPORTED;      // (bags are numbered in 32 bits)
    // float4 rows in one column block, or nothing: a row's norm is one lane-group's
    if (!pool_launch(D, ld, ldo, table, out, out_kind == 0 ? 4 : 2, B, F).vec || D > 256) return MREC_EUNSUPPORTED;
    if (B == 0) return MREC_OK;
    if (V == 0) return MREC_EINVAL;      // rows are read unconditionally at clamped addresses: an empty table has no valid one
    if (!table || !ids || !out || (key_bytes && !keys)) return MREC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const auto run = [&](auto* ip, auto* kp) {      // (the keyed forms first, then the dense ones: the kernels' order in the code object)
        return by_out(out, out_kind, [&](auto* op) { return pool_clip_impl(table, V, ld, D, ip, kp, B, F, Ls, maxL, pf, mask, mode, dv, c, op, ldo, st); });
    };
    if (key_bytes) return by_key(keys, key_bytes, [&](auto* kp) { return run((const int32_t*)ids, kp); });
    return by_key(ids, id_bytes, [&](auto* ip) { return run(ip, (const void*)nullptr); });
}

// the bags of a sample from the caller's lengths: what both fields entries check, in this order
int pool_fields_parse(int32_t F, const int32_t* field_len, PoolFields& pf, int32_t& Ls_out, int32_t& maxL_out) {
    if (F < 1 || !field_len) return MREC_EINVAL;
    if (F > MREC_POOL_MAX_FIELDS) return MREC_EUNSUPPORTED;
    int64_t Ls = 0;
    int32_t maxL = 0;
    for (int f = 0; f < F; ++f) {
        const int32_t Lf = field_len[f];
        if (Lf < 1) return MREC_EINVAL;
        if (Ls + Lf > MREC_POOL_MAX_BAG) return MREC_EUNSUPPORTED;
        pf.w[f] = (unsigned)Ls | ((unsigned)Lf << 16);
        Ls += Lf;
        maxL = Lf > maxL ? Lf : maxL;
    }
    Ls_out = (int32_t)Ls;
    maxL_out = maxL;
    return MREC_OK;
}

}  // namespace

MREC_API int mrec_gather_pool(const float* table, int64_t V, int64_t ld, int32_t D, const void* ids, int32_t id_bytes, int64_t B, int32_t L,
                              const float* mask, int32_t mode, void* out, int32_t out_kind, int64_t ldo, void* stream) {
    if (!pool_args_ok(id_bytes, out_kind, mode, B, D, V, ld) || L < 1) return MREC_EINVAL;
    if (ldo == 0) ldo = D;
    if (ldo < D) return MREC_EINVAL;
    if (L > MREC_POOL_MAX_BAG) return MREC_EUNSUPPORTED;
    PoolFields pf{};
    pf.w[0] = (unsigned)L << 16;         // one field: offset 0, length L
    return pool_run(table, V, ld, D, ids, id_bytes, B, 1, L, L, pf, mask, mode, out, out_kind, ldo, stream);
}

MREC_API int mrec_gather_pool_fields(const float* table, int64_t V, int64_t ld, int32_t D, const void* ids, int32_t id_bytes, int64_t B,
                                     int32_t F, const int32_t* field_len, const float* mask, int32_t mode, void* out, int32_t out_kind,
                                     int64_t ldo, void* stream) {
    if (!pool_args_ok(id_bytes, out_kind, mode, B, D, V, ld)) return MREC_EINVAL;
    PoolFields pf{};
    int32_t Ls = 0, maxL = 0;
    const int rc = pool_fields_parse(F, field_len, pf, Ls, maxL);
    if (rc != MREC_OK) return rc;
    if (ldo == 0) ldo = (int64_t)F * D;
    if (ldo < (int64_t)F * D) return MREC_EINVAL;
    return pool_run(table, V, ld, D, ids, id_bytes, B, F, Ls, maxL, pf, mask, mode, out, out_kind, ldo, stream);
}

MREC_API int mrec_gather_pool_fields_keyed(const float* table, int64_t V, int64_t ld, int32_t D, const int32_t* rows, const void* keys,
                                           int32_t key_bytes, int64_t B, int32_t F, const int32_t* field_len, const float* mask,
                                           int32_t mode, uint64_t seed, float sigma, float fill, void* out, int32_t out_kind, int64_t ldo,
                                           void* stream) {
    if (!pool_args_ok(key_bytes, out_kind, mode, B, D, V, ld)) return MREC_EINVAL;
    if (!(sigma - sigma == 0.0f) || !(fill - fill == 0.0f)) return MREC_EINVAL;      // NaN or infinite
    PoolFields pf{};
    int32_t Ls = 0, maxL = 0;
    const int rc = pool_fields_parse(F, field_len, pf, Ls, maxL);
    if (rc != MREC_OK) return rc;
    if (ldo == 0) ldo = (int64_t)F * D;
    if (ldo < (int64_t)F * D) return MREC_EINVAL;
    if (B * F > (int64_t(1) << 31) - 1) return MREC_EUNSUPPORTED;      // (bags are numbered in 32 bits)
    if (B == 0) return MREC_OK;
    if (V == 0) return MREC_EINVAL;      // rows are read unconditionally at clamped addresses: an empty table has no valid one
    if (!table || !rows || !keys || !out) return MREC_EINVAL;
    const MapDefault dv{seed, sigma, fill};
    hipStream_t st = (hipStream_t)stream;
    return by_key(keys, key_bytes, [&](auto* kp) {
        return by_out(out, out_kind, [&](auto* op) { return pool_keyed_impl(table, V, ld, D, rows, kp, B, F, Ls, maxL, pf, mask, mode, dv, op, ldo, st); });
    });
}

/* ... with max_norm: every looked-up row is clipped (nn.ClipByNorm) before its mask product */
MREC_API int mrec_gather_pool_fields_clip(const float* table, int64_t V, int64_t ld, int32_t D, const void* ids, int32_t id_bytes, int64_t B,
                                          int32_t F, const int32_t* field_len, const float* mask, int32_t mode, void* out, int32_t out_kind,
                                          int64_t ldo, float max_norm, void* stream) {
    if (!pool_args_ok(id_bytes, out_kind, mode, B, D, V, ld) || !pool_clip_ok(max_norm)) return MREC_EINVAL;
    PoolFields pf{};
    int32_t Ls = 0, maxL = 0;
    const int rc = pool_fields_parse(F, field_len, pf, Ls, maxL);
    if (rc != MREC_OK) return rc;
    if (ldo == 0) ldo = (int64_t)F * D;
    if (ldo < (int64_t)F * D) return MREC_EINVAL;
    return pool_clip_run(table, V, ld, D, ids, id_bytes, nullptr, 0, B, F, Ls, maxL, pf, mask, mode, MapDefault{0, 0.0f, 0.0f}, max_norm, out,
                         out_kind, ldo, stream);
}

MREC_API int mrec_gather_pool_fields_keyed_clip(const float* table, int64_t V, int64_t ld, int32_t D, const int32_t* rows, const void* keys,
                                                int32_t key_bytes, int64_t B, int32_t F, const int32_t* field_len, const float* mask,
                                                int32_t mode, uint64_t seed, float sigma, float fill, void* out, int32_t out_kind,
                                                int64_t ldo, float max_norm, void* stream) {
    if (!pool_args_ok(key_bytes, out_kind, mode, B, D, V, ld) || !pool_clip_ok(max_norm)) return MREC_EINVAL;
    if (!(sigma - sigma == 0.0f) || !(fill - fill == 0.0f)) return MREC_EINVAL;      // NaN or infinite
    PoolFields pf{};
    int32_t Ls = 0, maxL = 0;
    const int rc = pool_fields_parse(F, field_len, pf, Ls, maxL);
    if (rc != MREC_OK) return rc;
    if (ldo == 0) ldo = (int64_t)F * D;
    if (ldo < (int64_t)F * D) return MREC_EINVAL;
    return pool_clip_run(table, V, ld, D, rows, 4, keys, key_bytes, B, F, Ls, maxL, pf, mask, mode,
                         MapDefault{seed, sigma, fill}, max_norm, out, out_kind, ldo, stream);
}
