// mrec_multitable.hip -- the input stage of the reference's multitable Wide&Deep as ONE launch, for gfx950: the 16-bit (or fp32) input
// row of dense_layer_1 and the wide logit term beside it.
//
// Reference call sites: models/wide_and_deep_multitable/src/wide_and_deep.py:286-352 (input_embedding = Concat((val_hldr * 1, ind_emb,
// emb128_id_emb, emb64_sgl_emb, mult_embedding)): three Gather + Flatten, six Gather -> Mul(mask) -> ReduceMean(axis 1)) and :361-424
// (wide_out: Mul + ReduceSum of the continuous values, four Gather + ReduceSum, six Gather -> Mul(mask) -> ReduceSum, BiasAdd).
//
// Per sample b (the contract: include/mrec.h, mrec_mt_input):
//   x[b, 0:C]                         = cont[b, :]
//   x[b, col + s*D : col + (s+1)*D]   = table[ids[b, s]] * mask[b, s]                     (pooled == 0: L rows side by side)
//   x[b, col : col + D]               = (sum_s table[ids[b, s]] * mask[b, s]) / (float)L  (pooled == 1)
//   x[b, every other column < K0]     = +0
//   wide_out[b]                       = sum_c cont[b, c] * wide_cont[c] + sum_segments sum_s wide[ids[b, s]] * mask[b, s] + *wide_bias
// The deep arithmetic is mrec_gather_rows' (pooled == 0) and mrec_gather_pool_fields' mode 1 (pooled == 1), operation for operation:
// an id outside [0, V) is a +0.0 row, multiplied and added like any other; slot 0's product starts a pooled sum, every later slot is
// product then add (no fma: -ffp-contract=off) in ascending slot order, one IEEE division by (float)L, 16-bit outputs rounded once.
//
// Shape of the kernel: k_gather_rows' / k_gather_pool_fields' (mrec_gather.hip, mrec_pool.hip) -- a lane-group of lpr lanes holds a
// row, four columns per lane (float4 loads); the PB ids and mask values of a batch of slots are requested first, then the PB rows,
// all unconditionally at clamped addresses (a slot past the end reads the last slot, an id out of range row 0, a sample past the end
// the last sample; the values are dropped by selects), then the adds in slot order; one store per lane comes last.  No barriers, no
// LDS, no atomics.
// Work items: an ITEM is one output block of a sample -- the continuous block, a segment's block, a run of columns nobody covers
// (written as zero), or the wide sum -- and a work item is (item, sample), ITEM-major: a workgroup belongs to ONE item (it finds it
// from its block index in a table of first blocks) and its lane-groups take consecutive samples.  Every segment has an id tensor of
// its own ([B, L_i], the reference's twelve multi-hot tensors stay separate), so consecutive samples of one item read consecutive ids
// -- the start of the chain of dependent loads -- and the item's kind, its table, D, L and lane geometry are uniform over the
// workgroup: scalar registers and scalar branches, no divergence between lane-groups.  Each item has its own geometry: lpr = the
// power of two >= D / 4 (D <= 256: one column block), so a 128-wide row of the large table is one 512-byte request of 32 lanes.
// The wide sum: 16 lanes per sample; lane j takes terms j, j + 16, .. of the sample's term list (the C continuous products first, then
// every slot of every segment that has wide weights, in segment and slot order) in ascending order, then a butterfly over the 16
// lanes.  The order is a function of the layout alone: the same bits on every run.
// The descriptors travel BY VALUE in the kernel's arguments (under 3 KiB): no table in device memory, no copy, no allocation, no
// synchronisation -- the entry is one launch and capturable.
#include "mrec_common.h"

namespace {

// output rows: fp32, bf16 or IEEE half (round-to-nearest-even, once), as the lookups' (mrec_gather.hip; the tags: mrec_common.h)
__device__ __forceinline__ unsigned f2h2(float lo, float hi) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 v = {(_Float16)lo, (_Float16)hi};
    return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ void vstore(float* p, const float4& x) { *(float4*)p = x; }
__device__ __forceinline__ void vstore(bf16o_t* p, const float4& x) {
    uint2 u;
    u.x = (unsigned)f2bf(x.x) | ((unsigned)f2bf(x.y) << 16);
    u.y = (unsigned)f2bf(x.z) | ((unsigned)f2bf(x.w) << 16);
    *(uint2*)p = u;
}
__device__ __forceinline__ void vstore(f16o_t* p, const float4& x) { *(uint2*)p = make_uint2(f2h2(x.x, x.y), f2h2(x.z, x.w)); }
__device__ __forceinline__ float4 vscale(float4 x, float s) { x.x *= s; x.y *= s; x.z *= s; x.w *= s; return x; }
__device__ __forceinline__ float4 vadd(float4 a, const float4& b) { a.x = a.x + b.x; a.y = a.y + b.y; a.z = a.z + b.z; a.w = a.w + b.w; return a; }
__device__ __forceinline__ float4 vdiv(float4 x, float d) { x.x = x.x / d; x.y = x.y / d; x.z = x.z / d; x.w = x.w / d; return x; }
// "this value is needed here" (see k_gather_rows, mrec_gather.hip)
__device__ __forceinline__ void vtouch(float4& r) { asm volatile("" : "+v"(r.x), "+v"(r.y), "+v"(r.z), "+v"(r.w)); }

enum : int { kItemCont = 0, kItemSeg = 1, kItemZero = 2, kItemWide = 3 };
constexpr int kMaxItems = 2 * MREC_MT_MAX_SEGS + 4;      // the continuous block, the segments, the gaps between and around them, the wide sum
constexpr int kWideLanes = 16;

struct MtSeg {                     // a segment's deep side
    const float* table; const int32_t* ids; const float* mask;
    int64_t V, ld, ld_ids;
    int D, L, pooled, col;
};
struct MtWide {                    // a segment's wide side (segments without wide weights have none)
    const float* wide; const int32_t* ids; const float* mask;
    int64_t V, ld_ids;
};
struct MtItem { int kind, seg, col, width, lpr; unsigned blk0; };      // blk0: the item's first workgroup; seg: kItemSeg's segment
struct MtArgs {
    const float* cont; int64_t ld_cont; int C;
    const float* wide_cont; const float* wide_bias;
    int64_t B, ldx;
    float* wide_out;
    int n_items, n_wide, n_terms;              // n_terms: slots of all wide sides
    MtItem item[kMaxItems];
    MtSeg seg[MREC_MT_MAX_SEGS];
    MtWide ws[MREC_MT_MAX_SEGS];
    int woff[MREC_MT_MAX_SEGS + 1];            // woff[j]: the first term of wide side j
};

// one segment's block of one sample: PB slots in flight.  POOLED: k_gather_pool_fields' bag (mode 1); else k_gather_rows' rows, L of them.
template <int PB, bool POOLED, class OT>
__device__ __forceinline__ void seg_item(const MtSeg& s, int64_t b, bool live, int sub, OT* __restrict__ xb) {
    const int col = sub * 4;
    if (col >= s.D) return;                                       // spare lanes of a lane-group wider than the row
    const int32_t* __restrict__ idb = s.ids + b * s.ld_ids;
    const float* __restrict__ mb = s.mask ? s.mask + b * s.ld_ids : nullptr;
    const int L = s.L, llast = L - 1;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int l0 = 0; l0 < L; l0 += PB) {
        int64_t row[PB];
        float mk[PB];
        float4 x[PB];
        bool okr[PB];
#pragma unroll
        for (int k = 0; k < PB; ++k) {
            const int lc = l0 + k < L ? l0 + k : llast;           // (a slot past the end reads the last slot: inside the row of ids)
            row[k] = (int64_t)idb[lc];
            mk[k] = mb ? mb[lc] : 1.0f;
        }
#pragma unroll
        for (int k = 0; k < PB; ++k) {
            okr[k] = row[k] >= 0 && row[k] < s.V;
            x[k] = *(const float4*)(s.table + (okr[k] ? row[k] : 0) * s.ld + col);
        }
#pragma unroll
        for (int k = 0; k < PB; ++k) {
            vtouch(x[k]);
            if (!okr[k]) x[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int k = 0; k < PB; ++k) {
            if (l0 + k < L) {
                const float4 p = mb ? vscale(x[k], mk[k]) : x[k];
                if constexpr (POOLED) {
                    acc = (l0 + k == 0) ? p : vadd(acc, p);       // slot 0 starts the sum
                } else {
                    if (live) vstore(xb + s.col + (int64_t)(l0 + k) * s.D + col, p);
                }
            }
        }
    }
    if constexpr (POOLED) {
        acc = vdiv(acc, (float)L);
        if (live) vstore(xb + s.col + col, acc);
    }
}

template <class OT>
__global__ __launch_bounds__(256) void k_mt_input(OT* __restrict__ x, const MtArgs a) {
    int it = 0;
    for (int i = 1; i < a.n_items; ++i) it += blockIdx.x >= a.item[i].blk0 ? 1 : 0;      // (uniform: the workgroup's item)
    const MtItem im = a.item[it];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lpr = im.lpr, G = 64 / lpr;                         // (lpr is a power of two: no spare lane-group)
    const int grp = lane / lpr, sub = lane - grp * lpr;
    const int64_t bw = ((int64_t)(blockIdx.x - im.blk0) * 4 + wave) * G + grp;
    const bool live = bw < a.B;
    const int64_t b = live ? bw : a.B - 1;                        // a sample past the end reads the last sample, and stores nothing
    OT* __restrict__ xb = x + b * a.ldx;
    if (im.kind == kItemSeg) {
        const MtSeg& s = a.seg[im.seg];
        // slots in flight: 2, 4 or 8 -- the reference's fields are 2 .. 5 long, and a slot past the end is a request for nothing
        if (s.pooled) {
            if (s.L <= 2) seg_item<2, true>(s, b, live, sub, xb);
            else if (s.L <= 4) seg_item<4, true>(s, b, live, sub, xb);
            else seg_item<8, true>(s, b, live, sub, xb);
        } else {
            if (s.L <= 2) seg_item<2, false>(s, b, live, sub, xb);
            else if (s.L <= 4) seg_item<4, false>(s, b, live, sub, xb);
            else seg_item<8, false>(s, b, live, sub, xb);
        }
    } else if (im.kind == kItemCont) {                            // val_hldr * 1: the values themselves, in the net's type
        const float* __restrict__ cb = a.cont + b * a.ld_cont;
        for (int c = sub * 4; c < a.C; c += lpr * 4) {
            const float4 v = *(const float4*)(cb + c);
            if (live) vstore(xb + c, v);
        }
    } else if (im.kind == kItemZero) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int c = sub * 4; c < im.width; c += lpr * 4)
            if (live) vstore(xb + im.col + c, z);
    } else {                                                      // the wide sum: terms sub, sub + 16, .. then a butterfly
        float acc = 0.0f;
        if (a.C > 0) {
            const float* __restrict__ cb = a.cont + b * a.ld_cont;
            for (int c = sub; c < a.C; c += kWideLanes) acc = acc + cb[c] * a.wide_cont[c];
        }
        const int T = a.n_terms;
        for (int t0 = 0; t0 < T; t0 += 4 * kWideLanes) {          // four terms in flight per lane
            float w[4], mk[4];
            int64_t row[4];
            int j[4];
            bool has[4], okr[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int t = t0 + k * kWideLanes + sub;
                has[k] = t < T;
                const int tc = has[k] ? t : T - 1;                // (a term past the end reads the last term)
                int jj = 0;
                for (int i = 1; i < a.n_wide; ++i) jj += tc >= a.woff[i] ? 1 : 0;
                j[k] = jj;
                const int sl = tc - a.woff[jj];
                const MtWide& ws = a.ws[jj];
                row[k] = (int64_t)ws.ids[b * ws.ld_ids + sl];
                mk[k] = ws.mask ? ws.mask[b * ws.ld_ids + sl] : 1.0f;
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const MtWide& ws = a.ws[j[k]];
                okr[k] = row[k] >= 0 && row[k] < ws.V;
                w[k] = ws.wide[okr[k] ? row[k] : 0];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (has[k] && okr[k]) acc = acc + (a.ws[j[k]].mask ? w[k] * mk[k] : w[k]);      // (an id out of range contributes nothing)
            }
        }
#pragma unroll
        for (int m = 1; m < kWideLanes; m <<= 1) acc = acc + __shfl_xor(acc, m, 64);      // (partners inside the lane-group: m < 16)
        if (live && sub == 0) a.wide_out[b] = acc + a.wide_bias[0];
    }
}

inline int pow2_lanes(int quads) {       // lanes of a lane-group that holds `quads` float4 columns: a power of two, at most a wave
    int l = 1;
    while (l < quads && l < 64) l <<= 1;
    return l;
}

template <class OT>
int mt_launch(OT* x, const MtArgs& a, unsigned blocks, hipStream_t st) {
    k_mt_input<OT><<<blocks, 256, 0, st>>>(x, a);
    MREC_LAUNCH_CHECK();
    return MREC_OK;
}

}  // namespace

MREC_API int mrec_mt_input(const float* cont, int64_t ld_cont, int32_t C, const float* wide_cont, const float* wide_bias,
                           const mrec_mt_seg_t* segs, int32_t n_segs, int64_t B, void* x, int32_t out_kind, int64_t ldx, int32_t K0,
                           float* wide_out, void* stream) {
    // 1. the record: MREC_EINVAL
    if (n_segs < 0 || n_segs > MREC_MT_MAX_SEGS || (n_segs > 0 && !segs)) return MREC_EINVAL;
    if (B < 0 || C < 0 || K0 < 0 || out_kind < 0 || out_kind > 2 || ldx < K0 || (C > 0 && ld_cont < C)) return MREC_EINVAL;
    int64_t slots = 0;
    for (int i = 0; i < n_segs; ++i) {
        const mrec_mt_seg_t& s = segs[i];
        if (s.L < 1 || (s.pooled != 0 && s.pooled != 1) || s.D < 1 || s.V < 0 || s.ld < s.D || s.ld_ids < s.L || s.col < 0) return MREC_EINVAL;
        slots += s.L;
    }
    // 2. shapes outside what the kernel covers: MREC_EUNSUPPORTED
    if (C % 8 || K0 % 8 || ldx % 8 || (C > 0 && ld_cont % 4)) return MREC_EUNSUPPORTED;
    for (int i = 0; i < n_segs; ++i) {
        const mrec_mt_seg_t& s = segs[i];
        if (s.D % 8 || s.D > 256 || s.col % 8 || s.ld % 4) return MREC_EUNSUPPORTED;
    }
    if (slots > MREC_POOL_MAX_BAG) return MREC_EUNSUPPORTED;
    if (B * n_segs > (int64_t(1) << 31) - 1) return MREC_EUNSUPPORTED;
    // 3. the layout: the blocks in column order, disjoint and inside [0, K0); the gaps become zero items
    struct Blk { int64_t c0, c1; int seg; };
    Blk blk[MREC_MT_MAX_SEGS + 1];
    int nb = 0;
    if (C > 0) blk[nb++] = {0, C, -1};
    for (int i = 0; i < n_segs; ++i) {
        const int64_t w = (int64_t)segs[i].D * (segs[i].pooled ? 1 : segs[i].L);
        Blk nbk{segs[i].col, segs[i].col + w, i};
        int p = nb++;
        for (; p > 0 && blk[p - 1].c0 > nbk.c0; --p) blk[p] = blk[p - 1];
        blk[p] = nbk;
    }
    for (int p = 0; p < nb; ++p) {
        if (blk[p].c1 > K0 || (p > 0 && blk[p].c0 < blk[p - 1].c1)) return MREC_EINVAL;
    }
    if (B == 0) return MREC_OK;
    // 4. pointers and their alignment
    if (!x || !wide_out || !wide_bias || (C > 0 && (!cont || !wide_cont))) return MREC_EINVAL;
    for (int i = 0; i < n_segs; ++i) {
        if (!segs[i].table || !segs[i].ids || segs[i].V == 0) return MREC_EINVAL;      // (rows are read at clamped addresses: no empty table)
    }
    if (!al16(x) || (C > 0 && !al16(cont))) return MREC_EUNSUPPORTED;
    for (int i = 0; i < n_segs; ++i) {
        if (!al16(segs[i].table)) return MREC_EUNSUPPORTED;
    }

    MtArgs a{};
    a.cont = cont; a.ld_cont = ld_cont; a.C = C; a.wide_cont = wide_cont; a.wide_bias = wide_bias;
    a.B = B; a.ldx = ldx; a.wide_out = wide_out;
    uint64_t nblocks = 0;
    const auto add_item = [&](int kind, int seg, int64_t col, int64_t width, int lpr) {
        MtItem& im = a.item[a.n_items++];
        im = {kind, seg, (int)col, (int)width, lpr, (unsigned)nblocks};
        nblocks += (uint64_t)mrec_cdiv(B, (int64_t)4 * (64 / lpr));
    };
    // the segments first, in the caller's order (the rows of a table that does not sit in cache are requested early), then the cheap items
    for (int i = 0; i < n_segs; ++i) {
        const mrec_mt_seg_t& s = segs[i];
        a.seg[i] = {s.table, s.ids, s.mask, s.V, s.ld, s.ld_ids, s.D, s.L, s.pooled, s.col};
        add_item(kItemSeg, i, s.col, 0, pow2_lanes(s.D / 4));
        if (s.wide) {
            a.ws[a.n_wide] = {s.wide, s.ids, s.mask, s.V, s.ld_ids};
            a.woff[a.n_wide++] = a.n_terms;
            a.n_terms += s.L;
        }
    }
    a.woff[a.n_wide] = a.n_terms;
    if (C > 0) add_item(kItemCont, 0, 0, C, pow2_lanes(C / 4));
    int64_t at = 0;
    for (int p = 0; p <= nb; ++p) {                               // the columns of [0, K0) that no block covers
        const int64_t c0 = p < nb ? blk[p].c0 : K0;
        if (c0 > at) add_item(kItemZero, 0, at, c0 - at, pow2_lanes((int)((c0 - at) / 4 < 64 ? (c0 - at) / 4 : 64)));
        if (p < nb) at = blk[p].c1;
    }
    add_item(kItemWide, 0, 0, 0, kWideLanes);
    if (nblocks > 0x7FFFFFFFull) return MREC_EUNSUPPORTED;         // (the grid's x extent)
    hipStream_t st = (hipStream_t)stream;
    return by_out(x, out_kind, [&](auto* op) { return mt_launch(op, a, (unsigned)nblocks, st); });
}
