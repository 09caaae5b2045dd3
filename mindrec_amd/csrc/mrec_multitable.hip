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

// ---- the backward: mrec_mt_input_bwd (the contract and the order of every sum: include/mrec.h) ------------------------------------
// g_x's column blocks -> per-table row-gradient sums, g_wide -> the wide weights' gradient sums, both per GROUP of a sparse plan over
// the table's ids, and the continuous weights' / the bias' gradients.  Shape: a wave per run of the sorted index; lpr lanes hold a
// gradient row, eight columns each (one 16-byte load of a 16-bit gradient, two of an fp32 one), so a wave-instruction requests
// R = 64 / lpr rows, kBwUn of them in flight per lane; fp32 accumulation, a butterfly over the row slots last.  The first launch has
// three kinds of work, each in workgroups of its own (a workgroup's kind, group and geometry are uniform: scalar branches):
//   group waves   stride over the group indices u < U: a group of at most CHUNK positions is one run, its sums are stored at once;
//   window waves  stride over the windows of CHUNK sorted entries of a group's index that has more than CHUNK entries: a window meets
//                 at most two LONG groups (one that holds its first entry, one that holds its last: a third would have to fit inside),
//                 and their pieces go to slots 0 / 1 of the window's workspace record [2][D + 4] (column D: the wide sum);
//   slabs         256 samples of g_wide x cont.
// The second launch (only where a group can be long or there is more than one slab) folds: a wave per window adds the pieces of the
// long group that BEGINS in that window, in window order -- nobody waits for anybody: the launch boundary is the only hand-off.
namespace {

constexpr int kBwUn = 4;                          // rows in flight per lane
constexpr int kBwMaxWaves = 8192;                 // waves of one kind of work of one group: 256 CUs x 32
constexpr int kBwSlab = 256;                      // samples of a slab
constexpr int kBwPad = 4;                         // floats behind the D columns of a workspace record: [0] the wide sum

struct BwSeg { const float* mask; int64_t ld_mask; int s0, L, col, pooled; float inv_l; };
struct BwGrp {
    const int32_t* sorted_pos; const int32_t* sorted_seg; const int32_t* seg_offsets; const int64_t* n_uniq;
    float* sums; float* wsums; float* part;
    int64_t n;
    int D, Ls, seg0, nseg, lpr;
    unsigned blk_g, nblk_g, blk_w, nblk_w, blk_f, nblk_f;      // first workgroup and workgroups of: group waves, window waves, the fold
};
struct BwArgs {
    int64_t ldg, ld_cont, B;
    const float* g_wide; const float* cont;
    float* d_cont; float* d_bias; float* part_cont;
    float grad_scale;
    int C, n_groups, fold;
    unsigned blk_cont, blk_cont_f;                // the slabs' first workgroup; the fold launch's workgroup for them
    BwGrp grp[MREC_MT_BWD_MAX_GROUPS];
    BwSeg seg[MREC_MT_MAX_SEGS];
};

struct g_bf16_t { uint16_t v; };
struct g_f16_t { uint16_t v; };
__device__ __forceinline__ void bw_load8(const float* p, float v[8]) {
    const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void bw_load8(const g_bf16_t* p, float v[8]) {
    const uint4 u = *(const uint4*)p;
    const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = __uint_as_float(w[i] << 16); v[2 * i + 1] = __uint_as_float(w[i] & 0xFFFF0000u); }
}
__device__ __forceinline__ void bw_load8(const g_f16_t* p, float v[8]) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const uint4 u = *(const uint4*)p;
    const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) { const h2 h = __builtin_bit_cast(h2, w[i]); v[2 * i] = (float)h.x; v[2 * i + 1] = (float)h.y; }
}

// one run [e0, e1) of a group's sorted index: acc[8] (this lane's columns) and wacc, the same bits in every lane of a column / in every lane
template <class GT>
__device__ __forceinline__ void bw_run(const BwArgs& a, const BwGrp& gr, const GT* __restrict__ g, int64_t e0, int64_t e1, int lane,
                                       float acc[8], float& wacc) {
    const int lpr = gr.lpr, R = 64 / lpr;
    const int r = lane / lpr, c0 = (lane - r * lpr) * 8;
    const bool colok = c0 < gr.D, wide = gr.wsums != nullptr;
    const unsigned Ls = (unsigned)gr.Ls, nmax = (unsigned)(gr.n - 1);
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[i] = 0.0f;
    wacc = 0.0f;
    for (int64_t eb = e0; eb < e1; eb += (int64_t)kBwUn * R) {
        unsigned pos[kBwUn];
        bool has[kBwUn];
        float x[kBwUn][8], m[kBwUn], sc[kBwUn], gw[kBwUn];
#pragma unroll
        for (int k = 0; k < kBwUn; ++k) {
            const int64_t e = eb + (int64_t)k * R + r;
            has[k] = e < e1;
            pos[k] = 0;
            if (has[k]) {                          // (a slot past the end of the run requests nothing: short runs are the common case)
                const unsigned p = (unsigned)gr.sorted_pos[e];
                pos[k] = p < nmax ? p : nmax;      // a position is a position: inside [0, n)
            }
        }
#pragma unroll
        for (int k = 0; k < kBwUn; ++k) {
            m[k] = sc[k] = gw[k] = 0.0f;
            if (!has[k]) continue;
            const unsigned b = pos[k] / Ls, s = pos[k] - b * Ls;
            int j = gr.seg0;
            for (int i = 1; i < gr.nseg; ++i) j += (int)s >= a.seg[gr.seg0 + i].s0 ? 1 : 0;
            const BwSeg& sg = a.seg[j];
            const int sl = (int)s - sg.s0;
            m[k] = sg.mask ? sg.mask[(int64_t)b * sg.ld_mask + sl] : 1.0f;
            sc[k] = sg.pooled ? m[k] * sg.inv_l : m[k];
            gw[k] = wide ? a.g_wide[b] : 0.0f;
            const int col = sg.col + (sg.pooled ? 0 : sl * gr.D);
            if (colok) bw_load8(g + (int64_t)b * a.ldg + col + c0, x[k]);
        }
#pragma unroll
        for (int k = 0; k < kBwUn; ++k) {
            if (has[k]) {
                if (colok) {
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[i] = acc[i] + x[k][i] * sc[k];
                }
                wacc = wacc + gw[k] * m[k];
            }
        }
    }
    for (int d = lpr; d < 64; d <<= 1) {          // the row slots
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = acc[i] + __shfl_xor(acc[i], d, 64);
        wacc = wacc + __shfl_xor(wacc, d, 64);
    }
}

__device__ __forceinline__ void bw_store(float* __restrict__ dst, float* __restrict__ wdst, int D, int lpr, int lane, const float acc[8],
                                         float wacc, float gs) {
    const int c0 = lane * 8;
    if (lane < lpr && c0 < D) {
        *(float4*)(dst + c0) = make_float4(acc[0] * gs, acc[1] * gs, acc[2] * gs, acc[3] * gs);
        *(float4*)(dst + c0 + 4) = make_float4(acc[4] * gs, acc[5] * gs, acc[6] * gs, acc[7] * gs);
    }
    if (wdst && lane == 0) *wdst = wacc * gs;
}

// a group's bounds in the sorted index, inside [0, n] whatever the index holds
__device__ __forceinline__ void bw_bounds(const BwGrp& gr, int64_t u, int64_t& o0, int64_t& o1) {
    o0 = gr.seg_offsets[u];
    o1 = gr.seg_offsets[u + 1];
    o0 = o0 < 0 ? 0 : (o0 > gr.n ? gr.n : o0);
    o1 = o1 < o0 ? o0 : (o1 > gr.n ? gr.n : o1);
}
__device__ __forceinline__ int64_t bw_count(const BwGrp& gr) {
    const int64_t U = *gr.n_uniq;
    return U < 0 ? 0 : (U > gr.n ? gr.n : U);
}

template <class GT>
__global__ __launch_bounds__(256) void k_mt_input_bwd(const GT* __restrict__ g, const BwArgs a) {
    __shared__ float red[4][64];
    const unsigned blk = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blk >= a.blk_cont) {                      // a slab of samples: column c of cont (column C: ones, the bias) times g_wide
        const int64_t b0 = (int64_t)(blk - a.blk_cont) * kBwSlab + wave * 64;
        for (int cb = 0; cb <= a.C; cb += 64) {
            const int c = cb + lane;
            float acc = 0.0f;
            if (c <= a.C) {
                for (int i = 0; i < 64; ++i) {
                    const int64_t b = b0 + i;
                    if (b < a.B) acc = acc + a.g_wide[b] * (c < a.C ? a.cont[b * a.ld_cont + c] : 1.0f);
                }
            }
            red[wave][lane] = acc;
            __syncthreads();
            if (wave == 0 && c <= a.C) {
                const float t = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
                if (a.fold) a.part_cont[(int64_t)(blk - a.blk_cont) * (a.C + 1) + c] = t;
                else if (c < a.C) a.d_cont[c] = t * a.grad_scale;
                else a.d_bias[0] = t * a.grad_scale;
            }
            __syncthreads();
        }
        return;
    }
    int gi = 0, win = 0;                          // (uniform: the workgroup's group and kind)
    for (int i = 0; i < a.n_groups; ++i) {
        if (blk >= a.grp[i].blk_g) { gi = i; win = 0; }
        if (a.grp[i].nblk_w > 0 && blk >= a.grp[i].blk_w) { gi = i; win = 1; }
    }
    const BwGrp& gr = a.grp[gi];
    const int64_t U = bw_count(gr);
    float acc[8], wacc;
    if (!win) {
        const int64_t nw = (int64_t)gr.nblk_g * 4;
        for (int64_t u = (int64_t)(blk - gr.blk_g) * 4 + wave; u < U; u += nw) {
            int64_t o0, o1;
            bw_bounds(gr, u, o0, o1);
            if (o1 - o0 > MREC_MT_BWD_CHUNK) continue;            // a long group: the window waves and the fold
            bw_run(a, gr, g, o0, o1, lane, acc, wacc);
            bw_store(gr.sums + u * gr.D, gr.wsums ? gr.wsums + u : nullptr, gr.D, gr.lpr, lane, acc, wacc, a.grad_scale);
        }
        return;
    }
    const int64_t nw = (int64_t)gr.nblk_w * 4, nwin = (gr.n + MREC_MT_BWD_CHUNK - 1) / MREC_MT_BWD_CHUNK;
    for (int64_t c = (int64_t)(blk - gr.blk_w) * 4 + wave; c < nwin; c += nw) {
        const int64_t e0 = c * MREC_MT_BWD_CHUNK, e1 = e0 + MREC_MT_BWD_CHUNK < gr.n ? e0 + MREC_MT_BWD_CHUNK : gr.n;
        const int64_t ua = gr.sorted_seg[e0], ub = gr.sorted_seg[e1 - 1];
        for (int slot = 0; slot < 2; ++slot) {
            const int64_t u = slot ? ub : ua;
            if ((slot && ub == ua) || u < 0 || u >= U) continue;
            int64_t o0, o1;
            bw_bounds(gr, u, o0, o1);
            if (o1 - o0 <= MREC_MT_BWD_CHUNK) continue;
            const int64_t lo = o0 > e0 ? o0 : e0, hi = o1 < e1 ? o1 : e1;
            if (hi <= lo) continue;
            bw_run(a, gr, g, lo, hi, lane, acc, wacc);
            float* rec = gr.part + (c * 2 + slot) * (gr.D + kBwPad);
            bw_store(rec, rec + gr.D, gr.D, gr.lpr, lane, acc, wacc, 1.0f);
        }
    }
}

// the pieces of the long groups, added in window order; the slabs, in slab order
__global__ __launch_bounds__(256) void k_mt_input_bwd_fold(const BwArgs a) {
    const unsigned blk = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (blk == a.blk_cont_f) {
        if (wave != 0) return;
        const int64_t ns = (a.B + kBwSlab - 1) / kBwSlab;
        for (int c = lane; c <= a.C; c += 64) {
            float t = a.part_cont[c];
            for (int64_t s = 1; s < ns; ++s) t = t + a.part_cont[s * (a.C + 1) + c];
            if (c < a.C) a.d_cont[c] = t * a.grad_scale;
            else a.d_bias[0] = t * a.grad_scale;
        }
        return;
    }
    int gi = 0;
    for (int i = 1; i < a.n_groups; ++i) gi = (a.grp[i].nblk_f > 0 && blk >= a.grp[i].blk_f) ? i : gi;
    const BwGrp& gr = a.grp[gi];
    const int64_t U = bw_count(gr);
    const int64_t nw = (int64_t)gr.nblk_f * 4, nwin = (gr.n + MREC_MT_BWD_CHUNK - 1) / MREC_MT_BWD_CHUNK;
    const int D = gr.D, stride = D + kBwPad, c4 = lane * 4;
    for (int64_t c = (int64_t)(blk - gr.blk_f) * 4 + wave; c < nwin; c += nw) {
        const int64_t e0 = c * MREC_MT_BWD_CHUNK, e1 = e0 + MREC_MT_BWD_CHUNK < gr.n ? e0 + MREC_MT_BWD_CHUNK : gr.n;
        const int64_t ua = gr.sorted_seg[e0], ub = gr.sorted_seg[e1 - 1];
        for (int slot = 0; slot < 2; ++slot) {
            const int64_t u = slot ? ub : ua;
            if ((slot && ub == ua) || u < 0 || u >= U) continue;
            int64_t o0, o1;
            bw_bounds(gr, u, o0, o1);
            // the group that BEGINS here: at the window's first entry (slot 0) or inside it (slot 1)
            if (o1 - o0 <= MREC_MT_BWD_CHUNK || o0 < e0 || o0 >= e1 || (slot == 0) != (o0 == e0)) continue;
            const int64_t c1 = (o1 - 1) / MREC_MT_BWD_CHUNK;
            const float* __restrict__ rec = gr.part + (c * 2 + slot) * stride;
            float4 s = c4 < D ? *(const float4*)(rec + c4) : make_float4(0.f, 0.f, 0.f, 0.f);
            float w = rec[D];
#pragma unroll 4
            for (int64_t cc = c + 1; cc <= c1; ++cc) {            // every later window holds the group at its first entry: slot 0
                rec = gr.part + cc * 2 * stride;
                if (c4 < D) s = vadd(s, *(const float4*)(rec + c4));
                w = w + rec[D];
            }
            if (c4 < D) *(float4*)(gr.sums + u * D + c4) = vscale(s, a.grad_scale);
            if (gr.wsums && lane == 0) gr.wsums[u] = w * a.grad_scale;
        }
    }
}

// the layout of a call: the segments flattened, the workgroups of every kind of work, the workspace carved.  MREC_OK or the refusal.
int bw_plan(const mrec_mt_grp_t* groups, int32_t n_groups, int64_t B, int32_t C, int32_t K0, int64_t ldg, MrecArena& ar, BwArgs& a,
            unsigned* blocks, unsigned* blocks_f) {
    // 1. the record
    if (n_groups < 0 || n_groups > MREC_MT_BWD_MAX_GROUPS || (n_groups > 0 && !groups) || B < 0 || C < 0 || K0 < 0) return MREC_EINVAL;
    int total = 0;
    for (int gq = 0; gq < n_groups; ++gq) {
        const mrec_mt_grp_t& q = groups[gq];
        if (q.n_segs < 1 || !q.segs || q.n < 0) return MREC_EINVAL;
        total += q.n_segs;
        if (total > MREC_MT_MAX_SEGS) return MREC_EINVAL;
        int64_t Ls = 0;
        for (int i = 0; i < q.n_segs; ++i) {
            const mrec_mt_seg_t& s = q.segs[i];
            if (s.L < 1 || (s.pooled != 0 && s.pooled != 1) || s.D < 1 || s.ld_ids < s.L || s.col < 0) return MREC_EINVAL;
            Ls += s.L;
        }
        for (int i = 1; i < q.n_segs; ++i) {
            if (q.segs[i].D != q.segs[0].D) return MREC_EINVAL;
        }
        if (q.n % Ls || q.n / Ls != B) return MREC_EINVAL;
    }
    // 2. shapes outside what the kernels cover
    if (K0 % 8 || ldg % 8) return MREC_EUNSUPPORTED;
    for (int gq = 0; gq < n_groups; ++gq) {
        for (int i = 0; i < groups[gq].n_segs; ++i) {
            const mrec_mt_seg_t& s = groups[gq].segs[i];
            if (s.D % 8 || s.D > 256 || s.col % 8) return MREC_EUNSUPPORTED;
        }
        if (groups[gq].n > (int64_t(1) << 31) - 1) return MREC_EUNSUPPORTED;
    }
    // 3. the column blocks
    for (int gq = 0; gq < n_groups; ++gq) {
        for (int i = 0; i < groups[gq].n_segs; ++i) {
            const mrec_mt_seg_t& s = groups[gq].segs[i];
            if ((int64_t)s.col + (int64_t)s.D * (s.pooled ? 1 : s.L) > K0) return MREC_EINVAL;
        }
    }
    a.B = B; a.C = C; a.n_groups = n_groups;
    a.fold = (C > 0 && B > kBwSlab) ? 1 : 0;
    for (int gq = 0; gq < n_groups; ++gq) a.fold |= groups[gq].n > MREC_MT_BWD_CHUNK ? 1 : 0;
    uint64_t nb = 0, nbf = 0;
    int seg = 0;
    for (int gq = 0; gq < n_groups; ++gq) {
        const mrec_mt_grp_t& q = groups[gq];
        BwGrp& gr = a.grp[gq];
        gr.sorted_pos = q.sorted_pos; gr.sorted_seg = q.sorted_seg; gr.seg_offsets = q.seg_offsets; gr.n_uniq = q.n_uniq_dev;
        gr.sums = q.sums; gr.wsums = q.wsums; gr.n = q.n;
        gr.D = q.segs[0].D; gr.seg0 = seg; gr.nseg = q.n_segs; gr.lpr = pow2_lanes(gr.D / 8);
        int s0 = 0;
        for (int i = 0; i < q.n_segs; ++i) {
            const mrec_mt_seg_t& s = q.segs[i];
            a.seg[seg++] = {s.mask, s.ld_ids, s0, s.L, s.col, s.pooled, 1.0f / (float)s.L};
            s0 += s.L;
        }
        gr.Ls = s0;
        const int64_t nwin = q.n > MREC_MT_BWD_CHUNK ? mrec_cdiv(q.n, MREC_MT_BWD_CHUNK) : 0;
        gr.part = nwin ? ar.take<float>((size_t)nwin * 2 * (gr.D + kBwPad)) : nullptr;
        const auto blocks_of = [](int64_t waves) { return (unsigned)mrec_cdiv(waves < kBwMaxWaves ? waves : kBwMaxWaves, 4); };
        gr.blk_g = (unsigned)nb; gr.nblk_g = blocks_of(q.n); nb += gr.nblk_g;
        gr.blk_w = (unsigned)nb; gr.nblk_w = blocks_of(nwin); nb += gr.nblk_w;
        gr.blk_f = (unsigned)nbf; gr.nblk_f = gr.nblk_w; nbf += gr.nblk_f;
    }
    a.blk_cont = (unsigned)nb;
    a.blk_cont_f = 0xFFFFFFFFu;
    a.part_cont = nullptr;
    if (C > 0) {
        const int64_t ns = mrec_cdiv(B, kBwSlab);
        if (nb + (uint64_t)ns > 0x7FFFFFFFull) return MREC_EUNSUPPORTED;
        nb += (uint64_t)ns;
        if (a.fold) {
            a.part_cont = ar.take<float>((size_t)ns * (C + 1));
            a.blk_cont_f = (unsigned)nbf++;
        }
    }
    *blocks = (unsigned)nb;
    *blocks_f = a.fold ? (unsigned)nbf : 0;
    return MREC_OK;
}

}  // namespace

MREC_API int mrec_mt_input_bwd_workspace_bytes(const mrec_mt_grp_t* groups, int32_t n_groups, int64_t B, int32_t C, size_t* out) {
    if (!out) return MREC_EINVAL;
    MrecArena ar;
    BwArgs a{};
    unsigned nb, nbf;
    const int rc = bw_plan(groups, n_groups, B, C, 0x7FFFFFF8, 0, ar, a, &nb, &nbf);
    if (rc != MREC_OK) return rc;
    *out = ar.off;
    return MREC_OK;
}

MREC_API int mrec_mt_input_bwd(const void* g_x, int32_t g_kind, int64_t ldg, int32_t K0, const float* g_wide, const float* cont,
                               int64_t ld_cont, int32_t C, const mrec_mt_grp_t* groups, int32_t n_groups, int64_t B, float grad_scale,
                               float* d_wide_cont, float* d_wide_bias, void* ws, size_t ws_bytes, void* stream) {
    if (g_kind < 0 || g_kind > 2 || (K0 >= 0 && ldg < K0) || (C > 0 && ld_cont < C) || !(grad_scale - grad_scale == 0.0f)) return MREC_EINVAL;
    MrecArena count;
    BwArgs a{};
    unsigned nb = 0, nbf = 0;
    int rc = bw_plan(groups, n_groups, B, C, K0, ldg, count, a, &nb, &nbf);
    if (rc != MREC_OK) return rc;
    if (B == 0) return MREC_OK;
    // 5. pointers, the workspace, alignment
    bool wide = C > 0;
    for (int gq = 0; gq < n_groups; ++gq) {
        const mrec_mt_grp_t& q = groups[gq];
        if (!q.sorted_pos || !q.sorted_seg || !q.seg_offsets || !q.n_uniq_dev || !q.sums) return MREC_EINVAL;
        wide = wide || q.wsums;
    }
    if (!g_x || (wide && !g_wide) || (C > 0 && (!cont || !d_wide_cont || !d_wide_bias))) return MREC_EINVAL;
    if (count.off > 0 && (!ws || ws_bytes < count.off)) return MREC_EWORKSPACE;
    if (!al16(g_x) || (count.off > 0 && !al16(ws))) return MREC_EUNSUPPORTED;
    for (int gq = 0; gq < n_groups; ++gq) {
        if (!al16(groups[gq].sums)) return MREC_EUNSUPPORTED;
    }
    MrecArena ar(ws, count.off > 0 ? ws_bytes : 0);
    a = BwArgs{};
    rc = bw_plan(groups, n_groups, B, C, K0, ldg, ar, a, &nb, &nbf);
    if (rc != MREC_OK || !ar.ok) return rc != MREC_OK ? rc : MREC_EWORKSPACE;
    a.ldg = ldg; a.ld_cont = ld_cont; a.g_wide = g_wide; a.cont = cont; a.d_cont = d_wide_cont; a.d_bias = d_wide_bias;
    a.grad_scale = grad_scale;
    if (nb == 0) return MREC_OK;
    hipStream_t st = (hipStream_t)stream;
    if (g_kind == 0) k_mt_input_bwd<float><<<nb, 256, 0, st>>>((const float*)g_x, a);
    else if (g_kind == 1) k_mt_input_bwd<g_bf16_t><<<nb, 256, 0, st>>>((const g_bf16_t*)g_x, a);
    else k_mt_input_bwd<g_f16_t><<<nb, 256, 0, st>>>((const g_f16_t*)g_x, a);
    MREC_LAUNCH_CHECK();
    if (nbf > 0) {
        k_mt_input_bwd_fold<<<nbf, 256, 0, st>>>(a);
        MREC_LAUNCH_CHECK();
    }
    return MREC_OK;
}
