// mrec_q8.hip -- row-wise int8 serving tables for gfx950: the quantize pass over a trained fp32 table and the dequantizing lookup
// (record format and the entries' contract: include/mrec.h, "row-wise 8-bit serving records").
// build-flags: -Xclang -target-feature -Xclang -packed-fp32-ops
//
// A record is [lo scale wide 0 | D codes | zero padding]: a 16-byte header chunk and C = ceil(D / 16) chunks of 16 codes, row_bytes
// in all (compact: 16 (C + 1); D = 80 -> 96 B against the 336 B the fp32 folded lookup takes out of a 1-KB training row).
//
// k_q8_quantize  lane-group = D / 4 lanes per row, one 16-byte load each (a fused training row is read in place through ld); min and
//                max travel a butterfly inside the group (ds_bpermute; both are idempotent, so a lane whose partner lies past the row
//                reads the row's last lane instead and still ends with the row's exact extremes); four codes per lane leave as one
//                dword, lane 0 stores the header as one 16-byte word, the lanes share the padding's dwords.  Workgroups are persistent
//                over V, rows are counted in 64 bits.  Roofline bytes per row: 4 D + 4 (wide) read, row_bytes written.
// k_q8_gather    lane-group = C + 1 lanes per looked-up position: lane 0 loads the header chunk, lane c the c-th chunk of 16 codes --
//                ONE 16-byte load instruction per position, GB = 4 positions in flight per group before the first store.  lo and
//                scale reach the code lanes by two ds_bpermute reads of lane 0; bytes unpack on v_cvt_f32_ubyte0..3; x' = lo + code
//                * scale (a multiply and an add, each rounded), then * row_scale.  16-bit rows round once, to nearest even, on
//                gfx950's packed conversions (v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32) and a code lane leaves with two 16-byte stores
//                (fp32 rows: four); the header lane stores the wide product pair (wide * row_scale, 0) as 8 bytes.
//                Lanes per row: D = 80 -> 6 lanes, 10 positions per wave, 60 / 64 lanes busy; D = 256 -> 17 lanes, 3 per wave, 51 / 64
//                (a group of 16 code lanes with the header fetched a second time by every lane would fill the wave at D = 256 but
//                doubles the load instructions at every D; the header lane is also where the wide product comes from).
//                Roofline bytes per position: row_bytes read (+ id, + row_scale), 2 D (16-bit) or 4 D written, + 8 (wide pair).
// k_q8_fm_lookup DeepFM's evaluation lookup (k_fm_lookup, mrec_fm.hip) over records: k_q8_gather's lane-group turned from a position
//                onto a SAMPLE -- lane 0 owns the header chunk of every record of its sample, lane c the c-th 16 codes -- walking the
//                sample's F fields four at a time: the four ids and weights, then the four records (one 16-byte load per lane per
//                field, all requested unconditionally: a field past F re-reads the batch's last field and is dropped, an id out of
//                range reads record 0 and is zeroed), consumed in straight-line code.  A code lane writes its 16 masked values per
//                field under k_q8_gather's store rule and adds them, in fp32 and before any 16-bit rounding, into s[16] and q[16]
//                (32 VGPRs), field order; the header lane stores nothing per field and only adds wide * wt into the linear sum (no
//                8-byte wide pair exists here).  Column-sum order of lin_fm: inside a code lane, each group of four columns as
//                ((p0 + p1) + (p2 + p3)), p = s^2 - q, the lane's one to four valid groups added in ascending order; then the
//                group's lanes by a shuffle-down tree at distances 16, 8, 4, 2, 1 (lane sub adds lane sub + off where that is a
//                lane of the group; the header lane enters with +0 and ends with the sum); lane 0 writes lin + 0.5f * part.  No
//                LDS arrays, no barriers, no atomics.  Four waves per workgroup, a grid stride over samples, at most 2048 workgroups.
//                Roofline bytes per sample: F (row_bytes + id + weight) read, F D 2 (16-bit rows) or F D 4, + 4 written.
// k_q8_gather_pool_fields  the multi-hot lookup (k_gather_pool_fields, mrec_pool.hip: Gather -> Mul(mask) -> ReduceMean / ReduceSum per
//                field) over records, with the wide side (the sum of every slot's masked wide weight) out of the same header loads.
//                k_q8_fm_lookup's sample lane-group, walking the sample's Ls = sum L_f slots four at a time: four ids and mask values,
//                then four records (one 16-byte load per lane per slot, all requested unconditionally: a slot past Ls re-reads the
//                sample's last slot and is dropped, an id out of range reads record 0 and is zeroed).  The dequantization is factored
//                out of the bag's sum, sum_s m (lo + c scale) = sum_s m lo + sum_s (m scale) c: every lane forms t = m * scale,
//                u = m * lo and g = m * wide from ITS chunk's first three words (only the header lane's are the header; no branch),
//                ONE ds_bpermute brings the header lane's t, and a code byte costs v_cvt_f32_ubyteN + v_fma_f32 into acc[16]; the
//                header lane's own adds carry base = sum u and wsum = sum g (a code lane's copies of them, and the header lane's acc,
//                are never read).  The slot -> field mapping is the same for every sample, so slot numbers, field ends and the
//                closing of a field live in scalar registers and uniform branches: at a field's last slot one more permute brings
//                base, y = acc + base, one IEEE division by (float)L_f for the mean, one rounding to the output kind, k_q8_gather's
//                store rule to columns f * D + col0.., and acc, base and wsum start again at +0.  Field (offset, length) words travel
//                by value in the kernel arguments (read by a uniform index: scalar loads).  No LDS arrays, no barriers, no atomics;
//                four waves per workgroup, a grid stride over samples, at most 2048 workgroups.
//                Roofline bytes per sample: Ls (row_bytes + id + mask) read, F D 2 (16-bit rows) or F D 4, + 4 (wide sum) written.
//
// Row-wise 4-bit records (include/mrec.h, "row-wise 4-bit serving records"): the same header chunk, then C4 = ceil(D / 32) chunks of 32
// codes, two a byte, column d in bits 4 d of its dword (compact: 16 (C4 + 1); D = 80 -> 64 B, which never straddles a 128-byte line).
// k_q4_quantize  lane-group = ceil(D / 8) lanes per row, TWO 16-byte loads each, so that a lane's eight codes are exactly one dword of
//                the record: one 4-byte store a lane and no nibble ever crosses a lane (D / 4 lanes with one load each, k_q8_quantize's
//                split, would leave 2-byte stores everywhere, twice the store instructions, and half the rows per wave).  Where
//                D % 8 == 4 the row's last lane holds four columns: it reads its first 16 bytes twice instead of reading past the row,
//                and still leaves a whole dword, whose upper half is the first two padding bytes -- no 2-byte store at all.  Min and
//                max travel k_q8_quantize's idempotent butterfly, lane 0 stores the header as one 16-byte word, the lanes share the
//                padding's dwords, every byte of the record is written.  D = 80 -> 10 lanes, 6 rows a wave; D = 256 -> 32 lanes, 2.
//                Persistent workgroups over V, 64-bit row numbers.  Roofline bytes per row: 4 D + 4 read, row_bytes written.
// k_q4_gather    lane-group = C4 + 1 lanes per position: lane 0 loads the header chunk, lane c the c-th 32 codes -- one 16-byte load
//                instruction per position, GB = 4 positions in flight, every load unconditional (k_q8_gather's rule).  lo and scale
//                come by two ds_bpermute reads of lane 0.  A code dword w is taken once as w & 0x0F0F0F0F (its bytes: columns 0, 2, 4,
//                6 of the dword's eight) and once as (w >> 4) & 0x0F0F0F0F (columns 1, 3, 5, 7): two integer instructions per eight
//                codes, then v_cvt_f32_ubyte0..3 on either word; byte k of the two words is the adjacent column pair (2 k, 2 k + 1),
//                which is what v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32 take, so no permute follows.  x' = lo + code * scale (a multiply
//                and an add, each rounded), then * row_scale, rounded once.  A code lane's 32 values leave as four 16-byte stores
//                (fp32 rows: eight), one per code dword; the row's last chunk holds valid = 4, 8, .., 32 columns, 16-bit rows of
//                D % 8 == 4 columns take 8-byte stores (the st16 / valid rule); the header lane stores the wide pair.
//                Lanes per row: D = 80 -> 4 lanes, 16 positions a wave, 64 / 64 lanes busy; D = 64 -> 3 lanes, 21 positions, 63 / 64;
//                D = 256 -> 9 lanes, 7 positions, 63 / 64.
//                Roofline bytes per position: row_bytes read (+ id, + row_scale), 2 D (16-bit) or 4 D written, + 8 (wide pair).
// k_q4_fm_lookup k_q8_fm_lookup's contract over 4-bit records, designed for the 32-code chunk: lane-group = C4 + 1 lanes a SAMPLE, lane 0 the
//                header chunk of each of the sample's records, lane c the c-th 32 codes, one 16-byte load a lane a field.  D = 80 -> 4
//                lanes, 16 samples a wave, 64 / 64 lanes busy (8-bit: 6 lanes, 10 samples, 60 / 64); D = 64 -> 3 lanes, 21 samples;
//                D = 256 -> 9 lanes, 7 samples.  A code lane carries s[32] and q[32]: 64 VGPRs of sums against the 8-bit kernel's 32.
//                What keeps that affordable: (1) a field is consumed one code dword at a time -- q4_dequant8's eight values are added
//                into their sums, the sums are pinned by an empty asm, then the eight values are stored -- so no more than eight y are
//                alive beside the sums (left alone the compiler sinks every add behind the batch's last store branch and keeps 32 y a
//                field in flight alive: 242 VGPRs, occupancy 2); (2) no branch on the lane's role: the header lane runs the code lanes'
//                arithmetic over its header words into sums nobody reads (valid == 0: it stores nothing and is left out of the
//                column sum) and a code lane adds its third word into a `lin` nobody reads -- a divergent branch around 64 live sums
//                cost two more registers a sum.  Four fields in flight (kQ4FmNB): 135-140 VGPRs, occupancy 3, no scratch -- the
//                8-bit kernel's occupancy (152-154 VGPRs) with 16 samples a wave for its 10, so 3 x 4 x 16 = 192 records in flight a
//                SIMD against 120.  Two fields in flight: 111-112 VGPRs, occupancy 4, 4 x 2 x 16 = 128 records in flight and twice
//                the dependent round trips a sample (20 at F = 39 for 10); three: 128-131, occupancy 3 for most instantiations;
//                four held to 128 VGPRs: 44-52 bytes of scratch.  A 16-column lane with an 8-byte load halves the sums but is the
//                8-bit geometry again (6 lanes at D = 80, 10 samples a wave) with the header lane's load of another width: not taken.
//                Column-sum order of lin_fm: inside a code lane each group of four columns as ((p0 + p1) + (p2 + p3)), p = s^2 - q, the
//                lane's one to eight valid groups in ascending order; then the lanes by a shuffle-down tree at distances 8, 4, 2, 1
//                (lane sub adds lane sub + off where that is a lane of the group; the header lane enters with +0 and ends with the
//                sum).  No LDS arrays, no barriers, no atomics; four waves a workgroup, a grid stride over samples, at most 2048
//                workgroups.  Roofline bytes per sample: F (row_bytes + id + weight) read, F D 2 or F D 4, + 4 written.
// k_q4_gather_pool_fields  k_q8_gather_pool_fields over 4-bit records: the same sample lane-group of C4 + 1 lanes, the same scalar slot and
//                field bookkeeping, four slots in flight; a code lane holds acc[32], a code costs the nibble split's share (two integer
//                instructions a dword), v_cvt_f32_ubyteN and v_fma_f32; a field leaves under k_q4_gather's store rule, one 16-byte
//                store of 16-bit values a code dword.  78-79 VGPRs, occupancy 6, no scratch (8-bit: 61-65, occupancy 7-8).
//                Roofline bytes per sample: Ls (row_bytes + id + mask) read, F D 2 (16-bit rows) or F D 4, + 4 (wide sum) written.
//
// k_q8_fm_lookup_keyed, k_q4_fm_lookup_keyed  the two FM lookups over raw keys (hash-table DeepFM frozen for serving): the keys of a batch
//                of four fields are resolved in the frozen key index (mrec_kidx.h) by the lane-group itself -- lane `sub` probes batch
//                slot `sub`, one 16-byte slot load a step, at most max_probe steps; groups of 2 and 3 lanes take two rounds -- and
//                four ds_bpermute reads hand the rows to every lane; behind them the unkeyed kernels' code, bit for bit.  A key the
//                index does not hold is row -1: a zero record.  8-bit: 152-154 VGPRs, 4-bit: 157-162, occupancy 3, no scratch.
#include "mrec_common.h"
#include "mrec_kidx.h"

namespace {

constexpr int kQ8Hdr = 16;       // bytes of the header chunk
constexpr int kQ8GB = 4;         // positions in flight per lane-group of the lookup
constexpr int kQ8FmNB = 4;       // fields in flight per lane-group of the FM lookup (8: no faster)

__device__ __forceinline__ float bperm_f(int src_lane, float v) {
    return __int_as_float(__builtin_amdgcn_ds_bpermute(src_lane << 2, __float_as_int(v)));
}

__device__ __forceinline__ float q8_code(float x, float lo, float scale) {
    const float q = fminf(rintf((x - lo) / scale), 255.0f);
    return scale > 0.0f ? q : 0.0f;
}

__global__ __launch_bounds__(256) void k_q8_quantize(const float* __restrict__ table, int64_t V, int64_t ld, int D,
                                                     const float* __restrict__ wide, int64_t ldw, uint8_t* __restrict__ rec,
                                                     int64_t row_bytes, RowGeom gm) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / gm.lpr, ds = lane - grp * gm.lpr;
    if (grp >= gm.G) return;
    const int nd = gm.lpr, lane0 = lane - ds;
    const int pad_dw = (int)((row_bytes - kQ8Hdr - D) >> 2);          // zero dwords behind the codes
    const int64_t stride = (int64_t)gridDim.x * 4 * gm.G;
    for (int64_t r = ((int64_t)blockIdx.x * 4 + wave) * gm.G + grp; r < V; r += stride) {
        const float4 x = *(const float4*)(table + r * ld + 4 * ds);
        float w = 0.0f;
        if (ds == 0 && wide) w = wide[r * ldw];
        float lo = fminf(fminf(x.x, x.y), fminf(x.z, x.w));
        float hi = fmaxf(fmaxf(x.x, x.y), fmaxf(x.z, x.w));
        for (int m = 1; m < nd; m <<= 1) {
            const int p = ds ^ m;
            const int src = lane0 + (p < nd ? p : nd - 1);
            lo = fminf(lo, bperm_f(src, lo));
            hi = fmaxf(hi, bperm_f(src, hi));
        }
        const float scale = (hi - lo) / 255.0f;
        const unsigned codes = (unsigned)q8_code(x.x, lo, scale) | ((unsigned)q8_code(x.y, lo, scale) << 8) |
                               ((unsigned)q8_code(x.z, lo, scale) << 16) | ((unsigned)q8_code(x.w, lo, scale) << 24);
        uint8_t* const o = rec + r * row_bytes;
        if (ds == 0) *(uint4*)o = make_uint4(__float_as_uint(lo), __float_as_uint(scale), __float_as_uint(w), 0u);
        *(uint32_t*)(o + kQ8Hdr + 4 * ds) = codes;
        for (int j = ds; j < pad_dw; j += nd) *(uint32_t*)(o + kQ8Hdr + D + 4 * j) = 0u;
    }
}

// four dequantized, scaled values -> 8 bytes of 16-bit output, rounded once to nearest even
__device__ __forceinline__ uint2 q8_pack16(const f16o_t*, float a, float b, float c, float d) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 u = {(_Float16)a, (_Float16)b}, v = {(_Float16)c, (_Float16)d};
    return make_uint2(__builtin_bit_cast(unsigned, u), __builtin_bit_cast(unsigned, v));
}
__device__ __forceinline__ uint2 q8_pack16(const bf16o_t*, float a, float b, float c, float d) {
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    const b2 u = {(__bf16)a, (__bf16)b}, v = {(__bf16)c, (__bf16)d};
    return make_uint2(__builtin_bit_cast(unsigned, u), __builtin_bit_cast(unsigned, v));
}

// the four codes of one dword -> x' * sc
__device__ __forceinline__ float4 q8_dequant4(unsigned w, float lo, float scale, float sc) {
    float4 y;
    y.x = (lo + (float)(w & 0xFFu) * scale) * sc;
    y.y = (lo + (float)((w >> 8) & 0xFFu) * scale) * sc;
    y.z = (lo + (float)((w >> 16) & 0xFFu) * scale) * sc;
    y.w = (lo + (float)(w >> 24) * scale) * sc;
    return y;
}

// st16: the output rows are 16-byte aligned, so a code lane's 16 values leave as 16-byte stores; otherwise (16-bit rows of D % 8 == 4
// columns) as 8-byte ones.  The last chunk of a row holds 4, 8, 12 or 16 columns: `valid`.
template <class K, class OT>
__global__ __launch_bounds__(256) void k_q8_gather(const uint8_t* __restrict__ rec, int64_t V, int64_t row_bytes, int D,
                                                   const K* __restrict__ ids, int64_t n, const float* __restrict__ row_scale,
                                                   OT* __restrict__ out, int64_t ldo, float* __restrict__ wprod, int64_t ldw,
                                                   RowGeom gm, bool st16) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / gm.lpr, sub = lane - grp * gm.lpr;
    if (grp >= gm.G) return;
    const int lane0 = lane - sub;
    const int col0 = (sub - 1) * 16;                                    // (the header lane: -16, never used as a column)
    const int valid = sub == 0 ? 0 : (D - col0 < 16 ? D - col0 : 16);
    const int64_t wave_row0 = ((int64_t)blockIdx.x * 4 + wave) * (gm.G * kQ8GB);
    const int64_t nlast = n - 1;
    int64_t row[kQ8GB];
    float sc[kQ8GB];
    uint4 x[kQ8GB];
    // as k_gather_rows: every load is requested unconditionally (a position past the end reads the last id, an id out of range
    // record 0; both are dropped) so that the GB records are in flight together
#pragma unroll
    for (int k = 0; k < kQ8GB; ++k) {
        const int64_t i = wave_row0 + (int64_t)k * gm.G + grp;
        const int64_t ic = i < n ? i : nlast;
        row[k] = (int64_t)ids[ic];
        sc[k] = row_scale ? row_scale[ic] : 1.0f;
    }
#pragma unroll
    for (int k = 0; k < kQ8GB; ++k) {
        const bool ok = row[k] >= 0 && row[k] < V;
        x[k] = *(const uint4*)(rec + (ok ? row[k] : 0) * row_bytes + 16 * sub);
        if (!ok) row[k] = -1;
    }
#pragma unroll
    for (int k = 0; k < kQ8GB; ++k) {
        asm volatile("" : "+v"(x[k].x), "+v"(x[k].y), "+v"(x[k].z), "+v"(x[k].w));
        if (row[k] < 0) x[k] = make_uint4(0u, 0u, 0u, 0u);              // header and codes zero: a zero row, a zero product
    }
#pragma unroll
    for (int k = 0; k < kQ8GB; ++k) {
        const int64_t i = wave_row0 + (int64_t)k * gm.G + grp;
        const float lo = bperm_f(lane0, __uint_as_float(x[k].x));
        const float scale = bperm_f(lane0, __uint_as_float(x[k].y));
        if (i >= n) continue;
        if (sub == 0) {
            if (wprod) *(uint2*)(wprod + ldw * i) = make_uint2(__float_as_uint(__uint_as_float(x[k].z) * sc[k]), 0u);
            continue;
        }
        const float4 y0 = q8_dequant4(x[k].x, lo, scale, sc[k]), y1 = q8_dequant4(x[k].y, lo, scale, sc[k]);
        const float4 y2 = q8_dequant4(x[k].z, lo, scale, sc[k]), y3 = q8_dequant4(x[k].w, lo, scale, sc[k]);
        OT* const o = out + i * ldo + col0;
        if constexpr (sizeof(OT) == 4) {
            *(float4*)o = y0;
            if (valid > 4) *(float4*)(o + 4) = y1;
            if (valid > 8) *(float4*)(o + 8) = y2;
            if (valid > 12) *(float4*)(o + 12) = y3;
        } else {
            const uint2 h0 = q8_pack16((const OT*)nullptr, y0.x, y0.y, y0.z, y0.w), h1 = q8_pack16((const OT*)nullptr, y1.x, y1.y, y1.z, y1.w);
            const uint2 h2 = q8_pack16((const OT*)nullptr, y2.x, y2.y, y2.z, y2.w), h3 = q8_pack16((const OT*)nullptr, y3.x, y3.y, y3.z, y3.w);
            if (st16) {
                if (valid > 4) *(uint4*)o = make_uint4(h0.x, h0.y, h1.x, h1.y);
                else *(uint2*)o = h0;
                if (valid > 12) *(uint4*)(o + 8) = make_uint4(h2.x, h2.y, h3.x, h3.y);
                else if (valid > 8) *(uint2*)(o + 8) = h2;
            } else {
                *(uint2*)o = h0;
                if (valid > 4) *(uint2*)(o + 4) = h1;
                if (valid > 8) *(uint2*)(o + 8) = h2;
                if (valid > 12) *(uint2*)(o + 12) = h3;
            }
        }
    }
}

// A code lane's 16 masked values of one field: written once in the output kind (k_q8_gather's store rule: st16, valid) and added into
// the lane's column sums.  s and q take the fp32 values, whatever the output kind rounds them to.
template <class OT>
__device__ __forceinline__ void q8_fm_put(OT* __restrict__ o, const float4 (&y)[4], int valid, bool st16, bool store, float4 (&s)[4],
                                          float4 (&q)[4]) {
    if (store) {
        if constexpr (sizeof(OT) == 4) {
            *(float4*)o = y[0];
            if (valid > 4) *(float4*)(o + 4) = y[1];
            if (valid > 8) *(float4*)(o + 8) = y[2];
            if (valid > 12) *(float4*)(o + 12) = y[3];
        } else {
            uint2 h[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) h[j] = q8_pack16((const OT*)nullptr, y[j].x, y[j].y, y[j].z, y[j].w);
            if (st16) {
                if (valid > 4) *(uint4*)o = make_uint4(h[0].x, h[0].y, h[1].x, h[1].y);
                else *(uint2*)o = h[0];
                if (valid > 12) *(uint4*)(o + 8) = make_uint4(h[2].x, h[2].y, h[3].x, h[3].y);
                else if (valid > 8) *(uint2*)(o + 8) = h[2];
            } else {
                *(uint2*)o = h[0];
                if (valid > 4) *(uint2*)(o + 4) = h[1];
                if (valid > 8) *(uint2*)(o + 8) = h[2];
                if (valid > 12) *(uint2*)(o + 12) = h[3];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        s[j].x = s[j].x + y[j].x; s[j].y = s[j].y + y[j].y; s[j].z = s[j].z + y[j].z; s[j].w = s[j].w + y[j].w;
        q[j].x = q[j].x + y[j].x * y[j].x; q[j].y = q[j].y + y[j].y * y[j].y; q[j].z = q[j].z + y[j].z * y[j].z;
        q[j].w = q[j].w + y[j].w * y[j].w;
    }
}

// rows [B, F, D] contiguous.  A lane-group whose sample lies past B (the last wave's) reads sample 0's entries and stores nothing: every
// lane of a live group-slot stays in the loop, so the ds_bpermute reads below always find their source lane active.
template <class K, class OT>
__global__ __launch_bounds__(256) void k_q8_fm_lookup(const uint8_t* __restrict__ rec, int64_t V, int64_t row_bytes, int D,
                                                      const K* __restrict__ ids, const float* __restrict__ wts, int64_t B, int F,
                                                      OT* __restrict__ rows, float* __restrict__ lin_fm, RowGeom gm, bool st16) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / gm.lpr, sub = lane - grp * gm.lpr;
    if (grp >= gm.G) return;
    const int lane0 = lane - sub;
    const int col0 = (sub - 1) * 16;                                    // (the header lane: -16, never used as a column)
    const int valid = sub == 0 ? 0 : (D - col0 < 16 ? D - col0 : 16);
    const int64_t ng = (int64_t)gridDim.x * 4 * gm.G;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t b0 = ((int64_t)blockIdx.x * 4 + wave) * gm.G; b0 < B; b0 += ng) {
        const int64_t b = b0 + grp;
        const bool live = b < B;
        const int64_t e0 = (live ? b : 0) * (int64_t)F;
        float4 s[4] = {zero4, zero4, zero4, zero4}, q[4] = {zero4, zero4, zero4, zero4};
        float lin = 0.0f;
        // kQ8FmNB fields, nf of them real: a spare slot reads the batch's last field again and is dropped, so s, q and the linear sum see
        // the F fields alone, in field order (k_fm_lookup::fields4's rule)
        const auto fields = [&](const int f, const int nf) {
            int64_t r[kQ8FmNB];
            float t[kQ8FmNB];
            uint4 x[kQ8FmNB];
#pragma unroll
            for (int k = 0; k < kQ8FmNB; ++k) {
                const int64_t e = e0 + f + (k < nf ? k : nf - 1);
                r[k] = (int64_t)ids[e];
                t[k] = wts[e];
            }
#pragma unroll
            for (int k = 0; k < kQ8FmNB; ++k) {
                const bool ok = r[k] >= 0 && r[k] < V;
                x[k] = *(const uint4*)(rec + (ok ? r[k] : 0) * row_bytes + 16 * sub);
                if (!ok) r[k] = -1;
            }
#pragma unroll
            for (int k = 0; k < kQ8FmNB; ++k) {
                asm volatile("" : "+v"(x[k].x), "+v"(x[k].y), "+v"(x[k].z), "+v"(x[k].w));
                if (r[k] < 0) x[k] = make_uint4(0u, 0u, 0u, 0u);        // header and codes zero: a zero row, a zero linear weight
            }
#pragma unroll
            for (int k = 0; k < kQ8FmNB; ++k) {
                const float lo = bperm_f(lane0, __uint_as_float(x[k].x));
                const float scale = bperm_f(lane0, __uint_as_float(x[k].y));
                if (k >= nf) continue;
                if (sub == 0) {
                    lin = lin + __uint_as_float(x[k].z) * t[k];
                    continue;
                }
                const float4 y[4] = {q8_dequant4(x[k].x, lo, scale, t[k]), q8_dequant4(x[k].y, lo, scale, t[k]),
                                     q8_dequant4(x[k].z, lo, scale, t[k]), q8_dequant4(x[k].w, lo, scale, t[k])};
                q8_fm_put(rows + ((b * F + f + k) * (int64_t)D + col0), y, valid, st16, live, s, q);
            }
        };
        int f = 0;
        for (; f + kQ8FmNB <= F; f += kQ8FmNB) fields(f, kQ8FmNB);
        if (f < F) fields(f, F - f);
        float part = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (valid > 4 * j)
                part += ((s[j].x * s[j].x - q[j].x) + (s[j].y * s[j].y - q[j].y)) + ((s[j].z * s[j].z - q[j].z) + (s[j].w * s[j].w - q[j].w));
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) {
            const float o = __shfl_down(part, off, 64);
            if (sub + off < gm.lpr) part += o;
        }
        if (live && sub == 0) lin_fm[b] = lin + 0.5f * part;
    }
}

// ===== the pooled (multi-hot) lookup over records ======================================================================================
constexpr int kQ8PoolNB = 4;     // slots in flight per lane-group of the pooled lookup

struct Q8PoolFields { unsigned w[MREC_POOL_MAX_FIELDS]; };      // w[f] = off_f | L_f << 16 (off_f < 4096, off_f + L_f <= 4096)

// a code lane's 16 pooled values of one field, rounded once to the output kind: k_q8_gather's store rule (st16, valid)
template <class OT>
__device__ __forceinline__ void q8_pool_put(OT* __restrict__ o, const float4 (&y)[4], int valid, bool st16) {
    if constexpr (sizeof(OT) == 4) {
        *(float4*)o = y[0];
        if (valid > 4) *(float4*)(o + 4) = y[1];
        if (valid > 8) *(float4*)(o + 8) = y[2];
        if (valid > 12) *(float4*)(o + 12) = y[3];
    } else {
        uint2 h[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) h[j] = q8_pack16((const OT*)nullptr, y[j].x, y[j].y, y[j].z, y[j].w);
        if (st16) {
            if (valid > 4) *(uint4*)o = make_uint4(h[0].x, h[0].y, h[1].x, h[1].y);
            else *(uint2*)o = h[0];
            if (valid > 12) *(uint4*)(o + 8) = make_uint4(h[2].x, h[2].y, h[3].x, h[3].y);
            else if (valid > 8) *(uint2*)(o + 8) = h[2];
        } else {
            *(uint2*)o = h[0];
            if (valid > 4) *(uint2*)(o + 4) = h[1];
            if (valid > 8) *(uint2*)(o + 8) = h[2];
            if (valid > 12) *(uint2*)(o + 12) = h[3];
        }
    }
}

// the four codes of one dword into four column sums: acc = fma((float)code, t, acc), one byte conversion and one fma a code
__device__ __forceinline__ void q8_pool_fma4(unsigned w, float t, float4& a) {
    a.x = __builtin_fmaf((float)(w & 0xFFu), t, a.x);
    a.y = __builtin_fmaf((float)((w >> 8) & 0xFFu), t, a.y);
    a.z = __builtin_fmaf((float)((w >> 16) & 0xFFu), t, a.z);
    a.w = __builtin_fmaf((float)(w >> 24), t, a.w);
}

// ids, mask [B, Ls] contiguous.  Everything that names a slot or a field (s, f, fend, the branches on them) is the same for every lane of
// the wave: scalar registers and uniform branches, inside which every lane of a live group-slot runs, so the ds_bpermute reads always
// find their source lane active.  A lane-group whose sample lies past B (the last wave's) reads sample 0's entries and stores nothing.
// Every lane forms t, u and g from the first three words of its own chunk and adds u and g into its own base and wsum: only the header
// lane's are the header's, and only the header lane's base and wsum are ever read (as are only the code lanes' acc).
template <class K, class OT>
__global__ __launch_bounds__(256) void k_q8_gather_pool_fields(const uint8_t* __restrict__ rec, int64_t V, int64_t row_bytes, int D,
                                                               const K* __restrict__ ids, const float* __restrict__ mask, int64_t B, int F,
                                                               int Ls, int mode, OT* __restrict__ out, int64_t ldo,
                                                               float* __restrict__ wide_out, int64_t ldw, RowGeom gm, bool st16,
                                                               const Q8PoolFields pf) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int grp = lane / gm.lpr, sub = lane - grp * gm.lpr;
    if (grp >= gm.G) return;
    const int lane0 = lane - sub;
    const int col0 = (sub - 1) * 16;                                    // (the header lane: -16, never used as a column)
    const int valid = sub == 0 ? 0 : (D - col0 < 16 ? D - col0 : 16);
    const int64_t ng = (int64_t)gridDim.x * 4 * gm.G;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const int slast = Ls - 1;
    for (int64_t b0 = ((int64_t)blockIdx.x * 4 + wave) * gm.G; b0 < B; b0 += ng) {
        const int64_t b = b0 + grp;
        const bool live = b < B;
        const int64_t e0 = (live ? b : 0) * (int64_t)Ls;
        float4 acc[4] = {zero4, zero4, zero4, zero4};
        float base = 0.0f, wsum = 0.0f, wtot = 0.0f;
        int f = 0;
        unsigned fw = pf.w[0];
        int fend = (int)(fw >> 16);                                     // one past the open field's last slot (field 0 starts at slot 0)
        for (int s0 = 0; s0 < Ls; s0 += kQ8PoolNB) {
            int64_t r[kQ8PoolNB];
            float m[kQ8PoolNB];
            uint4 x[kQ8PoolNB];
#pragma unroll
            for (int k = 0; k < kQ8PoolNB; ++k) {
                const int64_t e = e0 + (s0 + k < slast ? s0 + k : slast);
                r[k] = (int64_t)ids[e];
                m[k] = mask ? mask[e] : 1.0f;
            }
#pragma unroll
            for (int k = 0; k < kQ8PoolNB; ++k) {
                const bool ok = r[k] >= 0 && r[k] < V;
                x[k] = *(const uint4*)(rec + (ok ? r[k] : 0) * row_bytes + 16 * sub);
                if (!ok) r[k] = -1;
            }
#pragma unroll
            for (int k = 0; k < kQ8PoolNB; ++k) {
                asm volatile("" : "+v"(x[k].x), "+v"(x[k].y), "+v"(x[k].z), "+v"(x[k].w));
                if (r[k] < 0) x[k] = make_uint4(0u, 0u, 0u, 0u);        // header and codes zero: a +0 row, a +0 wide product
            }
#pragma unroll
            for (int k = 0; k < kQ8PoolNB; ++k) {
                const int s = s0 + k;
                if (s > slast) continue;                                // a spare slot of the sample's last batch: dropped
                const float t = bperm_f(lane0, m[k] * __uint_as_float(x[k].y));
                base = base + m[k] * __uint_as_float(x[k].x);
                wsum = wsum + m[k] * __uint_as_float(x[k].z);
                q8_pool_fma4(x[k].x, t, acc[0]);
                q8_pool_fma4(x[k].y, t, acc[1]);
                q8_pool_fma4(x[k].z, t, acc[2]);
                q8_pool_fma4(x[k].w, t, acc[3]);
                if (s + 1 != fend) continue;
                // the field's last slot: y = acc + base, the mean's division by the field's own length, one rounding, one store
                const float bs = bperm_f(lane0, base);
                float4 y[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) y[j] = make_float4(acc[j].x + bs, acc[j].y + bs, acc[j].z + bs, acc[j].w + bs);
                if (mode == 1) {
                    const float fl = (float)(fw >> 16);
#pragma unroll
                    for (int j = 0; j < 4; ++j) y[j] = make_float4(y[j].x / fl, y[j].y / fl, y[j].z / fl, y[j].w / fl);
                }
                if (live && sub != 0) q8_pool_put(out + (b * ldo + (int64_t)f * D + col0), y, valid, st16);
                wtot = wtot + wsum;
                acc[0] = acc[1] = acc[2] = acc[3] = zero4;
                base = wsum = 0.0f;
                f = f + 1 < F ? f + 1 : f;                              // (behind the last field: its own word again, never closed twice)
                fw = pf.w[f];
                fend = (int)(fw & 0xFFFFu) + (int)(fw >> 16);
            }
        }
        if (live && sub == 0 && wide_out) wide_out[b * ldw] = wtot;
    }
}

// ===== row-wise 4-bit records: [lo scale wide 0 | D / 2 code bytes | zero padding] =====================================================
constexpr int kQ4GB = 4;         // positions in flight per lane-group of the 4-bit lookup

__device__ __forceinline__ float q4_code(float x, float lo, float scale) {
    const float q = fminf(rintf((x - lo) / scale), 15.0f);
    return scale > 0.0f ? q : 0.0f;
}

// four codes -> the 16 bits that hold them, column d in bits 4 d
__device__ __forceinline__ unsigned q4_codes4(const float4& x, float lo, float scale) {
    return (unsigned)q4_code(x.x, lo, scale) | ((unsigned)q4_code(x.y, lo, scale) << 4) | ((unsigned)q4_code(x.z, lo, scale) << 8) |
           ((unsigned)q4_code(x.w, lo, scale) << 12);
}

// gm.lpr = ceil(D / 8) lanes a row.  The row's last lane holds four columns where D % 8 == 4: it reads its first 16 bytes twice (never
// past the row: a contiguous table's last row ends there), which min and max do not notice, and the upper half of its dword is zero.
__global__ __launch_bounds__(256) void k_q4_quantize(const float* __restrict__ table, int64_t V, int64_t ld, int D,
                                                     const float* __restrict__ wide, int64_t ldw, uint8_t* __restrict__ rec,
                                                     int64_t row_bytes, RowGeom gm) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / gm.lpr, ds = lane - grp * gm.lpr;
    if (grp >= gm.G) return;
    const int nd = gm.lpr, lane0 = lane - ds;
    const bool two = 8 * ds + 4 < D;
    const int pad_dw = (int)((row_bytes - kQ8Hdr) >> 2) - nd;           // zero dwords behind the code dwords
    const int64_t stride = (int64_t)gridDim.x * 4 * gm.G;
    for (int64_t r = ((int64_t)blockIdx.x * 4 + wave) * gm.G + grp; r < V; r += stride) {
        const float* const src = table + r * ld + 8 * ds;
        const float4 a = *(const float4*)src;
        const float4 b = *(const float4*)(src + (two ? 4 : 0));
        float w = 0.0f;
        if (ds == 0 && wide) w = wide[r * ldw];
        float lo = fminf(fminf(fminf(a.x, a.y), fminf(a.z, a.w)), fminf(fminf(b.x, b.y), fminf(b.z, b.w)));
        float hi = fmaxf(fmaxf(fmaxf(a.x, a.y), fmaxf(a.z, a.w)), fmaxf(fmaxf(b.x, b.y), fmaxf(b.z, b.w)));
        for (int m = 1; m < nd; m <<= 1) {
            const int p = ds ^ m;
            const int src_lane = lane0 + (p < nd ? p : nd - 1);
            lo = fminf(lo, bperm_f(src_lane, lo));
            hi = fmaxf(hi, bperm_f(src_lane, hi));
        }
        const float scale = (hi - lo) / 15.0f;
        const unsigned upper = q4_codes4(b, lo, scale) << 16;
        const unsigned codes = q4_codes4(a, lo, scale) | (two ? upper : 0u);
        uint8_t* const o = rec + r * row_bytes;
        if (ds == 0) *(uint4*)o = make_uint4(__float_as_uint(lo), __float_as_uint(scale), __float_as_uint(w), 0u);
        *(uint32_t*)(o + kQ8Hdr + 4 * ds) = codes;
        for (int j = ds; j < pad_dw; j += nd) *(uint32_t*)(o + kQ8Hdr + 4 * (nd + j)) = 0u;
    }
}

// the eight codes of one dword -> x' * sc, in column order.  The even columns are the bytes of w & 0x0F0F0F0F, the odd ones the bytes
// of (w >> 4) & 0x0F0F0F0F: two integer instructions a dword, then v_cvt_f32_ubyte0..3 on either word.
__device__ __forceinline__ void q4_dequant8(unsigned w, float lo, float scale, float sc, float4& y0, float4& y1) {
    unsigned e = w & 0x0F0F0F0Fu, o = (w >> 4) & 0x0F0F0F0Fu;
    asm volatile("" : "+v"(e), "+v"(o));            // (keeps the two words: the compiler otherwise extracts a bit field per code)
    y0.x = (lo + (float)(e & 0xFFu) * scale) * sc;
    y0.y = (lo + (float)(o & 0xFFu) * scale) * sc;
    y0.z = (lo + (float)((e >> 8) & 0xFFu) * scale) * sc;
    y0.w = (lo + (float)((o >> 8) & 0xFFu) * scale) * sc;
    y1.x = (lo + (float)((e >> 16) & 0xFFu) * scale) * sc;
    y1.y = (lo + (float)((o >> 16) & 0xFFu) * scale) * sc;
    y1.z = (lo + (float)(e >> 24) * scale) * sc;
    y1.w = (lo + (float)(o >> 24) * scale) * sc;
}

// gm.lpr = ceil(D / 32) + 1 lanes a position: lane 0 the header chunk, lane c the c-th 32 codes (columns 32 (c - 1) ..).  The store rule
// is k_q8_gather's -- st16: 16-byte stores, else (16-bit rows of D % 8 == 4 columns) 8-byte ones -- over a last chunk of `valid` = 4, 8,
// .., 32 columns: code dword j of the chunk is columns 8 j .. 8 j + 7, one 16-byte store of 16-bit values or two of fp32 ones.
template <class K, class OT>
__global__ __launch_bounds__(256) void k_q4_gather(const uint8_t* __restrict__ rec, int64_t V, int64_t row_bytes, int D,
                                                   const K* __restrict__ ids, int64_t n, const float* __restrict__ row_scale,
                                                   OT* __restrict__ out, int64_t ldo, float* __restrict__ wprod, int64_t ldw,
                                                   RowGeom gm, bool st16) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / gm.lpr, sub = lane - grp * gm.lpr;
    if (grp >= gm.G) return;
    const int lane0 = lane - sub;
    const int col0 = (sub - 1) * 32;                                    // (the header lane: -32, never used as a column)
    const int valid = sub == 0 ? 0 : (D - col0 < 32 ? D - col0 : 32);
    const int64_t wave_row0 = ((int64_t)blockIdx.x * 4 + wave) * (gm.G * kQ4GB);
    const int64_t nlast = n - 1;
    int64_t row[kQ4GB];
    float sc[kQ4GB];
    uint4 x[kQ4GB];
    // k_q8_gather's rule: every load is requested unconditionally (a position past the end reads the last id, an id out of range
    // record 0; both are dropped) so that the GB records are in flight together
#pragma unroll
    for (int k = 0; k < kQ4GB; ++k) {
        const int64_t i = wave_row0 + (int64_t)k * gm.G + grp;
        const int64_t ic = i < n ? i : nlast;
        row[k] = (int64_t)ids[ic];
        sc[k] = row_scale ? row_scale[ic] : 1.0f;
    }
#pragma unroll
    for (int k = 0; k < kQ4GB; ++k) {
        const bool ok = row[k] >= 0 && row[k] < V;
        x[k] = *(const uint4*)(rec + (ok ? row[k] : 0) * row_bytes + 16 * sub);
        if (!ok) row[k] = -1;
    }
#pragma unroll
    for (int k = 0; k < kQ4GB; ++k) {
        asm volatile("" : "+v"(x[k].x), "+v"(x[k].y), "+v"(x[k].z), "+v"(x[k].w));
        if (row[k] < 0) x[k] = make_uint4(0u, 0u, 0u, 0u);              // header and codes zero: a zero row, a zero product
    }
#pragma unroll
    for (int k = 0; k < kQ4GB; ++k) {
        const int64_t i = wave_row0 + (int64_t)k * gm.G + grp;
        const float lo = bperm_f(lane0, __uint_as_float(x[k].x));
        const float scale = bperm_f(lane0, __uint_as_float(x[k].y));
        if (i >= n) continue;
        if (sub == 0) {
            if (wprod) *(uint2*)(wprod + ldw * i) = make_uint2(__float_as_uint(__uint_as_float(x[k].z) * sc[k]), 0u);
            continue;
        }
        const unsigned w[4] = {x[k].x, x[k].y, x[k].z, x[k].w};
        OT* const o = out + i * ldo + col0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float4 y0, y1;
            q4_dequant8(w[j], lo, scale, sc[k], y0, y1);
            if constexpr (sizeof(OT) == 4) {
                if (valid > 8 * j) *(float4*)(o + 8 * j) = y0;
                if (valid > 8 * j + 4) *(float4*)(o + 8 * j + 4) = y1;
            } else {
                const uint2 h0 = q8_pack16((const OT*)nullptr, y0.x, y0.y, y0.z, y0.w);
                const uint2 h1 = q8_pack16((const OT*)nullptr, y1.x, y1.y, y1.z, y1.w);
                if (st16 && valid > 8 * j + 4) {
                    *(uint4*)(o + 8 * j) = make_uint4(h0.x, h0.y, h1.x, h1.y);
                } else {
                    if (valid > 8 * j) *(uint2*)(o + 8 * j) = h0;
                    if (valid > 8 * j + 4) *(uint2*)(o + 8 * j + 4) = h1;
                }
            }
        }
    }
}

// ===== the FM lookup over 4-bit records ================================================================================================
constexpr int kQ4FmNB = 4;       // fields in flight per lane-group of the 4-bit FM lookup (the header comment has the register count)

// The eight masked values of one code dword of one field: written once in the output kind (k_q4_gather's store rule: st16, `left` = the
// chunk's valid columns from this dword on) and added into the lane's column sums.  s and q take the fp32 values, whatever the output
// kind rounds them to; columns past the row's end add into sums that the column sum never reads.
template <class OT>
__device__ __forceinline__ void q4_fm_put8(OT* __restrict__ o, const float4& y0, const float4& y1, int left, bool st16, bool store,
                                           float4& s0, float4& s1, float4& q0, float4& q1) {
    s0.x = s0.x + y0.x; s0.y = s0.y + y0.y; s0.z = s0.z + y0.z; s0.w = s0.w + y0.w;
    s1.x = s1.x + y1.x; s1.y = s1.y + y1.y; s1.z = s1.z + y1.z; s1.w = s1.w + y1.w;
    q0.x = q0.x + y0.x * y0.x; q0.y = q0.y + y0.y * y0.y; q0.z = q0.z + y0.z * y0.z; q0.w = q0.w + y0.w * y0.w;
    q1.x = q1.x + y1.x * y1.x; q1.y = q1.y + y1.y * y1.y; q1.z = q1.z + y1.z * y1.z; q1.w = q1.w + y1.w * y1.w;
    // (the sums are taken HERE: the compiler otherwise sinks all 64 adds of a field behind the last store branch of the batch and keeps
    // every field's 32 values alive until then -- 242 VGPRs instead of 137)
    asm volatile("" : "+v"(s0.x), "+v"(s0.y), "+v"(s0.z), "+v"(s0.w), "+v"(s1.x), "+v"(s1.y), "+v"(s1.z), "+v"(s1.w), "+v"(q0.x), "+v"(q0.y),
                 "+v"(q0.z), "+v"(q0.w), "+v"(q1.x), "+v"(q1.y), "+v"(q1.z), "+v"(q1.w));
    if (!store) return;
    if constexpr (sizeof(OT) == 4) {
        if (left > 0) *(float4*)o = y0;
        if (left > 4) *(float4*)(o + 4) = y1;
    } else {
        const uint2 h0 = q8_pack16((const OT*)nullptr, y0.x, y0.y, y0.z, y0.w);
        const uint2 h1 = q8_pack16((const OT*)nullptr, y1.x, y1.y, y1.z, y1.w);
        if (st16 && left > 4) {
            *(uint4*)o = make_uint4(h0.x, h0.y, h1.x, h1.y);
        } else {
            if (left > 0) *(uint2*)o = h0;
            if (left > 4) *(uint2*)(o + 4) = h1;
        }
    }
}

// rows [B, F, D] contiguous.  gm.lpr = ceil(D / 32) + 1 lanes a SAMPLE: lane 0 the header chunk of each of the sample's records, lane c
// the c-th 32 codes.  A lane-group whose sample lies past B (the last wave's) reads sample 0's entries and stores nothing: every lane of a
// live group-slot stays in the loop, so the ds_bpermute reads below always find their source lane active.
template <class K, class OT>
__global__ __launch_bounds__(256) void k_q4_fm_lookup(const uint8_t* __restrict__ rec, int64_t V, int64_t row_bytes, int D,
                                                      const K* __restrict__ ids, const float* __restrict__ wts, int64_t B, int F,
                                                      OT* __restrict__ rows, float* __restrict__ lin_fm, RowGeom gm, bool st16) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / gm.lpr, sub = lane - grp * gm.lpr;
    if (grp >= gm.G) return;
    const int lane0 = lane - sub;
    const int col0 = (sub - 1) * 32;                                    // (the header lane: -32, never used as a column)
    const int valid = sub == 0 ? 0 : (D - col0 < 32 ? D - col0 : 32);
    const int64_t ng = (int64_t)gridDim.x * 4 * gm.G;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t b0 = ((int64_t)blockIdx.x * 4 + wave) * gm.G; b0 < B; b0 += ng) {
        const int64_t b = b0 + grp;
        const bool live = b < B;
        const int64_t e0 = (live ? b : 0) * (int64_t)F;
        float4 s[8] = {zero4, zero4, zero4, zero4, zero4, zero4, zero4, zero4};
        float4 q[8] = {zero4, zero4, zero4, zero4, zero4, zero4, zero4, zero4};
        float lin = 0.0f;
        // kQ4FmNB fields, nf of them real: a spare slot reads the batch's last field again and is dropped, so s, q and the linear sum see
        // the F fields alone, in field order (k_q8_fm_lookup's rule)
        const auto fields = [&](const int f, const int nf) {
            int64_t r[kQ4FmNB];
            float t[kQ4FmNB];
            uint4 x[kQ4FmNB];
#pragma unroll
            for (int k = 0; k < kQ4FmNB; ++k) {
                const int64_t e = e0 + f + (k < nf ? k : nf - 1);
                r[k] = (int64_t)ids[e];
                t[k] = wts[e];
            }
#pragma unroll
            for (int k = 0; k < kQ4FmNB; ++k) {
                const bool ok = r[k] >= 0 && r[k] < V;
                x[k] = *(const uint4*)(rec + (ok ? r[k] : 0) * row_bytes + 16 * sub);
                if (!ok) r[k] = -1;
            }
#pragma unroll
            for (int k = 0; k < kQ4FmNB; ++k) {
                asm volatile("" : "+v"(x[k].x), "+v"(x[k].y), "+v"(x[k].z), "+v"(x[k].w));
                if (r[k] < 0) x[k] = make_uint4(0u, 0u, 0u, 0u);        // header and codes zero: a zero row, a zero linear weight
            }
#pragma unroll
            for (int k = 0; k < kQ4FmNB; ++k) {
                const float lo = bperm_f(lane0, __uint_as_float(x[k].x));
                const float scale = bperm_f(lane0, __uint_as_float(x[k].y));
                if (k >= nf) continue;
                // no branch on the lane's role: every lane adds its chunk's third word into lin and its 32 "codes" into s and q -- only
                // the header lane's lin and the code lanes' sums are ever read (valid == 0 keeps the header lane from storing)
                lin = lin + __uint_as_float(x[k].z) * t[k];
                const unsigned w[4] = {x[k].x, x[k].y, x[k].z, x[k].w};
                OT* const o = rows + ((b * F + f + k) * (int64_t)D + col0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float4 y0, y1;
                    q4_dequant8(w[j], lo, scale, t[k], y0, y1);
                    q4_fm_put8(o + 8 * j, y0, y1, valid - 8 * j, st16, live, s[2 * j], s[2 * j + 1], q[2 * j], q[2 * j + 1]);
                }
            }
        };
        int f = 0;
        for (; f + kQ4FmNB <= F; f += kQ4FmNB) fields(f, kQ4FmNB);
        if (f < F) fields(f, F - f);
        float part = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (valid > 4 * j)
                part += ((s[j].x * s[j].x - q[j].x) + (s[j].y * s[j].y - q[j].y)) + ((s[j].z * s[j].z - q[j].z) + (s[j].w * s[j].w - q[j].w));
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) {
            const float o = __shfl_down(part, off, 64);
            if (sub + off < gm.lpr) part += o;
        }
        if (live && sub == 0) lin_fm[b] = lin + 0.5f * part;
    }
}

// ===== the pooled (multi-hot) lookup over 4-bit records ================================================================================
constexpr int kQ4PoolNB = 4;     // slots in flight per lane-group of the 4-bit pooled lookup

// the eight codes of one dword into eight column sums, acc = fma((float)code, t, acc): q4_dequant8's two-word nibble split (two integer
// instructions a dword), then one byte conversion and one fma a code
__device__ __forceinline__ void q4_pool_fma8(unsigned w, float t, float4& a0, float4& a1) {
    unsigned e = w & 0x0F0F0F0Fu, o = (w >> 4) & 0x0F0F0F0Fu;
    asm volatile("" : "+v"(e), "+v"(o));            // (keeps the two words: the compiler otherwise extracts a bit field per code)
    a0.x = __builtin_fmaf((float)(e & 0xFFu), t, a0.x);
    a0.y = __builtin_fmaf((float)(o & 0xFFu), t, a0.y);
    a0.z = __builtin_fmaf((float)((e >> 8) & 0xFFu), t, a0.z);
    a0.w = __builtin_fmaf((float)((o >> 8) & 0xFFu), t, a0.w);
    a1.x = __builtin_fmaf((float)((e >> 16) & 0xFFu), t, a1.x);
    a1.y = __builtin_fmaf((float)((o >> 16) & 0xFFu), t, a1.y);
    a1.z = __builtin_fmaf((float)(e >> 24), t, a1.z);
    a1.w = __builtin_fmaf((float)(o >> 24), t, a1.w);
}

// eight pooled values (one code dword's columns), rounded once to the output kind: k_q4_gather's store rule (st16, `left` = the chunk's
// valid columns from this dword on)
template <class OT>
__device__ __forceinline__ void q4_pool_put8(OT* __restrict__ o, const float4& y0, const float4& y1, int left, bool st16) {
    if constexpr (sizeof(OT) == 4) {
        if (left > 0) *(float4*)o = y0;
        if (left > 4) *(float4*)(o + 4) = y1;
    } else {
        const uint2 h0 = q8_pack16((const OT*)nullptr, y0.x, y0.y, y0.z, y0.w);
        const uint2 h1 = q8_pack16((const OT*)nullptr, y1.x, y1.y, y1.z, y1.w);
        if (st16 && left > 4) {
            *(uint4*)o = make_uint4(h0.x, h0.y, h1.x, h1.y);
        } else {
            if (left > 0) *(uint2*)o = h0;
            if (left > 4) *(uint2*)(o + 4) = h1;
        }
    }
}

// ids, mask [B, Ls] contiguous.  k_q8_gather_pool_fields over the 4-bit record: gm.lpr = ceil(D / 32) + 1 lanes a sample, a code lane
// holds acc[32].  Slot numbers, field ends and the closing of a field are the same for every lane of the wave (scalar registers, uniform
// branches), inside which every lane of a live group-slot runs, so the ds_bpermute reads always find their source lane active.  A
// lane-group whose sample lies past B reads sample 0's entries and stores nothing.  Every lane forms t, u and g from the first three
// words of its own chunk; only the header lane's t, base and wsum are ever read (as are only the code lanes' acc).
template <class K, class OT>
__global__ __launch_bounds__(256) void k_q4_gather_pool_fields(const uint8_t* __restrict__ rec, int64_t V, int64_t row_bytes, int D,
                                                               const K* __restrict__ ids, const float* __restrict__ mask, int64_t B, int F,
                                                               int Ls, int mode, OT* __restrict__ out, int64_t ldo,
                                                               float* __restrict__ wide_out, int64_t ldw, RowGeom gm, bool st16,
                                                               const Q8PoolFields pf) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int grp = lane / gm.lpr, sub = lane - grp * gm.lpr;
    if (grp >= gm.G) return;
    const int lane0 = lane - sub;
    const int col0 = (sub - 1) * 32;                                    // (the header lane: -32, never used as a column)
    const int valid = sub == 0 ? 0 : (D - col0 < 32 ? D - col0 : 32);
    const int64_t ng = (int64_t)gridDim.x * 4 * gm.G;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const int slast = Ls - 1;
    for (int64_t b0 = ((int64_t)blockIdx.x * 4 + wave) * gm.G; b0 < B; b0 += ng) {
        const int64_t b = b0 + grp;
        const bool live = b < B;
        const int64_t e0 = (live ? b : 0) * (int64_t)Ls;
        float4 acc[8] = {zero4, zero4, zero4, zero4, zero4, zero4, zero4, zero4};
        float base = 0.0f, wsum = 0.0f, wtot = 0.0f;
        int f = 0;
        unsigned fw = pf.w[0];
        int fend = (int)(fw >> 16);                                     // one past the open field's last slot (field 0 starts at slot 0)
        for (int s0 = 0; s0 < Ls; s0 += kQ4PoolNB) {
            int64_t r[kQ4PoolNB];
            float m[kQ4PoolNB];
            uint4 x[kQ4PoolNB];
#pragma unroll
            for (int k = 0; k < kQ4PoolNB; ++k) {
                const int64_t e = e0 + (s0 + k < slast ? s0 + k : slast);
                r[k] = (int64_t)ids[e];
                m[k] = mask ? mask[e] : 1.0f;
            }
#pragma unroll
            for (int k = 0; k < kQ4PoolNB; ++k) {
                const bool ok = r[k] >= 0 && r[k] < V;
                x[k] = *(const uint4*)(rec + (ok ? r[k] : 0) * row_bytes + 16 * sub);
                if (!ok) r[k] = -1;
            }
#pragma unroll
            for (int k = 0; k < kQ4PoolNB; ++k) {
                asm volatile("" : "+v"(x[k].x), "+v"(x[k].y), "+v"(x[k].z), "+v"(x[k].w));
                if (r[k] < 0) x[k] = make_uint4(0u, 0u, 0u, 0u);        // header and codes zero: a +0 row, a +0 wide product
            }
#pragma unroll
            for (int k = 0; k < kQ4PoolNB; ++k) {
                const int s = s0 + k;
                if (s > slast) continue;                                // a spare slot of the sample's last batch: dropped
                const float t = bperm_f(lane0, m[k] * __uint_as_float(x[k].y));
                base = base + m[k] * __uint_as_float(x[k].x);
                wsum = wsum + m[k] * __uint_as_float(x[k].z);
                q4_pool_fma8(x[k].x, t, acc[0], acc[1]);
                q4_pool_fma8(x[k].y, t, acc[2], acc[3]);
                q4_pool_fma8(x[k].z, t, acc[4], acc[5]);
                q4_pool_fma8(x[k].w, t, acc[6], acc[7]);
                if (s + 1 != fend) continue;
                // the field's last slot: y = acc + base, the mean's division by the field's own length, one rounding, one store a dword
                const float bs = bperm_f(lane0, base);
                const float fl = (float)(fw >> 16);
                OT* const o = out + (b * ldo + (int64_t)f * D + col0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float4 y[2];
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const float4 a = acc[2 * j + h];
                        y[h] = make_float4(a.x + bs, a.y + bs, a.z + bs, a.w + bs);
                        if (mode == 1) y[h] = make_float4(y[h].x / fl, y[h].y / fl, y[h].z / fl, y[h].w / fl);
                    }
                    if (live && sub != 0) q4_pool_put8(o + 8 * j, y[0], y[1], valid - 8 * j, st16);
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] = zero4;
                wtot = wtot + wsum;
                base = wsum = 0.0f;
                f = f + 1 < F ? f + 1 : f;                              // (behind the last field: its own word again, never closed twice)
                fw = pf.w[f];
                fend = (int)(fw & 0xFFFFu) + (int)(fw >> 16);
            }
        }
        if (live && sub == 0 && wide_out) wide_out[b * ldw] = wtot;
    }
}

// ===== the keyed FM lookups: raw keys -> frozen key index -> records, one launch ========================================================
// The rows of one batch of NB fields of a lane-group's sample, resolved in the frozen index (mrec_kidx.h).  The batch's probes are dealt
// out over the group's lanes -- lane `sub` hashes and probes the key of batch slot `sub`, one 16-byte slot load a step -- instead of
// every lane walking every key's chain; a group of fewer than NB lanes (lpr = 2, 3) takes a second round for slots lpr .. NB - 1.  A
// spare slot (k >= nf) probes the batch's last field again, as the record loads do.  The probe loops' trip counts differ per lane:
// the loops are closed -- every lane of the group back in step -- before the ds_bpermute reads that hand slot k's row to all lanes
// (source lane and round are the same for the whole wave: lpr is a kernel argument).
template <int NB, class K>
__device__ __forceinline__ void q_keyed_rows(const uint8_t* __restrict__ kidx, uint32_t kmask, int cap, const K* __restrict__ keys, int64_t e,
                                             int nf, int sub, int lane0, int lpr, int64_t (&r)[NB]) {
    int mine[2] = {-1, -1};
#pragma unroll
    for (int rd = 0; rd < 2; ++rd) {
        const int k = sub + rd * lpr;
        if ((rd == 0 || lpr < NB) && k < NB) mine[rd] = kidx_probe(kidx, kmask, cap, (int64_t)keys[e + (k < nf ? k : nf - 1)]);
    }
#pragma unroll
    for (int k = 0; k < NB; ++k) {
        const bool second = k >= lpr;                                   // (uniform)
        r[k] = (int64_t)__builtin_amdgcn_ds_bpermute((lane0 + (second ? k - lpr : k)) << 2, second ? mine[1] : mine[0]);
    }
}

// k_q8_fm_lookup with q_keyed_rows in place of the id loads: same lane-group, same batch of kQ8FmNB fields, the same unconditional
// record loads, q8_dequant4 and q8_fm_put in the same order, the same column-sum tree -- rows and lin_fm are k_q8_fm_lookup's over
// ids[b, f] = find(keys[b, f]), bit for bit.  A key that is not in the index (and key -1) arrives as row -1: a zero record.
template <class K, class OT>
__global__ __launch_bounds__(256) void k_q8_fm_lookup_keyed(const uint8_t* __restrict__ rec, int64_t V, int64_t row_bytes, int D,
                                                            const uint8_t* __restrict__ kidx, uint32_t kmask, const K* __restrict__ keys,
                                                            const float* __restrict__ wts, int64_t B, int F, OT* __restrict__ rows,
                                                            float* __restrict__ lin_fm, RowGeom gm, bool st16) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / gm.lpr, sub = lane - grp * gm.lpr;
    if (grp >= gm.G) return;
    const int lane0 = lane - sub;
    const int col0 = (sub - 1) * 16;                                    // (the header lane: -16, never used as a column)
    const int valid = sub == 0 ? 0 : (D - col0 < 16 ? D - col0 : 16);
    const int64_t ng = (int64_t)gridDim.x * 4 * gm.G;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const int cap = kidx_cap(kidx, kmask);
    for (int64_t b0 = ((int64_t)blockIdx.x * 4 + wave) * gm.G; b0 < B; b0 += ng) {
        const int64_t b = b0 + grp;
        const bool live = b < B;
        const int64_t e0 = (live ? b : 0) * (int64_t)F;
        float4 s[4] = {zero4, zero4, zero4, zero4}, q[4] = {zero4, zero4, zero4, zero4};
        float lin = 0.0f;
        const auto fields = [&](const int f, const int nf) {
            int64_t r[kQ8FmNB];
            float t[kQ8FmNB];
            uint4 x[kQ8FmNB];
#pragma unroll
            for (int k = 0; k < kQ8FmNB; ++k) t[k] = wts[e0 + f + (k < nf ? k : nf - 1)];
            q_keyed_rows<kQ8FmNB>(kidx, kmask, cap, keys, e0 + f, nf, sub, lane0, gm.lpr, r);
#pragma unroll
            for (int k = 0; k < kQ8FmNB; ++k) {
                const bool ok = r[k] >= 0 && r[k] < V;
                x[k] = *(const uint4*)(rec + (ok ? r[k] : 0) * row_bytes + 16 * sub);
                if (!ok) r[k] = -1;
            }
#pragma unroll
            for (int k = 0; k < kQ8FmNB; ++k) {
                asm volatile("" : "+v"(x[k].x), "+v"(x[k].y), "+v"(x[k].z), "+v"(x[k].w));
                if (r[k] < 0) x[k] = make_uint4(0u, 0u, 0u, 0u);        // header and codes zero: a zero row, a zero linear weight
            }
#pragma unroll
            for (int k = 0; k < kQ8FmNB; ++k) {
                const float lo = bperm_f(lane0, __uint_as_float(x[k].x));
                const float scale = bperm_f(lane0, __uint_as_float(x[k].y));
                if (k >= nf) continue;
                if (sub == 0) {
                    lin = lin + __uint_as_float(x[k].z) * t[k];
                    continue;
                }
                const float4 y[4] = {q8_dequant4(x[k].x, lo, scale, t[k]), q8_dequant4(x[k].y, lo, scale, t[k]),
                                     q8_dequant4(x[k].z, lo, scale, t[k]), q8_dequant4(x[k].w, lo, scale, t[k])};
                q8_fm_put(rows + ((b * F + f + k) * (int64_t)D + col0), y, valid, st16, live, s, q);
            }
        };
        int f = 0;
        for (; f + kQ8FmNB <= F; f += kQ8FmNB) fields(f, kQ8FmNB);
        if (f < F) fields(f, F - f);
        float part = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (valid > 4 * j)
                part += ((s[j].x * s[j].x - q[j].x) + (s[j].y * s[j].y - q[j].y)) + ((s[j].z * s[j].z - q[j].z) + (s[j].w * s[j].w - q[j].w));
#pragma unroll
        for (int off = 16; off >= 1; off >>= 1) {
            const float o = __shfl_down(part, off, 64);
            if (sub + off < gm.lpr) part += o;
        }
        if (live && sub == 0) lin_fm[b] = lin + 0.5f * part;
    }
}

// k_q4_fm_lookup with q_keyed_rows in place of the id loads (see k_q8_fm_lookup_keyed): q4_dequant8 and q4_fm_put8 in k_q4_fm_lookup's
// order, its branch-free lane roles and its column-sum tree.
template <class K, class OT>
__global__ __launch_bounds__(256) void k_q4_fm_lookup_keyed(const uint8_t* __restrict__ rec, int64_t V, int64_t row_bytes, int D,
                                                            const uint8_t* __restrict__ kidx, uint32_t kmask, const K* __restrict__ keys,
                                                            const float* __restrict__ wts, int64_t B, int F, OT* __restrict__ rows,
                                                            float* __restrict__ lin_fm, RowGeom gm, bool st16) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / gm.lpr, sub = lane - grp * gm.lpr;
    if (grp >= gm.G) return;
    const int lane0 = lane - sub;
    const int col0 = (sub - 1) * 32;                                    // (the header lane: -32, never used as a column)
    const int valid = sub == 0 ? 0 : (D - col0 < 32 ? D - col0 : 32);
    const int64_t ng = (int64_t)gridDim.x * 4 * gm.G;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    const int cap = kidx_cap(kidx, kmask);
    for (int64_t b0 = ((int64_t)blockIdx.x * 4 + wave) * gm.G; b0 < B; b0 += ng) {
        const int64_t b = b0 + grp;
        const bool live = b < B;
        const int64_t e0 = (live ? b : 0) * (int64_t)F;
        float4 s[8] = {zero4, zero4, zero4, zero4, zero4, zero4, zero4, zero4};
        float4 q[8] = {zero4, zero4, zero4, zero4, zero4, zero4, zero4, zero4};
        float lin = 0.0f;
        const auto fields = [&](const int f, const int nf) {
            int64_t r[kQ4FmNB];
            float t[kQ4FmNB];
            uint4 x[kQ4FmNB];
#pragma unroll
            for (int k = 0; k < kQ4FmNB; ++k) t[k] = wts[e0 + f + (k < nf ? k : nf - 1)];
            q_keyed_rows<kQ4FmNB>(kidx, kmask, cap, keys, e0 + f, nf, sub, lane0, gm.lpr, r);
#pragma unroll
            for (int k = 0; k < kQ4FmNB; ++k) {
                const bool ok = r[k] >= 0 && r[k] < V;
                x[k] = *(const uint4*)(rec + (ok ? r[k] : 0) * row_bytes + 16 * sub);
                if (!ok) r[k] = -1;
            }
#pragma unroll
            for (int k = 0; k < kQ4FmNB; ++k) {
                asm volatile("" : "+v"(x[k].x), "+v"(x[k].y), "+v"(x[k].z), "+v"(x[k].w));
                if (r[k] < 0) x[k] = make_uint4(0u, 0u, 0u, 0u);        // header and codes zero: a zero row, a zero linear weight
            }
#pragma unroll
            for (int k = 0; k < kQ4FmNB; ++k) {
                const float lo = bperm_f(lane0, __uint_as_float(x[k].x));
                const float scale = bperm_f(lane0, __uint_as_float(x[k].y));
                if (k >= nf) continue;
                lin = lin + __uint_as_float(x[k].z) * t[k];
                const unsigned w[4] = {x[k].x, x[k].y, x[k].z, x[k].w};
                OT* const o = rows + ((b * F + f + k) * (int64_t)D + col0);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float4 y0, y1;
                    q4_dequant8(w[j], lo, scale, t[k], y0, y1);
                    q4_fm_put8(o + 8 * j, y0, y1, valid - 8 * j, st16, live, s[2 * j], s[2 * j + 1], q[2 * j], q[2 * j + 1]);
                }
            }
        };
        int f = 0;
        for (; f + kQ4FmNB <= F; f += kQ4FmNB) fields(f, kQ4FmNB);
        if (f < F) fields(f, F - f);
        float part = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (valid > 4 * j)
                part += ((s[j].x * s[j].x - q[j].x) + (s[j].y * s[j].y - q[j].y)) + ((s[j].z * s[j].z - q[j].z) + (s[j].w * s[j].w - q[j].w));
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) {
            const float o = __shfl_down(part, off, 64);
            if (sub + off < gm.lpr) part += o;
        }
        if (live && sub == 0) lin_fm[b] = lin + 0.5f * part;
    }
}

int q4_check(int32_t D, int64_t row_bytes) {
    if (D <= 0) return MREC_EINVAL;
    if (D % 4 || D > 256) return MREC_EUNSUPPORTED;
    if (row_bytes % 16 || row_bytes < kQ8Hdr + 16 * ((D + 31) / 32)) return MREC_EINVAL;
    return MREC_OK;
}

/* D and row_bytes as include/mrec.h states them: the shape first (MREC_EUNSUPPORTED), then the record size (MREC_EINVAL) */
int q8_check(int32_t D, int64_t row_bytes) {
    if (D <= 0) return MREC_EINVAL;
    if (D % 4 || D > 256) return MREC_EUNSUPPORTED;
    if (row_bytes % 16 || row_bytes < kQ8Hdr + 16 * ((D + 15) / 16)) return MREC_EINVAL;
    return MREC_OK;
}

// The two keyed FM entries (include/mrec.h): the unkeyed entry's refusals in its order -- `rc` is the format's shape / record-size code --,
// then the index's, all before the launch.
int q_fm_lookup_keyed(int bits, int rc, const void* records, int64_t V, int64_t row_bytes, int32_t D, const void* kidx, const void* keys,
                      int32_t key_bytes, const float* wts, int64_t B, int32_t F, void* rows, int32_t rows_kind, float* lin_fm, void* stream) {
    if (rc) return rc;
    if ((key_bytes != 4 && key_bytes != 8) || rows_kind < 0 || rows_kind > 2 || B < 0 || F < 1 || V < 1) return MREC_EINVAL;
    if (B == 0) return MREC_OK;
    if (!records || !keys || !wts || !rows || !lin_fm) return MREC_EINVAL;
    const int esz = rows_kind == 0 ? 4 : 2;
    if (!al16(records) || (((uintptr_t)rows) & (esz == 4 ? 15 : 7))) return MREC_EUNSUPPORTED;
    if (!kidx) return MREC_EINVAL;
    uint32_t kmask = 0;
    if (const int krc = mrec_kidx_host_mask(kidx, &kmask)) return krc;
    const bool st16 = al16(rows) && (D * esz) % 16 == 0;
    const int lpr = (bits == 4 ? (D + 31) / 32 : (D + 15) / 16) + 1;
    const RowGeom gm{lpr, 64 / lpr};
    int64_t blocks = mrec_cdiv(B, (int64_t)4 * gm.G);
    if (blocks > 2048) blocks = 2048;                                   // 256 CUs x 8 workgroups, each walking B
    return by_key(keys, key_bytes, [&](auto* kp) {
        return by_out(rows, rows_kind, [&](auto* op) {
            if (bits == 4)
                k_q4_fm_lookup_keyed<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>((const uint8_t*)records, V, row_bytes, D, (const uint8_t*)kidx,
                                                                                         kmask, kp, wts, B, F, op, lin_fm, gm, st16);
            else
                k_q8_fm_lookup_keyed<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>((const uint8_t*)records, V, row_bytes, D, (const uint8_t*)kidx,
                                                                                         kmask, kp, wts, B, F, op, lin_fm, gm, st16);
            MREC_LAUNCH_CHECK();
            return (int)MREC_OK;
        });
    });
}

}  // namespace

MREC_API int mrec_q8_row_bytes(int32_t D) {
    if (D <= 0) return MREC_EINVAL;
    if (D % 4 || D > 256) return MREC_EUNSUPPORTED;
    return kQ8Hdr + 16 * ((D + 15) / 16);
}

MREC_API int mrec_q8_quantize_rows(const float* table, int64_t V, int64_t ld, int32_t D, const float* wide, int64_t ldw, void* records,
                                   int64_t row_bytes, void* stream) {
    if (const int rc = q8_check(D, row_bytes)) return rc;
    if (V < 0 || ld < D || (wide && ldw < 1)) return MREC_EINVAL;
    if (V == 0) return MREC_OK;
    if (!table || !records) return MREC_EINVAL;
    if (ld % 4 || !al16(table) || !al16(records)) return MREC_EUNSUPPORTED;
    const RowGeom gm{D / 4, 64 / (D / 4)};
    int64_t blocks = mrec_cdiv(V, 4 * gm.G);
    if (blocks > 2048) blocks = 2048;                                   // 256 CUs x 8 workgroups, each walking V
    k_q8_quantize<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(table, V, ld, D, wide, ldw, (uint8_t*)records, row_bytes, gm);
    MREC_LAUNCH_CHECK();
    return MREC_OK;
}

MREC_API int mrec_q8_gather_rows(const void* records, int64_t V, int64_t row_bytes, int32_t D, const void* ids, int32_t id_bytes, int64_t n,
                                 const float* row_scale, void* out, int32_t out_kind, int64_t ldo, float* wide_prod, int64_t ldw,
                                 void* stream) {
    if (const int rc = q8_check(D, row_bytes)) return rc;
    if ((id_bytes != 4 && id_bytes != 8) || out_kind < 0 || out_kind > 2 || n < 0 || V < 1 || ldo < D) return MREC_EINVAL;
    if (wide_prod && (ldw < 2 || ldw % 2 || (((uintptr_t)wide_prod) & 7))) return MREC_EINVAL;
    if (n == 0) return MREC_OK;
    if (!records || !ids || !out) return MREC_EINVAL;
    const int esz = out_kind == 0 ? 4 : 2;
    if (ldo % 4 || !al16(records) || (((uintptr_t)out) & 7)) return MREC_EUNSUPPORTED;
    const bool st16 = al16(out) && (ldo * esz) % 16 == 0;
    if (esz == 4 && !st16) return MREC_EUNSUPPORTED;
    const int lpr = (D + 15) / 16 + 1;
    const RowGeom gm{lpr, 64 / lpr};
    const int64_t blocks = mrec_cdiv(n, (int64_t)4 * gm.G * kQ8GB);
    if (blocks >= (1ll << 31)) return MREC_EUNSUPPORTED;
    return by_key(ids, id_bytes, [&](auto* kp) {
        return by_out(out, out_kind, [&](auto* op) {
            k_q8_gather<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>((const uint8_t*)records, V, row_bytes, D, kp, n, row_scale, op, ldo,
                                                                            wide_prod, ldw, gm, st16);
            MREC_LAUNCH_CHECK();
            return (int)MREC_OK;
        });
    });
}

MREC_API int mrec_q8_fm_lookup(const void* records, int64_t V, int64_t row_bytes, int32_t D, const void* ids, int32_t id_bytes,
                               const float* wts, int64_t B, int32_t F, void* rows, int32_t rows_kind, float* lin_fm, void* stream) {
    if (const int rc = q8_check(D, row_bytes)) return rc;
    if ((id_bytes != 4 && id_bytes != 8) || rows_kind < 0 || rows_kind > 2 || B < 0 || F < 1 || V < 1) return MREC_EINVAL;
    if (B == 0) return MREC_OK;
    if (!records || !ids || !wts || !rows || !lin_fm) return MREC_EINVAL;
    const int esz = rows_kind == 0 ? 4 : 2;
    if (!al16(records) || (((uintptr_t)rows) & (esz == 4 ? 15 : 7))) return MREC_EUNSUPPORTED;
    const bool st16 = al16(rows) && (D * esz) % 16 == 0;
    const int lpr = (D + 15) / 16 + 1;
    const RowGeom gm{lpr, 64 / lpr};
    int64_t blocks = mrec_cdiv(B, (int64_t)4 * gm.G);
    if (blocks > 2048) blocks = 2048;                                   // 256 CUs x 8 workgroups, each walking B
    return by_key(ids, id_bytes, [&](auto* kp) {
        return by_out(rows, rows_kind, [&](auto* op) {
            k_q8_fm_lookup<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>((const uint8_t*)records, V, row_bytes, D, kp, wts, B, F, op,
                                                                               lin_fm, gm, st16);
            MREC_LAUNCH_CHECK();
            return (int)MREC_OK;
        });
    });
}

MREC_API int mrec_q8_gather_pool_fields(const void* records, int64_t V, int64_t row_bytes, int32_t D, const void* ids, int32_t id_bytes,
                                        int64_t B, int32_t F, const int32_t* field_len, const float* mask, int32_t mode, void* out,
                                        int32_t out_kind, int64_t ldo, float* wide_out, int64_t ldw, void* stream) {
    if (const int rc = q8_check(D, row_bytes)) return rc;
    if ((id_bytes != 4 && id_bytes != 8) || out_kind < 0 || out_kind > 2 || (mode != 0 && mode != 1) || B < 0 || V < 1 || F < 1 || !field_len)
        return MREC_EINVAL;
    for (int f = 0; f < F; ++f)
        if (field_len[f] < 1) return MREC_EINVAL;
    if (ldo == 0) ldo = (int64_t)F * D;
    if (ldo < (int64_t)F * D || (wide_out && ldw < 1)) return MREC_EINVAL;
    if (F > MREC_POOL_MAX_FIELDS) return MREC_EUNSUPPORTED;
    Q8PoolFields pf{};
    int64_t Ls = 0;
    for (int f = 0; f < F; ++f) {
        if (Ls + field_len[f] > MREC_POOL_MAX_BAG) return MREC_EUNSUPPORTED;
        pf.w[f] = (unsigned)Ls | ((unsigned)field_len[f] << 16);
        Ls += field_len[f];
    }
    if (B * F >= (int64_t(1) << 31)) return MREC_EUNSUPPORTED;
    if (B == 0) return MREC_OK;
    if (!records || !ids || !out) return MREC_EINVAL;
    const int esz = out_kind == 0 ? 4 : 2;
    if (ldo % 4 || !al16(records) || (((uintptr_t)out) & (esz == 4 ? 15 : 7))) return MREC_EUNSUPPORTED;
    const bool st16 = al16(out) && (ldo * esz) % 16 == 0 && (D * esz) % 16 == 0;      // (every field's column block, every row)
    const int lpr = (D + 15) / 16 + 1;
    const RowGeom gm{lpr, 64 / lpr};
    int64_t blocks = mrec_cdiv(B, (int64_t)4 * gm.G);
    if (blocks > 2048) blocks = 2048;                                   // 256 CUs x 8 workgroups, each walking B
    return by_key(ids, id_bytes, [&](auto* kp) {
        return by_out(out, out_kind, [&](auto* op) {
            k_q8_gather_pool_fields<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>((const uint8_t*)records, V, row_bytes, D, kp, mask, B, F,
                                                                                        (int)Ls, mode, op, ldo, wide_out, ldw, gm, st16, pf);
            MREC_LAUNCH_CHECK();
            return (int)MREC_OK;
        });
    });
}

MREC_API int mrec_q4_row_bytes(int32_t D) {
    if (D <= 0) return MREC_EINVAL;
    if (D % 4 || D > 256) return MREC_EUNSUPPORTED;
    return kQ8Hdr + 16 * ((D + 31) / 32);
}

MREC_API int mrec_q4_quantize_rows(const float* table, int64_t V, int64_t ld, int32_t D, const float* wide, int64_t ldw, void* records,
                                   int64_t row_bytes, void* stream) {
    if (const int rc = q4_check(D, row_bytes)) return rc;
    if (V < 0 || ld < D || (wide && ldw < 1)) return MREC_EINVAL;
    if (V == 0) return MREC_OK;
    if (!table || !records) return MREC_EINVAL;
    if (ld % 4 || !al16(table) || !al16(records)) return MREC_EUNSUPPORTED;
    const int nd = (D + 7) / 8;
    const RowGeom gm{nd, 64 / nd};
    int64_t blocks = mrec_cdiv(V, 4 * gm.G);
    if (blocks > 2048) blocks = 2048;                                   // 256 CUs x 8 workgroups, each walking V
    k_q4_quantize<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(table, V, ld, D, wide, ldw, (uint8_t*)records, row_bytes, gm);
    MREC_LAUNCH_CHECK();
    return MREC_OK;
}

MREC_API int mrec_q4_gather_rows(const void* records, int64_t V, int64_t row_bytes, int32_t D, const void* ids, int32_t id_bytes, int64_t n,
                                 const float* row_scale, void* out, int32_t out_kind, int64_t ldo, float* wide_prod, int64_t ldw,
                                 void* stream) {
    if (const int rc = q4_check(D, row_bytes)) return rc;
    if ((id_bytes != 4 && id_bytes != 8) || out_kind < 0 || out_kind > 2 || n < 0 || V < 1 || ldo < D) return MREC_EINVAL;
    if (wide_prod && (ldw < 2 || ldw % 2 || (((uintptr_t)wide_prod) & 7))) return MREC_EINVAL;
    if (n == 0) return MREC_OK;
    if (!records || !ids || !out) return MREC_EINVAL;
    const int esz = out_kind == 0 ? 4 : 2;
    if (ldo % 4 || !al16(records) || (((uintptr_t)out) & 7)) return MREC_EUNSUPPORTED;
    const bool st16 = al16(out) && (ldo * esz) % 16 == 0;
    if (esz == 4 && !st16) return MREC_EUNSUPPORTED;
    const int lpr = (D + 31) / 32 + 1;
    const RowGeom gm{lpr, 64 / lpr};
    const int64_t blocks = mrec_cdiv(n, (int64_t)4 * gm.G * kQ4GB);
    if (blocks >= (1ll << 31)) return MREC_EUNSUPPORTED;
    return by_key(ids, id_bytes, [&](auto* kp) {
        return by_out(out, out_kind, [&](auto* op) {
            k_q4_gather<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>((const uint8_t*)records, V, row_bytes, D, kp, n, row_scale, op, ldo,
                                                                            wide_prod, ldw, gm, st16);
            MREC_LAUNCH_CHECK();
            return (int)MREC_OK;
        });
    });
}

MREC_API int mrec_q4_fm_lookup(const void* records, int64_t V, int64_t row_bytes, int32_t D, const void* ids, int32_t id_bytes,
                               const float* wts, int64_t B, int32_t F, void* rows, int32_t rows_kind, float* lin_fm, void* stream) {
    if (const int rc = q4_check(D, row_bytes)) return rc;
    if ((id_bytes != 4 && id_bytes != 8) || rows_kind < 0 || rows_kind > 2 || B < 0 || F < 1 || V < 1) return MREC_EINVAL;
    if (B == 0) return MREC_OK;
    if (!records || !ids || !wts || !rows || !lin_fm) return MREC_EINVAL;
    const int esz = rows_kind == 0 ? 4 : 2;
    if (!al16(records) || (((uintptr_t)rows) & (esz == 4 ? 15 : 7))) return MREC_EUNSUPPORTED;
    const bool st16 = al16(rows) && (D * esz) % 16 == 0;
    const int lpr = (D + 31) / 32 + 1;
    const RowGeom gm{lpr, 64 / lpr};
    int64_t blocks = mrec_cdiv(B, (int64_t)4 * gm.G);
    if (blocks > 2048) blocks = 2048;                                   // 256 CUs x 8 workgroups, each walking B
    return by_key(ids, id_bytes, [&](auto* kp) {
        return by_out(rows, rows_kind, [&](auto* op) {
            k_q4_fm_lookup<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>((const uint8_t*)records, V, row_bytes, D, kp, wts, B, F, op,
                                                                               lin_fm, gm, st16);
            MREC_LAUNCH_CHECK();
            return (int)MREC_OK;
        });
    });
}

MREC_API int mrec_q4_gather_pool_fields(const void* records, int64_t V, int64_t row_bytes, int32_t D, const void* ids, int32_t id_bytes,
                                        int64_t B, int32_t F, const int32_t* field_len, const float* mask, int32_t mode, void* out,
                                        int32_t out_kind, int64_t ldo, float* wide_out, int64_t ldw, void* stream) {
    if (const int rc = q4_check(D, row_bytes)) return rc;
    if ((id_bytes != 4 && id_bytes != 8) || out_kind < 0 || out_kind > 2 || (mode != 0 && mode != 1) || B < 0 || V < 1 || F < 1 || !field_len)
        return MREC_EINVAL;
    for (int f = 0; f < F; ++f)
        if (field_len[f] < 1) return MREC_EINVAL;
    if (ldo == 0) ldo = (int64_t)F * D;
    if (ldo < (int64_t)F * D || (wide_out && ldw < 1)) return MREC_EINVAL;
    if (F > MREC_POOL_MAX_FIELDS) return MREC_EUNSUPPORTED;
    Q8PoolFields pf{};
    int64_t Ls = 0;
    for (int f = 0; f < F; ++f) {
        if (Ls + field_len[f] > MREC_POOL_MAX_BAG) return MREC_EUNSUPPORTED;
        pf.w[f] = (unsigned)Ls | ((unsigned)field_len[f] << 16);
        Ls += field_len[f];
    }
    if (B * F >= (int64_t(1) << 31)) return MREC_EUNSUPPORTED;
    if (B == 0) return MREC_OK;
    if (!records || !ids || !out) return MREC_EINVAL;
    const int esz = out_kind == 0 ? 4 : 2;
    if (ldo % 4 || !al16(records) || (((uintptr_t)out) & (esz == 4 ? 15 : 7))) return MREC_EUNSUPPORTED;
    const bool st16 = al16(out) && (ldo * esz) % 16 == 0 && (D * esz) % 16 == 0;      // (every field's column block, every row)
    const int lpr = (D + 31) / 32 + 1;
    const RowGeom gm{lpr, 64 / lpr};
    int64_t blocks = mrec_cdiv(B, (int64_t)4 * gm.G);
    if (blocks > 2048) blocks = 2048;                                   // 256 CUs x 8 workgroups, each walking B
    return by_key(ids, id_bytes, [&](auto* kp) {
        return by_out(out, out_kind, [&](auto* op) {
            k_q4_gather_pool_fields<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>((const uint8_t*)records, V, row_bytes, D, kp, mask, B, F,
                                                                                        (int)Ls, mode, op, ldo, wide_out, ldw, gm, st16, pf);
            MREC_LAUNCH_CHECK();
            return (int)MREC_OK;
        });
    });
}

MREC_API int mrec_q8_fm_lookup_keyed(const void* records, int64_t V, int64_t row_bytes, int32_t D, const void* kidx, const void* keys,
                                     int32_t key_bytes, const float* wts, int64_t B, int32_t F, void* rows, int32_t rows_kind, float* lin_fm,
                                     void* stream) {
    return q_fm_lookup_keyed(8, q8_check(D, row_bytes), records, V, row_bytes, D, kidx, keys, key_bytes, wts, B, F, rows, rows_kind, lin_fm, stream);
}

MREC_API int mrec_q4_fm_lookup_keyed(const void* records, int64_t V, int64_t row_bytes, int32_t D, const void* kidx, const void* keys,
                                     int32_t key_bytes, const float* wts, int64_t B, int32_t F, void* rows, int32_t rows_kind, float* lin_fm,
                                     void* stream) {
    return q_fm_lookup_keyed(4, q4_check(D, row_bytes), records, V, row_bytes, D, kidx, keys, key_bytes, wts, B, F, rows, rows_kind, lin_fm, stream);
}
