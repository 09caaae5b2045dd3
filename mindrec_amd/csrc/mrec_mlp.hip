// mrec_mlp.hip -- the elementwise / reduction ends of the Wide&Deep dense net, fused, for gfx950.
//
// The hidden DenseLayers (models/wide_deep/src/wide_and_deep.py:113-133) run on the matrix cores (mrec_dense.hip; their
// ReLU / BiasAdd bprops are GEMM epilogues there); what is left is the output end of the net, HBM-bound byte work that
// MindSpore runs as separate primitives (the 128 -> 1 output layer, wide + deep add :315,
// SigmoidCrossEntropyWithLogits + ReduceMean :352-354 and their bprops).  Three kernels cover it:
//
//  k_head_fwd_bwd    : logit = h4 . W5 + b5 + wide;  loss terms;  dlogit = (sigmoid(logit) - y) * scale;
//                      dh4 = dlogit * W5 masked by h4 > 0;  dW5 += h4 * dlogit;  db5 += dlogit
//                      -- forward AND backward of the output layer and the loss in one pass over h4.
//  k_head_any        : the same arithmetic for every K5 % 8 == 0 up to 2048 (k_head_fwd_bwd: K5 / 8 a power of two <= 64).
//  k_head_predict    : k_head_any's forward half for evaluation: logit, sigmoid(logit) and, with a label, the mean loss.
//
// What a row gets is written ONCE, in the head_* functions below, and every kernel calls them: its workgroup's rows, the wide
// term, the row dot's tree, the sums over a workgroup's row groups (sigmoid and loss term: mrec_mlp.h).  One host prologue
// (head_geom, head_check, head_dispatch) gives all three the same launch geometry.
// They reduce over the batch with per-block partials written to a workspace and a second tiny kernel
// that adds the partials in block order: bitwise reproducible, no float atomics.
#include <type_traits>

#include "mrec_common.h"
#include "mrec_dropout.h"
#include "mrec_mlp.h"

namespace {

// Output head.  K5 = 8 C = width of the last hidden layer.  A row belongs to a group of G adjacent lanes (a power of two <= 64),
// a workgroup meets MB / G rows a pass.
// partial layout per block: [K5] dW5 partials, [K5] column sums of dh4 (= bias gradient of the last
// hidden layer), then db5 partial, then loss partial.
// the row's 8 values of this lane: 16 bytes of 16-bit values, or 32 bytes of fp32 (KIND 2: the fp32 net)
template <int KIND> __device__ __forceinline__ void load8k(const uint4* __restrict__ h, int64_t idx, float (&f)[8]) {
    if (KIND == 2) {
        const float4 a = ((const float4*)h)[2 * idx], b = ((const float4*)h)[2 * idx + 1];
        f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
    } else {
        unpack8t<KIND == 1>(h[idx], f);
    }
}
template <int KIND> __device__ __forceinline__ void store8k(uint4* __restrict__ h, int64_t idx, const float (&f)[8]) {
    if (KIND == 2) {
        ((float4*)h)[2 * idx] = make_float4(f[0], f[1], f[2], f[3]);
        ((float4*)h)[2 * idx + 1] = make_float4(f[4], f[5], f[6], f[7]);
    } else {
        h[idx] = pack8t<KIND == 1>(f);
    }
}

// ---- what the head kernels share ------------------------------------------------------------------------------------------
// the rows [r_begin, r_end) of this workgroup
__device__ __forceinline__ void head_rows(int rows_per_block, int64_t B, int64_t& r_begin, int64_t& r_end) {
    r_begin = (int64_t)blockIdx.x * rows_per_block;
    r_end = (r_begin + rows_per_block < B) ? r_begin + rows_per_block : B;
}

// The wide branch of row r: either given per sample, or as the per-field products the fused lookup wrote ([B, F, 2]: product,
// pad).  The G lanes of the row load the products side by side (one pass of loads, not F dependent ones), then every
// lane adds them up in FIELD ORDER through shuffles -- ReduceSum over the fields, then + Wide_b: the same adds in the
// same order as mrec_wide_sum / the CPU restatement.  (The G lanes of a row are converged here.)
__device__ __forceinline__ float head_wide_term(const float* wprod, int F, const float* wide_bias,
                                                const float* wide, int64_t r, bool valid, int cg, int G) {
    float wv = 0.0f;
    if (wprod) {
        const int lane_row0 = (threadIdx.x & 63) - cg;           // first lane of this row's group
        float acc_w = 0.0f;
        for (int f0 = 0; f0 < F; f0 += G) {
            const int f = f0 + cg;
            const float mine = (valid && f < F) ? wprod[2 * (r * F + f)] : 0.0f;
            const int nf = (F - f0 < G) ? F - f0 : G;
            for (int c = 0; c < nf; ++c) acc_w = acc_w + __shfl(mine, lane_row0 + c, 64);
        }
        wv = acc_w + *wide_bias;
    } else if (valid) {
        wv = wide[r];
    }
    return wv;
}

// a lane's share of the row dot, added over the G lanes of the row (adjacent lanes): a fixed xor tree
__device__ __forceinline__ float head_group_sum(float part, int G) {
    for (int d = G >> 1; d >= 1; d >>= 1) part += __shfl_xor(part, d, 64);
    return part;
}

// One [8 columns a lane] accumulator of the workgroup's partial row: every lane leaves its 8 sums in red, then the lanes of row
// group 0 add the row groups' in group order (rows cg, G + cg, ..) and write dst[0..8) (own: this lane has columns there).
// red is free again after the caller's next __syncthreads().
__device__ __forceinline__ void head_block_sum(float (*red)[8], const float (&acc)[8], int cg, int rl, int G, int RP, bool own,
                                               float* dst) {
#pragma unroll
    for (int k = 0; k < 8; ++k) red[threadIdx.x][k] = acc[k];
    __syncthreads();
    if (rl == 0 && own) {
        float s[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] = red[cg][k];
        for (int q = 1; q < RP; ++q) {
#pragma unroll
            for (int k = 0; k < 8; ++k) s[k] += red[q * G + cg][k];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) dst[k] = s[k];
    }
}

// the N per-row scalars the first lane of every row group left in red2 (db5 and loss; loss alone), added in group order from 0:
// one thread's, after a barrier
template <int N> __device__ __forceinline__ void head_block_scalars(const float (*red2)[N], int G, int RP, float* dst) {
    float s[N];
#pragma unroll
    for (int n = 0; n < N; ++n) s[n] = 0.0f;
    for (int q = 0; q < RP; ++q) {
#pragma unroll
        for (int n = 0; n < N; ++n) s[n] += red2[q * G][n];
    }
#pragma unroll
    for (int n = 0; n < N; ++n) dst[n] = s[n];
}

template <int KIND>      // 0: bfloat16, 1: IEEE half, 2: fp32 activations
__global__ __launch_bounds__(MB) void k_head_fwd_bwd(const uint4* __restrict__ h4, const float* __restrict__ w5,
                                                     const float* __restrict__ b5, const float* __restrict__ wide,
                                                     const float* __restrict__ label, int64_t B, int CG,
                                                     int rows_per_block, float dscale, float* __restrict__ logit_out,
                                                     float* __restrict__ dlogit_out, uint4* __restrict__ dh4,
                                                     float* __restrict__ partial, const float* __restrict__ wprod, int F,
                                                     const float* __restrict__ wide_bias, float dh_scale) {
    __shared__ float red[MB][8];
    __shared__ float red2[MB][2];
    const int cg = threadIdx.x % CG, rl = threadIdx.x / CG, RP = MB / CG;
    int64_t r_begin, r_end;
    head_rows(rows_per_block, B, r_begin, r_end);
    float w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = w5[cg * 8 + k];
    const float bias = *b5;
    float accw[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float accd[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float accb = 0.0f, accl = 0.0f;
    // all threads of a row-group iterate together (the shuffles of head_group_sum / head_wide_term need the CG lanes of a row converged)
    for (int64_t r0 = r_begin; r0 < r_end; r0 += RP) {
        const int64_t r = r0 + rl;
        const bool valid = r < r_end;
        float fh[8];
        if (valid) load8k<KIND>(h4, r * CG + cg, fh);
        else {
#pragma unroll
            for (int k = 0; k < 8; ++k) fh[k] = 0.0f;
        }
        float part = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) part += fh[k] * w[k];
        part = head_group_sum(part, CG);
        const float wv = head_wide_term(wprod, F, wide_bias, wide, r, valid, cg, CG);
        if (valid) {
            const float z = part + bias + wv;
            const float y = label[r];
            const float loss = sigmoid_xent(z, y);
            const float dl = (sigmoid_of(z) - y) * dscale;
            if (cg == 0) {
                logit_out[r] = z;
                dlogit_out[r] = dl;
                accl += loss;
                accb += dl;
            }
            float o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                // d h4 through the last layer, masked by its ReLU (and, where h4 went through Dropout, by that mask: its zeros)
                o[k] = fh[k] > 0.0f ? (dl * w[k]) * dh_scale : 0.0f;
                accw[k] += fh[k] * dl;
                accd[k] += o[k];
            }
            store8k<KIND>(dh4, r * CG + cg, o);
        }
    }
    const int K5 = CG * 8;
    float* p = partial + (int64_t)blockIdx.x * (2 * K5 + 2);
    red2[threadIdx.x][0] = accb;
    red2[threadIdx.x][1] = accl;
    head_block_sum(red, accw, cg, rl, CG, RP, true, p + cg * 8);
    if (threadIdx.x == 0) head_block_scalars<2>(red2, CG, RP, p + 2 * K5);
    __syncthreads();
    head_block_sum(red, accd, cg, rl, CG, RP, true, p + K5 + cg * 8);
}

__global__ __launch_bounds__(MB) void k_head_finish(const float* __restrict__ partial, int nblk, int K5, float inv_B,
                                                    float* __restrict__ dw5, float* __restrict__ db4,
                                                    float* __restrict__ db5, float* __restrict__ loss,
                                                    float* __restrict__ dwide_b) {
    __shared__ float sm[8][32];
    const int W = 2 * K5 + 2;
    const int c = blockIdx.x * 32 + (threadIdx.x & 31);
    const float s = finish_column(partial, nblk, W, c, sm);
    if ((threadIdx.x >> 5) != 0 || c >= W) return;
    if (c < K5) dw5[c] = s;
    else if (c < 2 * K5) db4[c - K5] = s;
    else if (c == 2 * K5) {
        *db5 = s;
        if (dwide_b) *dwide_b = s;       // d loss / d Wide_b is the same sum of dlogit
    } else *loss = s * inv_B;
}

// ---- the same head at any K5 = 8 C, C <= 256 chunks of 8 values a row ------------------------------------------------------------
// A row belongs to a group of G = min(64, pow2ceil(C)) adjacent lanes; lane cg owns the chunks cg, cg + G, .. (NC = ceil(C / G) <= 4
// of them, those at or past C absent: they load zeros, add nothing and store nothing).  What a row gets -- the lane's products
// added chunk by chunk, then a fixed xor tree over the group -- depends on K5 alone, not on the row-group or block that met the
// row.  The raw bits of the NEXT pass's row are loaded before this pass's arithmetic (a block has one row per group in flight
// otherwise); they are widened twice, for the dot and for the bprop, instead of being held as 8 floats a chunk.
template <int KIND> struct HeadQ { static constexpr int n = KIND == 2 ? 2 : 1; };      // 16-byte words of a chunk
template <int KIND, int NC>
__device__ __forceinline__ void head_load_row(const uint4* __restrict__ h4, int64_t r, bool valid, int C, int G, int cg,
                                              uint4 (&raw)[NC][HeadQ<KIND>::n]) {
    constexpr int Q = HeadQ<KIND>::n;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = cg + j * G;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            if (valid && c < C) raw[j][q] = h4[Q * (r * C + c) + q];
            else raw[j][q] = make_uint4(0u, 0u, 0u, 0u);
        }
    }
}
template <int KIND> __device__ __forceinline__ void head_widen(const uint4 (&raw)[HeadQ<KIND>::n], float (&f)[8]) {
    if (KIND == 2) {
        const uint4 a = raw[0], b = raw[HeadQ<KIND>::n - 1];
        f[0] = __uint_as_float(a.x); f[1] = __uint_as_float(a.y); f[2] = __uint_as_float(a.z); f[3] = __uint_as_float(a.w);
        f[4] = __uint_as_float(b.x); f[5] = __uint_as_float(b.y); f[6] = __uint_as_float(b.z); f[7] = __uint_as_float(b.w);
    } else {
        unpack8t<KIND == 1>(raw[0], f);
    }
}
// h4[r] . W5: the lane's products added chunk by chunk, then head_group_sum's tree (k_head_fwd_bwd: its one chunk, the same tree)
template <int KIND, int NC>
__device__ __forceinline__ float head_row_dot(const uint4 (&cur)[NC][HeadQ<KIND>::n], const float (&w)[NC][8], int G) {
    float part = 0.0f;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        float fh[8];
        head_widen<KIND>(cur[j], fh);
#pragma unroll
        for (int k = 0; k < 8; ++k) part += fh[k] * w[j][k];
    }
    return head_group_sum(part, G);
}

template <int KIND, int NC>      // KIND as k_head_fwd_bwd's; NC chunks a lane
__global__ __launch_bounds__(MB) void k_head_any(const uint4* __restrict__ h4, const float* __restrict__ w5,
                                                 const float* __restrict__ b5, const float* __restrict__ wide,
                                                 const float* __restrict__ label, int64_t B, int C, int G, int rows_per_block,
                                                 float dscale, float* __restrict__ logit_out, float* __restrict__ dlogit_out,
                                                 uint4* __restrict__ dh4, float* __restrict__ partial,
                                                 const float* __restrict__ wprod, int F, const float* __restrict__ wide_bias,
                                                 float dh_scale) {
    constexpr int Q = HeadQ<KIND>::n;
    __shared__ float red[MB][8];
    __shared__ float red2[MB][2];
    const int cg = threadIdx.x % G, rl = threadIdx.x / G, RP = MB / G;
    int64_t r_begin, r_end;
    head_rows(rows_per_block, B, r_begin, r_end);
    float w[NC][8], accw[NC][8], accd[NC][8];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = cg + j * G;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            w[j][k] = c < C ? w5[c * 8 + k] : 0.0f;
            accw[j][k] = 0.0f;
            accd[j][k] = 0.0f;
        }
    }
    const float bias = *b5;
    float accb = 0.0f, accl = 0.0f;
    uint4 cur[NC][Q], nxt[NC][Q];
    head_load_row<KIND, NC>(h4, r_begin + rl, r_begin + rl < r_end, C, G, cg, cur);
    // all threads of a block iterate together (the shuffles of head_row_dot / head_wide_term need the G lanes of a row converged)
    for (int64_t r0 = r_begin; r0 < r_end; r0 += RP) {
        const int64_t r = r0 + rl;
        const bool valid = r < r_end;
        head_load_row<KIND, NC>(h4, r + RP, r + RP < r_end, C, G, cg, nxt);
        const float part = head_row_dot<KIND, NC>(cur, w, G);
        const float wv = head_wide_term(wprod, F, wide_bias, wide, r, valid, cg, G);
        if (valid) {
            const float z = part + bias + wv;
            const float y = label[r];
            const float loss = sigmoid_xent(z, y);
            const float dl = (sigmoid_of(z) - y) * dscale;
            if (cg == 0) {
                logit_out[r] = z;
                dlogit_out[r] = dl;
                accl += loss;
                accb += dl;
            }
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const int c = cg + j * G;
                if (c < C) {
                    float fh[8], o[8];
                    head_widen<KIND>(cur[j], fh);
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        o[k] = fh[k] > 0.0f ? (dl * w[j][k]) * dh_scale : 0.0f;
                        accw[j][k] += fh[k] * dl;
                        accd[j][k] += o[k];
                    }
                    store8k<KIND>(dh4, r * C + c, o);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NC; ++j) {
#pragma unroll
            for (int q = 0; q < Q; ++q) cur[j][q] = nxt[j][q];
        }
    }
    // the block's partial row [K5 dw5 | K5 db4 | db5 | loss]: the row groups added in group order, a chunk at a time
    const int K5 = C * 8;
    float* p = partial + (int64_t)blockIdx.x * (2 * K5 + 2);
    red2[threadIdx.x][0] = accb;
    red2[threadIdx.x][1] = accl;
#pragma unroll
    for (int t = 0; t < 2 * NC; ++t) {
        const int j = t >> 1, c = cg + j * G;
        head_block_sum(red, (t & 1) ? accd[j] : accw[j], cg, rl, G, RP, c < C, p + (t & 1) * K5 + c * 8);
        if (t == 0 && threadIdx.x == 0) head_block_scalars<2>(red2, G, RP, p + 2 * K5);
        __syncthreads();
    }
}

// ---- the forward half of k_head_any: evaluation ------------------------------------------------------------------------------
// Same lane geometry and the same functions for a row's weights, dot, wide term, sigmoid and loss term -- so a row's logit is
// k_head_any's bit for bit, and its prob is the sigmoid k_head_any forms.
// Nothing of the backward: no dh4, no dw5 / db4 / db5 accumulators, no red[MB][8].  label nullable: without it no loss term, no
// partial and no LDS use; with it the workgroup leaves ONE partial (its row groups' sums added in group order).
template <int KIND, int NC>      // KIND as k_head_fwd_bwd's; NC chunks a lane
__global__ __launch_bounds__(MB) void k_head_predict(const uint4* __restrict__ h4, const float* __restrict__ w5,
                                                     const float* __restrict__ b5, const float* __restrict__ wide,
                                                     const float* __restrict__ label, int64_t B, int C, int G, int rows_per_block,
                                                     float* __restrict__ logit_out, float* __restrict__ prob_out,
                                                     float* __restrict__ partial, const float* __restrict__ wprod, int F,
                                                     const float* __restrict__ wide_bias) {
    constexpr int Q = HeadQ<KIND>::n;
    __shared__ float red2[MB][1];
    const int cg = threadIdx.x % G, rl = threadIdx.x / G, RP = MB / G;
    int64_t r_begin, r_end;
    head_rows(rows_per_block, B, r_begin, r_end);
    float w[NC][8];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        const int c = cg + j * G;
#pragma unroll
        for (int k = 0; k < 8; ++k) w[j][k] = c < C ? w5[c * 8 + k] : 0.0f;      // (k_head_any's rows of W5)
    }
    const float bias = *b5;
    float accl = 0.0f;
    uint4 cur[NC][Q], nxt[NC][Q];
    head_load_row<KIND, NC>(h4, r_begin + rl, r_begin + rl < r_end, C, G, cg, cur);
    // all threads of a block iterate together (the shuffles of head_row_dot / head_wide_term need the G lanes of a row converged)
    for (int64_t r0 = r_begin; r0 < r_end; r0 += RP) {
        const int64_t r = r0 + rl;
        const bool valid = r < r_end;
        head_load_row<KIND, NC>(h4, r + RP, r + RP < r_end, C, G, cg, nxt);
        const float part = head_row_dot<KIND, NC>(cur, w, G);
        const float wv = head_wide_term(wprod, F, wide_bias, wide, r, valid, cg, G);
        if (valid && cg == 0) {
            const float z = part + bias + wv;
            const float sg = sigmoid_of(z);
            logit_out[r] = z;
            prob_out[r] = sg;
            if (label) {
                const float y = label[r];
                accl += sigmoid_xent(z, y);
            }
        }
#pragma unroll
        for (int j = 0; j < NC; ++j) {
#pragma unroll
            for (int q = 0; q < Q; ++q) cur[j][q] = nxt[j][q];
        }
    }
    if (!label) return;          // (uniform: a kernel argument)
    red2[threadIdx.x][0] = accl;
    __syncthreads();
    if (threadIdx.x == 0) head_block_scalars<1>(red2, G, RP, partial + blockIdx.x);
}

// loss = (the workgroups' partials added in workgroup order, finish_column's order as k_head_finish) / B: one workgroup
__global__ __launch_bounds__(MB) void k_head_predict_finish(const float* __restrict__ partial, int nblk, float inv_B,
                                                            float* __restrict__ loss) {
    __shared__ float sm[8][32];
    const float s = finish_column(partial, nblk, 1, threadIdx.x & 31, sm);
    if (threadIdx.x == 0) *loss = s * inv_B;
}

// ---- host: one launch geometry, one argument check, one (kind, chunks a lane) dispatch ---------------------------------------
inline bool pow2(int x) { return x > 0 && (x & (x - 1)) == 0; }

// C chunks of 8 values a row; G = min(64, pow2ceil(C)) lanes a row, NC chunks a lane, RP rows a pass; nblk workgroups budgeted (a
// power of two <= 256, each with at least a few passes) of which nb are launched, rows_per_block rows (whole passes) each
struct HeadGeom { int C, G, NC, RP, nblk, rows_per_block, nb; };
inline HeadGeom head_geom(int64_t B, int K5) {
    HeadGeom g;
    g.C = K5 / 8;
    g.G = 1;
    while (g.G < g.C && g.G < 64) g.G <<= 1;
    g.NC = (int)mrec_cdiv(g.C, g.G);
    g.RP = MB / g.G;
    int64_t nblk = 256;
    while (nblk > 1 && B / nblk < 4 * g.RP) nblk >>= 1;   // at least a few passes per block
    g.nblk = (int)nblk;
    g.rows_per_block = (int)mrec_cdiv(mrec_cdiv(B, nblk), g.RP) * g.RP;
    g.nb = (int)mrec_cdiv(B, g.rows_per_block);
    return g;
}

// What an entry refuses, in the order every entry refuses it.  HEAD_TRAIN: the backward's outputs (outs: dlogit, dh4, dw5, db4, db5),
// label, loss and the workspace are required, dh_scale >= 1, a workspace of nblk partial rows; without it (evaluation; outs: prob)
// label and loss come together or not at all and only they want a workspace, of nblk floats.  HEAD_POW2: k_head_fwd_bwd's widths.
enum { HEAD_TRAIN = 1, HEAD_POW2 = 2 };
int head_check(int flags, int kind, const void* h4, const float* w5, const float* b5, const float* wide, const float* wprod, int F,
               const float* wide_bias, const float* label, int64_t B, int K5, float dh_scale, const float* logit, bool outs,
               const void* dh4, const float* loss, const void* ws, size_t ws_bytes, HeadGeom* g) {
    const bool train = flags & HEAD_TRAIN;
    if (B <= 0 || K5 <= 0 || kind < 0 || kind > 2 || (train && !(dh_scale >= 1.0f))) return MREC_EINVAL;
    if (wprod && (F <= 0 || !wide_bias)) return MREC_EINVAL;
    if ((wide != nullptr) == (wprod != nullptr)) return MREC_EINVAL;
    if (!h4 || !w5 || !b5 || !logit || !outs) return MREC_EINVAL;
    if (train ? (!label || !loss || !ws) : ((label != nullptr) != (loss != nullptr))) return MREC_EINVAL;
    if (K5 % 8 || K5 > 2048 || ((flags & HEAD_POW2) && (!pow2(K5 / 8) || K5 / 8 > 64))) return MREC_EUNSUPPORTED;
    if ((((uintptr_t)h4 | (uintptr_t)dh4) & 15) != 0) return MREC_EINVAL;
    *g = head_geom(B, K5);
    if (train ? ws_bytes < (size_t)g->nblk * (2 * K5 + 2) * sizeof(float) : (label && (!ws || ws_bytes < (size_t)g->nblk * sizeof(float))))
        return MREC_EWORKSPACE;
    return MREC_OK;
}

// f(KIND, NC) with the two as compile-time constants (std::integral_constant): the kernels' template arguments
template <class Fn> inline void head_dispatch(int kind, int NC, Fn f) {
    auto chunks = [&](auto k) {
        if (NC == 1) f(k, std::integral_constant<int, 1>{});
        else if (NC == 2) f(k, std::integral_constant<int, 2>{});
        else if (NC == 3) f(k, std::integral_constant<int, 3>{});
        else f(k, std::integral_constant<int, 4>{});
    };
    if (kind == 2) chunks(std::integral_constant<int, 2>{});
    else if (kind == 1) chunks(std::integral_constant<int, 1>{});
    else chunks(std::integral_constant<int, 0>{});
}

// The training head.  fixed: k_head_fwd_bwd and its widths (K5 / 8 a power of two <= 64: G = C, one chunk a lane); else k_head_any.
int head_train(bool fixed, int kind, const void* h4, const float* w5, const float* b5, const float* wide, const float* wprod, int F,
               const float* wide_bias, const float* label, int64_t B, int K5, float dscale, float dh_scale, float* logit, float* dlogit,
               void* dh4, float* dw5, float* db4, float* db5, float* dwide_b, float* loss, void* ws, size_t ws_bytes, void* stream) {
    HeadGeom g;
    const int rc = head_check(HEAD_TRAIN | (fixed ? HEAD_POW2 : 0), kind, h4, w5, b5, wide, wprod, F, wide_bias, label, B, K5, dh_scale, logit,
                              dlogit && dh4 && dw5 && db4 && db5, dh4, loss, ws, ws_bytes, &g);
    if (rc != MREC_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    head_dispatch(kind, g.NC, [&](auto k, auto n) {
        constexpr int KIND = decltype(k)::value, NC = decltype(n)::value;
        if (fixed)
            k_head_fwd_bwd<KIND><<<g.nb, MB, 0, st>>>((const uint4*)h4, w5, b5, wide, label, B, g.G, g.rows_per_block, dscale, logit, dlogit,
                                                      (uint4*)dh4, (float*)ws, wprod, F, wide_bias, dh_scale);
        else
            k_head_any<KIND, NC><<<g.nb, MB, 0, st>>>((const uint4*)h4, w5, b5, wide, label, B, g.C, g.G, g.rows_per_block, dscale, logit,
                                                      dlogit, (uint4*)dh4, (float*)ws, wprod, F, wide_bias, dh_scale);
    });
    k_head_finish<<<(unsigned)mrec_cdiv(2 * K5 + 2, 32), MB, 0, st>>>((const float*)ws, g.nb, K5, 1.0f / (float)B, dw5, db4, db5, loss, dwide_b);
    MREC_LAUNCH_CHECK();
    return MREC_OK;
}

}  // namespace

MREC_API int mrec_head_workspace_bytes(int64_t B, int32_t K5, size_t* out) {
    if (!out || B < 0 || K5 <= 0) return MREC_EINVAL;
    *out = (size_t)512 * (2 * K5 + 2) * sizeof(float) + 256;
    return MREC_OK;
}

MREC_API int mrec_head_fwd_bwd_bf16(const uint16_t* h4, const float* w5, const float* b5, const float* wide,
                                    const float* label, int64_t B, int32_t K5, float dscale, float dh_scale, float* logit,
                                    float* dlogit, uint16_t* dh4, float* dw5, float* db4, float* db5, float* loss,
                                    void* ws, size_t ws_bytes, void* stream) {
    return head_train(true, 0, h4, w5, b5, wide, nullptr, 0, nullptr, label, B, K5, dscale, dh_scale, logit, dlogit, dh4, dw5, db4, db5, nullptr, loss, ws, ws_bytes, stream);
}

MREC_API int mrec_head_fwd_bwd_f16(const uint16_t* h4, const float* w5, const float* b5, const float* wide,
                                   const float* label, int64_t B, int32_t K5, float dscale, float dh_scale, float* logit,
                                   float* dlogit, uint16_t* dh4, float* dw5, float* db4, float* db5, float* loss,
                                   void* ws, size_t ws_bytes, void* stream) {
    return head_train(true, 1, h4, w5, b5, wide, nullptr, 0, nullptr, label, B, K5, dscale, dh_scale, logit, dlogit, dh4, dw5, db4, db5, nullptr, loss, ws, ws_bytes, stream);
}

/* fp32 activations (the fp32 net: mlp_dtype = fp32 of the Wide&Deep / DeepFM engines): h4, dh4 float32 [B, K5] */
MREC_API int mrec_head_fwd_bwd_f32(const float* h4, const float* w5, const float* b5, const float* wide,
                                   const float* label, int64_t B, int32_t K5, float dscale, float dh_scale, float* logit,
                                   float* dlogit, float* dh4, float* dw5, float* db4, float* db5, float* loss,
                                   void* ws, size_t ws_bytes, void* stream) {
    return head_train(true, 2, h4, w5, b5, wide, nullptr, 0, nullptr, label, B, K5, dscale, dh_scale, logit, dlogit, dh4, dw5, db4, db5, nullptr, loss, ws, ws_bytes, stream);
}

/* The same head with the wide branch given as per-field products [B, F] + the wide bias (see include/mrec.h). */
MREC_API int mrec_head_fwd_bwd_wide(int32_t f16, const uint16_t* h4, const float* w5, const float* b5, const float* wide_prod,
                                    int32_t F, const float* wide_bias, const float* label, int64_t B, int32_t K5, float dscale,
                                    float dh_scale, float* logit, float* dlogit, uint16_t* dh4, float* dw5, float* db4, float* db5, float* dwide_bias,
                                    float* loss, void* ws, size_t ws_bytes, void* stream) {
    return head_train(true, f16 != 0 ? 1 : 0, h4, w5, b5, nullptr, wide_prod, F, wide_bias, label, B, K5, dscale, dh_scale, logit, dlogit, dh4, dw5, db4, db5, dwide_bias, loss, ws, ws_bytes, stream);
}

/* The head at any K5 % 8 == 0, 8 <= K5 <= 2048 (k_head_any; see include/mrec.h). */
MREC_API int mrec_head_fwd_bwd_any(int32_t kind, const void* h4, const float* w5, const float* b5, const float* wide,
                                   const float* wide_prod, int32_t F, const float* wide_bias, const float* label, int64_t B, int32_t K5,
                                   float dscale, float dh_scale, float* logit, float* dlogit, void* dh4, float* dw5, float* db4, float* db5,
                                   float* dwide_bias, float* loss, void* ws, size_t ws_bytes, void* stream) {
    return head_train(false, kind, h4, w5, b5, wide, wide_prod, F, wide_bias, label, B, K5, dscale, dh_scale, logit, dlogit, dh4, dw5, db4, db5, dwide_bias, loss, ws, ws_bytes, stream);
}

/* The evaluation forward of the head at any K5 % 8 == 0, 8 <= K5 <= 2048 (k_head_predict; see include/mrec.h). */
MREC_API int mrec_head_predict_workspace_bytes(int64_t B, size_t* out) {
    if (!out || B < 0) return MREC_EINVAL;
    *out = (size_t)256 * sizeof(float) + 256;          // one loss partial a workgroup, at most 256 of them
    return MREC_OK;
}

MREC_API int mrec_head_predict(int32_t kind, const void* h4, const float* w5, const float* b5, const float* wide, const float* wide_prod,
                               int32_t F, const float* wide_bias, const float* label, int64_t B, int32_t K5, float* logit, float* prob,
                               float* loss, void* ws, size_t ws_bytes, void* stream) {
    HeadGeom g;
    const int rc = head_check(0, kind, h4, w5, b5, wide, wide_prod, F, wide_bias, label, B, K5, 1.0f, logit, prob != nullptr, nullptr, loss, ws,
                              ws_bytes, &g);
    if (rc != MREC_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    head_dispatch(kind, g.NC, [&](auto k, auto n) {
        k_head_predict<decltype(k)::value, decltype(n)::value><<<g.nb, MB, 0, st>>>(
            (const uint4*)h4, w5, b5, wide, label, B, g.C, g.G, g.rows_per_block, logit, prob, label ? (float*)ws : nullptr, wide_prod, F, wide_bias);
    });
    if (label) k_head_predict_finish<<<1, MB, 0, st>>>((const float*)ws, g.nb, 1.0f / (float)B, loss);
    MREC_LAUNCH_CHECK();
    return MREC_OK;
}

// ---- Dropout as a pass of its own (spec: mrec_dropout.h): the first DenseLayer's input (the looked-up rows) and the fp32 net --
namespace {
template <int KIND>      // 0: fp32, 1: bfloat16, 2: IEEE half
__global__ __launch_bounds__(256) void k_dropout(const void* __restrict__ x, int64_t ldx, void* __restrict__ y, int64_t ldy, int64_t M,
                                                 int W, DropArgs d) {
    const uint64_t key = drop_key(d);
    const int W4 = W >> 2;
    const int64_t nq = M * W4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nq; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / W4;
        const int c = (int)(i - r * W4) * 4;
        const uint64_t qd = drop_quad(key, d.row0 + r, W, c);
        float v[4];
        if (KIND == 0) {
            const float4 t = *(const float4*)((const float*)x + r * ldx + c);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
            const uint2 t = *(const uint2*)((const uint16_t*)x + r * ldx + c);
            const uint32_t b[4] = {t.x & 0xFFFFu, t.x >> 16, t.y & 0xFFFFu, t.y >> 16};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                v[j] = KIND == 1 ? __uint_as_float(b[j] << 16) : (float)__builtin_bit_cast(_Float16, (uint16_t)b[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = drop_keep(qd, j, d.thresh) ? v[j] * d.scale : 0.0f;
        if (KIND == 0) {
            *(float4*)((float*)y + r * ldy + c) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            uint32_t b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (KIND == 1) b[j] = f2bf(v[j]);
                else b[j] = __builtin_bit_cast(uint16_t, (_Float16)v[j]);
            }
            *(uint2*)((uint16_t*)y + r * ldy + c) = make_uint2(b[0] | (b[1] << 16), b[2] | (b[3] << 16));
        }
    }
}
__global__ __launch_bounds__(256) void k_dropout_mask(float* __restrict__ mask, int64_t ld, int64_t M, int W, DropArgs d) {
    const uint64_t key = drop_key(d);
    const int W4 = W >> 2;
    const int64_t nq = M * W4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nq; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / W4;
        const int c = (int)(i - r * W4) * 4;
        const uint64_t qd = d.thresh ? drop_quad(key, d.row0 + r, W, c) : 0ull;
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = d.thresh == 0 ? 1.0f : (drop_keep(qd, j, d.thresh) ? d.scale : 0.0f);
        *(float4*)(mask + r * ld + c) = make_float4(v[0], v[1], v[2], v[3]);
    }
}
}  // namespace

MREC_API int mrec_dropout(const void* x, int64_t ldx, void* y, int64_t ldy, int32_t kind, int64_t M, int32_t W,
                          const mrec_dropout_t* drop, void* stream) {
    if (M < 0 || W <= 0 || ldx < W || ldy < W || kind < 0 || kind > 2 || !drop) return MREC_EINVAL;
    DropArgs d;
    if (!drop_from(drop, W, &d)) return MREC_EINVAL;
    if (M == 0) return MREC_OK;
    if (!x || !y) return MREC_EINVAL;
    const int al = kind == 0 ? 15 : 7;
    if (ldx % 4 || ldy % 4 || (((uintptr_t)x | (uintptr_t)y) & al)) return MREC_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    if (d.thresh == 0) {             // keep_prob 1: the identity
        if (x != y) MREC_HIP_CHECK(hipMemcpy2DAsync(y, (size_t)ldy * (kind ? 2 : 4), x, (size_t)ldx * (kind ? 2 : 4),
                                                    (size_t)W * (kind ? 2 : 4), (size_t)M, hipMemcpyDeviceToDevice, st));
        return MREC_OK;
    }
    const int64_t nq = M * (W / 4);
    const unsigned g = (unsigned)(mrec_cdiv(nq, 256) < 8192 ? mrec_cdiv(nq, 256) : 8192);
    if (kind == 0) k_dropout<0><<<g, 256, 0, st>>>(x, ldx, y, ldy, M, W, d);
    else if (kind == 1) k_dropout<1><<<g, 256, 0, st>>>(x, ldx, y, ldy, M, W, d);
    else k_dropout<2><<<g, 256, 0, st>>>(x, ldx, y, ldy, M, W, d);
    MREC_LAUNCH_CHECK();
    return MREC_OK;
}

MREC_API int mrec_dropout_mask_f32(float* mask, int64_t ld, int64_t M, int32_t W, const mrec_dropout_t* drop, void* stream) {
    if (M < 0 || W <= 0 || ld < W || !drop) return MREC_EINVAL;
    DropArgs d;
    if (!drop_from(drop, W, &d)) return MREC_EINVAL;
    if (M == 0) return MREC_OK;
    if (!mask) return MREC_EINVAL;
    if (ld % 4 || (((uintptr_t)mask) & 15)) return MREC_EUNSUPPORTED;
    const int64_t nq = M * (W / 4);
    const unsigned g = (unsigned)(mrec_cdiv(nq, 256) < 8192 ? mrec_cdiv(nq, 256) : 8192);
    k_dropout_mask<<<g, 256, 0, (hipStream_t)stream>>>(mask, ld, M, W, d);
    MREC_LAUNCH_CHECK();
    return MREC_OK;
}
