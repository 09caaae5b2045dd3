// mrec_dense_optim.hip -- the dense (whole-tensor) optimizers, for gfx950: nn.Adam over a flat buffer (fp32 / bf16 gradient, bf16
// shadow, one FTRL element, fp32 gradient slabs), nn.Adam over a whole table with the loss's L2 term and with a Gather's row
// gradients, max_norm in front of it, the slab-segment sum and nn.FTRL.  HBM-bound streaming kernels: a thread owns a float4 (or an
// element) of p, m, v and walks the buffer with the grid's stride.
//
// Reference call sites: models/wide_deep/src/wide_and_deep.py:356-360,407-411,434-445; models/deep_and_cross/src/
// deep_and_cross.py:199,342-344; models/deepfm/src/deepfm.py:198,252-259,267.
#include <type_traits>

#include "mrec_common.h"
#include "mrec_optim.h"
#include "mrec_dense_adam.h"

namespace {

// Dense Adam over n elements.  GT = float or bf16 gradients (the GEMM that produced a weight gradient
// in a bf16 MLP writes bf16; widening on load is exact).  SH: also write the updated parameter, rounded
// to bf16, into a shadow buffer -- the operand copy the next forward's bf16 GEMMs read, so no separate
// cast pass over the weights is needed.
__device__ __forceinline__ float g_widen(float x) { return x; }
__device__ __forceinline__ float g_widen(uint16_t x) { return __uint_as_float(((unsigned)x) << 16); }

template <class GT, bool SH>
__global__ __launch_bounds__(256) void k_dense_adam(float* __restrict__ p, float* __restrict__ m,
                                                    float* __restrict__ v, const GT* __restrict__ g, int64_t n,
                                                    AdamH h, uint16_t* __restrict__ shadow, Ftrl1 f1,
                                                    const StepState* __restrict__ ss) {
    if (ss) h.lr_t = ss->lr_t;             // this step's bias-corrected step size from device memory (mrec_step_advance)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float pp = p[i], mm = m[i], vv = v[i];
        adam_or_ftrl(pp, mm, vv, g_widen(g[i]) * h.gscale, h, i == f1.idx, f1.h);
        p[i] = pp; m[i] = mm; v[i] = vv;
        if (SH) shadow[i] = f2bf(pp);
    }
}

template <bool SH>
__global__ __launch_bounds__(256) void k_dense_adam4(float4* __restrict__ p, float4* __restrict__ m,
                                                     float4* __restrict__ v, const float4* __restrict__ g,
                                                     int64_t n4, AdamH h, uint2* __restrict__ shadow, Ftrl1 f1,
                                                     const StepState* __restrict__ ss) {
    if (ss) h.lr_t = ss->lr_t;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 pp = p[i], mm = m[i], vv = v[i];
        const float4 gg = g[i];
        const int fq = (f1.idx >> 2) == i ? (int)(f1.idx & 3) : -1;
        adam_or_ftrl(pp.x, mm.x, vv.x, gg.x * h.gscale, h, fq == 0, f1.h);
        adam_or_ftrl(pp.y, mm.y, vv.y, gg.y * h.gscale, h, fq == 1, f1.h);
        adam_or_ftrl(pp.z, mm.z, vv.z, gg.z * h.gscale, h, fq == 2, f1.h);
        adam_or_ftrl(pp.w, mm.w, vv.w, gg.w * h.gscale, h, fq == 3, f1.h);
        p[i] = pp; m[i] = mm; v[i] = vv;
        if (SH) shadow[i] = make_uint2((unsigned)f2bf(pp.x) | ((unsigned)f2bf(pp.y) << 16),
                                       (unsigned)f2bf(pp.z) | ((unsigned)f2bf(pp.w) << 16));
    }
}

// Dense Adam whose gradient carries the L2 term of the loss: g_i = sums_i + l2s * p_i (l2s = l2_coef * sens: d/dp of
// l2_coef * sum(p^2) / 2 at the loss scale; NetWithLossClass.construct, wide_and_deep.py:356-360; deepfm.py:252-259), with the
// loss term's own by-product -- sum(p^2) BEFORE the update -- reduced in the same pass: per-thread fp64 partials, wave shuffle,
// LDS, one fp64 word per workgroup; k_sumsq_finish adds them in workgroup order.  Replaces three torch passes over the table
// (the product, the add onto the scattered sums, the sum of squares).
__global__ __launch_bounds__(256) void k_dense_adam4_l2(float4* __restrict__ p, float4* __restrict__ m, float4* __restrict__ v,
                                                        const float4* __restrict__ g, int64_t n4, AdamH h, float l2s,
                                                        double* __restrict__ partial, int tail) {
    __shared__ double red[4];
    double acc = 0.0;
    if (tail && blockIdx.x == 0 && threadIdx.x == 0) {          // the n % 4 elements behind the last whole float4 (DeepFM's [184 965, 1] table)
        float* ps = (float*)(p + n4); float* ms = (float*)(m + n4); float* vs = (float*)(v + n4);
        const float* gs = (const float*)(g + n4);
        for (int t = 0; t < tail; ++t) {
            float pp = ps[t], mm = ms[t], vv = vs[t], gg = gs[t];
            acc += (double)pp * pp;
            gg += l2s * pp;
            adam_elem(pp, mm, vv, gg * h.gscale, h);
            ps[t] = pp; ms[t] = mm; vs[t] = vv;
        }
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 pp = p[i], mm = m[i], vv = v[i];
        float4 gg = g[i];
        acc += (double)pp.x * pp.x + (double)pp.y * pp.y + (double)pp.z * pp.z + (double)pp.w * pp.w;
        gg.x += l2s * pp.x; gg.y += l2s * pp.y; gg.z += l2s * pp.z; gg.w += l2s * pp.w;       // product rounded, then added (no fma)
        adam_elem(pp.x, mm.x, vv.x, gg.x * h.gscale, h);
        adam_elem(pp.y, mm.y, vv.y, gg.y * h.gscale, h);
        adam_elem(pp.z, mm.z, vv.z, gg.z * h.gscale, h);
        adam_elem(pp.w, mm.w, vv.w, gg.w * h.gscale, h);
        p[i] = pp; m[i] = mm; v[i] = vv;
    }
    if (!partial) return;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_down(acc, d, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// One workgroup adds the per-workgroup partials in a FIXED order (thread t takes partials t, t + 256, ...; then a tree over the
// threads): the same bits every run.  (One thread walking all of them was a chain of ~2000 dependent loads: 110 us per table.)
__global__ __launch_bounds__(256) void k_sumsq_finish(const double* __restrict__ partial, int nb, double* __restrict__ out, int accumulate) {
    __shared__ double red[256];
    double s = 0.0;
    for (int b = threadIdx.x; b < nb; b += 256) s += partial[b];
    red[threadIdx.x] = s;
    __syncthreads();
#pragma unroll
    for (int d = 128; d > 0; d >>= 1) {
        if (threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = (accumulate ? *out : 0.0) + red[0];
}

// nn.Adam over a WHOLE table whose gradient is nonzero on the step's touched rows only (the bprop of a dense Gather:
// UnsortedSegmentSum into a [V, D] tensor, deep_and_cross.py:199,342-344; deepfm.py:198,267; wide_and_deep.py:434-437 with sparse False):
// the row sums stay where the segment-sum left them ([U, D], group order) and every row looks its group up in `row_group` (-1: no
// gradient) -- instead of zeroing a [V, D] gradient, scattering the sums into it and reading it back (three passes over the table's
// size per step).  VEC = 4: D % 4 == 0, a thread owns 4 columns of a row; VEC = 1: any D.  Same arithmetic, element for element, as
// k_dense_adam4_l2 on the scattered gradient.
template <int VEC>
__global__ __launch_bounds__(256) void k_dense_adam_rows_l2(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, int64_t V,
                                                            int D, const int* __restrict__ row_group, const float* __restrict__ sums,
                                                            AdamH h, float l2s, double* __restrict__ partial, const StepState* __restrict__ ss) {
    __shared__ double red[4];
    if (ss) h.lr_t = ss->lr_t;
    const int DV = D / VEC;
    const int64_t n = V * DV, stride = (int64_t)gridDim.x * 256;
    const int64_t sr = stride / DV;
    const int sc = (int)(stride - sr * DV);
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t r = i / DV;
    int c = (int)(i - r * DV);
    double acc = 0.0;
    for (; i < n; i += stride) {
        const int g = row_group[r];
        const int64_t e = (r * DV + c) * VEC;
        if (VEC == 4) {
            float4 pp = *(float4*)(p + e), mm = *(float4*)(m + e), vv = *(float4*)(v + e);
            float4 gg = g >= 0 ? *(const float4*)(sums + ((int64_t)g * DV + c) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            acc += (double)pp.x * pp.x + (double)pp.y * pp.y + (double)pp.z * pp.z + (double)pp.w * pp.w;
            gg.x += l2s * pp.x; gg.y += l2s * pp.y; gg.z += l2s * pp.z; gg.w += l2s * pp.w;
            adam_elem(pp.x, mm.x, vv.x, gg.x * h.gscale, h);
            adam_elem(pp.y, mm.y, vv.y, gg.y * h.gscale, h);
            adam_elem(pp.z, mm.z, vv.z, gg.z * h.gscale, h);
            adam_elem(pp.w, mm.w, vv.w, gg.w * h.gscale, h);
            *(float4*)(p + e) = pp; *(float4*)(m + e) = mm; *(float4*)(v + e) = vv;
        } else {
            float pp = p[e], mm = m[e], vv = v[e];
            float gg = g >= 0 ? sums[(int64_t)g * D + c] : 0.f;
            acc += (double)pp * pp;
            gg += l2s * pp;
            adam_elem(pp, mm, vv, gg * h.gscale, h);
            p[e] = pp; m[e] = mm; v[e] = vv;
        }
        r += sr; c += sc;
        if (c >= DV) { c -= DV; ++r; }
    }
    if (!partial) return;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_down(acc, d, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// row_group[uniq[g]] = g for the step's groups (row_group was set to -1 everywhere before; a negative / out-of-range row: no entry)
__global__ __launch_bounds__(256) void k_rows_to_groups(const int* __restrict__ uniq, const int64_t* __restrict__ n_uniq_dev, int64_t U, int64_t V,
                                                        int* __restrict__ row_group) {
    const int64_t n = n_uniq_dev ? min(U, *n_uniq_dev) : U;
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n; g += (int64_t)gridDim.x * 256) {
        const int r = uniq[g];
        if (r >= 0 && r < V) row_group[r] = (int)g;
    }
}

// max_norm in front of a DENSE optimizer (the bprop of mrec_gather_rows_clip_* where nn.Adam sweeps the whole table: DeepFM, Deep&Cross):
// every occurrence of a row shares the row's Jacobian, so the step's group sums [U, D] (mrec_segment_sum_*) go through it once per
// group, in place, before the optimizer reads them -- G <- (c / n) (G - (x.G / n^2) x) where n = |x| > c, x = p[uniq[g]] at its
// pre-update value (mrec_clip_jacobian: the sparse apply's arithmetic and the lookup's decision, bit for bit).  The lookup's geometry:
// a lane-group of nd = D / 4 lanes holds a row, one float4 per lane, 64 / nd groups per wave.  A group past min(U, *n_uniq_dev)
// or whose row is outside [0, V) (the -1 of an un-admitted key) loads nothing and stores nothing; an unclipped group stores nothing
// either, so its sum stays bit for bit.  Whole lane-groups take or skip every branch together and every lane of a live wave reaches the
// butterfly (its partners are lanes of its own lane-group); the spare lanes behind the last group leave at the top: nobody reads them.
__global__ __launch_bounds__(256) void k_clip_group_sums(const float* __restrict__ p, int64_t V, int64_t ld, const int* __restrict__ uniq,
                                                         int64_t U, const int64_t* __restrict__ n_uniq_dev, float* __restrict__ sums, int D,
                                                         RowGeom gm, float c) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane / gm.lpr, sub = lane - grp * gm.lpr;
    if (grp >= gm.G) return;
    int64_t n = U;
    if (n_uniq_dev) { const int64_t x = *n_uniq_dev; n = x < 0 ? 0 : (x < U ? x : U); }
    const int64_t g = ((int64_t)blockIdx.x * 4 + wave) * gm.G + grp;
    const int64_t r = g < n ? (int64_t)uniq[g] : -1;
    const bool ok = r >= 0 && r < V;
    const int col = sub * 4;
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f), G = x;
    if (ok) {
        x = *(const float4*)(p + r * ld + col);
        G = *(const float4*)(sums + g * D + col);
    }
    const bool hit = mrec_clip_jacobian(G, x, c, sub, gm.lpr, lane - sub);      // (a zero row -- every skipped group -- is never clipped)
    if (ok && hit) *(float4*)(sums + g * D + col) = G;
}

template <bool SH>
__global__ __launch_bounds__(256) void k_dense_adam4_g16(float4* __restrict__ p, float4* __restrict__ m,
                                                         float4* __restrict__ v, const uint2* __restrict__ g,
                                                         int64_t n4, AdamH h, uint2* __restrict__ shadow,
                                                         const StepState* __restrict__ ss) {
    if (ss) h.lr_t = ss->lr_t;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        float4 pp = p[i], mm = m[i], vv = v[i];
        const uint2 u = g[i];
        adam_elem(pp.x, mm.x, vv.x, __uint_as_float(u.x << 16) * h.gscale, h);
        adam_elem(pp.y, mm.y, vv.y, __uint_as_float(u.x & 0xFFFF0000u) * h.gscale, h);
        adam_elem(pp.z, mm.z, vv.z, __uint_as_float(u.y << 16) * h.gscale, h);
        adam_elem(pp.w, mm.w, vv.w, __uint_as_float(u.y & 0xFFFF0000u) * h.gscale, h);
        p[i] = pp; m[i] = mm; v[i] = vv;
        if (SH) shadow[i] = make_uint2((unsigned)f2bf(pp.x) | ((unsigned)f2bf(pp.y) << 16),
                                       (unsigned)f2bf(pp.z) | ((unsigned)f2bf(pp.w) << 16));
    }
}

// g[start_q + e] = sum over s of slabs_q[s * len_q + e], slab order, for every segment q in ONE launch (the data-parallel
// all-reduce needs the summed gradient; 7 launches of a one-segment kernel whose bias segments had 256 lanes of work and 64
// dependent loads each took 210 us).  A thread owns one float4 of one segment; 8 slab loads in flight.
__global__ __launch_bounds__(256) void k_sum_slab_segments(float4* __restrict__ g, SlabSegs sg, int64_t total4) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total4; t += (int64_t)gridDim.x * 256) {
        int k = 0;
        int64_t off = t;
        while (k < sg.n - 1 && off >= sg.len4[k]) { off -= sg.len4[k]; ++k; }
        const float4* src = sg.part[k] + off;
        const int S = sg.S[k];
        const int64_t L = sg.len4[k];
        float4 gg = src[0];
        for (int s0 = 1; s0 < S; s0 += 8) {
            float4 u[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) u[q] = (s0 + q < S) ? src[(int64_t)(s0 + q) * L] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (s0 + q < S) { gg.x += u[q].x; gg.y += u[q].y; gg.z += u[q].z; gg.w += u[q].w; }
        }
        g[sg.start4[k] + off] = gg;
    }
}

__global__ __launch_bounds__(256) void k_dense_ftrl(float* __restrict__ w, float* __restrict__ a,
                                                    float* __restrict__ lin, const float* __restrict__ g,
                                                    int64_t n, FtrlH h) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float ww = w[i], aa = a[i], ll = lin[i];
        ftrl_elem(ww, aa, ll, g[i] * h.gscale, h);
        w[i] = ww; a[i] = aa; lin[i] = ll;
    }
}

// shadow or none -> <SH>, decided in ONE place (as by_key / by_grad of mrec_apply.hip): f gets std::true_type / std::false_type
template <class F>
void by_shadow(const void* shadow, F&& f) {
    if (shadow) f(std::true_type{});
    else f(std::false_type{});
}

}  // namespace

static int dense_adam_launch(float* p, float* m, float* v, const void* g, int g_bf16, uint16_t* shadow, int64_t n,
                             float lr, float b1, float b2, float eps, float b1_pow, float b2_pow, float grad_scale,
                             int nesterov, void* stream, const mrec_ftrl1_t* one = nullptr, const void* step_state = nullptr) {
    if (n < 0) return MREC_EINVAL;
    Ftrl1 f1;
    if (int rc = ftrl1_from(one, n, grad_scale, &f1)) return rc;
    if (f1.idx >= 0 && g_bf16) return MREC_EUNSUPPORTED;
    if (n == 0) return MREC_OK;
    if (!p || !m || !v || !g) return MREC_EINVAL;
    const AdamH h = adam_hyper(lr, b1, b2, eps, b1_pow, b2_pow, grad_scale, nesterov);
    const StepState* ss = (const StepState*)step_state;
    hipStream_t st = (hipStream_t)stream;
    const bool al = al16(p) && al16(m) && al16(v) && ((((uintptr_t)g) & (g_bf16 ? 7 : 15)) == 0) &&
                    (!shadow || ((((uintptr_t)shadow) & 7) == 0));
    const int64_t n4 = al ? n / 4 : 0;
    if (n4 > 0) {
        const unsigned gr = stream_grid(n4);
        by_shadow(shadow, [&](auto with) {
            constexpr bool SH = decltype(with)::value;
            if (g_bf16) k_dense_adam4_g16<SH><<<gr, 256, 0, st>>>((float4*)p, (float4*)m, (float4*)v, (const uint2*)g, n4, h, (uint2*)shadow, ss);
            else k_dense_adam4<SH><<<gr, 256, 0, st>>>((float4*)p, (float4*)m, (float4*)v, (const float4*)g, n4, h, (uint2*)shadow, f1, ss);
        });
    }
    const int64_t done = n4 * 4, rem = n - done;
    if (rem > 0) {
        const unsigned gr = stream_grid(rem);
        uint16_t* sh = shadow ? shadow + done : nullptr;
        Ftrl1 fr = f1;
        fr.idx = f1.idx >= done ? f1.idx - done : -1;
        by_shadow(sh, [&](auto with) {
            constexpr bool SH = decltype(with)::value;
            if (g_bf16) k_dense_adam<uint16_t, SH><<<gr, 256, 0, st>>>(p + done, m + done, v + done, (const uint16_t*)g + done, rem, h, sh, fr, ss);
            else k_dense_adam<float, SH><<<gr, 256, 0, st>>>(p + done, m + done, v + done, (const float*)g + done, rem, h, sh, fr, ss);
        });
    }
    MREC_LAUNCH_CHECK();
    return MREC_OK;
}

MREC_API int mrec_dense_adam_f32(float* p, float* m, float* v, const float* g, int64_t n, float lr, float b1,
                                 float b2, float eps, float b1_pow, float b2_pow, float grad_scale, int nesterov,
                                 void* stream) {
    return dense_adam_launch(p, m, v, g, 0, nullptr, n, lr, b1, b2, eps, b1_pow, b2_pow, grad_scale, nesterov, stream);
}

MREC_API int mrec_dense_adam_ex_f32(float* p, float* m, float* v, const void* g, int g_is_bf16, uint16_t* shadow_bf16,
                                    int64_t n, float lr, float b1, float b2, float eps, float b1_pow, float b2_pow,
                                    float grad_scale, int nesterov, void* stream) {
    return dense_adam_launch(p, m, v, g, g_is_bf16, shadow_bf16, n, lr, b1, b2, eps, b1_pow, b2_pow, grad_scale, nesterov,
                             stream);
}

MREC_API int mrec_dense_adam_step_f32(float* p, float* m, float* v, const void* g, int g_is_bf16, uint16_t* shadow_bf16,
                                      int64_t n, float lr, float b1, float b2, float eps, float b1_pow, float b2_pow,
                                      float grad_scale, int nesterov, const void* step_state, void* stream) {
    return dense_adam_launch(p, m, v, g, g_is_bf16, shadow_bf16, n, lr, b1, b2, eps, b1_pow, b2_pow, grad_scale, nesterov,
                             stream, nullptr, step_state);
}

MREC_API int mrec_dense_adam_l2_workspace_bytes(int64_t n, size_t* out) {
    if (!out || n < 0) return MREC_EINVAL;
    *out = (size_t)stream_grid(n / 4 > 0 ? n / 4 : 1) * sizeof(double) + 256;
    return MREC_OK;
}

MREC_API int mrec_dense_adam_l2_f32(float* p, float* m, float* v, const float* g, int64_t n, float lr, float b1, float b2, float eps,
                                    float b1_pow, float b2_pow, float grad_scale, int nesterov, float l2_scaled, double* sumsq,
                                    int sumsq_accumulate, void* ws, size_t ws_bytes, void* stream) {
    if (n < 0) return MREC_EINVAL;
    if (n == 0) return MREC_OK;
    if (!p || !m || !v || !g) return MREC_EINVAL;
    if (!al16(p) || !al16(m) || !al16(v) || !al16(g)) return MREC_EUNSUPPORTED;
    const int64_t n4 = n / 4;
    const unsigned gr = stream_grid(n4 > 0 ? n4 : 1);
    double* partial = nullptr;
    if (sumsq) {
        MrecArena a(ws, ws_bytes);
        partial = a.take<double>(gr);
        if (!a.ok || !partial) return MREC_EWORKSPACE;
    }
    const AdamH h = adam_hyper(lr, b1, b2, eps, b1_pow, b2_pow, grad_scale, nesterov);
    hipStream_t st = (hipStream_t)stream;
    k_dense_adam4_l2<<<gr, 256, 0, st>>>((float4*)p, (float4*)m, (float4*)v, (const float4*)g, n4, h, l2_scaled, partial, (int)(n % 4));
    if (sumsq) k_sumsq_finish<<<1, 256, 0, st>>>(partial, (int)gr, sumsq, sumsq_accumulate);
    MREC_LAUNCH_CHECK();
    return MREC_OK;
}

MREC_API int mrec_dense_adam_rows_l2_workspace_bytes(int64_t V, int32_t D, size_t* out) {
    if (!out || V < 0 || D <= 0) return MREC_EINVAL;
    const int64_t items = V * (D % 4 == 0 ? D / 4 : D);
    *out = mrec_align_up((size_t)(V > 0 ? V : 1) * sizeof(int), 256) + (size_t)stream_grid(items > 0 ? items : 1) * sizeof(double) + 512;
    return MREC_OK;
}

MREC_API int mrec_dense_adam_rows_l2_f32(float* p, float* m, float* v, int64_t V, int32_t D, const int32_t* uniq_rows, int64_t U,
                                         const int64_t* n_uniq_dev, const float* sums, float lr, float b1, float b2, float eps, float b1_pow,
                                         float b2_pow, float grad_scale, int nesterov, float l2_scaled, double* sumsq, int sumsq_accumulate,
                                         const void* step_state, void* ws, size_t ws_bytes, void* stream) {
    if (V < 0 || D <= 0 || U < 0) return MREC_EINVAL;
    if (V == 0) return MREC_OK;
    if (!p || !m || !v || !ws || (U > 0 && (!uniq_rows || !sums))) return MREC_EINVAL;
    const bool v4 = D % 4 == 0;
    if (v4 && (!al16(p) || !al16(m) || !al16(v) || (sums && !al16(sums)))) return MREC_EUNSUPPORTED;
    if (V * (int64_t)D >= (int64_t(1) << 40)) return MREC_EUNSUPPORTED;
    const int64_t items = V * (v4 ? D / 4 : D);
    const unsigned gr = stream_grid(items);
    MrecArena a(ws, ws_bytes);
    int* row_group = a.take<int>(V);
    double* partial = sumsq ? a.take<double>(gr) : nullptr;
    if (!a.ok || !row_group || (sumsq && !partial)) return MREC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    MREC_HIP_CHECK(hipMemsetAsync(row_group, 0xFF, (size_t)V * sizeof(int), st));          // -1 everywhere
    if (U > 0) k_rows_to_groups<<<stream_grid(U), 256, 0, st>>>(uniq_rows, n_uniq_dev, U, V, row_group);
    const AdamH h = adam_hyper(lr, b1, b2, eps, b1_pow, b2_pow, grad_scale, nesterov);
    if (v4) k_dense_adam_rows_l2<4><<<gr, 256, 0, st>>>(p, m, v, V, D, row_group, sums, h, l2_scaled, partial, (const StepState*)step_state);
    else k_dense_adam_rows_l2<1><<<gr, 256, 0, st>>>(p, m, v, V, D, row_group, sums, h, l2_scaled, partial, (const StepState*)step_state);
    if (sumsq) k_sumsq_finish<<<1, 256, 0, st>>>(partial, (int)gr, sumsq, sumsq_accumulate);
    MREC_LAUNCH_CHECK();
    return MREC_OK;
}

/* max_norm in front of a dense optimizer (see include/mrec.h): one launch, no workspace; everything is checked before it. */
MREC_API int mrec_clip_group_sums_f32(const float* p, int64_t V, int64_t ld, int32_t D, const int32_t* uniq_rows, int64_t U,
                                      const int64_t* n_uniq_dev, float* sums, float max_norm, void* stream) {
    const int rc = clip_check(max_norm, D, 256);
    if (rc != MREC_OK) return rc;
    if (V < 0 || U < 0 || ld < D) return MREC_EINVAL;
    if (!p || !uniq_rows || !sums) return MREC_EINVAL;
    if (ld % 4 || !al16(p) || !al16(sums)) return MREC_EUNSUPPORTED;
    RowGeom gm{D / 4, 64 / (D / 4)};
    const int64_t blocks = mrec_cdiv(U, (int64_t)4 * gm.G);
    if (blocks > 0x7FFFFFFF) return MREC_EUNSUPPORTED;
    if (U == 0 || V == 0) return MREC_OK;
    k_clip_group_sums<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(p, V, ld, uniq_rows, U, n_uniq_dev, sums, D, gm, max_norm);
    MREC_LAUNCH_CHECK();
    return MREC_OK;
}

MREC_API int mrec_dense_adam_one_ftrl_f32(float* p, float* m, float* v, const float* g, int64_t n, float lr, float b1, float b2,
                                          float eps, float b1_pow, float b2_pow, float grad_scale, int nesterov,
                                          const mrec_ftrl1_t* one_ftrl, void* stream) {
    return dense_adam_launch(p, m, v, g, 0, nullptr, n, lr, b1, b2, eps, b1_pow, b2_pow, grad_scale, nesterov, stream, one_ftrl);
}

static int dense_adam_slabs_launch(float* p, float* m, float* v, const float* g, void* shadow16, int shadow_kind,
                                   int64_t n, int32_t nseg, const float* const* slabs, const int64_t* starts,
                                   const int64_t* lens, const int32_t* splits, float lr, float b1, float b2, float eps,
                                   float b1_pow, float b2_pow, float grad_scale, int nesterov, void* step_state,
                                   const mrec_ftrl1_t* one, void* stream) {
    if (n < 0 || nseg < 0 || nseg > 16 || shadow_kind < 0 || shadow_kind > 2) return MREC_EINVAL;
    Ftrl1 f1;
    if (int rc = ftrl1_from(one, n, grad_scale, &f1)) return rc;
    const StepState* ss = (const StepState*)step_state;
    if (n == 0) return MREC_OK;
    if (!p || !m || !v || !g || (nseg > 0 && (!slabs || !starts || !lens || !splits)) || (shadow_kind && !shadow16))
        return MREC_EINVAL;
    if (n % 4 || !al16(p) || !al16(m) || !al16(v) || !al16(g) || (shadow16 && (((uintptr_t)shadow16) & 7)))
        return MREC_EUNSUPPORTED;
    SlabSegs sg;
    if (int rc = slab_segs_from(nseg, slabs, starts, lens, splits, n, sg, nullptr)) return rc;
    const AdamH h = adam_hyper(lr, b1, b2, eps, b1_pow, b2_pow, grad_scale, nesterov);
    const int64_t n4 = n / 4;
    hipStream_t st = (hipStream_t)stream;
    const unsigned gr = stream_grid(n4);
    if (shadow_kind == 1) k_dense_adam4_slabs<1><<<gr, 256, 0, st>>>((float4*)p, (float4*)m, (float4*)v, (const float4*)g, n4, h, (uint2*)shadow16, sg, ss, f1);
    else if (shadow_kind == 2) k_dense_adam4_slabs<2><<<gr, 256, 0, st>>>((float4*)p, (float4*)m, (float4*)v, (const float4*)g, n4, h, (uint2*)shadow16, sg, ss, f1);
    else k_dense_adam4_slabs<0><<<gr, 256, 0, st>>>((float4*)p, (float4*)m, (float4*)v, (const float4*)g, n4, h, nullptr, sg, ss, f1);
    MREC_LAUNCH_CHECK();
    return MREC_OK;
}

MREC_API int mrec_dense_adam_slabs_f32(float* p, float* m, float* v, const float* g, void* shadow16, int shadow_kind,
                                       int64_t n, int32_t nseg, const float* const* slabs, const int64_t* starts,
                                       const int64_t* lens, const int32_t* splits, float lr, float b1, float b2, float eps,
                                       float b1_pow, float b2_pow, float grad_scale, int nesterov, void* step_state,
                                       void* stream) {
    return dense_adam_slabs_launch(p, m, v, g, shadow16, shadow_kind, n, nseg, slabs, starts, lens, splits, lr, b1, b2, eps, b1_pow,
                                   b2_pow, grad_scale, nesterov, step_state, nullptr, stream);
}

MREC_API int mrec_dense_adam_slabs_one_ftrl_f32(float* p, float* m, float* v, const float* g, void* shadow16, int shadow_kind,
                                                int64_t n, int32_t nseg, const float* const* slabs, const int64_t* starts,
                                                const int64_t* lens, const int32_t* splits, float lr, float b1, float b2, float eps,
                                                float b1_pow, float b2_pow, float grad_scale, int nesterov, void* step_state,
                                                const mrec_ftrl1_t* one_ftrl, void* stream) {
    return dense_adam_slabs_launch(p, m, v, g, shadow16, shadow_kind, n, nseg, slabs, starts, lens, splits, lr, b1, b2, eps, b1_pow,
                                   b2_pow, grad_scale, nesterov, step_state, one_ftrl, stream);
}

MREC_API int mrec_dense_sum_slab_segments_f32(float* g, int64_t n, int32_t nseg, const float* const* slabs, const int64_t* starts,
                                              const int64_t* lens, const int32_t* splits, void* stream) {
    if (n < 0 || nseg < 0 || nseg > 16) return MREC_EINVAL;
    if (nseg == 0) return MREC_OK;
    if (!g || !slabs || !starts || !lens || !splits) return MREC_EINVAL;
    if (!al16(g)) return MREC_EUNSUPPORTED;
    SlabSegs sg;
    int64_t total4 = 0;
    if (int rc = slab_segs_from(nseg, slabs, starts, lens, splits, n, sg, &total4)) return rc;
    k_sum_slab_segments<<<stream_grid(total4), 256, 0, (hipStream_t)stream>>>((float4*)g, sg, total4);
    MREC_LAUNCH_CHECK();
    return MREC_OK;
}

MREC_API int mrec_dense_ftrl_f32(float* var, float* accum, float* linear, const float* g, int64_t n, float lr,
                                 float l1, float l2, float lr_power, float grad_scale, void* stream) {
    if (n < 0) return MREC_EINVAL;
    if (n == 0) return MREC_OK;
    if (!var || !accum || !linear || !g) return MREC_EINVAL;
    FtrlH h{lr, l1, l2, lr_power, grad_scale};
    k_dense_ftrl<<<stream_grid(n), 256, 0, (hipStream_t)stream>>>(var, accum, linear, g, n, h);
    MREC_LAUNCH_CHECK();
    return MREC_OK;
}

