// mrec_gemm_fp8.hip -- the hidden DenseLayers of a serving predictor on the gfx950 8-bit-float matrix instruction
// (v_mfma_f32_16x16x128_f8f6f4, both operands OCP e4m3, fp32 accumulation, no block scales), and the row quantizer that
// freezes their weights.  Numeric contract: include/mrec.h, "FP8 hidden layers".
//
//   k_fp8_quantize_rows   W^T [N, K] (fp32 / 16-bit) -> e4m3 codes [N, ldq] (K-contiguous, zero past K) + one fp32 scale per row
//   k_gemm_fp8_fwd        Y[M, N] = epi(A[M, K] . Wq[N, K]^T): A as 16-bit rows converted WHILE STAGED (A16) or as e4m3 codes (A8);
//                         epi: y = fma(acc, sa * sw[n], bias[n]), ReLU, one rounding to 16 bits or to e4m3 codes for the next layer
//
// One workgroup = 8 waves (512 threads) owns a 128 (M) x 256 (N) output tile: 512 workgroups at (16384, ., 1024) and 256 at
// (16384, ., 512), at least one per CU of the 256 either way.  Wave (wr, wc) = (w >> 2, w & 3) owns 64 x 64 of it as 4 x 4
// accumulators of the 16x16x128 instruction (64 accumulator registers); the reduction is cut in K-tiles of 128 codes = ONE
// instruction deep, so a K-tile is 16 MFMAs per wave over 4 + 4 fragments of 32 bytes a lane.
//
// LDS image: a K-tile is 128 + 256 rows of 128 bytes (16 + 32 KB), two buffers = 96 KB.  A row's eight 16-byte chunks are stored at
// chunk ^ ((row >> 1) & 7): the sixteen rows a ds_read_b128 of a fragment touches (lanes 0-15: rows r, same logical chunk) fall on
// sixteen different 16-byte columns of the 256-byte bank line.  A lane's fragment for the instruction is the 32 consecutive k
// 32 (l >> 4) .. + 31 of row l & 15 (CDNA4 ISA, "MFMA with 8-bit operands": 8 registers a lane): logical chunks 2 (l >> 4) and
// 2 (l >> 4) + 1, two ds_read_b128.  Accumulators hold C transposed (the instruction's A = the W fragment, B = the activation
// fragment), so a lane owns 4 consecutive n of one m: 8-byte (16-bit) or 4-byte (e4m3) stores.
//
// Staging.  Codes (W always, A where it is A8) go global -> LDS by LDS-DMA, 16 bytes a lane, one wave instruction = 8 rows; the DMA
// writes lane-linear, so the swizzle is applied to the per-lane SOURCE address.  A16 cannot: its rows go global -> registers (four
// 16-byte buffer loads a thread = 32 elements) -> widen -> * inv_sa -> clamp +-448 -> v_cvt_pk_fp8_f32 -> two ds_write_b128, which
// is what saves layer 0 a separate cast pass over its input.  Rows past M / N and k past K are zero-filled by pointing the lane's
// load past the buffer (range check: nothing is fetched); the weight's own K tail needs no guard beyond its 16-byte chunk because
// the quantizer writes zero codes there.
//
// Overlap.  Double buffered, ONE barrier a K-tile: at the top of K-tile t every wave waits for its own staging of t (vmcnt(0),
// lgkmcnt(0)) and meets the barrier -- tile t has landed, and buffer (t + 1) & 1 is no longer read by anybody.  It then issues the
// whole staging of tile t + 1 (A16: the register loads first, so that the wait in front of their conversion leaves the DMA of W in
// flight: a counted vmcnt, placed by the compiler), reads its eight fragments of tile t, runs the 16 MFMAs, and only then converts
// and writes the A registers of t + 1.  Global latency is hidden behind a whole K-tile of MFMAs; the conversion of one wave runs
// beside the MFMAs of the other wave of its SIMD (2 waves a SIMD).  No phases inside a K-tile and no staggered wave rows, as
// mrec_gemm.h has them: measured first, tuned later ("FP8 hidden layers").
#include "mrec_common.h"

namespace f8g {

typedef int i32x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

#define F8_LDS __attribute__((address_space(3)))

constexpr int kThreads = 512;
constexpr int BM = 128, BN = 256, BK = 128;           // tile; BK in codes = bytes
constexpr int kABytes = BM * BK, kBuf = (BM + BN) * BK, kLds = 2 * kBuf;
constexpr uint32_t kOob = 0x80000000u;                // voffset beyond any buffer: the load is dropped (zero fill)

enum { KIND_BF16 = MREC_FP8_KIND_BF16, KIND_F16 = MREC_FP8_KIND_F16, KIND_E4M3 = MREC_FP8_KIND_E4M3 };

struct Args {
    const void* A;
    const void* W;
    void* Y;
    const float* sw;       // [N] per-channel weight scales
    const float* bias;     // [N] fp32, nullable
    int64_t lda, ldq, ldy; // row strides in elements
    int M, N, K;
    int nTm, nTn;
    float sa, inv_sa, inv_so;
    int relu;
};

template <int KIND> __device__ __forceinline__ float widen(uint32_t bits16);
template <> __device__ __forceinline__ float widen<KIND_BF16>(uint32_t bits16) { return __uint_as_float(bits16 << 16); }
template <> __device__ __forceinline__ float widen<KIND_F16>(uint32_t bits16) { return (float)__builtin_bit_cast(_Float16, (uint16_t)bits16); }

// the rule of mrec.h: e4m3_rne(clamp(v, -448, 448)), four values -> four codes in ascending byte order
__device__ __forceinline__ float clamp448(float v) { return __builtin_amdgcn_fmed3f(v, -448.0f, 448.0f); }
__device__ __forceinline__ uint32_t codes4(float v0, float v1, float v2, float v3) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(clamp448(v0), clamp448(v1), 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(clamp448(v2), clamp448(v3), w, true);
    return (uint32_t)w;
}

template <int KIND> __device__ __forceinline__ uint32_t pack16(float lo, float hi);
template <> __device__ __forceinline__ uint32_t pack16<KIND_BF16>(float lo, float hi) {
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    bf16x2_t v = {(__bf16)lo, (__bf16)hi};
    return __builtin_bit_cast(uint32_t, v);
}
template <> __device__ __forceinline__ uint32_t pack16<KIND_F16>(float lo, float hi) {
    typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
    f16x2_t v = {(_Float16)lo, (_Float16)hi};
    return __builtin_bit_cast(uint32_t, v);
}

// AK: the kind of A (KIND_BF16 / KIND_F16: converted while staged; KIND_E4M3: codes); OK: the kind of Y
template <int AK, int OK>
__global__ __launch_bounds__(kThreads, 2) void k_gemm_fp8_fwd(const Args a) {
    __shared__ __attribute__((aligned(1024))) char smem_[kLds];
    F8_LDS char* const smem = (F8_LDS char*)smem_;
    constexpr bool A16 = AK != KIND_E4M3;
    const int tid = threadIdx.x, l = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = w >> 2, wc = w & 3;

    // workgroup -> (tn, tm): neighbours in the remapped order share an XCD, whose L2 then serves the activation rows they share
    // (the remap of mrec_gemm.h: bijective for any grid size)
    int tn, tm;
    {
        const int nblk = (int)gridDim.x, bid = (int)blockIdx.x;
        const int q8 = nblk >> 3, r8 = nblk & 7, xcd = bid & 7;
        const int swz = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (bid >> 3);
        tn = swz % a.nTn;
        tm = swz / a.nTn;
    }
    const int m0 = tm * BM, n0 = tn * BN;
    const int T = (a.K + BK - 1) / BK;
    const int Kw = (a.K + 15) & ~15;                  // the weight's rows hold zero codes from K to here (at least)

    const __amdgpu_buffer_rsrc_t rA = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.A), 0, (int)((int64_t)a.M * a.lda * (A16 ? 2 : 1)), 0x00020000);
    const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.W), 0, (int)((int64_t)a.N * a.ldq), 0x00020000);

    // ---- LDS-DMA lanes: instruction i of a piece fills rows 8 i .. 8 i + 7; lane l writes row 8 i + (l >> 3), physical chunk l & 7,
    // which holds the logical chunk (l & 7) ^ ((row >> 1) & 7).  W: 4 instructions a wave, A8: 2.
    uint32_t voffW[4], voffA8[2];
    int kcW[4], kcA8[2];                              // the lane's k offset inside the K-tile, per instruction
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int row = 8 * (w * 4 + e) + (l >> 3);
        kcW[e] = 16 * ((l & 7) ^ ((row >> 1) & 7));
        voffW[e] = n0 + row < a.N ? (uint32_t)((int64_t)(n0 + row) * a.ldq + kcW[e]) : kOob;
    }
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const int row = 8 * (w * 2 + e) + (l >> 3);
        kcA8[e] = 16 * ((l & 7) ^ ((row >> 1) & 7));
        voffA8[e] = (!A16 && m0 + row < a.M) ? (uint32_t)((int64_t)(m0 + row) * a.lda + kcA8[e]) : kOob;
    }
    // ---- A16 lanes: thread -> row tid >> 2, k 32 (tid & 3) .. + 31 of the K-tile: four loads of 8 elements
    const int arow = tid >> 2, aq = tid & 3;
    const uint32_t voffA16 = (A16 && m0 + arow < a.M) ? (uint32_t)(((int64_t)(m0 + arow) * a.lda + 32 * aq) * 2) : kOob;
    const uint32_t awr0 = (uint32_t)(arow * 128 + 16 * ((2 * aq) ^ ((arow >> 1) & 7)));
    const uint32_t awr1 = (uint32_t)(arow * 128 + 16 * ((2 * aq + 1) ^ ((arow >> 1) & 7)));
    u32x4_t areg[4];

    auto stage_codes = [&](int t, int buf) {
        const int k0 = t * BK;
        F8_LDS char* const dA = smem + buf * kBuf, * const dW = dA + kABytes;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (F8_LDS void*)(dW + (w * 4 + e) * 1024), 16,
                                                     k0 + kcW[e] < Kw ? voffW[e] : kOob, (uint32_t)k0, 0, 0);
        if constexpr (!A16) {
#pragma unroll
            for (int e = 0; e < 2; ++e)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rA, (F8_LDS void*)(dA + (w * 2 + e) * 1024), 16,
                                                         k0 + kcA8[e] < a.K ? voffA8[e] : kOob, (uint32_t)k0, 0, 0);
        }
    };
    auto load_a16 = [&](int t) {
        const int k0 = t * BK;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            areg[j] = __builtin_amdgcn_raw_buffer_load_b128(rA, k0 + 32 * aq + 8 * j < a.K ? voffA16 + 16 * j : kOob, (uint32_t)(k0 * 2), 0);
    };
    auto convert_a16 = [&](int buf) {
        if constexpr (A16) {
            uint32_t c[8];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const uint32_t p0 = areg[j][2 * h], p1 = areg[j][2 * h + 1];
                    c[2 * j + h] = codes4(widen<A16 ? AK : KIND_BF16>(p0 & 0xFFFFu) * a.inv_sa, widen<A16 ? AK : KIND_BF16>(p0 >> 16) * a.inv_sa,
                                          widen<A16 ? AK : KIND_BF16>(p1 & 0xFFFFu) * a.inv_sa, widen<A16 ? AK : KIND_BF16>(p1 >> 16) * a.inv_sa);
                }
            F8_LDS char* const dA = smem + buf * kBuf;
            *(F8_LDS u32x4_t*)(dA + awr0) = u32x4_t{c[0], c[1], c[2], c[3]};
            *(F8_LDS u32x4_t*)(dA + awr1) = u32x4_t{c[4], c[5], c[6], c[7]};
        }
    };

    // ---- fragment reads: row l & 15 of the 16-row block, logical chunks 2 g and 2 g + 1, g = l >> 4
    const int fr = l & 15, fg = l >> 4;
    const uint32_t rd0 = (uint32_t)(fr * 128 + 16 * ((2 * fg) ^ ((fr >> 1) & 7)));
    const uint32_t rd1 = (uint32_t)(fr * 128 + 16 * ((2 * fg + 1) ^ ((fr >> 1) & 7)));
    auto frag = [&](uint32_t base) -> i32x8_t {
        const u32x4_t lo = *(const F8_LDS u32x4_t*)(smem + base + rd0);
        const u32x4_t hi = *(const F8_LDS u32x4_t*)(smem + base + rd1);
        return i32x8_t{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
    };

    f32x4_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    // ---- prologue: K-tile 0 into buffer 0
    if constexpr (A16) load_a16(0);
    stage_codes(0, 0);
    convert_a16(0);

    for (int t = 0; t < T; ++t) {
        const int cur = t & 1;
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        const bool more = t + 1 < T;
        if (more) {
            if constexpr (A16) load_a16(t + 1);
            stage_codes(t + 1, cur ^ 1);
        }
        i32x8_t fA[4], fW[4];
        const uint32_t bA = (uint32_t)(cur * kBuf + wr * 64 * BK), bW = (uint32_t)(cur * kBuf + kABytes + wc * 64 * BK);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            fW[i] = frag(bW + i * 16 * BK);
            fA[i] = frag(bA + i * 16 * BK);
        }
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
                acc[mi][ni] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fW[ni], fA[mi], acc[mi][ni], 0, 0, 0, 0, 0, 0);
        if (more) convert_a16(cur ^ 1);
    }

    // ---- epilogue: lane owns m = m0 + wr * 64 + mi * 16 + (l & 15), n = n0 + wc * 64 + ni * 16 + 4 (l >> 4) + {0..3}
    const int mb = m0 + wr * 64 + (l & 15);
    const int nb = n0 + wc * 64 + 4 * (l >> 4);
    float tq[4][4], bq[4][4];
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int n = nb + ni * 16 + r;
            tq[ni][r] = n < a.N ? a.sa * a.sw[n] : 0.f;
            bq[ni][r] = (a.bias != nullptr && n < a.N) ? a.bias[n] : 0.f;
        }
#pragma unroll
    for (int mi = 0; mi < 4; ++mi) {
        const int m = mb + mi * 16;
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
            const int n = nb + ni * 16;
            if (m >= a.M || n >= a.N) continue;           // (N % 8 == 0: the lane's four columns are inside together)
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = __builtin_fmaf(acc[mi][ni][r], tq[ni][r], bq[ni][r]);
                if (a.relu) v[r] = v[r] > 0.f ? v[r] : 0.f;
            }
            if constexpr (OK == KIND_E4M3) {
                *(uint32_t*)((uint8_t*)a.Y + (int64_t)m * a.ldy + n) = codes4(v[0] * a.inv_so, v[1] * a.inv_so, v[2] * a.inv_so, v[3] * a.inv_so);
            } else {
                *(u32x2_t*)((uint16_t*)a.Y + (int64_t)m * a.ldy + n) =
                    u32x2_t{pack16<OK == KIND_E4M3 ? KIND_BF16 : OK>(v[0], v[1]), pack16<OK == KIND_E4M3 ? KIND_BF16 : OK>(v[2], v[3])};
            }
        }
    }
}

// ---- the row quantizer (cold path: run when a predictor is frozen).  One wave per row, four rows a workgroup.
template <class T> __device__ __forceinline__ float ldsrc(const T* p);
template <> __device__ __forceinline__ float ldsrc<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float ldsrc<bf16o_t>(const bf16o_t* p) { return widen<KIND_BF16>(p->v); }
template <> __device__ __forceinline__ float ldsrc<f16o_t>(const f16o_t* p) { return widen<KIND_F16>(p->v); }

template <class T>
__global__ __launch_bounds__(256) void k_fp8_quantize_rows(const T* __restrict__ src, int64_t R, int C, int64_t lds, uint8_t* __restrict__ dst,
                                                           int64_t ldq, float* __restrict__ scale) {
    const int l = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= R) return;
    const T* s = src + row * lds;
    float amax = 0.f;
    for (int c = l; c < C; c += 64) amax = fmaxf(amax, fabsf(ldsrc(s + c)));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) amax = fmaxf(amax, __shfl_xor(amax, d, 64));
    const float sc = amax > 0.f ? amax * (1.0f / 448.0f) : 1.0f;
    if (l == 0) scale[row] = sc;
    uint32_t* d4 = (uint32_t*)(dst + row * ldq);
    for (int64_t c = 4 * l; c < ldq; c += 256) {          // ldq % 4 == 0; columns C .. ldq - 1: zero codes
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = c + r < C ? ldsrc(s + c + r) / sc : 0.f;
        d4[c >> 2] = codes4(v[0], v[1], v[2], v[3]);
    }
}

template <class T>
int quantize_impl(const T* src, int64_t R, int32_t C, int64_t lds, void* codes, int64_t ldq, float* scale, void* stream) {
    if (R < 0 || C <= 0 || lds < C || ldq < C) return MREC_EINVAL;
    if (R == 0) return MREC_OK;
    if (!src || !codes || !scale) return MREC_EINVAL;
    if ((((uintptr_t)src) & (sizeof(T) - 1)) || (((uintptr_t)codes) & 3) || (((uintptr_t)scale) & 3)) return MREC_EINVAL;
    if (ldq % 4 || R > (int64_t(1) << 31)) return MREC_EUNSUPPORTED;
    k_fp8_quantize_rows<T><<<(unsigned)mrec_cdiv(R, 4), 256, 0, (hipStream_t)stream>>>(src, R, C, lds, (uint8_t*)codes, ldq, scale);
    MREC_LAUNCH_CHECK();
    return MREC_OK;
}

template <int AK>
int launch_out(const Args& a, int y_kind, hipStream_t st) {
    const dim3 g((unsigned)(a.nTm * a.nTn));
    if (y_kind == KIND_BF16) k_gemm_fp8_fwd<AK, KIND_BF16><<<g, kThreads, 0, st>>>(a);
    else if (y_kind == KIND_F16) k_gemm_fp8_fwd<AK, KIND_F16><<<g, kThreads, 0, st>>>(a);
    else k_gemm_fp8_fwd<AK, KIND_E4M3><<<g, kThreads, 0, st>>>(a);
    MREC_LAUNCH_CHECK();
    return MREC_OK;
}

}  // namespace f8g

MREC_API int mrec_fp8_quantize_rows_f32(const float* src, int64_t R, int32_t C, int64_t lds, void* codes, int64_t ldq, float* scale,
                                        void* stream) {
    return f8g::quantize_impl(src, R, C, lds, codes, ldq, scale, stream);
}
MREC_API int mrec_fp8_quantize_rows_f16(const uint16_t* src, int64_t R, int32_t C, int64_t lds, void* codes, int64_t ldq, float* scale,
                                        void* stream) {
    return f8g::quantize_impl((const f16o_t*)src, R, C, lds, codes, ldq, scale, stream);
}
MREC_API int mrec_fp8_quantize_rows_bf16(const uint16_t* src, int64_t R, int32_t C, int64_t lds, void* codes, int64_t ldq, float* scale,
                                         void* stream) {
    return f8g::quantize_impl((const bf16o_t*)src, R, C, lds, codes, ldq, scale, stream);
}

MREC_API int mrec_dense_fwd_fp8(const void* x, int32_t x_kind, int64_t ldx, const void* wq, int64_t ldq, const float* sw, const float* bias,
                                int64_t M, int32_t K, int32_t N, float sa, float inv_sa, float inv_so, int relu, void* y, int32_t y_kind,
                                int64_t ldy, void* stream) {
    using namespace f8g;
    if (x_kind < KIND_BF16 || x_kind > KIND_E4M3 || y_kind < KIND_BF16 || y_kind > KIND_E4M3) return MREC_EINVAL;
    if (M < 0 || K <= 0 || N <= 0 || ldx < K || ldq < K || ldy < N) return MREC_EINVAL;
    if (M == 0) return MREC_OK;
    if (!x || !wq || !sw || !y) return MREC_EINVAL;
    const bool a8 = x_kind == KIND_E4M3, y8 = y_kind == KIND_E4M3;
    if (!al16(x) || !al16(wq) || (((uintptr_t)y) & (y8 ? 3 : 7)) || (((uintptr_t)sw) & 3) || (((uintptr_t)bias) & 3)) return MREC_EINVAL;
    if (K % (a8 ? 16 : 8) || N % 8 || ldx % (a8 ? 16 : 8) || ldq % 16 || ldq < ((K + 15) & ~15) || ldy % 4) return MREC_EUNSUPPORTED;
    if (M * ldx * (a8 ? 1 : 2) >= (int64_t(1) << 31) || (int64_t)N * ldq >= (int64_t(1) << 31) || M > (int64_t(1) << 30)) return MREC_EUNSUPPORTED;
    Args a{};
    a.A = x; a.W = wq; a.Y = y; a.sw = sw; a.bias = bias;
    a.lda = ldx; a.ldq = ldq; a.ldy = ldy;
    a.M = (int)M; a.N = N; a.K = K;
    a.nTm = (int)mrec_cdiv(M, BM); a.nTn = (int)mrec_cdiv(N, BN);
    a.sa = sa; a.inv_sa = inv_sa; a.inv_so = inv_so; a.relu = relu;
    hipStream_t st = (hipStream_t)stream;
    if (x_kind == KIND_BF16) return launch_out<KIND_BF16>(a, y_kind, st);
    if (x_kind == KIND_F16) return launch_out<KIND_F16>(a, y_kind, st);
    return launch_out<KIND_E4M3>(a, y_kind, st);
}

/* rows and columns of the kernel's output tile (the tests place their shapes around them) */
MREC_API int mrec_dense_fwd_fp8_tile(int32_t* rows_out, int32_t* cols_out) {
    if (!rows_out || !cols_out) return MREC_EINVAL;
    *rows_out = f8g::BM; *cols_out = f8g::BN;
    return MREC_OK;
}
