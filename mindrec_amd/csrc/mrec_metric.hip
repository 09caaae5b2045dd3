// mrec_metric.hip -- evaluation metrics on the device as exact integer counts (include/mrec.h "evaluation metrics").
//
//   mrec_auc_counts       {twoU, P, N, n_nan} of (pred, label): the ROC area is twoU / (2 P N), one division on the host
//   mrec_group_rank_hist  {hist[0..topk-1], G} of (pred, label, group index): MAP@topk is (sum_r hist[r] / (r + 1)) / G
//
// Every device-side sum is an integer (32-bit inside a tile or a group, 64-bit across them), every atomic an integer atomic: the
// outputs do not depend on the order the workgroups run in, two calls over the same input give the same bits.
#include "mrec_radix.h"

namespace {

constexpr int MT = 1024;                      // rows per tile of the count / boundary kernels: 256 threads x 4 consecutive rows
constexpr uint32_t KEY_NAN = 0xFFFFFFFFu;     // every NaN: above +inf (0xFF800000), the key of no number
constexpr uint32_t KEY_ZERO = 0x80000000u;    // +0.0 and -0.0

// float -> 32-bit key whose unsigned order is the IEEE order of the numbers: -inf < ... < -denormals < (-0.0 = +0.0) < denormals < ... < +inf
__device__ __forceinline__ uint32_t order_key(float x) {
    uint32_t u = __float_as_uint(x);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return KEY_NAN;
    if (u == 0x80000000u) u = 0;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ---- AUC ------------------------------------------------------------------------------------------------------------------
// value carried through the sort: 0 = negative, 1 = positive (label > 0.5), 2 = NaN prediction (sorts behind +inf, counts as neither)
__global__ __launch_bounds__(256) void k_auc_keys(const float* __restrict__ pred, const float* __restrict__ label, int n,
                                                  int* __restrict__ keys, int* __restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = order_key(pred[i]);
    keys[i] = (int)k;
    vals[i] = k == KEY_NAN ? 2 : (label[i] > 0.5f ? 1 : 0);
}

// A thread's 4 consecutive rows of the sorted order: how many positives, negatives and tie-group heads (a row whose key differs from
// the row before it; row 0) they hold, and which (bits 0..3 of *heads, *posm, *negm).
__device__ __forceinline__ void auc_rows4(const int* __restrict__ keys, const int* __restrict__ vals, int n, int64_t i0, int* heads,
                                          int* posm, int* negm) {
    const int64_t nl = n - 1;
    int k[5], v[4];
    k[0] = keys[i0 > 0 ? (i0 - 1 < nl ? i0 - 1 : nl) : 0];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t i = i0 + j < nl ? i0 + j : nl;
        k[j + 1] = keys[i];
        v[j] = vals[i];
    }
    int h = 0, p = 0, q = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (i0 + j < n) {
            h |= (int)(i0 + j == 0 || k[j + 1] != k[j]) << j;
            p |= (int)(v[j] == 1) << j;
            q |= (int)(v[j] == 0) << j;
        }
    }
    *heads = h; *posm = p; *negm = q;
}

// per tile of MT sorted rows: its positives, negatives and heads -> tcnt[0..2][tile]
__global__ __launch_bounds__(256) void k_auc_tile_counts(const int* __restrict__ keys, const int* __restrict__ vals, int n, int ntiles,
                                                         int* __restrict__ tcnt) {
    __shared__ int sm[8];
    int h, p, q, tp, tq, th;
    auc_rows4(keys, vals, n, (int64_t)blockIdx.x * MT + threadIdx.x * 4, &h, &p, &q);
    block_excl_scan_256(__popc(p), sm, &tp);
    block_excl_scan_256(__popc(q), sm, &tq);
    block_excl_scan_256(__popc(h), sm, &th);
    if (threadIdx.x == 0) {
        tcnt[blockIdx.x] = tp;
        tcnt[ntiles + blockIdx.x] = tq;
        tcnt[2 * ntiles + blockIdx.x] = th;
    }
}

// one workgroup: the three rows of tcnt become exclusive prefixes over the tiles; P, N, n_nan and a zeroed twoU go to out, the number of
// tie groups to *m_dev
__global__ __launch_bounds__(256) void k_auc_tile_scan(int* __restrict__ tcnt, int ntiles, int n, int64_t* __restrict__ out,
                                                       int* __restrict__ m_dev) {
    __shared__ int sm[8];
    int tot3[3];
    for (int r = 0; r < 3; ++r) {
        int* row = tcnt + (int64_t)r * ntiles;
        int carry = 0;
        for (int c = 0; c < ntiles; c += 256) {
            const int t = c + threadIdx.x;
            const int x = t < ntiles ? row[t] : 0;
            int tot;
            const int ex = block_excl_scan_256(x, sm, &tot);
            if (t < ntiles) row[t] = carry + ex;
            carry += tot;
        }
        tot3[r] = carry;
    }
    if (threadIdx.x == 0) {
        out[0] = 0;
        out[1] = tot3[0];
        out[2] = tot3[1];
        out[3] = (int64_t)n - tot3[0] - tot3[1];
        *m_dev = tot3[2];
    }
}

// the heads, compacted: bnd[j] = (positives, negatives) in front of the j-th tie group; bnd[m] = (P, N)
__global__ __launch_bounds__(256) void k_auc_bounds(const int* __restrict__ keys, const int* __restrict__ vals, int n, int ntiles,
                                                    const int* __restrict__ tcnt, int2* __restrict__ bnd) {
    __shared__ int sm[8];
    const int64_t i0 = (int64_t)blockIdx.x * MT + threadIdx.x * 4;
    int h, p, q, tot;
    auc_rows4(keys, vals, n, i0, &h, &p, &q);
    int cp = tcnt[blockIdx.x] + block_excl_scan_256(__popc(p), sm, &tot);
    int cn = tcnt[ntiles + blockIdx.x] + block_excl_scan_256(__popc(q), sm, &tot);
    int slot = tcnt[2 * ntiles + blockIdx.x] + block_excl_scan_256(__popc(h), sm, &tot);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (i0 + j < n) {
            if ((h >> j) & 1) bnd[slot++] = make_int2(cp, cn);
            cp += (p >> j) & 1;
            cn += (q >> j) & 1;
            if (i0 + j == (int64_t)n - 1) bnd[slot] = make_int2(cp, cn);
        }
    }
}

__device__ __forceinline__ long long wave_sum_i64(long long x) {
#pragma unroll
    for (int d = 32; d; d >>= 1) x += __shfl_down(x, d, 64);
    return x;
}

// neighbours paired: group j = [bnd[j], bnd[j+1]) adds (its positives) x (negatives below it + negatives below its end) to twoU
__global__ __launch_bounds__(256) void k_auc_pairs(const int2* __restrict__ bnd, const int* __restrict__ m_dev,
                                                   int64_t* __restrict__ out) {
    __shared__ long long part[4];
    const int m = *m_dev;
    long long s = 0;
    for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < m; j += (int64_t)gridDim.x * 256) {
        const int2 a = bnd[j], b = bnd[j + 1];
        s += (long long)(b.x - a.x) * ((long long)a.y + b.y);
    }
    s = wave_sum_i64(s);
    if (lane_id() == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        s = part[0] + part[1] + part[2] + part[3];
        if (s) atomicAdd((unsigned long long*)out, (unsigned long long)s);
    }
}

// ---- grouped rank histogram -----------------------------------------------------------------------------------------------
// Rows of one group that sit side by side in a wave are combined before they meet in memory: a lane's run is the stretch of equal
// neighbouring group numbers it lies in, the run's last lane ends up with the run's reduction and issues the one atomic.  A display
// holding every row costs one atomic per wave, not one per row; ids interleaved row by row spread their atomics over the groups.
struct WaveRun {
    int start;      // first lane of this lane's run
    bool tail;      // this lane is its run's last
};

__device__ __forceinline__ WaveRun wave_runs(int g) {
    const int l = lane_id();
    const int gp = __shfl_up(g, 1, 64);
    const uint64_t heads = __ballot(l == 0 || gp != g);                 // (bit 0 is always set)
    WaveRun r;
    r.start = 63 - __clzll((long long)(heads & (~0ull >> (63 - l))));
    r.tail = l == 63 || ((heads >> ((l + 1) & 63)) & 1);
    return r;
}

template <class T, class Op>
__device__ __forceinline__ T wave_run_scan(T v, int start, Op op) {
    const int l = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(v, d, 64);
        if (l - d >= start) v = op(v, y);
    }
    return v;
}

// best[g] = max over the group's rows of (label key, ~row): the first row holding the maximal label; size[g] = its rows
__global__ __launch_bounds__(256) void k_grp_click(const float* __restrict__ label, const int* __restrict__ inv, int n,
                                                   unsigned long long* __restrict__ best, int* __restrict__ size) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int g = i < n ? inv[i] : -1;
    if ((unsigned)g >= (unsigned)n) g = -1;                             // (a group number that is none: the row joins no group)
    unsigned long long v = 0;
    if (g >= 0) v = ((unsigned long long)order_key(label[i]) << 32) | (uint32_t)~(uint32_t)i;
    const WaveRun r = wave_runs(g);
    v = wave_run_scan(v, r.start, [](unsigned long long a, unsigned long long b) { return a > b ? a : b; });
    const int c = wave_run_scan(1, r.start, [](int a, int b) { return a + b; });
    if (r.tail && g >= 0) {
        atomicMax(&best[g], v);
        atomicAdd(&size[g], c);
    }
}

// gt[g] = rows of the group whose prediction is above the clicked row's
__global__ __launch_bounds__(256) void k_grp_rank(const float* __restrict__ pred, const int* __restrict__ inv, int n,
                                                  const unsigned long long* __restrict__ best, int* __restrict__ gt) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int g = i < n ? inv[i] : -1;
    if ((unsigned)g >= (unsigned)n) g = -1;
    int above = 0;
    if (g >= 0) {
        const uint32_t c = ~(uint32_t)best[g];
        const uint32_t kc = order_key(pred[c < (uint32_t)n ? c : 0]), ki = order_key(pred[i]);
        above = ki != KEY_NAN && kc != KEY_NAN && ki > kc;
    }
    const WaveRun r = wave_runs(g);
    above = wave_run_scan(above, r.start, [](int a, int b) { return a + b; });
    if (r.tail && g >= 0 && above) atomicAdd(&gt[g], above);
}

// per group: rank = gt (+ the pads above a negative clicked prediction) -> hist[rank]; out[topk] = G
__global__ __launch_bounds__(256) void k_grp_hist(const float* __restrict__ pred, int n, const int64_t* __restrict__ n_groups_dev,
                                                  const unsigned long long* __restrict__ best, const int* __restrict__ size,
                                                  const int* __restrict__ gt, int topk, int pad_to, int64_t* __restrict__ out) {
    __shared__ int h[64];
    int64_t G = *n_groups_dev;
    G = G < 0 ? 0 : (G < n ? G : n);
    if (blockIdx.x == 0 && threadIdx.x == 0) out[topk] = G;
    if ((int64_t)blockIdx.x * 256 >= G) return;
    if (threadIdx.x < 64) h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g < G) {
        const int m = size[g];
        const uint32_t c = ~(uint32_t)best[g];
        int64_t rank = gt[g];
        if (m < pad_to && order_key(pred[c < (uint32_t)n ? c : 0]) < KEY_ZERO) rank += pad_to - m;
        if (m > 0 && rank < topk) atomicAdd(&h[rank], 1);
    }
    __syncthreads();
    if ((int)threadIdx.x < topk && h[threadIdx.x]) atomicAdd((unsigned long long*)&out[threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

struct AucWs {
    int *ka, *va, *kb, *vb, *hist, *hscan, *totals, *tcnt, *m_dev;
    int2* bnd;
};

bool auc_carve(MrecArena& a, int64_t n, AucWs* w) {
    const size_t nblk = (size_t)mrec_cdiv(n, RT), ntiles = (size_t)mrec_cdiv(n, MT);
    w->ka = a.take<int>(n);
    w->va = a.take<int>(n);
    w->kb = a.take<int>(n);
    w->vb = a.take<int>(n);
    w->hist = a.take<int>(nblk * RNB);
    w->hscan = a.take<int>(nblk * RNB);
    w->totals = a.take<int>(RNB);
    w->tcnt = a.take<int>(3 * ntiles);
    w->m_dev = a.take<int>(1);
    w->bnd = a.take<int2>((size_t)n + 1);
    return a.ok;
}

}  // namespace

MREC_API int mrec_auc_ws_bytes(int64_t n, size_t* out) {
    if (!out || n < 0) return MREC_EINVAL;
    if (n >= (int64_t(1) << 31)) return MREC_EUNSUPPORTED;
    MrecArena a(nullptr, 0);
    AucWs w;
    auc_carve(a, n ? n : 1, &w);
    *out = a.off;
    return MREC_OK;
}

MREC_API int mrec_auc_counts(const float* pred, const float* label, int64_t n, int64_t* out4, void* ws, size_t ws_bytes, void* stream) {
    if (n < 1 || !pred || !label || !out4 || !ws) return MREC_EINVAL;
    if (n >= (int64_t(1) << 31)) return MREC_EUNSUPPORTED;
    MrecArena a(ws, ws_bytes);
    AucWs w;
    if (!auc_carve(a, n, &w)) return MREC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int ni = (int)n, ntiles = (int)mrec_cdiv(n, MT);
    k_auc_keys<<<(unsigned)mrec_cdiv(n, 256), 256, 0, st>>>(pred, label, ni, w.ka, w.va);
    radix_pass(w.ka, w.va, ni, 0, 11, w.hist, w.hscan, w.totals, nullptr, w.kb, w.vb, st);
    radix_pass(w.kb, w.vb, ni, 11, 11, w.hist, w.hscan, w.totals, nullptr, w.ka, w.va, st);
    radix_pass(w.ka, w.va, ni, 22, 10, w.hist, w.hscan, w.totals, nullptr, w.kb, w.vb, st);
    k_auc_tile_counts<<<ntiles, 256, 0, st>>>(w.kb, w.vb, ni, ntiles, w.tcnt);
    k_auc_tile_scan<<<1, 256, 0, st>>>(w.tcnt, ntiles, ni, out4, w.m_dev);
    k_auc_bounds<<<ntiles, 256, 0, st>>>(w.kb, w.vb, ni, ntiles, w.tcnt, w.bnd);
    const int64_t pb = mrec_cdiv(n, 256);
    k_auc_pairs<<<(unsigned)(pb < 1024 ? pb : 1024), 256, 0, st>>>(w.bnd, w.m_dev, out4);
    MREC_LAUNCH_CHECK();
    return MREC_OK;
}

MREC_API int mrec_group_rank_ws_bytes(int64_t n, size_t* out) {
    if (!out || n < 0) return MREC_EINVAL;
    if (n >= (int64_t(1) << 30)) return MREC_EUNSUPPORTED;
    const size_t nn = (size_t)(n ? n : 1);
    *out = mrec_align_up(nn * 8, 256) + 2 * mrec_align_up(nn * 4, 256);
    return MREC_OK;
}

MREC_API int mrec_group_rank_hist(const float* pred, const float* label, const int32_t* inv, const int64_t* n_groups_dev, int64_t n,
                                  int32_t topk, int32_t pad_to, int64_t* out, void* ws, size_t ws_bytes, void* stream) {
    if (n < 1 || topk < 1 || topk > 64 || pad_to < 0 || !pred || !label || !inv || !n_groups_dev || !out || !ws) return MREC_EINVAL;
    if (n >= (int64_t(1) << 30)) return MREC_EUNSUPPORTED;
    MrecArena a(ws, ws_bytes);
    unsigned long long* best = a.take<unsigned long long>(n);
    int* size = a.take<int>(n);
    int* gt = a.take<int>(n);
    if (!a.ok) return MREC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    MREC_HIP_CHECK(hipMemsetAsync(ws, 0, a.off, st));
    MREC_HIP_CHECK(hipMemsetAsync(out, 0, sizeof(int64_t) * (topk + 1), st));
    const unsigned nb = (unsigned)mrec_cdiv(n, 256);
    k_grp_click<<<nb, 256, 0, st>>>(label, inv, (int)n, best, size);
    k_grp_rank<<<nb, 256, 0, st>>>(pred, inv, (int)n, best, gt);
    k_grp_hist<<<nb, 256, 0, st>>>(pred, (int)n, n_groups_dev, best, size, gt, topk, pad_to, out);
    MREC_LAUNCH_CHECK();
    return MREC_OK;
}
