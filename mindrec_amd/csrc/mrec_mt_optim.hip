// mrec_mt_optim.hip -- the table optimizers of the multitable Wide&Deep's training step as ONE launch chain, for gfx950: nn.Adam over
// every table, nn.FTRL over every wide vector and over the plain wide parameters (wide_continue_w, wide_bias), all dense -- the tables
// are dense Parameters under P.Gather, so every element of every table moves every step.
//
// Reference call sites: models/wide_and_deep_multitable/src/wide_and_deep.py:510-535 (TrainStepWrap: FTRL over the parameters whose
// name holds "wide", Adam over the rest), :286-349, 361-424 (the Gathers whose bprop the row-gradient sums are).
//
// What it replaces, per table: mrec_dense_adam_rows_l2_f32 (a memset of the table's row -> group map, k_rows_to_groups, the update) and,
// for its wide vector, a scatter of the groups' sums into a zero [V] gradient, mrec_dense_ftrl_f32 and a second scatter that clears the
// touched entries again -- six launches, every one of which builds or reads the same row -> group map; plus one mrec_dense_ftrl_f32
// per plain vector.  Here: ONE memset of the concatenated map (sum of V ints), ONE k_mt_rows_to_groups over all tables, ONE
// k_mt_optim.  The element formulas are mrec_optim.h's (adam_elem, ftrl_elem), called with the expressions of k_dense_adam_rows_l2
// and k_dense_ftrl in their order (the l2 term: product rounded, then added; -ffp-contract=off): the same bits as the composition.
//
// Shape of k_mt_optim: an ITEM is a table (Adam), a table's wide vector (FTRL, gradient through the map) or a plain vector (FTRL,
// gradient as it is); a workgroup belongs to ONE item -- it finds it from its block index in a table of first blocks, as k_mt_input
// does -- so V, D, the pointers and the float4 / scalar choice are scalar per workgroup.  Inside an item the workgroups walk it with the
// item's stride: a thread owns a float4 (D % 4 == 0) or an element of p, m, v.  HBM-bound streaming: no LDS, no atomics, no barrier.
// The records travel BY VALUE in the kernels' arguments: no table in device memory, no copy, no allocation, no synchronisation -- the
// entry is capturable and every argument is constant from step to step (the step size: mrec_step_state_t).
#include "mrec_common.h"
#include "mrec_optim.h"

namespace {

enum : int { kMoTable = 0, kMoWide = 1, kMoVec = 2 };
constexpr int kMoMaxItems = 2 * MREC_MT_BWD_MAX_GROUPS + MREC_MT_OPT_MAX_VECS;

struct MoTab {
    float* p; float* m; float* v;
    float* w; float* a; float* lin;
    const int* uniq; const int64_t* n_uniq;
    const float* sums; const float* wsums;
    int64_t V, U, rg0;                 // rg0: the table's first word of the concatenated row -> group map
    int D;
    unsigned blk0, nblk;               // k_mt_rows_to_groups: the table's first workgroup and its workgroups
};
struct MoVec { float* w; float* a; float* lin; const float* g; int64_t n; };
struct MoItem { int kind, idx; unsigned blk0, nblk; };
struct MoArgs {
    AdamH ah; FtrlH fh; float l2s;
    const StepState* ss;
    int* row_group;
    int n_tabs, n_items;
    MoItem item[kMoMaxItems];
    MoTab tab[MREC_MT_BWD_MAX_GROUPS];
    MoVec vec[MREC_MT_OPT_MAX_VECS];
};

// row_group[rg0 + uniq[g]] = g for every table's groups g < min(U, *n_uniq) (the map was set to -1 everywhere before; a row outside
// [0, V) gets no entry): k_rows_to_groups (mrec_dense_optim.hip) over all tables, a workgroup in one table
__global__ __launch_bounds__(256) void k_mt_rows_to_groups(const MoArgs a) {
    int ti = 0;                        // (uniform: the workgroup's table; a table without groups has no workgroups)
    for (int i = 0; i < a.n_tabs; ++i)
        if (a.tab[i].nblk > 0 && blockIdx.x >= a.tab[i].blk0) ti = i;
    const MoTab& t = a.tab[ti];
    const int64_t n = t.n_uniq ? min(t.U, *t.n_uniq) : t.U;
    int* __restrict__ rg = a.row_group + t.rg0;
    for (int64_t g = (int64_t)(blockIdx.x - t.blk0) * 256 + threadIdx.x; g < n; g += (int64_t)t.nblk * 256) {
        const int r = t.uniq[g];
        if (r >= 0 && r < t.V) rg[r] = (int)g;
    }
}

// nn.Adam over a whole table through the map: k_dense_adam_rows_l2's loop (without its sum of squares), element for element
template <int VEC>
__device__ __forceinline__ void mo_table(const MoTab& t, const int* __restrict__ row_group, const AdamH& h, float l2s, int64_t blk,
                                         int64_t nblk) {
    float* __restrict__ p = t.p; float* __restrict__ m = t.m; float* __restrict__ v = t.v;
    const float* __restrict__ sums = t.sums;
    const int D = t.D, DV = D / VEC;
    const int64_t n = t.V * DV, stride = nblk * 256;
    const int64_t sr = stride / DV;
    const int sc = (int)(stride - sr * DV);
    int64_t i = blk * 256 + threadIdx.x;
    int64_t r = i / DV;
    int c = (int)(i - r * DV);
    for (; i < n; i += stride) {
        const int g = row_group[r];
        const int64_t e = (r * DV + c) * VEC;
        if (VEC == 4) {
            float4 pp = *(float4*)(p + e), mm = *(float4*)(m + e), vv = *(float4*)(v + e);
            float4 gg = g >= 0 ? *(const float4*)(sums + ((int64_t)g * DV + c) * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
            gg.x += l2s * pp.x; gg.y += l2s * pp.y; gg.z += l2s * pp.z; gg.w += l2s * pp.w;       // product rounded, then added (no fma)
            adam_elem(pp.x, mm.x, vv.x, gg.x * h.gscale, h);
            adam_elem(pp.y, mm.y, vv.y, gg.y * h.gscale, h);
            adam_elem(pp.z, mm.z, vv.z, gg.z * h.gscale, h);
            adam_elem(pp.w, mm.w, vv.w, gg.w * h.gscale, h);
            *(float4*)(p + e) = pp; *(float4*)(m + e) = mm; *(float4*)(v + e) = vv;
        } else {
            float pp = p[e], mm = m[e], vv = v[e];
            float gg = g >= 0 ? sums[(int64_t)g * D + c] : 0.f;
            gg += l2s * pp;
            adam_elem(pp, mm, vv, gg * h.gscale, h);
            p[e] = pp; m[e] = mm; v[e] = vv;
        }
        r += sr; c += sc;
        if (c >= DV) { c -= DV; ++r; }
    }
}

__global__ __launch_bounds__(256) void k_mt_optim(const MoArgs a) {
    int it = 0;
    for (int i = 1; i < a.n_items; ++i) it += blockIdx.x >= a.item[i].blk0 ? 1 : 0;      // (uniform: the workgroup's item)
    const MoItem im = a.item[it];
    const int64_t blk = (int64_t)(blockIdx.x - im.blk0), nblk = im.nblk;
    if (im.kind == kMoTable) {
        AdamH h = a.ah;
        if (a.ss) h.lr_t = a.ss->lr_t;         // this step's bias-corrected step size from device memory (mrec_step_advance)
        const MoTab& t = a.tab[im.idx];
        if (t.D % 4 == 0) mo_table<4>(t, a.row_group + t.rg0, h, a.l2s, blk, nblk);
        else mo_table<1>(t, a.row_group + t.rg0, h, a.l2s, blk, nblk);
    } else if (im.kind == kMoWide) {           // k_dense_ftrl on the gradient a scatter of wsums into a zero [V] buffer would hold
        const MoTab& t = a.tab[im.idx];
        const int* __restrict__ rg = a.row_group + t.rg0;
        float* __restrict__ w = t.w; float* __restrict__ ac = t.a; float* __restrict__ lin = t.lin;
        for (int64_t i = blk * 256 + threadIdx.x; i < t.V; i += nblk * 256) {
            const int g = rg[i];
            float ww = w[i], aa = ac[i], ll = lin[i];
            const float gg = g >= 0 ? t.wsums[g] : 0.f;
            ftrl_elem(ww, aa, ll, gg * a.fh.gscale, a.fh);
            w[i] = ww; ac[i] = aa; lin[i] = ll;
        }
    } else {                                   // k_dense_ftrl
        const MoVec& q = a.vec[im.idx];
        float* __restrict__ w = q.w; float* __restrict__ ac = q.a; float* __restrict__ lin = q.lin;
        for (int64_t i = blk * 256 + threadIdx.x; i < q.n; i += nblk * 256) {
            float ww = w[i], aa = ac[i], ll = lin[i];
            ftrl_elem(ww, aa, ll, q.g[i] * a.fh.gscale, a.fh);
            w[i] = ww; ac[i] = aa; lin[i] = ll;
        }
    }
}

// the record, the shapes: everything that is decided without looking at a pointer.  *total_v: the words of the concatenated map.
int mo_check(const mrec_mt_opt_tab_t* tabs, int32_t n_tabs, const mrec_mt_opt_vec_t* vecs, int32_t n_vecs, int64_t* total_v) {
    if (n_tabs < 0 || n_tabs > MREC_MT_BWD_MAX_GROUPS || n_vecs < 0 || n_vecs > MREC_MT_OPT_MAX_VECS) return MREC_EINVAL;
    if ((n_tabs > 0 && !tabs) || (n_vecs > 0 && !vecs)) return MREC_EINVAL;
    for (int i = 0; i < n_tabs; ++i)
        if (tabs[i].V < 0 || tabs[i].D <= 0 || tabs[i].U < 0) return MREC_EINVAL;
    for (int i = 0; i < n_vecs; ++i)
        if (vecs[i].n < 0) return MREC_EINVAL;
    int64_t tv = 0;
    for (int i = 0; i < n_tabs; ++i) {
        if (tabs[i].V >= (int64_t(1) << 31) || tabs[i].U >= (int64_t(1) << 31)) return MREC_EUNSUPPORTED;      // (a group index is an int)
        if (tabs[i].V * (int64_t)tabs[i].D >= (int64_t(1) << 40)) return MREC_EUNSUPPORTED;
        tv += tabs[i].V;
    }
    *total_v = tv;
    return MREC_OK;
}

}  // namespace

MREC_API int mrec_mt_optim_workspace_bytes(const mrec_mt_opt_tab_t* tabs, int32_t n_tabs, size_t* out) {
    if (!out) return MREC_EINVAL;
    int64_t tv = 0;
    const int rc = mo_check(tabs, n_tabs, nullptr, 0, &tv);
    if (rc != MREC_OK) return rc;
    MrecArena ar;
    if (tv > 0) ar.take<int>((size_t)tv);
    *out = ar.off;
    return MREC_OK;
}

MREC_API int mrec_mt_optim(const mrec_mt_opt_tab_t* tabs, int32_t n_tabs, const mrec_mt_opt_vec_t* vecs, int32_t n_vecs,
                           const mrec_mt_opt_adam_t* adam, const mrec_mt_opt_ftrl_t* ftrl, const void* step_state, void* ws,
                           size_t ws_bytes, void* stream) {
    // 1. the record, 2. shapes outside what the kernels cover
    int64_t tv = 0;
    const int rc = mo_check(tabs, n_tabs, vecs, n_vecs, &tv);
    if (rc != MREC_OK) return rc;
    if (!adam || !ftrl) return MREC_EINVAL;
    // 3. pointers
    for (int i = 0; i < n_tabs; ++i) {
        const mrec_mt_opt_tab_t& t = tabs[i];
        const int nw = (t.w ? 1 : 0) + (t.accum ? 1 : 0) + (t.linear ? 1 : 0);
        if (nw != 0 && nw != 3) return MREC_EINVAL;                   // a wide vector comes with its accum and linear, or not at all
        if (t.V == 0) continue;
        if (!t.p || !t.m || !t.v) return MREC_EINVAL;
        if (t.U > 0 && (!t.uniq || !t.sums || (nw && !t.wsums))) return MREC_EINVAL;
    }
    for (int i = 0; i < n_vecs; ++i) {
        const mrec_mt_opt_vec_t& q = vecs[i];
        if (q.n > 0 && (!q.w || !q.accum || !q.linear || !q.g)) return MREC_EINVAL;
    }
    // 4. the float4 path's alignment
    for (int i = 0; i < n_tabs; ++i) {
        const mrec_mt_opt_tab_t& t = tabs[i];
        if (t.V > 0 && t.D % 4 == 0 && (!al16(t.p) || !al16(t.m) || !al16(t.v) || (t.sums && !al16(t.sums)))) return MREC_EUNSUPPORTED;
    }
    // 5. the workspace: the concatenated row -> group map
    MrecArena ar(ws, tv > 0 ? ws_bytes : 0);
    int* row_group = tv > 0 ? ar.take<int>((size_t)tv) : nullptr;
    if (tv > 0 && (!ws || !ar.ok || !row_group)) return MREC_EWORKSPACE;

    MoArgs a{};
    a.ah = adam_hyper(adam->lr, adam->b1, adam->b2, adam->eps, adam->b1_pow, adam->b2_pow, adam->grad_scale, adam->nesterov);
    a.fh = FtrlH{ftrl->lr, ftrl->l1, ftrl->l2, ftrl->lr_power, ftrl->grad_scale};
    a.l2s = adam->l2_scaled;
    a.ss = (const StepState*)step_state;
    a.row_group = row_group;
    a.n_tabs = n_tabs;
    uint64_t nb = 0, nbr = 0;
    int64_t rg0 = 0;
    const auto add_item = [&](int kind, int idx, int64_t work) {
        if (work <= 0) return;
        MoItem& im = a.item[a.n_items++];
        im = {kind, idx, (unsigned)nb, stream_grid(work)};
        nb += im.nblk;
    };
    for (int i = 0; i < n_tabs; ++i) {
        const mrec_mt_opt_tab_t& t = tabs[i];
        MoTab& d = a.tab[i];
        d = {t.p, t.m, t.v, t.w, t.accum, t.linear, t.uniq, t.n_uniq_dev, t.sums, t.wsums, t.V, t.V > 0 ? t.U : 0, rg0, t.D, (unsigned)nbr, 0};
        if (d.U > 0) { d.nblk = stream_grid(d.U); nbr += d.nblk; }
        rg0 += t.V;
        add_item(kMoTable, i, t.V * (t.D % 4 == 0 ? t.D / 4 : t.D));
    }
    for (int i = 0; i < n_tabs; ++i)
        if (tabs[i].w) add_item(kMoWide, i, tabs[i].V);
    for (int i = 0; i < n_vecs; ++i) {
        a.vec[i] = {vecs[i].w, vecs[i].accum, vecs[i].linear, vecs[i].g, vecs[i].n};
        add_item(kMoVec, i, vecs[i].n);
    }
    if (nb == 0) return MREC_OK;
    hipStream_t st = (hipStream_t)stream;
    if (tv > 0) MREC_HIP_CHECK(hipMemsetAsync(row_group, 0xFF, (size_t)tv * sizeof(int), st));          // -1 everywhere
    if (nbr > 0) k_mt_rows_to_groups<<<(unsigned)nbr, 256, 0, st>>>(a);
    k_mt_optim<<<(unsigned)nb, 256, 0, st>>>(a);
    MREC_LAUNCH_CHECK();
    return MREC_OK;
}
