"""max_norm over multi-hot fields on the GPU: the clip instantiations of the pooled lookups (mrec_gather_pool_fields_clip,
mrec_gather_pool_fields_keyed_clip), the pooled apply under the clip (mrec_apply_opts_t's fields form with max_norm) and max_norm on
MultiHotEmbedding, MultiHotWideDeep and MultiHotHashEmbedding.

  lookup: bit for bit against ops.gather_rows(max_norm=c) -- an existing, separately tested kernel -- pooled on the host
    (tests/_pool_clip_ref.py);
  apply: bit for bit against ops.sparse_lazy_adam_(max_norm=c) on the expanded gradient where both form the same products; for
    unequal lengths in mean mode against the clip-aware oracle (tests/_oracle_clip_ops.py) within the bound of
    test_max_norm_gpu.py::test_sparse_lazy_adam_clip_matches_oracle; one clip decision per row in the forward and the backward;
  classes: against the ops calls, eager and captured; the wide half untouched by the clip; the hash table against MapTensorGet rows
    and against the dense sibling;
  refusals: nothing is launched, and the call after one is the plain call.
Tables hold a zero row, a row of norm exactly c and rows within a few ulps of c; ids include -1 and V."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _oracle_clip_ops as OC  # noqa: E402
import _pool_clip_ref as CR  # noqa: E402
import _pool_fields_ref as FR  # noqa: E402
from oracle import oracle as O  # noqa: E402

_KIND = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
_NP = {torch.int32: np.int32, torch.int64: np.int64}
SIX = (3, 5, 4, 3, 4, 2)
C = 0.75                      # (its square is an exact float32: the tie row's fp32 norm is c)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.detach().float().cpu().numpy().view(np.uint32)


def _same(got, ref, what):
    ref = np.ascontiguousarray(ref, np.float32).view(np.uint32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = (got != ref).reshape(got.shape[0], -1).any(axis=1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} rows differ, e.g. rows {np.nonzero(bad)[0][:6].tolist()}"


def _same_t(xs, ys, what):
    for i, (x, y) in enumerate(zip(xs, ys)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), f"{what}: array {i}"


def _masks(rng, B, Ls):
    """None, a 0/1 mask (an all-zero and an all-one sample among them), fractional weights"""
    m01 = (rng.random((B, Ls)) < 0.6).astype(np.float32)
    m01[0], m01[1] = 0.0, 1.0
    return (None, m01, (rng.standard_normal((B, Ls)) * 1.5).astype(np.float32))


def _clipped_rows(table_t, ids_t, dev):
    """[n, D] float32 on the host: gather_rows(max_norm=c) of every slot's id, a zero row where the id is outside [0, V)"""
    from mindrec_amd import ops
    flat = ids_t.reshape(-1)
    rows = ops.gather_rows(table_t, flat, max_norm=C).cpu().numpy()
    out = (flat < 0) | (flat >= table_t.shape[0])
    rows[out.cpu().numpy()] = 0.0
    return rows


# ---- 1. lookup -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [(1,), (2, 1), (9,), SIX])
@pytest.mark.parametrize("D", [4, 8, 12, 64, 252, 256])
def test_gather_pool_fields_clip_bitwise(dev, D, lens):
    """D = 12: a lane-group that is not a power of two; 252: 63 lanes; 256: all 64.  (2, 1): PB = 2; (9,): two batches of 8 slots.
    B = 37 does not fill the last workgroup; B = 300 (the six fields) is several workgroups."""
    from mindrec_amd import ops
    rng = np.random.default_rng(1000 * D + sum(lens))
    V, F, Ls = 50, len(lens), sum(lens)
    tab = CR.special_table(rng, V, D, C)
    t = T(tab, dev)
    nrm = np.linalg.norm(tab.astype(np.float64), axis=1)
    assert (nrm > 1.01 * C).sum() > 10 and ((nrm < 0.99 * C) & (nrm > 0)).sum() > 10
    for B in ((37, 300) if lens == SIX else (37,)):
        for idt in (torch.int32, torch.int64):
            ids = CR.ids_with_outsiders(rng, B, Ls, V, _NP[idt])
            tid = T(ids, dev)
            rows = _clipped_rows(t, tid, dev)
            assert not np.array_equal(rows, ops.gather_rows(t, tid.reshape(-1)).cpu().numpy())      # some row was clipped
            for mask in _masks(rng, B, Ls):
                tm = T(mask, dev) if mask is not None else None
                for mode in ("sum", "mean"):
                    for odt in (torch.float32, torch.bfloat16, torch.float16):
                        what = f"D={D} fields={lens} B={B} {idt} {mode} {odt} mask={mask is not None}"
                        ref = CR.clipped_pool(rows, B, lens, mask, mode, _KIND[odt])      # (16-bit: the reference rounded once)
                        got = ops.gather_pool_fields(t, tid, lens, tm, mode=mode, out_dtype=odt, max_norm=C)
                        _same(_bits(got), ref, what)
            if F == 1:                                                    # gather_pool(max_norm=): the one-field case
                got = ops.gather_pool(t, tid, None, mode="mean", max_norm=C)
                _same(_bits(got), CR.clipped_pool(rows, B, lens, None, "mean"), f"D={D} gather_pool L={Ls}")
    # max_norm=None is today's entry: the unclipped pooled lookup
    plain = ops.gather_pool_fields(t, tid, lens, None, mode="sum")
    _same(_bits(plain), FR.gather_pool_fields(tab, ids, lens, None, "sum"), "max_norm=None")


def test_gather_pool_fields_clip_column_block(dev):
    """out as a column block of a wider matrix: its other columns keep their bits"""
    from mindrec_amd import ops
    rng = np.random.default_rng(2)
    V, D, B, lens = 50, 8, 37, SIX
    F, Ls = len(lens), sum(lens)
    t = T(CR.special_table(rng, V, D, C), dev)
    tid = T(CR.ids_with_outsiders(rng, B, Ls, V, np.int32), dev)
    mask = _masks(rng, B, Ls)[2]
    wide0 = (rng.integers(-64, 65, size=(B, F * D + 8)) / 8.0).astype(np.float32)
    wide = T(wide0, dev)
    ops.gather_pool_fields(t, tid, lens, T(mask, dev), mode="mean", out=wide[:, 4:4 + F * D], max_norm=C)
    wide0[:, 4:4 + F * D] = CR.clipped_pool(_clipped_rows(t, tid, dev), B, lens, mask, "mean")
    _same(_bits(wide), wide0, "column block")


# ---- 2. apply ------------------------------------------------------------------------------------------------------------------------
def _state(rng, tab):
    return [tab.copy(), (rng.standard_normal(tab.shape) * 1e-3).astype(np.float32), (rng.random(tab.shape) * 1e-5).astype(np.float32)]


def _g_rows(rng, rows, D, gdt, dev):
    g = rng.standard_normal((rows, D)).astype(np.float32)
    if gdt != torch.float32:
        g = O.round16(g, _KIND[gdt])
    return g, T(g, dev).to(gdt)


_AKW = dict(beta1_power=0.81, beta2_power=0.998001, lr=0.01)


@pytest.mark.parametrize("gdt", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("mode,lens,B", [("sum", SIX, 300), ("sum", SIX, 37), ("sum", (4,), 300), ("mean", (1, 2, 4), 300)])
def test_pooled_clip_apply_is_the_clipped_apply_on_the_expanded_gradient(dev, mode, lens, B, gdt):
    """Both applies form the same fp32 products: in sum mode (g * mask) * grad_scale on either side; in mean mode with a 0/1 mask,
    power-of-two lengths and grad_scale 1, (g * mask) * (1 / L_f) here and (g * (mask / L_f)) * 1 there.  V = 50 under a few thousand
    positions: every id is a long run -- several windows with partials, the finishing pass."""
    from mindrec_amd import ops
    rng = np.random.default_rng(B + sum(lens) + len(mode))
    V, D = 50, 64
    F, Ls = len(lens), sum(lens)
    n = B * Ls
    ids = CR.ids_with_outsiders(rng, B, Ls, V, np.int64 if B == 37 else np.int32)
    g, tg = _g_rows(rng, B * F, D, gdt, dev)
    masks = _masks(rng, B, Ls)
    rows, f = FR.bag_rows(lens, n)
    if mode == "sum":
        mask, gs = masks[2].reshape(-1), 0.37
        fs, rs_plain, gs_plain = (gs,) * F, mask, gs
    else:
        mask, gs = masks[1].reshape(-1), 1.0
        fs = FR.field_scales(1.0, lens, "mean")
        assert fs == (1.0, 0.5, 0.25)
        tiny = np.finfo(np.float32).tiny                                  # the premise: no product is subnormal
        assert (np.abs(g[g != 0]) * np.float32(min(fs)) >= tiny).all()
        rs_plain, gs_plain = (mask * np.asarray(fs, np.float32)[f]).astype(np.float32), 1.0
    st = _state(rng, CR.special_table(rng, V, D, C))
    ta, tb, tc = ([T(x, dev) for x in st] for _ in range(3))
    plan = ops.sparse_plan(T(ids, dev))
    tg_big = tg[T(rows, dev)].contiguous()
    ops.sparse_lazy_adam_(*ta, plan, tg, T(mask, dev), fields=lens, field_scale=fs, pool_max_norm=C, **_AKW)
    ops.sparse_lazy_adam_(*tb, plan, tg_big, T(rs_plain, dev), grad_scale=gs_plain, max_norm=C, **_AKW)
    _same_t(ta, tb, f"{mode} {lens} {gdt}: table, m, v")
    ops.sparse_lazy_adam_(*tc, plan, tg, T(mask, dev), fields=lens, field_scale=fs, **_AKW)
    assert not torch.equal(ta[0], tc[0]), "the clip must change the update"
    assert not np.array_equal(ta[0].cpu().numpy(), st[0])
    if F == 1:                                                            # pool=L, pool_max_norm=c maps to F = 1
        td = [T(x, dev) for x in st]
        ops.sparse_lazy_adam_(*td, plan, tg, T(mask, dev), pool=lens[0], grad_scale=gs, pool_max_norm=C, **_AKW)
        _same_t(ta, td, "pool=L")


def _row_rel(a, b):
    den = np.maximum(np.abs(b).max(axis=1), 1e-30)
    return float((np.abs(a.astype(np.float64) - b).max(axis=1) / den).max())


@pytest.mark.parametrize("gdt", [torch.float32, torch.bfloat16])
def test_pooled_clip_apply_unequal_lengths_mean_matches_oracle(dev, gdt):
    """Fields (3, 5, 4, 3, 4, 2), mean: the contributions of _pool_fields_ref.contributions through the clip-aware oracle, within the
    bound of test_max_norm_gpu.py::test_sparse_lazy_adam_clip_matches_oracle (1e-5 of a row's largest element, table and first moment).
    The oracle decides |x| > c in float64, the kernel from an fp32 sum of squares (relative error below (log2(D / 4) + 4) * 2^-24 <
    2^-21 at D = 64): for the rows built to lie within a few ulps of c the reference itself does not know the kernel's decision, so
    those rows (at most the 8 of _pool_clip_ref.special_table; checked) are left out of this comparison -- their decision is pinned bit
    for bit by the test above (against the clipped apply) and the test below (forward against backward).  Every other row, the zero
    row and the row of norm exactly c among them, is compared."""
    from mindrec_amd import ops
    rng = np.random.default_rng(17)
    V, D, B, lens = 50, 64, 300, SIX
    F, Ls = len(lens), sum(lens)
    n = B * Ls
    ids = CR.ids_with_outsiders(rng, B, Ls, V, np.int32)
    g, tg = _g_rows(rng, B * F, D, gdt, dev)
    mask = _masks(rng, B, Ls)[2].reshape(-1)
    fs = FR.field_scales(1.0 / 8, lens, "mean")
    tab = CR.special_table(rng, V, D, C)
    p = T(tab, dev); m = torch.zeros_like(p); v = torch.zeros_like(p)
    plan = ops.sparse_plan(T(ids, dev))
    ops.sparse_lazy_adam_(p, m, v, plan, tg, T(mask, dev), fields=lens, field_scale=fs, pool_max_norm=C)
    rp, rm, rv = tab.copy(), np.zeros_like(tab), np.zeros_like(tab)
    u, sums = OC.clipped_sums(rp, ids, FR.contributions(g, lens, n, mask, fs), None, 1.0, C)
    O.sparse_lazy_adam(rp, rm, rv, u, sums, None, grad_scale=1.0)
    nrm = np.linalg.norm(tab.astype(np.float64), axis=1)
    near = np.abs(nrm / C - 1.0) < 2.0 ** -21
    near[CR.TIE_ROW] = False                                              # (exactly c in fp32 and in float64: not clipped by either)
    assert near.sum() <= CR.NEAR1 - CR.NEAR0 and not near[u].all()
    gp, gm = p.cpu().numpy(), m.cpu().numpy()
    print(f"rows: table {_row_rel(gp[~near], rp[~near]):.3e}  m {_row_rel(gm[u][~near[u]], rm[u][~near[u]]):.3e}")
    assert _row_rel(gp[~near], rp[~near]) <= 1e-5
    assert _row_rel(gm[u][~near[u]], rm[u][~near[u]]) <= 1e-5
    n0 = nrm[u]
    assert (n0 > C).sum() > 10 and (n0 <= C).sum() > 10


def test_forward_and_backward_take_the_same_decision(dev):
    """test_max_norm_gpu.py's pattern through MultiHotEmbedding: rows whose fp32 norm lies within a few ulps of c, every bag holds ONE id
    in all of its slots, fields (2, 1, 2), mean -- the pooled row is then the clipped row exactly ((y + y) / 2 = y), and the gradient
    dy = x / 2 of the bag reaches the row as G = x / 2, parallel to it ((x / 4) + (x / 4)).  J(x) annihilates such a G, so the row's
    LazyAdam moment stays at rounding level iff the apply clipped the row -- and that must be iff the lookup clipped it."""
    from mindrec_amd.multi_hot import MultiHotEmbedding
    rng = np.random.default_rng(5)
    lens, D, B, c = (2, 1, 2), 80, 1365, 1.0
    V = 3 * B
    x = rng.standard_normal((V, D))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x = (x * (1.0 + rng.integers(-6, 7, size=(V, 1)) * 2.0 ** -24)).astype(np.float32)
    emb = MultiHotEmbedding(V, D, lens, mode="mean", device=dev, max_norm=c)
    emb.table.copy_(T(x, dev))
    ids = np.repeat(rng.permutation(V).reshape(B, 3), lens, axis=1).astype(np.int32)      # [B, 5]: bag f holds ids[b, f] L_f times
    bag_id = ids[:, [0, 2, 3]].reshape(-1)
    y = emb.lookup(T(ids, dev)).cpu().numpy().reshape(V, D)
    clipped_fwd = np.zeros(V, bool)
    clipped_fwd[bag_id] = (y != x[bag_id]).any(axis=1)
    assert 200 < clipped_fwd.sum() < V - 200                # both decisions occur among the near-ties
    g = (x[bag_id] * np.float32(0.5)).astype(np.float32)
    emb.apply_(T(g.reshape(B, 3 * D), dev))
    mm = np.linalg.norm(emb.m.cpu().numpy().astype(np.float64)[bag_id], axis=1) / (0.1 * np.linalg.norm(g.astype(np.float64), axis=1))
    clipped_bwd = np.zeros(V, bool)
    clipped_bwd[bag_id] = mm < 1e-4
    assert ((mm < 1e-4) | (mm > 0.99)).all()
    assert np.array_equal(clipped_fwd, clipped_bwd), int((clipped_fwd != clipped_bwd).sum())


# ---- 3. the classes ------------------------------------------------------------------------------------------------------------------
def _class_inputs(rng, V, B, lens, D, steps, dev):
    Ls = sum(lens)
    ids = [T(CR.ids_with_outsiders(rng, B, Ls, V, np.int32), dev) for _ in range(steps)]
    masks = [T(_masks(rng, B, Ls)[1 + t % 2], dev) for t in range(steps)]
    targets = [T((rng.standard_normal((B, len(lens) * D)) * 0.05).astype(np.float32), dev) for _ in range(steps)]
    return ids, masks, targets


def _run(emb, ids, masks, targets, dy, outs=None):
    for t in range(len(ids)):
        pooled = emb.lookup(ids[t], masks[t])
        torch.sub(pooled, targets[t], out=dy)
        emb.apply_(dy)
        if outs is not None:
            outs.append(pooled.clone())


@pytest.mark.parametrize("mode,lens,B", [("mean", SIX, 300), ("sum", (4,), 37)])
def test_multi_hot_embedding_max_norm_two_steps_eager_and_captured(dev, mode, lens, B):
    from mindrec_amd import ops
    from mindrec_amd.multi_hot import MultiHotEmbedding
    rng = np.random.default_rng(B)
    V, D, steps, F = 50, 64, 2, len(lens)
    tab = T(CR.special_table(rng, V, D, C), dev)
    ids, masks, targets = _class_inputs(rng, V, B, lens, D, steps, dev)
    kw = dict(mode=mode, device=dev, lr=0.01, max_norm=C)
    # the ops calls
    p, m, v = tab.clone(), torch.zeros_like(tab), torch.zeros_like(tab)
    b1p, b2p = np.float32(1.0), np.float32(1.0)
    ref_out = []
    for t in range(steps):
        pooled = ops.gather_pool_fields(p, ids[t], lens, masks[t], mode=mode, max_norm=C)
        ref_out.append(pooled.clone())
        dy = pooled - targets[t]
        b1p, b2p = np.float32(b1p * np.float32(0.9)), np.float32(b2p * np.float32(0.999))
        ops.sparse_lazy_adam_(p, m, v, ops.sparse_plan(ids[t]), dy.view(B * F, D), masks[t], lr=0.01, beta1_power=float(b1p),
                              beta2_power=float(b2p), fields=lens, field_scale=FR.field_scales(1.0, lens, mode), pool_max_norm=C)
    eager = MultiHotEmbedding(V, D, lens, **kw)
    assert eager.max_norm == C
    eager.table.copy_(tab)
    outs = []
    _run(eager, ids, masks, targets, torch.empty((B, F * D), dtype=torch.float32, device=dev), outs)
    _same_t(outs, ref_out, "pooled rows")
    _same_t((eager.table, eager.m, eager.v), (p, m, v), "eager vs the ops calls")
    plain = MultiHotEmbedding(V, D, lens, mode=mode, device=dev, lr=0.01)
    plain.table.copy_(tab)
    _run(plain, ids, masks, targets, torch.empty((B, F * D), dtype=torch.float32, device=dev))
    assert not torch.equal(plain.table, eager.table)
    cap = MultiHotEmbedding(V, D, lens, **kw)
    cap.table.copy_(tab)
    dyc = torch.empty((B, F * D), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _run(cap, ids, masks, targets, dyc)
    torch.cuda.synchronize()
    assert torch.equal(cap.table, tab)                                    # (capture ran nothing)
    graph.replay()
    torch.cuda.synchronize()
    _same_t((cap.table, cap.m, cap.v), (p, m, v), "captured vs the ops calls")


def test_multi_hot_wide_deep_max_norm_clips_the_deep_half_only(dev):
    from mindrec_amd import ops
    from mindrec_amd.multi_hot import MultiHotEmbedding, MultiHotWideDeep
    rng = np.random.default_rng(8)
    V, D, B, lens, steps = 50, 64, 300, SIX, 2
    F = len(lens)
    tab = T(CR.special_table(rng, V, D, C), dev)
    wtab = T((rng.standard_normal((V, 1)) * 5).astype(np.float32), dev)      # wide weights far above c: never clipped
    ids, masks, targets = _class_inputs(rng, V, B, lens, D, steps, dev)
    dws = [T(rng.standard_normal(B).astype(np.float32), dev) for _ in range(steps)]
    kw = dict(mode="mean", device=dev, lr=0.01)
    pair, pair0 = MultiHotWideDeep(V, D, lens, max_norm=C, **kw), MultiHotWideDeep(V, D, lens, **kw)
    deep = MultiHotEmbedding(V, D, lens, max_norm=C, **kw)
    assert pair.deep.max_norm == C and pair.wide.max_norm is None
    for e in (pair.deep, pair0.deep, deep):
        e.table.copy_(tab)
    for e in (pair.wide, pair0.wide):
        e.table.copy_(wtab)
    for t in range(steps):
        x, w = pair.lookup(ids[t], masks[t])
        x0, w0 = pair0.lookup(ids[t], masks[t])
        xd = deep.lookup(ids[t], masks[t])
        _same_t((w, x), (w0, xd), f"step {t}: wide sums / deep rows")
        assert not torch.equal(x, x0)
        dy = x - targets[t]
        plan = pair.apply_(dy, dws[t])
        pair0.apply_(dy, dws[t])
        deep.apply_(dy, plan=ops.sparse_plan(ids[t]))
        assert plan.n == B * sum(lens)
        _same_t((pair.wide.table,) + tuple(pair.wide.state), (pair0.wide.table,) + tuple(pair0.wide.state), f"step {t}: the wide half")
        _same_t((pair.deep.table,) + tuple(pair.deep.state), (deep.table,) + tuple(deep.state), f"step {t}: the deep half")
    assert not torch.equal(pair.deep.table, pair0.deep.table) and not torch.equal(pair.wide.table, wtab)


def _distinct_keys(rng, n, kdt):
    lo, hi = (-2 ** 30, 2 ** 30) if kdt == torch.int32 else (-2 ** 40, 2 ** 40)
    k = np.unique(rng.integers(lo, hi, size=4 * n))
    assert k.size >= n
    return rng.permutation(k)[:n].astype(_NP[kdt])


def _new_map(dev, kdt, D, default, capacity=1024, **kw):
    from mindrec_amd.experimental import MapParameter
    return MapParameter(key_dtype=kdt, value_shape=D, default_value=default, capacity=capacity, device=dev, seed=11, **kw)


@pytest.mark.parametrize("kdt", [torch.int32, torch.int64])
@pytest.mark.parametrize("D,lens", [(8, SIX), (64, (9,)), (12, (2, 1))])
def test_hash_probe_lookup_clips_default_rows_too(dev, D, lens, kdt):
    """train=False against MapParameter.get(insert_default_value=False) on a twin map, its [n, D] rows clipped by
    ops.gather_rows(max_norm=c) and pooled on the host.  The default value is the constant 0.5: a default row's norm 0.5 * sqrt(D) is
    above c = 0.75 at every D here, so a missing key's row must come out clipped."""
    from mindrec_amd import ops
    from mindrec_amd.multi_hot import MultiHotHashEmbedding
    rng = np.random.default_rng(100 * D + sum(lens))
    B, F, Ls, R, fill = 37, len(lens), sum(lens), 50, 0.5
    assert fill * np.sqrt(D) > C
    allk = _distinct_keys(rng, 2 * R, kdt)
    res, fresh = allk[:R], allk[R:]
    vals = CR.special_table(rng, R, D, C)
    m, twin = (_new_map(dev, kdt, D, fill) for _ in range(2))
    for t in (m, twin):
        t.put(T(res, dev), T(vals, dev))
    embs = {mode: MultiHotHashEmbedding(m, bag=lens, mode=mode, max_norm=C) for mode in ("sum", "mean")}
    plain = MultiHotHashEmbedding(m, bag=lens, mode="sum")
    for frac in (0.0, 0.5, 1.0):
        miss = rng.random((B, Ls)) < frac
        keys = np.where(miss, rng.choice(fresh, size=(B, Ls)), rng.choice(res, size=(B, Ls))).astype(_NP[kdt])
        tk = T(keys, dev)
        rows_e = twin.get(tk.reshape(-1), insert_default_value=False)                       # [B * Ls, D]: the existing path
        n = rows_e.shape[0]
        rows_c = ops.gather_rows(rows_e, torch.arange(n, dtype=torch.int32, device=dev), max_norm=C).cpu().numpy()
        if frac > 0:
            dflt = rows_c[miss.reshape(-1)]
            assert np.allclose(np.linalg.norm(dflt.astype(np.float64), axis=1), C, rtol=1e-6) and (dflt != fill).all()
        for mask in _masks(rng, B, Ls):
            tm = T(mask, dev) if mask is not None else None
            for mode in ("sum", "mean"):
                for odt in (torch.float32, torch.bfloat16):
                    what = f"D={D} fields={lens} {kdt} missing={frac} {mode} {odt} mask={mask is not None}"
                    out = torch.empty((B, F * D), dtype=odt, device=dev)
                    got = embs[mode].lookup(tk, tm, out=out, train=False)
                    _same(_bits(got), CR.clipped_pool(rows_c, B, lens, mask, mode, _KIND[odt]), what)
        assert not torch.equal(plain.lookup(tk, train=False), embs["sum"].lookup(tk, train=False))
    assert len(m) == R and m.step == 0                                    # probes change nothing


def test_hash_training_two_steps_against_the_dense_sibling(dev):
    """lookup(train=True) + apply_ under max_norm against MultiHotEmbedding(max_norm=c) over CLONES of map.values and the slot tables
    and the admitted row numbers, as tests/test_pool_hash_gpu.py does without the clip.  New keys read the default row 0.5 (norm
    0.5 * sqrt(8) > c: clipped in the forward, and updated through the Jacobian); step 2 brings more new keys."""
    from mindrec_amd.multi_hot import MultiHotEmbedding, MultiHotHashEmbedding
    rng = np.random.default_rng(21)
    kdt, D, lens, B, fill = torch.int64, 8, SIX, 37, 0.5
    F, Ls = len(lens), sum(lens)
    pool = _distinct_keys(rng, 120, kdt)
    m, twin = _new_map(dev, kdt, D, fill), _new_map(dev, kdt, D, fill)
    res = pool[:40]
    vals = CR.special_table(rng, res.size, D, C)
    for t in (m, twin):
        t.put(T(res, dev), T(vals, dev))
    emb = MultiHotHashEmbedding(m, bag=lens, mode="mean", lr=0.05, max_norm=C)
    dense = MultiHotEmbedding(m.capacity, D, lens, mode="mean", device=dev, lr=0.05, max_norm=C)
    keys = [rng.choice(pool[:80], size=(B, Ls)), rng.choice(pool, size=(B, Ls))]
    keys[0][:, lens[0]] = keys[0][:, 0]                                    # a key in two fields of one sample: one update
    tm = T(_masks(rng, B, Ls)[2], dev)
    for s in range(2):
        tk = T(keys[s], dev)
        x = emb.lookup(tk, tm, train=True)
        dense.table.copy_(m.values)
        for dst, name in zip(dense.state, ("moment1", "moment2")):
            dst.copy_(m.slots[name]["table"])
        before = m.values.clone()
        xd = dense.lookup(m.lookup_rows(tk.reshape(-1), insert=False)[2].view(B, Ls), tm)      # every key holds a row by now
        _same_t((x,), (xd,), f"step {s + 1}: lookup")
        dense.lookup(emb.rows, tm)
        dy = T(rng.standard_normal((B, F * D)).astype(np.float32), dev)
        emb.apply_(dy)
        dense.apply_(dy)
        assert (emb.beta1_power, emb.beta2_power) == (dense.beta1_power, dense.beta2_power)
        _same_t((m.values, m.slots["moment1"]["table"], m.slots["moment2"]["table"]), (dense.table,) + tuple(dense.state), f"step {s + 1}")
        assert bool((m.values != before).any())
    assert emb.step_count == 2                                            # (m.step counts training lookups only under a filter)


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------
def _refusal_case(dev, D, lens=(3, 5, 4), B=300, V=50):
    from mindrec_amd import ops
    rng = np.random.default_rng(D)
    F, Ls = len(lens), sum(lens)
    tab = (rng.standard_normal((V, D)) * C / np.sqrt(D)).astype(np.float32)
    st = _state(rng, tab)
    ids = T(rng.integers(0, V, size=(B, Ls)).astype(np.int32), dev)
    tgs, tgb = T(rng.standard_normal((B * F, D)).astype(np.float32), dev), T(rng.standard_normal((B * Ls, D)).astype(np.float32), dev)
    return st, ids, ops.sparse_plan(ids), tgs, tgb


def _untouched(ts, st):
    torch.cuda.synchronize()
    for t, a in zip(ts, st):
        assert np.array_equal(t.cpu().numpy().view(np.uint32), a.view(np.uint32))


@pytest.mark.parametrize("D", [6, 260])
def test_widths_the_clip_cannot_run_at_are_refused(dev, D):
    from mindrec_amd import _lib, ops
    from mindrec_amd.multi_hot import MultiHotEmbedding
    lens = (3, 5, 4)
    st, ids, plan, tgs, tgb = _refusal_case(dev, D, lens)
    B, F = ids.shape[0], len(lens)
    never = [T(a, dev) for a in st]
    ops.sparse_lazy_adam_(*never, plan, tgb)
    ts = [T(a, dev) for a in st]
    out0 = np.full((B, F * D), 7.0, np.float32)
    out = T(out0, dev)
    with pytest.raises(_lib.MrecError) as e:
        ops.gather_pool_fields(ts[0], ids, lens, mode="mean", out=out, max_norm=C)
    assert e.value.code == -3
    _untouched([out], [out0])
    with pytest.raises(_lib.MrecError) as e:
        ops.sparse_lazy_adam_(*ts, plan, tgs, fields=lens, pool_max_norm=C)
    assert e.value.code == -3
    _untouched(ts, st)
    ops.sparse_lazy_adam_(*ts, plan, tgb)                                  # ... and disarmed: the never-armed call
    _same_t(ts, never, "the next plain call")
    with pytest.raises(ValueError, match="max_norm"):
        MultiHotEmbedding(50, D, lens, device=dev, max_norm=C)


def test_clip_arm_refusals_launch_nothing_and_disarm(dev, monkeypatch):
    """an FTRL apply, a segment sum and the folded wide forms under the pooled clip's record, invalid max_norm values, and the old
    max_norm= + fields= combination: tables untouched, and the next plain call is the plain call.  ops gives these calls no such
    record: they are handed it (mrec_apply_opts_t) here."""
    from mindrec_amd import _lib, ops
    import ctypes
    lens, D = (3, 5, 4), 64
    st, ids, plan, tgs, tgb = _refusal_case(dev, D, lens)
    F = len(lens)
    n = plan.n

    def clipped(fn, *args, c=C, **kwargs):
        rec = ops.ApplyOpts(n_fields=F, field_len=(ctypes.c_int32 * F)(*lens), field_scale=(ctypes.c_float * F)(1.0, 1.0, 1.0), max_norm=c)
        with monkeypatch.context() as mp:
            mp.setattr(ops, "_opts_ptr", lambda _: ctypes.byref(rec))
            return fn(*args, **kwargs)

    never = [T(a, dev) for a in st]
    ops.sparse_lazy_adam_(*never, plan, tgb)

    def plain_is_plain(ts):
        ops.sparse_lazy_adam_(*ts, plan, tgb)
        _same_t(ts, never, "the next plain call")

    # FTRL
    fst = [st[0], (np.abs(st[1]) + 0.5).astype(np.float32), st[2]]
    fnever = [T(a, dev) for a in fst]
    ops.sparse_ftrl_(*fnever, plan, tgb)
    ts = [T(a, dev) for a in fst]
    with pytest.raises(_lib.MrecError) as e:
        clipped(ops.sparse_ftrl_, *ts, plan, tgb)
    assert e.value.code == -3
    _untouched(ts, fst)
    ops.sparse_ftrl_(*ts, plan, tgb)
    _same_t(ts, fnever, "the next plain FTRL call")
    # a segment sum
    with pytest.raises(_lib.MrecError) as e:
        clipped(ops.segment_sum, plan, tgb)
    assert e.value.code == -3
    plain_is_plain([T(a, dev) for a in st])
    # the folded wide apply (fused rows [p | w accum linear pad | m | v | pad]), launched and deferred
    rng = np.random.default_rng(7)
    FW = sum(lens)
    ld = -(-(3 * D + 4) // 32) * 32
    buf = (rng.standard_normal((50, ld)) * 0.01).astype(np.float32)
    buf[:, D + 1] = 1.0 + rng.random(50).astype(np.float32)
    buf[:, 2 * D + 4:3 * D + 4] = np.abs(buf[:, 2 * D + 4:3 * D + 4]) * 1e-3
    gw = T(rng.standard_normal(n // FW).astype(np.float32), dev)
    trs = T((rng.random(n) + 0.25).astype(np.float32), dev)

    def wide(tb, **extra):
        return ops.sparse_lazy_adam_wide_(tb[:, :D], tb[:, D + 4:2 * D + 4], tb[:, 2 * D + 4:3 * D + 4], plan, tgb, trs, gw, FW, D, **extra)

    wnever = T(buf, dev)
    wide(wnever)
    for defer in (False, True):
        tb = T(buf, dev)
        with pytest.raises(_lib.MrecError) as e:
            clipped(wide, tb, defer=defer)
        assert e.value.code == -3
        _untouched([tb], [buf])
        wide(tb)                                                           # plain again
        assert torch.equal(tb.view(torch.int32), wnever.view(torch.int32))
    # max_norm values that are none
    for c in (0.0, -1.0, float("inf"), float("nan")):
        ts = [T(a, dev) for a in st]
        with pytest.raises(ValueError):
            ops.sparse_lazy_adam_(*ts, plan, tgs, fields=lens, pool_max_norm=c)
        with pytest.raises(ValueError):
            ops.gather_pool_fields(ts[0], ids, lens, max_norm=c)
        if c != 0.0:                                                       # (in the record itself, 0.0 is "no clip")
            with pytest.raises(_lib.MrecError) as e:
                clipped(ops.sparse_lazy_adam_, *ts, plan, tgs, fields=lens, c=c)
            assert e.value.code == -1
        _untouched(ts, st)
        plain_is_plain(ts)
    # the old combination: max_norm= with fields=, still MREC_EUNSUPPORTED
    ts = [T(a, dev) for a in st]
    with pytest.raises(_lib.MrecError) as e:
        ops.sparse_lazy_adam_(*ts, plan, tgs, fields=lens, max_norm=C)
    assert e.value.code == -3
    _untouched(ts, st)
    plain_is_plain(ts)
    # ... and with the clip arm under it
    ts = [T(a, dev) for a in st]
    with pytest.raises(_lib.MrecError) as e:
        ops.sparse_lazy_adam_(*ts, plan, tgs, fields=lens, pool_max_norm=C, max_norm=C)
    assert e.value.code == -3
    _untouched(ts, st)
    plain_is_plain(ts)
