"""max_norm (HashEmbeddingLookup / nn.EmbeddingLookup(max_norm=c): ClipByNorm of every looked-up row, mindspore_rec/ops/
embedding.py:156-161,202-205) on the GPU: the clip variants of the lookup kernels against a float64 restatement, the sparse apply's
Jacobian against the clip-aware oracle (tests/_oracle_clip_ops.py), one clip decision per row in the forward and the backward, the
engine against the oracle engine, bitwise agreements across the engine's code paths, and the lowering of a compat cell."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _oracle_clip_ops as OC  # noqa: E402


def row_rel(a, b):
    den = np.maximum(np.abs(b).max(axis=1), 1e-30)
    return float((np.abs(a.astype(np.float64) - b).max(axis=1) / den).max())


def _rows(rng, V, D, c):
    """rows whose norms are far above c, just below it, exactly zero, and ordinary ones"""
    t = rng.standard_normal((V, D)).astype(np.float32)
    t /= np.linalg.norm(t.astype(np.float64), axis=1, keepdims=True).astype(np.float32)
    scale = rng.choice([100.0, 3.0, 0.999, 0.5, 0.0], size=V).astype(np.float32)
    return (t * scale[:, None] * np.float32(c)).astype(np.float32)


_ULP = {torch.float32: 2.0 ** -23, torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
_TINY = {torch.float32: 1e-30, torch.bfloat16: 1e-30, torch.float16: 2.0 ** -24}        # (one ulp of IEEE half's subnormals)


@pytest.mark.parametrize("D", [16, 80, 252])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("id_dtype", [torch.int32, torch.int64])
def test_gather_clip_matches_float64_restatement(dev, D, out_dtype, id_dtype):
    from mindrec_amd import ops
    rng = np.random.default_rng(D)
    V, n, c = 3000, 4096, 0.75
    tab = _rows(rng, V, D, c)
    ids = rng.integers(-50, V + 50, size=n)                          # a few ids outside [0, V): zero rows, never clipped
    wts = rng.random(n).astype(np.float32)
    t = torch.from_numpy(tab).to(dev)
    got = ops.gather_rows(t, torch.from_numpy(ids).to(dev).to(id_dtype), torch.from_numpy(wts).to(dev), out_dtype=out_dtype,
                          max_norm=c).float().cpu().numpy()
    ref = OC.gather_rows(torch.from_numpy(tab), torch.from_numpy(ids), torch.from_numpy(wts), max_norm=c).numpy().astype(np.float64)
    ok = (ids >= 0) & (ids < V)
    assert np.array_equal(got[~ok], np.zeros_like(got[~ok]))
    # one ulp of the output type plus the fp32 norm's rounding (a few ulps of fp32 on c / n and the two multiplies)
    tol = np.abs(ref) * (_ULP[out_dtype] + 8 * 2.0 ** -24) + _TINY[out_dtype]
    assert (np.abs(got - ref) <= tol).all(), float((np.abs(got - ref) / np.maximum(np.abs(ref), 1e-30)).max())
    # the rows far above c came out at norm c (times the mask), the rows below untouched
    nrm = np.linalg.norm(tab[np.where(ok, ids, 0)].astype(np.float64), axis=1)
    assert ((nrm > 2 * c) & ok).sum() > 100 and ((nrm < 0.9999 * c) & (nrm > 0) & ok).sum() > 100
    # without max_norm: the plain lookup
    plain = ops.gather_rows(t, torch.from_numpy(ids).to(dev).to(id_dtype), torch.from_numpy(wts).to(dev), out_dtype=out_dtype)
    assert not torch.equal(plain.float().cpu(), torch.from_numpy(got))


@pytest.mark.parametrize("n", [4096, 4094])      # the 16-byte-store form (n % 4 == 0) and the plain one
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float16])
def test_gather_wide_clip(dev, n, out_dtype):
    """The fused-row lookup: the deep columns clipped, the wide word (column D of the same rows) not."""
    from mindrec_amd import ops
    rng = np.random.default_rng(n)
    V, D, c = 2000, 80, 0.5
    ld = 3 * D + 4
    buf = np.zeros((V, ld), np.float32)
    buf[:, :D] = _rows(rng, V, D, c)
    buf[:, D] = rng.standard_normal(V).astype(np.float32) * 5          # the wide weight: far above c, never clipped
    ids = rng.integers(0, V, size=n).astype(np.int32)
    wts = rng.random(n).astype(np.float32)
    b = torch.from_numpy(buf).to(dev)
    emb, wprod = ops.gather_rows_wide(b[:, :D], torch.from_numpy(ids).to(dev), torch.from_numpy(wts).to(dev), D, out_dtype=out_dtype,
                                      max_norm=c)
    ref = OC.gather_rows(torch.from_numpy(buf[:, :D].copy()), torch.from_numpy(ids), torch.from_numpy(wts), max_norm=c).numpy()
    tol = np.abs(ref) * (_ULP[out_dtype] + 8 * 2.0 ** -24) + _TINY[out_dtype]
    assert (np.abs(emb.float().cpu().numpy() - ref) <= tol).all()
    assert np.array_equal(wprod[:, 0].cpu().numpy(), buf[ids, D] * wts)


def _plan_and_grads(rng, dev, V, D, B, F, zipf=True):
    from mindrec_amd import ops
    if zipf:
        ids = np.minimum(rng.zipf(1.2, size=(B, F)) - 1, V - 1).astype(np.int32)
    else:
        ids = rng.integers(0, V, size=(B, F)).astype(np.int32)
    ids[:, 0] = 7                                        # one id in every sample: a run over many windows (the finishing pass)
    wts = rng.random((B, F)).astype(np.float32)
    g = (rng.standard_normal((B * F, D)) * 0.5).astype(np.float32)
    tid = torch.from_numpy(ids).to(dev)
    return ids, wts, g, tid, ops.sparse_plan(tid)


@pytest.mark.parametrize("g_dtype", [torch.float32, torch.bfloat16])
def test_sparse_lazy_adam_clip_matches_oracle(dev, g_dtype):
    from mindrec_amd import ops
    from oracle import oracle as O
    rng = np.random.default_rng(3)
    V, D, B, F, c = 5000, 80, 512, 26, 0.09
    tab = (rng.standard_normal((V, D)) * 0.01).astype(np.float32)          # norms around 0.09: both branches
    ids, wts, g, tid, plan = _plan_and_grads(rng, dev, V, D, B, F)
    g = torch.from_numpy(g).to(g_dtype).float().numpy()                     # what the kernel sees after widening
    p = torch.from_numpy(tab).to(dev); m = torch.zeros_like(p); v = torch.zeros_like(p)
    ops.sparse_lazy_adam_(p, m, v, plan, torch.from_numpy(g).to(dev).to(g_dtype), torch.from_numpy(wts).to(dev), grad_scale=1 / 1024,
                          max_norm=c)
    rp, rm, rv = tab.copy(), np.zeros_like(tab), np.zeros_like(tab)
    u, sums = OC.clipped_sums(rp, ids, g, wts, 1 / 1024, c)
    O.sparse_lazy_adam(rp, rm, rv, u, sums, None, grad_scale=1.0)
    assert row_rel(p.cpu().numpy(), rp) <= 1e-5
    assert row_rel(m.cpu().numpy()[u], rm[u]) <= 1e-5
    n0 = np.linalg.norm(tab[u].astype(np.float64), axis=1)
    assert (n0 > c).sum() > 50 and (n0 <= c).sum() > 50


@pytest.mark.parametrize("defer", [False, True])
def test_sparse_lazy_adam_wide_clip_matches_oracle(dev, defer):
    """The fold-wide apply (LazyAdam on the deep columns + FTRL on the wide record of the same fused rows): the deep columns against
    the clip-aware oracle, the wide record bit for bit what the apply without max_norm leaves (FTRL is not clipped)."""
    from mindrec_amd import ops
    from oracle import oracle as O
    rng = np.random.default_rng(4)
    V, D, B, F, c = 5000, 80, 512, 26, 0.09
    ld = 3 * D + 4
    buf0 = np.zeros((V, ld), np.float32)
    buf0[:, :D] = (rng.standard_normal((V, D)) * 0.01).astype(np.float32)
    buf0[:, D] = (rng.standard_normal(V) * 0.01).astype(np.float32)
    buf0[:, D + 1] = 1.0
    ids, wts, g, tid, plan = _plan_and_grads(rng, dev, V, D, B, F)
    gw = (rng.standard_normal(B) * 0.3).astype(np.float32)
    out = []
    for mn in (c, None):
        b = torch.from_numpy(buf0).to(dev)
        p, m, v = b[:, :D], b[:, D + 4:2 * D + 4], b[:, 2 * D + 4:]
        fin = ops.sparse_lazy_adam_wide_(p, m, v, plan, torch.from_numpy(g).to(dev), torch.from_numpy(wts).to(dev), torch.from_numpy(gw).to(dev),
                                         F, D, grad_scale=1 / 1024, defer=defer, max_norm=mn)
        if defer:
            z = torch.zeros(4, dtype=torch.float32, device=dev)
            ops.dense_adam_slabs_(z, torch.zeros_like(z), torch.zeros_like(z), torch.zeros_like(z), [], finish=fin)
        out.append(b.cpu().numpy())
    got, plain = out
    rp, rm, rv = buf0[:, :D].copy(), np.zeros((V, D), np.float32), np.zeros((V, D), np.float32)
    u, sums = OC.clipped_sums(rp, ids, g, wts, 1 / 1024, c)
    O.sparse_lazy_adam(rp, rm, rv, u, sums, None, grad_scale=1.0)
    assert row_rel(got[:, :D], rp) <= 1e-5
    assert row_rel(got[u, D + 4:2 * D + 4], rm[u]) <= 1e-5
    assert np.array_equal(got[:, D:D + 4], plain[:, D:D + 4])          # the wide record: untouched by the clip
    assert not np.array_equal(got[:, :D], plain[:, :D])


def test_forward_and_backward_take_the_same_decision(dev):
    """Rows whose fp32 norm lies within a few ulps of c, gradients parallel to the row (G = a x): J(x) annihilates such a G, so a
    row's LazyAdam moment stays at rounding level iff the apply clipped the row -- and that must be iff the lookup clipped it."""
    from mindrec_amd import ops
    rng = np.random.default_rng(5)
    V, D, c = 4096, 80, 1.0
    x = rng.standard_normal((V, D))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    x = (x * (1.0 + rng.integers(-6, 7, size=(V, 1)) * 2.0 ** -24)).astype(np.float32)
    p = torch.from_numpy(x).to(dev)
    ids = np.arange(V, dtype=np.int32)
    tid = torch.from_numpy(ids).to(dev)
    y = ops.gather_rows(p, tid, max_norm=c).cpu().numpy()
    clipped_fwd = (y != x).any(axis=1)
    assert 200 < clipped_fwd.sum() < V - 200                # both decisions occur among the near-ties
    g = (x * np.float32(0.5)).astype(np.float32)
    plan = ops.sparse_plan(tid)
    m = torch.zeros_like(p); v = torch.zeros_like(p)
    ops.sparse_lazy_adam_(p, m, v, plan, torch.from_numpy(g).to(dev), max_norm=c)
    mm = np.linalg.norm(m.cpu().numpy().astype(np.float64), axis=1) / (0.1 * np.linalg.norm(g.astype(np.float64), axis=1))
    clipped_bwd = mm < 1e-4
    assert ((mm < 1e-4) | (mm > 0.99)).all()
    assert np.array_equal(clipped_fwd, clipped_bwd), int((clipped_fwd != clipped_bwd).sum())


def test_engine_matches_oracle_engine_with_max_norm(dev, oracle):
    from _oracle_engine import OracleWideDeepEngine
    from mindrec_amd.wide_deep import WideDeepConfig, WideDeepEngine, synthetic_batch
    import _oracle_clip_ops

    class OracleClipEngine(OracleWideDeepEngine):
        _kernels = _oracle_clip_ops

    c = 0.09                                              # about the median initial row norm (0.01 * sqrt(80))
    cfg = WideDeepConfig(vocab_size=50_000, emb_dim=80, field_size=39, batch_size=256, deep_layer_dim=[64, 32], mlp_dtype="fp32",
                         max_norm=c)
    g = WideDeepEngine(cfg, dev)
    o = OracleClipEngine(cfg, "cpu")
    d0 = o.deep.numpy().copy()
    for s in range(3):
        ids, wts, label = synthetic_batch(cfg, "cpu", "zipf", seed=7 + s)
        if s == 0:
            n0 = np.linalg.norm(d0[np.unique(ids.numpy())].astype(np.float64), axis=1)
            assert (n0 > c).sum() > 100 and (n0 <= c).sum() > 100
        lc = float(o.train_step(ids, wts, label))
        lg = float(g.train_step(ids.to(dev), wts.to(dev), label.to(dev)))
        assert abs(lc - lg) <= 1e-5 * max(abs(lc), 1e-3)
    assert row_rel(g.deep.cpu().numpy(), o.deep.numpy()) <= 2e-5
    untouched = (o.deep_m.numpy() == 0).all(axis=1)
    assert np.array_equal(g.deep.cpu().numpy()[untouched], o.deep.numpy()[untouched])
    # evaluation sees clipped rows too
    ids, wts, _ = synthetic_batch(cfg, "cpu", "zipf", seed=99)
    lo, _ = o.predict(ids, wts)
    lg, _ = g.predict(ids.to(dev), wts.to(dev))
    assert np.allclose(lg.cpu().numpy(), lo.numpy(), rtol=1e-4, atol=1e-6)


def _run(cfg, dev, steps=3, seed=11):
    from mindrec_amd.wide_deep import WideDeepEngine, synthetic_batch
    e = WideDeepEngine(cfg, dev)
    losses = []
    for s in range(steps):
        ids, wts, label = synthetic_batch(cfg, dev, "zipf", seed=seed + s)
        losses.append(float(e.train_step(ids, wts, label)))
    return e, losses


def _small(**kw):
    from mindrec_amd.wide_deep import WideDeepConfig
    base = dict(vocab_size=20_000, emb_dim=80, field_size=26, batch_size=1024, deep_layer_dim=[128, 64], mlp_dtype="fp16")
    base.update(kw)
    return WideDeepConfig(**base)


def test_engine_max_norm_bitwise_across_paths(dev):
    """With max_norm: the captured step equals kernel-by-kernel launches, hash tables equal dense ones (the keys of a fresh
    table are numbered in first-seen order, so the rows are compared through the key index), and max_norm = 1e30 (never
    clipped) equals max_norm = None."""
    c = 0.09
    a, la = _run(_small(max_norm=c, graphs="step"), dev)
    b, lb = _run(_small(max_norm=c, graphs="none"), dev)
    assert la == lb and torch.equal(a.deep, b.deep) and torch.equal(a.deep_m, b.deep_m)
    h, lh = _run(_small(max_norm=c, graphs="none", dynamic_embedding=True, hash_capacity=1 << 15, const_columns=False), dev)
    d, ld = _run(_small(max_norm=c, graphs="none", const_columns=False), dev)
    assert lh == ld
    keys = torch.arange(20_000, dtype=torch.int32, device=dev)
    rows = h.index.lookup(keys, insert=False)
    seen = rows >= 0
    assert int(seen.sum()) > 1000
    assert torch.equal(h.deep[rows[seen].long()], d.deep[keys[seen].long()])
    x, lx = _run(_small(max_norm=1e30, const_columns=False), dev)
    y, ly = _run(_small(const_columns=False), dev)
    assert lx == ly and torch.equal(x.deep, y.deep) and torch.equal(x.deep_m, y.deep_m)


# ---- lowering -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def ms_hip(dev):
    compat = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "compat"))
    if compat not in sys.path:
        sys.path.insert(0, compat)
    import mindspore
    from mindspore import context
    from mindspore import _hip_kernels
    prev = mindspore._kernels._install(_hip_kernels)
    context.set_context(mode=context.GRAPH_MODE, device_target="GPU", device_id=0)
    yield mindspore
    context.set_context(mode=context.GRAPH_MODE)
    mindspore._kernels._install(prev)


def _clip_cell(ms, wide_max_norm=None, deep_max_norm=None):
    import _ms_models
    from mindspore import nn
    V, D, F, B = 3000, 8, 9, 64

    class WideDeepClip(_ms_models.WideDeep):
        def __init__(self):
            super().__init__(V, D, F, B, [32, 16], True, False)
            if deep_max_norm is not None:
                self.deep_table = nn.EmbeddingLookup(V, D, target="DEVICE", sparse=True, max_norm=deep_max_norm)
                self.table = self.deep_table.embedding_table
            if wide_max_norm is not None:
                self.wide_table = nn.EmbeddingLookup(V, 1, target="DEVICE", sparse=True, max_norm=wide_max_norm)

    ms.set_seed(1000)
    net = WideDeepClip()
    step = _ms_models.WideDeepTrainStep(_ms_models.WideDeepLoss(net, 8e-5, False), lazy=True)
    step.set_train()
    return step, net


def test_lowered_cell_with_max_norm_matches_pynative(ms_hip):
    """A compat Wide&Deep cell whose deep lookup has max_norm: GRAPH_MODE lowers it to the engine (kind wide_deep) and trains it
    like the same cell run primitive by primitive, over steps in which rows cross the bound."""
    from mindspore import context
    from mindrec_amd.lowering import LoweredStep
    c = 0.03                                   # between the median (0.027) and the 90th percentile of the initial row norms
    rng = np.random.default_rng(8)
    batches = [(rng.integers(0, 3000, size=(64, 9)).astype(np.int32), rng.random((64, 9)).astype(np.float32),
                (rng.random((64, 1)) < 0.3).astype(np.float32)) for _ in range(8)]
    for ids, _, _ in batches:
        ids[:, :8] = np.arange(5, 13)              # rows 5..12 in every sample: they move ~1e-3 per step ...
    step_g, net_g = _clip_cell(ms_hip, deep_max_norm=c)
    step_p, net_p = _clip_cell(ms_hip, deep_max_norm=c)
    d0 = net_g.deep_table.embedding_table.asnumpy().copy()
    u = d0[5:13] / np.linalg.norm(d0[5:13].astype(np.float64), axis=1, keepdims=True)
    d0[5:13] = u * (c * (1.0 + 1e-4 * np.array([-1, 1] * 4)))[:, None]        # ... from a norm within 1e-4 of the bound
    net_g.deep_table.embedding_table.set_data(ms_hip.Tensor(d0.astype(np.float32)))
    for a, b in zip(net_g.trainable_params(), net_p.trainable_params()):
        b.set_data(ms_hip.Tensor(a.asnumpy()))
    d0 = net_p.deep_table.embedding_table.asnumpy().copy()
    model = ms_hip.Model(step_g)
    lg = []
    for ids, wts, label in batches:
        lw, ld = model._run_step(step_g, tuple(ms_hip.Tensor(t) for t in (ids, wts, label)))
        lg.append((float(lw.asnumpy()), float(ld.asnumpy())))
    low = step_g.__dict__.get("_lowered")
    assert isinstance(low, LoweredStep) and low.kind == "wide_deep", step_g.__dict__.get("_lowering_refused")
    assert low.engine.cfg.max_norm == pytest.approx(c)
    context.set_context(mode=context.PYNATIVE_MODE)
    lp = []
    for ids, wts, label in batches:
        lw, ld = step_p(ms_hip.Tensor(ids), ms_hip.Tensor(wts), ms_hip.Tensor(label))
        lp.append((float(lw.asnumpy()), float(ld.asnumpy())))
    assert np.allclose(np.array(lg), np.array(lp), rtol=2e-6, atol=0), (lg, lp)
    dg, dp = net_g.deep_table.embedding_table.asnumpy(), net_p.deep_table.embedding_table.asnumpy()
    assert row_rel(dg, dp) <= 1e-5
    touched = np.unique(np.concatenate([b[0].reshape(-1) for b in batches]))
    n0 = np.linalg.norm(d0[touched].astype(np.float64), axis=1)
    n1 = np.linalg.norm(dp[touched].astype(np.float64), axis=1)
    assert ((n0 <= c) & (n1 > c)).sum() + ((n0 > c) & (n1 <= c)).sum() > 0        # rows crossed the bound during training
    assert (n0 > c).sum() > 50


def test_lowered_hash_table_cell_with_max_norm_matches_pynative(ms_hip, monkeypatch):
    """The same over the issue's own layer: two HashEmbeddingLookups over MapParameters, the deep one with max_norm (held as a
    Tensor there), lowered onto the engine's hash tables, against the same cell run primitive by primitive."""
    import _ms_models
    from mindspore import context
    from mindrec_amd.lowering import LoweredStep
    V, D, F, B, c = 3000, 8, 9, 64, 0.03
    orig = _ms_models.HashEmbeddingLookup

    def lookup(embedding_size, **kw):                     # the deep table (built first, so the seeds stay consecutive) gets max_norm
        if embedding_size == D:
            kw["max_norm"] = c
        return orig(embedding_size=embedding_size, **kw)
    monkeypatch.setattr(_ms_models, "HashEmbeddingLookup", lookup)

    def cell():
        ms_hip.set_seed(1000)
        net = _ms_models.WideDeep(V, D, F, B, [32, 16], True, True, capacity=4096)
        step = _ms_models.WideDeepTrainStep(_ms_models.WideDeepLoss(net, 8e-5, False), lazy=True)
        step.set_train()
        return step, net

    rng = np.random.default_rng(10)
    batches = [(rng.integers(0, V, size=(B, F)).astype(np.int32), rng.random((B, F)).astype(np.float32),
                (rng.random((B, 1)) < 0.3).astype(np.float32)) for _ in range(8)]
    step_g, net_g = cell()
    step_p, net_p = cell()
    assert net_g.deep_table.max_norm is not None and np.array_equal(net_g.layer0.weight.asnumpy(), net_p.layer0.weight.asnumpy())
    model = ms_hip.Model(step_g)
    lg = []
    for ids, wts, label in batches:
        lw, ld = model._run_step(step_g, tuple(ms_hip.Tensor(t) for t in (ids, wts, label)))
        lg.append((float(lw.asnumpy()), float(ld.asnumpy())))
    low = step_g.__dict__.get("_lowered")
    assert isinstance(low, LoweredStep) and low.kind == "wide_deep" and low.engine.index is not None, step_g.__dict__.get("_lowering_refused")
    assert low.engine.cfg.max_norm == pytest.approx(c)
    context.set_context(mode=context.PYNATIVE_MODE)
    lp = []
    for ids, wts, label in batches:
        lw, ld = step_p(ms_hip.Tensor(ids), ms_hip.Tensor(wts), ms_hip.Tensor(label))
        lp.append((float(lw.asnumpy()), float(ld.asnumpy())))
    assert np.allclose(np.array(lg), np.array(lp), rtol=2e-6, atol=0), (lg, lp)
    kg, vg = (t.asnumpy() for t in net_g.deep_table.embedding_table.get_data())
    kp, vp = (t.asnumpy() for t in net_p.deep_table.embedding_table.get_data())
    og, op = np.argsort(kg), np.argsort(kp)
    assert np.array_equal(kg[og], kp[op])
    assert row_rel(vg[og], vp[op]) <= 1e-5
    n1 = np.linalg.norm(vp.astype(np.float64), axis=1)
    assert (n1 > c).sum() > 50 and (n1 <= c).sum() > 50           # both branches of the clip were taken


@pytest.mark.parametrize("which", ["wide", "dcn"])
def test_lowering_refuses_max_norm_it_cannot_run(ms_hip, which):
    import _ms_models
    from mindspore import nn
    if which == "wide":
        step, _ = _clip_cell(ms_hip, wide_max_norm=0.05)
    else:
        ms_hip.set_seed(1000)
        net = _ms_models.DeepCross(3000, 8, 9, 64, [32, 16], 2)
        net.lookup = nn.EmbeddingLookup(3000, 8, target="DEVICE", sparse=False, max_norm=0.05)
        step = _ms_models.AdamTrainStep(_ms_models.LogLoss(net))
        step.set_train()
    rng = np.random.default_rng(9)
    batch = (rng.integers(0, 3000, size=(64, 9)).astype(np.int32), rng.random((64, 9)).astype(np.float32),
             (rng.random((64, 1)) < 0.3).astype(np.float32))
    model = ms_hip.Model(step)
    model._run_step(step, tuple(ms_hip.Tensor(t) for t in batch))
    assert not step.__dict__.get("_lowered")
    assert "max_norm" in (step.__dict__.get("_lowering_refused") or ""), step.__dict__.get("_lowering_refused")
